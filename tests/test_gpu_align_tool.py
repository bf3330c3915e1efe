"""The command lines and the script on top of rn_voxel_align: `compare_voxels --align`, `python -m rendernet_amd.tools.align_voxels`
and the reconstruction script's "align_shape" key, against the NumPy twin (tests/voxel_align_ref.py).  -m gpu."""
import json
import os

import numpy as np
import pytest

import voxel_align_ref as R
from test_gpu_voxel_edt_cli import _matches, _reconstruct

pytestmark = pytest.mark.gpu
ROOT = R.ROOT
CHAIR = os.path.join(ROOT, "binvox", "chair.binvox")
MOVE = (13, (0, -1, 3))                   # the chair spans its grid along y: no shift on the axis y lands on


def _read(path):
    from rendernet_amd.tools import binvox_rw
    with open(path, "rb") as fh:
        return np.ascontiguousarray(binvox_rw.read_as_3d_array(fh).data).astype(bool)


@pytest.fixture
def moved_chair(tmp_path):
    """The chair moved inside its grid (no voxel leaves) as a .binvox file, and the move that undoes it."""
    from rendernet_amd.tools import binvox_rw
    chair = R.load_binvox("chair")
    moved = R.transform(chair, *MOVE)
    assert moved.sum() == chair.sum() == 5277
    path = str(tmp_path / "moved.binvox")
    binvox_rw.save_binvox(moved, path)
    o, t, n, ties = R.winner(R.scores(moved, chair, 4, 24), 4)
    assert (o, n, ties) == (18, 5277, 1) and np.array_equal(R.transform(moved, o, t), chair)
    return path, moved, o, list(t)


def test_compare_voxels_align(moved_chair, capsys):
    from rendernet_amd.tools import compare_voxels
    path, moved, o, t = moved_chair
    chair = R.load_binvox("chair")
    plain = compare_voxels.main([path, CHAIR])
    line = capsys.readouterr().out.strip().splitlines()[-1]
    _matches(plain, moved, chair, 1)
    assert list(plain) == ["words", "tau2"] + list(E_NAMES) + ["a", "b", "size", "tau"] and line == json.dumps(plain)
    row = compare_voxels.main([path, CHAIR, "--align", "4"])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == row
    assert row["align_orientation"] == o and row["align_shift"] == t
    assert row["iou_unaligned"] == plain["iou"] < 0.2 and row["iou"] == 1.0 and row["hausdorff"] == 0.0
    _matches(row, chair, chair, 1)
    assert compare_voxels.main([path, CHAIR, "--align"])["align_shift"] == t                 # R = 8 when no number follows
    kept = compare_voxels.main([path, CHAIR, "--align", "4", "--align-orientations", "none"])
    words, _ = R.align(moved, chair, 4, "none")
    assert kept["align_orientation"] == 0 and kept["align_shift"] == words[1:4].tolist() and kept["words"][2] == words[4] < 5277
    capsys.readouterr()
    with pytest.raises(SystemExit) as e:
        compare_voxels.main([path, CHAIR, "--align", "17"])
    assert "max_shift" in str(e.value)


E_NAMES = ("iou", "dice", "chamfer", "chamfer_sq", "hausdorff", "precision", "recall", "fscore")


def test_align_voxels_round_trips(moved_chair, tmp_path, capsys):
    from rendernet_amd import mesh
    from rendernet_amd.tools import align_voxels
    path, moved, o, t = moved_chair
    out = str(tmp_path / "back.binvox")
    row = align_voxels.main([path, CHAIR, out, "--max-shift", "4"])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == row
    assert row["orientation"] == o and row["shift"] == t and row["n_and"] == row["n_a"] == row["n_b"] == 5277
    assert row["iou_after"] == 1.0 and row["iou_before"] < 0.2 and row["size"] == 64
    assert np.array_equal(_read(out), R.load_binvox("chair"))
    # a soft volume at its own threshold, a mesh out
    np.savez(str(tmp_path / "soft_Param.txt"), np.where(moved, np.float32(0.3), np.float32(0.02)))
    ply = str(tmp_path / "back.ply")
    soft = align_voxels.main([str(tmp_path / "soft_Param.txt.npz"), CHAIR, ply, "--max-shift", "4", "--threshold", "0.1,0.5"])
    capsys.readouterr()
    assert (soft["orientation"], soft["shift"], soft["n_and"]) == (o, t, 5277)
    verts, faces = mesh.load_mesh(ply)[:2]
    want = mesh.extract(R.load_binvox("chair").astype(np.uint8))
    assert len(verts) == len(want[0]) > 1000 and len(faces) > 1000
    with pytest.raises(SystemExit) as e:
        align_voxels.main([path, CHAIR, str(tmp_path / "back.txt")])
    assert "align_voxels" in str(e.value)


def test_reconstruct_script_aligns_before_it_scores(tmp_path, capsys):
    out = _reconstruct(tmp_path, {"target_shape": CHAIR, "align_shape": 2})
    log = capsys.readouterr().out
    with open(os.path.join(out, "shape_metrics.json")) as fh:
        scores = json.load(fh)
    files = sorted(f for f in os.listdir(out) if f.endswith(".binvox"))
    assert len(files) == 5 and log.count(" Shape aligned o ") == 5 and log.count(" Shape IoU ") == 5
    chair = R.load_binvox("chair")
    for k, f in enumerate(files):
        row = scores[f[:-7]]
        assert set(("align_orientation", "align_shift", "aligned")) <= set(row)
        assert "%s Shape aligned o %d t %d,%d,%d IoU %r " % ((f[:-7], row["align_orientation"]) + tuple(row["align_shift"])
                                                             + (row["aligned"]["iou"],)) in log
        assert row["aligned"]["iou"] >= row["iou"]
        if k == 0:                                                                           # one hypothesis against the twin, in full
            grid = _read(os.path.join(out, f))
            words, _ = R.align(grid, chair, 2, "rotations")
            assert [row["align_orientation"]] + row["align_shift"] == words[:4].tolist()
            _matches(row["aligned"], R.transform(grid, int(words[0]), tuple(int(v) for v in words[1:4])), chair, 1)
    with pytest.raises(SystemExit) as e:
        _reconstruct(tmp_path, {"align_shape": 2})
    assert "align_shape" in str(e.value)
    with pytest.raises(SystemExit) as e:
        _reconstruct(tmp_path, {"target_shape": CHAIR, "align_shape": 17})
    assert "align_shape" in str(e.value)
