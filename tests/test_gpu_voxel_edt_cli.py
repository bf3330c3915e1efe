"""The command line and the script on top of rn_voxel_shape_metrics: `python -m rendernet_amd.tools.compare_voxels` on grids and
on a mesh, and the reconstruction script's "target_shape" key; every number against the NumPy twin (tests/voxel_edt_ref.py).
-m gpu."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import voxel_edt_ref as R

pytestmark = pytest.mark.gpu
ROOT = R.ROOT
NAMES = ("iou", "dice", "chamfer", "chamfer_sq", "hausdorff", "precision", "recall", "fscore")


def _matches(row, a, b, tau2):
    want = R.shape_words(a, b, tau2)
    assert row["words"] == want.tolist() and row["tau2"] == tau2
    d = R.derived(want)
    for name in NAMES:
        assert row[name] == d[name] or (row[name] != row[name] and d[name] != d[name]), (name, row[name], d[name])


def test_compare_voxels_on_two_binvox_files():
    chair, teapot = os.path.join(ROOT, "binvox", "chair.binvox"), os.path.join(ROOT, "binvox", "teapot.binvox")
    r = subprocess.run([sys.executable, "-m", "rendernet_amd.tools.compare_voxels", chair, teapot, "--tau", "2.5"], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    row = json.loads(r.stdout.strip().splitlines()[-1])
    assert row["size"] == 64 and row["a"] == chair and row["b"] == teapot and row["tau"] == 2.5
    _matches(row, R.load_binvox("chair"), R.load_binvox("teapot"), 6)


def test_compare_voxels_with_a_mesh_an_npz_and_unequal_sizes(tmp_path, capsys):
    from rendernet_amd import mesh
    from rendernet_amd.tools import compare_voxels
    chair = R.load_binvox("chair")
    teapot_path = os.path.join(ROOT, "binvox", "teapot.binvox")
    ply = str(tmp_path / "chair.ply")
    mesh.save_mesh(ply, *mesh.extract(chair.astype(np.uint8)))
    row = compare_voxels.main([ply, teapot_path])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1])["words"] == row["words"]
    grid = mesh.voxelize(ply, S=64, mode="both").cpu().numpy()[0, ..., 0].astype(bool)
    assert grid.sum() > 1000
    _matches(row, grid, R.load_binvox("teapot"), 1)
    # a soft volume at its own threshold against the binvox at 0.5
    soft = np.where(chair, np.float32(0.3), np.float32(0.02))
    np.savez(str(tmp_path / "soft_Param.txt"), soft)
    row = compare_voxels.main([str(tmp_path / "soft_Param.txt.npz"), teapot_path, "--threshold", "0.1,0.5"])
    capsys.readouterr()
    _matches(row, chair, R.load_binvox("teapot"), 1)
    # two meshes take --size; unequal grids are refused with a message
    row = compare_voxels.main([ply, ply, "--size", "32"])
    capsys.readouterr()
    assert row["size"] == 32 and row["iou"] == 1.0 and row["hausdorff"] == 0.0
    np.savez(str(tmp_path / "small"), soft[::2, ::2, ::2])
    with pytest.raises(SystemExit) as e:
        compare_voxels.main([str(tmp_path / "small.npz"), teapot_path])
    assert "unequal size" in str(e.value)


def _reconstruct(tmp_path, extra):
    from PIL import Image
    import Reconstruct_RenderNet_Face
    rng = np.random.default_rng(0)
    for name in ("albedo.png", "normal.png"):
        Image.fromarray((rng.random((512, 512, 3)) * 255).astype(np.uint8)).save(str(tmp_path / name))
    cfg = {"target_albedo": str(tmp_path / "albedo.png"), "target_normal": str(tmp_path / "normal.png"),
           "target_azimuth_light": 294, "target_elevation_light": 105, "weight_dir": str(tmp_path / "nope"),
           "weight_dir_decoder": str(tmp_path / "nope2"), "gpu": 0, "batch_size": 5, "z_dim": 200, "inner_step": 1,
           "max_epochs": 1, "threshold": 0.1, "shape_eta": 0.8, "pose_eta": 0.01, "tex_eta": 0.8, "light_eta": 0.4,
           "sample_save": str(tmp_path / "out")}
    cfg.update(extra)
    cfgp = str(tmp_path / "config.json")
    with open(cfgp, "w") as fh:
        json.dump(cfg, fh)
    Reconstruct_RenderNet_Face.main([cfgp, "--max-steps", "1"])
    return cfg["sample_save"]


def test_reconstruct_script_scores_its_hypotheses_against_a_target_shape(tmp_path, capsys):
    from rendernet_amd.tools import binvox_rw
    out = _reconstruct(tmp_path, {"target_shape": os.path.join(ROOT, "binvox", "chair.binvox"), "shape_tau": 2.5})
    log = capsys.readouterr().out
    with open(os.path.join(out, "shape_metrics.json")) as fh:
        scores = json.load(fh)
    files = sorted(f for f in os.listdir(out) if f.endswith(".binvox"))
    assert len(files) == 5 and sorted(scores) == [f[:-7] for f in files]
    chair = R.load_binvox("chair")
    for f in files:
        with open(os.path.join(out, f), "rb") as fh:
            grid = np.ascontiguousarray(binvox_rw.read_as_3d_array(fh).data).astype(bool)
        _matches(scores[f[:-7]], grid, chair, 6)
        assert (f[:-7] + " Shape IoU ") in log
    assert log.count(" Shape IoU ") == 5 and " chamfer " in log and " hausdorff " in log and " F " in log
    small = str(tmp_path / "small.npz")
    np.savez(small, np.zeros((32, 32, 32), np.float32))
    with pytest.raises(SystemExit) as e:
        _reconstruct(tmp_path, {"target_shape": small})
    assert "target_shape" in str(e.value) and "64^3" in str(e.value)


def test_reconstruct_script_without_the_key_writes_no_scores(tmp_path, capsys):
    out = _reconstruct(tmp_path, {})
    assert "Shape IoU" not in capsys.readouterr().out
    assert "shape_metrics.json" not in os.listdir(out) and any(f.endswith(".binvox") for f in os.listdir(out))


def test_shape_metrics_log_line():
    import torch
    from rendernet_amd import metrics
    chair, teapot = R.load_binvox("chair"), R.load_binvox("teapot")
    log = metrics.ShapeMetricsLog(tau=1.0)
    pred = torch.as_tensor(np.stack([chair, teapot]).astype(np.uint8)).cuda()
    rows = log.add(pred, np.stack([teapot, teapot]).astype(np.uint8))
    log.add(pred[:1], torch.zeros((1, 64, 64, 64), dtype=torch.uint8, device="cuda"))      # NaN distances: left out of their means
    d = [R.derived(R.shape_words(chair, teapot)), R.derived(R.shape_words(teapot, teapot))]
    assert [rows[0][n] for n in NAMES] == [d[0][n] for n in NAMES] and len(log.rows) == 3
    want = {"iou": np.mean([d[0]["iou"], 1.0, 0.0])}
    for n in ("chamfer", "hausdorff", "fscore"):
        want[n] = np.mean([d[0][n], d[1][n]])
    assert log.means() == {k: float(v) for k, v in want.items()}
    assert log.line() == "Shape IoU %r chamfer %r hausdorff %r F %r" % tuple(float(want[k]) for k in ("iou", "chamfer", "hausdorff", "fscore"))
