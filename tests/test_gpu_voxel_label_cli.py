"""The command line and the script on top of rn_voxel_label: `python -m rendernet_amd.tools.clean_voxels` on a grid and on a
mesh, and the reconstruction script's "clean_shape" key; every number against the NumPy twin (tests/voxel_label_ref.py).
-m gpu."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import voxel_label_ref as R

pytestmark = pytest.mark.gpu
ROOT = R.ROOT


def _read_binvox(path):
    from rendernet_amd.tools import binvox_rw
    with open(path, "rb") as fh:
        return np.ascontiguousarray(binvox_rw.read_as_3d_array(fh).data).astype(bool)


def _dirty_chair():
    chair = R.load_binvox("chair")
    dirty = chair.copy()
    dirty[3, 3, 3] = dirty[60, 60, 60] = dirty[2, 60, 2:4] = True
    return chair, dirty


def test_clean_voxels_on_a_binvox_file(tmp_path):
    from rendernet_amd.tools import binvox_rw
    chair, dirty = _dirty_chair()
    src, dst = str(tmp_path / "dirty.binvox"), str(tmp_path / "clean.binvox")
    binvox_rw.save_binvox(dirty, src)
    r = subprocess.run([sys.executable, "-m", "rendernet_amd.tools.clean_voxels", src, dst], cwd=ROOT, capture_output=True, text=True,
                       timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    row = json.loads(r.stdout.strip().splitlines()[-1])
    assert row["input"] == src and row["output"] == dst and row["size"] == 64
    assert row["before"]["words"] == R.topology(dirty).tolist() and row["after"]["words"] == R.topology(chair).tolist()
    assert row["before"]["components"] == 4 and row["after"]["components"] == 1 and row["after"]["handles"] == 1
    assert row["dropped"] == R.clean(dirty)[1] and sorted(row["dropped"]) == [1, 1, 2]
    assert np.array_equal(_read_binvox(dst), chair)


def test_clean_voxels_on_a_mesh_an_npz_and_its_options(tmp_path, capsys):
    from rendernet_amd import mesh
    from rendernet_amd.tools import clean_voxels
    chair, dirty = _dirty_chair()
    ply, out = str(tmp_path / "chair.ply"), str(tmp_path / "clean.ply")
    mesh.save_mesh(ply, *mesh.extract(chair.astype(np.uint8)))
    row = clean_voxels.main([ply, out, "--size", "64"])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == row
    grid = mesh.voxelize(ply, S=64, mode="both").cpu().numpy()[0, ..., 0].astype(bool)
    cleaned = R.clean(grid)[0]
    assert row["before"]["words"] == R.topology(grid).tolist() and row["after"]["words"] == R.topology(cleaned).tolist()
    back = mesh.voxelize(out, S=64, mode="solid")
    assert back.sum() > 1000 and os.path.getsize(out) > 1000
    # a soft volume at its own threshold, every option, a mesh out
    soft = np.where(dirty, np.float32(0.3), np.float32(0.02))
    np.savez(str(tmp_path / "soft_Param.txt"), soft)
    dst = str(tmp_path / "kept.binvox")
    row = clean_voxels.main([str(tmp_path / "soft_Param.txt.npz"), dst, "--threshold", "0.1", "--keep", "0", "--min-voxels", "2", "--no-fill",
                             "--connectivity", "6"])
    capsys.readouterr()
    want, dropped = R.clean(dirty, keep_largest=0, min_voxels=2, fill_cavities=False, connectivity=6)
    assert np.array_equal(_read_binvox(dst), want) and row["dropped"] == dropped == [1, 1]
    assert row["after"]["words"] == R.topology(want).tolist()
    with pytest.raises(SystemExit) as e:
        clean_voxels.main([str(tmp_path / "soft_Param.txt.npz"), str(tmp_path / "out.stl")])
    assert "clean_voxels" in str(e.value) and ".binvox, .obj or .ply" in str(e.value)


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


def test_reconstruct_script_cleans_its_hypotheses(tmp_path, capsys):
    out = _reconstruct(tmp_path, {"clean_shape": True, "clean_min_voxels": 2, "save_mesh": True,
                                  "target_shape": os.path.join(ROOT, "binvox", "chair.binvox")})
    log = capsys.readouterr().out
    with open(os.path.join(out, "topology.json")) as fh:
        rows = json.load(fh)
    raw = sorted(f for f in os.listdir(out) if f.endswith(".binvox") and not f.endswith("_clean.binvox"))
    assert len(raw) == 5 and sorted(rows) == [f[:-7] for f in raw]
    for f in raw:
        name = f[:-7]
        grid = _read_binvox(os.path.join(out, f))
        w = R.topology(grid)
        assert rows[name]["words"] == w.tolist()
        assert "%s Topology components %d cavities %d handles %d" % (name, w[1], w[2], w[7]) in log
        assert np.array_equal(_read_binvox(os.path.join(out, name + "_clean.binvox")), R.clean(grid, min_voxels=2)[0])
        assert os.path.isfile(os.path.join(out, name + "_clean.ply")) and os.path.isfile(os.path.join(out, name + ".ply"))
        assert (name + " Shape(clean) IoU ") in log and (name + " Shape IoU ") in log
    assert log.count(" Topology components ") == 5 and log.count(" Shape(clean) IoU ") == 5 and log.count(" Shape IoU ") == 5


def test_reconstruct_script_without_the_key_writes_none_of_it(tmp_path, capsys):
    out = _reconstruct(tmp_path, {"save_mesh": True})
    log = capsys.readouterr().out
    assert "Topology" not in log and "Shape(clean)" not in log
    files = os.listdir(out)
    assert "topology.json" not in files and not any("_clean" in f for f in files) and sum(f.endswith(".binvox") for f in files) == 5
