"""The user surface of the mesh voxeliser on the device: RenderNet_demo.py --mesh_path, the mesh_to_binvox tool and
RenderNet_Shader.py --train --synthetic --synthetic-meshes.  -m gpu."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

import mesh_voxel_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write_obj(path, scale=(1.0, 2.0, 1.5)):
    """A box with extents `scale` as an OBJ of six quads."""
    q, _ = R.cube(0, 1)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    with open(path, "w") as f:
        f.write("# a box\n" + "".join("v %g %g %g\n" % tuple(p * scale) for p in q.astype(float)))
        f.write("".join("f %d %d %d %d\n" % tuple(i + 1 for i in quad) for quad in quads))


def _child(args):
    return subprocess.run([sys.executable] + args, cwd=ROOT, capture_output=True, text=True, timeout=600)


def test_demo_renders_a_mesh_and_saves_its_grid(tmp_path):
    from PIL import Image
    from rendernet_amd import mesh
    from rendernet_amd.tools import binvox_rw
    obj, out, path = str(tmp_path / "box.obj"), tmp_path / "render", str(tmp_path / "box.binvox")
    _write_obj(obj)
    r = _child([os.path.join(ROOT, "RenderNet_demo.py"), "--mesh_path", obj, "--save_binvox", path, "--render_dir", str(out),
                "--reference_render", "True"])
    assert r.returncode == 0, r.stderr[-2000:]
    stem = "000_box_pose_250.000000_60.000000_3.300000_light_250.000000_60.000000"
    assert sorted(os.listdir(out)) == [stem + ".png", stem + "_reference_normal.png", stem + "_reference_phong.png"]
    assert np.asarray(Image.open(out / (stem + ".png"))).shape == (512, 512, 3)
    hit = np.asarray(Image.open(out / (stem + "_reference_normal.png"))).any(-1)
    assert 0.02 < hit.mean() < 0.6                                             # the ray caster sees the mesh's grid
    with open(path, "rb") as f:
        back = binvox_rw.read_as_3d_array(f)
    grid = mesh.voxelize(obj).cpu().numpy()
    assert grid.shape == (1, 64, 64, 64, 1) and back.dims == [64, 64, 64]
    assert np.array_equal(back.data, grid[0, ..., 0].astype(bool))
    # extents 1 : 2 : 1.5 on array axes 0, 1, 2 and margin 1: the box is [16.5, 47.5] x [1, 63] x [8.75, 55.25] in voxels.  The
    # surface rule is closed against closed, so the faces lying exactly on the cell boundaries 1 and 63 also set layers 0 and 63.
    want = np.zeros((64, 64, 64), bool)
    want[16:48, :, 8:56] = True
    assert np.array_equal(back.data, want)
    # the tool writes the same file's grid, with its own options
    tool = str(tmp_path / "tool.binvox")
    r = _child(["-m", "rendernet_amd.tools.mesh_to_binvox", obj, tool, "--size", "32", "--mode", "surface", "--axes", "y,x,z"])
    assert r.returncode == 0 and tool in r.stdout, r.stderr[-2000:]
    with open(tool, "rb") as f:
        back = binvox_rw.read_as_3d_array(f)
    q, t = mesh.load_mesh(obj)
    q = mesh.fit(q, 32, 1, "y,x,z")
    assert np.array_equal(back.data, R.surface(q, t, 32)) and back.data.any() and not back.data[8:24, 12:20, 10:22].any()
    # flags that contradict each other, before the net is built
    r = _child([os.path.join(ROOT, "RenderNet_demo.py"), "--mesh_path", obj, "--voxel_shape", "1a2b3c4d"])
    assert r.returncode != 0 and "give one" in r.stderr


def test_shader_script_trains_on_a_mesh_folder(tmp_path, capsys, monkeypatch):
    """Three steps at the first epochs' crop of 32: the mesh's name is among the drawn samples and its grid is what the feed holds."""
    import torch
    import RenderNet_Shader
    from rendernet_amd import mesh, synth
    models, meshes = tmp_path / "models", tmp_path / "meshes"
    models.mkdir()
    (meshes / "sub").mkdir(parents=True)
    shutil.copy(os.path.join(ROOT, "binvox", "chair.binvox"), models / "chair.binvox")
    _write_obj(str(meshes / "sub" / "box.obj"))
    cfg = {"model_path": str(models), "is_greyscale": "True", "gpu": 0, "batch_size": 2, "max_epochs": 1, "batches_chunk": 1,
           "threshold": 0.1, "e_eta": 1e-5, "keep_prob": 1.0, "decay_steps": 100000, "trained_model_name": "3d2d_renderer",
           "sample_save": str(tmp_path / "out"), "checkpoint_secs": 7200}
    cfgp = str(tmp_path / "config.json")
    json.dump(cfg, open(cfgp, "w"))
    seen, feeds = [], []
    plain_next = synth.SyntheticTargets.__next__

    def recording_next(self):
        batch = plain_next(self)
        seen.extend(batch[3])
        feeds.append(self)
        return batch
    monkeypatch.setattr(synth.SyntheticTargets, "__next__", recording_next)
    RenderNet_Shader.main([cfgp, "--train", "--synthetic", "--synthetic-steps", "3", "--max-steps", "3", "--synthetic-meshes", str(meshes)])
    out = capsys.readouterr().out
    steps = [l for l in out.splitlines() if l.startswith("Step")]
    assert len(steps) == 3 and all(np.isfinite(float(l.split("Loss")[1])) for l in steps)
    assert "synthetic meshes: box" in out
    models_drawn = sorted({n.split("_p")[0] for n in seen})
    print("drawn: %s" % seen)
    assert models_drawn == ["box", "chair"]
    feed = feeds[0]
    assert feed.names == ["chair", "box"] and tuple(feed.models.shape) == (2, 64, 64, 64, 1)
    assert torch.equal(feed.models[1:], mesh.voxelize(str(meshes / "sub" / "box.obj")))
    # a stem the pose parser cannot tell from a pose tag, a name that is taken, an empty folder, and the flag without --synthetic
    for bad, what in (("my_plane.obj", "pose tags"), ("chair.obj", "already in the set")):
        other = tmp_path / ("bad_" + bad.split(".")[0])
        other.mkdir()
        _write_obj(str(other / bad))
        with pytest.raises(SystemExit, match=what):
            RenderNet_Shader.main([cfgp, "--train", "--synthetic", "--synthetic-meshes", str(other)])
    (tmp_path / "none").mkdir()
    with pytest.raises(SystemExit, match="no .obj or .ply"):
        RenderNet_Shader.main([cfgp, "--train", "--synthetic", "--synthetic-meshes", str(tmp_path / "none")])
    with pytest.raises(SystemExit, match="needs --synthetic"):
        RenderNet_Shader.main([cfgp, "--train", "--synthetic-meshes", str(meshes)])
