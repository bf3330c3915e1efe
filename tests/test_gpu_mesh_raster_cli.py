"""The layers above the mesh rasteriser on the device: mesh.MeshSet, synth.SyntheticTargets(mesh_set=...),
RenderNet_Shader.py --train --synthetic --synthetic-meshes DIR --synthetic-mesh-targets and RenderNet_demo.py --reference_mesh.
-m gpu."""
import json
import os
import shutil
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _write_convex_obj(path, verts, faces):
    """A convex polyhedron as OBJ, every face wound so that its normal points away from the centroid."""
    verts = np.asarray(verts, np.float64)
    centre = verts.mean(0)
    with open(path, "w") as f:
        f.write("".join("v %.9g %.9g %.9g\n" % tuple(p) for p in verts))
        for face in faces:
            p = verts[list(face)]
            if np.dot(np.cross(p[1] - p[0], p[2] - p[1]), p.mean(0) - centre) < 0:
                face = face[::-1]
            f.write("f " + " ".join("%d" % (i + 1) for i in face) + "\n")


def write_box(path, scale=(1.0, 2.0, 1.5)):
    verts = [[(i >> a) & 1 for a in range(3)] for i in range(8)]
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    _write_convex_obj(path, np.asarray(verts, np.float64) * np.asarray(scale), quads)


def write_icosphere(path, levels=2):
    t = (1.0 + 5.0 ** 0.5) / 2.0
    verts = [(-1, t, 0), (1, t, 0), (-1, -t, 0), (1, -t, 0), (0, -1, t), (0, 1, t), (0, -1, -t), (0, 1, -t), (t, 0, -1), (t, 0, 1),
             (-t, 0, -1), (-t, 0, 1)]
    faces = [(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6), (7, 1, 8),
             (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7), (9, 8, 1)]
    verts = [np.asarray(v, np.float64) / np.linalg.norm(v) for v in verts]
    for _ in range(levels):
        mid, out = {}, []

        def middle(a, b):
            key = (min(a, b), max(a, b))
            if key not in mid:
                m = verts[a] + verts[b]
                verts.append(m / np.linalg.norm(m))
                mid[key] = len(verts) - 1
            return mid[key]
        for a, b, c in faces:
            ab, bc, ca = middle(a, b), middle(b, c), middle(c, a)
            out += [(a, ab, ca), (b, bc, ab), (c, ca, bc), (ab, bc, ca)]
        faces = out
    _write_convex_obj(path, verts, faces)


@pytest.fixture(scope="module")
def folder(tmp_path_factory):
    d = tmp_path_factory.mktemp("meshes")
    write_box(str(d / "box.obj"))
    write_icosphere(str(d / "ico.obj"))
    return d


def _overlay(raster_u8, cast_u8):
    """(share of pixels whose hit / miss state agrees, median byte difference where both hit)."""
    a, b = raster_u8.cpu().numpy(), cast_u8.cpu().numpy()
    ha, hb = a.any(-1), b.any(-1)
    both = ha & hb
    return float((ha == hb).mean()), float(np.median(np.abs(a[both].astype(np.int64) - b[both].astype(np.int64))))


@pytest.mark.parametrize("axes", ["x,y,z", "z,y,x"])
def test_mesh_set_overlays_the_ray_cast_grid(folder, axes):
    """The rasterised meshes lie over the caster's picture of their voxelisation and, being wound outwards (also under axes that
    mirror the mesh), show the same side of the surface.  The box with face normals: away from its edges the caster's stencil sees
    a plane, so on most pixels the two normals are the same axis and the bytes differ by rounding at most (median <= 1).  The
    icosphere with interpolated normals against the caster's +-2 voxel stencil on a radius of 31 voxels: the stencil's normal is
    quantised to steps of about 1 / 25 of its length per component, a few bytes, and a picture of the far side would differ by
    well over 100 in the third byte; median <= 40."""
    import torch
    from rendernet_amd import mesh, ops
    files = [str(folder / "box.obj"), str(folder / "ico.obj")]
    ms = mesh.MeshSet.from_files(files, S=64, axes=axes)
    assert len(ms) == 2 and ms.names == ["box", "ico"] and ms.tri_offsets.tolist() == [0, 12, 12 + 320]
    assert ms.vertex_normals.dtype is torch.int64 and tuple(ms.vertex_normals.shape) == tuple(ms.q.shape)
    pose = torch.tensor([[4.36, 0.52, 1.0], [0.3, 1.2, 0.9], [2.0, 2.6, 0.8], [1.0, 1.0, 1.1]], device="cuda")
    ids = [0, 1, 1, 0]
    frames = ms.rasterize(ids, pose)
    assert frames.dtype is torch.uint8 and tuple(frames.shape) == (4, 512, 512, 3)
    vox = torch.cat([mesh.voxelize(files[i], S=64, axes=axes) for i in ids])
    cast = ops.raycast_normals(vox, pose)
    flat_back = ms.rasterize(ids, pose, smooth=False)
    for b in range(4):
        agree, diff = _overlay((flat_back if ids[b] == 0 else frames)[b], cast[b])
        assert agree > 0.95 and diff <= (1 if ids[b] == 0 else 40), (b, agree, diff)
    flat = ms.rasterize(ids, pose, smooth=False, cull="none")
    assert bool((flat.any(-1) == frames.any(-1)).all())          # closed meshes: the same silhouette


def _models(folder):
    import RenderNet_Shader
    from rendernet_amd import synth
    chair, names = synth.read_models(os.path.join(ROOT, "binvox"))
    keep = names.index("chair")
    grids, mesh_names, ms = RenderNet_Shader.read_meshes(str(folder), "cuda", with_set=True)
    return np.concatenate([chair[keep:keep + 1], grids]), ["chair"] + list(mesh_names), ms


def test_feed_targets_are_the_rasterised_meshes(folder, capsys):
    import torch
    from rendernet_amd import mesh, ops, synth
    models, names, ms = _models(folder)
    assert names == ["chair", "box", "ico"]
    kw = dict(batch_size=6, steps=3, seed=[7, 0])
    plain = list(synth.SyntheticTargets(models, names, **kw))
    with_meshes = list(synth.SyntheticTargets(models, names, mesh_set=ms, mesh_models=[-1, 0, 1], **kw))
    single = {n: mesh.MeshSet.from_files([str(folder / (n + ".obj"))], S=64) for n in ("box", "ico")}
    kinds = set()
    for (f0, v0, p0, n0), (f1, v1, p1, n1) in zip(plain, with_meshes):
        assert n0 == n1 and torch.equal(v0, v1) and torch.equal(p0, p1)
        assert f1.dtype is torch.uint8 and f1.shape == f0.shape
        for b, name in enumerate(n1):
            model = name.split("_p")[0]
            kinds.add(model)
            if model == "chair":
                assert torch.equal(f1[b], f0[b])
            else:
                s = single[model]
                want = ops.rasterize_mesh(s.q, s.tris, p1[b:b + 1], 64)
                assert torch.equal(f1[b:b + 1], want)
                agree, _ = _overlay(f1[b], f0[b])
                assert agree > 0.95, (name, agree)
    assert kinds == {"chair", "box", "ico"}
    # "phong" shades the rasterised map as it shades the caster's
    grey = next(iter(synth.SyntheticTargets(models, names, greyscale=True, mesh_set=ms, mesh_models=[-1, 0, 1], **kw)))
    assert grey[0].dtype is torch.float32 and torch.equal(grey[0], synth.shade(with_meshes[0][0]).mean(dim=3, keepdim=True))
    for bad in (dict(mesh_set=ms), dict(mesh_set=ms, mesh_models=[-1, 0]), dict(mesh_set=ms, mesh_models=[-1, 0, 2]),
                dict(mesh_set=ms, mesh_models=[-1, 0, 1], shader="ao"), dict(mesh_set=ms, mesh_models=[-1, 0, 1], mesh_cull="front")):
        with pytest.raises(ValueError):
            synth.SyntheticTargets(models, names, **dict(kw, **bad))


def test_shader_script_trains_on_mesh_targets(folder, tmp_path, capsys, monkeypatch):
    import RenderNet_Shader
    from rendernet_amd import synth
    models = tmp_path / "models"
    models.mkdir()
    shutil.copy(os.path.join(ROOT, "binvox", "chair.binvox"), models / "chair.binvox")
    cfg = {"model_path": str(models), "is_greyscale": "True", "gpu": 0, "batch_size": 2, "max_epochs": 1, "batches_chunk": 1,
           "threshold": 0.1, "e_eta": 1e-5, "keep_prob": 1.0, "decay_steps": 100000, "trained_model_name": "3d2d_renderer",
           "sample_save": str(tmp_path / "out"), "checkpoint_secs": 7200}
    cfgp = str(tmp_path / "config.json")
    json.dump(cfg, open(cfgp, "w"))
    drawn = []
    plain = synth._raster

    def recording(mesh_set, mesh_ids, poses, new_size, pixels_per_cell, cull):
        drawn.append((list(np.asarray(mesh_ids)), cull))
        return plain(mesh_set, mesh_ids, poses, new_size, pixels_per_cell, cull)
    monkeypatch.setattr(synth, "_raster", recording)
    base = [cfgp, "--train", "--synthetic", "--synthetic-steps", "3", "--max-steps", "3", "--synthetic-meshes", str(folder)]
    RenderNet_Shader.main(base + ["--synthetic-mesh-targets", "--mesh_cull", "none"])
    out = capsys.readouterr().out
    steps = [l for l in out.splitlines() if l.startswith("Step")]
    assert len(steps) == 3 and all(np.isfinite(float(l.split("Loss")[1])) for l in steps)
    assert drawn and all(c == "none" for _, c in drawn) and all(set(i) <= {0, 1} for i, _ in drawn)
    # misuse, each with its message, before anything is trained
    for extra, what in ((["--synthetic-mesh-targets", "--synthetic-shader", "ao"], "needs voxel hits"),
                        (["--synthetic-mesh-targets", "--mesh_cull", "front"], "expected back or none"),
                        (["--mesh_cull", "none"], "needs --synthetic-mesh-targets")):
        with pytest.raises(SystemExit, match=what):
            RenderNet_Shader.main(base + extra)
    with pytest.raises(SystemExit, match="needs --synthetic-meshes"):
        RenderNet_Shader.main([cfgp, "--train", "--synthetic", "--synthetic-mesh-targets"])
    json.dump(dict(cfg, synthetic_mesh_targets="maybe"), open(cfgp, "w"))
    with pytest.raises(SystemExit, match="neither true nor false"):
        RenderNet_Shader.main(base)


def test_demo_writes_the_mesh_pictures(folder, tmp_path):
    from PIL import Image
    out = tmp_path / "render"
    r = subprocess.run([sys.executable, os.path.join(ROOT, "RenderNet_demo.py"), "--mesh_path", str(folder / "ico.obj"), "--render_dir",
                        str(out), "--reference_render", "True", "--reference_mesh", "True", "--mesh_flat", "True"],
                       cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    stem = "000_ico_pose_250.000000_60.000000_3.300000_light_250.000000_60.000000"
    assert sorted(os.listdir(out)) == [stem + ".png", stem + "_reference_mesh_normal.png", stem + "_reference_mesh_phong.png",
                                       stem + "_reference_normal.png", stem + "_reference_phong.png"]
    mesh_hit = np.asarray(Image.open(out / (stem + "_reference_mesh_normal.png"))).any(-1)
    grid_hit = np.asarray(Image.open(out / (stem + "_reference_normal.png"))).any(-1)
    assert mesh_hit.shape == (512, 512) and 0.02 < mesh_hit.mean() < 0.6 and (mesh_hit == grid_hit).mean() > 0.95
    assert np.asarray(Image.open(out / (stem + "_reference_mesh_phong.png"))).shape == (512, 512, 3)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "RenderNet_demo.py"), "--reference_mesh", "True"], cwd=ROOT,
                       capture_output=True, text=True, timeout=600)
    assert r.returncode != 0 and "give one" in r.stderr
