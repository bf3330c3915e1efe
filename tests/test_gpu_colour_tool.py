"""python -m rendernet_amd.tools.colour_voxels on the device: the self-check returns the chair's colour field exactly and writes a
coloured .ply, and a folder of pose-named PNGs gives the vertex colours of the direct `ops` path.  -m gpu."""
import json
import os

import numpy as np
import pytest

from conftest import BINVOX_DIR

pytestmark = pytest.mark.gpu

CHAIR = os.path.join(BINVOX_DIR, "chair.binvox")


def test_self_check_is_exact_and_writes_colours(tmp_path, capsys):
    from rendernet_amd import mesh
    from rendernet_amd.tools import colour_voxels as CT
    out = str(tmp_path / "chair.ply")
    row = CT.main(["--from-voxels", CHAIR, "--views", "6", "--size", "32", out])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == row
    assert row["exact"] is True and row["views"] == 6 and row["size"] == 64          # a grid file keeps its own side
    assert row["seen"] > 1000 and row["filled"] == 0 and 0 < row["unseen"] < row["surface"]
    verts, tris = mesh.load_mesh(out)
    cols = mesh.load_mesh_colours(out)
    assert cols is not None and cols.dtype == np.uint8 and cols.shape == (len(verts), 3) == (row["vertices"], 3)
    assert len(tris) == 2 * row["faces"] and len(np.unique(cols, axis=0)) > 100
    # the fill leaves fewer surface voxels without a colour, and the .obj carries the same colours
    obj = str(tmp_path / "chair.obj")
    filled = CT.main(["--from-voxels", CHAIR, "--views", "6", "--fill", "4", obj])
    assert filled["exact"] is True and filled["filled"] > 0 and filled["unseen"] < row["unseen"] and filled["seen"] == row["seen"]
    assert mesh.load_mesh_colours(obj).shape == cols.shape


def test_pictures_give_the_colours_of_the_direct_path(tmp_path, capsys):
    import torch
    from PIL import Image
    from oracle.io_phong import read_binvox
    from rendernet_amd import mesh, ops, synth
    from rendernet_amd.tools import colour_voxels as CT
    occ = read_binvox(CHAIR).astype(bool)
    vox = torch.from_numpy(occ.astype(np.uint8))[None, ..., None].cuda()
    shots = tmp_path / "shots"
    shots.mkdir()
    names = ["chair_p%.2f_t%.2f_r3.3.png" % (az, el) for az, el in ((10.0, 70.0), (100.0, 40.0), (190.0, 85.0), (280.0, 55.0),
                                                                      (55.0, 20.0), (325.0, 60.0))]
    poses = torch.from_numpy(np.stack([CT.pose_of_name(n) for n in names])).cuda()
    cm = synth.ColourModel(5, 8)
    code_q = torch.from_numpy(np.repeat(cm.quantise(np.random.default_rng(5).standard_normal((1, 8))), 6, 0)).cuda()
    six = vox.expand(6, -1, -1, -1, -1).contiguous()
    rgb, _ = ops.raycast_albedo(six, poses, torch.from_numpy(cm.waves).cuda(), code_q, cm.base, new_size=128, pixels_per_cell=2,
                                smooth=2)
    for n, frame in zip(names, rgb.cpu().numpy()):
        Image.fromarray(frame).save(str(shots / n))
    out, npz = str(tmp_path / "chair.ply"), str(tmp_path / "colours.npz")
    row = CT.main([CHAIR, str(shots), out, "--threshold", "0", "--fill", "2", "--save-colours", npz])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == row
    assert row["views"] == 6 and row["size"] == 64 and row["seen"] > 1000 and row["filled"] > 0 and "exact" not in row
    # the same through ops, in the sorted order the tool reads the folder in
    images, masks, read_poses, f, read_names = CT.read_pictures(str(shots), 64, "black", 0.0)
    assert f == 2 and read_names == sorted(names)
    order = [names.index(n) for n in read_names]
    assert np.array_equal(images, rgb.cpu().numpy()[order])
    _, hits = ops.voxel_scan(vox, torch.from_numpy(read_poses).cuda()[None], new_size=128, pixels_per_cell=2, return_hits=True)
    sums = ops.voxel_colour_sums(torch.from_numpy(images).cuda()[None], hits, 64, torch.from_numpy(masks).cuda()[None])
    col, known = ops.voxel_colours(sums, vox, fill=2)
    m = ops.extract_mesh(vox)
    want = ops.mesh_vertex_colours(m, col, known).cpu().numpy()
    assert np.array_equal(mesh.load_mesh_colours(out), want) and len(want) == row["vertices"]
    with np.load(npz) as z:
        assert np.array_equal(z["colours"], col[0].cpu().numpy()) and np.array_equal(z["known"], known[0].cpu().numpy())
    assert row["seen"] == int((known == 1).sum()) and row["filled"] == int((known == 2).sum())
