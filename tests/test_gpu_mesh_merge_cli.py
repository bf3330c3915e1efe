"""The tools' --merge flags on the device, on the chair at 64^3: binvox_to_mesh --blocky --merge writes a file that reloads,
voxelises to the grid and has the twin's face count; colour_voxels --blocky --merge stays exact and writes rectangles of one
colour; and without --merge both write the file they wrote before.  -m gpu."""
import json
import os

import numpy as np
import pytest

import mesh_merge_ref as M
from conftest import BINVOX_DIR

pytestmark = pytest.mark.gpu

CHAIR = os.path.join(BINVOX_DIR, "chair.binvox")


@pytest.fixture(scope="module")
def chair():
    from rendernet_amd.tools.binvox_to_mesh import load_grid
    return load_grid(CHAIR)


@pytest.mark.parametrize("ext", ["obj", "ply"])
def test_binvox_to_mesh_merge(tmp_path, capsys, chair, ext):
    import torch
    from rendernet_amd import mesh, ops
    from rendernet_amd.tools import binvox_to_mesh
    out, unit = str(tmp_path / ("merged." + ext)), str(tmp_path / ("unit." + ext))
    binvox_to_mesh.main([CHAIR, out, "--blocky", "--merge"])
    assert "1180 vertices, 831 quads" in capsys.readouterr().out
    q, faces = M.merge(chair)[:2]
    assert (len(faces), len(q)) == (831, 1180)
    verts, tris = mesh.load_mesh(out)
    assert np.array_equal(verts, q.astype(np.float64) / 256) and np.array_equal(tris, M.fan(faces))
    loaded = torch.as_tensor(np.rint(verts * 256).astype(np.int32)).cuda()    # the file as it was read, back on the lattice
    vox = ops.voxelize_mesh(loaded, torch.as_tensor(tris).cuda(), 64, mode="solid")
    assert np.array_equal(vox.cpu().numpy()[0, ..., 0], chair)
    # without --merge: the file mesh.save_mesh writes of the blocky mesh, as before
    binvox_to_mesh.main([CHAIR, unit, "--blocky"])
    assert "6780 quads" in capsys.readouterr().out
    want = str(tmp_path / ("want." + ext))
    mesh.save_mesh(want, *mesh.extract(chair, smooth=False))
    assert open(unit, "rb").read() == open(want, "rb").read()


def test_colour_voxels_merge_is_exact_and_keeps_each_colour(tmp_path, capsys):
    from rendernet_amd import mesh
    from rendernet_amd.tools import colour_voxels as CT
    merged, unit = str(tmp_path / "merged.ply"), str(tmp_path / "unit.ply")
    plain = CT.main(["--from-voxels", CHAIR, "--views", "6", "--blocky", unit])
    capsys.readouterr()
    row = CT.main(["--from-voxels", CHAIR, "--views", "6", "--blocky", "--merge", merged])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == row
    assert row["exact"] is True and plain["exact"] is True and "merged_faces" not in plain
    assert {k: v for k, v in row.items() if k not in ("merged_faces", "output")} == {k: v for k, v in plain.items() if k != "output"}
    assert 831 <= row["merged_faces"] < row["faces"] == 6780                  # the colours cut the rectangles, never join them
    verts, tris = mesh.load_mesh(merged)
    cols = mesh.load_mesh_colours(merged)
    assert len(verts) == 4 * row["merged_faces"] and len(tris) == 2 * row["merged_faces"] and cols.shape == (len(verts), 3)
    assert (cols.reshape(-1, 4, 3) == cols.reshape(-1, 4, 3)[:, :1]).all()    # four private corners, one colour per rectangle
    # the rectangles cover the unit faces: the same area
    p = verts[tris]
    area = np.abs(np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 0])).sum() / 2
    assert area == row["faces"]
    # without --merge the file is the coloured unit-quad file of before: shared vertices, the vertex colours
    uverts, utris = mesh.load_mesh(unit)
    assert len(uverts) == plain["vertices"] and len(utris) == 2 * plain["faces"]
