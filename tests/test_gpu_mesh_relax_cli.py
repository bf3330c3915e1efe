"""The command lines of the surface-net relaxation on the device: binvox_to_mesh --relax writes the twin's relaxed mesh and,
without the flag, the file it always wrote; colour_voxels --relax keeps the self-check exact and the colours what they were.
-m gpu."""
import os

import numpy as np
import pytest

import mesh_extract_ref as E
import mesh_relax_ref as X
from conftest import BINVOX_DIR

pytestmark = pytest.mark.gpu

CHAIR = os.path.join(BINVOX_DIR, "chair.binvox")


@pytest.fixture(scope="module")
def chair_mesh():
    from rendernet_amd.tools import binvox_rw
    with open(CHAIR, "rb") as f:
        grid = np.ascontiguousarray(binvox_rw.read_as_3d_array(f).data).astype(np.uint8)
    return E.extract(grid, 0.5, True)


def test_binvox_to_mesh_relax_writes_the_twins_mesh(tmp_path, capsys, chair_mesh):
    from rendernet_amd import mesh
    from rendernet_amd.tools import binvox_to_mesh
    q, faces = chair_mesh
    out = str(tmp_path / "chair.ply")
    binvox_to_mesh.main([CHAIR, out, "--relax", "4"])
    v, t = mesh.load_mesh(out)
    want = X.relax(q, faces, 64, 4, 256)
    assert not np.array_equal(want, q)
    assert np.array_equal(v, want / 256.0) and np.array_equal(t, E.fan(faces))
    obj = str(tmp_path / "chair.obj")
    binvox_to_mesh.main([CHAIR, obj, "--relax", "5", "--relax-weight", "128"])
    v, t = mesh.load_mesh(obj)
    assert np.array_equal(v, X.relax(q, faces, 64, 5, 128) / 256.0) and np.array_equal(t, E.fan(faces))
    capsys.readouterr()
    for argv in ([CHAIR, out, "--relax", "65"], [CHAIR, out, "--relax", "-1"], [CHAIR, out, "--relax", "4", "--relax-weight", "0"]):
        with pytest.raises(SystemExit):
            binvox_to_mesh.main(argv)


def test_without_the_flag_the_file_is_what_it_was(tmp_path, capsys, chair_mesh):
    """The bytes of the file are those of save_mesh on the unrelaxed twin mesh, which is what the tool wrote before the flag
    existed (tests/test_gpu_mesh_extract.py pins the device to that twin); --relax 0 writes the same bytes."""
    from rendernet_amd import mesh
    from rendernet_amd.tools import binvox_to_mesh
    q, faces = chair_mesh
    for ext in ("ply", "obj"):
        want, out, zero = str(tmp_path / ("want." + ext)), str(tmp_path / ("out." + ext)), str(tmp_path / ("zero." + ext))
        mesh.save_mesh(want, q, faces)
        binvox_to_mesh.main([CHAIR, out])
        binvox_to_mesh.main([CHAIR, zero, "--relax", "0"])
        data = open(want, "rb").read()
        assert len(data) > 100000 and open(out, "rb").read() == data and open(zero, "rb").read() == data
    capsys.readouterr()


def test_colour_voxels_relax_keeps_the_self_check_exact_and_the_colours(tmp_path, capsys, chair_mesh):
    from rendernet_amd import mesh
    from rendernet_amd.tools import colour_voxels as CT
    q, faces = chair_mesh
    plain, relaxed = str(tmp_path / "plain.ply"), str(tmp_path / "relaxed.ply")
    row0 = CT.main(["--from-voxels", CHAIR, "--views", "6", plain])
    row4 = CT.main(["--from-voxels", CHAIR, "--views", "6", "--relax", "4", relaxed])
    capsys.readouterr()
    assert row0["exact"] is True and row4["exact"] is True and dict(row4, output=plain) == row0
    v0, t0 = mesh.load_mesh(plain)
    v4, t4 = mesh.load_mesh(relaxed)
    assert np.array_equal(v0, q / 256.0) and np.array_equal(v4, X.relax(q, faces, 64, 4, 256) / 256.0) and np.array_equal(t0, t4)
    c0, c4 = mesh.load_mesh_colours(plain), mesh.load_mesh_colours(relaxed)
    assert c0 is not None and np.array_equal(c0, c4) and len(np.unique(c0, axis=0)) > 100


def test_save_meshes_passes_relax_through(tmp_path):
    """What the reconstruction script does with "mesh_relax": soft volumes at the config's threshold, one relaxed .ply each."""
    import torch
    from rendernet_amd import mesh
    soft = np.stack([E.sphere_field(32) * np.float32(0.2), np.zeros((32, 32, 32), np.float32)])
    paths = [str(tmp_path / ("h%d.ply" % b)) for b in range(2)]
    mesh.save_meshes(paths, torch.as_tensor(soft[..., None]).cuda(), threshold=0.1, relax=4, relax_weight=128)
    q, faces = E.extract(soft[0], 0.1, True)
    v, t = mesh.load_mesh(paths[0])
    want = X.relax(q, faces, 32, 4, 128)
    assert not np.array_equal(want, q) and np.array_equal(v, want / 256.0) and np.array_equal(t, E.fan(faces))
    assert len(mesh.load_mesh(paths[1])[0]) == 0
