"""The command lines above the coloured-mesh rasteriser on the device: `colour_voxels --preview DIR` and `RenderNet_demo.py
--mesh_path coloured.ply --reference_mesh True`, with mesh.MeshSet's colours between them.  -m gpu."""
import json
import os

import numpy as np
import pytest

import mesh_extract_ref as XR
from conftest import BINVOX_DIR

pytestmark = pytest.mark.gpu

CHAIR = os.path.join(BINVOX_DIR, "chair.binvox")


@pytest.mark.parametrize("blocky", [False, True])
def test_colour_voxels_preview(tmp_path, capsys, blocky):
    """Four views of the self-check: four pictures of the frame's size named by their poses, none of them black, and the count in
    the JSON line; without the flag the line has no such field (tests/test_gpu_colour_tool.py pins the rest of it)."""
    from PIL import Image
    from rendernet_amd import synth
    from rendernet_amd.tools import colour_voxels as CT
    from rendernet_amd.tools.pose_voxels import pose_name
    out, shots = str(tmp_path / "chair.ply"), tmp_path / "preview"
    row = CT.main(["--from-voxels", CHAIR, "--views", "4", out, "--preview", str(shots)] + (["--blocky"] if blocky else []))
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == row
    assert row["preview"] == 4 and row["exact"] is True and row["views"] == 4
    poses, _ = synth.scan_poses(4)
    names = sorted(pose_name(CHAIR, p.tolist(), "_mesh.png") for p in poses)
    assert sorted(os.listdir(shots)) == names and all(n.startswith("chair_p") for n in names)
    side = 2 * 64 * CT.SCAN_PIXELS_PER_CELL
    for n in names:
        a = np.asarray(Image.open(shots / n))
        assert a.shape == (side, side, 3) and a.dtype == np.uint8
        assert 0.02 < a.any(-1).mean() < 0.6 and len(np.unique(a.reshape(-1, 3), axis=0)) > 50
    if not blocky:
        plain = CT.main(["--from-voxels", CHAIR, "--views", "4", str(tmp_path / "plain.ply")])
        assert "preview" not in plain and {k: v for k, v in row.items() if k not in ("preview", "output")} == \
            {k: v for k, v in plain.items() if k != "output"}
        with open(out) as a, open(tmp_path / "plain.ply") as b:
            assert a.read() == b.read()


@pytest.fixture(scope="module")
def sphere_files(tmp_path_factory):
    """The sphere net of 32^3 as quads, saved with seeded vertex colours and without."""
    from rendernet_amd import mesh
    d = tmp_path_factory.mktemp("coloured")
    q, faces = XR.extract(*XR.cases32()["sphere"])
    colours = np.random.RandomState(31).randint(40, 256, (len(q), 3)).astype(np.uint8)
    mesh.save_mesh(str(d / "ball.ply"), q, faces, colours=colours)
    mesh.save_mesh(str(d / "plain.ply"), q, faces)
    return d, colours


def test_mesh_set_keeps_the_colours_of_its_files(sphere_files):
    import torch
    from rendernet_amd import mesh, ops
    d, colours = sphere_files
    both = mesh.MeshSet.from_files([str(d / "ball.ply"), str(d / "ball.ply")], S=32)
    assert both.colours.dtype is torch.uint8 and np.array_equal(both.colours.cpu().numpy(), np.concatenate([colours, colours]))
    assert mesh.MeshSet.from_files([str(d / "ball.ply"), str(d / "plain.ply")], S=32).colours is None
    plain = mesh.MeshSet.from_files([str(d / "plain.ply")], S=32)
    assert plain.colours is None
    pose = torch.tensor([[4.36, 0.52, 1.0], [0.3, 1.2, 0.9]], device="cuda")
    with pytest.raises(ValueError, match="no colours"):
        plain.rasterize_colour([0, 0], pose, new_size=32)
    got, normals = both.rasterize_colour([1, 0], pose, new_size=32, return_normals=True)
    assert torch.equal(normals, both.rasterize([1, 0], pose, new_size=32))
    want = ops.rasterize_mesh_colour(both.q, both.tris, pose, 32, new_size=32, vert_offsets=both.vert_offsets,
                                     tri_offsets=both.tri_offsets, mesh_of_item=torch.tensor([1, 0], dtype=torch.int32, device="cuda"),
                                     vertex_colours=both.colours)
    assert torch.equal(got, want) and (got.reshape(-1, 3).max(0).values >= 40).all()
    flat = torch.full((int(plain.tris.shape[0]), 3), 200, dtype=torch.uint8, device="cuda")
    lit = plain.rasterize_colour([0], pose[:1], new_size=32, face_colours=flat)
    assert set(np.unique(lit.cpu().numpy()).tolist()) == {0, 200}
    with pytest.raises(ValueError, match="colours"):
        mesh.MeshSet([(both.q.cpu().numpy()[:len(colours)], both.tris.cpu().numpy()[:10])], ["x"], S=32, colours=[colours[:-1]])


def test_demo_writes_the_colour_pictures_only_for_a_coloured_mesh(sphere_files, tmp_path):
    from PIL import Image
    import RenderNet_demo
    d, _ = sphere_files
    stem = "000_%s_pose_250.000000_60.000000_3.300000_light_250.000000_60.000000"
    old = ["%s.png", "%s_reference_mesh_normal.png", "%s_reference_mesh_phong.png"]
    new = ["%s_reference_mesh_colour.png", "%s_reference_mesh_colour_phong.png"]
    RenderNet_demo.main(["--mesh_path", str(d / "ball.ply"), "--render_dir", str(tmp_path / "ball"), "--reference_mesh", "True"])
    assert sorted(os.listdir(tmp_path / "ball")) == sorted(n % (stem % "ball") for n in old + new)
    RenderNet_demo.main(["--mesh_path", str(d / "plain.ply"), "--render_dir", str(tmp_path / "plain"), "--reference_mesh", "True"])
    assert sorted(os.listdir(tmp_path / "plain")) == sorted(n % (stem % "plain") for n in old)
    hit = np.asarray(Image.open(tmp_path / "ball" / (old[1] % (stem % "ball")))).any(-1)
    albedo = np.asarray(Image.open(tmp_path / "ball" / (new[0] % (stem % "ball"))))
    phong = np.asarray(Image.open(tmp_path / "ball" / (new[1] % (stem % "ball"))))
    assert albedo.shape == phong.shape == (512, 512, 3) and 0.02 < hit.mean() < 0.6
    assert (albedo[hit] >= 40).all() and (albedo[~hit] == 0).all()            # interpolated inside the colours' range; black outside
    assert phong[hit].any() and len(np.unique(phong[hit].reshape(-1, 3), axis=0)) > 100
    for name in old[1:]:                                                     # the pictures both write are the same bytes
        with open(tmp_path / "ball" / (name % (stem % "ball")), "rb") as a, open(tmp_path / "plain" / (name % (stem % "plain")), "rb") as b:
            assert a.read() == b.read()
