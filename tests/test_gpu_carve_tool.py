"""python -m rendernet_amd.tools.carve_voxels on the device: a folder of PNGs written from `raycast_normals` is carved into the
visual hull, and the --from-voxels round trip returns the chair.  -m gpu."""
import json
import os

import numpy as np
import pytest

from conftest import BINVOX_DIR

pytestmark = pytest.mark.gpu


def test_images_to_hull_and_round_trip(tmp_path, capsys):
    import torch
    from PIL import Image
    from oracle.io_phong import read_binvox
    from rendernet_amd import ops
    from rendernet_amd.tools import binvox_rw, carve_voxels as CV
    occ = read_binvox(os.path.join(BINVOX_DIR, "chair.binvox")).astype(bool)
    vox = torch.from_numpy(occ.astype(np.uint8))[None, ..., None].cuda()
    shots = tmp_path / "shots"
    shots.mkdir()
    names = ["chair_p%.2f_t%.2f_r3.3.png" % (az, el) for az, el in ((10.0, 70.0), (100.0, 40.0), (190.0, 85.0), (280.0, 55.0),
                                                                      (55.0, 20.0), (325.0, 60.0))]
    poses = torch.from_numpy(np.stack([CV.pose_of_name(n) for n in names])).cuda()
    rgb = ops.raycast_normals(vox.expand(len(names), -1, -1, -1, -1).contiguous(), poses, new_size=128, pixels_per_cell=2)
    for n, frame in zip(names, rgb.cpu().numpy()):
        Image.fromarray(frame).save(str(shots / n))
    out = str(tmp_path / "hull.binvox")
    row = CV.main([str(shots), out, "--threshold", "0"])
    assert json.loads(capsys.readouterr().out.strip().splitlines()[-1]) == row
    assert row["views"] == 6 and row["size"] == 64 and row["mode"] == "silhouettes" and "warning" not in row
    assert abs(row["pixels_per_voxel"] - 2.0) < 1e-3
    with open(out, "rb") as fh:
        hull = binvox_rw.read_as_3d_array(fh).data.astype(bool)
    assert hull.shape == (64, 64, 64) and hull.sum() == row["voxels"]
    assert not (occ & ~hull).any() and occ.sum() < hull.sum() < 64 ** 3 // 4     # the visual hull holds the chair, loosely
    # the same call through ops: the tool adds nothing to the rule
    views, read_poses, f, read_names = CV.read_views(str(shots), 64, "black", 0.0)     # in sorted file order
    assert f == 2 and read_names == sorted(names)
    want = ops.voxel_carve(torch.from_numpy(views).cuda()[None], torch.from_numpy(read_poses).cuda()[None], 64, new_size=128,
                           pixels_per_cell=2, use_depth=False)
    assert np.array_equal(want[0, ..., 0].cpu().numpy().astype(bool), hull)
    # the round trip with depth
    back = str(tmp_path / "back.binvox")
    row = CV.main(["--from-voxels", os.path.join(BINVOX_DIR, "chair.binvox"), "--views", "24", back])
    assert row["views"] == 24 and row["mode"] == "depth" and row["iou"] >= 0.999 and row["hausdorff"] <= 2.0
    with open(back, "rb") as fh:
        again = binvox_rw.read_as_3d_array(fh).data.astype(bool)
    assert not (occ & ~again).any() and again.sum() == row["voxels"]
