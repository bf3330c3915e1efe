"""python -m rendernet_amd.tools.pose_voxels on the device: two pictures of the chair written from `raycast_normals` at lattice
poses are given their poses back, and the names --copy-to writes parse back to the poses printed beside them.  -m gpu."""
import json
import os

import numpy as np
import pytest

from conftest import BINVOX_DIR

pytestmark = pytest.mark.gpu


def test_pictures_get_their_poses_back(tmp_path, capsys):
    import torch
    from PIL import Image
    from oracle.io_phong import read_binvox
    from rendernet_amd import ops, synth
    from rendernet_amd.tools import data_util, pose_voxels as PV
    model = os.path.join(BINVOX_DIR, "chair.binvox")
    occ = read_binvox(model).astype(bool)
    vox = torch.from_numpy(occ.astype(np.uint8))[None, ..., None].cuda()
    lattice = synth.pose_lattice(24, synth.POSE_ELEVATIONS, synth.POSE_SCALES)
    truth = [24 * (5 * 1 + 2) + 7, 24 * (5 * 2 + 3) + 20]          # (scale 1.0, elevation 0.7, azimuth 7), (1.25, 1.0, 20)
    poses = torch.from_numpy(lattice[truth]).cuda()
    rgb = ops.raycast_normals(vox.expand(2, -1, -1, -1, -1).contiguous(), poses, new_size=128, pixels_per_cell=2)
    shots = [str(tmp_path / ("shot%d.png" % i)) for i in range(2)]
    for path, frame in zip(shots, rgb.cpu().numpy()):
        Image.fromarray(frame).save(path)
    out = tmp_path / "named"
    rows = PV.main([model] + shots + ["--threshold", "0", "--refine", "0", "--copy-to", str(out)])
    lines = [json.loads(l) for l in capsys.readouterr().out.strip().splitlines()]
    assert lines == json.loads(json.dumps(rows)) and len(rows) == 2
    for row, t, shot in zip(rows, truth, shots):
        assert row["image"] == shot and row["size"] == 64 and row["pixels_per_cell"] == 2 and row["footprint"] == 4
        assert np.array_equal(np.asarray(row["pose"], np.float32), lattice[t])
        assert row["n_inter"] <= min(row["n_splat"], row["n_mask"]) and 0.5 < row["iou"] <= 1.0
        assert abs(row["iou"] - row["n_inter"] / (row["n_splat"] + row["n_mask"] - row["n_inter"])) < 1e-12
        # the copy's name parses back, through the reference's reader, to the pose printed beside it
        assert os.path.exists(str(out / row["name"])) and row["name"].startswith("chair_p")
        back = data_util.extract_param_from_names(row["name"])[0].astype(np.float32)
        assert np.array_equal(back, np.asarray(row["name_pose"], np.float32))
        assert abs(back[0] - lattice[t][0]) < 2e-4 and abs(back[1] - lattice[t][1]) < 2e-4 and abs(3.3 / back[2] - 3.3 / lattice[t][2]) <= 0.0501
        assert 0.0 < row["name_iou"] <= 1.0
    # carve_voxels reads the folder the copies were written to
    from rendernet_amd.tools import carve_voxels as CV
    views, read_poses, f, names = CV.read_views(str(out), 64, "black", 0.0)
    assert f == 2 and sorted(r["name"] for r in rows) == names
