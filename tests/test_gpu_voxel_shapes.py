"""rn_voxel_shapes on the device against its NumPy twin (tests/voxel_shapes_ref.py): every voxel of every grid, exactly.
Then what is built on it: the generator's grids through the packer and the caster, the synthetic feed with procedural
grids only, one trainer step on them, and the demo's --voxel_shape.  -m gpu."""
import ctypes
import dataclasses
import os

import numpy as np
import pytest

import voxel_shapes_ref as VR
from conftest import demo_pose

pytestmark = pytest.mark.gpu


def _rot(rng):
    q = rng.standard_normal(4)
    w, x, y, z = q / np.sqrt((q * q).sum())
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return np.rint(64 * R).astype(np.int64)


def _device_grid(prims, S):
    import torch
    from rendernet_amd import ops
    return ops.voxel_shapes(torch.as_tensor(np.ascontiguousarray(prims, np.int32)).cuda(), S).cpu().numpy()


def _same(prims, S):
    got, want = _device_grid(prims, S), VR.voxel_shapes(prims, S)
    assert got.dtype == np.uint8 and got.shape == want.shape == (len(prims), S, S, S, 1)
    diff = int((got != want).sum())
    print("S %d B %d K %d: %d of %d voxels differ, fill %.4f" % (S, len(prims), prims.shape[1], diff, want.size, want.mean()))
    assert diff == 0
    return want


@pytest.mark.parametrize("rotated", [False, True])
def test_each_type_alone(rotated):
    """One primitive per item, the five types in one launch; semi-axes that tell the three axes apart, an off-centre centre."""
    rng = np.random.default_rng(1)
    prims = np.stack([[VR.make_prim(t, 0, (3, -4, 5), (22, 8 if t == 4 else 13, 17), _rot(rng) if rotated else None)]
                      for t in range(5)])
    want = _same(prims, 32)
    assert want.reshape(5, -1).any(1).all() and len({int(w.sum()) for w in want}) == 5


def _full_slots(rng, B, S):
    """Eight live slots per item: slot 0 a large union, then unions and subtractions in a drawn order."""
    prims = np.zeros((B, 8, 16), np.int32)
    for b in range(B):
        for k in range(8):
            op = 0 if k == 0 else int(rng.integers(0, 2))
            a = rng.integers(S // 4, S // 2, 3) if k == 0 else rng.integers(S // 10, S // 3, 3)
            c = rng.integers(-S // 3, S // 3 + 1, 3)
            prims[b, k] = VR.make_prim(int(rng.integers(0, 5)), op, c, a, _rot(rng))
    return prims


@pytest.mark.parametrize("S,B", [(32, 3), (64, 2)])
def test_eight_slots_of_unions_and_subtractions(S, B):
    """Slot order, both grid sizes (one and four z slices per block) and the batch stride."""
    prims = _full_slots(np.random.default_rng(S), B, S)
    assert set(np.unique(prims[:, 1:, 0] >> 8)) == {0, 1}
    want = _same(prims, S)
    assert want.reshape(B, -1).any(1).all()
    swapped = prims.copy()                                                       # the order of the slots is part of the rule
    swapped[:, 1:] = prims[:, :0:-1]
    assert not np.array_equal(VR.voxel_shapes(swapped, S), want)
    _same(swapped, S)


def test_garbage_words_are_clamped():
    """Any int32 is a legal word.  Items 0 and 1 are garbage throughout (a live slot needs 24 zero bits: they are all no-ops);
    items 2 and 3 keep garbage in words 1..15 under a drawn legal word 0, so that the clamps decide what is rasterised."""
    rng = np.random.default_rng(2)
    prims = rng.integers(-2 ** 31, 2 ** 31, (4, 8, 16)).astype(np.int32)
    prims[2:, :, 0] = rng.integers(0, 5, (2, 8)) | rng.integers(0, 2, (2, 8)) << 8
    prims[2:, 0, 0] &= 255                                                       # slot 0 unites
    want = _same(prims, 32)
    assert not want[:2].any() and want[2:].any()


def test_no_primitives_no_items():
    import torch
    from rendernet_amd import ops
    assert not _device_grid(np.zeros((2, 0, 16), np.int32), 32).any()            # K = 0
    dead = np.random.default_rng(0).integers(-99, 99, (2, 8, 16)).astype(np.int32)
    dead[:, :, 0] = [VR.NOOP, 5, 2 << 8, 1 | 2 << 8, -1, -256, 1 | -1 << 8, 1 << 30]
    assert not _device_grid(dead, 32).any() and not VR.voxel_shapes(dead, 32).any()
    out = ops.voxel_shapes(torch.zeros((0, 8, 16), dtype=torch.int32, device="cuda"), 64)
    assert out.shape == (0, 64, 64, 64, 1) and out.dtype is torch.uint8
    torch.cuda.synchronize()


def test_ops_refuses_bad_arguments():
    import torch
    from rendernet_amd import ops
    from rendernet_amd._lib import RenderNetHipError
    good = torch.zeros((1, 2, 16), dtype=torch.int32, device="cuda")
    for prims, S in ((good, 128), (good, 48), (good, 64.0), (good.long(), 32), (good[0], 32), (good[:, :, :8], 32),
                     (torch.zeros((1, 9, 16), dtype=torch.int32, device="cuda"), 32), (good.cpu(), 32)):
        with pytest.raises(RenderNetHipError):
            ops.voxel_shapes(prims, S)


def test_the_c_entry_refuses_before_it_launches():
    """RN_E_INVALID, and an output buffer filled with 0xAA keeps every byte, for each bad argument."""
    import torch
    from rendernet_amd import _lib
    L = _lib.lib()
    prims = torch.zeros((2 * 9 * 16 + 4,), dtype=torch.int32, device="cuda")
    prims[0::16] = 1                                                             # boxes, if anything were launched
    prims[4:7] = 100
    vox = torch.full((2 * 64 ** 3,), 0xAA, dtype=torch.uint8, device="cuda")
    vp, st = ctypes.c_void_p, _lib.stream_ptr()
    assert prims.data_ptr() % 16 == 0 and vox.data_ptr() % 16 == 0
    cases = {"S = 128": (vp(prims.data_ptr()), vp(vox.data_ptr()), 1, 8, 128),
             "S = 48": (vp(prims.data_ptr()), vp(vox.data_ptr()), 2, 8, 48),
             "K = 9": (vp(prims.data_ptr()), vp(vox.data_ptr()), 2, 9, 32),
             "K = -1": (vp(prims.data_ptr()), vp(vox.data_ptr()), 2, -1, 32),
             "B = -1": (vp(prims.data_ptr()), vp(vox.data_ptr()), -1, 8, 32),
             "misaligned prims": (vp(prims.data_ptr() + 4), vp(vox.data_ptr()), 2, 8, 32),
             "misaligned vox": (vp(prims.data_ptr()), vp(vox.data_ptr() + 4), 2, 8, 32),
             "null prims": (None, vp(vox.data_ptr()), 2, 8, 32),
             "null vox": (vp(prims.data_ptr()), None, 2, 8, 32)}
    for what, args in cases.items():
        assert L.rn_voxel_shapes(*args, st) == -1, what                          # RN_E_INVALID
        assert b"rn_voxel_shapes" in L.rn_last_error(), what
    torch.cuda.synchronize()
    assert bool((vox == 0xAA).all())
    assert L.rn_voxel_shapes(None, None, 0, 8, 64, st) == 0                      # B == 0 is a no-op whatever the pointers
    assert L.rn_voxel_shapes(vp(prims.data_ptr()), vp(vox.data_ptr()), 2, 8, 32, st) == 0
    torch.cuda.synchronize()
    assert bool((vox[:2 * 32 ** 3] <= 1).all()) and bool(vox[:2 * 32 ** 3].any()) and bool((vox[2 * 32 ** 3:] == 0xAA).all())


SHAPE_SEED, SHAPE_IDS = 1234, [0, 1, 2, 0x1a2b3c4d, 0xdeadbeef, 0xffffffff]


def test_generator_grids_reach_the_packer_and_the_caster():
    import torch
    from rendernet_amd import ops, synth
    prims = synth.shape_prims(SHAPE_SEED, SHAPE_IDS, 64)
    want = _same(prims, 64)
    vox = torch.as_tensor(want).cuda()
    _, box = ops.voxel_pack(vox)
    box = box.cpu().numpy()
    print("boxes:\n%s" % box)
    assert (box[:, :3] >= 1).all() and (box[:, 3:] <= 62).all() and (box[:, :3] <= box[:, 3:]).all()     # strictly inside
    pose = torch.as_tensor(np.tile(demo_pose(), (len(SHAPE_IDS), 1))).cuda()
    normals = ops.raycast_normals(vox, pose)
    hits = (normals.amax(dim=3) > 0).reshape(len(SHAPE_IDS), -1).sum(1).cpu().numpy()
    print("hit pixels: %s" % hits)
    assert (hits >= 1).all()


def test_feed_of_shapes_alone_trains():
    """SyntheticTargets(shapes=1.0, models=None): the documented dtypes and shapes, the grids of the ids in the names, and one
    finite step of a reduced trainer on them (tiny_spec on 32^3 grids: 32^3 -> 32^3 -> 128^2)."""
    import torch
    from rendernet_amd import ops, synth
    from rendernet_amd.shader import init_shader_weights, tiny_spec
    from rendernet_amd.train import Trainer
    spec = dataclasses.replace(tiny_spec(3), size=32).check()
    tr = Trainer(spec, init_shader_weights(spec, seed=1234), device="cuda", e_eta=1e-4, keep_prob=1.0)
    feed = synth.SyntheticTargets(None, (), 2, 1, seed=3, device="cuda", new_size=32, shapes=1.0, shape_seed=77, shape_size=32)
    losses = []
    for frames, vox, poses, names in feed:
        assert frames.dtype is torch.uint8 and frames.shape == (2, 128, 128, 3) and frames.is_cuda
        assert vox.dtype is torch.uint8 and vox.shape == (2, 32, 32, 32, 1) and vox.is_cuda
        assert poses.dtype is torch.float32 and poses.shape == (2, 3) and poses.is_cuda and len(names) == 2
        ids = [int(n[len("shape"):len("shape") + 8], 16) for n in names]
        prims = synth.shape_prims(77, ids, 32)
        assert torch.equal(vox, ops.voxel_shapes(torch.as_tensor(prims).cuda(), 32))
        assert np.array_equal(vox.cpu().numpy(), VR.voxel_shapes(prims, 32))
        assert torch.equal(frames, ops.raycast_normals(vox, poses, new_size=32, pixels_per_cell=4))
        assert int((frames.amax(dim=3) > 0).sum()) > 0
        losses.append(float(tr.step(vox, poses, frames, patch_size=8, start_point=(8, 8)).item()))
    print("losses: %s" % losses)
    assert len(losses) == 1 and np.isfinite(losses).all()


def test_demo_renders_a_shape_and_saves_its_grid(tmp_path):
    import RenderNet_demo
    from rendernet_amd import synth
    from rendernet_amd.tools import binvox_rw
    out, path = tmp_path / "render", str(tmp_path / "shape.binvox")
    RenderNet_demo.main(["--voxel_shape", "1a2b3c4d", "--shape_seed", str(SHAPE_SEED), "--save_binvox", path, "--render_dir", str(out)])
    assert sorted(os.listdir(out)) == ["000_shape1a2b3c4d_pose_250.000000_60.000000_3.300000_light_250.000000_60.000000.png"]
    with open(path, "rb") as f:
        back = binvox_rw.read_as_3d_array(f)
    grid = _device_grid(synth.shape_prims(SHAPE_SEED, [0x1a2b3c4d], 64), 64)
    assert back.dims == [64, 64, 64] and grid.any() and np.array_equal(back.data, grid[0, ..., 0].astype(bool))
