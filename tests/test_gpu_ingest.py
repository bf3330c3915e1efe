"""rn_target_u8_crop_fwd (rendernet_amd/csrc/ingest.hip): decoded 8-bit frames -> the float32 target window, bit-equal to
the host path (`ops.target_u8_crop_reference`, itself pinned to data_loader's NumPy expressions in tests/test_loader_cpu.py),
and the trainers taking uint8 device batches through it.  -m gpu."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

PAIRS = ((1, 1), (3, 1), (4, 1), (3, 3), (4, 3))          # (Cs, Co)
GUARD = 64                                                 # floats of sentinel on either side of the output
SENTINEL = -7.25


def _exhaustive_frames(cs):
    """[1, 1, n, cs]: every channel sum (cs 3: 0..765, cs 4: 0..1020) or every byte (cs 1), plus the reversed channel order."""
    if cs == 1:
        return np.arange(256, dtype=np.uint8).reshape(1, 1, 256, 1)
    sums = np.arange(255 * cs + 1)
    img = np.zeros((len(sums), cs), np.uint8)
    for k in range(cs):
        img[:, k] = np.clip(sums - 255 * k, 0, 255)
    both = np.concatenate([img, img[:, ::-1]], 0)
    pad = (-len(both)) % 4                                 # a multiple of four columns: the vector kernel sees them too
    both = np.concatenate([both, np.zeros((pad, cs), np.uint8)], 0)
    return np.ascontiguousarray(both.reshape(1, 1, len(both), cs))


def _run(frames_dev, shape, window, co, offset_floats=0):
    """Raw C-ABI call into a sentinel-framed buffer; returns (rc, patch as NumPy, guards untouched?)."""
    import torch
    from rendernet_amd import _lib as L
    B, H, W, Cs = shape
    row0, col0, ph, pw = window
    n = max(0, B * ph * pw * co)
    buf = torch.full((GUARD + offset_floats + n + GUARD,), SENTINEL, dtype=torch.float32, device="cuda")
    out = buf[GUARD + offset_floats:GUARD + offset_floats + n]
    rc = L.lib().rn_target_u8_crop_fwd(ctypes.c_void_p(frames_dev.data_ptr() if frames_dev is not None else None),
                                       ctypes.c_void_p(out.data_ptr() if n else buf.data_ptr()), B, H, W, Cs, co, row0, col0,
                                       ph, pw, L.stream_ptr())
    torch.cuda.synchronize()
    host = buf.cpu().numpy()
    lo, hi = host[:GUARD + offset_floats], host[GUARD + offset_floats + n:]
    return rc, host[GUARD + offset_floats:GUARD + offset_floats + n], bool((lo == SENTINEL).all() and (hi == SENTINEL).all())


def test_kernel_is_bit_equal_on_every_input_value():
    import torch
    from rendernet_amd import ops
    for cs, co in PAIRS:
        fr = _exhaustive_frames(cs)
        n = fr.shape[2]
        dev = torch.as_tensor(fr).cuda()
        for window, off in (((0, 0, 1, n), 0),             # vector kernel (n % 4 == 0, aligned output)
                            ((0, 0, 1, n), 1),             # same window into a float-aligned-only output: pixel kernel
                            ((0, 1, 1, n - 2), 0),         # odd start, width not a multiple of four: pixel kernel, unaligned bytes
                            ((0, 1, 1, n - 4), 0)):         # vector kernel on source bytes that are not dword aligned
            want = ops.target_u8_crop_reference(fr, window, co)
            rc, got, clean = _run(dev, fr.shape, window, co, off)
            assert rc == 0 and clean
            assert np.array_equal(got.reshape(want.shape), want), (cs, co, window, off)
        # and through the Python wrapper
        assert np.array_equal(ops.target_u8_crop(dev, (0, 0, 1, n), co).cpu().numpy(), ops.target_u8_crop_reference(fr, (0, 0, 1, n), co))


def test_kernel_is_bit_equal_on_training_windows():
    """512^2 frames; windows of 128, 256 and 512 pixels at offset 0, an odd multiple of four, and flush with the far edge;
    B 1, 3, 24; all five (Cs, Co) pairs; the guard band stays untouched."""
    import torch
    from rendernet_amd import ops
    rng = np.random.default_rng(11)
    H = W = 512
    cases = [(128, 0, 0), (128, 4 * 31, 4 * 17), (128, 512 - 128, 512 - 128), (128, 0, 512 - 128),
             (256, 0, 0), (256, 4 * 33, 4 * 5), (256, 512 - 256, 512 - 256), (512, 0, 0)]
    for cs, co in PAIRS:
        full = rng.integers(0, 256, (24, H, W, cs), dtype=np.uint8)
        for B in (1, 3, 24):
            fr = np.ascontiguousarray(full[24 - B:])
            dev = torch.as_tensor(fr).cuda()
            for p, r0, c0 in cases:
                want = ops.target_u8_crop_reference(fr, (r0, c0, p, p), co)
                rc, got, clean = _run(dev, fr.shape, (r0, c0, p, p), co)
                assert rc == 0 and clean, (cs, co, B, p, r0, c0)
                assert np.array_equal(got.reshape(want.shape), want), (cs, co, B, p, r0, c0)
    # a non-square window that is not a multiple of four wide, not on a multiple of four
    fr = rng.integers(0, 256, (2, 40, 52, 4), dtype=np.uint8)
    dev = torch.as_tensor(fr).cuda()
    for co in (1, 3):
        want = ops.target_u8_crop_reference(fr, (3, 5, 37, 47), co)
        rc, got, clean = _run(dev, fr.shape, (3, 5, 37, 47), co)
        assert rc == 0 and clean and np.array_equal(got.reshape(want.shape), want)


def test_bad_arguments_are_refused_without_a_launch():
    import torch
    from rendernet_amd import _lib as L
    from rendernet_amd import ops
    fr = np.full((2, 16, 16, 3), 200, np.uint8)
    dev = torch.as_tensor(fr).cuda()
    bad = [((2, 16, 16, 3), (0, 0, 17, 16), 1), ((2, 16, 16, 3), (0, 1, 16, 16), 1), ((2, 16, 16, 3), (-4, 0, 8, 8), 3),
           ((2, 16, 16, 3), (0, 0, 0, 8), 1), ((2, 16, 16, 3), (12, 12, 8, 8), 3), ((2, 16, 16, 3), (0, 0, 8, 8), 2),
           ((2, 16, 16, 1), (0, 0, 8, 8), 3), ((2, 16, 16, 2), (0, 0, 8, 8), 1), ((-1, 16, 16, 3), (0, 0, 8, 8), 1),
           ((2, 0, 16, 3), (0, 0, 8, 8), 1)]
    for shape, window, co in bad:
        rc, got, clean = _run(dev, shape, window, co)
        assert rc != 0 and clean and (got == SENTINEL).all(), (shape, window, co)
        assert b"rn_target_u8_crop_fwd" in L.lib().rn_last_error()
    rc, got, clean = _run(None, (2, 16, 16, 3), (0, 0, 8, 8), 1)                      # null frames
    assert rc != 0 and clean and (got == SENTINEL).all() and b"null" in L.lib().rn_last_error()
    rc, got, clean = _run(dev, (0, 16, 16, 3), (0, 0, 8, 8), 1)                       # B == 0: a no-op
    assert rc == 0 and clean
    with pytest.raises(ValueError):
        ops.target_u8_crop(dev, (0, 0, 17, 16), 1)
    with pytest.raises(L.RenderNetHipError):
        ops.target_u8_crop(dev.float(), (0, 0, 8, 8), 1)
    with pytest.raises(L.RenderNetHipError):
        ops.target_u8_crop(torch.as_tensor(fr), (0, 0, 8, 8), 1)                      # host tensor: no CPU path


def test_the_step_sees_the_same_bits(fixtures_vox):
    """One set of weights, one window: uint8 device voxels / frames against today's float host arrays give the same
    prediction, the same target and so the same d(pred), bit for bit.  The scalar loss is summed in double precision with
    atomics in free order: the two values may differ by reordering only, n * 2^-53 relative for n prediction elements
    (no cancellation: BCE terms are above -1e-6) = 3.7e-12 here; asserted at 1e-10."""
    import torch
    from rendernet_amd.shader import ShaderSpec, init_shader_weights
    from rendernet_amd.train import Trainer
    spec = ShaderSpec(out_ch=1).check()
    tr = Trainer(spec, init_shader_weights(spec, seed=1234), keep_prob=0.75)
    rng = np.random.default_rng(5)
    B, crop, start = 2, 32, (7, 20)
    frames = rng.integers(0, 256, (B, 512, 512, 3), dtype=np.uint8)
    vox_u8 = (fixtures_vox[[0, 3]] > 0).astype(np.uint8)
    poses = np.array([[4.36, 0.52, 1.0], [1.0, -0.3, 1.1]], np.float32)
    # today's host feed: data_loader's float frames (mean over the channels), the script's / 255.0, float voxels
    host_frames = np.stack([np.reshape(np.mean(f.astype(np.float32), axis=2), (512, 512, 1)) for f in frames]) / 255.0
    host_vox = vox_u8.astype(np.float32)
    dev_frames, dev_vox, dev_poses = (torch.as_tensor(a).to(tr.device) for a in (frames, vox_u8, poses))

    pred_a, (r, c, p, _) = tr.forward(host_vox, poses, crop, start)
    pred_b, win_b = tr.forward(dev_vox, dev_poses, crop, start)
    assert (r, c, p) == (7, 20, 32) and win_b[:3] == (r, c, p) and pred_a.shape == (B, 128, 128, 1)
    assert torch.equal(pred_a, pred_b)
    tgt_a = tr._target_patch(host_frames, r, c, p, 1)
    tgt_b = tr._target_patch(dev_frames, r, c, p, 1)
    assert tgt_b.dtype == torch.float32 and tgt_b.is_contiguous() and torch.equal(tgt_a, tgt_b)
    losses, grads = [], []
    for pred, tgt in ((pred_a, tgt_a), (pred_b, tgt_b)):
        tr.loss_buf.zero_()
        grads.append(tr._loss_grad(pred.detach(), tgt, B, False))
        losses.append(float(tr.loss_buf[0].item()))
    assert torch.equal(grads[0], grads[1])
    bound = 1e-10
    rel = abs(losses[0] - losses[1]) / abs(losses[0])
    print("loss host %r uint8 %r rel %.3g" % (losses[0], losses[1], rel))
    assert np.isfinite(losses[0]) and losses[0] > 0 and rel <= bound
    # and the whole step on the uint8 batch: same global_step -> same dropout masks -> the same loss again
    loss = float(tr.step(dev_vox, dev_poses, dev_frames, patch_size=crop, start_point=start, global_batch=B).item())
    print("step loss %r" % loss)
    assert abs(loss - losses[0]) / abs(losses[0]) <= bound and tr.global_step == 1
    # the texture trainer shares the helper (three-channel targets)
    rgb_a = tr._target_patch(frames.astype(np.float32) / 255.0, r, c, p, 3)
    rgb_b = tr._target_patch(dev_frames, r, c, p, 3)
    assert torch.equal(rgb_a, rgb_b)
