"""rn_image_metrics on the device against its NumPy twin (tests/image_metrics_ref.py), every image of every batch: sad and ssd
equal as integers, the mean SSIM within 1e-9, a second call bit-identical.  The bound: the moments are exact integers on both
sides; device and twin differ by a few float64 roundings per window (about 1e-15) and by the order of the sum, at worst
n_win 2^-53 relative, below 1e-10 at 512 x 512 x 3 and far below it at these sizes.  Then the dtypes and layouts, the refusals,
and ValidationMetrics.  -m gpu."""
import os

import numpy as np
import pytest

import image_metrics_ref as MR
from conftest import BINVOX_DIR, demo_pose

pytestmark = pytest.mark.gpu

# the last: three tiles of 16 rows x 64 samples along x with one channel too (140 windows), two along y
SHAPES = [(11, 11), (11, 40), (40, 11), (12, 43), (75, 34), (128, 128), (27, 150)]


def _dev(x):
    import torch
    return torch.as_tensor(np.ascontiguousarray(x)).cuda()


def _check(a, b, a_dev=None, b_dev=None):
    """ops.image_metrics(a, b) against the twin on every image; returns (device result, twin)."""
    import torch
    from rendernet_amd import ops
    a_dev = _dev(a) if a_dev is None else a_dev
    b_dev = _dev(b) if b_dev is None else b_dev
    got, again = ops.image_metrics(a_dev, b_dev), ops.image_metrics(a_dev, b_dev)
    want = MR.image_metrics(a, b)
    Bn, H, W, C = a.shape
    assert got.sad.dtype == got.ssd.dtype == torch.int64 and got.ssim_sum.dtype == torch.float64
    assert tuple(got.sad.shape) == tuple(got.ssd.shape) == tuple(got.ssim_sum.shape) == (Bn,)
    sad, ssd, ssim_sum = got.sad.cpu().numpy(), got.ssd.cpu().numpy(), got.ssim_sum.cpu().numpy()
    n_win = (H - 10) * (W - 10) * C
    err = np.abs(ssim_sum / n_win - want["ssim"])
    print("%s: sad %s ssd %s ssim %s worst |ssim - twin| %.3g" % (a.shape, sad.tolist(), ssd.tolist(),
                                                                  (ssim_sum / n_win).tolist(), err.max() if Bn else 0.0))
    assert (sad == want["sad"]).all() and (ssd == want["ssd"]).all()
    assert (err <= 1e-9).all()
    for x, y in ((got.sad, again.sad), (got.ssd, again.ssd), (got.ssim_sum, again.ssim_sum)):      # the same bits
        assert torch.equal(x.view(torch.int64), y.view(torch.int64))
    # the derived values
    assert np.allclose(got.l1.cpu().numpy(), want["l1"], rtol=1e-14, atol=0)
    assert np.allclose(got.ssim.cpu().numpy(), ssim_sum / n_win, rtol=1e-15, atol=0)
    psnr = got.psnr.cpu().numpy()
    assert (np.isposinf(psnr) == (want["ssd"] == 0)).all()
    fin = want["ssd"] != 0
    assert np.allclose(psnr[fin], want["psnr"][fin], rtol=1e-12, atol=1e-12)
    return got, want


def _contents(H, W, C, seed):
    """Six image pairs [6,H,W,C] bytes: uniform noise, a smooth field plus small noise, black against white, a 0 / 255
    checkerboard against its inverse, identical images, white against white."""
    rng = np.random.default_rng(seed)
    yy, xx, cc = np.mgrid[0:H, 0:W, 0:C].astype(np.float64)
    smooth = 127.5 + 100.0 * np.sin(xx / 5.0 + cc) * np.cos(yy / 7.0 - cc)
    to_u8 = lambda v: np.clip(np.rint(v), 0, 255).astype(np.uint8)
    board = ((((yy + xx).astype(np.int64)) & 1) * 255).astype(np.uint8)
    noise = rng.integers(0, 256, (2, H, W, C), dtype=np.uint8)
    a = np.stack([noise[0], to_u8(smooth), np.zeros((H, W, C), np.uint8), board, noise[1], np.full((H, W, C), 255, np.uint8)])
    b = np.stack([noise[1], to_u8(smooth + rng.normal(0.0, 6.0, (H, W, C))), np.full((H, W, C), 255, np.uint8), 255 - board,
                  noise[1], np.full((H, W, C), 255, np.uint8)])
    return a, b


@pytest.mark.parametrize("C", [1, 3])
@pytest.mark.parametrize("shape", SHAPES, ids=lambda s: "%dx%d" % s)
def test_against_the_twin(shape, C):
    """One window, single rows and columns of windows, sizes that are no multiple of the 16 x 64-sample tile with seams in
    both directions, several images per launch; the largest magnitudes (black / white, checkerboard) and identical images."""
    H, W = shape
    a, b = _contents(H, W, C, seed=H * 1000 + W * 10 + C)
    got, want = _check(a, b)
    n_win = (H - 10) * (W - 10) * C
    ssim = got.ssim_sum.cpu().numpy() / n_win
    assert ssim[4] == 1.0 and ssim[5] == 1.0 and np.isposinf(got.psnr.cpu().numpy()[4:]).all()       # exactly
    assert got.ssd.cpu().numpy()[2] == 65025 * H * W * C
    assert len({float(v) for v in ssim[:4]}) == 4                    # per-image indexing: four different answers


def test_three_different_pairs_and_an_empty_batch():
    import torch
    from rendernet_amd import ops
    a, b = _contents(75, 34, 3, seed=3)
    _check(a[:3], b[:3])
    m = ops.image_metrics(_dev(a[:0]), _dev(b[:0]))
    assert tuple(m.sad.shape) == tuple(m.ssd.shape) == tuple(m.ssim_sum.shape) == (0,)
    assert m.sad.dtype == torch.int64 and m.ssim_sum.dtype == torch.float64 and m.sad.is_cuda
    assert tuple(m.psnr.shape) == tuple(m.ssim.shape) == tuple(m.l1.shape) == (0,)


def test_raycast_normals_against_a_shifted_copy():
    """A ray-cast normal map of the chair at 128 x 128 (N 32, f 4) against itself shifted by one column."""
    import torch
    from oracle.io_phong import read_binvox
    from rendernet_amd import ops
    vox = read_binvox(os.path.join(BINVOX_DIR, "chair.binvox")).astype(np.float32)[None, ..., None]
    img = ops.raycast_normals(torch.as_tensor(vox).cuda(), torch.as_tensor(demo_pose()[None]).cuda(), new_size=32, pixels_per_cell=4)
    assert tuple(img.shape) == (1, 128, 128, 3) and img.dtype == torch.uint8
    shifted = torch.roll(img, 1, dims=2)
    got, want = _check(img.cpu().numpy(), shifted.cpu().numpy(), img, shifted)
    assert 0 < got.sad.item() and 0.0 < got.ssim.item() < 1.0


def test_dtypes_and_layouts():
    import torch
    from rendernet_amd import ops
    a, b = _contents(75, 34, 3, seed=9)
    ref = ops.image_metrics(_dev(a), _dev(b))
    fa, fb = a.astype(np.float32) / np.float32(255.0), (b / 255.0).astype(np.float32)
    for x, y in ((fa, b), (a, fb), (fa, fb)):                          # k / 255 is compared as the byte k: the same bits
        m = ops.image_metrics(_dev(x), _dev(y))
        assert torch.equal(m.sad, ref.sad) and torch.equal(m.ssd, ref.ssd)
        assert torch.equal(m.ssim_sum.view(torch.int64), ref.ssim_sum.view(torch.int64))
    _check(fa, b)

    # floats that are no bytes: NaN, -1, 2, infinities, the half-way points (k + 0.5) / 255, noise beyond [0, 1]
    rng = np.random.default_rng(4)
    f = rng.uniform(-0.2, 1.2, (2, 43, 29, 3)).astype(np.float32)
    f[0, :8, :8, 0] = np.nan
    f[0, 8:12, :, 1] = -1.0
    f[0, 12:16, :, 2] = 2.0
    f[1, 0, :4, 0] = [np.inf, -np.inf, 0.0, 1.0]
    half = ((np.arange(256) + 0.5) / 255.0).astype(np.float32)
    f[1, 20:30].reshape(-1)[:256] = half
    g = rng.integers(0, 256, f.shape, dtype=np.uint8)
    _check(f, g)
    _check(g, f)

    # a non-contiguous slice: every other column of a wider image, and channels taken from a 4-channel tensor
    wide = _dev(rng.integers(0, 256, (2, 40, 70, 4), dtype=np.uint8))
    other = _dev(rng.uniform(0, 1, (2, 40, 35, 3)).astype(np.float32))
    view = wide[:, :, ::2, :3]
    assert not view.is_contiguous()
    _check(view.cpu().numpy(), other.cpu().numpy(), view, other)


def test_refusals_leave_the_device_usable():
    import torch
    from rendernet_amd import ops
    from rendernet_amd._lib import RenderNetHipError
    z = lambda *s, dt=torch.uint8: torch.zeros(*s, dtype=dt, device="cuda")
    for a, b in ((z(1, 10, 64, 3), z(1, 10, 64, 3)),                  # H = 10
                 (z(1, 64, 10, 1), z(1, 64, 10, 1)),
                 (z(1, 32, 32, 2), z(1, 32, 32, 2)),                  # C = 2
                 (z(1, 32, 32, 3), z(1, 32, 33, 3)),                  # mismatched shapes
                 (z(2, 32, 32, 3), z(1, 32, 32, 3)),
                 (z(1, 32, 32, 3, dt=torch.int32), z(1, 32, 32, 3)),  # int32 input
                 (z(1, 32, 32, 3), z(1, 32, 32, 3, dt=torch.float64)),
                 (z(32, 32, 3), z(32, 32, 3))):
        with pytest.raises(RenderNetHipError):
            ops.image_metrics(a, b)
    a, b = _contents(12, 43, 1, seed=1)
    _check(a, b)


def test_validation_metrics_accumulator():
    from rendernet_amd.metrics import ValidationMetrics, psnr_for_mean
    rng = np.random.default_rng(8)
    H, W, C = 24, 20, 3
    pred1 = rng.uniform(0, 1, (2, H, W, C)).astype(np.float32)
    tgt1 = np.clip(pred1 + rng.normal(0, 0.05, pred1.shape), 0, 1).astype(np.float64)        # a NumPy float target
    pred2 = rng.uniform(0, 1, (3, H, W, C)).astype(np.float32)
    tgt2 = MR.quantise(pred2)                                                                  # uint8 on the device
    tgt2[1] = rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    vm = ValidationMetrics()
    vm.add(_dev(pred1), tgt1)
    w1 = MR.image_metrics(pred1, tgt1.astype(np.float32))
    words = vm.line().split()
    assert words[0] == "Validation" and words[1] == "PSNR" and words[3] == "SSIM" and len(words) == 5
    assert not vm.line().startswith("Validation accuracy")
    assert (float(words[2]), float(words[4])) == vm.last()
    assert abs(vm.last()[0] - w1["psnr"].mean()) <= 1e-9 and abs(vm.last()[1] - w1["ssim"].mean()) <= 1e-9
    vm.add(_dev(pred2), _dev(tgt2))
    w2 = MR.image_metrics(pred2, tgt2)
    assert np.isposinf(w2["psnr"][[0, 2]]).all() and np.isposinf(np.asarray(vm.psnr)[[2, 4]]).all()      # equal images
    assert vm.line(prefix="normal ").startswith("normal PSNR ")
    psnr, ssim = vm.epoch_means()
    want_psnr = np.concatenate([w1["psnr"], psnr_for_mean(w2["psnr"], H * W * C)]).mean()
    want_ssim = np.concatenate([w1["ssim"], w2["ssim"]]).mean()
    assert np.isfinite(psnr) and abs(psnr - want_psnr) <= 1e-9 and abs(ssim - want_ssim) <= 1e-9
    assert len(vm.psnr) == len(vm.ssim) == 5
