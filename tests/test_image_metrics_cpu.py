"""Image metrics without a GPU: the header's weights and bounds against the rule computed afresh and Python's unbounded
integers, closed forms, the NumPy twin (tests/image_metrics_ref.py) against standard float64 SSIM, the quantisation rule, the
--val-metrics option, the host derivation and the error text of ops.image_metrics."""
import os
import re

import numpy as np
import pytest

import image_metrics_ref as MR
from conftest import ROOT

T = 1 << 24


def _header():
    return open(os.path.join(ROOT, "include", "rendernet_hip.h")).read()


def test_weights_in_the_header_follow_the_rule():
    m = re.search(r"#define\s+RN_SSIM_WEIGHTS\s+([0-9, ]+)", _header())
    hdr = tuple(int(v) for v in m.group(1).split(","))
    assert len(hdr) == 11 and hdr == MR.weights_from_rule() == MR.WEIGHTS
    assert sum(hdr) == 4096 and hdr == hdr[::-1]
    assert sum(hdr[i] * hdr[j] for i in range(11) for j in range(11)) == T
    k1 = float(re.search(r"#define\s+RN_SSIM_K1\s+([0-9.]+)", _header()).group(1))
    k2 = float(re.search(r"#define\s+RN_SSIM_K2\s+([0-9.]+)", _header()).group(1))
    assert (k1, k2) == (MR.K1, MR.K2) and abs(k1 - (0.01 * 255) ** 2) < 1e-12 and abs(k2 - (0.03 * 255) ** 2) < 1e-12


def test_bounds_are_reached_exactly():
    """Black against white and a 0 / 255 checkerboard against its inverse: the header's maxima, in unbounded integers, and the
    twin's 64-bit arithmetic gives the same numbers."""
    white, black = np.full((11, 11), 255, np.uint8), np.zeros((11, 11), np.uint8)
    m = MR.window_moments_bigint(white, black)
    assert m["A"] == 255 * T < 2 ** 32 and m["B"] == 0
    assert m["Saa"] == 65025 * T < 2 ** 40
    assert m["TSaa"] == m["AA"] == 65025 * 2 ** 48 == 18302910360610406400 < 2 ** 64       # the largest product there is
    assert m["Va"] == m["Vb"] == m["Cab"] == 0
    m = MR.window_moments_bigint(white, white)
    assert m["TSab"] == m["AB"] == 65025 * 2 ** 48 and m["Cab"] == 0

    yy, xx = np.mgrid[0:11, 0:11]
    board = (((yy + xx) & 1) * 255).astype(np.uint8)
    m = MR.window_moments_bigint(board, 255 - board)
    even, odd = sum(MR.WEIGHTS[0::2]), sum(MR.WEIGHTS[1::2])
    assert (even, odd) == (2046, 2050)
    bound = 65025 * T * T // 4                                                            # 16256.25 * 2^48
    assert m["Va"] == m["Vb"] == -m["Cab"] == 65025 * (T * T // 4 - 64)                     # T/2 +- 8 on the two values
    assert 0 <= bound - m["Va"] == 64 * 65025 and bound < 2 ** 63
    assert all(0 <= m[k] < 2 ** 64 for k in ("TSaa", "TSbb", "TSab", "AA", "BB", "AB"))

    # the twin's uint64 / wrap-around arithmetic at the same windows
    for a, b in ((white, black), (white, white), (board, 255 - board), (255 - board, board), (board, board)):
        big = MR.window_moments_bigint(a, b)
        A, B, Saa, Sbb, Sab = (int(v[0, 0, 0, 0]) for v in MR.moments(a[None, ..., None], b[None, ..., None]))
        assert (A, B, Saa, Sbb, Sab) == tuple(big[k] for k in ("A", "B", "Saa", "Sbb", "Sab"))
        Va = (T * Saa - A * A) % 2 ** 64
        Cab = (T * Sab - A * B) % 2 ** 64
        assert Va == big["Va"] and (Cab - 2 ** 64 if Cab >= 2 ** 63 else Cab) == big["Cab"]


def test_random_windows_against_unbounded_integers():
    rng = np.random.default_rng(5)
    for _ in range(20):
        a, b = rng.integers(0, 256, (2, 11, 11), dtype=np.uint8)
        big = MR.window_moments_bigint(a, b)
        got = float(MR.ssim_map(a[None, ..., None], b[None, ..., None])[0, 0, 0, 0])
        c1, c2 = MR.C1, MR.C2
        want = ((2 * big["AB"] + c1) * (2 * big["Cab"] + c2)) / ((big["AA"] + big["BB"] + c1) * (big["Va"] + big["Vb"] + c2))
        assert abs(got - want) <= 1e-12


def test_closed_forms():
    rng = np.random.default_rng(0)
    img = rng.integers(0, 256, (2, 23, 19, 3), dtype=np.uint8)
    m = MR.image_metrics(img, img.copy())
    assert (m["sad"] == 0).all() and (m["ssd"] == 0).all() and np.isposinf(m["psnr"]).all()
    assert (MR.ssim_map(img, img) == 1.0).all()                        # exactly, at every window
    assert (m["ssim"] == 1.0).all() and (m["l1"] == 0.0).all()

    for C in (1, 3):
        black, white = np.zeros((1, 14, 17, C), np.uint8), np.full((1, 14, 17, C), 255, np.uint8)
        m = MR.image_metrics(black, white)
        n = 14 * 17 * C
        assert m["sad"][0] == 255 * n and m["ssd"][0] == 65025 * n and m["l1"][0] == 1.0 and abs(m["psnr"][0]) < 1e-12
        want = MR.C1 * MR.C2 / ((65025.0 * 2.0 ** 48 + MR.C1) * MR.C2)
        assert abs(m["ssim"][0] - want) <= 4 * np.finfo(np.float64).eps * want
        assert abs(want - MR.K1 / (65025.0 + MR.K1)) < 1e-18


def _five_pairs(S=96):
    rng = np.random.default_rng(11)
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float64)
    smooth = 127.5 + 90.0 * np.sin(xx / 9.0) * np.cos(yy / 13.0)
    disk = lambda cx: np.where((xx - cx) ** 2 + (yy - S / 2) ** 2 <= (S / 4) ** 2, 220, 30)
    to_u8 = lambda v: np.clip(np.rint(v), 0, 255).astype(np.uint8)
    return {
        "uniform noise": (rng.integers(0, 256, (S, S), dtype=np.uint8), rng.integers(0, 256, (S, S), dtype=np.uint8)),
        "smooth field plus noise": (to_u8(smooth), to_u8(smooth + rng.normal(0.0, 8.0, (S, S)))),
        "a disk shifted by two pixels": (to_u8(disk(S / 2)), to_u8(disk(S / 2 + 2))),
        "all-black against all-white": (np.zeros((S, S), np.uint8), np.full((S, S), 255, np.uint8)),
        "flat 17 against flat 18": (np.full((S, S), 17, np.uint8), np.full((S, S), 18, np.uint8)),
    }


def test_against_standard_ssim():
    """The integer weights against float64 SSIM with the unquantised Gaussian on the same bytes: the mean differs by at most
    1e-3 (four times the worst value measured when the rule was chosen, 2.5e-4); a property of the definition."""
    worst = 0.0
    for name, (a, b) in _five_pairs().items():
        got = float(MR.image_metrics(a[None, ..., None], b[None, ..., None])["ssim"][0])
        want = MR.standard_ssim_mean(a, b)
        print("%-30s integer %.9f standard %.9f difference %.3g" % (name, got, want, abs(got - want)))
        worst = max(worst, abs(got - want))
        assert abs(got - want) <= 1e-3
    print("worst %.3g" % worst)


def test_quantisation():
    k = np.arange(256)
    f = (k / 255.0).astype(np.float32)                                # float32(k / 255)
    assert (MR.quantise(f) == k).all()
    assert (MR.quantise(k.astype(np.float32) / np.float32(255.0)) == k).all()     # the quotient taken in float32
    assert (np.rint(np.float32(255.0) * f) == k).all()
    assert MR.quantise(np.array([np.nan, -1.0, 2.0, np.inf, -np.inf], np.float32)).tolist() == [0, 0, 255, 255, 0]
    # half-way points round to even
    half = np.array([0.5, 1.5, 2.5, 253.5, 254.5], np.float32) / np.float32(255.0)
    prod = np.float32(255.0) * half
    exact = prod == np.array([0.5, 1.5, 2.5, 253.5, 254.5], np.float32)
    assert (MR.quantise(half)[exact] == np.array([0, 2, 2, 254, 254])[exact]).all()
    # rint is the nearest byte: a value just under a byte goes up to it, where the truncation of _save_png would lose it
    assert MR.quantise(np.array([np.nextafter(np.float32(0.5), np.float32(0))])).tolist() == [127]        # 127.49999 -> 127
    assert MR.quantise(np.array([0.7], np.float32)).tolist() == [178] and int(np.float32(255.0) * np.float32(0.7)) == 178
    assert MR.quantise(np.array([0.999], np.float32)).tolist() == [255] and int(np.float32(255.0) * np.float32(0.999)) == 254


def test_metrics_options_and_usage():
    from rendernet_amd.metrics import metrics_options
    assert metrics_options({}, ["cfg.json", "--train"]) is False
    assert metrics_options({}, ["cfg.json", "--train", "--val-metrics"]) is True
    assert metrics_options({"val_metrics": True}, ["cfg.json", "--train"]) is True
    assert metrics_options({"val_metrics": "true"}, ["cfg.json", "--train"]) is True
    assert metrics_options({"val_metrics": False}, ["cfg.json", "--train", "--val-metrics"]) is True      # the flag wins
    assert metrics_options({"val_metrics": "False"}, ["cfg.json", "--train"]) is False
    assert metrics_options({"val_metrics": True}, ["cfg.json"]) is True                                    # a shared config
    for bad in (1, 0.5, "yes", None, [True]):
        with pytest.raises(SystemExit):
            metrics_options({"val_metrics": bad}, ["cfg.json", "--train"])
    with pytest.raises(SystemExit):
        metrics_options({}, ["cfg.json", "--val-metrics"])
    import RenderNet_Shader
    import RenderNet_Texture_Face_Normal
    for script in (RenderNet_Shader, RenderNet_Texture_Face_Normal):
        with pytest.raises(SystemExit) as e:
            script.main([])
        assert "--val-metrics" in str(e.value)
        assert "--val-metrics" in script.__doc__ and "val_metrics" in script.__doc__


def test_host_derivation():
    from rendernet_amd.metrics import derive, psnr_for_mean, ValidationMetrics
    H, W, C = 20, 30, 3
    n, n_win = H * W * C, 10 * 20 * C
    l1, mse, psnr, ssim = derive([0, 255 * n, 1800], [0, 65025 * n, 3600], [n_win, 0.0, 0.25 * n_win], H, W, C)
    assert l1.dtype == mse.dtype == psnr.dtype == ssim.dtype == np.float64
    assert l1.tolist() == [0.0, 1.0, 1800 / (255.0 * n)]
    assert mse.tolist() == [0.0, 65025.0, 2.0]
    assert np.isposinf(psnr[0]) and psnr[1] == 0.0 and abs(psnr[2] - 10 * np.log10(65025 / 2.0)) < 1e-12
    assert ssim.tolist() == [1.0, 0.0, 0.25]
    m = psnr_for_mean(psnr, n)
    assert abs(m[0] - 10 * np.log10(65025.0 * n / 0.5)) < 1e-12 and (m[1:] == psnr[1:]).all()
    assert m[0] > 10 * np.log10(65025.0 * n / 1.0)                    # above the best PSNR a differing pair can have
    # the twin derives the same values
    rng = np.random.default_rng(2)
    a, b = rng.integers(0, 256, (2, 2, H, W, C), dtype=np.uint8)
    t = MR.image_metrics(a, b)
    l1, mse, psnr, ssim = derive(t["sad"], t["ssd"], t["ssim_sum"], H, W, C)
    assert (l1 == t["l1"]).all() and (psnr == t["psnr"]).all() and (ssim == t["ssim"]).all()
    with pytest.raises(ValueError):
        ValidationMetrics().line()


def test_ops_image_metrics_refuses_cpu_tensors():
    import torch
    from rendernet_amd import ops
    from rendernet_amd._lib import RenderNetHipError
    with pytest.raises(RenderNetHipError, match="HIP tensors"):
        ops.image_metrics(torch.zeros(1, 16, 16, 3), torch.zeros(1, 16, 16, 3, dtype=torch.uint8))
    with pytest.raises(RenderNetHipError, match="expected a uint8 or float32 tensor"):
        ops.image_metrics(np.zeros((1, 16, 16, 3), np.uint8), torch.zeros(1, 16, 16, 3))


def test_workspace_helper_is_host_code():
    """rn_image_metrics_workspace_bytes: 24 bytes per tile of 16 rows x 64 samples of the valid region; 0 for a refused shape.
    rn_image_metrics checks its arguments before any launch, so the refusals run without a device."""
    import ctypes
    from rendernet_amd import _lib
    L = _lib.lib()
    assert L.rn_image_metrics_workspace_bytes(24, 512, 512, 3) == 24 * 32 * 24 * 24
    assert L.rn_image_metrics_workspace_bytes(1, 11, 11, 1) == 24
    assert L.rn_image_metrics_workspace_bytes(2, 27, 139, 1) == 2 * 2 * 3 * 24
    assert L.rn_image_metrics_workspace_bytes(1, 10, 64, 3) == 0 and b"11 x 11" in L.rn_last_error()
    assert L.rn_image_metrics_workspace_bytes(1, 64, 64, 2) == 0 and b"C=2" in L.rn_last_error()
    buf = (ctypes.c_longlong * 64)()
    p = ctypes.addressof(buf)
    vp = ctypes.c_void_p
    call = lambda H, W, C, ws, nws, da=0: L.rn_image_metrics(vp(p), da, vp(p), 0, 1, H, W, C, vp(p), vp(p), vp(p), vp(ws), nws, None)
    assert call(10, 64, 3, p, 512) == -1 and b"11 x 11" in L.rn_last_error()
    assert call(64, 64, 2, p, 512) == -1 and b"C=2" in L.rn_last_error()
    assert call(64, 64, 3, p + 4, 512) == -1 and b"aligned" in L.rn_last_error()
    assert call(64, 64, 3, p, 24 * 4 * 3 - 1) == -1 and b"needed" in L.rn_last_error()
    assert call(64, 64, 3, p, 512, da=7) == -1 and b"dtypes" in L.rn_last_error()
