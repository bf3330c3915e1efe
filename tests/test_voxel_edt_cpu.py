"""The NumPy twin of rn_voxel_edt / rn_voxel_shape_metrics (tests/voxel_edt_ref.py) against the definition it stands for: a
brute-force minimum over every seed, scipy's transform where scipy is present, closed forms, the integer square root, the metric
identities; and the argument checks of the C entries, which run before any launch and so need no device."""
import ctypes
import math

import numpy as np
import pytest

import voxel_edt_ref as R


@pytest.fixture(scope="module")
def chair():
    return R.load_binvox("chair")


@pytest.mark.parametrize("seeds", ["solid", "empty", "surface"])
def test_twin_equals_the_minimum_over_every_seed(chair, seeds):
    small = chair[::2, ::2, ::2]
    assert small.shape == (32, 32, 32) and 500 < small.sum() < 1000
    assert np.array_equal(R.edt(small, seeds), R.brute(small, seeds))
    sparse = np.random.default_rng(7).random((16, 16, 16)) < 0.02
    assert 40 < sparse.sum() < 160
    assert np.array_equal(R.edt(sparse, seeds), R.brute(sparse, seeds))
    dense = ~sparse                                               # the EMPTY rule with most seeds outside the grid
    assert np.array_equal(R.edt(dense, seeds), R.brute(dense, seeds))


def test_twin_equals_scipy_on_the_chair(chair):
    ndi = pytest.importorskip("scipy.ndimage")
    for seeds, field in (("solid", ndi.distance_transform_edt(~chair)),
                         ("empty", ndi.distance_transform_edt(np.pad(chair, 1))[1:-1, 1:-1, 1:-1]),
                         ("surface", ndi.distance_transform_edt(~R.surface(chair)))):
        sq = field.astype(np.float64) ** 2
        assert np.abs(sq - np.rint(sq)).max() < 1e-9
        assert np.array_equal(R.edt(chair, seeds), np.rint(sq).astype(np.int32)), seeds


def test_closed_forms(chair):
    S = 16
    z, y, x = np.meshgrid(np.arange(S), np.arange(S), np.arange(S), indexing="ij")
    lone = np.zeros((S, S, S), bool)
    lone[3, 15, 8] = True
    want = (z - 3) ** 2 + (y - 15) ** 2 + (x - 8) ** 2
    assert np.array_equal(R.edt(lone, "solid"), want) and np.array_equal(R.edt(lone, "surface"), want)
    assert np.array_equal(R.edt(lone, "signed"), want - lone)    # D_EMPTY of the lone voxel is 1
    full = np.ones((S, S, S), bool)
    border = np.minimum(np.minimum(np.minimum(z + 1, S - z), np.minimum(y + 1, S - y)), np.minimum(x + 1, S - x)) ** 2
    assert np.array_equal(R.edt(full, "empty"), border) and np.array_equal(R.edt(full, "signed"), -border)
    assert np.array_equal(R.edt(full, "solid"), np.zeros_like(border))
    empty = np.zeros((S, S, S), bool)
    for seeds in ("solid", "surface", "signed"):
        assert (R.edt(empty, seeds) == R.NONE).all(), seeds
    assert (R.edt(empty, "empty") == 0).all()
    for grid in (chair, full, lone):
        assert np.array_equal(R.surface(grid), grid & (R.edt(grid, "empty") == 1))
    signed = R.edt(chair, "signed")
    assert (signed[chair] < 0).all() and (signed[~chair] > 0).all()
    assert ((R.edt(chair, "solid") == 0) ^ (R.edt(chair, "empty") == 0)).all()


def test_q_is_the_integer_square_root():
    for D in range(0, 3 * 127 ** 2 + 1):
        q = R.q_of(D)
        assert q * q <= 65536 * D < (q + 1) * (q + 1)
    assert R.q_of(1) == 256 and R.q_of(2) == 362 and R.q_of(3 * 127 ** 2) == 56312


def test_metric_closed_forms(chair):
    w = R.shape_words(chair, chair, 1)
    d = R.derived(w)
    assert w[0] == w[1] == w[2] == w[3] == chair.sum() and w[4] == w[5] == R.surface(chair).sum()
    assert not w[6:12].any() and w[12] == w[4] and w[13] == w[5] and not w[14:].any()
    assert d["iou"] == d["dice"] == d["fscore"] == d["precision"] == d["recall"] == 1.0
    assert d["chamfer"] == d["chamfer_sq"] == d["hausdorff"] == 0.0
    # a copy shifted by (2, 1, 0) that loses nothing has every surface voxel's copy |(2, 1, 0)|^2 = 5 away.  The chair reaches the
    # last ys layer (its zs layers 0..16 and 47..63 are empty), so that one layer is cleared first.
    chair = chair.copy()
    chair[:, -1] = False
    assert not chair[-2:].any() and not chair[:, -1:].any()
    shifted = np.roll(chair, (2, 1, 0), (0, 1, 2))
    w = R.shape_words(chair, shifted, 6)
    assert w[4] == w[5] and 0 < w[10] <= 5 and 0 < w[11] <= 5 and w[12] == w[4] and w[13] == w[5]
    assert 0 < R.derived(w)["iou"] < 1 and R.derived(w)["hausdorff"] <= math.sqrt(5)
    # tau2 is a threshold on the integer D
    assert R.shape_words(chair, shifted, 0)[12] < w[12]
    nothing = np.zeros_like(chair)
    for pair in ((chair, nothing), (nothing, chair)):
        w = R.shape_words(*pair)
        d = R.derived(w)
        assert not w[6:].any() and w[3] == chair.sum() and w[2] == 0
        assert d["iou"] == 0.0 and d["dice"] == 0.0 and math.isnan(d["chamfer"]) and math.isnan(d["hausdorff"]) and math.isnan(d["fscore"])
    w = R.shape_words(nothing, nothing)
    assert not w.any() and R.derived(w)["iou"] == 1.0 and R.derived(w)["dice"] == 1.0 and math.isnan(R.derived(w)["chamfer"])


def test_pack_is_the_bit_order_of_the_header():
    occ = np.zeros((1, 32, 32, 32), bool)
    occ[0, 1, 2, 3] = occ[0, 0, 0, 31] = True
    bits = R.pack(occ).view(np.uint32)
    i = (1 * 32 + 2) * 32 + 3
    assert bits[0, i >> 5] == 1 << (i & 31) and bits[0, 0] == 1 << 31 and int((bits != 0).sum()) == 2


def test_workspace_sizes_and_refusals_without_a_device():
    """rn_voxel_edt and rn_voxel_shape_metrics check every argument before any launch."""
    from rendernet_amd import _lib as L
    lib = L.lib()
    assert lib.rn_voxel_edt_workspace_bytes(24, 64, L.RN_EDT_SIGNED) == 24 * 64 ** 3 * 2
    assert lib.rn_voxel_edt_workspace_bytes(1, 128, L.RN_EDT_SOLID) == 128 ** 3 * 2
    assert lib.rn_voxel_shape_metrics_workspace_bytes(3, 32) == 3 * 32 ** 3 * 4
    assert lib.rn_voxel_edt_workspace_bytes(1, 48, 0) == 0 and b"S=48" in lib.rn_last_error()
    assert lib.rn_voxel_edt_workspace_bytes(1, 64, 4) == 0 and b"seeds=4" in lib.rn_last_error()
    assert lib.rn_voxel_edt_workspace_bytes(65536, 64, 0) == 0 and b"B=65536" in lib.rn_last_error()
    assert lib.rn_voxel_shape_metrics_workspace_bytes(-1, 64) == 0 and b"B=-1" in lib.rn_last_error()
    buf = (ctypes.c_char * 64)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    odd = ctypes.c_void_p(p.value + 4)
    big = 1 << 40
    edt = lambda B=1, S=32, seeds=0, bits=p, out=p, ws=p, n=big: lib.rn_voxel_edt(bits, B, S, seeds, out, ws, n, None)
    for kw, text in ((dict(S=48), b"S=48"), (dict(S=256), b"S=256"), (dict(B=-1), b"B=-1"), (dict(B=65536), b"B=65536"),
                     (dict(seeds=-1), b"seeds=-1"), (dict(seeds=4), b"seeds=4"), (dict(bits=None), b"null"), (dict(out=None), b"null"),
                     (dict(ws=None), b"null"), (dict(ws=odd), b"16-byte"), (dict(bits=odd), b"16-byte"), (dict(n=65535), b"65536 needed")):
        assert edt(**kw) == -1 and b"rn_voxel_edt:" in lib.rn_last_error() and text in lib.rn_last_error(), (kw, lib.rn_last_error())
    sm = lambda B=1, S=32, tau2=1, a=p, b=p, out=p, ws=p, n=big: lib.rn_voxel_shape_metrics(a, b, B, S, tau2, out, ws, n, None)
    for kw, text in ((dict(S=96), b"S=96"), (dict(B=70000), b"B=70000"), (dict(tau2=-1), b"tau2=-1"), (dict(a=None), b"null"),
                     (dict(b=None), b"null"), (dict(out=None), b"null"), (dict(out=odd), b"8-byte"), (dict(ws=odd), b"16-byte"),
                     (dict(n=131071), b"131072 needed")):
        assert sm(**kw) == -1 and b"rn_voxel_shape_metrics:" in lib.rn_last_error() and text in lib.rn_last_error(), (kw, lib.rn_last_error())
    assert edt(B=0, bits=None, out=None, ws=None, n=0) == 0 and sm(B=0, a=None, b=None, out=None, ws=None, n=0) == 0


def test_ops_refuse_host_tensors_and_bad_arguments():
    import torch
    from rendernet_amd import ops
    from rendernet_amd._lib import RenderNetHipError
    g = torch.zeros((1, 32, 32, 32, 1))
    for call in (lambda: ops.voxel_edt(g), lambda: ops.voxel_shape_metrics(g, g), lambda: ops.voxel_offset(g, 1.0),
                 lambda: ops.voxel_edt(g, seeds="hollow"), lambda: ops.voxel_edt(), lambda: ops.voxel_shape_metrics(g, g, tau=-1.0),
                 lambda: ops.voxel_offset(g, float("nan"))):
        with pytest.raises(RenderNetHipError):
            call()
