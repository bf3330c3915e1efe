"""Pins tests/resample_grad_ref.py -- the float64 autograd reference of the resampler gradients -- before the GPU tests rely on it,
and checks, from the reference alone, the conditions the GPU case table must meet.  No GPU."""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_grad_ref as R  # noqa: E402
from oracle import resample as OR  # noqa: E402
import test_oracle_resample_bwd as TO  # noqa: E402  (its float64 NumPy forward and its smooth problem)


@functools.lru_cache(maxsize=None)
def _case(name):
    o = R.case(name)
    return o, R.reference(o)


@pytest.mark.parametrize("name", R.CASES)
def test_reference_agrees_with_the_hand_derived_oracle(name):
    """oracle.resample.resampling_affine_bwd writes the gradient formulas by hand with float32 coordinates inside the weights; the
    autograd reference differs from it by that rounding only: <= 1e-5 * max|ref| per item (measured 7e-7 ... 4e-6), and not at all on
    the lattice view, where every coordinate is an integer (dM: two float64 sums in different orders, <= 1e-14)."""
    o, g = _case(name)
    dv, dM = OR.resampling_affine_bwd(o["vox"], o["M32"], R.raw_dout(o["dout"], o["N"], o["layout"], o["window"]), o["N"])
    rv, rm = R.ratios(dv, g["dvox"]), R.ratios(dM, g["dM"])
    print("%s: dvox %s  dM %s" % (name, rv, rm))
    if name == "lattice":
        assert np.array_equal(dv, g["dvox"]) and rm.max() <= 1e-14
    elif name in R.DEGENERATE:
        # nothing active: the reference is exactly zero; so is the oracle's dM, and its dvox is the float64 rounding noise left by
        # cancelling +w and -w terms of size ~90^3 |dout| on the border voxels
        assert not g["dvox"].any() and not g["dM"].any() and not dM.any()
        assert np.abs(dv).max() <= 2.0 ** -52 * 8 * o["N"] ** 3 * 106.0 ** 3 * np.abs(o["dout"]).max()
    else:
        assert rv.max() <= 1e-5 and rm.max() <= 1e-5


def _smooth_problem():
    """The problem of tests/test_oracle_resample_bwd.py: S=8, N=16, C=2, empty border (the sampler is continuous), samples off the cell
    boundaries."""
    vox, _, M, dout, S, N = TO._problem()
    return vox, M, dout, S, N


def _loss(vox64, M64, dout, N):
    """That file's NumPy float64 forward: taps from the float64 coordinates of the matrix it is given, nothing shared with R.forward."""
    return float(np.sum(TO._f64_forward(vox64[0], M64[0], N) * dout[0].reshape(-1, dout.shape[4]).astype(np.float64)))


def test_reference_matches_central_differences():
    """dM against central differences of the float64 forward at the bar of test_oracle_resample_bwd.py (2e-3 relative + 1e-3), dvox
    through the adjoint identity <J e, dout> = <e, dvox> (exact here: the forward is linear in the voxels and both sides are float64)."""
    vox, M, dout, S, N = _smooth_problem()
    g = R.gradients(vox, dout, N, M32=M)
    M64, v64 = M.astype(np.float64), vox.astype(np.float64)
    for r, c in [(0, 0), (0, 3), (1, 1), (1, 2), (2, 0), (2, 3)]:
        h = 1e-7
        Mp, Mm = M64.copy(), M64.copy()
        Mp[0, r, c] += h
        Mm[0, r, c] -= h
        fd = (_loss(v64, Mp, dout, N) - _loss(v64, Mm, dout, N)) / (2 * h)
        assert abs(fd - g["dM"][0, r, c]) <= 2e-3 * max(abs(fd), abs(g["dM"][0, r, c])) + 1e-3, (r, c, fd, g["dM"][0, r, c])
    rng = np.random.default_rng(1)
    for _ in range(3):
        e = rng.standard_normal(vox.shape)
        lhs = _loss(v64 + e, M64, dout, N) - _loss(v64, M64, dout, N)
        assert abs(lhs - np.sum(e * g["dvox"])) <= 1e-9 * abs(lhs) + 1e-9


def test_reference_pose_gradient_matches_central_differences():
    """dpose (autograd through pose_to_minv) against central differences of the whole float64 chain pose -> matrix -> forward, on the
    smooth problem, at the same bar."""
    vox, _, dout, S, N = _smooth_problem()
    pose = np.array([[1.0, 0.6, 0.9]], np.float32)
    g = R.gradients(vox, dout, N, pose=pose)
    v64 = vox.astype(np.float64)

    def loss(p):
        M64 = R.pose_to_minv(torch.as_tensor(p), S, N).numpy()
        return _loss(v64, M64, dout, N)
    for k in range(3):
        h = 1e-7
        pp, pm = pose.astype(np.float64), pose.astype(np.float64)
        pp[0, k] += h
        pm[0, k] -= h
        fd = (loss(pp) - loss(pm)) / (2 * h)
        assert abs(fd - g["dpose"][0, k]) <= 2e-3 * max(abs(fd), abs(g["dpose"][0, k])) + 1e-3, (k, fd, g["dpose"][0, k])


@pytest.mark.parametrize("window", [None, R.WINDOW])
def test_image_layout_and_window_mapping(window):
    """to_window against oracle.resample.transform_voxel_to_match_image plus a crop, on a grid whose every entry is distinct; and the
    float64 forward against the float32 oracle forward in that layout."""
    N = 16
    raw = np.arange(N * N * N * 2, dtype=np.float64).reshape(1, N, N, N, 2)
    want = OR.transform_voxel_to_match_image(raw)
    h0, w0, ph, pw = window or (0, 0, N, N)
    want = want[:, h0:h0 + ph, w0:w0 + pw]
    got = R.to_window(torch.as_tensor(raw[0]), "image", window).numpy()
    assert np.array_equal(got, want[0])
    assert np.array_equal(R.to_window(torch.as_tensor(raw[0]), "raw", None).numpy(), raw[0])
    # raw_dout is its adjoint: <to_window(x), d> = <x, raw_dout(d)>
    d = np.random.default_rng(0).standard_normal((1, ph, pw, N, 2))
    assert np.isclose(np.sum(want * d), np.sum(raw * R.raw_dout(d, N, "image", window)), rtol=1e-12)
    o, g = _case("window_b3" if window else "dense_borders")
    f32 = OR.transform_voxel_to_match_image(OR.resampling_affine(o["vox"], o["M32"], o["N"], mode="ordered"))
    if o["window"]:
        f32 = f32[:, h0:h0 + ph, w0:w0 + pw]
    assert np.abs(g["out"] - f32).max() <= 1e-5 * np.abs(f32).max()


@pytest.mark.parametrize("S,N", [(8, 16), (8, 32), (64, 128)])
def test_pose_chain_matches_the_float64_oracle(S, N):
    pose = np.concatenate([R.JACOBIAN_POSES, np.array(R.POSES, np.float32)])
    got = R.pose_to_minv(torch.as_tensor(pose).double(), S, N).numpy()
    want = OR.inverse_affine_f64(pose, S, N)
    assert np.abs(got - want).max() <= 1e-11 * np.abs(want).max()       # the oracle inverts numerically (scale 0.2: entries up to 5 N/2)
    # and its Jacobian against central differences of the oracle's chain
    J = R.pose_jacobian(pose, S, N)
    for k in range(3):
        h = 1e-6
        pp, pm = pose.astype(np.float64), pose.astype(np.float64)
        pp[:, k] += h
        pm[:, k] -= h
        fd = (OR.inverse_affine_f64(pp, S, N) - OR.inverse_affine_f64(pm, S, N)) / (2 * h)
        assert np.abs(J[..., k] - fd).max() <= 1e-6 * max(1.0, np.abs(fd).max())


@pytest.mark.parametrize("name", R.CASES)
def test_conditions_of_the_gpu_table(name):
    """Every item of every non-degenerate case has >= 2 % of its window's samples and >= 20 samples active, and non-zero reference
    dvox, dM (and dpose where the case has poses); the off-side case has none active."""
    o, g = _case(name)
    ph, pw = (o["window"][2], o["window"][3]) if o["window"] else (o["N"], o["N"])
    total = ph * pw * o["N"]
    print("%s: active %s of %d = %s" % (name, g["active"], total, np.round(g["active"] / total, 3)))
    assert g["active"].shape == (o["B"],)
    if name in R.DEGENERATE:
        assert not g["active"].any() and not g["dvox"].any() and not g["dM"].any()
        return
    assert (g["active"] >= 20).all() and (g["active"] >= 0.02 * total).all()
    assert (np.abs(g["dvox"]).reshape(o["B"], -1).max(1) > 0).all()
    assert (np.abs(g["dM"]).reshape(o["B"], -1).max(1) > 0).all()
    if o["pose"] is not None:
        assert (np.abs(g["dpose"]) > 0).all()
        assert np.array_equal(g["M32"], o["M32"])


def test_block_structure_of_the_windows():
    """The tails the table is there for: samples per item that are no multiple of the 256-thread block, odd block counts, B = 3."""
    s = R.WINDOW[2] * R.WINDOW[3] * 16
    assert (s, s // 256, s % 256) == (560, 2, 48)
    s = R.WINDOW_BIG[2] * R.WINDOW_BIG[3] * 32
    assert (s, s // 256, s % 256) == (25920, 101, 64)
    assert R.WINDOW_BIG[0] + R.WINDOW_BIG[2] <= 32 and R.WINDOW_BIG[1] + R.WINDOW_BIG[3] <= 32
    assert R.case("raw_b3")["B"] == 3 and R.case("window_b3")["B"] == 3


def test_jacobian_case_covers_the_pose_edges():
    p = R.JACOBIAN_POSES
    assert (p[:, 1] == 0).any() and (p[:, 1] < 0).any() and (p[:, 0] == np.float32(np.pi / 2)).any()
    assert {int(a // (np.pi / 2)) for a in p[:, 0]} == {0, 1, 2, 3}
    assert np.float32(0.2) in p[:, 2] and np.float32(3.0) in p[:, 2]
    pose, dm, terms = R.jacobian_case(130, 8, 32)
    assert pose.shape == (130, 3) and dm.shape == (130, 12) and terms.shape == (130, 12, 3)
    scale = np.abs(dm).max(1)
    assert scale.min() < 30 and scale.max() > 300
