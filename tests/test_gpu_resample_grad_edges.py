"""The resampler backward (csrc/resample_bwd.hip) at its edges, against the float64 autograd reference of tests/resample_grad_ref.py
(pinned on the CPU by tests/test_resample_grad_ref_cpu.py).  -m gpu.

C-level cases go through rendernet_amd._lib with every output buffer pre-filled with 0.25 -- the kernels accumulate -- and `got - 0.25` is
compared with the reference per batch item: dvox <= 1e-4 * max|ref|, dM <= 2e-4 * max|ref|, no absolute floor; voxels the reference leaves
at exactly 0 must still hold the bits of 0.25.  The cases: an odd item count, windows whose sample count is no multiple of the 256-thread
block (3 blocks with 48 live threads in the last; 101 blocks + 64 threads), null outputs, the lattice view, a volume wholly off one side,
a dense volume with occupied borders and a zeroed dout channel, the atomic pile-up of a zoomed-in pose, the strided concat form with dM
accumulated over its two calls, and rn_pose_to_affine_bwd alone over several blocks and pose edges.  The ops-level cases check which
inputs get a gradient (and None otherwise) in every form of ops.resample / ops.resample_concat, and the argument checks.

Atomics make dvox and dM differ from run to run: nothing here asserts bit-equality between launches, only to the pre-fill where the
reference is exactly zero.  Every test prints the ratios it measured.
"""
import functools
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import resample_grad_ref as R  # noqa: E402

pytestmark = pytest.mark.gpu
FILL = 0.25
FILL_BITS = np.float32(FILL).view(np.uint32)


def _dev(a):
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _filled(*shape):
    return torch.full(shape, FILL, dtype=torch.float32, device="cuda")


@functools.lru_cache(maxsize=None)
def _case(name):
    """Operands and reference of a table case: computed once, shared, never written to."""
    o = R.case(name)
    return o, R.reference(o)


def _window(o):
    return o["window"] or (0, 0, o["N"], o["N"])


def _bwd(o, want_dvox=True, want_dm=True, vox=None, dout=None, channels=None, dvox=None, dm=None):
    """One rn_resample_affine_bwd (or, with channels = (dout_channels, offset), rn_resample_affine_bwd_strided) launch on pre-filled buffers."""
    from rendernet_amd import _lib as L
    vox = o["vox"] if vox is None else vox
    B, S, N, C = o["B"], o["S"], o["N"], vox.shape[4]
    h0, w0, ph, pw = _window(o)
    vd = _dev(vox) if want_dm else None                                    # vox is needed for the matrix gradient only
    md, dd = _dev(o["M32"].reshape(B, 12)), _dev(o["dout"] if dout is None else dout)
    if want_dvox and dvox is None:
        dvox = _filled(B, S, S, S, C)
    if want_dm and dm is None:
        dm = _filled(B, 12)
    tail = (B, S, N, C, h0, w0, ph, pw, 1 if o["layout"] == "image" else 0, L.stream_ptr())
    if channels is None:
        L.check(L.lib().rn_resample_affine_bwd(L.ptr(vd), L.ptr(md), L.ptr(dd), L.ptr(dvox), L.ptr(dm), *tail), "rn_resample_affine_bwd")
    else:
        L.check(L.lib().rn_resample_affine_bwd_strided(L.ptr(vd), L.ptr(md), L.ptr(dd), channels[0], channels[1], L.ptr(dvox), L.ptr(dm),
                                                       *tail), "rn_resample_affine_bwd_strided")
    torch.cuda.synchronize()
    return dvox, dm


def _check_dvox(got, ref, log, what="dvox"):
    got = got.cpu().numpy()
    untouched = ref == 0
    assert np.all(got[untouched].view(np.uint32) == FILL_BITS), "%s: a voxel the reference leaves at 0 no longer holds the pre-fill" % what
    r = R.ratios(got.astype(np.float64) - FILL, ref)
    log.append("%s %s" % (what, " ".join("%.2e" % v for v in r)))
    assert r.max() <= R.RTOL_DVOX, "%s: max|got - ref| / max|ref| per item = %s > %g" % (what, r, R.RTOL_DVOX)


def _check_dm(got, ref, log):
    r = R.ratios(got.cpu().numpy().astype(np.float64).reshape(-1, 3, 4) - FILL, ref)
    log.append("dM %s" % " ".join("%.2e" % v for v in r))
    assert r.max() <= R.RTOL_DM, "dM: max|got - ref| / max|ref| per item = %s > %g" % (r, R.RTOL_DM)


@pytest.mark.parametrize("name", ["raw_b3", "window_b3", "window_big", "lattice", "dense_borders"])
def test_backward_on_prefilled_buffers(name):
    """raw_b3: three items, three different poses.  window_b3: 560 samples per item = 3 blocks, the last with 48 live threads, so the item
    of a block is blockIdx / 3 and one wave and a quarter of the block's reduction is idle.  window_big: 25 920 samples = 101 blocks + 64
    threads.  lattice: M = [I | -S/2], every coordinate an integer, plane S-1 clamps onto itself.  dense_borders: N(0,1) in every voxel,
    border included (the skipped samples' +w / -w do not cancel against zeros there), and one dout channel all zero (`d == 0`)."""
    o, g = _case(name)
    dvox, dm = _bwd(o)
    log = []
    _check_dvox(dvox, g["dvox"], log)
    _check_dm(dm, g["dM"], log)
    print("%s: %s" % (name, "  ".join(log)))


def test_null_outputs_give_the_halves_of_the_full_call():
    """dvox alone (vox and dm null), then dm alone (dvox null): each is the corresponding half of the full call's reference."""
    o, g = _case("raw_b3")
    log = []
    dvox, none = _bwd(o, want_dm=False)
    assert none is None
    _check_dvox(dvox, g["dvox"], log)
    none, dm = _bwd(o, want_dvox=False)
    assert none is None
    _check_dm(dm, g["dM"], log)
    print("null outputs: %s" % "  ".join(log))


def test_volume_off_one_side_touches_nothing():
    """Matrix column 3 moved by +90: every sample clamps both taps of an axis onto one plane and is skipped.  dvox and dm keep the bits
    of their pre-fill, and the zero matrix gradient leaves a pre-filled dpose alone."""
    from rendernet_amd import _lib as L
    o, g = _case("off_side")
    assert not g["active"].any()
    dvox, dm = _bwd(o)
    assert np.all(dvox.cpu().numpy().view(np.uint32) == FILL_BITS) and np.all(dm.cpu().numpy().view(np.uint32) == FILL_BITS)
    dpose, pose, zero = _filled(o["B"], 3), _dev(np.array(R.POSES, np.float32)), dm - FILL
    assert not zero.any()
    L.check(L.lib().rn_pose_to_affine_bwd(L.ptr(pose), L.ptr(zero), L.ptr(dpose), o["B"], o["S"], o["N"], L.stream_ptr()), "rn_pose_to_affine_bwd")
    assert np.all(dpose.cpu().numpy().view(np.uint32) == FILL_BITS)
    print("off one side: dvox, dM, dpose bit-equal to the pre-fill")


def test_atomic_pile_up_of_a_zoomed_in_pose():
    """S=8, N=32, scale 3.0: 9 212 active samples land on 8^3 voxels, 8 atomics each per channel -- up to 224 (on average 144) float32
    adds per gradient entry in an arbitrary order, on top of a pre-fill.  Measured on the MI355X: dvox 6.9e-7 * max|ref|, dM 3.8e-7 *
    max|ref|, i.e. the project's bars hold as they stand and the case is NOT rescaled by sum|w * dout|.  The same error against that sum,
    the natural scale of a reordered float32 sum, is printed next to it (8.9e-5: the half-ulp of the 0.25 pre-fill, 1.5e-8, on an entry
    whose few terms are of size 1e-4)."""
    o, g = _case("pile_up")
    dvox, dm = _bwd(o)
    log = []
    _check_dvox(dvox, g["dvox"], log)
    _check_dm(dm, g["dM"], log)
    sums = R.abs_terms(o)
    err = np.abs(dvox.cpu().numpy().astype(np.float64) - FILL - g["dvox"])
    log.append("dvox / sum|w dout| %.2e (adds per entry: max %d)" % ((err / np.maximum(sums["abs"], 1e-300)).max(), sums["count"].max()))
    print("pile_up: %s" % "  ".join(log))


@pytest.mark.parametrize("name", ["concat_full", "concat_window"])
def test_strided_concat_backward_against_the_concatenated_volume(name):
    """rn_resample_affine_bwd_strided once per source (Ca = 1 at channel 0, Cb = 4 at channel 1 of a 5-channel dout, so the second call
    has dout_offset != 0), dm pre-filled once and accumulated over the two calls: equal to the reference on the channel-concatenated
    volume, on the full grid and in the (5,4,7,5) window."""
    o, g = _case(name)
    ca, cb = R.CONCAT_SPLIT
    va, vb = np.ascontiguousarray(o["vox"][..., :ca]), np.ascontiguousarray(o["vox"][..., ca:])
    da, dm = _bwd(o, vox=va, channels=(ca + cb, 0))
    db, dm = _bwd(o, vox=vb, channels=(ca + cb, ca), dm=dm)
    log = []
    _check_dvox(da, g["dvox"][..., :ca], log, "dvox_a")
    _check_dvox(db, g["dvox"][..., ca:], log, "dvox_b")
    _check_dm(dm, g["dM"], log)
    print("%s: %s" % (name, "  ".join(log)))


@pytest.mark.parametrize("S,N", R.JACOBIAN_SIZES)
@pytest.mark.parametrize("B", R.JACOBIAN_BATCHES)
def test_pose_jacobian_alone(B, S, N):
    """rn_pose_to_affine_bwd on a pre-filled dpose: one thread per item in blocks of 64 (B = 65, 130 reach the second and third block),
    poses cycling through elevation 0, a negative elevation, azimuth float32(pi/2), every quadrant, scales 0.2 and 3.0; dm = N(0,1) times
    a per-item scale in [1, 1e3].  The kernel sums in double, rounds once and adds in float:
    |got - (fill + g)| <= 2^-22 (|fill| + |g|) + 1e-12 * sum|terms| per entry, terms = dm_rc * dM_rc/dp_k from the float64 autograd chain."""
    from rendernet_amd import _lib as L
    pose, dm, terms = R.jacobian_case(B, S, N)
    dpose, pd, dd = _filled(B, 3), _dev(pose), _dev(dm)              # named: a temporary's memory would be handed to the next allocation
    L.check(L.lib().rn_pose_to_affine_bwd(L.ptr(pd), L.ptr(dd), L.ptr(dpose), B, S, N, L.stream_ptr()), "rn_pose_to_affine_bwd")
    got = dpose.cpu().numpy().astype(np.float64)
    g = terms.sum(1)
    bound = 2.0 ** -22 * (FILL + np.abs(g)) + 1e-12 * np.abs(terms).sum(1)
    r = np.abs(got - (FILL + g)) / bound
    print("pose Jacobian B=%d S=%d N=%d: max error / bound %.3f (max|g| %.3g)" % (B, S, N, r.max(), np.abs(g).max()))
    assert r.max() <= 1.0, "item %d: %s" % (int(np.argmax(r.max(1))), r.max(1))


# ---------------------------------------------------------------------------------------------
# ops-level autograd

OPS_WINDOW = (11, 5, 10, 16)       # odd offsets, rows no multiple of 8; 10 * 16 pixels are whole blocks of the forward at N = 32, which it needs


@functools.lru_cache(maxsize=None)
def _ops_problem(layout):
    rng = np.random.default_rng(7)
    B, S, N, C = (3, 16, 32, 2) if layout == "image" else (3, 8, 16, 2)
    window = OPS_WINDOW if layout == "image" else None
    ph, pw = (window[2], window[3]) if window else (N, N)
    vox = (rng.random((B, S, S, S, C)) * (rng.random((B, S, S, S, 1)) < 0.4)).astype(np.float32)
    pose = np.array(R.POSES, np.float32)
    dout = rng.standard_normal((B, ph, pw, N, C)).astype(np.float32)
    g = R.gradients(vox, dout, N, pose=pose, layout=layout, window=window)
    assert (g["active"] >= 20).all() and (g["active"] >= 0.02 * ph * pw * N).all()
    return dict(B=B, S=S, N=N, C=C, window=window, vox=vox, pose=pose, dout=dout, J=R.pose_jacobian(pose, S, N)), g


def _check_grad(what, got, ref, rtol, log):
    r = R.ratios(got.detach().cpu().numpy().astype(np.float64), ref)
    log.append("%s %.2e" % (what, r.max()))
    assert r.max() <= rtol, "%s: per item %s > %g" % (what, r, rtol)


def _check_dpose(got, g, J, log):
    """The dM bar carried through the Jacobian: |got_k - ref_k| <= 2e-4 * max|dM_ref| * sum_rc |dM_rc/dp_k| per item and pose entry."""
    B = len(J)
    bound = R.RTOL_DM * np.abs(g["dM"]).reshape(B, -1).max(1)[:, None] * np.abs(J).reshape(B, 12, 3).sum(1)
    r = np.abs(got.detach().cpu().numpy().astype(np.float64) - g["dpose"]) / bound
    log.append("dpose/bound %.2e" % r.max())
    assert r.max() <= 1.0, "dpose: error / bound per item and entry %s" % r


@pytest.mark.parametrize("layout", ["raw", "image"])
@pytest.mark.parametrize("form", ["pose", "affine34", "affine12"])
def test_ops_resample_gradients_for_whichever_input_asks(form, layout):
    """ops.resample with requires_grad on the voxels only, the pose (or matrix) only, and both: the asked-for gradients match the
    reference, the matrix gradient comes back in the matrix's own shape, and an input that does not ask gets None."""
    from rendernet_amd import ops
    o, g = _ops_problem(layout)
    second = {"pose": o["pose"], "affine34": g["M32"], "affine12": g["M32"].reshape(o["B"], 12)}[form]
    log = []
    for want_vox, want_second in ((True, False), (False, True), (True, True)):
        v = _dev(o["vox"]).requires_grad_(want_vox)
        p = _dev(second).requires_grad_(want_second)
        out = ops.resample(v, p, o["N"], o["window"], image_layout=(layout == "image"), affine=(form != "pose"))
        out.backward(_dev(o["dout"]))
        assert (v.grad is not None) == want_vox and (p.grad is not None) == want_second
        if want_vox:
            _check_grad("dvox", v.grad, g["dvox"], R.RTOL_DVOX, log)
        if want_second and form == "pose":
            _check_dpose(p.grad, g, o["J"], log)
        elif want_second:
            assert p.grad.shape == p.shape
            _check_grad("dM", p.grad.reshape(o["B"], 3, 4), g["dM"], R.RTOL_DM, log)
    print("ops.resample %s %s: %s" % (form, layout, "  ".join(log)))


def test_ops_resample_concat_gradients_for_whichever_input_asks():
    """ops.resample_concat with requires_grad on source a only, source b only, the pose only, and all three, against the reference on
    the channel-concatenated volume."""
    from rendernet_amd import ops
    o, g = _case("concat_full")
    ca, _ = R.CONCAT_SPLIT
    va, vb = np.ascontiguousarray(o["vox"][..., :ca]), np.ascontiguousarray(o["vox"][..., ca:])
    J = R.pose_jacobian(o["pose"], o["S"], o["N"])
    log = []
    for wants in ((True, False, False), (False, True, False), (False, False, True), (True, True, True)):
        a, b, p = (_dev(x).requires_grad_(w) for x, w in zip((va, vb, o["pose"]), wants))
        ops.resample_concat(a, b, p, o["N"]).backward(_dev(o["dout"]))
        assert tuple(t.grad is not None for t in (a, b, p)) == wants
        if wants[0]:
            _check_grad("dvox_a", a.grad, g["dvox"][..., :ca], R.RTOL_DVOX, log)
        if wants[1]:
            _check_grad("dvox_b", b.grad, g["dvox"][..., ca:], R.RTOL_DVOX, log)
        if wants[2]:
            _check_dpose(p.grad, g, J, log)
    print("ops.resample_concat: %s" % "  ".join(log))


def test_pose_and_voxel_shapes_are_checked_before_any_launch():
    """A [B,5] pose would be read with stride 3, a pose batch shorter than the voxel batch past its end: both raise in Python."""
    from rendernet_amd import ops
    from rendernet_amd._lib import RenderNetHipError
    B = 2
    vox = torch.zeros((B, 8, 8, 8, 1), device="cuda")
    tex = torch.zeros((B, 8, 8, 8, 4), device="cuda")
    bad_poses = [torch.zeros((B, 5), device="cuda"), torch.zeros((1, 3), device="cuda"), torch.zeros((B, 2), device="cuda")]
    bad_matrices = [torch.zeros((B, 4, 3), device="cuda"), torch.zeros((B, 3), device="cuda"), torch.zeros((1, 3, 4), device="cuda"),
                    torch.zeros((B, 16), device="cuda")]
    for pose in bad_poses:
        with pytest.raises(RenderNetHipError, match="expected poses"):
            ops.resample(vox, pose, 16)
        with pytest.raises(RenderNetHipError, match="expected poses"):
            ops.resample_concat(vox, tex, pose, 16)
    for pose in (bad_poses[0], bad_poses[2], torch.zeros(3, device="cuda")):
        with pytest.raises(RenderNetHipError, match="expected poses"):
            ops.pose_to_affine(pose, 8, 16)
    for m in bad_matrices:
        with pytest.raises(RenderNetHipError, match="matrices"):
            ops.resample(vox, m, 16, affine=True)
        with pytest.raises(RenderNetHipError, match="matrices"):
            ops.resample_concat(vox, tex, m, 16, affine=True)
    good = torch.zeros((B, 3), device="cuda")
    for bad_vox in (torch.zeros((B, 8, 8, 4, 1), device="cuda"), torch.zeros((B, 8, 8, 8), device="cuda")):
        with pytest.raises(RenderNetHipError, match="voxel cube"):
            ops.resample(bad_vox, good, 16)
        with pytest.raises(RenderNetHipError, match="voxel cube"):
            ops.resample_concat(vox, bad_vox, good, 16)
