"""The memory-bound helper kernels against float64 at the edges of their launch geometry.  -m gpu.

Epilogue backward, loss, Adam, SGD, fully connected forward / backward, stand-alone PReLU, Phong backward and the strided gather
input gradient, through the C ABI (through ops.* where the branch is chosen in Python), on the seeded inputs of
tests/helper_kernels_ref.py and inside the bounds derived there: grid caps and grid-stride loops, tails, batch chunks, template
switches, NULL outputs, aliasing, the accumulate contracts and every refusal (each followed by a launch that must pass).
tests/test_helper_kernels_ref_cpu.py shows on the CPU that the same inputs reach the same bounds.  Every test prints the largest
observed / bound ratio per output.
"""
import functools
import os
import sys
import zlib

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backward_cases as BC  # noqa: E402
import helper_kernels_ref as HR  # noqa: E402

pytestmark = pytest.mark.gpu
F32 = np.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _dev(a):
    return None if a is None else torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _np(t):
    return t.detach().cpu().numpy()


def _merge(worst, new):
    for k, v in new.items():
        worst[k] = max(worst.get(k, 0.0), v)


def _report(what, worst):
    print("%s observed / bound: %s" % (what, "  ".join("%s %.3f" % kv for kv in sorted(worst.items()))))
    assert max(worst.values()) <= 1.0, (what, worst)


# ---------------------------------------------------------------------------------------------
# epilogue backward

@functools.lru_cache(maxsize=2)
def _epi(M, C, act):
    o = HR.epi_inputs(M, C, act)
    return o, HR.epi_ref(o, act)


def _epi_launch(o, M, C, act, ws=None, alias=False, dbias=True, dalpha=True):
    """One call of rn_epilogue_bwd (ws None) or rn_epilogue_bwd_ws; the sums start from EPI_START_*.  -> (rc, dz, dbias, dalpha)."""
    from rendernet_amd import _lib as L
    lib = L.lib()
    dy, z, y, al = _dev(o["dy"]), _dev(o["z"]), _dev(o["y"]), _dev(o["alpha"])
    dz = dy if alias else torch.full((M, C), float("nan"), device="cuda")
    db = torch.full((C,), HR.EPI_START_B, device="cuda")
    da = torch.full((C,), HR.EPI_START_A, device="cuda")
    args = (L.ptr(dy), L.ptr(z), L.ptr(y), L.ptr(al), L.ptr(dz), L.ptr(db) if dbias else None, L.ptr(da) if dalpha else None, M, C, act)
    if ws is None:
        rc = lib.rn_epilogue_bwd(*args, L.stream_ptr())
    else:
        rc = lib.rn_epilogue_bwd_ws(*args, L.ptr(ws), ws.numel(), L.stream_ptr())
    return rc, _np(dz), _np(db), _np(da)


def _epi_check(got, ref, act, what, worst, dbias=True, dalpha=True):
    rc, dz, db, da = got
    assert rc == 0, what
    prelu = bool(act & HR.ACT_PRELU)
    _merge(worst, HR.epi_ratios(dz, db if dbias else None, da if (dalpha and prelu) else None, ref, act, what))
    if not dbias:
        assert (db == F32(HR.EPI_START_B)).all(), what + ": dbias = NULL, yet the buffer beside it changed"
    if not (dalpha and prelu):
        assert (da == F32(HR.EPI_START_A)).all(), what + ": dalpha must stay as it was"


@pytest.mark.parametrize("M,C,act", HR.EPI_CASES)
def test_epilogue_bwd_at_the_launch_geometry_edges(M, C, act):
    """dz fresh and aliasing dy (bit-equal), each sum alone, the plain and the workspace entry (bit-equal dz), sums onto non-zero
    start values.  The cases: 1024-thread vector kernel with 8 channel groups and two-stage sums; two group columns; ELU on the
    vector and on the generic kernel; ELU | PReLU, which the launcher accepts (both factors apply); C = 4 with M = 1 and M = 3."""
    from rendernet_amd import _lib as L
    o, ref = _epi(M, C, act)
    ws = torch.full((L.lib().rn_epilogue_bwd_workspace_floats(M, C),), float("nan"), device="cuda")
    assert ws.numel() == 512 * 2 * C and ws.data_ptr() % 16 == 0
    worst = {}
    base = _epi_launch(o, M, C, act)
    _epi_check(base, ref, act, "plain", worst)
    for name, kw in (("plain, dz = dy", dict(alias=True)), ("ws", dict(ws=ws)), ("ws, dz = dy", dict(ws=ws, alias=True)),
                     ("plain, dalpha only", dict(dbias=False)), ("plain, dbias only", dict(dalpha=False)),
                     ("ws, dalpha only", dict(ws=ws, dbias=False)), ("ws, dbias only", dict(ws=ws, dalpha=False))):
        got = _epi_launch(o, M, C, act, **kw)
        _epi_check(got, ref, act, name, worst, kw.get("dbias", True), kw.get("dalpha", True))
        assert np.array_equal(got[1], base[1]), name + ": dz differs in bits from the plain call's"
    _report("epilogue_bwd (%d, %d, act %d) %s" % (M, C, act, HR.epi_geometry(M, C)["path"]), worst)


def test_epilogue_bwd_refuses_wide_generic_rows_and_goes_on():
    M, C, act = HR.EPI_REFUSED
    assert HR.epi_geometry(M, C)["path"] == "refused"
    rc, _, db, da = _epi_launch(HR.epi_inputs(M, C, act), M, C, act)
    assert rc == HR.RN_E_UNSUPPORTED
    assert (db == F32(HR.EPI_START_B)).all() and (da == F32(HR.EPI_START_A)).all()
    worst = {}
    M, C, act = 3, 4, 3
    o, ref = _epi(M, C, act)
    _epi_check(_epi_launch(o, M, C, act), ref, act, "after the refusal", worst)
    _report("epilogue_bwd after a refused C = 1028", worst)


def test_epilogue_bwd_ws_off_a_16_byte_boundary_takes_the_atomics():
    """A workspace 4 bytes off a 16-byte boundary: the partials would be stored as float4, so the launcher must fall back to the
    atomics and write nothing into it (the sums meet their bars, every sentinel word is unchanged)."""
    from rendernet_amd import _lib as L
    src = open(os.path.join(ROOT, "rendernet_amd", "csrc", "train_kernels.hip")).read()
    assert "((uintptr_t)ws & 15) == 0" in src                    # the library under test is built from a source that checks
    M, C, act = 65573, 32, 1
    assert HR.epi_geometry(M, C)["two_stage"]
    o, ref = _epi(M, C, act)
    n = L.lib().rn_epilogue_bwd_workspace_floats(M, C)
    sentinel = -7.5
    ws_base = torch.full((n + 1,), sentinel, device="cuda")
    ws = ws_base[1:]
    assert ws.data_ptr() % 16 == 4 and ws.numel() == n
    worst = {}
    _epi_check(_epi_launch(o, M, C, act, ws=ws), ref, act, "misaligned ws", worst)
    assert bool((ws_base == sentinel).all()), "the misaligned workspace was written"
    aligned = torch.full((n,), sentinel, device="cuda")
    _epi_check(_epi_launch(o, M, C, act, ws=aligned), ref, act, "aligned ws", worst)
    assert not bool((aligned == sentinel).all())                  # the two-stage path is what an aligned workspace gets
    _report("epilogue_bwd_ws (%d, %d) misaligned workspace" % (M, C), worst)


# ---------------------------------------------------------------------------------------------
# loss

@pytest.mark.parametrize("mode", [0, 1])
def test_loss_grid_stride_null_dpred_and_sharded_divisor(mode):
    """n past the 2048-workgroup cap; dpred given and NULL; the local divisor and twice it; BCE's guard elements (p in {0, 1, 1e-7,
    1 - 2^-24} x t in {0, 1}); the loss accumulated onto a non-zero loss_sum."""
    from rendernet_amd import _lib as L
    p, t = HR.loss_inputs(mode)
    pd, td = _dev(p), _dev(t)
    worst = {}
    for div in (HR.loss_local_divisor(mode, p.size), 2 * HR.loss_local_divisor(mode, p.size)):
        loss, dp, bound = HR.loss_ref(p, t, mode, div)
        for with_dp in (True, False):
            got_dp = torch.full((p.size,), float("nan"), device="cuda")
            acc = torch.full((1,), HR.LOSS_START, dtype=torch.float64, device="cuda")
            L.check(L.lib().rn_loss_fwd_bwd(L.ptr(pd), L.ptr(td), L.ptr(got_dp) if with_dp else None, acc.data_ptr(), p.size, div, mode,
                                            L.stream_ptr()), "rn_loss_fwd_bwd")
            _merge(worst, {"loss": abs(float(acc.item()) - HR.LOSS_START - loss) / (HR.LOSS_BAR * abs(loss))})
            if with_dp:
                _merge(worst, {"dpred": HR.worst(_np(got_dp), dp, bound, "dpred")})
            else:
                assert bool(torch.isnan(got_dp).all())
    _report("loss mode %d n = %d" % (mode, p.size), worst)


# ---------------------------------------------------------------------------------------------
# Adam and SGD

def _adam_launch(o, n, gs, views=None):
    from rendernet_amd import _lib as L
    h = HR.ADAM_HYPER
    t = views or {k: _dev(o[k]) for k in ("p", "g", "m", "v")}
    rc = L.lib().rn_adam_step(L.ptr(t["p"]), L.ptr(t["g"]), L.ptr(t["m"]), L.ptr(t["v"]), n, float(h["lr_t"]), float(h["b1"]),
                              float(h["b2"]), float(h["eps"]), gs, L.stream_ptr())
    return rc, {k: _np(t[k]) for k in ("p", "m", "v")}


@pytest.mark.parametrize("n", HR.ADAM_NS)
def test_adam_one_step_from_a_given_state(n):
    """No vector part (n < 4), no tail (n % 4 == 0), both, grad_scale 1 and 0.125, g = 0 elements."""
    o = HR.adam_inputs(n)
    worst = {}
    for gs in HR.ADAM_GRAD_SCALES:
        rc, got = _adam_launch(o, n, gs)
        assert rc == 0
        _merge(worst, HR.adam_ratios(got, HR.adam_ref(o, gs), "Adam"))
    _report("Adam n = %d" % n, worst)


def test_adam_refuses_a_misaligned_buffer_and_writes_nothing():
    n = 1024
    o = HR.adam_inputs(n)
    base = torch.zeros(n + 1, device="cuda")
    base[1:] = _dev(o["p"])
    before = base.clone()
    views = {"p": base[1:], "g": _dev(o["g"]), "m": _dev(o["m"]), "v": _dev(o["v"])}
    assert views["p"].data_ptr() % 16 == 4
    rc, got = _adam_launch(o, n, 1.0, views)
    assert rc == HR.RN_E_INVALID
    assert torch.equal(base, before) and np.array_equal(got["m"], o["m"]) and np.array_equal(got["v"], o["v"])
    rc, got = _adam_launch(o, n, 1.0)
    assert rc == 0
    _report("Adam after a refused misaligned buffer", HR.adam_ratios(got, HR.adam_ref(o, 1.0), "Adam"))


@pytest.mark.parametrize("n", HR.SGD_NS)
def test_sgd_step(n):
    from rendernet_amd import _lib as L
    p, g = HR.sgd_inputs(n)
    pd, gd = _dev(p), _dev(g)
    L.check(L.lib().rn_sgd_step(L.ptr(pd), L.ptr(gd), n, float(HR.SGD_LR), L.stream_ptr()), "rn_sgd_step")
    ref, bound = HR.sgd_ref(p, g)
    assert np.array_equal(_np(gd), g)
    _report("SGD n = %d" % n, {"p": HR.worst(_np(pd), ref, bound, "sgd")})


# ---------------------------------------------------------------------------------------------
# fully connected

@pytest.mark.parametrize("bias", [True, False], ids=["bias", "nobias"])
@pytest.mark.parametrize("B,fin,fout", HR.FC_CASES)
def test_fully_connected_forward_and_backward(B, fin, fout, bias):
    """Every activation through rn_fully_connected_fwd and _fwd_train (bit-equal y; the pre-activation and the activation of it
    against float64), then rn_fully_connected_bwd: dw onto a buffer of 0.25 with dx, dx alone, dw alone (bit-equal to the joint call;
    the sentinel-filled buffer of the output that was not asked for is unchanged)."""
    from rendernet_amd import _lib as L
    lib, st = L.lib(), L.stream_ptr()
    o = HR.fc_inputs(B, fin, fout)
    ref = HR.fc_ref(o, bias)
    x, w, dz = _dev(o["x"]), _dev(o["w"]), _dev(o["dz"])
    b, al = (_dev(o["b"]) if bias else None), _dev(o["alpha"])
    worst = {}
    for name, act in HR.FC_ACTS.items():
        y0 = torch.full((B, fout), float("nan"), device="cuda")
        y1, pre = y0.clone(), y0.clone()
        a = al if act == HR.ACT_PRELU else None
        L.check(lib.rn_fully_connected_fwd(L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(a), L.ptr(y0), B, fin, fout, act, st), "fc fwd")
        L.check(lib.rn_fully_connected_fwd_train(L.ptr(x), L.ptr(w), L.ptr(b), L.ptr(a), L.ptr(y1), L.ptr(pre), B, fin, fout, act, st), "fc fwd_train")
        assert torch.equal(y0, y1), name + ": fwd and fwd_train differ in bits"
        z32 = _np(pre)
        _merge(worst, {"z": HR.worst(z32, ref["z"], ref["bound_z"], "preact")})
        want, bound = HR.act_ref(z32, o["alpha"], act)
        if act == 0:
            assert np.array_equal(_np(y0), z32)
        else:
            _merge(worst, {name: HR.worst(_np(y0), want, bound, name)})
    sentinel = -7.5
    dw = torch.full((fin, fout), HR.FC_DW_START, device="cuda")
    dx = torch.full((B, fin), sentinel, device="cuda")
    L.check(lib.rn_fully_connected_bwd(L.ptr(x), L.ptr(w), L.ptr(dz), L.ptr(dx), L.ptr(dw), B, fin, fout, st), "fc bwd")
    _merge(worst, {"dw": HR.worst(_np(dw), HR.FC_DW_START + ref["dw"], ref["bound_dw"], "dw"),
                   "dx": HR.worst(_np(dx), ref["dx"], ref["bound_dx"], "dx")})
    dw_idle = torch.full((fin, fout), HR.FC_DW_START, device="cuda")
    dx_only = torch.full((B, fin), sentinel, device="cuda")
    L.check(lib.rn_fully_connected_bwd(None, L.ptr(w), L.ptr(dz), L.ptr(dx_only), None, B, fin, fout, st), "fc bwd dx only")
    assert torch.equal(dx_only, dx) and bool((dw_idle == HR.FC_DW_START).all())
    dw_only = torch.full((fin, fout), HR.FC_DW_START, device="cuda")
    dx_idle = torch.full((B, fin), sentinel, device="cuda")
    L.check(lib.rn_fully_connected_bwd(L.ptr(x), None, L.ptr(dz), None, L.ptr(dw_only), B, fin, fout, st), "fc bwd dw only")
    assert torch.equal(dw_only, dw) and bool((dx_idle == sentinel).all())
    _report("FC (%d, %d, %d) %s" % (B, fin, fout, "bias" if bias else "no bias"), worst)


@pytest.mark.parametrize("B,fin,fout", HR.FC_CASES)
def test_fully_connected_through_ops_chooses_dx_and_dw(B, fin, fout):
    """ops.fully_connected picks the outputs of the backward: frozen weights give dx alone and touch no gradient buffer, an input
    that needs no gradient gives dw alone.  bias + PReLU, so the epilogue backward runs on rows [B, fout]."""
    from rendernet_amd import ops
    o = HR.fc_inputs(B, fin, fout)
    w, b, al = _dev(o["w"]), _dev(o["b"]), _dev(o["alpha"])
    fill = HR.FC_DW_START
    worst = {}
    for frozen, x_grad in ((False, True), (True, True), (False, False)):
        x = _dev(o["x"]).requires_grad_(x_grad)
        bufs = {k: torch.full_like(p, fill) for k, p in (("w", w), ("b", b), ("alpha", al))}
        tc = ops.TrainContext({w.data_ptr(): bufs["w"], b.data_ptr(): bufs["b"], al.data_ptr(): bufs["alpha"]}, frozen=frozen)
        with ops.training(tc):
            y = ops.fully_connected(x, w, b, al)
            y.backward(_dev(o["dz"]))
        z32 = HR.fc_emulate_fwd(o, True, 0)[0]                  # branches: from a pre-activation; the kernel's own is checked above
        yv = _np(y)
        assert np.array_equal(yv > 0, z32 > 0), "a pre-activation within rounding of zero: choose another seed"
        e = HR.epi_ref({"dy": o["dz"], "z": z32, "y": None, "alpha": o["alpha"]}, HR.ACT_PRELU)
        # the epilogue's dz is ONE product of fp32 operands (dy * alpha): its float64 value rounded to fp32 is what the kernel stores
        ref = HR.fc_ref(dict(o, dz=e["dz"].astype(F32)), True)
        if x_grad:
            _merge(worst, {"dx": HR.worst(_np(x.grad), ref["dx"], ref["bound_dx"], "dx")})
        else:
            assert x.grad is None
        if frozen:
            assert all(bool((v == fill).all()) for v in bufs.values()), "frozen weights, yet a gradient buffer changed"
        else:
            want_a = fill + e["dalpha"]                         # the sums' bars with the start value among the magnitudes
            _merge(worst, {"dw": HR.worst(_np(bufs["w"]), fill + ref["dw"], ref["bound_dw"], "dw"),
                           "dbias": HR.worst(_np(bufs["b"]), fill + e["dbias"], HR.DBIAS_BAR * (e["abs_b"].max() + fill), "dbias"),
                           "dalpha": HR.worst(_np(bufs["alpha"]), want_a, HR.DALPHA_BAR * max(np.abs(want_a).max(), 1.0), "dalpha")})
    _report("ops.fully_connected (%d, %d, %d)" % (B, fin, fout), worst)


# ---------------------------------------------------------------------------------------------
# stand-alone PReLU

@pytest.mark.parametrize("n", HR.PRELU_NS)
def test_prelu_grid_stride_with_a_channel_count_that_does_not_divide_256(n):
    from rendernet_amd import _lib as L
    v, alpha = HR.prelu_inputs(n)
    vd, ad = _dev(v), _dev(alpha)
    y = torch.full((n,), float("nan"), device="cuda")
    L.check(L.lib().rn_prelu_fwd(L.ptr(vd), L.ptr(ad), L.ptr(y), n, HR.PRELU_C, L.stream_ptr()), "rn_prelu_fwd")
    got, want = _np(y), HR.prelu_expect(v, alpha)
    bad = np.flatnonzero(got.view(np.uint32) != want.view(np.uint32))
    assert bad.size == 0, "%d of %d elements differ in bits, the first at %d" % (bad.size, n, bad[0])
    print("prelu n = %d C = %d: bit-equal" % (n, HR.PRELU_C))


# ---------------------------------------------------------------------------------------------
# Phong backward

@pytest.mark.parametrize("mode", HR.PHONG_MODES)
def test_phong_backward_sums_dlight_over_workgroups_and_accumulates(mode):
    """47 x 45 pixels: two workgroups per item add into one dlight.  Then the C entry once more ONTO that dlight: it doubles."""
    from rendernet_amd import _lib as L, ops
    img, light, col, albedo, wgt = HR.phong_inputs()
    B, H, W = HR.PHONG_SHAPE
    ref = HR.phong_grads(mode, img, light, col, albedo, wgt)
    i, l, a = (_dev(t).requires_grad_(True) for t in (img, light, albedo))
    cd, wd = _dev(col), _dev(wgt)
    out = ops.phong_composite(i, l, cd, HR.PHONG_AMBIENT, HR.PHONG_KD, mode, albedo=a)
    assert np.abs(_np(out) - ref["out"]).max() <= 3e-5
    (out * wd).sum().backward()
    worst = HR.phong_ratios({"dimg": _np(i.grad), "dlight": _np(l.grad), "dalbedo": _np(a.grad)}, ref, "Phong " + mode)
    dl = l.grad.clone()
    L.check(L.lib().rn_phong_composite_bwd(L.ptr(i.detach()), L.ptr(l.detach()), L.ptr(cd), L.ptr(a.detach()), HR.PHONG_AMBIENT, HR.PHONG_KD,
                                           L.ptr(wd), None, L.ptr(dl), None, B, H, W, HR.PHONG_CODES[mode], L.stream_ptr()), "phong bwd")
    twice = 2 * ref["dlight"]
    worst["dlight x2"] = HR.worst(_np(dl), twice, HR.PHONG_RTOL * np.abs(twice).max() + HR.PHONG_ATOL, "accumulated dlight")
    assert np.abs(ref["dlight"]).max() > 0.1
    _report("Phong backward %s %dx%d" % (mode, H, W), worst)


# ---------------------------------------------------------------------------------------------
# strided input gradient

def _strided_row(row):
    from rendernet_amd import ops
    from test_gpu_backward_routes import FILL, _check, _run
    assert BC.routes_of(ops, row) == "direct direct direct"
    o = BC.layer_operands(row, zlib.crc32(repr(row).encode()))
    ref = BC.Reference(row, o)
    log = []
    got = _run(row, o, o["dy"], None)
    _check("forward", got["y"], ref.forward(), log)
    want = ref.grads(o["dy"], (got["y"].cpu() > 0) if row[7] == "prelu" else None)
    _check("dx", got["dx"], want["dx"], log)
    for k in got["params"]:
        _check(k, got["bufs"][k].double() - FILL, want[k], log)
    print("%s (%d channels per thread): %s" % (BC.case_id((row,)), HR.strided_chunk(row[3]), "  ".join(log)))


def test_strided_input_gradient_narrow_chunks_and_the_lds_refusal():
    """Cin = 3 (4 channels per thread), then a filter whose staged copy exceeds 64 KiB (the launcher refuses; nothing is launched),
    then Cin = 5 (a ragged chunk of 8) on the device the refusal left behind."""
    from rendernet_amd import _lib as L, ops
    from test_gpu_backward_routes import _run
    _strided_row(HR.STRIDED_ROWS[0])
    row = HR.STRIDED_OVER_LDS
    assert BC.routes_of(ops, row) == "direct direct direct" and HR.strided_lds_bytes(row) > 64 * 1024
    o = BC.layer_operands(row, 7)
    with pytest.raises(L.RenderNetHipError, match="exceeds LDS budget"):
        _run(row, o, o["dy"], None)
    torch.cuda.synchronize()
    _strided_row(HR.STRIDED_ROWS[1])
