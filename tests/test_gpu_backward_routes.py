"""Every backward route in every multiply-stage mode against float64.  -m gpu.

The rows of tests/backward_cases.py (each pinned to its forward / input-gradient / filter-gradient route, asserted again here before
anything is launched) run through ops.<flavour> under ops.training(...) in "f32", "split" and "split16": forward, dx, dw, dbias, dalpha
and dresidual against float64 autograd over the oracle op on the same fp32 operands.

The bar is max|got - ref| <= 2e-4 * max|ref| with NO absolute floor, and max|ref| > 0.  The reference takes the branch of every PReLU
element from the sign of the launched forward's own output (the slopes are positive, so sign(y) = sign(z)), after the two forwards were
found to agree: a pre-activation within rounding of zero cannot flip a branch, and no element is left out.

Then the same case with dy * 2^-30 (what a training step feeds: every backward step is linear with constant coefficients, so the
deterministic launches -- dx, dresidual -- must give 2^-30 times the same bits, and a hidden absolute constant or a lost scale cannot),
with dy = 0, with frozen weights, the carried skip gradient of a res block on every route that fuses it, and ops.res_stack_2d.
Every test prints the ratios it measured.
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

pytestmark = pytest.mark.gpu
FILL = 0.25                       # what the gradient buffers hold before the backward: the kernels accumulate
SMALL = np.float32(2.0 ** -30)    # gradient-sized dy: a power of two, so it commutes exactly with every linear step


def _dev(a):
    return None if a is None else torch.as_tensor(a).cuda()


@functools.lru_cache(maxsize=None)
def _reference(i):
    """Operands and the float64 forward graph of case i: built once, shared by every test and mode."""
    row = BC.CASES[i][0]
    o = BC.layer_operands(row, zlib.crc32(repr(row).encode()))
    return o, BC.Reference(row, o)


def _run(row, o, dy, mode, frozen=False, fill=FILL, want_routes=None):
    """One forward + backward of a row through ops.<flavour> under a TrainContext whose gradient buffers are pre-filled."""
    from rendernet_amd import ops
    flavour, stride, epi = row[0], row[6], row[7]
    x = _dev(o["x"]).requires_grad_(True)
    res = _dev(o["res"])
    if res is not None:
        res.requires_grad_(True)
    params = {k: _dev(o[n]) for k, n in (("dw", "w"), ("dbias", "b"), ("dalpha", "alpha")) if o[n] is not None}
    bufs = {k: torch.full_like(p, fill) for k, p in params.items()}
    ready = []
    tc = ops.TrainContext({p.data_ptr(): bufs[k] for k, p in params.items()}, on_ready=ready.append, frozen=frozen)
    with ops.gemm_mode(mode), ops.training(tc):
        w = params["dw"]
        pw = ops.pack_conv_transpose(w, stride[0]) if flavour.endswith("transpose") else ops.pack_conv(w)
        if want_routes is not None:
            assert BC.routes_of(ops, row, pw) == want_routes           # before anything is launched
        y = getattr(ops, flavour)(x, pw, params["dbias"], params.get("dalpha"), res, stride, elu=(epi == "elu"))
        y.backward(_dev(dy))
    torch.cuda.synchronize()
    names = {p.data_ptr(): k for k, p in params.items()}
    out = {"y": y.detach(), "dx": x.grad, "dresidual": None if res is None else res.grad, "bufs": bufs,
           "ready": sorted(names[p] for p in ready), "params": sorted(params), "keep": (params, pw, tc)}
    return out


def _check(what, got, ref, log):
    r = BC.ratio(got, ref)
    log.append("%s %.2e" % (what, r))
    assert r <= BC.RTOL, "%s: max|got - ref| = %.3g * max|ref| > %.3g (%s)" % (what, r, BC.RTOL, "  ".join(log))


@pytest.mark.parametrize("mode", BC.MODES)
@pytest.mark.parametrize("i", range(len(BC.CASES)), ids=[BC.case_id(c) for c in BC.CASES])
def test_layer_backward_on_its_routes(i, mode):
    """Forward and every gradient of a row on the routes the table pins, accumulated onto a non-zero buffer; then gradient-sized dy;
    then dy = 0."""
    row, routes = BC.CASES[i]
    epi = row[7]
    o, ref = _reference(i)
    log = []
    got = _run(row, o, o["dy"], mode, want_routes=routes[mode])
    _check("forward", got["y"], ref.forward(), log)
    want = ref.grads(o["dy"], (got["y"].cpu() > 0) if epi == "prelu" else None)
    assert set(want) == {"dx"} | set(got["params"]) | ({"dresidual"} if epi == "res" else set())
    _check("dx", got["dx"], want["dx"], log)
    for k in got["params"]:                                              # the accumulate contract: constant + gradient
        _check(k, got["bufs"][k].double() - FILL, want[k], log)
    if epi == "res":
        _check("dresidual", got["dresidual"], want["dresidual"], log)
    assert got["ready"] == got["params"], "on_ready fired for %s, registered %s" % (got["ready"], got["params"])

    # gradient-sized operands: the float64 reference of dy * 2^-30 is 2^-30 * the reference above (exact in float64, as in the kernels)
    small = _run(row, o, o["dy"] * SMALL, mode, fill=FILL * float(SMALL))
    assert torch.equal(small["y"], got["y"])
    s = float(SMALL)
    _check("2^-30: dx", small["dx"], want["dx"] * s, log)
    for k in small["params"]:
        _check("2^-30: " + k, small["bufs"][k].double() - FILL * s, want[k] * s, log)
    if epi == "res":
        _check("2^-30: dresidual", small["dresidual"], want["dresidual"] * s, log)
    if epi != "elu":
        for k in ("dx", "dresidual"):
            if got[k] is not None:
                same = torch.equal(small[k], got[k] * s)
                log.append("2^-30: %s bit-equal %s" % (k, same))
                assert same, "%s of dy * 2^-30 is not 2^-30 * (%s of dy): max diff %.3g of max %.3g (%s)" % (
                    k, k, float((small[k] - got[k] * s).abs().max()), float((got[k] * s).abs().max()), "  ".join(log))

    # all-zero dy (split16: the launch sees max|dz| = 0)
    zero = _run(row, o, np.zeros_like(o["dy"]), mode)
    assert bool((zero["dx"] == 0).all()), "dx of dy = 0: max %.3g" % float(zero["dx"].abs().max())
    for k, buf in zero["bufs"].items():
        assert bool(torch.isfinite(buf).all()) and bool((buf == FILL).all()), "%s changed under dy = 0" % k
    if epi == "res":
        assert bool((zero["dresidual"] == 0).all())
    print("%s [%s] %s: %s" % (BC.case_id(BC.CASES[i]), mode, routes[mode], "  ".join(log)))


# The strided input gradient is a gather kernel that owns 16 input channels per thread; layers wider than that (none in the nets: the
# 32 -> 32 row of the table found the launcher refusing them) take it in chunks of 16: a ragged last chunk, 2-D and 3-D.
WIDE_STRIDED = [("conv2d", 2, (7, 9), 20, 8, 3, (2, 2), "res"), ("conv3d", 2, (4, 5, 6), 40, 8, 3, (1, 1, 2), "prelu")]


@pytest.mark.parametrize("row", WIDE_STRIDED, ids=lambda r: BC.case_id((r,)))
def test_strided_input_gradient_beyond_16_channels(row):
    from rendernet_amd import ops
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
    print("%s: %s" % (BC.case_id((row,)), "  ".join(log)))


def _takes_three_launch(case):
    return any("wino3l" in r for r in case[1].values())


FROZEN = [(i, None) for i in range(len(BC.CASES))] + [(i, m) for i, c in enumerate(BC.CASES) if _takes_three_launch(c) for m in BC.MODES]


@pytest.mark.parametrize("i,mode", FROZEN, ids=["%s-%s" % (BC.case_id(BC.CASES[i]), m or "default") for i, m in FROZEN])
def test_frozen_weights_give_the_same_input_gradient_and_touch_nothing(i, mode):
    """TrainContext(frozen=True), what inverse rendering runs on: the same deterministic input-gradient kernels (bit-identical dx and
    dresidual), no registered gradient buffer touched, on_ready never called.  Every row in the process default mode, the three-launch
    rows in all three."""
    row, _routes = BC.CASES[i]
    o, _ref = _reference(i)
    live = _run(row, o, o["dy"], mode)
    frozen = _run(row, o, o["dy"], mode, frozen=True)
    assert float(live["dx"].abs().max()) > 0
    assert torch.equal(frozen["y"], live["y"]) and torch.equal(frozen["dx"], live["dx"])
    if row[7] == "res":
        assert torch.equal(frozen["dresidual"], live["dresidual"])
    for k, buf in frozen["bufs"].items():
        assert bool((buf == FILL).all()), "%s was written with frozen weights" % k
        assert not bool((live["bufs"][k] == FILL).all())
    assert frozen["ready"] == [] and live["ready"] == live["params"]
    print("%s [%s]: frozen dx bit-identical, max|dx| %.3g" % (BC.case_id(BC.CASES[i]), mode or "default", float(live["dx"].abs().max())))


# ------------------------------------------------------------------------------------------------------------------------------
# the carried skip gradient (carry=True) and ops.res_stack_2d
# ------------------------------------------------------------------------------------------------------------------------------
@functools.lru_cache(maxsize=None)
def _stack_reference(flavour, sp, C, n_blocks, skip):
    o = BC.stack_operands(flavour, sp, C, n_blocks, skip, zlib.crc32(repr((flavour, sp, C, n_blocks, skip)).encode()))
    return o, BC.StackReference(flavour, o)


def _run_stack(flavour, o, mode, through_res_stack, monkeypatch=None):
    """n res blocks (+ skip conv with the input as its residual) as tools/layer_util.py launches them.  Returns y, the h of every block
    -- of THIS training forward: res_stack_2d keeps its h to itself, so its calls of ops.conv2d are recorded on their way through
    (monkeypatch) -- dx, the gradient buffers by "<block>.<name>" and the on_ready calls."""
    from rendernet_amd import ops
    conv = getattr(ops, flavour)
    x = _dev(o["x"]).requires_grad_(True)
    params, blocks = {}, []
    for i, b in enumerate(o["blocks"]):
        p = {k: _dev(v) for k, v in b.items()}
        params.update({"%d.%s" % (i, k): v for k, v in p.items()})
        blocks.append(p)
    skip = None if o["skip"] is None else {k: _dev(v) for k, v in o["skip"].items()}
    if skip is not None:
        params.update({"skip.%s" % k: v for k, v in skip.items()})
    bufs = {k: torch.full_like(p, FILL) for k, p in params.items()}
    ready = []
    tc = ops.TrainContext({p.data_ptr(): bufs[k] for k, p in params.items()}, on_ready=ready.append)
    hs = []
    if through_res_stack:
        def recording(*a, carry=False, **kw):
            out = conv(*a, carry=carry, **kw)
            if carry:                                  # a block's first conv: (h, carried x)
                hs.append(out[0].detach())
            return out
        monkeypatch.setattr(ops, flavour, recording)
    with ops.gemm_mode(mode):
        packs = [(ops.pack_conv(p["w1"]), p["b1"], p["a1"], ops.pack_conv(p["w2"]), p["b2"]) for p in blocks]
        spw = None if skip is None else ops.pack_conv(skip["w"])
        with ops.training(tc):
            if through_res_stack:
                y = ops.res_stack_2d(x, packs, None if skip is None else (spw, skip["b"], x))
            else:
                net = x
                for pw1, b1, a1, pw2, b2 in packs:
                    h, xc = conv(net, pw1, b1, a1, carry=True)
                    hs.append(h.detach())
                    net = conv(h, pw2, b2, None, residual=xc)
                y = net
            y.backward(_dev(o["dy"]))
    if through_res_stack:
        assert len(hs) == len(packs)
    torch.cuda.synchronize()
    names = {p.data_ptr(): k for k, p in params.items()}
    return {"y": y.detach(), "hs": hs, "dx": x.grad, "bufs": bufs, "ready": sorted(names[p] for p in ready), "params": sorted(params),
            "keep": (packs, spw, tc, params), "pw1": packs[0][0]}


def _check_stack(got, ref, o, log, tag=""):
    hs_ref, y_ref = ref.forward()
    _check(tag + "forward", got["y"], y_ref, log)
    for i, (h, h_ref) in enumerate(zip(got["hs"], hs_ref)):
        _check(tag + "h%d" % i, h, h_ref, log)
    want = ref.grads(o["dy"], [h.cpu() > 0 for h in got["hs"]])
    _check(tag + "dx", got["dx"], want["dx"], log)
    assert set(want) == {"dx"} | set(got["params"])
    for k in got["params"]:
        _check(tag + k, got["bufs"][k].double() - FILL, want[k], log)
    assert got["ready"] == got["params"]
    return want


@pytest.mark.parametrize("mode", BC.MODES)
@pytest.mark.parametrize("case", BC.BLOCK_CASES, ids=BC.block_id)
def test_res_block_carried_skip_gradient(case, mode, monkeypatch):
    """x + conv2(prelu(conv1(x) + b1)) + b2 with conv1 carrying x: the skip path's gradient comes back into conv1's node and is added
    to dx by the input-gradient launch's residual epilogue (the routes of ops.CARRY_IN_EPILOGUE) or by one add_ (direct).  Which of
    the two ran is asserted from ops._route on the dual pack.  With ops.CARRY_SKIP_GRADIENT off autograd adds the two paths: both
    settings meet the reference and agree within 1e-6 * max|dx| (the sum is rounded at another point; equal bits are not demanded)."""
    from rendernet_amd import ops
    (flavour, sp, C), routes = case
    o, ref = _stack_reference(flavour, sp, C, 1, False)
    log = []
    assert ops.CARRY_SKIP_GRADIENT is True
    fused = _run_stack(flavour, o, mode, False)
    with ops.gemm_mode(mode):
        r = ops._route(flavour, fused["pw1"].dgrad_pack(True), tuple(sp), (1,) * len(sp))
    assert BC.route_name(r) == routes[mode]
    assert (r.name in ops.CARRY_IN_EPILOGUE) == (routes[mode] != "direct")       # the epilogue branch / the add_ branch
    want = _check_stack(fused, ref, o, log)
    # the skip path must be IN dx: without it dx misses dy itself
    assert float(want["dx"].abs().max()) > 0
    monkeypatch.setattr(ops, "CARRY_SKIP_GRADIENT", False)
    plain = _run_stack(flavour, o, mode, False)
    _check_stack(plain, ref, o, log, "no carry: ")
    gap = float((plain["dx"] - fused["dx"]).abs().max()) / float(plain["dx"].abs().max())
    log.append("carry vs autograd sum %.2e" % gap)
    assert gap <= 1e-6, log
    print("res block %s [%s] conv1 dgrad on %s: %s" % (BC.block_id(case), mode, routes[mode], "  ".join(log)))


@pytest.mark.parametrize("mode", BC.MODES)
def test_res_stack_2d_gradients(mode, monkeypatch):
    """ops.res_stack_2d: two blocks and the skip conv whose residual is the stack's input, 256 channels on 8x13.  The output and every
    gradient; dx collects three paths -- the chain of blocks, the carried copies, the skip residual.  The PReLU branches of the reference
    come from the h of the training forward itself."""
    o, ref = _stack_reference("conv2d", (8, 13), 256, 2, True)
    log = []
    got = _run_stack("conv2d", o, mode, True, monkeypatch)
    _check_stack(got, ref, o, log)
    assert len(got["params"]) == 12
    print("res_stack_2d [%s]: %s" % (mode, "  ".join(log)))
