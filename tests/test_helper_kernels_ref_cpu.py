"""tests/helper_kernels_ref.py pinned without a GPU: every float64 reference against torch float64 autograd over the oracle op, the
launch-geometry branch every case is meant to reach, and an fp32 emulation of every kernel's arithmetic inside every bound on the very
inputs tests/test_gpu_helper_kernels.py launches (so the bounds and the inputs are reachable before anything runs on a device).
Every test prints the largest observed / bound ratio it measured."""
import os
import sys

import numpy as np
import pytest
import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import backward_cases as BC  # noqa: E402
import helper_kernels_ref as HR  # noqa: E402

from oracle import layers as OL  # noqa: E402
from oracle import reconstruct as ORC  # noqa: E402
from oracle import train as OT  # noqa: E402

F32, U = np.float32, HR.U


def _t64(a, grad=True):
    return torch.from_numpy(np.ascontiguousarray(a)).double().requires_grad_(grad)


def _agree(got, want, rtol, what):
    top = np.abs(want).max()
    assert np.abs(np.asarray(got) - np.asarray(want)).max() <= rtol * top, (what, np.abs(got - want).max(), top)


def _merge(worst, new):
    for k, v in new.items():
        worst[k] = max(worst.get(k, 0.0), v)


# ---------------------------------------------------------------------------------------------
def test_epilogue_cases_reach_the_branches_they_name():
    g = {c: HR.epi_geometry(c[0], c[1]) for c in HR.EPI_CASES}
    a = g[(65573, 32, 1)]
    assert (a["path"], a["NT"], a["G"], a["nb"], a["two_stage"]) == ("vec", 1024, 8, 129, True)
    b = g[(1031, 2048, 1)]
    assert (b["path"], b["NT"], b["gy"], b["nb"], b["two_stage"]) == ("vec", 1024, 2, 65, True)
    assert g[(1000, 8, 4)]["path"] == "vec" and g[(1000, 8, 4)]["NT"] == 256
    assert g[(1000, 3, 4)]["path"] == "gen" and g[(1000, 20, 5)]["path"] == "gen"
    assert g[(1, 4, 1)] == {"path": "vec", "NT": 256, "G": 1, "gy": 1, "rstep": 256, "rpb": 1024, "nb": 1, "two_stage": False}
    assert g[(3, 4, 3)]["path"] == "vec"
    c = g[(777, 1024, 1)]
    assert (c["path"], c["NT"], c["G"], c["rstep"]) == ("vec", 256, 256, 1)
    assert HR.epi_geometry(*HR.EPI_REFUSED[:2]) == {"path": "refused"}
    for geo in g.values():                                        # the workspace of 512 x 2 x C floats always holds the partials
        assert geo["nb"] <= 512


@pytest.mark.parametrize("M,C,act", HR.EPI_CASES)
def test_epilogue_reference_and_emulation(M, C, act):
    o = HR.epi_inputs(M, C, act)
    ref = HR.epi_ref(o, act)
    # the oracle graph in float64: y = sigmoid?(elu?(prelu?(z + b)))
    z, al, b = _t64(o["z"]), _t64(o["alpha"]), torch.zeros(C, dtype=torch.float64, requires_grad=True)
    y = z + b
    if act & HR.ACT_PRELU:
        y = OL.prelu(y, al)
    if act & HR.ACT_ELU:
        y = F.elu(y)
    if act & HR.ACT_SIGMOID:
        y = torch.sigmoid(y)
    if o["y"] is not None:
        assert np.abs(y.detach().numpy() - o["y"]).max() <= 2 * U                         # the y the kernel is given is this forward's
    gz, ga, gb = torch.autograd.grad(y, [z, al, b], _t64(o["dy"], False), allow_unused=True)
    _agree(ref["dz"], gz.numpy(), 1e-6, "dz")
    _agree(ref["dbias"], gb.numpy(), 1e-6 * M ** 0.5, "dbias")
    if act & HR.ACT_PRELU:
        _agree(ref["dalpha"], ga.numpy(), 1e-6 * M ** 0.5, "dalpha")
    else:
        assert not ref["dalpha"].any()
    em = HR.epi_emulate(o, act, M, C)
    r = HR.epi_ratios(em["dz"], em["dbias"], em["dalpha"], ref, act, "emulation")
    print("epilogue (%d, %d, act %d) emulation / bound: %s" % (M, C, act, "  ".join("%s %.3f" % kv for kv in r.items())))
    assert max(r.values()) <= 1.0, r
    assert np.abs(ref["dz"]).max() > 0


# ---------------------------------------------------------------------------------------------
def test_loss_reference_against_the_oracle():
    rng = np.random.default_rng(0)
    p = rng.uniform(0.01, 0.99, (3, 20, 20, 1)).astype(F32)
    t = rng.uniform(0, 1, p.shape).astype(F32)
    for mode, div in ((0, 3.0), (1, float(p.size))):
        pt = _t64(p)
        loss = OL.bce_loss(pt, _t64(t, False)) if mode == 0 else OT.mse_loss(pt, _t64(t, False))
        loss.backward()
        got, dp, bound = HR.loss_ref(p.ravel(), t.ravel(), mode, div)
        # the reference forms 1e-6 + p and (1e-6 + 1) - p in fp32, the oracle in float64: 4.6e-8 absolute on a1 >= 0.01
        assert abs(got - loss.item()) <= 1e-5 * abs(loss.item())
        # relative to the magnitudes the bound is made of (BCE's two quotients cancel)
        assert (np.abs(dp - pt.grad.numpy().ravel()) <= 1e-5 * bound / (4 * U)).all()
        assert (bound > 0).all()
    # the edge elements: a1 at p = 1 is the fp32 value 9.54e-7, a0 at p = 0 is fp32(1e-6)
    p, t = HR.loss_inputs(0)
    assert list(p[:8]) == [0, 1, F32(1e-7), F32(1 - 2.0 ** -24)] * 2 and list(t[:8]) == [0] * 4 + [1] * 4
    _, dp, _ = HR.loss_ref(p[:8], t[:8], 0, 1.0)
    a1 = float((F32(1e-6) + F32(1)) - F32(1))
    assert a1 == 2.0 ** -20 and abs(a1 - 9.5367e-7) < 1e-10
    assert dp[1] == 1.0 / a1 and dp[4] == -1.0 / float(F32(1e-6))
    assert np.isfinite(dp).all()


@pytest.mark.parametrize("mode", [0, 1])
def test_loss_emulation_inside_the_bounds(mode):
    p, t = HR.loss_inputs(mode)
    assert p.size == HR.LOSS_N > 2048 * 256
    worst = {}
    for div in (HR.loss_local_divisor(mode, p.size), 2 * HR.loss_local_divisor(mode, p.size)):
        loss, dp, bound = HR.loss_ref(p, t, mode, div)
        for fma in (False, True):
            got_loss, got_dp = HR.loss_emulate(p, t, mode, div, fma)
            _merge(worst, {"loss": abs(got_loss - loss) / (HR.LOSS_BAR * abs(loss)), "dpred": HR.worst(got_dp, dp, bound, "dpred")})
    print("loss mode %d emulation / bound: %s" % (mode, "  ".join("%s %.3f" % kv for kv in worst.items())))
    assert max(worst.values()) <= 1.0, worst


# ---------------------------------------------------------------------------------------------
def test_adam_reference_against_the_oracle():
    o = HR.adam_inputs(1024)
    opt = OT.Adam(e_eta=1e-3, decay_steps=2, beta1=0.9, beta2=0.999, epsilon=1e-8)
    opt.t = 3
    opt.m["p"], opt.v["p"] = o["m"].copy(), o["v"].copy()
    import math
    lr_t = F32(OT.exponential_decay(1e-3, 3, 2) * math.sqrt(1.0 - 0.999 ** 4) / (1.0 - 0.9 ** 4))
    for gs in HR.ADAM_GRAD_SCALES:
        opt.t = 3
        opt.m["p"], opt.v["p"] = o["m"].copy(), o["v"].copy()
        want = opt.apply({"p": o["p"].copy()}, {"p": o["g"] * F32(gs)})["p"]                 # the oracle is fp32: 1e-5 of the largest
        ref = HR.adam_ref(o, gs, dict(HR.ADAM_HYPER, lr_t=lr_t))
        _agree(ref["p"], want, 1e-6, "p")
        _agree(ref["m"], opt.m["p"], 1e-6, "m")
        _agree(ref["v"], opt.v["p"], 1e-6, "v")
        assert np.abs(ref["step"]).max() > 1e-4


@pytest.mark.parametrize("n", HR.ADAM_NS)
def test_adam_emulation_inside_the_bounds(n):
    o = HR.adam_inputs(n)
    assert (o["m"] != 0).all() and (o["v"] > 0).all() and (n < 3 or (o["g"] == 0).any())
    b1, c1 = float(HR.ADAM_HYPER["b1"]), float(F32(1) - HR.ADAM_HYPER["b1"])
    worst = {}
    for gs in HR.ADAM_GRAD_SCALES:
        ref = HR.adam_ref(o, gs)
        # the inputs keep m_new clear of cancellation: |m_new| >= 0.98 (b1 |m| + (1 - b1) |g gs|)
        assert (np.abs(ref["m"]) >= 0.97 * (b1 * np.abs(HR.f64(o["m"])) + c1 * np.abs(HR.f64(o["g"]) * gs))).all()
        zero = o["g"] == 0
        assert np.array_equal(ref["m"][zero], b1 * HR.f64(o["m"])[zero])                       # g = 0: m and v decay
        for fma in (False, True):
            _merge(worst, HR.adam_ratios(HR.adam_emulate(o, gs, fma), ref, "emulation"))
    print("Adam n = %d emulation / bound: %s" % (n, "  ".join("%s %.3f" % kv for kv in worst.items())))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("n", HR.SGD_NS)
def test_sgd_emulation_inside_the_bound(n):
    p, g = HR.sgd_inputs(n)
    ref, bound = HR.sgd_ref(p, g)
    r = max(HR.worst(HR.sgd_emulate(p, g, fma), ref, bound, "sgd") for fma in (False, True))
    print("SGD n = %d emulation / bound: %.3f" % (n, r))
    assert r <= 1.0 and (n <= 4096 * 256) == (n < 1000)


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,fin,fout", HR.FC_CASES)
def test_fc_reference_and_emulation(B, fin, fout):
    o = HR.fc_inputs(B, fin, fout)
    worst = {}
    for bias in (True, False):
        ref = HR.fc_ref(o, bias)
        x, w, b = _t64(o["x"]), _t64(o["w"]), _t64(o["b"])
        z = OL.fully_connected(x, w, b if bias else None)
        gx, gw = torch.autograd.grad(z, [x, w], _t64(o["dz"], False))
        assert np.abs(ref["z"] - z.detach().numpy()).max() <= 1e-12 * max(np.abs(ref["z"]).max(), 1)
        assert np.abs(ref["dx"] - gx.numpy()).max() <= 1e-12 * max(np.abs(ref["dx"]).max(), 1)
        assert np.abs(ref["dw"] - gw.numpy()).max() <= 1e-12 * max(np.abs(ref["dw"]).max(), 1)
        assert np.abs(ref["z"]).max() <= HR.SIGMOID_MAX_Z - 1
        for name, act in HR.FC_ACTS.items():
            z32, y32 = HR.fc_emulate_fwd(o, bias, act)
            _merge(worst, {"z": HR.worst(z32, ref["z"], ref["bound_z"], "z")})
            want, bound = HR.act_ref(z32, o["alpha"], act)
            zt = torch.from_numpy(HR.f64(z32))
            oracle = {"none": zt, "prelu": OL.prelu(zt, torch.from_numpy(HR.f64(o["alpha"]))), "elu": F.elu(zt), "sigmoid": torch.sigmoid(zt)}[name]
            assert np.abs(want - oracle.numpy()).max() <= 1e-15
            _merge(worst, {name: HR.worst(y32, want, bound, name)})
    dw, dx = HR.fc_emulate_bwd(o)
    ref = HR.fc_ref(o, True)
    _merge(worst, {"dw": HR.worst(dw, HR.FC_DW_START + ref["dw"], ref["bound_dw"], "dw"), "dx": HR.worst(dx, ref["dx"], ref["bound_dx"], "dx")})
    print("FC (%d, %d, %d) emulation / bound: %s" % (B, fin, fout, "  ".join("%s %.3f" % kv for kv in worst.items())))
    assert max(worst.values()) <= 1.0, worst


def test_standalone_prelu_expression():
    for n in HR.PRELU_NS:
        assert n > 16384 * 256
    assert HR.PRELU_NS[1] % HR.PRELU_C == 0 and 256 % HR.PRELU_C != 0
    v, alpha = HR.prelu_inputs(4099)
    got = HR.prelu_expect(v, alpha)
    want = OL.prelu(torch.from_numpy(HR.f64(v)).reshape(-1, 1)[:4095].reshape(-1, HR.PRELU_C), torch.from_numpy(HR.f64(alpha))).numpy().ravel()
    assert (np.abs(got[:4095] - want) <= U * np.abs(want)).all()
    assert (v < 0).any() and (v > 0).any() and (alpha < 0).any()


# ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("mode", HR.PHONG_MODES)
def test_phong_reference_against_the_oracle(mode):
    img, light, col, albedo, wgt = HR.phong_inputs()
    B, H, W = HR.PHONG_SHAPE
    assert img.shape == (B, H, W, 3) and (H * W + 2047) // 2048 == 2                      # two workgroups per item
    ref = HR.phong_grads(mode, img, light, col, albedo, wgt)
    i, l, a = _t64(img), _t64(light), _t64(albedo)
    out = ORC.tf_phong_composite(i, l, _t64(col, False), HR.PHONG_AMBIENT, HR.PHONG_KD, with_black_background=mode == "tf_black",
                                 with_mask=mode != "none") * a
    gi, gl, ga = torch.autograd.grad((out * _t64(wgt, False)).sum(), [i, l, a])
    for k, want in (("out", out.detach()), ("dimg", gi), ("dlight", gl), ("dalbedo", ga)):
        _agree(ref[k], want.numpy(), 1e-12, k)
    if mode != "none":
        assert np.abs(ref["dimg"][1, 1]).max() > 1.0                                      # the mask gradient is in play
    worst = {}
    for fma in (False, True):
        _merge(worst, HR.phong_ratios(HR.phong_emulate_bwd(mode, img, light, col, albedo, wgt, fma=fma), ref, "emulation"))
    print("Phong %s emulation / bar: %s" % (mode, "  ".join("%s %.3f" % kv for kv in worst.items())))
    assert max(worst.values()) <= 1.0, worst


@pytest.mark.parametrize("row", HR.STRIDED_ROWS, ids=lambda r: BC.case_id((r,)))
def test_strided_rows_take_the_gather_kernel(row):
    from rendernet_amd import ops
    assert BC.routes_of(ops, row) == "direct direct direct"
    assert HR.strided_chunk(row[3]) == {3: 4, 5: 8}[row[3]] and row[3] % HR.strided_chunk(row[3]) != 0
    assert HR.strided_lds_bytes(row) <= 64 * 1024
    o = BC.layer_operands(row, 1)
    ref = BC.Reference(row, o)
    want = ref.grads(o["dy"])["dx"]
    # fp32 autograd over the oracle op (not the kernel's order) against the float64 reference, inside the project's bar
    x = torch.from_numpy(o["x"]).requires_grad_(True)
    z = getattr(OL, row[0])(x, torch.from_numpy(o["w"]), torch.from_numpy(o["b"]), row[6])
    y = OL.prelu(z, torch.from_numpy(o["alpha"])) if row[7] == "prelu" else z
    got, = torch.autograd.grad(y, [x], torch.from_numpy(o["dy"]))
    assert BC.ratio(got, want) <= BC.RTOL


def test_strided_refusal_case_exceeds_the_lds_budget():
    from rendernet_amd import ops
    assert BC.routes_of(ops, HR.STRIDED_OVER_LDS) == "direct direct direct"
    assert HR.strided_lds_bytes(HR.STRIDED_OVER_LDS) == 125 * 32 * 16 * 4 > 64 * 1024
