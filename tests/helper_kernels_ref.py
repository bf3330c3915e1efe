"""float64 references, seeded inputs, fp32 emulations and error bounds for the memory-bound helper kernels of
rendernet_amd/csrc/train_kernels.hip and misc_kernels.hip: epilogue backward, loss, Adam, SGD, fully connected forward / backward,
stand-alone PReLU, Phong backward.  A plain module (no test in it): tests/test_helper_kernels_ref_cpu.py pins the references against
autograd over the oracle ops and shows that an fp32 emulation of every kernel stays inside every bound on the inputs below;
tests/test_gpu_helper_kernels.py launches the kernels on the same inputs and asserts the same bounds.

A reference restates the OPERATION in float64 on the very fp32 operands the kernel receives.  Hyper-parameters are the fp32 values
that cross the ABI (np.float32(beta1); 1 - beta1 formed in fp32, as the kernel forms it); everything after that is float64.

The bounds.  u = 2^-24 is the unit roundoff of fp32: one correctly rounded operation (+, -, *, /, sqrt, fma) has a relative error <= u.
A bound counts the roundings on the path to one output and multiplies u by the magnitude they are relative to.  None is fitted to
what a kernel gives.

  epilogue dz          |got - ref| <= 4 u |ref|, no floor; ref == 0 implies got == 0.  At most four roundings, all on one product:
                       1 - y (or y + 1), y * (1 - y), * dy, * alpha.  The one subtraction is of fp32 inputs, so no rounded
                       quantity is ever cancelled.
  dbias, dalpha        the bars of tests/test_gpu_train.py: |got - (start + sum)| <= 2e-6 * max_c sum_rows |term| for dbias and
                       <= 2e-5 * max(max_c |start + sum|, 1) for dalpha, ACCUMULATED onto a non-zero start value.
  loss value           |got - ref| <= 2e-6 |ref| (the existing bar; the terms of one loss all have one sign).
  dpred, BCE           <= 6 u (t / a0 + (1 - t) / a1) / div: 1 - t, two quotients, their difference, fp32(1 / div) and the product
                       with it; the two quotients cancel, hence the sum of their magnitudes.  a0 = 1e-6 + p and
                       a1 = (1e-6 + 1) - p are formed in fp32 in the order of the original graph (RenderNet_Shader.py:160): at
                       p = 1 a1 is 9.54e-7 and not 1e-6, which is the defined behaviour.  log and the quotients are float64.
  dpred, MSE           <= 4 u |ref|: p - t, * 2 (exact), fp32(1 / div), the product.
  Adam m               <= 4 u (b1 |m| + (1 - b1) |g gs|): g * gs, (1 - b1) * that, b1 * m, the sum.
  Adam v               <= 5 u v_ref: g * gs counts twice (it is squared), two products, the sum; b2 * v has fewer.
  Adam p               <= u |p_ref| + 8 u |lr_t m / (sqrt(v) + eps)|: the last subtraction, and on the step the roundings of m (<= 4),
                       half those of v under the root (<= 2.5), the root, + eps, * lr_t, the quotient; in the worst case the list
                       adds up to a little more than 8, which needs every rounding at its maximum with one sign.  The step is
                       relative to |m_ref|, so the inputs keep b1 m and (1 - b1) g from cancelling (see adam_inputs).
  SGD                  <= u |p_ref| + 2 u |lr g|: the product and the subtraction (one rounding when contracted to an fma).
  FC pre-activation    <= (fin + 2) u (sum_k |x_k w_k| + |b|) per element: fin fma steps and the bias add.
  FC dw increment      <= (B + 2) u (sum_b |x_b dz_b| + |start|), onto a buffer that held `start`: B fma steps in chunks of 8 rows
                       and one add onto dw per chunk (B + ceil(B / 8) roundings: within B + 2 up to B = 16, one more at B = 17,
                       where the form is kept as it is -- reaching it would need every rounding at its maximum with one sign).
  FC dx                <= (fout + 2 + 8) u sum_col |dz_col w_col|: the 8 is for the wave butterfly and the LDS sum, whose order is not
                       the column order.
  activations          against the float64 activation of the kernel's OWN fp32 pre-activation:
                       PReLU 1 u relative (one term is zero, one product);
                       ELU 2^-22 + u |ref| (expf(z) - 1 cancels near 0: absolute, in units of exp <= 1);
                       sigmoid 2^-20 absolute for |z| <= 16 (the fast exponential scales its argument: ~|z| 6e-8 relative on exp, at
                       most a quarter of that on the output).  fc_inputs keeps |z| <= 16.
  stand-alone PReLU    bit-equal to the fp32 expression max(v, 0) + alpha * min(v, 0): one term is always zero.
  Phong backward       the bars of tests/test_gpu_reconstruct.py: 2e-4 max|ref| + 1e-6 for dimg and dlight, 1e-5 for dalbedo.
  strided dgrad        tests/backward_cases.py RTOL (2e-4 of max|ref|, no floor).

The fp32 emulations follow each kernel's operation order with np.float32 arithmetic; where hipcc's default contraction may fuse a
product into the following sum the emulation is run both ways (fma = one rounding of the exact a * b + c, formed in float64, where
the 48-bit product is exact).  Sums over rows are emulated in the launcher's row-block order.
"""
import os
import sys
import zlib

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from rendernet_amd._lib import RN_E_INVALID, RN_E_UNSUPPORTED  # noqa: E402,F401

F32, F64 = np.float32, np.float64
U = 2.0 ** -24
ACT_PRELU, ACT_SIGMOID, ACT_ELU = 1, 2, 4

DBIAS_BAR, DALPHA_BAR, LOSS_BAR = 2e-6, 2e-5, 2e-6
PHONG_RTOL, PHONG_ATOL, PHONG_DALBEDO = 2e-4, 1e-6, 1e-5
ELU_ABS, SIGMOID_ABS, SIGMOID_MAX_Z = 2.0 ** -22, 2.0 ** -20, 16.0


def _rng(*key):
    return np.random.default_rng(zlib.crc32(repr(key).encode()))


def f64(a):
    return np.asarray(a, F32).astype(F64)


def fma32(a, b, c):
    """One fp32 fma: the product of two fp32 numbers is exact in float64; the sum is rounded to float64 and then to fp32."""
    return (np.asarray(a, F32).astype(F64) * np.asarray(b, F32).astype(F64) + np.asarray(c, F32).astype(F64)).astype(F32)


def worst(got, ref, bound, what=""):
    """max (|got - ref| / bound) over the elements with bound > 0; where the bound is 0 the values must be equal."""
    got, ref, bound = np.asarray(got, F64), np.asarray(ref, F64), np.broadcast_to(np.asarray(bound, F64), np.shape(ref))
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert np.isfinite(got).all(), "%s: non-finite values" % what
    err = np.abs(got - ref)
    zero = bound == 0
    assert (err[zero] == 0).all(), "%s: %d elements differ where the bound is zero" % (what, int((err[zero] != 0).sum()))
    return float((err[~zero] / bound[~zero]).max()) if (~zero).any() else 0.0


# ---------------------------------------------------------------------------------------------
# epilogue backward

EPI_CASES = [(65573, 32, 1), (1031, 2048, 1), (1000, 8, 4), (1000, 3, 4), (1000, 20, 5), (1, 4, 1), (3, 4, 3), (777, 1024, 1)]
EPI_REFUSED = (300, 1028, 1)
EPI_START_B, EPI_START_A = 0.5, -0.25


def epi_geometry(M, C):
    """The launch geometry rn_epilogue_bwd chooses (restated from the launcher, for the emulation's row-block order and for the
    CPU test that pins which branch a case reaches)."""
    G = C // 4
    if C % 4 == 0 and ((G <= 256 and 256 % G == 0) or G % 256 == 0):
        NT = 1024 if M * C >= (2 << 20) else 256
        gper = min(G, 256)
        rstep = NT // gper
        rpb = max(-(-(-(-M // 512)) // (4 * rstep)) * 4 * rstep, 4 * rstep)
        nb = -(-M // rpb)
        return {"path": "vec", "NT": NT, "G": G, "gy": 1 if G <= 256 else G // 256, "rstep": rstep, "rpb": rpb, "nb": nb,
                "two_stage": nb >= 32 and nb * 2 * C <= 512 * 2 * C}
    if C > 1024:
        return {"path": "refused"}
    rpb = max(-(-M // 4096), 256)
    return {"path": "gen", "rpb": rpb, "nb": -(-M // rpb), "two_stage": False}


def _elu64(z):
    return np.where(z > 0, z, np.expm1(np.minimum(z, 0)))


def epi_inputs(M, C, act):
    """dy, z ~ N(0,1); slopes in (0.05, 0.3); y the fp32 output of the forward epilogue the flags describe."""
    rng = _rng("epi", M, C, act)
    dy, z = rng.standard_normal((M, C)).astype(F32), rng.standard_normal((M, C)).astype(F32)
    alpha = rng.uniform(0.05, 0.3, C).astype(F32)
    t = f64(z)
    if act & ACT_PRELU:
        t = np.where(z > 0, t, f64(alpha) * t)
    y = None
    if act & ACT_ELU:
        y = _elu64(t).astype(F32)
    if act & ACT_SIGMOID:
        y = (1.0 / (1.0 + np.exp(-t))).astype(F32)
    return {"dy": dy, "z": z, "y": y, "alpha": alpha}


def epi_ref(o, act):
    """dz, the per-channel sums and sum |term| of dbias in float64.  PReLU branches from z > 0 on the fp32 z itself."""
    d = f64(o["dy"])
    if act & ACT_SIGMOID:
        y = f64(o["y"])
        d = d * (y * (1.0 - y))
    if act & ACT_ELU:
        y = f64(o["y"])
        d = np.where(o["y"] < 0, d * (y + 1.0), d)
    da = np.zeros(d.shape[1])
    if act & ACT_PRELU:
        da = (d * np.minimum(f64(o["z"]), 0.0)).sum(0)
        d = np.where(o["z"] > 0, d, d * f64(o["alpha"]))
    return {"dz": d, "dbias": d.sum(0), "dalpha": da, "abs_b": np.abs(d).sum(0)}


def _rows_in_blocks32(t, rpb, start):
    """Per-channel fp32 sum of t [M, C]: sequential inside each block of rpb rows, then block after block onto `start`."""
    M, C = t.shape
    nb = -(-M // rpb)
    pad = np.zeros((nb * rpb, C), F32)
    pad[:M] = t
    part = np.add.accumulate(pad.reshape(nb, rpb, C), axis=1, dtype=F32)[:, -1]
    acc = np.full(C, start, F32)
    for b in range(nb):
        acc = (acc + part[b]).astype(F32)
    return acc


def epi_emulate(o, act, M, C):
    """fp32 arithmetic of epilogue_bwd_*_kernel: dz element by element, the sums in row-block order onto the start values."""
    d = o["dy"].copy()
    one = F32(1)
    if act & ACT_SIGMOID:
        d = d * (o["y"] * (one - o["y"]))
    if act & ACT_ELU:
        d = np.where(o["y"] < 0, d * (o["y"] + one), d)
    rpb = epi_geometry(M, C)["rpb"]
    da = np.full(C, EPI_START_A, F32)
    if act & ACT_PRELU:
        da = _rows_in_blocks32(d * np.minimum(o["z"], F32(0)), rpb, EPI_START_A)
        d = np.where(o["z"] > 0, d, d * o["alpha"])
    assert d.dtype == F32
    return {"dz": d, "dbias": _rows_in_blocks32(d, rpb, EPI_START_B), "dalpha": da}


def epi_ratios(got_dz, got_db, got_da, ref, act, what):
    """observed / bound for dz (None: not produced), dbias and dalpha (None: not asked for) accumulated onto the start values."""
    out = {}
    if got_dz is not None:
        out["dz"] = worst(got_dz, ref["dz"], 4 * U * np.abs(ref["dz"]), what + " dz")
    if got_db is not None:
        out["dbias"] = worst(got_db, EPI_START_B + ref["dbias"], DBIAS_BAR * ref["abs_b"].max(), what + " dbias")
    if got_da is not None:
        want = EPI_START_A + ref["dalpha"]
        out["dalpha"] = worst(got_da, want, DALPHA_BAR * max(np.abs(want).max(), 1.0), what + " dalpha")
    return out


# ---------------------------------------------------------------------------------------------
# loss

LOSS_N = 3 * 2048 * 256 + 17
LOSS_START = 3.25
_EDGE_P = np.array([0.0, 1.0, 1e-7, 1.0 - 2.0 ** -24], F32)


def loss_local_divisor(mode, n):
    return 3.0 if mode == 0 else float(n)


def loss_inputs(mode, n=LOSS_N):
    """p in (0.001, 0.999), t in (0, 1); BCE: the first eight elements are p in {0, 1, 1e-7, 1 - 2^-24} x t in {0, 1}."""
    rng = _rng("loss", mode, n)
    p = rng.uniform(0.001, 0.999, n).astype(F32)
    t = rng.uniform(0, 1, n).astype(F32)
    if mode == 0:
        p[:8] = np.tile(_EDGE_P, 2)
        t[:8] = np.repeat(np.array([0, 1], F32), 4)
    return p, t


def loss_ref(p, t, mode, div):
    """loss, dpred and the bound on dpred, float64; BCE's a0 / a1 in fp32 first (module docstring)."""
    div = float(div)
    if mode == 0:
        a0 = f64(F32(1e-6) + p)
        a1 = f64((F32(1e-6) + F32(1)) - p)
        tt = f64(t)
        loss = -(tt * np.log(a0) + (1.0 - tt) * np.log(a1)).sum() / div
        dp = -(tt / a0 - (1.0 - tt) / a1) / div
        return loss, dp, 6 * U * (tt / a0 + (1.0 - tt) / a1) / div
    d = f64(p) - f64(t)
    dp = 2.0 * d / div
    return (d * d).sum() / div, dp, 4 * U * np.abs(dp)


def loss_emulate(p, t, mode, div, fma=False):
    """fp32 arithmetic of loss_kernel; the running sum is a double there and here."""
    inv = F32(1.0 / float(div))
    one = F32(1)
    if mode == 0:
        a0, a1 = F32(1e-6) + p, (F32(1e-6) + one) - p
        l0, l1 = np.log(a0), np.log(a1)
        assert l0.dtype == F32
        term = -(fma32(t, l0, (one - t) * l1) if fma else (t * l0 + (one - t) * l1))
        dp = -(t / a0 - (one - t) / a1) * inv
    else:
        d = p - t
        term = d * d
        dp = F32(2) * d * inv
    assert dp.dtype == F32 and term.dtype == F32
    return float(term.astype(F64).sum() * float(inv)), dp


# ---------------------------------------------------------------------------------------------
# Adam and SGD

ADAM_NS = (1, 3, 4, 7, 1024, 100003)
ADAM_GRAD_SCALES = (1.0, 0.125)
ADAM_HYPER = {"lr_t": F32(1.7e-3), "b1": F32(0.9), "b2": F32(0.999), "eps": F32(1e-8)}
SGD_NS = (1, 255, 4096 * 256 + 5)
SGD_LR = F32(0.05)


def adam_inputs(n):
    """A random non-zero state (p, m, v) and a gradient of magnitude 1e-3 .. 1e1.  Even elements: g has the sign of m.  Odd elements: g
    has the other sign and (1 - b1) |g| <= 0.012 b1 |m| (|g| in 1e-3 .. 1e-2, |m| in 0.1 .. 1), so that m_new never loses more than
    1.2 % of b1 |m| to cancellation: the bound on p is relative to |m_new|, which no fp32 evaluation could meet on a cancelled m.
    Every fifth element from index 2 has g = 0: m and v decay, p moves by lr_t b1 m / (sqrt(b2 v) + eps)."""
    rng = _rng("adam", n)
    i = np.arange(n)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    odd = i % 2 == 1
    m = sign * 10.0 ** np.where(odd, rng.uniform(-1, 0, n), rng.uniform(-3, 0, n))
    g = np.where(odd, -sign, sign) * 10.0 ** np.where(odd, rng.uniform(-3, -2, n), rng.uniform(-3, 1, n))
    g[i % 5 == 2] = 0.0
    v = (10.0 ** rng.uniform(-3, 1, n)) ** 2
    return {"p": rng.standard_normal(n).astype(F32), "m": m.astype(F32), "v": v.astype(F32), "g": g.astype(F32)}


def adam_ref(o, gs, h=ADAM_HYPER):
    b1, b2, lr_t, eps = (float(h[k]) for k in ("b1", "b2", "lr_t", "eps"))
    c1, c2 = float(F32(1) - h["b1"]), float(F32(1) - h["b2"])              # 1 - beta formed in fp32, as the kernel forms it
    gq = f64(o["g"]) * float(F32(gs))
    m = b1 * f64(o["m"]) + c1 * gq
    v = b2 * f64(o["v"]) + c2 * gq * gq
    step = lr_t * m / (np.sqrt(v) + eps)
    p = f64(o["p"]) - step
    return {"m": m, "v": v, "p": p, "step": step,
            "bound_m": 4 * U * (b1 * np.abs(f64(o["m"])) + c1 * np.abs(gq)), "bound_v": 5 * U * v,
            "bound_p": U * np.abs(p) + 8 * U * np.abs(step)}


def adam_emulate(o, gs, fma=False, h=ADAM_HYPER):
    b1, b2, lr_t, eps = h["b1"], h["b2"], h["lr_t"], h["eps"]
    one = F32(1)
    gq = o["g"] * F32(gs)
    if fma:
        m = fma32(b1, o["m"], (one - b1) * gq)
        v = fma32(b2, o["v"], (one - b2) * gq * gq)
    else:
        m = b1 * o["m"] + (one - b1) * gq
        v = b2 * o["v"] + (one - b2) * gq * gq
    p = o["p"] - lr_t * m / (np.sqrt(v) + eps)
    assert m.dtype == F32 and v.dtype == F32 and p.dtype == F32
    return {"m": m, "v": v, "p": p}


def adam_ratios(got, ref, what):
    return {k: worst(got[k], ref[k], ref["bound_" + k], "%s %s" % (what, k)) for k in ("m", "v", "p")}


def sgd_inputs(n):
    rng = _rng("sgd", n)
    return rng.standard_normal(n).astype(F32), (rng.standard_normal(n) * 10.0 ** rng.uniform(-3, 1, n)).astype(F32)


def sgd_ref(p, g, lr=SGD_LR):
    step = float(lr) * f64(g)
    out = f64(p) - step
    return out, U * np.abs(out) + 2 * U * np.abs(step)


def sgd_emulate(p, g, fma=False, lr=SGD_LR):
    return fma32(-lr, g, p) if fma else p - lr * g


# ---------------------------------------------------------------------------------------------
# fully connected

FC_CASES = [(1, 1, 1), (8, 37, 255), (9, 37, 257), (17, 199, 300), (5, 3, 1024)]
FC_ACTS = {"none": 0, "prelu": ACT_PRELU, "elu": ACT_ELU, "sigmoid": ACT_SIGMOID}
FC_DW_START = 0.25


def fc_inputs(B, fin, fout):
    rng = _rng("fc", B, fin, fout)
    lim = np.sqrt(6.0 / (fin + fout))
    return {"x": rng.standard_normal((B, fin)).astype(F32), "w": rng.uniform(-lim, lim, (fin, fout)).astype(F32),
            "b": (0.1 * rng.standard_normal(fout)).astype(F32), "alpha": rng.uniform(0.05, 0.3, fout).astype(F32),
            "dz": rng.standard_normal((B, fout)).astype(F32)}


def fc_ref(o, bias):
    x, w, dz = f64(o["x"]), f64(o["w"]), f64(o["dz"])
    b = f64(o["b"]) if bias else np.zeros(w.shape[1])
    B, fin = x.shape
    fout = w.shape[1]
    return {"z": x @ w + b, "bound_z": (fin + 2) * U * (np.abs(x) @ np.abs(w) + np.abs(b)),
            "dw": x.T @ dz, "bound_dw": (B + 2) * U * (np.abs(x).T @ np.abs(dz) + FC_DW_START),
            "dx": dz @ w.T, "bound_dx": (fout + 2 + 8) * U * (np.abs(dz) @ np.abs(w).T)}


def act_ref(z32, alpha, act):
    """float64 activation of an fp32 pre-activation, and the bound an fp32 evaluation is held to."""
    z = f64(z32)
    if act == ACT_PRELU:
        y = np.where(z32 > 0, z, f64(alpha) * z)
        return y, U * np.abs(y)
    if act == ACT_ELU:
        y = _elu64(z)
        return y, ELU_ABS + U * np.abs(y)
    if act == ACT_SIGMOID:
        assert np.abs(z).max() <= SIGMOID_MAX_Z
        return 1.0 / (1.0 + np.exp(-z)), np.full(z.shape, SIGMOID_ABS)
    return z, np.zeros(z.shape)


def fc_emulate_fwd(o, bias, act):
    """fc_kernel: an fma chain over k, + bias, the activation; returns (preact, y) in fp32."""
    x, w = o["x"], o["w"]
    acc = np.zeros((x.shape[0], w.shape[1]), F32)
    for k in range(x.shape[1]):
        acc = fma32(x[:, k:k + 1], w[k:k + 1, :], acc)
    z = acc + (o["b"] if bias else F32(0))
    zero, one = F32(0), F32(1)
    y = z
    if act == ACT_PRELU:
        y = np.maximum(z, zero) + o["alpha"] * np.minimum(z, zero)
    elif act == ACT_ELU:
        y = np.where(z > 0, z, np.exp(np.minimum(z, zero)) - one)
    elif act == ACT_SIGMOID:
        y = one / (one + np.exp(-z))
    assert z.dtype == F32 and y.dtype == F32
    return z, y


def fc_emulate_bwd(o):
    """fc_wgrad_kernel (fma chains over chunks of 8 batch rows, each added onto dw) and fc_dgrad_kernel (256 column lanes, wave
    butterfly, the four waves summed left to right)."""
    x, w, dz = o["x"], o["w"], o["dz"]
    B, fin = x.shape
    fout = w.shape[1]
    dw = np.full((fin, fout), FC_DW_START, F32)
    for b0 in range(0, B, 8):
        s = np.zeros((fin, fout), F32)
        for b in range(b0, min(b0 + 8, B)):
            s = fma32(x[b][:, None], dz[b][None, :], s)
        dw = dw + s
    lanes = np.zeros((B, fin, 256), F32)
    for c0 in range(0, fout, 256):
        n = min(256, fout - c0)
        lanes[:, :, :n] = fma32(dz[:, None, c0:c0 + n], w[None, :, c0:c0 + n], lanes[:, :, :n])
    v = lanes.reshape(B, fin, 4, 64)
    idx = np.arange(64)
    for s in (32, 16, 8, 4, 2, 1):
        v = v + v[..., idx ^ s]
    r = v[..., 0]
    dx = ((r[..., 0] + r[..., 1]) + r[..., 2]) + r[..., 3]
    assert dw.dtype == F32 and dx.dtype == F32
    return dw, dx


# ---------------------------------------------------------------------------------------------
# stand-alone PReLU

PRELU_C = 5
PRELU_NS = (16384 * 256 * 1 + 3 * 5, 16384 * 256 + 1)      # past the grid cap; the second one is a multiple of C = 5


def prelu_inputs(n, C=PRELU_C):
    rng = _rng("prelu", n, C)
    return rng.standard_normal(n).astype(F32), rng.uniform(-0.3, 0.3, C).astype(F32)


def prelu_expect(v, alpha):
    """The fp32 expression of the kernel: bit-equal is demanded (alpha indexed by element % C)."""
    a = alpha[np.arange(v.size) % alpha.size]
    out = np.maximum(v, F32(0)) + a * np.minimum(v, F32(0))
    assert out.dtype == F32
    return out


# ---------------------------------------------------------------------------------------------
# Phong composite

PHONG_SHAPE = (2, 47, 45)             # 2115 pixels: two workgroups per item
# The masked flavour is tf_black.  dalbedo = dout * shading carries the bar 1e-5 ABSOLUTE, and in the mask's transition band the
# shading moves by 0.25 (1 - ambient - D) <= 0.23 per unit of the sigmoid's argument 255 s - 80.  tf_black has s = |img| ~ 0.31:
# about 1.5 roundings on the norm and one on the product, each u * 80 -> 1.2e-5 on the argument, 2.8e-6 on the shading, 8e-6 with
# |dout| up to 3: inside the bar in the worst case.  tf_white has s = sqrt(3) - |img| with |img| ~ 1.42: the norm's rounding is
# not reduced by the subtraction, 255 * 1.5 u * 1.42 = 3.2e-5 on the argument and up to 2.5e-5 on dalbedo -- no fp32 evaluation is
# inside 1e-5 there in the worst case (tests/test_gpu_reconstruct.py covers tf_white on a shorter band).
PHONG_MODES = ("tf_black", "none")
PHONG_CODES = {"tf_black": 2, "tf_white": 3, "none": 4}
PHONG_AMBIENT, PHONG_KD = 0.1, 0.9


def phong_inputs(seed=0, B=PHONG_SHAPE[0], H=PHONG_SHAPE[1], W=PHONG_SHAPE[2]):
    """The recipe of tests/test_gpu_reconstruct.py's _phong_inputs at another size: uniform normals with a band of pixels on the
    transition of the tf_white mask (item 0) and of the tf_black mask (item 1)."""
    rng = np.random.default_rng(seed)
    img = rng.uniform(0.02, 0.98, (B, H, W, 3)).astype(F32)
    img[0, 0, :] = np.linspace(0.815, 0.822, W, dtype=F32)[:, None]
    img[1, 1, :] = np.linspace(0.17, 0.20, W, dtype=F32)[:, None]
    light = rng.standard_normal((B, 3)).astype(F32)
    col = rng.uniform(0.5, 1.0, (B, 3)).astype(F32)
    albedo = rng.uniform(0, 1, (B, H, W, 3)).astype(F32)
    wgt = np.random.default_rng(9).standard_normal(img.shape).astype(F32)
    return img, light, col, albedo, wgt


def phong_forward(mode, img, light, col, albedo, ambient=PHONG_AMBIENT, kd=PHONG_KD):
    """The composite of include/rendernet_hip.h restated with torch ops in the dtype of its arguments (the TF flavours and none)."""
    n = img - 0.5
    n = n / torch.sqrt((n * n).sum(-1, keepdim=True))
    l = light / torch.sqrt((light * light).sum(-1, keepdim=True))
    d = torch.clamp_min((n * l[:, None, None, :]).sum(-1, keepdim=True), 0.0)
    diffuse = torch.clamp(kd * (d * col[:, None, None, :]), 0.0, 1.0)
    if mode == "none":
        comp = ambient + diffuse
    else:
        s = torch.sqrt((img * img).sum(-1, keepdim=True))
        if mode == "tf_white":
            s = 3.0 ** 0.5 - s
        else:
            assert mode == "tf_black"
        mask = torch.sigmoid(255.0 * s - 80.0)
        comp = mask * (ambient + diffuse) + (1.0 - mask)
    out = torch.clamp(comp, 0.0, 1.0)
    return out if albedo is None else out * albedo


def phong_grads(mode, img, light, col, albedo, wgt):
    """out and the gradients of sum(out * wgt) w.r.t. the normal map, the light and the albedo, by float64 autograd."""
    t = lambda a, g=True: torch.from_numpy(np.ascontiguousarray(a)).double().requires_grad_(g)
    i, l, a = t(img), t(light), t(albedo)
    out = phong_forward(mode, i, l, t(col, False), a)
    gi, gl, ga = torch.autograd.grad((out * t(wgt, False)).sum(), [i, l, a])
    return {"out": out.detach().numpy(), "dimg": gi.numpy(), "dlight": gl.numpy(), "dalbedo": ga.numpy()}


def phong_emulate_bwd(mode, img, light, col, albedo, dout, ambient=PHONG_AMBIENT, kd=PHONG_KD, fma=False):
    """fp32 arithmetic of phong_eval + phong_bwd_kernel, pixel by pixel in the kernel's order (fma: the mask argument 255 s - 80
    as one fma, the contraction that matters); dlight is summed per item in fp32 pixel order."""
    one, zero, half = F32(1), F32(0), F32(0.5)
    ambient, kd = F32(ambient), F32(kd)
    B = img.shape[0]
    r, g, bl = (img[..., c].reshape(B, -1) for c in range(3))
    go = dout.reshape(B, -1, 3)
    alb = albedo.reshape(B, -1, 3)
    lx, ly, lz = (light[:, c:c + 1] for c in range(3))
    ln = np.sqrt(lx * lx + ly * ly + lz * lz)
    lx, ly, lz = lx / ln, ly / ln, lz / ln
    vx, vy, vz = r - half, g - half, bl - half
    nn = np.sqrt(vx * vx + vy * vy + vz * vz)
    nx, ny, nz = vx / nn, vy / nn, vz / nn
    dot = nx * lx + ny * ly + nz * lz
    d = np.maximum(dot, zero)
    masked = mode != "none"
    if masked:
        nrm = np.sqrt(r * r + g * g + bl * bl)
        s = F32(1.7320508075688772) - nrm if mode == "tf_white" else nrm
        arg = fma32(F32(255), s, F32(-80)) if fma else F32(255) * s - F32(80)
        m = one / (one + np.exp(-arg))
    dalbedo = np.zeros_like(go)
    dd = np.zeros_like(r)
    dm = np.zeros_like(r)
    for c in range(3):
        dc = kd * (d * col[:, c:c + 1])
        D = np.minimum(np.maximum(dc, zero), one)
        comp = m * (ambient + D) + (one - m) if masked else ambient + D
        sh = np.minimum(np.maximum(comp, zero), one)
        dalbedo[..., c] = go[..., c] * sh
        gc = np.where((comp >= 0) & (comp <= 1), go[..., c] * alb[..., c], zero)
        if masked:
            dm = dm + gc * (ambient + D - one)
        gD = gc * m if masked else gc
        dd = dd + np.where((dc >= 0) & (dc <= 1), gD * kd * col[:, c:c + 1], zero)
    gdot = np.where(dot > 0, dd, zero)
    gi = [gdot * (lx - nx * dot) / nn, gdot * (ly - ny * dot) / nn, gdot * (lz - nz * dot) / nn]
    if masked:
        f = (F32(255) * dm * m * (one - m)) * (F32(-1) if mode == "tf_white" else one) / nrm
        gi = [gi[0] + f * r, gi[1] + f * g, gi[2] + f * bl]
    gl = [np.add.accumulate(gdot * n_, axis=1, dtype=F32)[:, -1:] for n_ in (nx, ny, nz)]
    ldg = lx * gl[0] + ly * gl[1] + lz * gl[2]
    dlight = np.concatenate([(gl[0] - lx * ldg) / ln, (gl[1] - ly * ldg) / ln, (gl[2] - lz * ldg) / ln], axis=1)
    dimg = np.stack(gi, axis=-1).reshape(img.shape)
    assert dimg.dtype == F32 and dlight.dtype == F32 and dalbedo.dtype == F32
    return {"dimg": dimg, "dlight": dlight, "dalbedo": dalbedo.reshape(img.shape)}


def phong_ratios(got, ref, what):
    """observed / bar for dimg, dlight (got may be onto a start value the caller subtracted) and dalbedo."""
    out = {}
    for k in ("dimg", "dlight"):
        out[k] = worst(got[k], ref[k], PHONG_RTOL * np.abs(ref[k]).max() + PHONG_ATOL, "%s %s" % (what, k))
    out["dalbedo"] = worst(got["dalbedo"], ref["dalbedo"], PHONG_DALBEDO, what + " dalbedo")
    return out


# ---------------------------------------------------------------------------------------------
# strided input gradient (rows in the format of tests/backward_cases.py)

STRIDED_ROWS = [("conv2d", 2, (7, 9), 3, 8, 3, (2, 2), "res"),                 # Cin <= 4: 4 input channels per thread
                ("conv3d", 2, (5, 7, 6), 5, 8, 5, (2, 2, 2), "prelu")]         # Cin = 5: a ragged chunk of 8 (the texture stem)
STRIDED_OVER_LDS = ("conv3d", 1, (4, 4, 4), 16, 32, 5, (2, 2, 2), "res")       # 125 taps x 32 x 16 floats = 250 KiB staged: refused


def strided_chunk(Cin):
    return 4 if Cin <= 4 else 8 if Cin <= 8 else 16


def strided_lds_bytes(row):
    _, _, sp, Cin, Cout, k, _, _ = row
    return k ** len(sp) * Cout * strided_chunk(Cin) * 4
