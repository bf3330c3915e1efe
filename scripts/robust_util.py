"""Hostile input statistics and scheme-forcing harness for the Winograd robustness suite (scripts/wino_robustness.py,
tests/test_gpu_wino_robust.py).  Test / measurement infrastructure: nothing on the product path imports it.

The layer under test is the res2 conv of the reference (3x3, SAME, C -> C; tools/layer_util.py:91-105,
RenderNet_Shader.py:71-84).  `hostile_inputs` yields (name, x, w, b) with activations that look like what a TRAINED
net feeds that layer rather than like N(0,1): post-PReLU outputs have a large positive mean and heavy per-channel tails --
the known bad case for large-tile Winograd, whose transforms subtract neighbouring pixels of equal magnitude."""
import functools

import numpy as np
import torch

from rendernet_amd import ops
from rendernet_amd import _lib as L

SCHEMES = ("direct", "f22", "f43", "f63", "f43s", "f63s", "f43h", "f63h")      # ...s: the split (bf16x3) GEMM stage of the same scheme; ...h: fp16x2


def xavier(rng, shape):
    rf = int(np.prod(shape[:-2]))
    lim = np.sqrt(6.0 / ((shape[-2] + shape[-1]) * rf))
    return rng.uniform(-lim, lim, shape).astype(np.float32)


def hostile_inputs(rng, B, H, W, Cin, Cout):
    w = xavier(rng, (3, 3, Cin, Cout))
    b = (0.1 * rng.standard_normal(Cout)).astype(np.float32)
    n = lambda: rng.standard_normal((B, H, W, Cin)).astype(np.float32)
    yield "N(0,1) inputs, Xavier filter (round-2 statistics)", n(), w, b
    yield "abs(N(0,1)) + 3 inputs (post-PReLU-like positive mean)", (np.abs(n()) + 3.0).astype(np.float32), w, b
    yield "abs(N(0,1)) + 30 inputs (mean 30x the spread)", (np.abs(n()) + 30.0).astype(np.float32), w, b
    gains = np.exp(1.5 * rng.standard_normal(Cin)).astype(np.float32)
    yield "abs(N(0,1)) x log-normal(sigma 1.5) per-channel gains", (np.abs(n()) * gains).astype(np.float32), w, b
    sparse = n() * (rng.random((B, H, W, Cin)) < 0.02)
    yield "2 % sparse spikes x 100 on a +1 floor", (1.0 + 100.0 * np.abs(sparse)).astype(np.float32), w, b
    x = (np.abs(n()) + 3.0).astype(np.float32)
    y = np.abs(x).max() * np.abs(w).sum(axis=(0, 1, 2)).max()
    yield "abs(N)+3 inputs, filter scaled so that outputs reach +-8", x, (w * np.float32(64.0 / y)).astype(np.float32), b
    wp = (np.abs(w) * 0.5 + w * 0.5).astype(np.float32)      # mostly positive filter: no cancellation in y, outputs ~ mean * sum|w|
    yield "abs(N)+3 inputs, 75 % positive filter (large outputs)", x, wp, b


def hostile_gradients(rng, shape):
    """(name, dz) for dz of `shape` = (B, H, W, C) with what a training step feeds a layer's backward instead of N(0,1): tiny, sparse,
    and differing by orders of magnitude between the images of a batch and between positions."""
    B, H, W, C = shape
    n = lambda: rng.standard_normal(shape).astype(np.float32)
    yield "N(0,1) x 1e-7", (n() * np.float32(1e-7)).astype(np.float32)
    yield "1 % sparse, x 1e-6", (n() * (rng.random(shape) < 0.01) * np.float32(1e-6)).astype(np.float32)
    g = n().astype(np.float64)
    yield "per-channel zero mean, x 1e-7", ((g - g.mean(axis=(0, 1, 2), keepdims=True)) * 1e-7).astype(np.float32)
    gain = np.ones((B, 1, 1, 1), np.float32)
    gain[0] = 2.0 ** 20
    yield "one image with gain 2^20 over the other, x 1e-9", (n() * gain * np.float32(1e-9)).astype(np.float32)
    pos = np.exp2(20.0 * rng.random((B, H, W, 1))).astype(np.float32)
    yield "2^20 range across positions (log-uniform), x 1e-9", (n() * pos * np.float32(1e-9)).astype(np.float32)


def conv_with_scheme(x, w, b, scheme, alpha=None, residual=None):
    """x [B,H,W,Cin], w [3,3,Cin,Cout] HIP tensors -> conv through the kernel family `scheme` forces."""
    pw = ops.pack_conv(w)
    split = {"s": "split", "h": "split16"}.get(scheme[-1]) if scheme[-1] in "sh" and scheme[:-1] in ("f43", "f63") else None
    if split:
        scheme = scheme[:-1]
    if scheme == "direct":
        pw.wino43 = None
        pw.wino = None
    elif scheme == "f22":
        pw.wino43 = None
        assert pw.wino is not None
    elif scheme == "f43":
        pw.wino63 = None
        assert pw.has("wino43")
    elif scheme == "f63":
        assert pw.has("wino63")
        pw.force_scheme = "f63"
    else:
        raise ValueError(scheme)
    with torch.no_grad(), ops.gemm_mode(split or "f32"):
        return ops.conv2d(x, pw, b, alpha, residual)


def res_stack_weights(rng, C, n_blocks=10):
    """10 res_block_2d + the res2_skip conv: 21 3x3 convs.  Biases positive and PReLU slopes small so that activations carry a
    positive mean from block to block (what trained nets do)."""
    blocks = []
    for _ in range(n_blocks):
        blk = []
        for _ in range(2):
            blk.append((xavier(rng, (3, 3, C, C)), (0.05 + 0.05 * rng.random(C)).astype(np.float32),
                        rng.uniform(0.0, 0.25, C).astype(np.float32)))
        blocks.append(blk)
    skip = (xavier(rng, (3, 3, C, C)), (0.05 * rng.random(C)).astype(np.float32))
    return blocks, skip


def _prelu64(x, a):
    return torch.clamp(x, min=0) + torch.as_tensor(a).double() * torch.clamp(x, max=0)


def res_stack_f64(x0, net, conv_f64):
    """x + conv(prelu(conv(x))) x 10, then conv + shortcut (tools/layer_util.py:91-105, RenderNet_Shader.py:71-84), float64."""
    blocks, skip = net
    x = torch.as_tensor(x0).double()
    short = x
    for (w1, b1, a1), (w2, b2, _a2) in blocks:
        x = x + conv_f64(_prelu64(conv_f64(x, w1, b1), a1), w2, b2)
    return conv_f64(x, skip[0], skip[1]) + short


def res_stack_gpu(x0, net, scheme):
    blocks, skip = net
    d = lambda a: torch.as_tensor(a).cuda()
    x = x0
    for (w1, b1, a1), (w2, b2, _a2) in blocks:
        h = conv_with_scheme(x, d(w1), d(b1), scheme, alpha=d(a1))
        x = conv_with_scheme(h, d(w2), d(b2), scheme, residual=x)
    return conv_with_scheme(x, d(skip[0]), d(skip[1]), scheme, residual=x0)


# ------------------------------------------------------------------------------------------------------------------------------
# the backward of the wide 2-D layers on hostile statistics (tests/test_gpu_backward_robust.py, scripts/backward_robustness.py)
# ------------------------------------------------------------------------------------------------------------------------------
BACKWARD_LAYERS = {"3x3 512->512": (3, 512, 512), "4x4 512->256": (4, 512, 256)}      # name -> (k, Cin, Cout); B = 2 on a 24 x 24 map:
BACKWARD_MAP = (2, 24, 24)                                                             # ragged F(6x6) tiles, cheap float64
X_CASES = (1, 2, 4)                                                                    # of hostile_inputs
# every route the filter gradient of such a layer can be forced onto (ops._wgrad_route names) ...
WGRAD_ROUTES = {3: ("direct", "wino2", "wino43", "wino3l_split"), 4: ("direct", "wino44", "wino3l_split")}
# ... and every launch its input gradient can: the scheme, then its multiply stage ("": exact fp32, "s": bf16x3, "h": fp16x2)
DGRAD_SCHEMES = {3: ("direct", "f22", "f43", "f43s", "f43h", "f63", "f63s", "f63h"), 4: ("direct", "f22x4", "f44", "f44s", "f44h")}
_STAGE = {"s": "split", "h": "split16"}
GRAD_BAR = 2e-4          # the project's gradient bar, purely relative: max|got - f64| <= GRAD_BAR * max|f64|


def _same_pads(k):
    return (k - 1) // 2, (k - 1) - (k - 1) // 2          # TF SAME at stride 1: 3 -> (1, 1), 4 -> (1, 2)


def wgrad_f64(x, dz, k):
    """float64 filter gradient [k,k,Cin,Cout] of the stride-1 SAME conv: dw[i,j] = sum over positions of x_pad[.., h+i, w+j, :]^T dz[.., h, w, :]."""
    x, dz = torch.as_tensor(x).double(), torch.as_tensor(dz).double()
    B, H, W, Cin = x.shape
    lo, hi = _same_pads(k)
    xp = torch.nn.functional.pad(x, (0, 0, lo, hi, lo, hi))
    d = dz.reshape(-1, dz.shape[-1])
    return torch.stack([torch.stack([xp[:, i:i + H, j:j + W, :].reshape(-1, Cin).T @ d for j in range(k)]) for i in range(k)])


def dgrad_f64(dz, w):
    """float64 input gradient [B,H,W,Cin] of the stride-1 SAME conv with filter w [k,k,Cin,Cout]."""
    dz, w = torch.as_tensor(dz).double(), torch.as_tensor(w).double()
    B, H, W, Cout = dz.shape
    k, Cin = w.shape[0], w.shape[2]
    lo, hi = _same_pads(k)
    dxp = torch.zeros((B, H + lo + hi, W + lo + hi, Cin), dtype=torch.float64)
    for i in range(k):
        for j in range(k):
            dxp[:, i:i + H, j:j + W, :] += dz @ w[i, j].T
    return dxp[:, lo:lo + H, lo:lo + W, :].contiguous()


def wgrad_with_route(x, dz, k, route):
    """x [B,H,W,Cin], dz [B,H,W,Cout] HIP tensors -> dw [k,k,Cin,Cout] through ops._launch_wgrad pinned to `route` (its workspace
    sizing and argument order are part of what is measured)."""
    lib = L.lib()
    Cin, Cout = x.shape[-1], dz.shape[-1]
    sch = L.RN_WINO_F43 if k == 3 else L.RN_WINO_F44
    assert route in WGRAD_ROUTES[k] and {"direct": 1, "wino2": lib.rn_conv2d_wino_wgrad_supported(Cin, Cout),
                                         "wino43": lib.rn_conv2d_wino43_wgrad_supported(Cin, Cout),
                                         "wino44": lib.rn_conv2d_wino44_wgrad_supported(Cin, Cout),
                                         "wino3l_split": lib.rn_winograd_split_wgrad_supported(sch, Cin, Cout)}[route] == 1, route
    pw = ops.PackedWeight.describe(L.RN_PACK_CONV, 2, (k, k), Cin, Cout)
    dw = torch.zeros((k, k, Cin, Cout), dtype=torch.float32, device=x.device)
    L.check(ops._launch_wgrad("conv2d", None, x, dz, dw, pw, (k, k), (1, 1), route=route), "filter gradient on " + route)
    return dw


def dgrad_with_scheme(dz, w, scheme):
    """dz [B,H,W,Cout], w [k,k,Cin,Cout] HIP tensors -> dx through the input-gradient launch that `scheme` forces: the launch
    _Conv._backward makes, on the dual pack."""
    pw = ops.pack_conv(w)
    dp = pw.dgrad_pack(True)
    stage = _STAGE.get(scheme[3:]) if scheme[:3] in ("f43", "f63", "f44") else None
    base = scheme[:3] if stage else scheme
    if base == "direct":
        dp.wino43 = dp.wino = dp.wino4 = None
        want = "direct"
    elif base == "f22":
        dp.wino43 = None
        want = "wino2"
    elif base == "f22x4":
        dp.wino43 = None
        want = "wino4"
    elif base == "f63":
        dp.force_scheme = "f63"
        want = "wino3l:f63"
    elif base in ("f43", "f44"):
        dp.wino63 = None
        want = "wino3l:" + base
    else:
        raise ValueError(scheme)
    B, H, W, _ = dz.shape
    dx = torch.empty((B, H, W, pw.cin), dtype=torch.float32, device=dz.device)
    with torch.no_grad(), ops.gemm_mode(stage or "f32"):
        r = ops._route("conv2d", dp, (H, W), (1, 1))
        assert r.name + (":" + r.scheme if r.scheme else "") == want, (scheme, r)
        if r.name != "direct":
            rc = ops._launch_route(r, dz, dp, (None, None, None, L.ptr(dx), None), 0)
        else:
            rc = ops._launch_direct("dgrad", "conv2d", dx, pw, (L.ptr(dz), L.ptr(dp.data), L.ptr(dx)), pw.kdims, (1, 1), (L.stream_ptr(),))
        L.check(rc, "input gradient on " + scheme)
    return dx


@functools.lru_cache(maxsize=None)
def backward_inputs(layer):
    """The operands of a BACKWARD_LAYERS entry: {x case name: x}, w, {dz case name: dz} -- seeded, built once."""
    k, Cin, Cout = BACKWARD_LAYERS[layer]
    B, H, W = BACKWARD_MAP
    rng = np.random.default_rng(20261017 + k)
    xs = list(hostile_inputs(rng, B, H, W, Cin, Cout))
    w = xavier(rng, (k, k, Cin, Cout))
    return ({xs[i][0]: xs[i][1] for i in X_CASES}, w, dict(hostile_gradients(rng, (B, H, W, Cout))))


def _rel(got, ref):
    top = float(ref.abs().max())
    assert top > 0.0 and bool(torch.isfinite(got).all())
    return float((got.cpu().double() - ref).abs().max()) / top


def measure_filter_gradient(layer, x_name):
    """{(route, dz case): max|dw - f64| / max|f64|} of a layer on one hostile x crossed with every hostile dz."""
    k = BACKWARD_LAYERS[layer][0]
    xs, _w, dzs = backward_inputs(layer)
    xd = torch.as_tensor(xs[x_name]).cuda()
    out = {}
    for dz_name, dz in dzs.items():
        ref = wgrad_f64(xs[x_name], dz, k)
        dzd = torch.as_tensor(dz).cuda()
        for route in WGRAD_ROUTES[k]:
            out[(route, dz_name)] = _rel(wgrad_with_route(xd, dzd, k, route), ref)
    return out


def measure_input_gradient(layer):
    """{(scheme, dz case): (whole-tensor error, [per-image error])}: max|dx - f64| / max|f64| over the tensor, and over each image
    against that image's own max|f64|."""
    k = BACKWARD_LAYERS[layer][0]
    _xs, w, dzs = backward_inputs(layer)
    wd = torch.as_tensor(w).cuda()
    out = {}
    for dz_name, dz in dzs.items():
        ref = dgrad_f64(dz, w)
        dzd = torch.as_tensor(dz).cuda()
        for scheme in DGRAD_SCHEMES[k]:
            got = dgrad_with_scheme(dzd, wd, scheme)
            out[(scheme, dz_name)] = (_rel(got, ref), [_rel(got[b], ref[b]) for b in range(ref.shape[0])])
    return out
