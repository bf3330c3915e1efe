"""The layer cases of the backward-route tests, each with the routes it must take, and the float64 reference they are compared with.
A plain module (no test in it): tests/test_backward_routes_cpu.py pins the routes on filter descriptions, tests/test_gpu_backward_routes.py
launches the same rows and asserts the same routes first.

A row is (flavour, B, spatial, Cin, Cout, k, stride, epilogue) -> routes, where routes is one string "forward input-gradient
filter-gradient" when the three multiply-stage modes agree, else {"f32": ..., "split": ..., "split16": ...}; a three-launch or 1x1-GEMM
route carries its scheme ("wino3l:f43").  Every shape is the smallest found that takes its route and is still ragged (odd map sizes, tile
tails); B = 2 throughout.  Epilogues: "prelu" = bias + PReLU, "res" = bias + residual (the nets never combine the two), "elu" = bias + ELU.
"""
import os
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import layers as OL  # noqa: E402
from scripts.robust_util import xavier  # noqa: E402

MODES = ("f32", "split", "split16")
RTOL = 2e-4           # the project's bar for a forward / a gradient against the reference: max|got - ref| <= RTOL * max|ref|, no absolute floor


def _by_mode(f32, split):
    return {"f32": f32, "split": split, "split16": split}


_ROWS = [
    # conv2d, stride 1
    (("conv2d", 2, (5, 7), 16, 32, 3, (1, 1)), "wino2 wino2 direct"),
    (("conv2d", 2, (5, 7), 256, 256, 3, (1, 1)), "wino2 wino2 wino2"),
    (("conv2d", 2, (8, 13), 256, 256, 3, (1, 1)), "wino3l:f43 wino3l:f43 wino43"),
    (("conv2d", 2, (11, 13), 256, 256, 3, (1, 1)), "wino3l:f63 wino3l:f63 wino43"),
    (("conv2d", 2, (8, 13), 512, 256, 3, (1, 1)), _by_mode("wino3l:f43 wino3l:f43 wino43", "wino3l:f43 wino3l:f43 wino3l_split")),
    (("conv2d", 2, (8, 13), 32, 256, 3, (1, 1)), "wino3l:f43 wino2 direct"),
    (("conv2d", 2, (8, 9), 256, 256, 4, (1, 1)), "wino3l:f44 wino3l:f44 wino44"),
    (("conv2d", 2, (8, 9), 512, 256, 4, (1, 1)), _by_mode("wino3l:f44 wino3l:f44 wino44", "wino3l:f44 wino3l:f44 wino3l_split")),
    (("conv2d", 2, (9, 11), 64, 32, 4, (1, 1)), "wino4 wino4 direct"),
    (("conv2d", 2, (32, 32), 256, 256, 1, (1, 1)), _by_mode("direct direct direct", "split11:f11 split11:f11 direct")),
    (("conv2d", 2, (6, 6), 64, 64, 1, (1, 1)), "direct direct direct"),
    # the other flavours
    (("conv2d", 2, (16, 16), 32, 32, 3, (2, 2)), "direct direct direct"),
    (("conv2d", 2, (12, 12), 3, 8, 3, (1, 1)), "direct direct direct"),
    (("conv2d_transpose", 2, (9, 7), 64, 32, 4, (2, 2)), "convt_s2_wino direct direct"),
    (("conv2d_transpose", 2, (8, 9), 256, 256, 4, (1, 1)), "wino3l:f44 wino3l:f44 direct"),
    (("conv2d_transpose", 2, (9, 9), 32, 16, 4, (1, 1)), "wino4 wino4 direct"),
    (("conv2d_transpose", 2, (9, 9), 16, 1, 4, (1, 1)), "direct direct direct"),
    (("conv3d", 2, (16, 8, 3), 32, 32, 3, (1, 1, 1)), _by_mode("wino3d wino3d direct", "split3d split3d split3d")),
    (("conv3d", 2, (5, 7, 3), 32, 32, 3, (1, 1, 1)), _by_mode("wino3d wino3d direct", "wino3d wino3d split3d")),
    (("conv3d", 2, (5, 7, 3), 16, 32, 3, (1, 1, 1)), "wino3d wino3d direct"),
    (("conv3d", 2, (8, 8, 8), 8, 16, 3, (1, 1, 2)), "direct direct direct"),
    (("conv3d_transpose", 2, (4, 4, 4), 8, 4, 4, (2, 2, 2)), "direct direct direct"),
]
# the two rows that also run with an ELU epilogue: the stride-1 transposed 4x4 conv on F(4x4,4x4) and the conv3d_transpose
_ELU_ROWS = (14, 21)

CASES = []            # (row, routes by mode)
for _i, (_row, _routes) in enumerate(_ROWS):
    CASES.append((_row + (("prelu", "res")[_i % 2],), _routes if isinstance(_routes, dict) else _by_mode(_routes, _routes)))
for _i in _ELU_ROWS:
    CASES.append((_ROWS[_i][0] + ("elu",), CASES[_i][1]))
assert len(CASES) == 24


def case_id(case):
    flavour, B, sp, Cin, Cout, k, stride, epi = case[0]
    return "%s-k%d-s%d-%dto%d-%s-%s" % (flavour, k, stride[-1], Cin, Cout, "x".join(str(n) for n in sp), epi)


def route_name(r):
    return r.name + (":" + r.scheme if r.scheme else "")


def routes_of(ops, row, pw=None):
    """"forward input-gradient filter-gradient" of a row in the multiply-stage mode in force, from the filter's description (pw: the
    packed filter a launch is about to use, instead of a description)."""
    from rendernet_amd import _lib as L
    flavour, B, sp, Cin, Cout, k, stride = row[:7]
    unit = max(stride) == 1
    if pw is None:
        kind = L.RN_PACK_CONV if flavour in ("conv2d", "conv3d") else L.RN_PACK_CONVT_S1 if unit else L.RN_PACK_CONVT_S2
        pw = ops.PackedWeight.describe(kind, len(sp), (k,) * len(sp), Cin, Cout)
    fr = ops._route(flavour, pw, tuple(sp), stride)
    dr = ops._route(flavour, pw.dgrad_pack(unit), tuple(sp), stride)
    wr = ops._wgrad_route(flavour, fr, pw, (B,) + tuple(sp) + (Cin,), stride)
    return "%s %s %s" % (route_name(fr), route_name(dr), wr)


def layer_operands(row, seed):
    """The fp32 operands of a row: x ~ N(0,1), Xavier filter, bias 0.1 N(0,1), PReLU slopes in (0.05, 0.3) (so sign(y) = sign(z)),
    residual and dy ~ N(0,1)."""
    flavour, B, sp, Cin, Cout, k, stride, epi = row
    rng = np.random.default_rng(seed)
    n = lambda *s: rng.standard_normal(s).astype(np.float32)
    transposed = flavour.endswith("transpose")
    out_sp = tuple(n_ * s for n_, s in zip(sp, stride)) if transposed else tuple(-(-n_ // s) for n_, s in zip(sp, stride))
    return {"x": n(B, *sp, Cin),
            "w": xavier(rng, (k,) * len(sp) + ((Cout, Cin) if transposed else (Cin, Cout))),
            "b": 0.1 * n(Cout),
            "alpha": rng.uniform(0.05, 0.3, Cout).astype(np.float32) if epi == "prelu" else None,
            "res": n(B, *out_sp, Cout) if epi == "res" else None,
            "dy": n(B, *out_sp, Cout)}


def prelu_by_mask(z, alpha, positive):
    """PReLU whose branch is GIVEN per element (positive: bool tensor) instead of taken from sign(z): the reference follows the branches
    the kernel took, so a pre-activation within rounding of zero cannot flip one."""
    return torch.where(positive, z, alpha * z)


class Reference:
    """float64 autograd over the oracle op on the same fp32 operands.  forward() -> the pre-activation z and the output y with the
    natural PReLU; grads(dy, positive) -> every gradient, PReLU branches from `positive` (the sign of the launched forward's output)."""

    def __init__(self, row, o):
        self.row = row
        d = lambda a: None if a is None else torch.from_numpy(a).double().requires_grad_(True)
        self.x, self.w, self.b, self.alpha, self.res = (d(o[k]) for k in ("x", "w", "b", "alpha", "res"))
        flavour, stride = row[0], row[6]
        self.z = getattr(OL, flavour)(self.x, self.w, self.b, stride)

    def _out(self, positive=None):
        epi = self.row[7]
        if epi == "prelu":
            return OL.prelu(self.z, self.alpha) if positive is None else prelu_by_mask(self.z, self.alpha, positive)
        if epi == "elu":
            return F.elu(self.z)
        return self.z + self.res

    def forward(self):
        return self._out().detach()

    def grads(self, dy, positive=None):
        ins = {"dx": self.x, "dw": self.w, "dbias": self.b, "dalpha": self.alpha, "dresidual": self.res}
        ins = {k: v for k, v in ins.items() if v is not None}
        g = torch.autograd.grad(self._out(positive), list(ins.values()), torch.as_tensor(dy).double(), retain_graph=True)
        return dict(zip(ins, g))


def ratio(got, ref):
    """max|got - ref| / max|ref| in float64; max|ref| must not vanish (a case cannot pass on zeros)."""
    got = got.detach().cpu().double() if isinstance(got, torch.Tensor) else torch.as_tensor(got).double()
    ref = ref.detach().double()
    assert tuple(got.shape) == tuple(ref.shape), (got.shape, ref.shape)
    top = float(ref.abs().max())
    assert top > 0.0, "the reference is all zero"
    assert bool(torch.isfinite(got).all()), "non-finite values"
    return float((got - ref).abs().max()) / top


# One res block x + conv2(prelu(conv1(x) + b1)) + b2 as tools/layer_util.py writes it (conv1 with carry=True, conv2 with the carried x as
# its residual): (flavour, spatial, C) -> the route of conv1's INPUT-GRADIENT launch per mode.  One shape per member of
# ops.CARRY_IN_EPILOGUE (the carried skip gradient rides in that launch's residual epilogue) and one whose input gradient goes direct
# (the skip gradient is added by one add_ afterwards).
BLOCK_CASES = [
    (("conv2d", (5, 7), 32), _by_mode("wino2", "wino2")),
    (("conv2d", (8, 13), 256), _by_mode("wino3l:f43", "wino3l:f43")),
    (("conv2d", (11, 13), 256), _by_mode("wino3l:f63", "wino3l:f63")),
    (("conv3d", (5, 7, 3), 32), _by_mode("wino3d", "wino3d")),
    (("conv3d", (16, 8, 3), 32), _by_mode("wino3d", "split3d")),
    (("conv2d", (6, 6), 8), _by_mode("direct", "direct")),
]


def block_id(case):
    flavour, sp, C = case[0]
    return "%s-%d-%s" % (flavour, C, "x".join(str(n) for n in sp))


def block_dgrad_route(ops, block, pw=None):
    """The route of the input-gradient launch of a res block's first conv in the mode in force."""
    from rendernet_amd import _lib as L
    flavour, sp, C = block
    if pw is None:
        pw = ops.PackedWeight.describe(L.RN_PACK_CONV, len(sp), (3,) * len(sp), C, C)
    return ops._route(flavour, pw.dgrad_pack(True), tuple(sp), (1,) * len(sp))


def stack_operands(flavour, sp, C, n_blocks, skip, seed, B=2):
    """x, dy and the parameters of n_blocks res blocks (w1, b1, a1, w2, b2 each) and, with skip, of the conv behind them (w, b)."""
    rng = np.random.default_rng(seed)
    n = lambda *s: rng.standard_normal(s).astype(np.float32)
    wshape = (3,) * len(sp) + (C, C)
    blocks = [{"w1": xavier(rng, wshape), "b1": 0.1 * n(C), "a1": rng.uniform(0.05, 0.3, C).astype(np.float32),
               "w2": xavier(rng, wshape), "b2": 0.1 * n(C)} for _ in range(n_blocks)]
    return {"x": n(B, *sp, C), "dy": n(B, *sp, C), "blocks": blocks,
            "skip": {"w": xavier(rng, wshape), "b": 0.1 * n(C)} if skip else None}


class StackReference:
    """float64 autograd over n res blocks (+ the skip conv, whose residual is the stack's input x).  forward() -> ([h of every block], y)
    with the natural PReLU; grads(dy, [positive of every block]) -> dx and {"<block>.<name>": gradient}."""

    def __init__(self, flavour, o):
        d = lambda a: torch.from_numpy(a).double().requires_grad_(True)
        self.conv = getattr(OL, flavour)
        self.x = d(o["x"])
        self.blocks = [{k: d(v) for k, v in b.items()} for b in o["blocks"]]
        self.skip = {k: d(v) for k, v in o["skip"].items()} if o["skip"] else None

    def _run(self, positives=None):
        net, hs = self.x, []
        for i, p in enumerate(self.blocks):
            z = self.conv(net, p["w1"], p["b1"])
            h = OL.prelu(z, p["a1"]) if positives is None else prelu_by_mask(z, p["a1"], positives[i])
            hs.append(h)
            net = net + self.conv(h, p["w2"], p["b2"])
        if self.skip is not None:
            net = self.conv(net, self.skip["w"], self.skip["b"]) + self.x
        return hs, net

    def forward(self):
        with torch.no_grad():
            hs, y = self._run()
        return hs, y

    def grads(self, dy, positives):
        _, y = self._run(positives)
        ins = {"dx": self.x}
        for i, p in enumerate(self.blocks):
            ins.update({"%d.%s" % (i, k): v for k, v in p.items()})
        if self.skip is not None:
            ins.update({"skip.%s" % k: v for k, v in self.skip.items()})
        g = torch.autograd.grad(y, list(ins.values()), torch.as_tensor(dy).double())
        return dict(zip(ins, g))
