"""Tensor-level operators over the C ABI (include/rendernet_hip.h).

Every function takes and returns torch tensors on the HIP device, launches on torch's current
stream and allocates its output from torch's caching allocator; there is no CPU path.  Two parts:

The network operators (packed weights, resampling, the conv family, projection, fully connected,
dropout, PReLU, Phong) take contiguous float32 tensors, channels-last as TF holds them.  The conv
family are `torch.autograd.Function`s whose forward AND backward are HIP kernels behind the C ABI
(dgrad / wgrad / epilogue backward); torch's autograd engine only orders the calls.  Parameter
gradients do not travel through autograd: inside a `training(...)` context each backward
accumulates them straight into the gradient views the context maps the parameter tensors to (one
flat buffer, see rendernet_amd/train.py) and reports completion so that gradient buckets can be
all-reduced while the rest of the backward is still running.

The tools, from `target_u8_crop` on (uint8 target ingest, voxel packing and procedural shapes, the
mesh voxeliser, surface-net extraction and rasteriser, image metrics, the distance transform and
shape metrics and registration, connected components and topology, the voxel ray casters), are integer work on
uint8 / int32 / int64 tensors (float32 where a docstring says so) and carry no autograd.  They
check their arguments before anything is launched and name the public function in every message;
what their wrappers share (`_vp`, `_workspace`, `_grid_side`, `_occupancy`, `_finite`,
`_packed_grids`) stands at the head of that part.
"""
import collections
import contextlib
import math
import threading
import os
import ctypes

import numpy as np

import torch

from . import _lib as L


# Optional measurement hook (bench.py): called as LAUNCH_HOOK(mode, x_shape, packed_weight) and must
# return None or a (start_event, end_event) pair that is recorded around the launch on the
# current stream.
LAUNCH_HOOK = None


def _chk_dev(*ts):
    for t in ts:
        if t is not None and not t.is_cuda:
            raise L.RenderNetHipError("rendernet_amd ops need HIP tensors (got %s); there is no CPU path" % t.device)


def _transposed(pw):
    return 1 if pw.kind == L.RN_PACK_CONVT_S1 else 0


# A packed form of a filter is (family, argument); a family declares (buffer dtype, element count, the C entry that fills it):
#   "pack":    argument = a pack kind (RN_PACK_*): the direct kernels' [phase][K/4][Npad][4] layout and the fp32 Winograd forms
#   "split":   argument = a Winograd scheme | the operand format flag: operands of the split GEMM stage (csrc/conv_wino_bf3.hip)
#   "split3d": argument = the operand format (0: bf16x3, 1: fp16x2): the fused 3x3x3 kernel's, in MFMA fragment order (csrc/conv3d_wino_bf3.hip)
_FAMILIES = {
    "pack": (torch.float32,
             lambda lib, pw, a: lib.rn_packed_weight_floats(a, pw.ndim, L.ivec(pw.kdims), pw.cin, pw.cout),
             lambda lib, pw, a, buf: lib.rn_pack_weights(a, pw.ndim, L.ivec(pw.kdims), pw.cin, pw.cout, L.ptr(pw.w_tf), L.ptr(buf), L.stream_ptr())),
    "split": (torch.uint8,
              lambda lib, pw, a: lib.rn_winograd_split_packed_bytes(a, pw.cin, pw.cout),
              lambda lib, pw, a, buf: lib.rn_winograd_split_pack(a, L.ptr(pw.w_tf), ctypes.c_void_p(buf.data_ptr()), pw.cin, pw.cout,
                                                                 _transposed(pw), L.stream_ptr())),
    "split3d": (torch.uint8,
                lambda lib, pw, a: lib.rn_conv3d_winograd_split_packed_bytes_ex(a, pw.cin, pw.cout),
                lambda lib, pw, a, buf: lib.rn_conv3d_winograd_split_pack_ex(a, L.ptr(pw.w_tf), ctypes.c_void_p(buf.data_ptr()), pw.cin, pw.cout,
                                                                             _transposed(pw), L.stream_ptr())),
}


class _Packed:
    """One packed form of one filter: its buffer, whether the master changed since it was filled, (stream, event) behind its last pack kernel."""
    buf, dirty, on = None, True, None


def _form_property(form, doc):
    def get(self):
        kind = self.forms.get(form)
        return None if kind is None else self._packed("pack", kind)

    def switch_off(self, value):
        if value is not None:
            raise ValueError("a packed form can only be switched off (set to None)")
        self.disable(form)
    return property(get, switch_off, doc=doc)


class PackedWeight:
    """A conv filter converted once from TF layout to the kernels' [phase][K/4][Npad][4] layout."""

    def __init__(self, w_tf, kind, ndim):
        _chk_dev(w_tf)
        w_tf = w_tf.contiguous().float()
        a, b = int(w_tf.shape[ndim]), int(w_tf.shape[ndim + 1])
        cin, cout = (a, b) if kind == L.RN_PACK_CONV else (b, a)
        self._describe(kind, ndim, [int(k) for k in w_tf.shape[:ndim]], cin, cout, w_tf)

    @classmethod
    def describe(cls, kind, ndim, kdims, cin, cout, w_tf=None):
        """A filter from its description; without w_tf everything the route decision reads, on no device (nothing can be packed)."""
        pw = cls.__new__(cls)
        pw._describe(kind, ndim, [int(k) for k in kdims], int(cin), int(cout), w_tf)
        return pw

    def _describe(self, kind, ndim, kdims, cin, cout, w_tf):
        self.kind, self.ndim, self.kdims, self.cin, self.cout = kind, ndim, kdims, cin, cout
        lib = L.lib()
        if lib.rn_packed_weight_floats(kind, ndim, L.ivec(kdims), cin, cout) == 0:
            raise L.RenderNetHipError("rn_packed_weight_floats: %s" % lib.rn_last_error().decode())
        self.w_tf = w_tf                  # the TF-layout master copy (what the optimiser updates)
        self._dgrad = None
        # Every packed form is built LAZILY, on first use after the master changed: a layer that runs the Winograd kernel
        # never materialises its direct pack (949 MB for the net), and a training step re-derives only the forms its
        # forward and input-gradient launches actually read.
        self._slots = {}                  # (family, argument) -> _Packed
        self.force_scheme = None          # measurement / tests: pin the three-launch scheme of this filter ("f43" | "f63")
        self._wino63_verdict = None       # the F(6x6,3x3) self-check's verdict on this filter, once it has run
        self.demoted = False              # ... it failed: F(6x6,3x3) dropped (here and on the dgrad pack)
        self.gemm_f32 = False             # ... and every launch of this filter takes the exact-fp32 multiply stage
        # Which forms beside the direct pack this filter has: form -> its pack kind (its scheme for "split11").  The route decision reads this.
        conv, convt1 = kind == L.RN_PACK_CONV, kind == L.RN_PACK_CONVT_S1
        pick = lambda of_conv, of_convt1: of_conv if conv else of_convt1
        f = self.forms = {}
        if conv or convt1:
            # Winograd F(2x2,3x3) (csrc/conv_wino.hip): 3x3 / 3x3x3 filters whose channel counts the kernel takes; used by every
            # stride-1 launch of this filter (forward, and the input gradient through the dgrad pack).
            if ((ndim == 2 and kdims == [3, 3] and lib.rn_conv2d_wino_supported(cin, cout)) or
                    (ndim == 3 and kdims == [3, 3, 3] and lib.rn_conv3d_wino_supported(cin, cout))):
                f["wino"] = pick(L.RN_PACK_CONV_WINO, L.RN_PACK_CONVT_S1_WINO)
                # ... and the split forms of the fused 3x3x3 32 -> 32 kernel
                if ndim == 3 and lib.rn_conv3d_winograd_split_supported(cin, cout):
                    f["split3d"] = True
            # 4x4 stride-1 filters (e_conv5, e_conv6; e_conv7_1 as a transposed conv): four 2x2 sub-filters, each F(2x2,2x2)
            if ndim == 2 and kdims == [4, 4] and lib.rn_conv2d_wino4_supported(cin, cout):
                f["wino4"] = pick(L.RN_PACK_CONV_WINO4, L.RN_PACK_CONVT_S1_WINO4)
            # Winograd with 4x4 output tiles in three launches (csrc/conv_wino43.hip): F(4x4,3x3) for the wide 3x3 2-D layers
            # (res2, res3 and their skips), F(4x4,4x4) for the wide 4x4 ones (e_conv5, e_conv6)
            if ndim == 2 and kdims == [3, 3] and lib.rn_conv2d_wino43_supported(cin, cout):
                f["wino43"] = pick(L.RN_PACK_CONV_WINO43, L.RN_PACK_CONVT_S1_WINO43)
                # ... and F(6x6,3x3) for the same 3x3 layers on maps where the 6-pixel tile grid pays (_wino_scheme picks per launch)
                if lib.rn_conv2d_wino63_supported(cin, cout):
                    f["wino63"] = pick(L.RN_PACK_CONV_WINO63, L.RN_PACK_CONVT_S1_WINO63)
            elif ndim == 2 and kdims == [4, 4] and lib.rn_conv2d_wino44_supported(cin, cout):
                f["wino43"] = pick(L.RN_PACK_CONV_WINO44, L.RN_PACK_CONVT_S1_WINO44)
            # 1x1 filters (the projection unit, tools/layer_util.py:8-22): on the split multiply stage a plain GEMM, scheme RN_WINO_F11 (one plane,
            # identity transforms; csrc/conv_wino_bf3.hip).  The exact-fp32 mode keeps the implicit-GEMM kernel for them.
            if ndim == 2 and kdims == [1, 1] and lib.rn_winograd_split_supported(L.RN_WINO_F11, cin, cout):
                f["split11"] = L.RN_WINO_F11
        # 4x4 STRIDE-2 transposed filters (e_conv7, e_conv8, e_conv9 and the texture net's heads): every output phase is a 2x2
        # conv, each F(2x2,2x2); the four phases run as one launch (rides in the "wino4" slot: a filter is one or the other)
        elif kind == L.RN_PACK_CONVT_S2 and ndim == 2 and kdims == [4, 4] and lib.rn_conv2d_transpose_s2_wino_supported(cin, cout):
            f["wino4"] = L.RN_PACK_CONVT_S2_WINO

    def has(self, form):
        """Whether this filter has the form ("wino" | "wino4" | "wino43" | "wino63" | "split11" | "split3d") -- a pure predicate:
        nothing is packed or allocated."""
        return form in self.forms

    # switching a form off takes the forms built on it along (F(6x6,3x3) goes with the three-launch path as a whole)
    _GOES_WITH = {"wino": ("split3d",), "wino43": ("wino63",)}

    def disable(self, form):
        for f in (form,) + self._GOES_WITH.get(form, ()):
            self.forms.pop(f, None)

    def demote(self):
        """The F(6x6,3x3) self-check rejected this filter: it -- and its input-gradient pack, now or when that is created -- takes
        F(4x4,3x3) on the exact-fp32 stage from now on."""
        for p in (self, self._dgrad):
            if p is not None:
                p.disable("wino63")
                p.gemm_f32 = p.demoted = True

    def _packed(self, family, arg):
        slot = self._slots.get((family, arg))
        if slot is None:
            slot = self._slots[(family, arg)] = _Packed()
        if slot.dirty:
            lib = L.lib()
            dtype, count, pack = _FAMILIES[family]
            if slot.buf is None:
                n = count(lib, self, arg)
                if n == 0:
                    raise L.RenderNetHipError("packed form %s %d: unsupported filter (%s)" % (family, arg, lib.rn_last_error().decode()))
                slot.buf = torch.empty(n, dtype=dtype, device=self.w_tf.device)
            L.check(pack(lib, self, arg, slot.buf), "packing form %s %d" % (family, arg))
            slot.dirty = False
            # the pack runs on the stream that first needed it; a launch on ANOTHER stream (two-stream serving sharing one
            # Renderer) must not read the buffer before that kernel has finished
            # (inside a hipGraph capture no event is recorded: it would become part of the capture and a later query() from
            # another stream would fail; Renderer.capture joins the warm-up stream before capturing, and a REpack -- an
            # optimiser step or a demotion -- is single-stream by contract: the trainers run pack and readers on one stream)
            if torch.cuda.is_current_stream_capturing():
                slot.on = None
            else:
                ev = torch.cuda.Event()
                ev.record()
                slot.on = (torch.cuda.current_stream(), ev)
        elif slot.on is not None:
            cur = torch.cuda.current_stream()
            # (not while a hipGraph is being captured: event queries are illegal there, and Renderer.capture has joined
            # the warm-up stream before it starts capturing)
            if cur != slot.on[0] and not torch.cuda.is_current_stream_capturing():
                if slot.on[1].query():
                    slot.on = None      # finished: no stream needs to wait any more
                else:
                    cur.wait_event(slot.on[1])
        return slot.buf

    @property
    def data(self):
        """The direct-kernel pack [phase][K/4][Npad][4]."""
        return self._packed("pack", self.kind)

    # readable (None when the filter has no such form); assigning None switches the form off
    wino = _form_property("wino", "The Winograd F(2x2,3x3) pack, or None when this filter does not take that path.")
    wino4 = _form_property("wino4", "The 4x4 (four F(2x2,2x2) sub-filters) pack, or None.")
    wino43 = _form_property("wino43", "The Winograd F(4x4,3x3) (3x3 filters) / F(4x4,4x4) (4x4 filters) pack, or None; None also switches F(6x6,3x3) off.")
    wino63 = _form_property("wino63", "The Winograd F(6x6,3x3) pack (3x3 filters), or None.")
    # two views of `forms` under the names the kernel tests read
    _split11 = property(lambda self: "split11" in self.forms)
    _wino4_kind = property(lambda self: self.forms.get("wino4"))

    def split(self, which, fmt=0):
        """The split form (uint8 buffer) of scheme `which` ("f43" | "f44" | "f63" | "f11") for the split GEMM stage, or None.  fmt: 0 = three
        bf16 pieces, L.RN_SPLIT_FMT_H2 = two fp16 pieces of the scaled value."""
        if which == "f11":
            form, scheme = "split11", L.RN_WINO_F11
        elif which == "f63":
            form, scheme = "wino63", L.RN_WINO_F63
        else:
            form, scheme = "wino43", L.RN_WINO_F44 if self.kdims == [4, 4] else L.RN_WINO_F43
        return self._packed("split", scheme | fmt) if form in self.forms else None

    def split3d(self, fmt=0):
        """A split form of a 3x3x3 32 -> 32 filter for rn_conv3d_winograd_split_fwd_ex (uint8 buffer), or None.  fmt 0: three bf16
        pieces; 1: two fp16 pieces of the scaled value."""
        return self._packed("split3d", 1 if fmt else 0) if "split3d" in self.forms else None

    def repack(self):
        """The TF-layout master changed (an optimiser step): every packed form is stale and is rebuilt when next read."""
        for slot in self._slots.values():
            slot.dirty = True
        if self._dgrad is not None:
            self._dgrad.repack()

    def dgrad_pack(self, unit_stride):
        """The packing the layer's input-gradient kernel reads (include/rendernet_hip.h, dgrad section):
        conv, stride 1 -> the same TF tensor packed as a stride-1 transposed-conv filter; strided conv ->
        the forward pack itself; transposed conv -> the same TF tensor packed as a conv filter."""
        if self.kind == L.RN_PACK_CONV and not unit_stride:
            return self
        if self._dgrad is None:
            kind = L.RN_PACK_CONVT_S1 if self.kind == L.RN_PACK_CONV else L.RN_PACK_CONV
            self._dgrad = PackedWeight.describe(kind, self.ndim, self.kdims, self.cout, self.cin, self.w_tf)      # (the channel roles swap)
            if self.demoted:
                self.demote()                                 # the forward pack was demoted by the F(6x6,3x3) self-check
        return self._dgrad


def pack_conv(w_tf):
    """TF conv filter [k..., Cin, Cout] (2-D or 3-D)."""
    return PackedWeight(w_tf, L.RN_PACK_CONV, w_tf.dim() - 2)


def pack_conv_transpose(w_tf, stride):
    """TF conv_transpose filter [k..., Cout, Cin]."""
    return PackedWeight(w_tf, L.RN_PACK_CONVT_S1 if stride == 1 else L.RN_PACK_CONVT_S2, w_tf.dim() - 2)


def _act_code(alpha, sigmoid, elu=False):
    if elu and (alpha is not None or sigmoid):
        raise L.RenderNetHipError("ELU does not combine with PReLU / sigmoid in one epilogue")
    return (L.RN_ACT_PRELU if alpha is not None else 0) | (L.RN_ACT_SIGMOID if sigmoid else 0) | (L.RN_ACT_ELU if elu else 0)


class _ForwardOnly(torch.autograd.Function):
    @staticmethod
    def backward(ctx, *grads):
        raise NotImplementedError("rendernet_amd: this inference-only entry has no backward; inside ops.training(...) "
                                  "the projection unit runs through the differentiable conv2d path instead")


class _Resample(torch.autograd.Function):
    """Forward: rn_resample_fwd / rn_resample_affine_fwd.  Backward: rn_resample_affine_bwd (+ rn_pose_to_affine_bwd
    for the pose path) -- gradients w.r.t. the voxel grid and the pose / matrix, whichever require grad."""

    @staticmethod
    def forward(ctx, vox, pose, N, window, image_layout, affine):
        _chk_dev(vox, pose)
        B, S, C = vox.shape[0], vox.shape[1], vox.shape[4]
        h0, w0, ph, pw = window
        out = torch.empty((B, ph, pw, N, C), dtype=torch.float32, device=vox.device)
        lib = L.lib()
        nws = int(lib.rn_resample_workspace_bytes(B, S, C))
        ws = torch.empty(max(nws, 16), dtype=torch.uint8, device=vox.device) if nws else None
        fn = lib.rn_resample_affine_fwd if affine else lib.rn_resample_fwd
        ev = LAUNCH_HOOK("resample", tuple(vox.shape), None) if LAUNCH_HOOK is not None else None
        if ev is not None:
            ev[0].record()
        L.check(fn(L.ptr(vox), L.ptr(pose), L.ptr(out), B, S, N, C, h0, w0, ph, pw, 1 if image_layout else 0,
                   ctypes.c_void_p(ws.data_ptr()) if ws is not None else None, nws, L.stream_ptr()),
                "rn_resample_fwd")
        if ev is not None:
            ev[1].record()
        ctx.save_for_backward(vox, pose)
        ctx.cfg = (N, window, image_layout, affine)
        return out

    @staticmethod
    def backward(ctx, dout):
        vox, pose = ctx.saved_tensors
        N, (h0, w0, ph, pw), image_layout, affine = ctx.cfg
        B, S, C = vox.shape[0], vox.shape[1], vox.shape[4]
        lib, st = L.lib(), L.stream_ptr()
        dout = dout.contiguous()
        m = pose if affine else pose_to_affine(pose, S, N).reshape(B, 12)
        want_vox, want_pose = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dvox = torch.zeros_like(vox) if want_vox else None
        dm = torch.zeros((B, 12), dtype=torch.float32, device=vox.device) if want_pose else None
        if want_vox or want_pose:
            L.check(lib.rn_resample_affine_bwd(L.ptr(vox), L.ptr(m.contiguous()), L.ptr(dout), L.ptr(dvox), L.ptr(dm),
                                               B, S, N, C, h0, w0, ph, pw, 1 if image_layout else 0, st),
                    "rn_resample_affine_bwd")
        dpose = None
        if want_pose:
            if affine:
                dpose = dm.reshape(pose.shape)
            else:
                dpose = torch.zeros_like(pose)
                L.check(lib.rn_pose_to_affine_bwd(L.ptr(pose), L.ptr(dm), L.ptr(dpose), B, S, N, st), "rn_pose_to_affine_bwd")
        return dvox, dpose, None, None, None, None


def _chk_resample_args(what, voxels, pose, affine):
    """The kernels index pose with stride 3 (matrices with stride 12) and one entry per voxel item: anything else would be read
    with the wrong stride or past its end, silently.  Raised here, before any launch."""
    B = None
    for vox in voxels:
        if vox.dim() != 5 or not (vox.shape[1] == vox.shape[2] == vox.shape[3]):
            raise L.RenderNetHipError("%s: expected a voxel cube [B,S,S,S,C], got %s" % (what, tuple(vox.shape)))
        B = int(vox.shape[0])
    shape = tuple(pose.shape)
    if affine:
        if B is not None and shape not in ((B, 3, 4), (B, 12)):
            raise L.RenderNetHipError("%s: expected %d matrices [B,3,4] (or [B,12]), got %s" % (what, B, shape))
    elif len(shape) != 2 or shape[1] != 3 or (B is not None and shape[0] != B):
        raise L.RenderNetHipError("%s: expected poses [%s,3] (azimuth, elevation, scale), got %s"
                                  % (what, "B" if B is None else B, shape))


def resample(vox, pose, new_size=128, window=None, image_layout=True, affine=False):
    """vox [B,S,S,S,C], pose [B,3] (or M_inv [B,3,4] / [B,12] with affine=True) -> [B,ph,pw,N,C]."""
    _chk_resample_args("resample", (vox,), pose, affine)
    vox = vox.contiguous().float()
    pose = pose.contiguous().float()
    if window is None:
        window = (0, 0, new_size, new_size)
    return _Resample.apply(vox, pose, int(new_size), tuple(int(v) for v in window), image_layout, affine)


class _ResampleConcat(torch.autograd.Function):
    """Two volumes, one pose, one channel-concatenated output (rn_resample_concat_fwd); backward: one
    rn_resample_affine_bwd_strided per source that needs a gradient, the matrix gradient accumulated over both."""

    @staticmethod
    def forward(ctx, vox_a, vox_b, pose, N, window, image_layout, affine):
        _chk_dev(vox_a, vox_b, pose)
        B, S, Ca, Cb = vox_a.shape[0], vox_a.shape[1], vox_a.shape[4], vox_b.shape[4]
        h0, w0, ph, pw = window
        out = torch.empty((B, ph, pw, N, Ca + Cb), dtype=torch.float32, device=vox_a.device)
        ev = LAUNCH_HOOK("resample", (B, S, S, S, Ca + Cb), None) if LAUNCH_HOOK is not None else None
        if ev is not None:
            ev[0].record()
        # poses become matrices in one small launch (the same closed form the kernel would evaluate per workgroup)
        m = pose if affine else pose_to_affine(pose, S, N)
        L.check(L.lib().rn_resample_concat_fwd(L.ptr(vox_a), Ca, L.ptr(vox_b), Cb, L.ptr(m), 1, L.ptr(out),
                                               B, S, N, h0, w0, ph, pw, 1 if image_layout else 0, L.stream_ptr()),
                "rn_resample_concat_fwd")
        if ev is not None:
            ev[1].record()
        ctx.save_for_backward(vox_a, vox_b, pose)
        ctx.cfg = (N, window, image_layout, affine)
        return out

    @staticmethod
    def backward(ctx, dout):
        vox_a, vox_b, pose = ctx.saved_tensors
        N, (h0, w0, ph, pw), image_layout, affine = ctx.cfg
        B, S, Ca, Cb = vox_a.shape[0], vox_a.shape[1], vox_a.shape[4], vox_b.shape[4]
        lib, st = L.lib(), L.stream_ptr()
        dout = dout.contiguous()
        m = (pose if affine else pose_to_affine(pose, S, N).reshape(B, 12)).contiguous()
        want_pose = ctx.needs_input_grad[2]
        dm = torch.zeros((B, 12), dtype=torch.float32, device=vox_a.device) if want_pose else None
        grads = []
        for vox, C, off, want in ((vox_a, Ca, 0, ctx.needs_input_grad[0]), (vox_b, Cb, Ca, ctx.needs_input_grad[1])):
            dv = torch.zeros_like(vox) if want else None
            if want or want_pose:
                L.check(lib.rn_resample_affine_bwd_strided(L.ptr(vox), L.ptr(m), L.ptr(dout), Ca + Cb, off, L.ptr(dv), L.ptr(dm),
                                                           B, S, N, C, h0, w0, ph, pw, 1 if image_layout else 0, st),
                        "rn_resample_affine_bwd_strided")
            grads.append(dv)
        dpose = None
        if want_pose:
            if affine:
                dpose = dm.reshape(pose.shape)
            else:
                dpose = torch.zeros_like(pose)
                L.check(lib.rn_pose_to_affine_bwd(L.ptr(pose), L.ptr(dm), L.ptr(dpose), B, S, N, st), "rn_pose_to_affine_bwd")
        return grads[0], grads[1], dpose, None, None, None, None


def resample_concat(vox_a, vox_b, pose, new_size=128, window=None, image_layout=True, affine=False):
    """vox_a [B,S,S,S,Ca], vox_b [B,S,S,S,Cb], one pose [B,3] (or M_inv, affine=True) -> [B,ph,pw,N,Ca+Cb]: what
    `concat([resample(vox_a), resample(vox_b)], -1)` computes, in one pass and without the intermediates."""
    _chk_resample_args("resample_concat", (vox_a, vox_b), pose, affine)
    vox_a, vox_b, pose = vox_a.contiguous().float(), vox_b.contiguous().float(), pose.contiguous().float()
    if vox_a.shape[:4] != vox_b.shape[:4]:
        raise L.RenderNetHipError("resample_concat: grids %s and %s differ" % (tuple(vox_a.shape), tuple(vox_b.shape)))
    if window is None:
        window = (0, 0, new_size, new_size)
    return _ResampleConcat.apply(vox_a, vox_b, pose, int(new_size), tuple(int(v) for v in window), image_layout, affine)


def pose_to_affine(pose, size=64, new_size=128):
    """pose [B,3] (azimuth, elevation, scale) -> M_inv [B,3,4]."""
    _chk_resample_args("pose_to_affine", (), pose, False)
    pose = pose.contiguous().float()
    _chk_dev(pose)
    m = torch.empty((pose.shape[0], 3, 4), dtype=torch.float32, device=pose.device)
    L.check(L.lib().rn_pose_to_affine(L.ptr(pose), L.ptr(m), pose.shape[0], size, new_size, L.stream_ptr()),
            "rn_pose_to_affine")
    return m


# ---------------------------------------------------------------------------------------------
# training context
# ---------------------------------------------------------------------------------------------
class TrainContext:
    """Maps parameter tensors (by data_ptr) to the gradient views they accumulate into and is told
    when a parameter's gradient is complete.  `anchor` is a dummy leaf that requires grad: it rides
    along every conv call so that autograd schedules the backward of layers whose data input does
    not require grad (the first conv reads the resampled voxels)."""

    def __init__(self, grad_of=None, on_ready=None, device="cuda", frozen=False):
        self.grad_of = grad_of or {}      # {data_ptr: grad tensor}
        self.on_ready = on_ready          # callable(data_ptr) or None
        self.frozen = frozen              # pretrained weights (inverse rendering): input gradients only, no wgrad
        self.anchor = torch.zeros(1, device=device, requires_grad=True)

    def grad(self, t):
        if self.frozen:
            return None
        g = self.grad_of.get(t.data_ptr())
        if g is None:
            raise L.RenderNetHipError("no gradient buffer registered for a parameter of shape %s" % (tuple(t.shape),))
        return g

    def grad_if_param(self, t):
        """The gradient view of t, or None for a tensor MARKED as a constant that rides in a parameter slot (ops.mark_constant: the
        all-zero PReLU slope that makes the pretrained res blocks' ReLU, tools/layer_util.py:_relu_slope) -- no gradient is produced
        for it.  Any other tensor must be registered: a PReLU slope that was never registered is a bug that would otherwise show up
        as a parameter that silently never trains."""
        if self.frozen or t is None:
            return None
        g = self.grad_of.get(t.data_ptr())
        if g is None and not is_constant(t):
            raise L.RenderNetHipError("no gradient buffer registered for a parameter of shape %s (a constant in a parameter slot "
                                      "must be marked with ops.mark_constant)" % (tuple(t.shape),))
        return g

    def ready(self, *ts):
        if self.on_ready is not None:
            for t in ts:
                if t is None or is_constant(t):
                    continue
                if t.data_ptr() not in self.grad_of:
                    raise L.RenderNetHipError("ready(): a tensor of shape %s is neither a registered parameter nor a marked constant"
                                              % (tuple(t.shape),))
                self.on_ready(t.data_ptr())


def mark_constant(t):
    """Marks a tensor that sits in a parameter slot of an operator (bias / alpha) as a constant: no gradient, no on_ready call."""
    t._rn_constant = True
    return t


def is_constant(t):
    return bool(getattr(t, "_rn_constant", False))


TRAIN = None


@contextlib.contextmanager
def training(ctx):
    """Within this context the conv operators save what their backward needs and are differentiable."""
    global TRAIN
    old, TRAIN = TRAIN, ctx
    try:
        yield ctx
    finally:
        TRAIN = old


AMAX_MISSES = None     # diagnostics: set to a list to record the split-format-H2 launches that had to make their own pass over x
STAGE_HOOK = None      # bench.py: callable(stage, (T, Cin, Cout, which)) -> (start_event, end_event) | None, brackets the GEMM stage


def _stage_events(stage, T, Cin, Cout, which):
    """The (start, end) events of a STAGE_HOOK that wants this stage bracketed, else None (also for a GEMM stage of a size the stage
    entry points do not take)."""
    if STAGE_HOOK is None or (stage == "gemm" and T * max(Cin, Cout) * 4 >= 0x7fffff00):
        return None
    return STAGE_HOOK(stage, (T, Cin, Cout, which))


def _bracketed(ev, launch):
    """rc = launch(), with the (start, end) events of a measurement hook recorded around it on the current stream."""
    if ev is None:
        return launch()
    ev[0].record()
    rc = launch()
    ev[1].record()
    return rc


def _staged(ev, transform_in, gemm, transform_out):
    """The three launches of the three-launch path through the stage entry points, the GEMM bracketed by the caller's events."""
    rc = transform_in()
    if rc == 0:
        rc = _bracketed(ev, gemm)
    if rc == 0:
        rc = transform_out()
    return rc


def _wino_scheme(pw, H, W):
    """Which three-launch scheme a stride-1 launch of this filter on an H x W map takes: "f44" (4x4 filters), "f63" where
    ceil(H/6)*ceil(W/6) tiles of 64 products undercut ceil(H/4)*ceil(W/4) tiles of 36 by at least WINO63_MIN_GAIN (64x64:
    7744 against 9216; 32x32 and 16x16: equal, so the more accurate F(4x4,3x3) keeps them), else "f43"."""
    if pw.kdims == [4, 4]:
        return "f44"
    if pw.force_scheme is not None:                   # measurement / tests: pin the scheme of this filter
        return pw.force_scheme
    if pw.has("wino63"):
        c63 = -(-H // 6) * -(-W // 6) * 64
        c43 = -(-H // 4) * -(-W // 4) * 36
        if c63 <= (1.0 - WINO63_MIN_GAIN) * c43:
            return "f63"
    return "f43"

# Rounding guard of the F(6x6,3x3) route.  Measured on hostile statistics (profiles/r03a_wino_robustness.md: N(0,1), large
# positive means, log-normal channel gains, sparse spikes, 21 stacked convs) the scheme stays within 4.0e-5 * max|y| of the
# float64 conv at Cin = 1024 (F(4x4,3x3): 9.7e-6, direct: 6e-6), i.e. 5x inside the 2e-4 * max|y| bar of the per-tap tests.
# For weights / activations one does not trust, WINO63_CHECK_TOL (env RN_WINO63_CHECK_TOL, or Renderer.validate_winograd)
# turns on a self-check: before the FIRST F(6x6,3x3) launch of every filter both schemes run on that input WITHOUT epilogue (raw
# conv outputs: a residual would inflate the reference), and if max|y63 - y43| > tol * max|y43| the filter -- and its
# input-gradient pack -- is demoted to F(4x4,3x3) for good (two extra convs and one host sync per layer, once; off by default;
# never inside a hipGraph capture).  WINO63_DEMOTED lists the demotions.  RenderNet_demo.py --weights runs it at load.
WINO63_CHECK_TOL = float(os.environ["RN_WINO63_CHECK_TOL"]) if os.environ.get("RN_WINO63_CHECK_TOL") else None
WINO63_DEMOTED = []


def _wino43_fwd(x, pw, e, B, H, W, Cin, Cout, act, y_t=None, amax_out=None, route=None):
    """rn_conv2d_wino43_fwd / _wino63_fwd / _wino44_fwd with the workspace (V and M planes) from torch's caching allocator.
    pw: the PackedWeight whose .wino43 / .wino63 form the launch reads (a stride-1 transposed 4x4 pack pads two pixels before).
    y_t: the output tensor behind e[3] (needed by the F(6x6,3x3) self-check only).  amax_out: a list that receives the device word
    with max|y| when the launch produced one (split format H2).  route: the "wino3l" route of this launch (scheme, multiply stage);
    a caller that comes here on its own (the kernel tests) leaves it out and gets the one a stride-1 conv of this pack would take."""
    if route is None:
        route = _route("conv2d", pw, (H, W), (1, 1))
        if route.name != "wino3l":
            raise L.RenderNetHipError("this filter does not take the three-launch path on a %d x %d map" % (H, W))
    which, gemm = route.scheme, route.gemm
    if (which == "f63" and WINO63_CHECK_TOL is not None and y_t is not None and pw._wino63_verdict is None
            and pw.force_scheme is None and not torch.cuda.is_current_stream_capturing()):
        # Both schemes on the same input with NO epilogue (no bias, activation or residual): the residual of a res block or a
        # *_skip conv would inflate max|y| and hide a conv error well above tol * max|conv|.  Then the real launch.
        # The candidate is the route this launch would take (F(6x6,3x3) in the ACTIVE multiply-stage mode: bf16x3 by default); the
        # yardstick is F(4x4,3x3) on the exact-fp32 MFMA stage, the most accurate three-launch route there is -- so the check covers
        # the transform's rounding and the operand split in one comparison.
        raw = (None, None, None)
        y63, y43 = torch.empty_like(y_t), torch.empty_like(y_t)
        rc = _wino43_run(x, pw, raw + (L.ptr(y63), None), B, H, W, Cin, Cout, 0, "f63", gemm)
        if rc != 0:
            return rc
        rc = _wino43_run(x, pw, raw + (L.ptr(y43), None), B, H, W, Cin, Cout, 0, "f43", "f32")
        if rc != 0:
            return rc
        diff, ref = float((y63 - y43).abs().max()), float(y43.abs().max())
        pw._wino63_verdict = diff <= WINO63_CHECK_TOL * ref
        if not pw._wino63_verdict:
            WINO63_DEMOTED.append({"cin": Cin, "cout": Cout, "map": (H, W), "rel_diff": diff / max(ref, 1e-30), "mode": gemm_mode_now()})
            pw.demote()
            which, gemm = "f43", "f32"
    return _wino43_run(x, pw, e, B, H, W, Cin, Cout, act, which, gemm, amax_out)


# Multiply stage of the three-launch path: "f32" = exact-fp32 MFMA (v_mfma_f32_32x32x2_f32), "split" = the same products on
# the 16x faster bf16 pipe with every fp32 operand as three bf16 pieces and six piece products, fp32 accumulation
# (csrc/conv_wino_bf3.hip; fp32-class error, not bit-identical to "f32").  env RN_WINO_GEMM = the process default; per call: ops.gemm_mode(...).
# "split16": the same stage with every operand as TWO fp16 pieces of value / (power-of-two scale of its tensor) and three products --
# half the matrix work of "split"; 22-bit operands, fp32 accumulation (the accumulation error, which all three modes share, dominates).
# DEFAULT since round 5: "split" -- the bf16x3 form carries the full 24-bit significand of every fp32 operand (the three pieces sum
# EXACTLY to the fp32 value) and accumulates in fp32, its error against float64 equals the exact route's on every case of the hostile-
# statistics suite, and it is 1.3x faster end to end.  RN_WINO_GEMM=f32 restores the exact-fp32 MFMA stage everywhere (it is also what a
# filter is demoted to when the F(6x6,3x3) self-check above rejects it); "split16" is the opt-in fast mode.
GEMM_MODES = ("f32", "split", "split16")
WINO_GEMM = os.environ.get("RN_WINO_GEMM", "split")         # the PROCESS DEFAULT only: what a caller that names no mode gets
if WINO_GEMM not in GEMM_MODES:
    raise ValueError("RN_WINO_GEMM=%r: expected one of %s" % (WINO_GEMM, ", ".join(GEMM_MODES)))
# The mode of a call is the innermost `with ops.gemm_mode(m)` of the calling thread, else the process default above.  Renderer /
# TextureRenderer / Trainer / Reconstructor carry it as an attribute (`gemm=`) and enter the context around everything they launch, so
# two renderers of one process can run different modes; a conv's backward runs under the mode its forward captured (autograd calls it
# from its own thread).  Nothing in this module WRITES WINO_GEMM.
_MODE = threading.local()


def gemm_mode_now():
    """The multiply-stage mode of a launch made now by this thread."""
    return getattr(_MODE, "mode", None) or WINO_GEMM


@contextlib.contextmanager
def gemm_mode(mode):
    """`with ops.gemm_mode("f32" | "split" | "split16")`: every launch of this thread inside the block uses that multiply stage;
    None = leave whatever is in force."""
    if mode is None:
        yield
        return
    if mode not in GEMM_MODES:
        raise ValueError("gemm mode %r: expected one of %s" % (mode, ", ".join(GEMM_MODES)))
    prev = getattr(_MODE, "mode", None)
    _MODE.mode = mode
    try:
        yield
    finally:
        _MODE.mode = prev
# The fused 3x3x3 32 -> 32 kernel of the 3-D encoder has a bf16x3 variant too (csrc/conv3d_wino_bf3.hip: 0.50 ms against 0.82 ms on
# the B = 24 64x64x32 layer, error 2.4e-7 .. 3.8e-7 of max|y| against the fp32 kernel's 3.2e-7 .. 4.9e-7).  None: it follows
# WINO_GEMM ("split" turns both on); True / False (env RN_CONV3D_SPLIT=1 / 0) force it independently.
CONV3D_SPLIT = {"": None, "0": False}.get(os.environ.get("RN_CONV3D_SPLIT", ""), True)

# The gates of the routes (module constants: tests and measurements patch them)
WINO43_MIN_PIXELS = 64             # pixels per image from which a filter with a three-launch form takes that path (_use_wino43)
WINO63_MIN_GAIN = 0.08             # share of products F(6x6,3x3) must save over F(4x4,3x3) to be picked (_wino_scheme)
SPLIT11_MIN_PIXELS = 1024          # pixels per image from which a 1x1 filter takes the split GEMM stage (_use_split11)
CONV3D_SPLIT_MIN_ROWS = 8          # rows of tiles per image from which the split 3-D kernel is picked (_conv3d_split)
WGRAD_SPLIT = True                 # the filter gradients of the wide 2-D convs in split mode too (False: keep them on the exact-fp32 route)
CARRY_SKIP_GRADIENT = True         # res blocks: the skip path's gradient is added inside conv1's input-gradient launch (see _conv_apply)
# the wider of (Cin, Cout) from which the 2-D Winograd filter gradient takes the split GEMM stage.  Measured at crop 64: 1024 -> 1024 1.10 -> 0.79 ms, 1024 -> 512 (4x4)
# 0.92 -> 0.65; 512 -> 512 no gain on the 32x32x16 form of the stage, on the 16x16x32 form the training step goes 87.1 -> 85.9 ms (profiles/r06z_wgrad_min_ch.txt)
WGRAD_SPLIT_MIN_CH = 512


def _conv3d_split(B=None, H=None, W=None):
    """An item of the split kernel is a row of 16 tiles through the depth slices (ceil(H/2) * ceil(W/32) rows per image), cut into depth
    segments when the rows do not fill the 256 workgroups (csrc/conv3d_wino_bf3.hip: c3_depth_segments; res1 layer 0.048 against 0.057 ms
    at B = 1, 0.068 against 0.093 at B = 2).  The gate is a PER-IMAGE quantity (round 6, advisor finding on round 5's B * rows >= 64):
    a frame takes the same kernels, and gets the same bits, alone and inside a batch -- the split kernel's results do not depend on the
    item count (any segment count sums the same taps in the same order).  Maps of fewer than 8 rows of tiles per image (16 x 16 at crop
    32 is the smallest the nets produce: 8 rows) stay on the fp32 kernel.  B is accepted and ignored."""
    if CONV3D_SPLIT is not None:
        return bool(CONV3D_SPLIT)
    return gemm_mode_now() in ("split", "split16") and (H is None or ((H + 1) // 2) * ((W + 31) // 32) >= CONV3D_SPLIT_MIN_ROWS)


def _gemm_mode(pw, gemm=None):
    """The multiply-stage mode of a launch of this filter: the per-call override, else exact fp32 for a filter the self-check demoted,
    else the module-wide mode."""
    if gemm is not None:
        return gemm
    return "f32" if pw.gemm_f32 else gemm_mode_now()


def _wino43_run(x, pw, e, B, H, W, Cin, Cout, act, which, gemm=None, amax_out=None):
    """The three-launch path with scheme `which` on multiply stage `gemm` (None: the filter's, _gemm_mode): one C entry, or -- when a
    STAGE_HOOK wants the GEMM stage bracketed -- the same three launches through the stage entry points (_staged)."""
    lib = L.lib()
    gmode = _gemm_mode(pw, gemm)
    f44, f63, f11 = which == "f44", which == "f63", which == "f11"
    transposed = _transposed(pw)
    m = 6 if f63 else 1 if f11 else 4
    T = B * ((H + m - 1) // m) * ((W + m - 1) // m)
    scheme, nxi = (L.RN_WINO_F44, 49) if f44 else (L.RN_WINO_F63, 64) if f63 else (L.RN_WINO_F11, 1) if f11 else (L.RN_WINO_F43, 36)
    if f11 and gmode == "f32":
        raise L.RenderNetHipError("the 1x1 GEMM route exists on the split multiply stage only")
    st = L.stream_ptr()
    pad = 0 if f11 else 2 if (f44 and transposed) else 1
    if gmode in ("split", "split16") and lib.rn_winograd_split_supported(scheme, Cin, Cout):
        fmt = L.RN_SPLIT_FMT_H2 if gmode == "split16" else 0
        us = ctypes.c_void_p(pw.split(which, fmt).data_ptr())
        scheme |= fmt
        ws = torch.empty(lib.rn_winograd_split_workspace_bytes(scheme, B, H, W, Cin, Cout), dtype=torch.uint8, device=x.device)
        wsp = ctypes.c_void_p(ws.data_ptr())
        # format H2 scales every operand tensor by (a bound from) its max|x|: the launch that produced x left it in x._rn_amax (a device
        # word); without one the launcher makes a pass over x.  This launch leaves max|y| for the next layer the same way.
        ax = _amax_of(x) if fmt else None
        if fmt and ax is None and AMAX_MISSES is not None:
            AMAX_MISSES.append(("conv2d", which, Cin, Cout, H, W))
        ay = torch.empty(1, dtype=torch.int32, device=x.device) if fmt else None
        axp = ctypes.c_void_p(ax.data_ptr()) if ax is not None else None
        ayp = ctypes.c_void_p(ay.data_ptr()) if ay is not None else None
        if ay is not None and amax_out is not None:
            amax_out.append(ay)
        ev = _stage_events("gemm", T, Cin, Cout, which)
        if ev is None:
            return lib.rn_conv2d_winograd_split_fwd_ex(scheme, L.ptr(x), us, *e, wsp, B, H, W, Cin, Cout, transposed, act, axp, ayp, st)
        M = ctypes.c_void_p(ws.data_ptr() + lib.rn_winograd_split_v_bytes(scheme, T, Cin))
        return _staged(ev, lambda: lib.rn_winograd_split_input_transform_ex(scheme, L.ptr(x), wsp, B, H, W, Cin, pad, axp, st),
                       lambda: lib.rn_winograd_split_gemm(scheme, wsp, us, M, T, Cin, Cout, st),
                       lambda: lib.rn_winograd_output_transform_ex(scheme & 0xff, M, *e, B, H, W, Cout, act, ayp, st))
    u = pw.wino63 if f63 else pw.wino43
    n = (lib.rn_conv2d_wino44_workspace_floats if f44 else lib.rn_conv2d_wino63_workspace_floats if f63
         else lib.rn_conv2d_wino43_workspace_floats)(B, H, W, Cin, Cout)
    ws = torch.empty(n, dtype=torch.float32, device=x.device)
    ev = _stage_events("gemm", T, Cin, Cout, which)
    if ev is None:
        if f44:
            return lib.rn_conv2d_wino44_fwd(L.ptr(x), L.ptr(u), *e, L.ptr(ws), B, H, W, Cin, Cout, transposed, act, st)
        if f63:
            return lib.rn_conv2d_wino63_fwd(L.ptr(x), L.ptr(u), *e, L.ptr(ws), B, H, W, Cin, Cout, act, st)
        return lib.rn_conv2d_wino43_fwd(L.ptr(x), L.ptr(u), *e, L.ptr(ws), B, H, W, Cin, Cout, act, st)
    V, M = L.ptr(ws), ctypes.c_void_p(ws.data_ptr() + 4 * nxi * T * Cin)
    return _staged(ev, lambda: lib.rn_winograd_input_transform(scheme, L.ptr(x), V, B, H, W, Cin, pad, st),
                   lambda: lib.rn_winograd_gemm(scheme, V, L.ptr(u), M, T, Cin, Cout, st),
                   lambda: lib.rn_winograd_output_transform(scheme, M, *e, B, H, W, Cout, act, st))


def _use_wino43(pw, H, W):
    return pw.has("wino43") and H * W >= WINO43_MIN_PIXELS


def _use_split11(pw, pixels):
    """A 1x1 filter takes the split GEMM stage (three launches: split, GEMM, epilogue) in the split modes when ONE IMAGE has at least
    `SPLIT11_MIN_PIXELS` pixels (pixels = H * W: a per-image gate, so that a frame is routed alike alone and in a batch); below that the
    one-launch implicit-GEMM kernel wins.  32 x 32 (the projection unit at crop 64) is the smallest map measured faster on the stage."""
    return pw.has("split11") and _gemm_mode(pw) in ("split", "split16") and pixels >= SPLIT11_MIN_PIXELS


def _amax_of(x):
    """The device word with max|x| that the launch which produced x left on it (split format H2) -- only while x is what that launch
    wrote: an in-place change bumps the tensor's version counter and the word is ignored (the launcher then makes its own pass)."""
    tag = getattr(x, "_rn_amax", None)
    if tag is None:
        return None
    word, version = tag
    return word if _version_of(x) == version else None


def _version_of(t):
    """t._version, or None where the counter does not exist (tensors created under torch.inference_mode() raise on access): such a
    tensor gets no tag and the launcher makes its own pass over it."""
    try:
        return t._version
    except RuntimeError:
        return None


def _tag_amax(y, word):
    v = _version_of(y)
    if word is not None and v is not None:
        y._rn_amax = (word, v)


def _conv3d_split_launch(x, pw, e, B, H, W, D, Cin, Cout, act, st, amax_out=None):
    """The fused 3x3x3 32 -> 32 kernel in the split format of the mode: bf16x3 ("split"), fp16x2 ("split16": max|x| from the producing
    launch via x._rn_amax, else a pass; max|y| left for the consumer in amax_out)."""
    lib = L.lib()
    fmt = 1 if gemm_mode_now() == "split16" else 0
    us = ctypes.c_void_p(pw.split3d(fmt).data_ptr())
    if not fmt:
        return lib.rn_conv3d_winograd_split_fwd_ex(0, L.ptr(x), us, *e, B, H, W, D, Cin, Cout, act, None, None, None, st)
    ax = _amax_of(x)
    if ax is None and AMAX_MISSES is not None:
        AMAX_MISSES.append(("conv3d", Cin, Cout, H, W, D))
    words = torch.empty(2, dtype=torch.int32, device=x.device)       # [0]: max|y| for the consumer, [1]: scratch for a pass over x
    if amax_out is not None:
        amax_out.append(words[:1])
    return lib.rn_conv3d_winograd_split_fwd_ex(1, L.ptr(x), us, *e, B, H, W, D, Cin, Cout, act,
                                               ctypes.c_void_p(ax.data_ptr()) if ax is not None else None,
                                               ctypes.c_void_p(words.data_ptr() + 4), ctypes.c_void_p(words.data_ptr()), st)


# Which kernel a conv launch runs on.
# name: "split3d" (the fused 3x3x3 kernel on split operands) | "wino3d" (the same in fp32)                               -- 3-D
#       "wino3l" (three-launch Winograd; scheme "f43" | "f44" | "f63") | "split11" (1x1 on the split GEMM stage; scheme "f11")
#       | "wino2" (F(2x2,3x3)) | "wino4" (4x4 as four F(2x2,2x2)) | "convt_s2_wino" (4x4 stride-2 transposed, F(2x2,2x2) per phase)  -- 2-D
#       "direct" (the implicit-GEMM / tiled kernels: rn_<mode>_fwd_train, rn_<mode>_dgrad)
# gemm: the multiply stage of this filter's launches (_gemm_mode)
Route = collections.namedtuple("Route", "name scheme gemm")

# The routes whose epilogue takes the carried skip gradient as the residual of the input-gradient launch (see _Conv.forward, carry);
# on the others it is added to dx by one add_ afterwards.
CARRY_IN_EPILOGUE = frozenset(("split3d", "wino3d", "wino3l", "wino2"))


def _route(mode, pw, spatial, stride):
    """The route of a launch of LAYER flavour `mode` that reads pack `pw` on a map of `spatial` = (H, W[, D]) pixels: the forward with the
    layer's own pack, the input gradient with its dual (pw.dgrad_pack: the same conv with the flipped, transposed filter, so the same
    decision).  Host arithmetic on the filter's description only: nothing is packed, allocated or launched."""
    unit, forms = max(stride) == 1, pw.forms
    name, scheme = "direct", None
    if mode == "conv3d":
        if unit and "split3d" in forms and _conv3d_split(None, spatial[0], spatial[1]):
            name = "split3d"
        elif unit and "wino" in forms:
            name = "wino3d"
    elif mode in ("conv2d", "conv2d_transpose"):
        H, W = spatial
        if unit and _use_wino43(pw, H, W):
            name, scheme = "wino3l", _wino_scheme(pw, H, W)
        elif unit and mode == "conv2d" and _use_split11(pw, H * W):
            name, scheme = "split11", "f11"
        elif unit and mode == "conv2d" and "wino" in forms:
            name = "wino2"
        elif unit and "wino4" in forms:
            name = "wino4"
        elif mode == "conv2d_transpose" and stride[0] == 2 and pw.kind == L.RN_PACK_CONVT_S2 and "wino4" in forms:
            name = "convt_s2_wino"
    elif mode != "conv3d_transpose":
        raise ValueError(mode)
    return Route(name, scheme, _gemm_mode(pw))


def _launch_route(r, x, pw, e, act, y_t=None, amax_out=None):
    """The launch of route r (any but "direct"): the stride-1 conv (4x4 stride-2 transposed conv: "convt_s2_wino") of x with pack pw and the
    epilogue e = (bias, alpha, residual, y, z).  An input gradient is such a launch too: x = dz, pw = the dual pack, y = dx."""
    lib, st = L.lib(), L.stream_ptr()
    Cin, Cout = x.shape[-1], pw.cout
    if r.name == "split3d":
        return _conv3d_split_launch(x, pw, e, *x.shape[:4], Cin, Cout, act, st, amax_out)
    if r.name == "wino3d":
        return lib.rn_conv3d_wino_fwd(L.ptr(x), L.ptr(pw.wino), *e, *x.shape[:4], Cin, Cout, act, st)
    B, H, W = x.shape[:3]
    if r.name == "wino3l":
        return _wino43_fwd(x, pw, e, B, H, W, Cin, Cout, act, y_t, amax_out, r)
    if r.name == "split11":
        return _wino43_run(x, pw, e, B, H, W, Cin, Cout, act, "f11", r.gemm, amax_out)
    if r.name == "wino2":
        return lib.rn_conv2d_wino_fwd(L.ptr(x), L.ptr(pw.wino), *e, B, H, W, Cin, Cout, act, st)
    if r.name == "wino4":
        # (a stride-1 transposed pack -- a transposed conv's forward, a conv's input gradient -- pads two pixels before)
        return lib.rn_conv2d_wino4_fwd(L.ptr(x), L.ptr(pw.wino4), *e, B, H, W, Cin, Cout, _transposed(pw), act, st)
    if r.name == "convt_s2_wino":
        return lib.rn_conv2d_transpose_s2_wino_fwd(L.ptr(x), L.ptr(pw.wino4), *e, B, H, W, Cin, Cout, act, st)
    raise ValueError(r.name)


def _launch_direct(what, mode, x, pw, ptrs, ksize, stride, tail):
    """rn_<mode>_<what> (what: "fwd_train" | "dgrad" | "wgrad"), the kernels that take any filter size and stride: the pointers, the
    LAYER's dimensions (its input x, its forward pack pw), filter size and stride, `tail`."""
    ks = (L.ivec(ksize), L.ivec(stride)) if mode in ("conv2d", "conv3d") else (ksize[0], stride[0])
    return getattr(L.lib(), "rn_%s_%s" % (mode, what))(*ptrs, *x.shape, pw.cout, *ks, *tail)


def _launch_conv(mode, x, pw, bias, alpha, residual, y, z, ksize, stride, act, amax_out=None):
    e = (L.ptr(bias), L.ptr(alpha), L.ptr(residual), L.ptr(y), L.ptr(z))          # the epilogue arguments of every entry
    r = _route(mode, pw, x.shape[1:-1], stride)
    if r.name != "direct":
        return _launch_route(r, x, pw, e, act, y if mode == "conv2d" else None, amax_out)
    return _launch_direct("fwd_train", mode, x, pw, (L.ptr(x), L.ptr(pw.data)) + e, ksize, stride, (act, L.stream_ptr()))


def _wgrad_route(mode, fr, pw, x_shape, stride):
    """What the filter gradient of a layer runs on, from its FORWARD route fr and the shape of its input: "split3d" (rn_conv3d_wgrad_split) |
    "wino3l_split" (rn_conv2d_winograd_split_wgrad) | "wino43" | "wino44" | "wino2" (rn_conv2d_wino_wgrad) | "direct" (rn_<mode>_wgrad)."""
    lib = L.lib()
    Cin, Cout = x_shape[-1], pw.cout
    split = fr.gemm in ("split", "split16") and WGRAD_SPLIT
    if mode == "conv3d":
        # the 3-D encoder's 32 -> 32 filter gradients: the reduction over the positions on the bf16 pipe (bf16x3 in both split modes).
        # Wgrad-only conditions: the forward's per-image gate and CONV3D_SPLIT do not apply; one image must lie inside the 2 GiB
        # buffer window (else the exact kernel's launcher reports the limit)
        H, W, D = x_shape[1:4]
        if (split and pw.kdims == [3, 3, 3] and max(stride) == 1 and lib.rn_conv3d_wgrad_split_supported(Cin, Cout)
                and H * W * D * Cin * 4 < 0x80000000):
            return "split3d"
    elif mode == "conv2d" and fr.name == "wino3l":
        k3 = pw.kdims == [3, 3]
        if (split and max(Cin, Cout) >= WGRAD_SPLIT_MIN_CH
                and lib.rn_winograd_split_wgrad_supported(L.RN_WINO_F43 if k3 else L.RN_WINO_F44, Cin, Cout)):
            return "wino3l_split"
        if k3 and lib.rn_conv2d_wino43_wgrad_supported(Cin, Cout):
            return "wino43"
        if not k3 and lib.rn_conv2d_wino44_wgrad_supported(Cin, Cout):
            return "wino44"
    if mode == "conv2d" and fr.name in ("wino3l", "wino2") and pw.has("wino") and lib.rn_conv2d_wino_wgrad_supported(Cin, Cout):
        return "wino2"
    return "direct"


def _launch_wgrad(mode, fr, x, dz, dw, pw, ksize, stride, route=None):
    """dw += the filter gradient (TF layout) of the layer whose forward took route fr (route: a _wgrad_route name to run on instead of
    the one that decision gives -- measurements pin it; fr is then not looked at)."""
    lib, st = L.lib(), L.stream_ptr()
    name = route or _wgrad_route(mode, fr, pw, x.shape, stride)
    Cin, Cout = x.shape[-1], pw.cout
    if name == "split3d":
        return lib.rn_conv3d_wgrad_split(L.ptr(x), L.ptr(dz), L.ptr(dw), *x.shape[:4], Cin, Cout, st)
    if name == "direct":
        return _launch_direct("wgrad", mode, x, pw, (L.ptr(x), L.ptr(dz), L.ptr(dw)), ksize, stride, (st,))
    B, H, W = x.shape[:3]
    if name == "wino2":
        return lib.rn_conv2d_wino_wgrad(L.ptr(x), L.ptr(dz), L.ptr(dw), B, H, W, Cin, Cout, st)
    T, k3 = B * (-(-H // 4)) * (-(-W // 4)), pw.kdims == [3, 3]
    if name == "wino3l_split":
        # the reduction over the tiles on the bf16 pipe (csrc/conv_wino_bf3_wgrad.hip)
        sch = L.RN_WINO_F43 if k3 else L.RN_WINO_F44
        ws = torch.empty(lib.rn_winograd_split_wgrad_workspace_bytes(sch, B, H, W, Cin, Cout), dtype=torch.uint8, device=x.device)
        ev = _stage_events("wgrad", T, Cin, Cout, "f43s" if k3 else "f44s")
        return _bracketed(ev, lambda: lib.rn_conv2d_winograd_split_wgrad(sch, L.ptr(x), L.ptr(dz), L.ptr(dw), ctypes.c_void_p(ws.data_ptr()),
                                                                         B, H, W, Cin, Cout, st))
    if name == "wino43":
        ws = torch.empty(lib.rn_conv2d_wino43_wgrad_workspace_floats(B, H, W, Cin, Cout), dtype=torch.float32, device=x.device)
        ev = _stage_events("wgrad", T, Cin, Cout, "f43")
        return _bracketed(ev, lambda: lib.rn_conv2d_wino43_wgrad(L.ptr(x), L.ptr(dz), L.ptr(dw), L.ptr(ws), B, H, W, Cin, Cout, st))
    ws = torch.empty(lib.rn_conv2d_wino44_wgrad_workspace_floats(B, H, W, Cin, Cout), dtype=torch.float32, device=x.device)
    return lib.rn_conv2d_wino44_wgrad(L.ptr(x), L.ptr(dz), L.ptr(dw), L.ptr(ws), B, H, W, Cin, Cout, st)


def _out_shape(mode, x, pw, stride):
    sp = x.shape[1:-1]
    if mode in ("conv3d", "conv2d"):
        return (x.shape[0],) + tuple(-(-int(n) // int(s)) for n, s in zip(sp, stride)) + (pw.cout,)
    return (x.shape[0],) + tuple(int(n) * int(stride[0]) for n in sp) + (pw.cout,)


_EPI_WS = {}


def _epilogue_ws(device, C):
    """The partial-sum workspace of rn_epilogue_bwd_ws: one per (device, stream) -- its contents live only inside a call, calls on one
    stream are ordered -- grown to the widest layer seen (512 row blocks x [2][C] floats: 4 MiB at C = 1024)."""
    key = (device, torch.cuda.current_stream(device).cuda_stream)
    n = L.lib().rn_epilogue_bwd_workspace_floats(0, int(C))
    ws = _EPI_WS.get(key)
    if ws is None or ws.numel() < n:
        ws = _EPI_WS[key] = torch.empty(n, dtype=torch.float32, device=device)
    return ws


class _Conv(torch.autograd.Function):
    """y = sigmoid?( prelu?( conv(x, w) + bias ) + residual ) for the four conv flavours; one HIP launch
    forward (plus the saved pre-activation when training), three backward (epilogue, dgrad, wgrad)."""

    @staticmethod
    def forward(ctx, x, pw, bias, alpha, residual, ksize, stride, sigmoid, mode, anchor, elu=False, amax_box=None, carry=False):
        _chk_dev(x, pw.w_tf, bias, alpha, residual)
        ev = LAUNCH_HOOK(mode, tuple(x.shape), pw) if LAUNCH_HOOK is not None else None
        if ev is not None:
            ev[0].record()
        act = _act_code(alpha, sigmoid, elu)
        train = anchor is not None
        y = torch.empty(_out_shape(mode, x, pw, stride), dtype=torch.float32, device=x.device)
        if residual is not None and residual.shape != y.shape:
            raise L.RenderNetHipError("residual shape %s != output shape %s" % (tuple(residual.shape), tuple(y.shape)))
        z = torch.empty_like(y) if (train and alpha is not None) else None
        # split format H2: the launch leaves the device word with max|y| in `amax`; it travels to the consumer as a tag on y (the
        # caller's box carries it across _Conv.apply, which may hand back another tensor object for the same storage)
        amax = [] if amax_box is None else amax_box
        L.check(_launch_conv(mode, x, pw, bias, alpha, residual, y, z, ksize, stride, act, amax), "rn_%s_fwd" % mode)
        if amax:
            _tag_amax(y, amax[-1])
        if ev is not None:
            ev[1].record()
        if train:
            ctx.save_for_backward(x, z, y if (sigmoid or elu) else None)
            ctx.cfg = (pw, bias, alpha, residual is not None, tuple(ksize), tuple(stride), act, mode, TRAIN)
            ctx.gemm = gemm_mode_now()                # the backward runs on autograd's thread: it takes the forward's mode along
            ctx.carry = bool(carry)
        if carry:
            # training only (conv*(..., carry=True)): x rides along as a second output.  A res block hands THAT to its second conv as the
            # residual, so the skip path's gradient comes back into THIS node (as the gradient of the second output) and is added to dx
            # in the epilogue of the input-gradient launch -- instead of a separate read-modify-write add_ by the autograd engine
            # (27 per training step of the shader net, 100 MB tensors)
            return y, x.view_as(x)
        return y

    @staticmethod
    def backward(ctx, dy, dcarry=None):
        with gemm_mode(ctx.gemm):
            return _Conv._backward(ctx, dy, dcarry)

    @staticmethod
    def _backward(ctx, dy, dcarry=None):
        x, z, y = ctx.saved_tensors
        pw, bias, alpha, has_res, ksize, stride, act, mode, tc = ctx.cfg
        lib, st = L.lib(), L.stream_ptr()
        dy = dy.contiguous()
        C = dy.shape[-1]
        M = dy.numel() // C
        # 1. epilogue backward: dz (new buffer only when the values change), dbias, dalpha
        dz = torch.empty_like(dy) if act else dy
        if act or (bias is not None and not tc.frozen):
            ws = _epilogue_ws(dy.device, C)
            L.check(lib.rn_epilogue_bwd_ws(L.ptr(dy), L.ptr(z), L.ptr(y), L.ptr(alpha), L.ptr(dz) if act else None,
                                           L.ptr(tc.grad(bias)) if bias is not None else None,
                                           L.ptr(tc.grad_if_param(alpha)),
                                           M, C, act, L.ptr(ws), ws.numel(), st), "rn_epilogue_bwd_ws")
        d_res = None
        if has_res and ctx.needs_input_grad[4]:
            if act & L.RN_ACT_SIGMOID:
                raise L.RenderNetHipError("backward of sigmoid + residual in one epilogue is not supported")
            d_res = dy                      # PReLU sits before the residual add: its gradient is dy itself
        # 2. wgrad, accumulated into the registered gradient view (TF layout); none with frozen weights
        dw = tc.grad(pw.w_tf)
        spatial = x.shape[1:-1]
        if dw is not None:
            L.check(_launch_wgrad(mode, _route(mode, pw, spatial, stride), x, dz, dw, pw, ksize, stride), "rn_%s_wgrad" % mode)
        # 3. dgrad: the same conv with the dual pack (the flipped, transposed filter), dz in, dx out, no bias or activation
        dx = None
        if ctx.needs_input_grad[0]:
            dx = torch.empty_like(x)
            dp = pw.dgrad_pack(max(stride) == 1)
            r = _route(mode, dp, spatial, stride)
            # the gradient that came in through the carried copy of x (a res block's skip path): added by the launch's residual epilogue where
            # the route has one, by one add_ otherwise
            if dcarry is not None:
                dcarry = dcarry.contiguous()
            fused = dcarry is not None and r.name in CARRY_IN_EPILOGUE
            if r.name != "direct":
                rc = _launch_route(r, dz, dp, (None, None, L.ptr(dcarry) if fused else None, L.ptr(dx), None), 0)
            else:
                rc = _launch_direct("dgrad", mode, x, pw, (L.ptr(dz), L.ptr(dp.data), L.ptr(dx)), ksize, stride, (st,))
            L.check(rc, "rn_%s_dgrad" % mode)
            if dcarry is not None and not fused:
                dx.add_(dcarry)
        if not tc.frozen:
            tc.ready(pw.w_tf, bias, alpha)
        return dx, None, None, None, d_res, None, None, None, None, None, None, None, None


def _prep(x, pw):
    x = x.contiguous().float()
    if x.shape[-1] != pw.cin:
        raise L.RenderNetHipError("input has %d channels, filter expects %d" % (x.shape[-1], pw.cin))
    return x


def _conv_apply(x, pw, bias, alpha, residual, ksize, stride, sigmoid, mode, elu=False, carry=False):
    """carry=True: returns (y, x') with x' = x; under an ops.training context x' is a second output of the conv's graph node, and a gradient
    that reaches it (the skip path of a res block that uses x' as its residual) is added to dx inside the input-gradient launch."""
    anchor = TRAIN.anchor if (TRAIN is not None and torch.is_grad_enabled()) else None
    if anchor is None and not torch.is_grad_enabled():
        # inference: no graph to record -- skip the autograd.Function machinery (at batch 1 the 80 launches of a render
        # are host-bound; this is a fifth of the per-launch cost)
        y = _Conv.forward(None, x, pw, bias, alpha, residual, tuple(ksize), tuple(stride), sigmoid, mode, None, elu)
        return (y, x) if carry else y
    box = []
    fuse = bool(carry) and anchor is not None and CARRY_SKIP_GRADIENT
    out = _Conv.apply(x, pw, bias, alpha, residual, tuple(ksize), tuple(stride), sigmoid, mode, anchor, elu, box, fuse)
    xc = x
    if fuse:
        out, xc = out
    if box and getattr(out, "_rn_amax", None) is None:
        _tag_amax(out, box[-1])                                     # autograd returned another tensor object for the same storage
    return (out, xc) if carry else out


def conv3d(x, pw, bias=None, alpha=None, residual=None, stride=(1, 1, 1), sigmoid=False, elu=False, carry=False):
    x = _prep(x, pw)
    return _conv_apply(x, pw, bias, alpha, residual, pw.kdims, stride, sigmoid, "conv3d", elu, carry)


def conv2d(x, pw, bias=None, alpha=None, residual=None, stride=(1, 1), sigmoid=False, elu=False, carry=False):
    x = _prep(x, pw)
    return _conv_apply(x, pw, bias, alpha, residual, pw.kdims, stride, sigmoid, "conv2d", elu, carry)


def conv2d_transpose(x, pw, bias=None, alpha=None, residual=None, stride=(1, 1), sigmoid=False, elu=False):
    x = _prep(x, pw)
    if stride[0] != stride[1] or pw.kdims[0] != pw.kdims[1]:
        raise L.RenderNetHipError("conv2d_transpose: square kernels/strides only")
    return _conv_apply(x, pw, bias, alpha, residual, pw.kdims, stride, sigmoid, "conv2d_transpose", elu)


def conv3d_transpose(x, pw, bias=None, alpha=None, residual=None, stride=(1, 1, 1), sigmoid=False, elu=False):
    x = _prep(x, pw)
    return _conv_apply(x, pw, bias, alpha, residual, pw.kdims, stride, sigmoid, "conv3d_transpose", elu)


def res_stack_2d(x, blocks, skip=None):
    """A stack of res_block_2d (tools/layer_util.py:91-105: x + conv(prelu(conv(x)))) and, optionally, the *_skip conv behind
    it (conv(x_n) + skip residual; RenderNet_Shader.py:71-84, :91-99), 3x3 stride 1, C -> C throughout, as the loop over the
    per-layer launches.
        blocks: [(pw1, bias1, alpha1, pw2, bias2), ...]    skip: (pw, bias, residual tensor) | None"""
    net = x.contiguous().float()
    for pw1, b1, a1, pw2, b2 in blocks:
        h, net = conv2d(net, pw1, b1, a1, carry=True)      # (training: the skip path's gradient joins dx inside this conv's input-gradient launch)
        net = conv2d(h, pw2, b2, None, net)
    if skip is not None:
        net = conv2d(net, skip[0], skip[1], None, skip[2])
    return net


class _Projection(_ForwardOnly):
    @staticmethod
    def forward(ctx, x, pw, bias, alpha):
        _chk_dev(x, pw.w_tf, bias, alpha)
        B, H, W, D, C = x.shape
        y = torch.empty((B, H, W, D * C), dtype=torch.float32, device=x.device)
        L.check(L.lib().rn_projection_fwd(L.ptr(x), L.ptr(pw.data), L.ptr(bias), L.ptr(alpha), L.ptr(y),
                                          B, H, W, D, C, L.stream_ptr()), "rn_projection_fwd")
        return y


def projection(x, pw, bias, alpha):
    """x [B,H,W,D,C] -> prelu(1x1 conv over the depth-flattened features) [B,H,W,D*C]."""
    x = x.contiguous().float()
    if x.shape[3] * x.shape[4] != pw.cin or pw.cin != pw.cout:
        raise L.RenderNetHipError("projection: D*C=%d but filter is %dx%d" % (x.shape[3] * x.shape[4], pw.cin, pw.cout))
    B, H, W, D, C = x.shape
    if (TRAIN is not None and torch.is_grad_enabled()) or _route("conv2d", pw, (H, W), (1, 1)).name == "split11":
        # training: the same GEMM through the differentiable 1x1 conv2d path (the reshape is a view); split modes: that path takes the 1x1
        # filter through the split GEMM stage (exact fp32: the one-launch kernel below)
        return _conv_apply(x.view(B, H, W, D * C), pw, bias, alpha, None, (1, 1), (1, 1), False, "conv2d")
    return _Projection.apply(x, pw, bias, alpha)


class _FC(torch.autograd.Function):
    """y = prelu?(x @ w + b) (tools/layer_util.py:311-343); backward through rn_epilogue_bwd + rn_fully_connected_bwd."""

    @staticmethod
    def forward(ctx, x, w, bias, alpha, anchor):
        _chk_dev(x, w, bias, alpha)
        B, fin = x.shape
        fout = w.shape[1]
        train = anchor is not None
        y = torch.empty((B, fout), dtype=torch.float32, device=x.device)
        z = torch.empty_like(y) if (train and alpha is not None) else None
        act = _act_code(alpha, False)
        L.check(L.lib().rn_fully_connected_fwd_train(L.ptr(x), L.ptr(w), L.ptr(bias), L.ptr(alpha), L.ptr(y), L.ptr(z),
                                                     B, fin, fout, act, L.stream_ptr()), "rn_fully_connected_fwd")
        if train:
            ctx.save_for_backward(x, z)
            ctx.cfg = (w, bias, alpha, act, TRAIN)
        return y

    @staticmethod
    def backward(ctx, dy):
        x, z = ctx.saved_tensors
        w, bias, alpha, act, tc = ctx.cfg
        lib, st = L.lib(), L.stream_ptr()
        dy = dy.contiguous()
        B, fin = x.shape
        fout = w.shape[1]
        dz = torch.empty_like(dy) if act else dy
        if act or (bias is not None and not tc.frozen):
            L.check(lib.rn_epilogue_bwd(L.ptr(dy), L.ptr(z), None, L.ptr(alpha), L.ptr(dz) if act else None,
                                        L.ptr(tc.grad(bias)) if bias is not None else None,
                                        L.ptr(tc.grad(alpha)) if alpha is not None else None, B, fout, act, st),
                    "rn_epilogue_bwd")
        dx = torch.empty_like(x) if ctx.needs_input_grad[0] else None
        L.check(lib.rn_fully_connected_bwd(L.ptr(x), L.ptr(w), L.ptr(dz), L.ptr(dx), L.ptr(tc.grad(w)), B, fin, fout, st),
                "rn_fully_connected_bwd")
        if not tc.frozen:
            tc.ready(w, bias, alpha)
        return dx, None, None, None, None


def fully_connected(x, w, bias=None, alpha=None):
    anchor = TRAIN.anchor if (TRAIN is not None and torch.is_grad_enabled()) else None
    return _FC.apply(x.contiguous().float(), w.contiguous().float(), bias, alpha, anchor)


class _Dropout(torch.autograd.Function):
    """tf.nn.dropout through rn_dropout: the mask is a pure function of (seed, stream id, element index), so the
    backward regenerates it by running the same call on the gradient -- nothing is saved."""

    @staticmethod
    def forward(ctx, x, keep_prob, seed, stream_id):
        _chk_dev(x)
        y = torch.empty_like(x)
        L.check(L.lib().rn_dropout(L.ptr(x), L.ptr(y), x.numel(), keep_prob, seed, stream_id, L.stream_ptr()), "rn_dropout")
        ctx.cfg = (keep_prob, seed, stream_id)
        return y

    @staticmethod
    def backward(ctx, dy):
        keep_prob, seed, stream_id = ctx.cfg
        dy = dy.contiguous()              # may be an offset view of a larger gradient buffer: rn_dropout takes any alignment
        dx = torch.empty_like(dy)
        L.check(L.lib().rn_dropout(L.ptr(dy), L.ptr(dx), dy.numel(), keep_prob, seed, stream_id, L.stream_ptr()), "rn_dropout (bwd)")
        return dx, None, None, None


_DROPOUT_SEED = [0x5EED0FD50, 0]          # process-wide (seed, next stream id): every call draws a fresh stream


def mix_seed(*parts):
    """splitmix64 over a sequence of integers -> one 64-bit seed (e.g. (trainer seed, rank): ranks of a data-parallel job
    must not draw the same masks for their shards)."""
    z = 0x9E3779B97F4A7C15
    for p in parts:
        z = (z + (int(p) & (2 ** 64 - 1)) * 0xBF58476D1CE4E5B9 + 0x9E3779B97F4A7C15) & (2 ** 64 - 1)
        z ^= z >> 30
        z = (z * 0xBF58476D1CE4E5B9) & (2 ** 64 - 1)
        z ^= z >> 27
        z = (z * 0x94D049BB133111EB) & (2 ** 64 - 1)
        z ^= z >> 31
    return z


def seed_dropout(seed, first_stream=0):
    """Re-seed the dropout generator and set the id of the next stream: two runs with the same (seed, first_stream) and the
    same sequence of dropout calls draw the same masks.  The trainers call this at the start of every forward with
    seed = mix_seed(trainer seed, rank) and first_stream = global_step << 16, so a mask is a pure function of
    (seed, rank, step, position of the dropout site in the graph): independent across ranks and steps like tf.nn.dropout's,
    and a resumed run continues the sequence instead of replaying it."""
    _DROPOUT_SEED[0], _DROPOUT_SEED[1] = int(seed) & (2 ** 64 - 1), int(first_stream)


def dropout_state():
    return tuple(_DROPOUT_SEED)


def dropout(x, keep_prob, seed=None, stream_id=None):
    """tf.nn.dropout(x, keep_prob) (RenderNet_Shader.py:39 ...): x / keep_prob * floor(keep_prob + U[0,1)); the identity
    at keep_prob >= 1.  Differentiable.  (seed, stream_id) pin the mask; by default every call takes the next stream of
    the process-wide generator (see seed_dropout)."""
    if keep_prob >= 1.0 or x.numel() == 0:
        return x
    if seed is None:
        seed = _DROPOUT_SEED[0]
    if stream_id is None:
        stream_id = _DROPOUT_SEED[1]
        _DROPOUT_SEED[1] += 1
    return _Dropout.apply(x.contiguous().float(), float(keep_prob), int(seed), int(stream_id))


def prelu(x, alpha):
    """Stand-alone PReLU over the last dim (tools/layer_util.py:27-45)."""
    x = x.contiguous().float()
    _chk_dev(x, alpha)
    y = torch.empty_like(x)
    L.check(L.lib().rn_prelu_fwd(L.ptr(x), L.ptr(alpha), L.ptr(y), x.numel(), x.shape[-1], L.stream_ptr()),
            "rn_prelu_fwd")
    return y


PHONG_MODES = {"np_black": L.RN_PHONG_NP_BLACK, "np_white": L.RN_PHONG_NP_WHITE, "tf_black": L.RN_PHONG_TF_BLACK,
               "tf_white": L.RN_PHONG_TF_WHITE, "none": L.RN_PHONG_NO_MASK}


class _Phong(torch.autograd.Function):
    """Phong composite (all flavours of tools/Phong_shading.py) with TF's gradients w.r.t. the normal map, the light
    direction and the albedo it is multiplied with (Reconstruct_RenderNet_Face.py:377-378)."""

    @staticmethod
    def forward(ctx, normals, light_dir, light_col, albedo, ambient, k_diffuse, mode):
        _chk_dev(normals, light_dir, light_col, albedo)
        B, H, W, _ = normals.shape
        out = torch.empty_like(normals)
        L.check(L.lib().rn_phong_composite_ex_fwd(L.ptr(normals), L.ptr(light_dir), L.ptr(light_col), L.ptr(albedo),
                                                  ambient, k_diffuse, L.ptr(out), B, H, W, mode, L.stream_ptr()),
                "rn_phong_composite_ex_fwd")
        ctx.save_for_backward(normals, light_dir, light_col, albedo)
        ctx.cfg = (ambient, k_diffuse, mode)
        return out

    @staticmethod
    def backward(ctx, dout):
        normals, light_dir, light_col, albedo = ctx.saved_tensors
        ambient, k_diffuse, mode = ctx.cfg
        B, H, W, _ = normals.shape
        dout = dout.contiguous()
        dn = torch.empty_like(normals) if ctx.needs_input_grad[0] else None
        dl = torch.zeros_like(light_dir) if ctx.needs_input_grad[1] else None
        da = torch.empty_like(albedo) if (albedo is not None and ctx.needs_input_grad[3]) else None
        L.check(L.lib().rn_phong_composite_bwd(L.ptr(normals), L.ptr(light_dir), L.ptr(light_col), L.ptr(albedo),
                                               ambient, k_diffuse, L.ptr(dout), L.ptr(dn), L.ptr(dl), L.ptr(da),
                                               B, H, W, mode, L.stream_ptr()), "rn_phong_composite_bwd")
        return dn, dl, None, da, None, None, None


def phong_composite(normals, light_dir, light_col, ambient, k_diffuse, mode="np_black", albedo=None):
    """normals [B,H,W,3] in [0,1]; light_dir, light_col [B,3] -> shading [B,H,W,3] (times `albedo` when given).
    mode: mask flavour, see include/rendernet_hip.h (np_black = the demo)."""
    normals = normals.contiguous().float()
    if normals.dim() != 4 or normals.shape[-1] != 3:
        raise L.RenderNetHipError("phong_composite: normals must be [B,H,W,3], got %s" % (tuple(normals.shape),))
    B = normals.shape[0]
    light_dir = light_dir.float().expand(B, 3).contiguous()
    light_col = light_col.float().expand(B, 3).contiguous()
    if albedo is not None:
        albedo = albedo.contiguous().float()
        if albedo.shape != normals.shape:
            raise L.RenderNetHipError("phong_composite: albedo shape %s != normals shape %s" % (tuple(albedo.shape), tuple(normals.shape)))
    return _Phong.apply(normals, light_dir, light_col, albedo, float(ambient), float(k_diffuse), PHONG_MODES[mode])


# ---- The ingest, voxel, mesh, metric and ray-cast tools.  What their wrappers share comes first; `what` is the public function
# ---- the user called, which every message names.

GRID_SIDES = (32, 64, 128)         # the sides the voxel and mesh tools are built for (the ray caster also takes 96)


def _vp(t):
    """The device pointer of a tensor of any dtype for the C ABI; None -> NULL.  (L.ptr is the float32-only one.)"""
    return None if t is None else ctypes.c_void_p(t.data_ptr())


def _workspace(size_entry, dev, *shape):
    """What an entry with a workspace is given: (an int32 tensor on `dev`, its size in bytes), the size being what the entry's
    rn_*_workspace_bytes companion `size_entry` answers for `shape`."""
    nbytes = int(size_entry(*shape))
    return torch.empty((nbytes // 4,), dtype=torch.int32, device=dev), nbytes


def _one_of(values):
    return "%s or %s" % (", ".join(str(v) for v in values[:-1]), values[-1])


def _grid_side(what, S, sides=GRID_SIDES):
    """S as an int: an integer -- no bool, no float, not None -- out of `sides`."""
    if S is None or isinstance(S, (bool, float)) or int(S) not in sides:
        raise L.RenderNetHipError("%s: S=%r (%s)" % (what, S, _one_of(sides)))
    return int(S)


def _grid_view(vox):
    """[B,S,S,S,1] as its 4-D view, anything else as it is."""
    return vox[..., 0] if vox.dim() == 5 and vox.shape[4] == 1 else vox


def _occupancy(what, vox, sides=None):
    """Grids [B,S,S,S,1] or [B,S,S,S], cubic, with S out of `sides` where given: (the 4-D view, B, S)."""
    v = _grid_view(vox)
    if v.dim() != 4 or not (v.shape[1] == v.shape[2] == v.shape[3]) or (sides is not None and int(v.shape[1]) not in sides):
        raise L.RenderNetHipError("%s: expected [B,S,S,S,1] occupancy%s, got %s"
                                  % (what, "" if sides is None else " with S = " + _one_of(sides), tuple(vox.shape)))
    return v, int(v.shape[0]), int(v.shape[1])


def _finite(what, name, v, unit):
    """v as a float: a finite real number, no bool.  `unit` says in the message what the number is."""
    if isinstance(v, bool) or not isinstance(v, (int, float, np.integer, np.floating)) or not math.isfinite(v):
        raise L.RenderNetHipError("%s: %s=%r (a finite %s)" % (what, name, v, unit))
    return float(v)


def _u8_crop_args(shape, window, out_ch):
    """Shared argument check of target_u8_crop and its NumPy twin: returns (B, H, W, Cs, row0, col0, ph, pw)."""
    if len(shape) != 4:
        raise ValueError("frames must be [B, H, W, Cs], got shape %s" % (tuple(shape),))
    B, H, W, Cs = (int(v) for v in shape)
    row0, col0, ph, pw = (int(v) for v in window)
    if not ((out_ch == 1 and Cs in (1, 3, 4)) or (out_ch == 3 and Cs in (3, 4))):
        raise ValueError("frames with %d channels cannot give %d target channels (1 takes 1|3|4, 3 takes 3|4)" % (Cs, out_ch))
    if row0 < 0 or col0 < 0 or ph < 1 or pw < 1 or row0 + ph > H or col0 + pw > W:
        raise ValueError("window rows %d+%d cols %d+%d is outside the %dx%d frame" % (row0, ph, col0, pw, H, W))
    return B, H, W, Cs, row0, col0, ph, pw


def target_u8_crop(frames_u8, window, out_ch):
    """The training target from decoded 8-bit frames (rn_target_u8_crop_fwd): frames_u8 [B, H, W, Cs] uint8 on the device,
    window = (row0, col0, ph, pw) in frame pixels, out_ch 1 (greyscale: mean over all Cs channels) or 3 (colour: channels
    0..2) -> [B, ph, pw, out_ch] float32 in [0, 1], bit-equal to what the host path feeds (target_u8_crop_reference).
    No autograd: the target has no gradient."""
    _chk_dev(frames_u8)
    if frames_u8.dtype is not torch.uint8:
        raise L.RenderNetHipError("target_u8_crop takes uint8 frames, got %s" % frames_u8.dtype)
    B, H, W, Cs, row0, col0, ph, pw = _u8_crop_args(frames_u8.shape, window, int(out_ch))
    frames_u8 = frames_u8.contiguous()
    patch = torch.empty((B, ph, pw, int(out_ch)), dtype=torch.float32, device=frames_u8.device)
    L.check(L.lib().rn_target_u8_crop_fwd(_vp(frames_u8), L.ptr(patch), B, H, W, Cs, int(out_ch),
                                          row0, col0, ph, pw, L.stream_ptr()), "rn_target_u8_crop_fwd")
    return patch


def target_u8_crop_reference(frames_u8, window, out_ch):
    """NumPy statement of target_u8_crop, operation by operation what the host loader and the script compute today
    (tools/data_util.py data_loader, then `images / 255.0`, then the trainer's window): bytes -> float32; colour keeps
    channels 0..2; greyscale passes a single channel on and otherwise takes the float32 sum over ALL channels (alpha
    included) divided by float32(Cs) -- what np.mean(img, axis=2) returns on a float32 image; then the float32 division
    by 255.  The crop commutes with all of it (element-wise), so it is taken first."""
    import numpy as np
    f = np.asarray(frames_u8)
    if f.dtype != np.uint8:
        raise ValueError("target_u8_crop_reference takes uint8 frames, got %s" % f.dtype)
    B, H, W, Cs, row0, col0, ph, pw = _u8_crop_args(f.shape, window, int(out_ch))
    img = f[:, row0:row0 + ph, col0:col0 + pw, :].astype(np.float32)
    if int(out_ch) == 3:
        img = img[..., :3]
    elif Cs != 1:
        img = np.sum(img, axis=3, dtype=np.float32, keepdims=True) / np.float32(Cs)
    return img / np.float32(255.0)


def voxel_pack(vox, threshold=0.5):
    """vox [B,S,S,S,1] (or [B,S,S,S]) float32 or uint8 on the device -> (bits int32 [B, S^3/32], box int32 [B,6]): one bit
    per voxel with value > threshold, bit (i & 31) of word (i >> 5) for the flat index i = (zs*S + ys)*S + xs, and the
    occupied bounding box (x_lo, y_lo, z_lo, x_hi, y_hi, z_hi), inclusive; an empty item gets (S, S, S, -1, -1, -1)
    (rn_voxel_pack).  No autograd."""
    _chk_dev(vox)
    vox, B, S = _occupancy("voxel_pack", vox)
    if vox.dtype is not torch.uint8:
        vox = vox.float()
    vox = vox.contiguous()
    bits = torch.empty((B, max(S ** 3 // 32, 1)), dtype=torch.int32, device=vox.device)
    box = torch.empty((B, 6), dtype=torch.int32, device=vox.device)
    L.check(L.lib().rn_voxel_pack(_vp(vox), 1 if vox.dtype is torch.uint8 else 0, float(threshold), _vp(bits), _vp(box), B, S,
                                  L.stream_ptr()), "rn_voxel_pack")
    return bits, box


def voxel_shapes(prims, S=64):
    """prims int32 [B,K,16] on the device, 0 <= K <= 8 primitives per item -> uint8 [B,S,S,S,1] on the same device, S = 32 or
    64: the occupancy grid (0 or 1, flat index (zs*S + ys)*S + xs, what `voxel_pack` reads) of the constructive-solid-geometry
    description in `prims` -- per primitive word 0 = type | op << 8 (ellipsoid, box, cylinder, cone, torus; union or
    subtraction, applied in slot order; 255 marks an unused slot), the centre, the semi-axes and the rotation times 64, all
    integers, clamped by the kernel (rn_voxel_shapes; include/rendernet_hip.h states the rule and its bounds).
    `synth.shape_prims` draws such descriptions from a seed.  No autograd."""
    if not torch.is_tensor(prims):
        raise L.RenderNetHipError("voxel_shapes: expected an int32 tensor [B,K,16], got %s" % type(prims).__name__)
    _chk_dev(prims)
    if prims.dtype is not torch.int32 or prims.dim() != 3 or prims.shape[2] != 16 or prims.shape[1] > L.RN_SHAPES_MAX_PRIMS:
        raise L.RenderNetHipError("voxel_shapes: expected int32 [B,K,16] with K <= %d, got %s %s"
                                  % (L.RN_SHAPES_MAX_PRIMS, prims.dtype, tuple(prims.shape)))
    B, K, S = int(prims.shape[0]), int(prims.shape[1]), _grid_side("voxel_shapes", S, (32, 64))
    if B > 65535:
        raise L.RenderNetHipError("voxel_shapes: B=%d (at most 65535 per call)" % B)
    prims = prims.contiguous()
    vox = torch.empty((B, S, S, S, 1), dtype=torch.uint8, device=prims.device)
    L.check(L.lib().rn_voxel_shapes(_vp(prims) if K else None, _vp(vox), B, K, S, L.stream_ptr()), "rn_voxel_shapes")
    return vox


MESH_LISTS = ("small_solid", "large_solid", "small_surf", "large_surf")


def voxelize_mesh(q, tris=None, S=64, mode="both", return_bits=False, lists=None, device=None):
    """The occupancy grid of a triangle mesh on the device: uint8 [1,S,S,S,1], 0 or 1, and with `return_bits` also the packed
    mask int32 [1, S^3/32] in the layout of `voxel_pack` (rn_mesh_voxelize; include/rendernet_hip.h states the two rules and
    their bounds).  `q` int32 [V,3] are lattice coordinates, 256 units per voxel, column j = array axis j (`mesh.fit` makes
    them; the kernel clamps them to [0, 256 S]); `tris` int32 [T,3] vertex indices.  Either both are device tensors -- they are
    read back once, `mesh.prepare` drops the zero-area triangles and builds the work lists, which are uploaded -- or `q` is the
    dict `mesh.prepare` returned, uploaded to `device` (default "cuda").  `lists` (a dict of the four int32 index arrays
    "small_solid", "large_solid", "small_surf", "large_surf") replaces prepare's split; `tris` is then used as given.
    S is 32, 64 or 128; mode "solid" (parity of the crossings along array axis 2 at the voxel centres), "surface" (every voxel
    a triangle touches) or "both", their union.  T = 0 gives an empty grid.  dtype, shapes, the index range, S and the mode are
    checked before anything is launched.  No autograd."""
    from . import mesh as M
    err = L.RenderNetHipError
    S = _grid_side("voxelize_mesh", S, M.SIZES)
    if mode not in M.MODES:
        raise err("voxelize_mesh: mode=%r (solid, surface or both)" % (mode,))
    if isinstance(q, dict):
        if tris is not None or lists is not None:
            raise err("voxelize_mesh: a prepared dict brings its own triangles and lists")
        if int(q.get("S", S)) != S:
            raise err("voxelize_mesh: the lists were prepared for S=%r, not %d" % (q.get("S"), S))
        prepared, device = q, torch.device(device if device is not None else "cuda")
    else:
        for name, t in (("q", q), ("tris", tris)):
            if not torch.is_tensor(t):
                raise err("voxelize_mesh: expected an int32 tensor [n,3] for %s, got %s" % (name, type(t).__name__))
            if t.dtype is not torch.int32 or t.dim() != 2 or t.shape[1] != 3:
                raise err("voxelize_mesh: expected int32 [n,3] for %s, got %s %s" % (name, t.dtype, tuple(t.shape)))
        _chk_dev(q, tris)
        if device is not None and torch.device(device).type != "cuda":
            raise err("voxelize_mesh: device=%r; there is no CPU path" % (device,))
        device = q.device
        hq, ht = q.cpu().numpy(), tris.cpu().numpy()
        if len(ht) and (int(ht.min()) < 0 or int(ht.max()) >= len(hq)):
            raise err("voxelize_mesh: a triangle index outside [0, %d)" % len(hq))
        if lists is None:
            prepared = M.prepare(hq, ht, S)
        else:
            prepared = {"q": hq, "tris": ht}
            for name in MESH_LISTS:
                a = np.asarray(lists.get(name, ()))
                if a.size and (a.dtype.kind not in "iu" or a.ndim != 1 or int(a.min()) < 0 or int(a.max()) >= len(ht)):
                    raise err("voxelize_mesh: lists[%r] must be indices into the %d triangles" % (name, len(ht)))
                prepared[name] = a.astype(np.int32).reshape(-1)
    if device.type != "cuda":
        raise err("rendernet_amd ops need a HIP device (got %s); there is no CPU path" % device)
    hq, ht = np.ascontiguousarray(prepared["q"], np.int32), np.ascontiguousarray(prepared["tris"], np.int32)
    if hq.ndim != 2 or hq.shape[1] != 3 or ht.ndim != 2 or ht.shape[1] != 3:
        raise err("voxelize_mesh: expected q [V,3] and tris [T,3], got %s and %s" % (hq.shape, ht.shape))
    V, T = len(hq), len(ht)
    if T and (int(ht.min()) < 0 or int(ht.max()) >= V):
        raise err("voxelize_mesh: a triangle index outside [0, %d)" % V)
    host = [np.ascontiguousarray(prepared[name], np.int32).reshape(-1) for name in MESH_LISTS]
    for name, a in zip(MESH_LISTS, host):
        if a.size and (int(a.min()) < 0 or int(a.max()) >= T):
            raise err("voxelize_mesh: %s holds an index outside the %d triangles" % (name, T))
    # one upload: vertices, triangles and the four lists behind one another, each part starting on 16 bytes
    parts, offs, n = [hq.reshape(-1), ht.reshape(-1)] + host, [], 0
    for a in parts:
        offs.append(n)
        n += (a.size + 3) // 4 * 4
    flat = np.zeros(max(n, 4), np.int32)
    for a, o in zip(parts, offs):
        flat[o:o + a.size] = a
    dev = torch.as_tensor(flat).to(device)
    words = S ** 3 // 32
    ws = torch.empty((2 * words,), dtype=torch.int32, device=device)
    bits = torch.empty((1, words), dtype=torch.int32, device=device)
    vox = torch.empty((1, S, S, S, 1), dtype=torch.uint8, device=device)

    def at(k):
        return ctypes.c_void_p(dev.data_ptr() + 4 * offs[k]) if parts[k].size else None
    with torch.cuda.device(device):
        L.check(L.lib().rn_mesh_voxelize(at(0), V, at(1), T, at(2), host[0].size, at(3), host[1].size, at(4), host[2].size,
                                         at(5), host[3].size, _vp(ws), _vp(bits), _vp(vox), S, M.MODES[mode], L.stream_ptr()),
                "rn_mesh_voxelize")
    return (vox, bits) if return_bits else vox


class ExtractedMesh(object):
    """What `extract_mesh` returns, all on the device: `q` int32 [V,3] lattice vertices (256 units per voxel, column j = array
    axis j), `faces` int32 [F,4] quads (or [2F,3] triangles) of vertex indices LOCAL to their grid, and `vert_offsets`,
    `face_offsets` int64 [B+1]: grid b owns q[vert_offsets[b]:vert_offsets[b+1]] and faces[face_offsets[b]:face_offsets[b+1]]."""
    __slots__ = ("q", "faces", "vert_offsets", "face_offsets")

    def __init__(self, q, faces, vert_offsets, face_offsets):
        self.q, self.faces, self.vert_offsets, self.face_offsets = q, faces, vert_offsets, face_offsets

    def grid(self, b):
        """(q, faces) of grid b, as views."""
        vo, fo = self.vert_offsets.tolist(), self.face_offsets.tolist()
        return self.q[vo[b]:vo[b + 1]], self.faces[fo[b]:fo[b + 1]]


def _extract_args(vol, threshold, smooth, triangles):
    """The checks of extract_mesh that need no device: (vol [B,S,S,S], threshold)."""
    err = L.RenderNetHipError
    if not torch.is_tensor(vol):
        raise err("extract_mesh: expected a float32 or uint8 tensor [B,S,S,S,1], got %s" % type(vol).__name__)
    if vol.dtype not in (torch.float32, torch.uint8):
        raise err("extract_mesh: expected float32 or uint8 voxels, got %s" % vol.dtype)
    vol, B, _ = _occupancy("extract_mesh", vol, GRID_SIDES)
    if B > 65535:
        raise err("extract_mesh: B=%d (at most 65535 per call)" % B)
    threshold = _finite("extract_mesh", "threshold", threshold, "number")
    if not isinstance(smooth, bool) or not isinstance(triangles, bool):
        raise err("extract_mesh: smooth=%r triangles=%r (True or False)" % (smooth, triangles))
    return vol, threshold


RELAX_MAX_PASSES = 64              # include/rendernet_hip.h, rn_mesh_relax
RELAX_MAX_WEIGHT = 256


def _relax_args(what, relax, relax_weight):
    """The checks of the relaxation arguments, which need no device: (passes, weight) as ints."""
    err = L.RenderNetHipError
    for name, v, lo, hi in (("relax", relax, 0, RELAX_MAX_PASSES), ("relax_weight", relax_weight, 1, RELAX_MAX_WEIGHT)):
        if isinstance(v, bool) or not isinstance(v, int) or not lo <= v <= hi:
            raise err("%s: %s=%r (an int %d..%d)" % (what, name, v, lo, hi))
    return int(relax), int(relax_weight)


def extract_mesh(vol, threshold=0.5, smooth=True, triangles=False, relax=0, relax_weight=256):
    """The surface-net mesh of voxel grids on the device: vol [B,S,S,S,1] (or [B,S,S,S]) float32 or uint8, S = 32, 64 or 128 ->
    ExtractedMesh (q, faces, vert_offsets, face_offsets).  A sample is inside iff value > threshold, the bits `voxel_pack`
    returns; everything outside the grid is outside.  One vertex per cell of 2^3 samples that the surface crosses -- `smooth`
    places it at the rounded mean of the edge crossings, clamped strictly inside the cell; otherwise on the voxel corner, which
    gives exactly the exposed voxel faces -- and one quad per pair of neighbouring samples that differ, wound so that its normal
    points outwards (`triangles` fans it as (0,1,2),(0,2,3)).  Vertices are in cell order, quads by (owning cell, axis): the
    same input gives the same arrays on every call, and `voxelize_mesh(..., mode="solid")` of the mesh returns the inside set
    voxel for voxel (rn_mesh_extract_count / _emit; include/rendernet_hip.h states the rule).
    The per-grid totals [B,2] are read back ONCE between the count and the emit launches to size the outputs, as `torch.nonzero`
    does; dtype, shape, S, device and finiteness are checked before anything is launched.  An empty grid gives zero vertices
    and faces.
    `relax` > 0 adds that many passes of surface-net relaxation (rn_mesh_relax), which on a binary grid turn the terraced surface
    into a smooth one: every vertex moves `relax_weight` / 256 of the way towards the mean of its linked neighbours and stays
    inside its own cell.  Only `q` changes: faces, order, offsets, `mesh_vertex_colours` and the solid round trip are the same.
    4 passes at weight 256 is the recommended setting and more is not better (the surface shrinks against the cell walls:
    DESIGN.md 5c).  `relax` with smooth=False starts from the cell centres.  relax=0 is the mesh without it, byte for byte.
    No autograd."""
    vol, threshold = _extract_args(vol, threshold, smooth, triangles)
    relax, relax_weight = _relax_args("extract_mesh", relax, relax_weight)
    _chk_dev(vol)
    vol = vol.detach().contiguous()
    if vol.dtype is torch.float32 and not bool(torch.isfinite(vol).all()):
        raise L.RenderNetHipError("extract_mesh: the voxels hold a non-finite value")
    B, S, dev = int(vol.shape[0]), int(vol.shape[1]), vol.device
    width = 3 if triangles else 4
    vert_offsets = torch.zeros((B + 1,), dtype=torch.int64, device=dev)
    quad_offsets = torch.zeros((B + 1,), dtype=torch.int64, device=dev)
    if B == 0:
        return ExtractedMesh(torch.empty((0, 3), dtype=torch.int32, device=dev),
                             torch.empty((0, width), dtype=torch.int32, device=dev), vert_offsets, quad_offsets)
    lib = L.lib()
    is_u8 = 1 if vol.dtype is torch.uint8 else 0
    ws, nws = _workspace(lib.rn_mesh_extract_workspace_bytes, dev, B, S)
    totals = torch.empty((B, 2), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.rn_mesh_extract_count(_vp(vol), is_u8, threshold, B, S, _vp(ws), nws, _vp(totals), L.stream_ptr()),
                "rn_mesh_extract_count")
        sums = torch.cumsum(totals.long(), 0)
        vert_offsets[1:] = sums[:, 0]
        quad_offsets[1:] = sums[:, 1]
        n_verts, n_quads = (int(v) for v in sums[-1].tolist())                             # the one read-back
        q = torch.empty((n_verts, 3), dtype=torch.int32, device=dev)
        faces = torch.empty((n_quads * (2 if triangles else 1), width), dtype=torch.int32, device=dev)
        if n_verts:
            cellvert = torch.empty((B, (S + 1) ** 3), dtype=torch.int32, device=dev)
            L.check(lib.rn_mesh_extract_emit(_vp(vol), is_u8, threshold, B, S, L.RN_EXTRACT_SMOOTH if smooth else L.RN_EXTRACT_BLOCKY,
                                             1 if triangles else 0, _vp(ws), nws, _vp(vert_offsets), _vp(quad_offsets), n_verts, n_quads,
                                             _vp(cellvert), _vp(q), _vp(faces) if n_quads else None, L.stream_ptr()),
                    "rn_mesh_extract_emit")
            if relax:
                rws, nrws = _workspace(lib.rn_mesh_relax_workspace_bytes, dev, n_verts)
                L.check(lib.rn_mesh_relax(_vp(vol), is_u8, threshold, B, S, _vp(cellvert), _vp(vert_offsets), n_verts, relax,
                                          relax_weight, _vp(rws), nrws, _vp(q), L.stream_ptr()), "rn_mesh_relax")
    return ExtractedMesh(q, faces, vert_offsets, quad_offsets * 2 if triangles else quad_offsets)


class MergedMesh(ExtractedMesh):
    """What `extract_mesh_merged` returns: the arrays of an `ExtractedMesh` and, per QUAD (also when `faces` holds its two fan
    triangles), `face_voxel` int32 [F] the flat index within its grid of the inside voxel at the rectangle's corner (u0, v0),
    `face_dir` int32 [F] = 2 a + side (the normal is +a on side 0 and -a on side 1) and `face_size` int32 [F,2] the rectangle's
    extent in voxels along (u, v) = (a + 1, a + 2) mod 3."""
    __slots__ = ("face_voxel", "face_dir", "face_size")

    def __init__(self, q, faces, vert_offsets, face_offsets, face_voxel, face_dir, face_size):
        ExtractedMesh.__init__(self, q, faces, vert_offsets, face_offsets)
        self.face_voxel, self.face_dir, self.face_size = face_voxel, face_dir, face_size

    def unshared(self):
        """The same faces with private vertices, one per face corner in face order: what a writer of per-vertex colours needs,
        because two rectangles of different colour may share a corner.  A torch gather."""
        faces = self.faces
        F, width = int(faces.shape[0]), int(faces.shape[1])
        with torch.no_grad():
            fo = self.face_offsets
            grid = torch.searchsorted(fo[1:].contiguous(), torch.arange(F, dtype=torch.int64, device=faces.device), right=True)
            grid = grid.clamp_(max=max(int(fo.shape[0]) - 2, 0))
            q = self.q[(faces.long() + self.vert_offsets[grid][:, None]).reshape(-1)].contiguous()
            local = torch.arange(F, dtype=torch.int64, device=faces.device) - fo[grid]
            new = (width * local[:, None] + torch.arange(width, dtype=torch.int64, device=faces.device)[None]).to(torch.int32)
        return MergedMesh(q, new.contiguous(), fo * width, fo, self.face_voxel, self.face_dir, self.face_size)


def _merge_labels(labels, vol):
    """The checks of extract_mesh_merged's labels, which need no launch: int32, the grids' B and S, on their device."""
    if labels is None:
        return None
    err = L.RenderNetHipError
    if not torch.is_tensor(labels) or labels.dtype is not torch.int32:
        raise err("extract_mesh_merged: expected labels as an int32 tensor [B,S,S,S], got %s"
                  % (labels.dtype if torch.is_tensor(labels) else type(labels).__name__))
    if labels.dim() == 5 and labels.shape[-1] == 1:
        labels = labels[..., 0]
    if tuple(labels.shape) != tuple(vol.shape) or labels.device != vol.device:
        raise err("extract_mesh_merged: labels %s on %s for grids %s on %s"
                  % (tuple(labels.shape), labels.device, tuple(vol.shape), vol.device))
    return labels.detach().contiguous()


def extract_mesh_merged(vol, threshold=0.5, labels=None, triangles=False):
    """The blocky mesh of voxel grids with coplanar faces merged into rectangles, on the device (rn_mesh_merge_count / _emit;
    include/rendernet_hip.h states the rule): vol [B,S,S,S,1] (or [B,S,S,S]) float32 or uint8, S = 32, 64 or 128 -> MergedMesh
    (q, faces, vert_offsets, face_offsets, face_voxel, face_dir, face_size).  The surface is exactly that of
    `extract_mesh(smooth=False)`: per axis, plane and side the exposed faces are cut into maximal runs along v, and a run that
    the row above holds identically continues that rectangle -- a run merge, not an optimal cover, so every rectangle is a
    function of the bits alone.  `labels` int32 [B,S,S,S] keeps faces of voxels with different labels apart (only equality is
    used).  Quads are ordered by (axis, plane, side, u0, v0) and wound outwards; vertices are the lattice corners in use, shared,
    in the blocky extractor's order; `triangles` fans each quad as (0,1,2),(0,2,3).  The same input gives the same arrays on
    every call, and `voxelize_mesh(..., mode="solid")` of the mesh returns the inside set voxel for voxel.
    The merged form is for export, voxelisation and area statistics.  It has T-junctions -- a corner of one rectangle inside
    another's edge -- and `rasterize_mesh` keeps every pixel on shared edges only, so a merged mesh drawn there may lose or double
    single pixels along such edges: the unit-quad form is the one to draw.
    The per-grid totals [B,2] are read back ONCE between the count and the emit launches; dtype, shape, S, device, finiteness
    and the labels are checked before anything is launched.  An empty grid gives zero vertices and faces.  No autograd."""
    vol, threshold = _extract_args(vol, threshold, False, triangles)
    labels = _merge_labels(labels, vol)
    _chk_dev(vol)
    vol = vol.detach().contiguous()
    if vol.dtype is torch.float32 and not bool(torch.isfinite(vol).all()):
        raise L.RenderNetHipError("extract_mesh_merged: the voxels hold a non-finite value")
    B, S, dev = int(vol.shape[0]), int(vol.shape[1]), vol.device
    width = 3 if triangles else 4
    vert_offsets = torch.zeros((B + 1,), dtype=torch.int64, device=dev)
    quad_offsets = torch.zeros((B + 1,), dtype=torch.int64, device=dev)

    def result(q, faces, n_quads):
        per_quad = [torch.empty(shape, dtype=torch.int32, device=dev) for shape in ((n_quads,), (n_quads,), (n_quads, 2))]
        return MergedMesh(q, faces, vert_offsets, quad_offsets * 2 if triangles else quad_offsets, *per_quad)
    if B == 0:
        return result(torch.empty((0, 3), dtype=torch.int32, device=dev), torch.empty((0, width), dtype=torch.int32, device=dev), 0)
    lib = L.lib()
    ws, nws = _workspace(lib.rn_mesh_merge_workspace_bytes, dev, B, S)
    totals = torch.empty((B, 2), dtype=torch.int32, device=dev)
    with torch.cuda.device(dev):
        L.check(lib.rn_mesh_merge_count(_vp(vol), 1 if vol.dtype is torch.uint8 else 0, _vp(labels), threshold, B, S, _vp(ws), nws,
                                        _vp(totals), L.stream_ptr()), "rn_mesh_merge_count")
        sums = torch.cumsum(totals.long(), 0)
        vert_offsets[1:] = sums[:, 0]
        quad_offsets[1:] = sums[:, 1]
        n_verts, n_quads = (int(v) for v in sums[-1].tolist())                             # the one read-back
        out = result(torch.empty((n_verts, 3), dtype=torch.int32, device=dev),
                     torch.empty((n_quads * (2 if triangles else 1), width), dtype=torch.int32, device=dev), n_quads)
        if n_quads:
            L.check(lib.rn_mesh_merge_emit(_vp(labels), B, S, 1 if triangles else 0, _vp(ws), nws, _vp(vert_offsets), _vp(quad_offsets),
                                           n_verts, n_quads, _vp(out.q), _vp(out.faces), _vp(out.face_voxel), _vp(out.face_dir),
                                           _vp(out.face_size), L.stream_ptr()), "rn_mesh_merge_emit")
    return out


def merged_face_colours(mesh, colours, known=None, unseen=(128, 128, 128)):
    """The colour of every quad of a `MergedMesh`: colours[face_voxel], from colours uint8 [B,S,S,S,3] (and known uint8
    [B,S,S,S]) as `voxel_colours` returns them for the grids the mesh was extracted from -> uint8 [F,3], `unseen` where `known`
    is 0.  With the packed colour as the label every voxel under a rectangle has this colour.  A torch gather.  No autograd."""
    what = "merged_face_colours"
    if not isinstance(mesh, MergedMesh):
        raise L.RenderNetHipError("%s: expected a MergedMesh (ops.extract_mesh_merged), got %s" % (what, type(mesh).__name__))
    colours, known, B, S = _colour_grids(what, colours, known)
    unseen = _colour_bytes(what, "unseen", unseen)
    ids = mesh.face_voxel
    F, dev = int(ids.shape[0]), ids.device
    if dev != colours.device or int(mesh.vert_offsets.shape[0]) != B + 1:
        raise L.RenderNetHipError("%s: a mesh of %d grids on %s for %d coloured grids on %s"
                                  % (what, int(mesh.vert_offsets.shape[0]) - 1, dev, B, colours.device))
    if F == 0:
        return torch.empty((0, 3), dtype=torch.uint8, device=dev)
    with torch.no_grad():
        per_quad = mesh.face_offsets // (int(mesh.faces.shape[0]) // F)
        grid = torch.searchsorted(per_quad[1:].contiguous(), torch.arange(F, dtype=torch.int64, device=dev), right=True).clamp_(max=B - 1)
        flat = grid * S ** 3 + ids.clamp(0, S ** 3 - 1).long()
        out = colours.reshape(-1, 3)[flat]
        if known is not None:
            fill = torch.tensor(unseen, dtype=torch.uint8, device=dev)
            out = torch.where((known.reshape(-1)[flat] != 0)[:, None], out, fill[None])
        return out.contiguous()


MESH_CULL = {"none": L.RN_CULL_NONE, "back": L.RN_CULL_BACK}
RASTER_MAX_SIDE = 2048             # pixels_per_cell * new_size (include/rendernet_hip.h, rn_mesh_rasterize: the bounds need it)
RASTER_MAX_ROWS = 1 << 28          # vertices, triangles or faces of a concatenated set


def _mesh_set_args(what, q, tris, S, vert_offsets, tri_offsets):
    """The checks a mesh set gets before anything is launched: (q, tris, vert_offsets, tri_offsets, M, host tri_offsets | None)."""
    err = L.RenderNetHipError
    _grid_side(what, S)
    for name, t in (("q", q), ("tris", tris)):
        if not torch.is_tensor(t):
            raise err("%s: expected an int32 tensor [n,3] for %s, got %s" % (what, name, type(t).__name__))
        if t.dtype is not torch.int32 or t.dim() != 2 or t.shape[1] != 3:
            raise err("%s: expected int32 [n,3] for %s, got %s %s" % (what, name, t.dtype, tuple(t.shape)))
    _chk_dev(q, tris)
    V, T = int(q.shape[0]), int(tris.shape[0])
    if T and not V:
        raise err("%s: %d triangles without vertices" % (what, T))
    if (vert_offsets is None) != (tri_offsets is None):
        raise err("%s: vert_offsets and tri_offsets come together" % what)
    host_to = None
    if vert_offsets is None:
        vert_offsets = torch.tensor([0, V], dtype=torch.int64, device=q.device)
        tri_offsets = torch.tensor([0, T], dtype=torch.int64, device=q.device)
        host_to = [0, T]
    for name, t, n in (("vert_offsets", vert_offsets, V), ("tri_offsets", tri_offsets, T)):
        if not torch.is_tensor(t) or t.dtype is not torch.int64 or t.dim() != 1 or t.shape[0] < 2:
            raise err("%s: %s must be an int64 tensor [M+1]" % (what, name))
        _chk_dev(t)
    if vert_offsets.shape != tri_offsets.shape or vert_offsets.shape[0] - 1 > 65535:
        raise err("%s: vert_offsets %s and tri_offsets %s (the same length, at most 65535 meshes)"
                  % (what, tuple(vert_offsets.shape), tuple(tri_offsets.shape)))
    return q.contiguous(), tris.contiguous(), vert_offsets.contiguous(), tri_offsets.contiguous(), int(vert_offsets.shape[0]) - 1, host_to


def _check_offsets(what, vert_offsets, tri_offsets, V, T):
    """One read-back: both offset arrays start at 0, end at the array length and never decrease.  Returns tri_offsets as a list."""
    vo, to = vert_offsets.tolist(), tri_offsets.tolist()
    for name, o, n in (("vert_offsets", vo, V), ("tri_offsets", to, T)):
        if o[0] != 0 or o[-1] != n or any(b < a for a, b in zip(o, o[1:])):
            raise L.RenderNetHipError("%s: %s must rise from 0 to %d" % (what, name, n))
    for m in range(len(vo) - 1):
        if to[m + 1] > to[m] and vo[m + 1] == vo[m]:
            raise L.RenderNetHipError("%s: mesh %d has triangles and no vertices" % (what, m))
    return to


def mesh_vertex_normals(q, tris, S, vert_offsets=None, tri_offsets=None):
    """The smooth-shading input of `rasterize_mesh`: int64 [V,3], per lattice vertex the exact sum of the integer face normals
    (p1 - p0) x (p2 - p1) of the triangles of its mesh that use it, in array-axis order (rn_mesh_vertex_normals).  q int32
    [V,3], tris int32 [T,3] with indices local to their mesh, and for a concatenated set the int64 [M+1] offsets of
    `ExtractedMesh`.  Coordinates are clamped to [0, 256 S] and indices into their mesh as the rasteriser clamps them.  Run it
    once per mesh set, not per batch.  No autograd."""
    q, tris, vo, to, M, host_to = _mesh_set_args("mesh_vertex_normals", q, tris, S, vert_offsets, tri_offsets)
    V, T = int(q.shape[0]), int(tris.shape[0])
    if host_to is None:
        _check_offsets("mesh_vertex_normals", vo, to, V, T)
    out = torch.empty((V, 3), dtype=torch.int64, device=q.device)
    with torch.cuda.device(q.device):
        L.check(L.lib().rn_mesh_vertex_normals(_vp(q) if V else None, V, _vp(tris) if T else None, T, _vp(vo), _vp(to), M, int(S),
                                               _vp(out) if V else None, L.stream_ptr()), "rn_mesh_vertex_normals")
    return out


def _raster_camera_args(what, pose_or_m_inv, S, new_size, pixels_per_cell, affine):
    err = L.RenderNetHipError
    N, f = int(new_size), int(pixels_per_cell)
    if not (1 <= N <= 256 and 1 <= f <= 16 and f * N <= RASTER_MAX_SIDE):
        raise err("%s: new_size=%d, pixels_per_cell=%d (new_size <= 256, pixels_per_cell <= 16, their product <= %d)"
                  % (what, N, f, RASTER_MAX_SIDE))
    if not torch.is_tensor(pose_or_m_inv):
        raise err("%s: expected a float tensor for the pose, got %s" % (what, type(pose_or_m_inv).__name__))
    _chk_dev(pose_or_m_inv)
    m = pose_or_m_inv.detach().contiguous().float()
    B = int(m.shape[0]) if m.dim() else -1
    if B > 65535:
        raise err("%s: B=%d (at most 65535 per call)" % (what, B))
    if not affine:
        if m.dim() != 2 or m.shape[1] != 3:
            raise err("%s: expected poses [B,3], got %s" % (what, tuple(m.shape)))
        m = pose_to_affine(m, int(S), N) if B else m.new_empty((0, 3, 4))
    if m.dim() != 3 or tuple(m.shape[1:]) != (3, 4):
        raise err("%s: expected matrices [B,3,4], got %s" % (what, tuple(m.shape)))
    return m, B, N, f


def mesh_camera(pose_or_m_inv, S, new_size=128, pixels_per_cell=4, affine=False, view_from_low_x=False):
    """The rasteriser's integer camera (rn_mesh_camera): pose [B,3] (or M_inv [B,3,4] with affine=True) -> int64 [B,3,4], rows
    256 X, 256 Y, 256 D as affine functions of a lattice vertex, 2^20 fixed point -- what `rasterize_mesh` computes first and
    projects every vertex with."""
    m, B, N, f = _raster_camera_args("mesh_camera", pose_or_m_inv, S, new_size, pixels_per_cell, affine)
    cam = torch.empty((B, 3, 4), dtype=torch.int64, device=m.device)
    if B:
        with torch.cuda.device(m.device):
            L.check(L.lib().rn_mesh_camera(L.ptr(m), _vp(cam), B, N, f, 1 if view_from_low_x else 0,
                                           L.stream_ptr()), "rn_mesh_camera")
    return cam


def rasterize_mesh(q, tris, pose_or_m_inv, S, new_size=128, pixels_per_cell=4, window=None, affine=False, smooth=True,
                   cull="back", view_from_low_x=False, vert_offsets=None, tri_offsets=None, mesh_of_item=None,
                   vertex_normals=None, return_ids=False):
    """The normal map of triangle meshes under the ray caster's camera (rn_mesh_rasterize; include/rendernet_hip.h states the
    rule): q int32 [V,3] lattice vertices (256 units per voxel of the S^3 grid the mesh was fitted to, column j = array axis j,
    as `mesh.fit` and `extract_mesh` give them), tris int32 [T,3], pose [B,3] (or M_inv [B,3,4] with affine=True) -> uint8
    [B,ph,pw,3] in `raycast_normals`' colours, black where nothing is hit, so the picture overlays the ray-cast view of the
    mesh's voxelisation pixel for pixel.  window = (row0, col0, ph, pw) in pixels of the (pixels_per_cell * new_size)^2 frame.
    Several meshes: q and tris concatenated with int64 [M+1] `vert_offsets`, `tri_offsets` (vertex indices local to their mesh,
    the layout of `ExtractedMesh`) and `mesh_of_item` int32 [B]; without them every item draws the one mesh.
    smooth=True interpolates the vertex normals (`vertex_normals` = what `mesh_vertex_normals` returned for the set, computed
    here when absent), smooth=False shades with the face normal.  cull="back" drops triangles seen from inside (outward winding
    as `extract_mesh` writes it); "none" keeps both sides and turns the normal towards the viewer.  return_ids=True also returns
    the visible triangle's index within its mesh and the depth in 1/256 camera cell, int32 [B,ph,pw], -1 for a miss.
    Visibility and depth are integer functions of the input: the same bits on every call.  dtype, shapes, offsets, the window
    and the options are checked before anything is launched.  No autograd."""
    out, tri_id, depth, _ = _rasterize_mesh("rasterize_mesh", q, tris, pose_or_m_inv, S, new_size, pixels_per_cell, window, affine,
                                            smooth, cull, view_from_low_x, vert_offsets, tri_offsets, mesh_of_item, vertex_normals,
                                            return_ids)
    return (out, tri_id, depth) if return_ids else out


def _rasterize_mesh(what, q, tris, pose_or_m_inv, S, new_size, pixels_per_cell, window, affine, smooth, cull, view_from_low_x,
                    vert_offsets, tri_offsets, mesh_of_item, vertex_normals, want_ids, before_launch=None):
    """The checks and the one rn_mesh_rasterize call of `rasterize_mesh` and `rasterize_mesh_colour`: (out, tri_id, depth, set-up),
    the set-up being what the colour resolve takes over -- the contiguous set, the float matrices, the integer camera the call
    wrote and the window.  `before_launch(V, T, B, dev)` runs after every check made here and before anything is launched."""
    err = L.RenderNetHipError
    q, tris, vo, to, M, host_to = _mesh_set_args(what, q, tris, S, vert_offsets, tri_offsets)
    if cull not in MESH_CULL:
        raise err("%s: cull=%r (back or none)" % (what, cull))
    if not isinstance(smooth, bool):
        raise err("%s: smooth=%r (True or False)" % (what, smooth))
    m, B, N, f = _raster_camera_args(what, pose_or_m_inv, S, new_size, pixels_per_cell, affine)
    if m.device != q.device:
        raise err("%s: the mesh is on %s and the poses on %s" % (what, q.device, m.device))
    if window is None:
        window = (0, 0, f * N, f * N)
    row0, col0, ph, pw = (int(v) for v in window)
    if ph < 1 or pw < 1 or row0 < 0 or col0 < 0 or row0 + ph > f * N or col0 + pw > f * N:
        raise err("%s: window %s outside the %d x %d frame" % (what, (row0, col0, ph, pw), f * N, f * N))
    V, T, dev = int(q.shape[0]), int(tris.shape[0]), q.device
    if mesh_of_item is None:
        if M != 1:
            raise err("%s: %d meshes need mesh_of_item [B]" % (what, M))
        mesh_of_item = torch.zeros((B,), dtype=torch.int32, device=dev)
    if not torch.is_tensor(mesh_of_item) or mesh_of_item.dtype is not torch.int32 or tuple(mesh_of_item.shape) != (B,):
        raise err("%s: mesh_of_item must be an int32 tensor [%d]" % (what, B))
    _chk_dev(mesh_of_item)
    mesh_of_item = mesh_of_item.contiguous()
    if host_to is None:
        host_to = _check_offsets(what, vo, to, V, T)
    if B and M > 1:
        lo, hi = (int(v) for v in torch.aminmax(mesh_of_item))
        if lo < 0 or hi >= M:
            raise err("%s: mesh_of_item names a mesh outside [0, %d)" % (what, M))
    max_tris = max(b - a for a, b in zip(host_to, host_to[1:]))
    if vertex_normals is not None:
        if (not torch.is_tensor(vertex_normals) or vertex_normals.dtype is not torch.int64
                or tuple(vertex_normals.shape) != (V, 3) or vertex_normals.device != dev):
            raise err("%s: vertex_normals must be the int64 tensor [%d,3] of mesh_vertex_normals, on %s" % (what, V, dev))
        vertex_normals = vertex_normals.contiguous()
    if before_launch is not None:
        before_launch(V, T, B, dev)
    if vertex_normals is None and smooth and B and T:
        vertex_normals = mesh_vertex_normals(q, tris, S, vo, to)
    out = torch.empty((B, ph, pw, 3), dtype=torch.uint8, device=dev)
    tri_id = torch.empty((B, ph, pw), dtype=torch.int32, device=dev) if want_ids else None
    depth = torch.empty((B, ph, pw), dtype=torch.int32, device=dev) if want_ids else None
    cam = torch.empty((B, 3, 4), dtype=torch.int64, device=dev)
    if B:
        keys = torch.empty((B, ph, pw), dtype=torch.int64, device=dev)
        use_vn = smooth and T > 0 and V > 0
        with torch.cuda.device(dev):
            L.check(L.lib().rn_mesh_rasterize(
                _vp(q) if V else None, V, _vp(tris) if T else None, T, _vp(vo), _vp(to), M, _vp(mesh_of_item), max_tris, L.ptr(m),
                _vp(vertex_normals) if use_vn else None, _vp(cam), _vp(keys), _vp(out), _vp(tri_id), _vp(depth), B, int(S), N, f,
                row0, col0, ph, pw, MESH_CULL[cull], 1 if view_from_low_x else 0, L.stream_ptr()), "rn_mesh_rasterize")
    return out, tri_id, depth, (q, tris, vo, to, M, mesh_of_item, cam, N, f, (row0, col0, ph, pw))


class ImageMetrics(object):
    """What `image_metrics` returns: [B] tensors on the device.  `sad`, `ssd` (int64) and `ssim_sum` (float64) are the kernel's
    outputs; `l1`, `mse`, `psnr` and `ssim` (float64) are derived from them on first use (include/rendernet_hip.h,
    rn_image_metrics: l1 = sad / (255 n), mse = ssd / n, psnr = 10 log10(65025 / mse), +inf where ssd = 0, ssim = ssim_sum /
    n_win)."""
    __slots__ = ("sad", "ssd", "ssim_sum", "n", "n_win")

    def __init__(self, sad, ssd, ssim_sum, n, n_win):
        self.sad, self.ssd, self.ssim_sum, self.n, self.n_win = sad, ssd, ssim_sum, int(n), int(n_win)

    @property
    def l1(self):
        return self.sad.double() / (255.0 * self.n)

    @property
    def mse(self):
        return self.ssd.double() / float(self.n)

    @property
    def psnr(self):
        return 10.0 * torch.log10(65025.0 / self.mse)             # 65025 / 0 = inf

    @property
    def ssim(self):
        return self.ssim_sum / float(self.n_win)


def image_metrics(a, b):
    """a, b [B,H,W,C] on the device, C = 1 or 3, H, W >= 11, each uint8 or float32 (mixed freely; a float image is quantised
    to bytes, rint(clip(255 x, 0, 255)), NaN -> 0) -> ImageMetrics: per image the exact sums sad = sum |a - b| and ssd =
    sum (a - b)^2 (int64) and ssim_sum (float64), the sum over the (H-10)(W-10)C valid windows of the 11 x 11 Gaussian SSIM
    on integer moments, with l1, mse, psnr and ssim derived from them (rn_image_metrics; include/rendernet_hip.h states the
    rule).  Non-contiguous input is made contiguous.  The same inputs give the same bits on every call.  No autograd."""
    for name, t in (("a", a), ("b", b)):
        if not torch.is_tensor(t):
            raise L.RenderNetHipError("image_metrics: %s: expected a uint8 or float32 tensor [B,H,W,C], got %s"
                                      % (name, type(t).__name__))
    _chk_dev(a, b)
    for name, t in (("a", a), ("b", b)):
        if t.dtype not in (torch.uint8, torch.float32) or t.dim() != 4:
            raise L.RenderNetHipError("image_metrics: %s: expected uint8 or float32 [B,H,W,C], got %s %s"
                                      % (name, t.dtype, tuple(t.shape)))
    if a.shape != b.shape or a.device != b.device:
        raise L.RenderNetHipError("image_metrics: a is %s on %s and b is %s on %s" % (tuple(a.shape), a.device, tuple(b.shape), b.device))
    B, H, W, C = (int(v) for v in a.shape)
    if C not in (1, 3) or H < 11 or W < 11 or H > 32768 or W > 32768 or B > 65535:
        raise L.RenderNetHipError("image_metrics: shape %s: expected C = 1 or 3, 11 <= H, W <= 32768 (the SSIM window is "
                                  "11 x 11) and at most 65535 images" % (tuple(a.shape),))
    dev = a.device
    sad = torch.empty((B,), dtype=torch.int64, device=dev)
    ssd = torch.empty((B,), dtype=torch.int64, device=dev)
    ssim_sum = torch.empty((B,), dtype=torch.float64, device=dev)
    out = ImageMetrics(sad, ssd, ssim_sum, H * W * C, (H - 10) * (W - 10) * C)
    if B == 0:
        return out
    a, b = a.detach().contiguous(), b.detach().contiguous()
    lib = L.lib()
    ws, nws = _workspace(lib.rn_image_metrics_workspace_bytes, dev, B, H, W, C)
    with torch.cuda.device(dev):
        L.check(lib.rn_image_metrics(_vp(a), L.RN_METRICS_F32 if a.dtype is torch.float32 else L.RN_METRICS_U8,
                                     _vp(b), L.RN_METRICS_F32 if b.dtype is torch.float32 else L.RN_METRICS_U8,
                                     B, H, W, C, _vp(sad), _vp(ssd), _vp(ssim_sum), _vp(ws), nws, L.stream_ptr()), "rn_image_metrics")
    return out


EDT_SEEDS = {"solid": L.RN_EDT_SOLID, "empty": L.RN_EDT_EMPTY, "surface": L.RN_EDT_SURFACE, "signed": L.RN_EDT_SIGNED}


def _packed_grids(what, vox, threshold, bits=None, S=None):
    """The packed occupancy the distance, labelling and topology entries read: (bits int32 [B, S^3/32], B, S), from `vox`
    through `voxel_pack` or from the caller's `bits` with `S`; S must be 32, 64 or 128 and B at most 65535."""
    err = L.RenderNetHipError
    if (vox is None) == (bits is None):
        raise err("%s: give either the voxels or bits= with S=" % what)
    if bits is not None:
        if not torch.is_tensor(bits):
            raise err("%s: expected int32 bits [B, S^3/32], got %s" % (what, type(bits).__name__))
        _chk_dev(bits)
        S = _grid_side(what, S)
        if bits.dtype is not torch.int32 or bits.dim() != 2 or int(bits.shape[1]) != S ** 3 // 32:
            raise err("%s: expected int32 bits [B,%d] for S=%d, got %s %s" % (what, S ** 3 // 32, S, bits.dtype, tuple(bits.shape)))
        bits = bits.detach().contiguous()
    else:
        if not torch.is_tensor(vox):
            raise err("%s: expected a float32 or uint8 tensor [B,S,S,S,1], got %s" % (what, type(vox).__name__))
        _chk_dev(vox)
        v, B, S = _occupancy(what, vox, GRID_SIDES)
        if B == 0:
            bits = torch.empty((0, S ** 3 // 32), dtype=torch.int32, device=vox.device)
        else:
            with torch.cuda.device(vox.device):
                bits, _ = voxel_pack(v.detach(), threshold)
    B = int(bits.shape[0])
    if B > 65535:
        raise err("%s: %d grids (at most 65535 per call)" % (what, B))
    return bits, B, S


def voxel_edt(vox=None, threshold=0.5, seeds="solid", bits=None, S=None):
    """The exact squared Euclidean distance transform of occupancy grids on the device: vox [B,S,S,S,1] (or [B,S,S,S]) float32 or
    uint8 as `voxel_pack` takes it, S = 32, 64 or 128 -> int32 [B,S,S,S], per voxel min |v - u|^2 over the seed set, in voxels:
    seeds "solid" (the occupied voxels), "empty" (the empty cells, those outside the grid included), "surface" (occupied with an
    empty 6-neighbour) or "signed" (solid minus empty: positive outside, negative inside).  An empty seed set gives 1 << 30
    everywhere.  Callers that hold the pack pass `bits=` (int32 [B, S^3/32]) and `S=` instead of `vox` (rn_voxel_edt;
    include/rendernet_hip.h states the rule).  The same input gives the same bits on every call.  No autograd."""
    if not isinstance(seeds, str) or seeds not in EDT_SEEDS:
        raise L.RenderNetHipError("voxel_edt: seeds=%r (%s)" % (seeds, ", ".join(sorted(EDT_SEEDS))))
    bits, B, S = _packed_grids("voxel_edt", vox, threshold, bits, S)
    dev = bits.device
    out = torch.empty((B, S, S, S), dtype=torch.int32, device=dev)
    if B == 0:
        return out
    lib = L.lib()
    ws, nws = _workspace(lib.rn_voxel_edt_workspace_bytes, dev, B, S, EDT_SEEDS[seeds])
    with torch.cuda.device(dev):
        L.check(lib.rn_voxel_edt(_vp(bits), B, S, EDT_SEEDS[seeds], _vp(out), _vp(ws), nws, L.stream_ptr()), "rn_voxel_edt")
    return out


class ShapeMetrics(object):
    """What `voxel_shape_metrics` returns.  `words` int64 [B,16] stays on the device: n_A, n_B, n_and, n_or, the two surface
    counts, and both ways the sums of D and of floor(256 sqrt(D)), the maxima of D and the counts with D <= floor(tau^2), D the
    squared distance from a surface voxel to the other grid's surface (include/rendernet_hip.h, rn_voxel_shape_metrics).  The
    properties are float64 [B] tensors derived on first use: `iou` = n_and / n_or and `dice` = 2 n_and / (n_A + n_B), both 1 for
    two empty grids; `chamfer` = (w8 / w4 + w9 / w5) / 2 / 256 voxels; `chamfer_sq` = (w6 / w4 + w7 / w5) / 2; `hausdorff` =
    sqrt(max(w10, w11)); `precision` = w12 / w4, `recall` = w13 / w5 and `fscore` their harmonic mean (0 when both are 0).  The
    distance values are NaN where either surface is empty."""
    __slots__ = ("words", "tau2")

    def __init__(self, words, tau2):
        self.words, self.tau2 = words, int(tau2)

    def _w(self, k):
        return self.words[:, k].double()

    def _where_surfaces(self, v):
        ok = (self.words[:, 4] > 0) & (self.words[:, 5] > 0)
        return torch.where(ok, v, torch.full_like(v, float("nan")))

    @property
    def iou(self):
        n = self._w(3)
        return torch.where(n > 0, self._w(2) / n, torch.ones_like(n))

    @property
    def dice(self):
        n = self._w(0) + self._w(1)
        return torch.where(n > 0, 2.0 * self._w(2) / n, torch.ones_like(n))

    @property
    def chamfer(self):
        return self._where_surfaces(0.5 * (self._w(8) / self._w(4) + self._w(9) / self._w(5)) / 256.0)

    @property
    def chamfer_sq(self):
        return self._where_surfaces(0.5 * (self._w(6) / self._w(4) + self._w(7) / self._w(5)))

    @property
    def hausdorff(self):
        return self._where_surfaces(torch.sqrt(torch.maximum(self._w(10), self._w(11))))

    @property
    def precision(self):
        return self._where_surfaces(self._w(12) / self._w(4))

    @property
    def recall(self):
        return self._where_surfaces(self._w(13) / self._w(5))

    @property
    def fscore(self):
        p, r = self.precision, self.recall
        return torch.where(p + r > 0, 2.0 * p * r / (p + r), torch.where(torch.isnan(p + r), p + r, torch.zeros_like(p)))

    def as_dicts(self):
        """One {name: value} dict per pair -- the sixteen words as ints and the derived values as floats -- for JSON output."""
        names = ("iou", "dice", "chamfer", "chamfer_sq", "hausdorff", "precision", "recall", "fscore")
        cols = torch.stack([getattr(self, n) for n in names], 1).cpu().tolist() if int(self.words.shape[0]) else []
        return [dict([("words", w), ("tau2", self.tau2)] + list(zip(names, c))) for w, c in zip(self.words.cpu().tolist(), cols)]


def _tau2(tau):
    """floor(tau^2), the integer the kernel compares D with; capped at 1 << 30, above every distance."""
    tau = _finite("voxel_shape_metrics", "tau", tau, "distance in voxels, >= 0")
    if tau < 0:
        raise L.RenderNetHipError("voxel_shape_metrics: tau=%r (a distance in voxels, >= 0)" % (tau,))
    return int(min(math.floor(tau * tau), 1 << 30))


def voxel_shape_metrics(a, b, threshold=0.5, tau=1.0):
    """How close grids a (prediction) and b (target) are, pair by pair, on the device: a, b [B,S,S,S,1] (or [B,S,S,S]) float32
    or uint8, the same shape, S = 32, 64 or 128 -> ShapeMetrics (int64 words [B,16] and the IoU, Dice, chamfer, Hausdorff,
    precision / recall / F-score at distance `tau` voxels derived from them).  `threshold` is a scalar or a pair (for a, for b):
    a reconstruction is thresholded at 0.1, a binvox at 0.5.  Distances run between the grids' surface voxels (occupied with an
    empty 6-neighbour), exact; the field itself is never written to memory (rn_voxel_shape_metrics; include/rendernet_hip.h
    states the rule).  The same inputs give the same bits on every call.  No autograd."""
    thr = tuple(threshold) if isinstance(threshold, (tuple, list)) else (threshold, threshold)
    if len(thr) != 2:
        raise L.RenderNetHipError("voxel_shape_metrics: threshold=%r (a number, or one for a and one for b)" % (threshold,))
    tau2 = _tau2(tau)
    for name, t in (("a", a), ("b", b)):
        if not torch.is_tensor(t):
            raise L.RenderNetHipError("voxel_shape_metrics: %s: expected a tensor [B,S,S,S,1], got %s" % (name, type(t).__name__))
    _chk_dev(a, b)
    if _grid_view(a).shape != _grid_view(b).shape or a.device != b.device:
        raise L.RenderNetHipError("voxel_shape_metrics: a is %s on %s and b is %s on %s" % (tuple(a.shape), a.device, tuple(b.shape), b.device))
    bits_a, B, S = _packed_grids("voxel_shape_metrics", a, thr[0])
    bits_b, _, _ = _packed_grids("voxel_shape_metrics", b, thr[1])
    dev = bits_a.device
    words = torch.empty((B, L.RN_SHAPE_WORDS), dtype=torch.int64, device=dev)
    out = ShapeMetrics(words, tau2)
    if B == 0:
        return out
    lib = L.lib()
    ws, nws = _workspace(lib.rn_voxel_shape_metrics_workspace_bytes, dev, B, S)
    with torch.cuda.device(dev):
        L.check(lib.rn_voxel_shape_metrics(_vp(bits_a), _vp(bits_b), B, S, tau2, _vp(words), _vp(ws), nws, L.stream_ptr()),
                "rn_voxel_shape_metrics")
    return out


def voxel_offset(vox, radius, threshold=0.5):
    """Thickens or thins occupancy grids by a Euclidean ball: vox as `voxel_edt` takes it -> uint8 [B,S,S,S,1], 0 or 1.
    radius > 0 dilates (D_solid <= floor(r^2)), radius < 0 erodes (D_empty > floor(r^2)), radius = 0 returns the thresholded
    grid.  A comparison on the `voxel_edt` output.  No autograd."""
    radius = _finite("voxel_offset", "radius", radius, "number of voxels")
    r2 = int(min(math.floor(radius * radius), 1 << 29))
    if radius > 0:
        out = voxel_edt(vox, threshold, "solid") <= r2
    elif radius < 0:
        out = voxel_edt(vox, threshold, "empty") > r2
    else:
        out = voxel_edt(vox, threshold, "solid") == 0
    return out.to(torch.uint8).unsqueeze(-1)


def _orientations():
    """The 48 signed axis permutations in the header's numbering: rows (pi0, pi1, pi2, f0, f1, f2); the rotations come first."""
    rows = [p + f for p in ((0, 1, 2), (0, 2, 1), (1, 0, 2), (1, 2, 0), (2, 0, 1), (2, 1, 0))
            for f in ((a, b, c) for a in (0, 1) for b in (0, 1) for c in (0, 1))]
    odd = lambda r: (sum(1 for i in range(3) for j in range(i + 1, 3) if r[i] > r[j]) + sum(r[3:])) & 1
    return tuple([r for r in rows if not odd(r)] + [r for r in rows if odd(r)])


ORIENTATIONS = _orientations()
ALIGN_SETS = {"none": L.RN_ALIGN_NONE, "rotations": L.RN_ALIGN_ROTATIONS, "all": L.RN_ALIGN_ALL}
ALIGN_SET_SIZES = {"none": 1, "rotations": 24, "all": 48}
ALIGN_MAX_SHIFT = L.RN_ALIGN_MAX_SHIFT


def _per_item(what, name, v, B, width, lo, hi):
    """v as B rows of `width` ints in [lo, hi]: one row for every item, or a row for each."""
    if torch.is_tensor(v):
        v = v.detach().cpu().tolist()
    shape = () if width == 1 else (width,)
    a = np.asarray(v)
    if a.size == 0 and B == 0:
        a = np.zeros((0,) + shape, np.int64)                      # the rows of no items
    if a.dtype.kind not in "iu" or a.dtype == np.bool_:
        raise L.RenderNetHipError("%s: %s=%r (integers)" % (what, name, v))
    if a.shape == shape:
        a = np.broadcast_to(a, (B,) + shape)
    if a.shape != (B,) + shape:
        raise L.RenderNetHipError("%s: %s of shape %s for %d grids (%s or %s)" % (what, name, a.shape, B, shape, (B,) + shape))
    if a.size and (a.min() < lo or a.max() > hi):
        raise L.RenderNetHipError("%s: %s=%r (%d..%d)" % (what, name, v, lo, hi))
    return a.reshape(B, width).tolist()


def voxel_transform(vox, orientation, shift):
    """Moves grids by a signed axis permutation about the centre and an integer shift, the candidate (o, t) of `voxel_align`:
    vox [B,S,S,S] or [B,S,S,S,1], any dtype, on any device -> the same shape, out(p) = orient_o(vox)(p - t) with zeros where
    nothing lands and what leaves the grid dropped.  `orientation` is an int in 0..47 (a row of ORIENTATIONS) or one per item,
    `shift` is (tz, ty, tx) or one per item.  Torch indexing, not a kernel.  No autograd."""
    what = "voxel_transform"
    if not torch.is_tensor(vox):
        raise L.RenderNetHipError("%s: expected a tensor [B,S,S,S,1], got %s" % (what, type(vox).__name__))
    v, B, S = _occupancy(what, vox)
    os_ = _per_item(what, "orientation", orientation, B, 1, 0, len(ORIENTATIONS) - 1)
    ts = _per_item(what, "shift", shift, B, 3, -S, S)
    out = torch.zeros_like(v.detach())
    for b in range(B):
        row = ORIENTATIONS[os_[b][0]]
        g = v[b].detach().permute(*row[:3])
        flips = [k for k in range(3) if row[3 + k]]
        if flips:
            g = g.flip(flips)
        dst = tuple(slice(max(t, 0), S + min(t, 0)) for t in ts[b])
        src = tuple(slice(max(-t, 0), S - max(t, 0)) for t in ts[b])
        out[b][dst] = g[src]
    return out.reshape(vox.shape)


class VoxelAlignment(object):
    """What `voxel_align` returns.  `words` int32 [B,8] stays on the device: o, tz, ty, tx and n_and of the winner, n_A, n_B, and
    n_and of the identity candidate (include/rendernet_hip.h, rn_voxel_align).  `orientation` int32 [B], `shift` int32 [B,3] and
    `n_and` int32 [B] are views of it; `iou_before` and `iou_after` are float64 [B], n_and / (n_A + n_B - n_and) of the identity
    candidate and of the winner, 1 for two empty grids.  `scores` is the whole table int32 [B, n_orient, 2R+1, 2R+1, 2R+1] when it
    was asked for, otherwise None.  `apply(vox)` moves grids by the winner."""
    __slots__ = ("words", "scores", "max_shift", "orientations")

    def __init__(self, words, scores, max_shift, orientations):
        self.words, self.scores, self.max_shift, self.orientations = words, scores, int(max_shift), orientations

    orientation = property(lambda self: self.words[:, 0])
    shift = property(lambda self: self.words[:, 1:4])
    n_and = property(lambda self: self.words[:, 4])

    def _iou(self, k):
        n = self.words[:, k].double()
        n_or = self.words[:, 5].double() + self.words[:, 6].double() - n
        return torch.where(n_or > 0, n / n_or, torch.ones_like(n))

    iou_before = property(lambda self: self._iou(7))
    iou_after = property(lambda self: self._iou(4))

    def apply(self, vox):
        """`voxel_transform` of vox (float32 or uint8, [B,S,S,S] or [B,S,S,S,1]) by each item's winner."""
        return voxel_transform(vox, self.words[:, 0], self.words[:, 1:4])

    def as_dicts(self):
        """One dict per pair for JSON output."""
        cols = zip(self.words.cpu().tolist(), self.iou_before.cpu().tolist(), self.iou_after.cpu().tolist())
        return [{"orientation": w[0], "shift": w[1:4], "n_and": w[4], "n_a": w[5], "n_b": w[6], "n_and_before": w[7],
                 "iou_before": before, "iou_after": after} for w, before, after in cols]


def _align_args(what, max_shift, orientations, threshold):
    """(R, the name of the orientation set, the thresholds of a and b), checked with no device."""
    if isinstance(max_shift, (bool, float)) or not isinstance(max_shift, (int, np.integer)) or not 0 <= int(max_shift) <= ALIGN_MAX_SHIFT:
        raise L.RenderNetHipError("%s: max_shift=%r (an integer, 0..%d)" % (what, max_shift, ALIGN_MAX_SHIFT))
    if not isinstance(orientations, str) or orientations not in ALIGN_SETS:
        raise L.RenderNetHipError("%s: orientations=%r (%s)" % (what, orientations, ", ".join(ALIGN_SETS)))
    thr = tuple(threshold) if isinstance(threshold, (tuple, list)) else (threshold, threshold)
    if len(thr) != 2:
        raise L.RenderNetHipError("%s: threshold=%r (a number, or one for a and one for b)" % (what, threshold))
    return int(max_shift), orientations, tuple(_finite(what, "threshold", t, "number") for t in thr)


def voxel_orient(vox=None, threshold=0.5, first=0, count=48, bits=None, S=None):
    """The packed oriented copies of grids, on the device: vox as `voxel_pack` takes it (or bits= with S=) -> int32
    [B, count, S^3/32], orient_o of every grid for o = first .. first + count - 1 (rn_voxel_orient).  No autograd."""
    what = "voxel_orient"
    for name, v in (("first", first), ("count", count)):
        if isinstance(v, (bool, float)) or not isinstance(v, (int, np.integer)):
            raise L.RenderNetHipError("%s: %s=%r (an integer)" % (what, name, v))
    if first < 0 or count < 0 or first + count > len(ORIENTATIONS):
        raise L.RenderNetHipError("%s: orientations %d .. %d + %d (inside 0..47)" % (what, first, first, count))
    bits, B, S = _packed_grids(what, vox, threshold, bits, S)
    out = torch.empty((B, int(count), S ** 3 // 32), dtype=torch.int32, device=bits.device)
    if B and count:
        with torch.cuda.device(bits.device):
            L.check(L.lib().rn_voxel_orient(_vp(bits), B, S, int(first), int(count), _vp(out), L.stream_ptr()), "rn_voxel_orient")
    return out


def voxel_align(a, b, max_shift=8, orientations="rotations", threshold=0.5, return_scores=False):
    """The signed axis permutation o and integer shift t that put grid a (moving) on grid b (fixed), pair by pair, on the device:
    a, b [B,S,S,S,1] (or [B,S,S,S]) float32 or uint8, the same shape, S = 32, 64 or 128 -> VoxelAlignment.  Every candidate is
    scored: o out of `orientations` ("none" = the identity, "rotations" = the 24 proper ones, "all" = with the 24 mirrored), each
    of tz, ty, tx in [-max_shift, max_shift], max_shift at most 16, by n_and = |a' & b| with a'(p) = orient_o(a)(p - t), nothing
    wrapping.  The largest n_and -- which is the largest IoU -- wins; ties go to the smallest |t|^2, then the smallest o, then
    the smallest (tz, ty, tx), so aligned grids return (0, (0,0,0)).  `threshold` is a scalar or a pair (for a, for b).
    (rn_voxel_align; include/rendernet_hip.h states the rule.)  The same inputs give the same bits on every call.  No autograd."""
    what = "voxel_align"
    R, orientations, thr = _align_args(what, max_shift, orientations, threshold)
    for name, t in (("a", a), ("b", b)):
        if not torch.is_tensor(t):
            raise L.RenderNetHipError("%s: %s: expected a tensor [B,S,S,S,1], got %s" % (what, name, type(t).__name__))
    _chk_dev(a, b)
    if _grid_view(a).shape != _grid_view(b).shape or a.device != b.device:
        raise L.RenderNetHipError("%s: a is %s on %s and b is %s on %s" % (what, tuple(a.shape), a.device, tuple(b.shape), b.device))
    bits_a, B, S = _packed_grids(what, a, thr[0])
    bits_b, _, _ = _packed_grids(what, b, thr[1])
    dev, n_orient, T = bits_a.device, ALIGN_SET_SIZES[orientations], 2 * R + 1
    words = torch.empty((B, L.RN_ALIGN_WORDS), dtype=torch.int32, device=dev)
    scores = torch.empty((B, n_orient, T, T, T), dtype=torch.int32, device=dev) if return_scores else None
    out = VoxelAlignment(words, scores, R, orientations)
    if B == 0:
        return out
    lib = L.lib()
    ws, nws = _workspace(lib.rn_voxel_align_workspace_bytes, dev, B, S, R, n_orient)
    with torch.cuda.device(dev):
        L.check(lib.rn_voxel_align(_vp(bits_a), _vp(bits_b), B, S, R, ALIGN_SETS[orientations], _vp(words), _vp(scores), _vp(ws), nws,
                                   L.stream_ptr()), "rn_voxel_align")
    return out


LABEL_OF ={"solid": L.RN_LABEL_SOLID, "empty": L.RN_LABEL_EMPTY}
VoxelComponents = collections.namedtuple("VoxelComponents", "labels counts offsets stats")


def _label_args(what, of, connectivity):
    if not isinstance(of, str) or of not in LABEL_OF:
        raise L.RenderNetHipError("%s: of=%r (solid or empty)" % (what, of))
    if isinstance(connectivity, (bool, float)) or connectivity not in (6, 26):
        raise L.RenderNetHipError("%s: connectivity=%r (6 or 26)" % (what, connectivity))
    return LABEL_OF[of], int(connectivity)


def voxel_components(vox=None, threshold=0.5, of="solid", connectivity=26, bits=None, S=None):
    """The connected components of occupancy grids on the device, exactly: vox [B,S,S,S,1] (or [B,S,S,S]) float32 or uint8 as
    `voxel_pack` takes it, S = 32, 64 or 128 (or `bits=` int32 [B, S^3/32] with `S=`) -> VoxelComponents(labels, counts, offsets,
    stats), all on the device.  of "solid" labels the occupied voxels 1..K per item, by ascending minimum flat index (the numbering
    of scipy.ndimage.label); of "empty" labels the empty space: 1 is the component joined with the outside of the grid (every
    empty voxel connected to the border), 2..K+1 the closed cavities.  labels int32 [B,S,S,S] is 0 on the other voxels; counts int32
    [B] = K; stats int32 [total, 8] has one row per component -- size, minimum flat index, inclusive box (x_lo, y_lo, z_lo, x_hi,
    y_hi, z_hi) -- the items concatenated by offsets int64 [B+1] (for the empty space row 0 of an item is the outside component,
    restricted to the grid).  connectivity is 6 (faces) or 26 (faces, edges, corners); a solid at 26 goes with its empty space at
    6 and conversely.  The counts are read back ONCE between the labelling and the statistics to size the rows, as `extract_mesh`
    does (rn_voxel_label / rn_voxel_label_stats; include/rendernet_hip.h states the rule).  The same input gives the same bits on
    every call.  No autograd."""
    of_empty, connectivity = _label_args("voxel_components", of, connectivity)
    bits, B, S = _packed_grids("voxel_components", vox, threshold, bits, S)
    dev = bits.device
    labels = torch.empty((B, S, S, S), dtype=torch.int32, device=dev)
    counts = torch.empty((B,), dtype=torch.int32, device=dev)
    offsets = torch.zeros((B + 1,), dtype=torch.int64, device=dev)
    if B == 0:
        return VoxelComponents(labels, counts, offsets, torch.empty((0, 8), dtype=torch.int32, device=dev))
    lib = L.lib()
    ws, nws = _workspace(lib.rn_voxel_label_workspace_bytes, dev, B, S)
    with torch.cuda.device(dev):
        L.check(lib.rn_voxel_label(_vp(bits), B, S, of_empty, connectivity, _vp(labels), _vp(counts), _vp(ws), nws, L.stream_ptr()),
                "rn_voxel_label")
        rows = counts.cpu().to(torch.int64) + of_empty            # the one host read
        offsets[1:] = torch.cumsum(rows, 0).to(dev)
        total = int(rows.sum())
        stats = torch.empty((total, 8), dtype=torch.int32, device=dev)
        if total:
            L.check(lib.rn_voxel_label_stats(_vp(labels), _vp(offsets), B, S, of_empty, _vp(stats), L.stream_ptr()),
                    "rn_voxel_label_stats")
    return VoxelComponents(labels, counts, offsets, stats)


def _clean_args(what, keep_largest, min_voxels, connectivity):
    for name, v, low in (("keep_largest", keep_largest, 0), ("min_voxels", min_voxels, 1)):
        if v is None and name == "keep_largest":
            continue
        if isinstance(v, (bool, float)) or not isinstance(v, (int, np.integer)) or v < low:
            raise L.RenderNetHipError("%s: %s=%r (an integer >= %d)" % (what, name, v, low))
    return int(keep_largest or 0), int(min_voxels), _label_args(what, "solid", connectivity)[1]


def _clean(vox, threshold, keep_largest, min_voxels, fill_cavities, connectivity):
    """voxel_clean, and per item the sizes of the dropped components in label order."""
    keep_largest, min_voxels, connectivity = _clean_args("voxel_clean", keep_largest, min_voxels, connectivity)
    comps = voxel_components(vox, threshold, "solid", connectivity)
    labels, B = comps.labels, int(comps.labels.shape[0])
    total = int(comps.stats.shape[0])
    dev = labels.device
    if total == 0:
        return torch.zeros(tuple(labels.shape) + (1,), dtype=torch.uint8, device=dev), [[] for _ in range(B)]
    size = comps.stats[:, 0].to(torch.int64)
    item = torch.repeat_interleave(torch.arange(B, device=dev), comps.counts.to(torch.int64))
    order = torch.argsort(-size, stable=True)                     # rows stand in (item, label) order: on equal size the lower label wins
    order = order[torch.argsort(item[order], stable=True)]
    rank = torch.empty_like(order)
    rank[order] = torch.arange(total, device=dev) - comps.offsets[item[order]]
    keep = size >= min_voxels
    if keep_largest:
        keep &= rank < keep_largest
    row = (comps.offsets[:-1].view(B, 1, 1, 1) + labels - 1).clamp_(0, total - 1)
    kept = (labels > 0) & keep[row]
    out = kept.to(torch.uint8)
    if fill_cavities:
        out |= (voxel_components(out, 0.5, "empty", 26 if connectivity == 6 else 6).labels >= 2).to(torch.uint8)
    dropped_size, dropped_item = size[~keep].cpu().tolist(), item[~keep].cpu().tolist()
    dropped = [[] for _ in range(B)]
    for b, n in zip(dropped_item, dropped_size):
        dropped[b].append(n)
    return out.unsqueeze(-1), dropped


def voxel_clean(vox, threshold=0.5, keep_largest=1, min_voxels=1, fill_cavities=True, connectivity=26):
    """Removes the floaters and closes the bubbles of occupancy grids on the device: vox as `voxel_components` takes it -> uint8
    [B,S,S,S,1], 0 or 1.  First the components of at least `min_voxels` voxels are kept, and of those the `keep_largest` biggest
    (None or 0 keeps all; on equal size the lower label wins); then, on the grid kept so far, every cavity of the dual
    connectivity (6 for 26 and conversely) is filled.  The labelling is `voxel_components`; choosing the rows of its statistics
    and indexing the keep table with the labels is tensor arithmetic on the device.  No autograd."""
    return _clean(vox, threshold, keep_largest, min_voxels, fill_cavities, connectivity)[0]


class VoxelTopology(object):
    """What `voxel_topology` returns.  `words` int64 [B,8] stays on the device: the occupied voxels n, the components (26-connected),
    the cavities (6-connected empty space that does not reach the outside of the grid), the vertices V, edges E and faces F of the
    union of the closed unit cubes, the Euler number V - E + F - n, and the handles = components + cavities - Euler number
    (include/rendernet_hip.h, rn_voxel_topology).  `components`, `cavities`, `euler` and `handles` are its int64 [B] columns."""
    __slots__ = ("words",)
    NAMES = ("voxels", "components", "cavities", "vertices", "edges", "faces", "euler", "handles")

    def __init__(self, words):
        self.words = words

    components = property(lambda self: self.words[:, 1])
    cavities = property(lambda self: self.words[:, 2])
    euler = property(lambda self: self.words[:, 6])
    handles = property(lambda self: self.words[:, 7])

    def as_dicts(self):
        """One {name: int} dict per grid, with the eight words under "words", for JSON output."""
        return [dict([("words", w)] + list(zip(self.NAMES, w))) for w in self.words.cpu().tolist()]


def voxel_topology(vox=None, threshold=0.5, bits=None, S=None):
    """The topology of occupancy grids on the device, exactly: vox as `voxel_components` takes it (or `bits=` with `S=`) ->
    VoxelTopology (int64 words [B,8]: voxels, components, cavities, V, E, F, Euler number, handles).  A chair whose leg gap has
    been filled in keeps its IoU and loses a handle.  Two labellings -- the solid at 26, the empty space at 6 -- and one count of
    the cells of the cubical complex (rn_voxel_topology).  The same input gives the same bits on every call.  No autograd."""
    bits, B, S = _packed_grids("voxel_topology", vox, threshold, bits, S)
    dev = bits.device
    words = torch.empty((B, L.RN_TOPOLOGY_WORDS), dtype=torch.int64, device=dev)
    if B == 0:
        return VoxelTopology(words)
    lib = L.lib()
    ws, nws = _workspace(lib.rn_voxel_topology_workspace_bytes, dev, B, S)
    with torch.cuda.device(dev):
        L.check(lib.rn_voxel_topology(_vp(bits), B, S, _vp(words), _vp(ws), nws, L.stream_ptr()), "rn_voxel_topology")
    return VoxelTopology(words)


def _pose_matrices(what, pose_or_m_inv, B, S, N, affine):
    """M_inv float32 [B,3,4] for the casters: `pose_or_m_inv` itself with affine=True, else `pose_to_affine` of poses [B,3] for
    grids of side S in a frame of N cells.  B = None takes the batch from the tensor."""
    with torch.no_grad():
        m = pose_or_m_inv.detach().contiguous().float()
        B = int(m.shape[0]) if B is None else B
        if not affine:
            m = pose_to_affine(m, int(S), int(N)) if B else m.new_empty((0, 3, 4))
    if tuple(m.shape) != (B, 3, 4):
        raise L.RenderNetHipError("%s: expected %s matrices [B,3,4], got %s" % (what, B, tuple(m.shape)))
    return m


def _check_ranges(what, ranges, opts, also=None):
    """Integer options against a table name -> (lowest, highest, default), before anything is launched: returns them as
    ints.  `also` maps a name to the one value it takes besides its range."""
    out = {}
    for k, v in opts.items():
        lo, hi, _ = ranges[k]
        extra = (also or {}).get(k)
        if isinstance(v, (bool, float)) or not isinstance(v, (int, np.integer)):
            raise L.RenderNetHipError("%s: %s=%r is not an integer" % (what, k, v))
        if not (lo <= int(v) <= hi or int(v) == extra):
            raise L.RenderNetHipError("%s: %s=%d (%s%d..%d)" % (what, k, int(v), "" if extra is None else "%d, or " % extra, lo, hi))
        out[k] = int(v)
    return out


def _check_hits(what, bits, box, hit, face, S):
    """The inputs of a second stage on given hits: bits, box as `voxel_pack` returns them for grids of side S, hit int32 and
    face int8 [B,ph,pw] -> (bits, box, hit, face, B, ph, pw), the tensors contiguous."""
    if hit.dim() != 3 or hit.shape != face.shape or hit.dtype is not torch.int32 or face.dtype is not torch.int8:
        raise L.RenderNetHipError("%s: expected hit int32 and face int8 [B,ph,pw], got %s %s and %s %s"
                                  % (what, hit.dtype, tuple(hit.shape), face.dtype, tuple(face.shape)))
    B, ph, pw = (int(v) for v in hit.shape)
    S = int(S)
    if bits.dtype is not torch.int32 or box.dtype is not torch.int32 or tuple(box.shape) != (B, 6) or \
            tuple(bits.shape) != (B, max(S ** 3 // 32, 1)):
        raise L.RenderNetHipError("%s: expected int32 bits [%d,%d] and box [%d,6], got %s and %s"
                                  % (what, B, S ** 3 // 32, B, tuple(bits.shape), tuple(box.shape)))
    return bits.contiguous(), box.contiguous(), hit.contiguous(), face.contiguous(), B, ph, pw


def _raycast(what, vox, pose_or_m_inv, new_size, pixels_per_cell, window, affine, threshold, normal_radius, view_from_low_x,
             want_hits):
    """pack + rn_raycast_fwd for `raycast_normals` and `raycast_ao`: (bits, box, S, rgb, hit | None, face | None)."""
    _chk_dev(vox, pose_or_m_inv)
    N, f = int(new_size), int(pixels_per_cell)
    if window is None:
        window = (0, 0, f * N, f * N)
    row0, col0, ph, pw = (int(v) for v in window)
    with torch.no_grad():
        bits, box = voxel_pack(vox, threshold)
        B, S = int(vox.shape[0]), int(vox.shape[1])
        m = _pose_matrices(what, pose_or_m_inv, B, S, N, affine)
        out = torch.empty((B, max(ph, 0), max(pw, 0), 3), dtype=torch.uint8, device=vox.device)
        hit = torch.empty((B, max(ph, 0), max(pw, 0)), dtype=torch.int32, device=vox.device) if want_hits else None
        face = torch.empty((B, max(ph, 0), max(pw, 0)), dtype=torch.int8, device=vox.device) if want_hits else None
        L.check(L.lib().rn_raycast_fwd(_vp(bits), _vp(box), L.ptr(m), _vp(out), _vp(hit), _vp(face), B, S, N, f, row0, col0, ph, pw, int(normal_radius), 1 if view_from_low_x else 0,
                                       L.stream_ptr()), "rn_raycast_fwd")
    return bits, box, S, out, hit, face


def raycast_normals(vox, pose_or_m_inv, new_size=128, pixels_per_cell=4, window=None, affine=False, threshold=0.5,
                    normal_radius=2, view_from_low_x=False, return_hits=False):
    """The ground-truth normal map of an occupancy grid at a pose (rn_voxel_pack + rn_raycast_fwd): vox [B,S,S,S,1] float32
    or uint8, pose [B,3] (azimuth, elevation, scale; or M_inv [B,3,4] with affine=True -- the resampler's matrix) ->
    uint8 [B,ph,pw,3], colours R = right, G = up, B = towards the camera, black where the ray misses.  window = (row0, col0,
    ph, pw) in image pixels of the (pixels_per_cell * new_size)^2 frame, default the whole frame.  One orthographic ray per
    pixel, first voxel with value > threshold, normal from the occupancy within `normal_radius` voxels
    (include/rendernet_hip.h states geometry and rules).  return_hits=True also returns the flat index of the hit voxel
    (int32 [B,ph,pw], -1 = miss) and the face the ray entered it by (int8, 0..5).
    NOT differentiable: the outputs are bytes and indices; they carry no gradient to the grid or the pose."""
    _, _, _, out, hit, face = _raycast("raycast_normals", vox, pose_or_m_inv, new_size, pixels_per_cell, window, affine,
                                       threshold, normal_radius, view_from_low_x, return_hits)
    return (out, hit, face) if return_hits else out


def raycast_ao_from_hits(bits, box, hit, face, S, max_distance=16, smooth=0, return_counts=False):
    """The second stage of `raycast_ao` on given hits (rn_raycast_ao_fwd + rn_ao_encode): bits, box as `voxel_pack` returns
    them for grids of side S, hit int32 [B,ph,pw] (flat index of the hit voxel, < 0 = miss) and face int8 [B,ph,pw] (0..5) as
    rn_raycast_fwd writes them -> uint8 [B,ph,pw]; return_counts=True also returns the open-ray counts (uint8, 0..64, 255 =
    miss).  `smooth` is the radius of the masked mean in pixels, 0..8.  No autograd."""
    _chk_dev(bits, box, hit, face)
    bits, box, hit, face, B, ph, pw = _check_hits("raycast_ao_from_hits", bits, box, hit, face, S)
    with torch.no_grad():
        count = torch.empty((B, ph, pw), dtype=torch.uint8, device=hit.device)
        out = torch.empty_like(count)
        L.check(L.lib().rn_raycast_ao_fwd(_vp(bits), _vp(box), _vp(hit), _vp(face), _vp(count), B, int(S), ph, pw, int(max_distance),
                                          L.stream_ptr()), "rn_raycast_ao_fwd")
        L.check(L.lib().rn_ao_encode(_vp(count), _vp(out), B, ph, pw, int(smooth), L.stream_ptr()), "rn_ao_encode")
    return (out, count) if return_counts else out


def raycast_ao(vox, pose_or_m_inv, new_size=128, pixels_per_cell=4, window=None, affine=False, threshold=0.5,
               max_distance=16, smooth=None, view_from_low_x=False, return_counts=False):
    """The ground-truth ambient occlusion of an occupancy grid at a pose (rn_voxel_pack + rn_raycast_fwd with hits +
    rn_raycast_ao_fwd + rn_ao_encode): arguments as `raycast_normals` -> uint8 [B,ph,pw], 255 = fully open, 0 where the ray
    misses.  Per hit pixel, 64 cosine-weighted rays leave the centre of the voxel face the camera ray entered by; the byte is
    the share that meets no occupied voxel within `max_distance` voxels (Chebyshev, 1..32), averaged over the hit pixels
    within `smooth` pixels (0..8; None = pixels_per_cell, the footprint of one voxel face; the window of the mean is clipped
    to the cast window, so a cropped cast differs from the crop of a whole frame within `smooth` pixels of its border).
    include/rendernet_hip.h states the rule; it is integer given the hits.  return_counts=True also returns the open-ray
    counts (uint8 [B,ph,pw], 0..64, 255 = miss).
    NOT differentiable: the outputs are bytes; they carry no gradient to the grid or the pose."""
    smooth = int(pixels_per_cell) if smooth is None else int(smooth)
    if not 1 <= int(max_distance) <= 32 or not 0 <= smooth <= 8:        # before the first stage is launched
        raise L.RenderNetHipError("raycast_ao: max_distance=%d (1..32), smooth=%d (0..8)" % (int(max_distance), smooth))
    bits, box, S, _, hit, face = _raycast("raycast_ao", vox, pose_or_m_inv, new_size, pixels_per_cell, window, affine,
                                          threshold, 1, view_from_low_x, True)
    return raycast_ao_from_hits(bits, box, hit, face, S, max_distance, smooth, return_counts)


# the parameters of the two line pictures: name -> (lowest, highest, default); `levels` also takes 0 (no bands: the outline),
# which _LINE_ALSO says
LINE_RANGES = {"normal_radius": (1, 3, 2), "line_radius": (1, 4, 2), "depth_gap": (1, 127, 2), "crease_q": (0, 8, 4),
               "edge_mask": (1, 7, 7), "levels": (2, 8, 4), "shadow_byte": (0, 254, 64)}
_LINE_ALSO = {"levels": 0}


def check_line_options(what, **opts):
    """The integer parameters of rn_raycast_edges_fwd / rn_lines_encode against LINE_RANGES, before anything is launched:
    returns them as ints."""
    return _check_ranges(what, LINE_RANGES, opts, _LINE_ALSO)


def quantise_light(l):
    """A light direction in the normal map's channel order (right, up, towards the camera) -> the three ints rn_lines_encode
    takes: rint(32767 l / |l|).  `tools.Phong_shading.generate_light_pos` returns directions in this order."""
    v = np.asarray(l, np.float64).reshape(-1)
    if v.shape != (3,) or not np.isfinite(v).all() or not np.sqrt(np.sum(v * v)) > 0.0:
        raise L.RenderNetHipError("quantise_light: expected three finite components, not all zero, got %r" % (l,))
    return tuple(int(c) for c in np.rint(32767.0 * v / np.sqrt(np.sum(v * v))))


def raycast_edges_from_hits(bits, box, hit, face, S, normal_radius=2, line_radius=2, depth_gap=2, crease_q=4):
    """The edge bits of given hits (rn_raycast_edges_fwd): bits, box as `voxel_pack` returns them for grids of side S, hit
    int32 [B,ph,pw] and face int8 [B,ph,pw] as rn_raycast_fwd writes them -> uint8 [B,ph,pw], the OR of 1 (silhouette: a miss
    within `line_radius` pixels), 2 (depth: a hit voxel more than `depth_gap` voxels away) and 4 (crease: a stencil normal of
    radius `normal_radius` at more than the angle of `crease_q`), 0 for a miss.  The window is clipped to [ph,pw].  No autograd."""
    _chk_dev(bits, box, hit, face)
    o = check_line_options("raycast_edges_from_hits", normal_radius=normal_radius, line_radius=line_radius,
                           depth_gap=depth_gap, crease_q=crease_q)
    bits, box, hit, face, B, ph, pw = _check_hits("raycast_edges_from_hits", bits, box, hit, face, S)
    with torch.no_grad():
        edge = torch.empty((B, ph, pw), dtype=torch.uint8, device=hit.device)
        L.check(L.lib().rn_raycast_edges_fwd(_vp(bits), _vp(box), _vp(hit), _vp(face), _vp(edge), B, int(S), ph, pw, o["normal_radius"],
                                             o["line_radius"], o["depth_gap"], o["crease_q"], L.stream_ptr()), "rn_raycast_edges_fwd")
    return edge


def _raycast_lines(what, vox, pose_or_m_inv, new_size, pixels_per_cell, window, affine, threshold, view_from_low_x, light,
                   return_edges, **opts):
    """cast + edges + encode for `raycast_outline` (levels 0) and `raycast_cel`; every parameter is checked first."""
    o = check_line_options(what, **opts)
    lq = (0, 0, 0)
    if o["levels"]:
        lq = quantise_light(_demo_light() if light is None else light)
    bits, box, S, normals, hit, face = _raycast(what, vox, pose_or_m_inv, new_size, pixels_per_cell, window, affine, threshold,
                                                o["normal_radius"], view_from_low_x, True)
    edge = raycast_edges_from_hits(bits, box, hit, face, S, o["normal_radius"], o["line_radius"], o["depth_gap"], o["crease_q"])
    with torch.no_grad():
        out = torch.empty_like(edge)
        B, ph, pw = (int(v) for v in edge.shape)
        L.check(L.lib().rn_lines_encode(_vp(normals), _vp(edge), _vp(out), B, ph, pw, o["edge_mask"],
                                        o["levels"], o["shadow_byte"], lq[0], lq[1], lq[2], L.stream_ptr()), "rn_lines_encode")
    return (out, edge) if return_edges else out


def raycast_outline(vox, pose_or_m_inv, new_size=128, pixels_per_cell=4, window=None, affine=False, threshold=0.5,
                    normal_radius=2, line_radius=2, depth_gap=2, crease_q=4, edge_mask=7, view_from_low_x=False,
                    return_edges=False):
    """The ground-truth contour drawing of an occupancy grid at a pose (rn_voxel_pack + rn_raycast_fwd with hits +
    rn_raycast_edges_fwd + rn_lines_encode): arguments as `raycast_normals` -> uint8 [B,ph,pw], black lines (0) on white (255),
    the background white.  A hit pixel is inked when, within `line_radius` pixels (1..4, clipped to the cast window), a ray
    misses (silhouette), hits a voxel more than `depth_gap` voxels away (1..127, Chebyshev) or hits a surface whose normal
    makes more than the angle cos^2 = crease_q / 8 with its own (0..8; 4 = 45 degrees); `edge_mask` (1..7) selects which of
    the three draw.  include/rendernet_hip.h states the rule; it is integer given the hits.  return_edges=True also returns
    the edge bits (uint8 [B,ph,pw]).
    NOT differentiable: the outputs are bytes; they carry no gradient to the grid or the pose."""
    return _raycast_lines("raycast_outline", vox, pose_or_m_inv, new_size, pixels_per_cell, window, affine, threshold,
                          view_from_low_x, None, return_edges, normal_radius=normal_radius, line_radius=line_radius,
                          depth_gap=depth_gap, crease_q=crease_q, edge_mask=edge_mask, levels=0, shadow_byte=0)


def raycast_cel(vox, pose_or_m_inv, new_size=128, pixels_per_cell=4, window=None, affine=False, threshold=0.5,
                normal_radius=2, line_radius=2, depth_gap=2, crease_q=4, edge_mask=7, light=None, levels=4, shadow_byte=64,
                view_from_low_x=False, return_edges=False):
    """The ground-truth cel shading of an occupancy grid at a pose: the contours of `raycast_outline` over `levels` (2..8) flat
    tones of the diffuse term n . l, from `shadow_byte` (0..254) where the surface faces away to 255, on a white background.
    `light` is the direction to the light in the normal map's channel order (right, up, towards), as
    `tools.Phong_shading.generate_light_pos` returns it; None = the demo's light (synth.LIGHT_ELEVATION, LIGHT_AZIMUTH).  It
    is quantised by `quantise_light`; the band is then an integer function of the normal bytes.
    NOT differentiable."""
    if levels == 0 and not isinstance(levels, bool):
        raise L.RenderNetHipError("raycast_cel: levels=0 (2..8; the picture without bands is raycast_outline)")
    return _raycast_lines("raycast_cel", vox, pose_or_m_inv, new_size, pixels_per_cell, window, affine, threshold,
                          view_from_low_x, light, return_edges, normal_radius=normal_radius, line_radius=line_radius,
                          depth_gap=depth_gap, crease_q=crease_q, edge_mask=edge_mask, levels=levels, shadow_byte=shadow_byte)


# the parameters of the shadow picture: name -> (lowest, highest, default); the default of `smooth` is pixels_per_cell
SHADOW_RANGES = {"normal_radius": (1, 3, 2), "bias": (0, 3, 1), "smooth": (0, 8, None), "ambient_byte": (0, 254, 26)}


def check_shadow_options(what, **opts):
    """The integer parameters of rn_raycast_shadow_fwd / rn_shadow_encode against SHADOW_RANGES, before anything is
    launched: returns them as ints."""
    return _check_ranges(what, SHADOW_RANGES, opts)


def _demo_light():
    from . import synth
    from .tools.Phong_shading import generate_light_pos
    return generate_light_pos(synth.LIGHT_ELEVATION, synth.LIGHT_AZIMUTH)


def shadow_light(m_inv_or_pose, light=None, S=None, new_size=128, affine=True, view_from_low_x=False):
    """The direction to the light per item in source-grid coordinates, quantised (rn_shadow_light): M_inv [B,3,4] as
    `pose_to_affine` returns it (or poses [B,3] with affine=False and the grid side S) and `light`, three numbers in the normal
    map's channel order (right, up, towards the camera) as `tools.Phong_shading.generate_light_pos` returns them, None = the
    demo's light -> int32 [B,3], the largest component +-1023.  A voxel face is turned to that direction exactly when its
    encoded normal is turned to `light`.  No autograd."""
    _chk_dev(m_inv_or_pose)
    v = np.asarray(_demo_light() if light is None else light, np.float64).reshape(-1)
    if v.shape != (3,) or not np.isfinite(v).all() or not np.abs(v).max() > 0.0 or not np.isfinite(v.astype(np.float32)).all() \
            or not np.abs(v.astype(np.float32)).max() > 0.0:
        raise L.RenderNetHipError("shadow_light: expected three finite components, not all zero, got %r" % (light,))
    if not affine and S is None:
        raise L.RenderNetHipError("shadow_light: poses need the grid side S")
    m = _pose_matrices("shadow_light", m_inv_or_pose, None, S, new_size, affine)
    B = int(m.shape[0])
    with torch.no_grad():
        out = torch.empty((B, 3), dtype=torch.int32, device=m.device)
        host = (ctypes.c_float * 3)(*[float(c) for c in v])
        L.check(L.lib().rn_shadow_light(L.ptr(m) if B else None, ctypes.cast(host, ctypes.c_void_p), 1 if view_from_low_x else 0,
                                        _vp(out), B, L.stream_ptr()), "rn_shadow_light")
    return out


def raycast_shadow_from_hits(bits, box, hit, face, light_src, S, bias=1):
    """The lit flags of given hits (rn_raycast_shadow_fwd): bits, box as `voxel_pack` returns them for grids of side S, hit
    int32 [B,ph,pw] and face int8 [B,ph,pw] as rn_raycast_fwd writes them, light_src int32 [B,3] as `shadow_light` returns it
    -> uint8 [B,ph,pw]: 1 = the light reaches the entry face of the hit voxel, 0 = the face is turned away or an occupied
    voxel more than `bias` voxels (0..3, Chebyshev) from the hit voxel lies on the way, 255 = a miss.  No autograd."""
    _chk_dev(bits, box, hit, face, light_src)
    o = check_shadow_options("raycast_shadow_from_hits", bias=bias)
    bits, box, hit, face, B, ph, pw = _check_hits("raycast_shadow_from_hits", bits, box, hit, face, S)
    if light_src.dtype is not torch.int32 or tuple(light_src.shape) != (B, 3):
        raise L.RenderNetHipError("raycast_shadow_from_hits: expected light_src int32 [%d,3], got %s %s"
                                  % (B, light_src.dtype, tuple(light_src.shape)))
    with torch.no_grad():
        light_src = light_src.contiguous()
        lit = torch.empty((B, ph, pw), dtype=torch.uint8, device=hit.device)
        L.check(L.lib().rn_raycast_shadow_fwd(_vp(bits), _vp(box), _vp(hit), _vp(face), _vp(light_src), _vp(lit), B, int(S), ph, pw,
                                              o["bias"], L.stream_ptr()), "rn_raycast_shadow_fwd")
    return lit


def shadow_encode(normals, lit, light=None, smooth=0, ambient_byte=26):
    """The bytes of the shadow picture (rn_shadow_encode): normal bytes uint8 [B,ph,pw,3] and lit flags uint8 [B,ph,pw] ->
    uint8 [B,ph,pw] = ambient_byte + (255 - ambient_byte) * max(n . l, 0) * the share of lit pixels among the hit pixels within
    `smooth` pixels (0..8), rounded; 0 for a miss.  `light` as in `shadow_light`, quantised by `quantise_light`.  No autograd."""
    _chk_dev(normals, lit)
    o = check_shadow_options("shadow_encode", smooth=smooth, ambient_byte=ambient_byte)
    lq = quantise_light(_demo_light() if light is None else light)
    if lit.dim() != 3 or lit.dtype is not torch.uint8 or normals.dtype is not torch.uint8 or \
            tuple(normals.shape) != tuple(lit.shape) + (3,):
        raise L.RenderNetHipError("shadow_encode: expected uint8 normals [B,ph,pw,3] and lit [B,ph,pw], got %s %s and %s %s"
                                  % (normals.dtype, tuple(normals.shape), lit.dtype, tuple(lit.shape)))
    B, ph, pw = (int(v) for v in lit.shape)
    with torch.no_grad():
        normals, lit = normals.contiguous(), lit.contiguous()
        out = torch.empty_like(lit)
        L.check(L.lib().rn_shadow_encode(_vp(normals), _vp(lit), _vp(out), B, ph, pw, o["smooth"],
                                         o["ambient_byte"], lq[0], lq[1], lq[2], L.stream_ptr()), "rn_shadow_encode")
    return out


def raycast_shadow(vox, pose_or_m_inv, new_size=128, pixels_per_cell=4, window=None, affine=False, threshold=0.5,
                   normal_radius=2, light=None, bias=1, smooth=None, ambient_byte=26, view_from_low_x=False,
                   return_parts=False):
    """The ground-truth diffuse shading WITH CAST SHADOWS of an occupancy grid at a pose (rn_voxel_pack + rn_raycast_fwd with
    hits + rn_shadow_light + rn_raycast_shadow_fwd + rn_shadow_encode): arguments as `raycast_normals` -> uint8 [B,ph,pw], black
    where the ray misses.  `light` is the direction to the light in the normal map's channel order (right, up, towards), as
    `tools.Phong_shading.generate_light_pos` returns it; None = the demo's light.  Per hit pixel a shadow ray leaves the centre
    of the voxel face the camera ray entered by and is walked through the grid in integers; occupied voxels within `bias`
    voxels of the hit voxel (0..3) are ignored.  The byte is ambient_byte + (255 - ambient_byte) * max(n . l, 0) * lit, lit
    averaged over the hit pixels within `smooth` pixels (0..8; None = pixels_per_cell; the window of the mean is clipped to the
    cast window).  Visibility is that of the voxel solid, the diffuse term that of the stencil normal: near the terminator a
    face can be shadowed while n . l > 0.  include/rendernet_hip.h states the rule; it is integer given the hits.
    return_parts=True returns (bytes, normals uint8 [B,ph,pw,3], hit, face, light_src int32 [B,3], lit uint8 [B,ph,pw]).
    NOT differentiable: the outputs are bytes; they carry no gradient to the grid, the pose or the light."""
    smooth = int(pixels_per_cell) if smooth is None else smooth
    o = check_shadow_options("raycast_shadow", normal_radius=normal_radius, bias=bias, smooth=smooth, ambient_byte=ambient_byte)
    light = _demo_light() if light is None else light
    quantise_light(light)                                              # refused before the first stage is launched
    _chk_dev(vox, pose_or_m_inv)
    m = _pose_matrices("raycast_shadow", pose_or_m_inv, int(vox.shape[0]), vox.shape[1], new_size, affine)
    bits, box, S, normals, hit, face = _raycast("raycast_shadow", vox, m, new_size, pixels_per_cell, window, True, threshold,
                                                o["normal_radius"], view_from_low_x, True)
    light_src = shadow_light(m, light, view_from_low_x=view_from_low_x)
    lit = raycast_shadow_from_hits(bits, box, hit, face, light_src, S, o["bias"])
    out = shadow_encode(normals, lit, light, o["smooth"], o["ambient_byte"])
    return (out, normals, hit, face, light_src, lit) if return_parts else out


def _albedo_args(what, B, waves, code_q, S, base, smooth):
    """The arguments of rn_raycast_albedo_fwd / rn_albedo_encode, checked before anything is launched: (K, base as three
    ints, smooth)."""
    if not torch.is_tensor(waves) or not torch.is_tensor(code_q):
        raise L.RenderNetHipError("%s: waves and code_q must be device tensors, got %s and %s"
                                  % (what, type(waves).__name__, type(code_q).__name__))
    _chk_dev(waves, code_q)
    if waves.dtype is not torch.int16 or waves.dim() != 2 or waves.shape[1] != 8 or not 1 <= waves.shape[0] <= 256:
        raise L.RenderNetHipError("%s: expected waves int16 [K,8] with K in 1..256 (synth.ColourModel.waves), got %s %s"
                                  % (what, waves.dtype, tuple(waves.shape)))
    K = int(waves.shape[0])
    if code_q.dtype is not torch.int8 or tuple(code_q.shape) != (B, K):
        raise L.RenderNetHipError("%s: expected code_q int8 [%d,%d] (synth.ColourModel.quantise), got %s %s"
                                  % (what, B, K, code_q.dtype, tuple(code_q.shape)))
    S = int(S)
    if S < 32 or S > 128 or S % 32 != 0:
        raise L.RenderNetHipError("%s: S=%d (a multiple of 32 up to 128)" % (what, S))
    try:
        base = tuple(int(c) for c in base)
    except (TypeError, ValueError):
        base = ()
    if len(base) != 3 or not all(0 <= c <= 255 for c in base):
        raise L.RenderNetHipError("%s: base=%r, expected three bytes 0..255" % (what, base))
    if isinstance(smooth, (bool, float)) or not 0 <= int(smooth) <= 8:
        raise L.RenderNetHipError("%s: smooth=%r (0..8 pixels)" % (what, smooth))
    return K, base, int(smooth)


def albedo_from_hits(hit, waves, code_q, S, base, smooth=0):
    """The albedo picture of given hits (rn_raycast_albedo_fwd, then rn_albedo_encode when smooth > 0): hit int32 [B,ph,pw]
    (flat index of the hit voxel in a grid of side S, as rn_raycast_fwd writes it; < 0 or >= S^3 = a miss), waves int16 [K,8]
    and base as `synth.ColourModel` holds them, code_q int8 [B,K] -> uint8 [B,ph,pw,3]: base + the code-weighted sum of K
    quantised plane waves at the hit voxel, black for a miss, averaged over the hit pixels within `smooth` pixels (0..8; the
    window of the mean is clipped to the picture).  include/rendernet_hip.h states the rule; it is integer.  No autograd."""
    _chk_dev(hit)
    if hit.dim() != 3 or hit.dtype is not torch.int32:
        raise L.RenderNetHipError("albedo_from_hits: expected hit int32 [B,ph,pw], got %s %s" % (hit.dtype, tuple(hit.shape)))
    B, ph, pw = (int(v) for v in hit.shape)
    K, base, smooth = _albedo_args("albedo_from_hits", B, waves, code_q, S, base, smooth)
    with torch.no_grad():
        hit, waves, code_q = hit.contiguous(), waves.contiguous(), code_q.contiguous()
        colour = torch.empty((B, ph, pw, 3), dtype=torch.uint8, device=hit.device)
        host = (ctypes.c_int * 3)(*base)
        L.check(L.lib().rn_raycast_albedo_fwd(_vp(hit), _vp(waves), _vp(code_q), ctypes.cast(host, ctypes.c_void_p), _vp(colour), B,
                                              int(S), K, ph, pw, L.stream_ptr()), "rn_raycast_albedo_fwd")
        if smooth == 0:
            return colour
        out = torch.empty_like(colour)
        L.check(L.lib().rn_albedo_encode(_vp(colour), _vp(hit), _vp(out), B, int(S), ph, pw, smooth,
                                         L.stream_ptr()), "rn_albedo_encode")
    return out


def raycast_albedo(vox, pose_or_m_inv, waves, code_q, base, new_size=128, pixels_per_cell=4, window=None, affine=False,
                   threshold=0.5, normal_radius=2, smooth=None, view_from_low_x=False):
    """The ground-truth albedo AND normal map of an occupancy grid at a pose, from one pack and one cast (rn_voxel_pack +
    rn_raycast_fwd with hits + rn_raycast_albedo_fwd + rn_albedo_encode): vox, pose and the geometry arguments as
    `raycast_normals`; waves, code_q, base as `albedo_from_hits` -> (albedo uint8 [B,ph,pw,3], normals uint8 [B,ph,pw,3]), both
    black where the ray misses.  The albedo is a linear colour field over the voxel lattice weighted by the quantised texture
    code, the stand-in for a morphable model's mean + basis * beta; `smooth` (0..8; None = pixels_per_cell, the footprint of
    one voxel) averages it over the hit pixels nearby, as `raycast_ao` does.
    NOT differentiable: the outputs are bytes; they carry no gradient to the grid, the pose or the code."""
    smooth = int(pixels_per_cell) if smooth is None else smooth
    _chk_dev(vox)
    if vox.dim() not in (4, 5):
        raise L.RenderNetHipError("raycast_albedo: expected [B,S,S,S,1] occupancy, got %s" % (tuple(vox.shape),))
    _albedo_args("raycast_albedo", int(vox.shape[0]), waves, code_q, int(vox.shape[1]), base, smooth)   # before the first stage
    _, _, S, normals, hit, _ = _raycast("raycast_albedo", vox, pose_or_m_inv, new_size, pixels_per_cell, window, affine, threshold,
                                        normal_radius, view_from_low_x, True)
    return albedo_from_hits(hit, waves, code_q, S, base, smooth), normals


# ---- Voxel carving: from views back to a grid (rn_hit_depth, rn_voxel_carve; include/rendernet_hip.h states the rule).

CARVE_RANGES = {"slack": (0, 65535, 8), "tolerance": (0, 254, 0)}
CARVE_OUTSIDE = {"keep": 1, "carve": 0}
CARVE_MAX_VIEWS = 255              # votes is a byte
CARVE_MAX_VIEW_SETS = 65535        # B K (item, view) pairs per call
CARVE_MIN_PIXELS_PER_VOXEL = 1.5   # below it the hull may lose voxels of the grid that was scanned


def _frame_window(what, window, new_size, pixels_per_cell):
    """The frame and the window inside it, before anything is launched: (N, f, row0, col0, ph, pw)."""
    N, f = int(new_size), int(pixels_per_cell)
    if not (1 <= N <= 256 and 1 <= f <= 16 and f * N <= RASTER_MAX_SIDE):
        raise L.RenderNetHipError("%s: new_size=%d, pixels_per_cell=%d (new_size <= 256, pixels_per_cell <= 16, their product <= %d)"
                                  % (what, N, f, RASTER_MAX_SIDE))
    if window is None:
        window = (0, 0, f * N, f * N)
    if len(tuple(window)) != 4:
        raise L.RenderNetHipError("%s: window=%r (row0, col0, ph, pw)" % (what, window))
    row0, col0, ph, pw = (int(v) for v in window)
    if ph < 1 or pw < 1 or row0 < 0 or col0 < 0 or row0 + ph > f * N or col0 + pw > f * N:
        raise L.RenderNetHipError("%s: window %s outside the %d x %d frame" % (what, (row0, col0, ph, pw), f * N, f * N))
    return N, f, row0, col0, ph, pw


def _ray_ends(what, view_from_low_x, K):
    """view_from_low_x as K bools: one bool for all views, or a sequence of K."""
    if isinstance(view_from_low_x, (bool, np.bool_)):
        return [bool(view_from_low_x)] * K
    try:
        low = list(view_from_low_x)
    except TypeError:
        low = None
    if low is None or len(low) != K or not all(isinstance(v, (bool, np.bool_)) for v in low):
        raise L.RenderNetHipError("%s: view_from_low_x=%r (a bool, or %d bools, one per view)" % (what, view_from_low_x, K))
    return [bool(v) for v in low]


def _view_poses(what, pose_or_m_inv, affine):
    """Poses [B,K,3] (or matrices [B,K,3,4] with affine=True) -> (the tensor flattened over (item, view), B, K)."""
    err = L.RenderNetHipError
    if not torch.is_tensor(pose_or_m_inv):
        raise err("%s: expected a float tensor for the poses, got %s" % (what, type(pose_or_m_inv).__name__))
    tail = (3, 4) if affine else (3,)
    if pose_or_m_inv.dim() != 2 + len(tail) or tuple(pose_or_m_inv.shape[2:]) != tail:
        raise err("%s: expected %s [B,K,%s], got %s" % (what, "matrices" if affine else "poses", ",".join(str(v) for v in tail),
                                                        tuple(pose_or_m_inv.shape)))
    B, K = int(pose_or_m_inv.shape[0]), int(pose_or_m_inv.shape[1])
    if not 1 <= K <= CARVE_MAX_VIEWS:
        raise err("%s: K=%d views (1..%d)" % (what, K, CARVE_MAX_VIEWS))
    if B * K > CARVE_MAX_VIEW_SETS:
        raise err("%s: B K = %d (item, view) pairs (at most %d per call)" % (what, B * K, CARVE_MAX_VIEW_SETS))
    return pose_or_m_inv.reshape((B * K,) + tail), B, K


def carve_cameras(pose_or_m_inv, S, new_size=128, pixels_per_cell=4, affine=False, view_from_low_x=False):
    """The integer cameras `voxel_carve` projects with: poses [B,K,3] (or M_inv [B,K,3,4] with affine=True) -> int64 [B,K,3,4],
    `mesh_camera` of every (item, view); view_from_low_x is one bool or K bools, and rn_mesh_camera is called once per ray end
    that occurs."""
    what = "carve_cameras"
    S = _grid_side(what, S)
    flat, B, K = _view_poses(what, pose_or_m_inv, affine)
    low = _ray_ends(what, view_from_low_x, K)
    cams = {end: mesh_camera(flat, S, new_size, pixels_per_cell, affine, end) for end in sorted(set(low))}
    if len(cams) == 1:
        return cams[low[0]].view(B, K, 3, 4)
    pick = torch.tensor(low, dtype=torch.bool, device=flat.device).view(1, K, 1, 1)
    return torch.where(pick, cams[True].view(B, K, 3, 4), cams[False].view(B, K, 3, 4)).contiguous()


def carve_pixels_per_voxel(cam):
    """Pixels per voxel of integer cameras int64 [...,3,4]: the smaller of |row 0| and |row 1| (the Euclidean norm of the three
    coefficients) over 2^20, float64 [...] -- f * scale for a pose.  At 1.5 or more the hull of `voxel_carve` cannot lose a voxel
    of the grid that was scanned (include/rendernet_hip.h has the argument)."""
    if not torch.is_tensor(cam) or cam.dtype is not torch.int64 or cam.dim() < 2 or tuple(cam.shape[-2:]) != (3, 4):
        raise L.RenderNetHipError("carve_pixels_per_voxel: expected int64 cameras [...,3,4]")
    a = cam[..., :2, :3].to(torch.float64)
    return torch.sqrt((a * a).sum(-1)).amin(-1) / float(1 << 20)


def hit_depth(hit, face, pose_or_m_inv, S, new_size=128, pixels_per_cell=4, window=None, affine=False, view_from_low_x=False):
    """The depth at which each ray of a cast entered the voxel it hit (rn_hit_depth): hit int32 and face int8 [B,ph,pw] as
    `raycast_normals(..., return_hits=True)` returns them for the same pose, window and ray end -> int32 [B,ph,pw] in 1/256
    camera cell, the unit and the meaning of `rasterize_mesh`'s depth, -1 for a miss.  It is the caster's own ray parameter at
    the entry face, re-derived in float64.  No autograd."""
    what, err = "hit_depth", L.RenderNetHipError
    S = _grid_side(what, S)
    if not torch.is_tensor(hit) or not torch.is_tensor(face):
        raise err("%s: expected hit int32 and face int8 tensors [B,ph,pw]" % what)
    _chk_dev(hit, face)
    if hit.dim() != 3 or hit.shape != face.shape or hit.dtype is not torch.int32 or face.dtype is not torch.int8:
        raise err("%s: expected hit int32 and face int8 [B,ph,pw], got %s %s and %s %s"
                  % (what, hit.dtype, tuple(hit.shape), face.dtype, tuple(face.shape)))
    N, f, row0, col0, ph, pw = _frame_window(what, window, new_size, pixels_per_cell)
    if (ph, pw) != tuple(hit.shape[1:]):
        raise err("%s: hits of %d x %d pixels for a window of %d x %d" % (what, hit.shape[1], hit.shape[2], ph, pw))
    if not torch.is_tensor(pose_or_m_inv) or pose_or_m_inv.dim() < 1 or int(pose_or_m_inv.shape[0]) != int(hit.shape[0]) \
            or pose_or_m_inv.device != hit.device:
        raise err("%s: expected one pose on %s for each of the %d items of hit" % (what, hit.device, hit.shape[0]))
    m, B, N, f = _raster_camera_args(what, pose_or_m_inv, S, N, f, affine)
    hit, face = hit.contiguous(), face.contiguous()
    depth = torch.empty((B, ph, pw), dtype=torch.int32, device=hit.device)
    if B:
        with torch.cuda.device(hit.device):
            L.check(L.lib().rn_hit_depth(_vp(hit), _vp(face), L.ptr(m), _vp(depth), B, S, N, f, row0, col0, ph, pw,
                                         1 if view_from_low_x else 0, L.stream_ptr()), "rn_hit_depth")
    return depth


def voxel_carve(views, pose_or_m_inv, S, new_size=128, pixels_per_cell=4, window=None, affine=False, view_from_low_x=False,
                use_depth=True, slack=8, tolerance=0, outside="keep", return_votes=False):
    """A grid carved from views (rn_voxel_carve; include/rendernet_hip.h states the rule): views int32 [B,K,ph,pw] on the device
    -- -1 = background, otherwise the depth at which the pixel's ray enters the surface, in 1/256 camera cell, as `hit_depth`,
    `voxel_scan` and `rasterize_mesh(..., return_ids=True)` give it; for silhouettes any value >= 0 is foreground -- and the
    poses [B,K,3] they were taken at (or M_inv [B,K,3,4] with affine=True) -> uint8 [B,S,S,S,1], 0 or 1: the voxels that at least
    K - tolerance views are consistent with.  A view is consistent with a voxel when the pixel holding the voxel's centre is
    foreground and, with use_depth, the centre is not more than `slack` units in front of the surface seen there; a centre that
    falls outside the window is consistent under outside="keep" (a view cannot carve what it does not see) and inconsistent
    under "carve".  use_depth=False gives the visual hull.  view_from_low_x is a bool or K bools.  return_votes=True also returns
    the count of consistent views, uint8 [B,S,S,S]; `voxel_pack(votes, K - tolerance - 0.5)` is the hull as a bit grid.
    With cameras of at least 1.5 pixels per voxel (`carve_pixels_per_voxel(carve_cameras(...))`; pixels_per_cell * scale for a
    pose) the hull of a scan contains every voxel of the grid that was scanned; smaller cameras are not refused.
    views is B K ph pw words -- 604 MB for 24 items of 24 views at 512^2; when that does not fit, carve K in chunks with
    return_votes=True and add the votes.  One launch, no atomics: the same input gives the same bits.  dtype, shapes, the window
    and the options are checked before anything is launched.  No autograd."""
    what, err = "voxel_carve", L.RenderNetHipError
    S = _grid_side(what, S)
    if not torch.is_tensor(views) or views.dtype is not torch.int32 or views.dim() != 4:
        raise err("%s: expected views as an int32 tensor [B,K,ph,pw], got %s"
                  % (what, "%s %s" % (views.dtype, tuple(views.shape)) if torch.is_tensor(views) else type(views).__name__))
    _chk_dev(views)
    opts = _check_ranges(what, CARVE_RANGES, {"slack": slack, "tolerance": tolerance})
    if not isinstance(outside, str) or outside not in CARVE_OUTSIDE:
        raise err("%s: outside=%r (keep or carve)" % (what, outside))
    for name, v in (("use_depth", use_depth), ("return_votes", return_votes)):
        if not isinstance(v, bool):
            raise err("%s: %s=%r (True or False)" % (what, name, v))
    flat, B, K = _view_poses(what, pose_or_m_inv, affine)
    if opts["tolerance"] >= K:
        raise err("%s: tolerance=%d for %d views (0..%d)" % (what, opts["tolerance"], K, K - 1))
    _ray_ends(what, view_from_low_x, K)
    _chk_dev(flat)
    N, f, row0, col0, ph, pw = _frame_window(what, window, new_size, pixels_per_cell)
    if tuple(views.shape) != (B, K, ph, pw) or views.device != flat.device:
        raise err("%s: views %s on %s for %d items of %d views, a window of %d x %d, poses on %s"
                  % (what, tuple(views.shape), views.device, B, K, ph, pw, flat.device))
    views = views.contiguous()
    dev = views.device
    votes = torch.empty((B, S, S, S), dtype=torch.uint8, device=dev)
    if B:
        cam = carve_cameras(pose_or_m_inv, S, N, f, affine, view_from_low_x)
        with torch.cuda.device(dev):
            L.check(L.lib().rn_voxel_carve(_vp(views), _vp(cam), _vp(votes), B, K, S, N, f, row0, col0, ph, pw,
                                           1 if use_depth else 0, opts["slack"], CARVE_OUTSIDE[outside], L.stream_ptr()),
                    "rn_voxel_carve")
    hull = (votes >= K - opts["tolerance"]).to(torch.uint8).unsqueeze(-1)
    return (hull, votes) if return_votes else hull


def voxel_scan(vox, poses, new_size=128, pixels_per_cell=4, window=None, view_from_low_x=False, threshold=0.5, return_hits=False):
    """The depth views of grids from K poses each, what `voxel_carve` takes: vox [B,S,S,S,1] as `raycast_normals` takes it, poses
    [B,K,3] -> int32 [B,K,ph,pw].  One pack, K casts with hits (rn_raycast_fwd) and their entry depths (`hit_depth`); view_from_low_x is a
    bool or K bools.  `voxel_carve(voxel_scan(vox, poses, ...), poses, S, ...)` is the round trip.  return_hits=True returns
    (views, hits), hits int32 [B,K,ph,pw] being the flat index of the voxel each ray hit (-1 = miss), what `voxel_colour_sums`
    takes.  No autograd."""
    what = "voxel_scan"
    if not isinstance(return_hits, bool):
        raise L.RenderNetHipError("%s: return_hits=%r (True or False)" % (what, return_hits))
    if not torch.is_tensor(vox):
        raise L.RenderNetHipError("%s: expected a tensor [B,S,S,S,1], got %s" % (what, type(vox).__name__))
    _chk_dev(vox)
    _, B, S = _occupancy(what, vox, GRID_SIDES)
    flat, Bp, K = _view_poses(what, poses, False)
    if Bp != B or flat.device != vox.device:
        raise L.RenderNetHipError("%s: poses %s on %s for %d grids on %s" % (what, tuple(poses.shape), flat.device, B, vox.device))
    low = _ray_ends(what, view_from_low_x, K)
    N, f, row0, col0, ph, pw = _frame_window(what, window, new_size, pixels_per_cell)
    views = torch.empty((B, K, ph, pw), dtype=torch.int32, device=vox.device)
    hits = torch.empty((B, K, ph, pw), dtype=torch.int32, device=vox.device) if return_hits else None
    if B == 0:
        return (views, hits) if return_hits else views
    out = torch.empty((B, ph, pw, 3), dtype=torch.uint8, device=vox.device)
    hit = torch.empty((B, ph, pw), dtype=torch.int32, device=vox.device)
    face = torch.empty((B, ph, pw), dtype=torch.int8, device=vox.device)
    with torch.no_grad(), torch.cuda.device(vox.device):
        bits, box = voxel_pack(vox, threshold)                    # once: the K casts read the same bits
        m_all = pose_to_affine(flat.detach().contiguous().float(), S, N).view(B, K, 3, 4)
        for k in range(K):
            m = m_all[:, k].contiguous()
            L.check(L.lib().rn_raycast_fwd(_vp(bits), _vp(box), L.ptr(m), _vp(out), _vp(hit), _vp(face), B, S, N, f, row0, col0, ph, pw,
                                           2, 1 if low[k] else 0, L.stream_ptr()), "rn_raycast_fwd")
            views[:, k] = hit_depth(hit, face, m, S, N, f, (row0, col0, ph, pw), True, low[k])
            if return_hits:
                hits[:, k] = hit
    return (views, hits) if return_hits else views


# ---- Voxel colouring: from posed pictures back to the colour of a grid and of its mesh (rn_voxel_colour_accumulate, _resolve,
# ---- _fill, rn_colour_from_hits, rn_mesh_vertex_colours; include/rendernet_hip.h states the rule).

COLOUR_MAX_PIXELS = 8421504        # K ph pw per call: 255 times more would reach 2^31, the int32 sums could wrap
COLOUR_MAX_VIEWS = 65535
COLOUR_MAX_FILL = 64
COLOUR_MAX_SIDE = 4096             # ph, pw


def _colour_bytes(what, name, c):
    """A colour as three ints 0..255."""
    try:
        c = tuple(c)
    except TypeError:
        c = ()
    if len(c) != 3 or not all(isinstance(v, (int, np.integer)) and not isinstance(v, bool) and 0 <= int(v) <= 255 for v in c):
        raise L.RenderNetHipError("%s: %s=%r, expected three bytes 0..255" % (what, name, c))
    return tuple(int(v) for v in c)


def _colour_grids(what, colours, known=None):
    """colours uint8 [B,S,S,S,3] on the device (and known uint8 [B,S,S,S] beside it): (colours, known, B, S), contiguous."""
    err = L.RenderNetHipError
    if not torch.is_tensor(colours) or colours.dtype is not torch.uint8 or colours.dim() != 5 or colours.shape[4] != 3 \
            or not (colours.shape[1] == colours.shape[2] == colours.shape[3]) or int(colours.shape[1]) not in GRID_SIDES:
        raise err("%s: expected colours uint8 [B,S,S,S,3] with S = %s, got %s"
                  % (what, _one_of(GRID_SIDES), "%s %s" % (colours.dtype, tuple(colours.shape)) if torch.is_tensor(colours)
                     else type(colours).__name__))
    _chk_dev(colours)
    B, S = int(colours.shape[0]), int(colours.shape[1])
    if B > 65535:
        raise err("%s: B=%d (at most 65535 per call)" % (what, B))
    if known is not None:
        if not torch.is_tensor(known) or known.dtype is not torch.uint8 or tuple(known.shape) != (B, S, S, S) \
                or known.device != colours.device:
            raise err("%s: expected known uint8 [%d,%d,%d,%d] on %s, got %s"
                      % (what, B, S, S, S, colours.device, "%s %s on %s" % (known.dtype, tuple(known.shape), known.device)
                         if torch.is_tensor(known) else type(known).__name__))
        known = known.contiguous()
    return colours.contiguous(), known, B, S


def voxel_colour_sums(images, hits, S, mask=None, sums=None):
    """The colour sums of posed pictures per voxel (rn_voxel_colour_accumulate; include/rendernet_hip.h states the rule): images
    uint8 [B,K,ph,pw,3], hits int32 [B,K,ph,pw] -- the flat index of the voxel each pixel's ray hit in a grid of side S, as
    `voxel_scan(..., return_hits=True)` and `raycast_normals(..., return_hits=True)` give it for the picture's pose, window and
    ray end -- and optionally mask uint8 [B,K,ph,pw], 0 = ignore the pixel -> int32 [B,S,S,S,4]: (sum of red, of green, of blue,
    count) over the pixels that hit the voxel.  A hit outside [0, S^3) is ignored.  `sums`, if given, is ADDED into and returned;
    otherwise the sums start at zero.  One call takes at most COLOUR_MAX_PIXELS = 8 421 504 pixels per item (K ph pw; 255 times
    more would wrap an int32) and refuses more: chunking K is the caller's job, as with `voxel_carve` -- pass the `sums` of one
    chunk to the next -- and so is keeping the total of the chunks within what an int32 holds.  Integer adds commute: the same
    input gives the same bits.  Everything is checked before anything is launched.  No autograd."""
    what, err = "voxel_colour_sums", L.RenderNetHipError
    S = _grid_side(what, S)
    if not torch.is_tensor(images) or images.dtype is not torch.uint8 or images.dim() != 5 or images.shape[4] != 3:
        raise err("%s: expected images as a uint8 tensor [B,K,ph,pw,3], got %s"
                  % (what, "%s %s" % (images.dtype, tuple(images.shape)) if torch.is_tensor(images) else type(images).__name__))
    _chk_dev(images)
    B, K, ph, pw = (int(v) for v in images.shape[:4])
    dev = images.device
    for name, t, dtype in (("hits", hits, torch.int32), ("mask", mask, torch.uint8)):
        if t is None and name == "mask":
            continue
        if not torch.is_tensor(t) or t.dtype is not dtype or tuple(t.shape) != (B, K, ph, pw) or t.device != dev:
            raise err("%s: expected %s %s [%d,%d,%d,%d] on %s, got %s"
                      % (what, name, dtype, B, K, ph, pw, dev, "%s %s on %s" % (t.dtype, tuple(t.shape), t.device)
                         if torch.is_tensor(t) else type(t).__name__))
    if B > 65535:
        raise err("%s: B=%d (at most 65535 per call)" % (what, B))
    if not 1 <= K <= COLOUR_MAX_VIEWS or not (1 <= ph <= COLOUR_MAX_SIDE and 1 <= pw <= COLOUR_MAX_SIDE):
        raise err("%s: images of %d views of %d x %d pixels (1..%d views, 1..%d pixels each way)"
                  % (what, K, ph, pw, COLOUR_MAX_VIEWS, COLOUR_MAX_SIDE))
    if K * ph * pw > COLOUR_MAX_PIXELS:
        raise err("%s: K ph pw = %d pixels per item, the limit per call is %d (255 times more would wrap an int32 sum): "
                  "accumulate K in chunks" % (what, K * ph * pw, COLOUR_MAX_PIXELS))
    if sums is None:
        sums = torch.zeros((B, S, S, S, 4), dtype=torch.int32, device=dev)
    elif not torch.is_tensor(sums) or sums.dtype is not torch.int32 or tuple(sums.shape) != (B, S, S, S, 4) or sums.device != dev \
            or not sums.is_contiguous():
        raise err("%s: expected sums as a contiguous int32 tensor [%d,%d,%d,%d,4] on %s, got %s"
                  % (what, B, S, S, S, dev, "%s %s on %s" % (sums.dtype, tuple(sums.shape), sums.device)
                     if torch.is_tensor(sums) else type(sums).__name__))
    if B:
        images, hits = images.contiguous(), hits.contiguous()
        mask = None if mask is None else mask.contiguous()
        with torch.cuda.device(dev):
            L.check(L.lib().rn_voxel_colour_accumulate(_vp(images), _vp(hits), _vp(mask), _vp(sums), B, K, S, ph, pw,
                                                       L.stream_ptr()), "rn_voxel_colour_accumulate")
    return sums


def voxel_colours(sums, vox=None, threshold=0.5, fill=0, unseen=(128, 128, 128)):
    """The colour of every voxel from its sums (rn_voxel_colour_resolve, then `fill` passes of rn_voxel_colour_fill): sums int32
    [B,S,S,S,4] as `voxel_colour_sums` returns them -> (colours uint8 [B,S,S,S,3], known uint8 [B,S,S,S]).  A voxel that pixels
    hit gets the mean of their colours, rounded half up, and known = 1; every other voxel the `unseen` colour and known = 0.
    fill = 1..64 then runs that many Jacobi passes over the voxels of `vox` ([B,S,S,S,1], occupied above `threshold`): an
    occupied voxel without a colour takes the rounded mean of those of its 26 neighbours that had one before the pass, and
    known = 2.  fill > 0 requires vox.  No autograd."""
    what, err = "voxel_colours", L.RenderNetHipError
    if not torch.is_tensor(sums) or sums.dtype is not torch.int32 or sums.dim() != 5 or sums.shape[4] != 4 \
            or not (sums.shape[1] == sums.shape[2] == sums.shape[3]) or int(sums.shape[1]) not in GRID_SIDES:
        raise err("%s: expected sums int32 [B,S,S,S,4] with S = %s, got %s"
                  % (what, _one_of(GRID_SIDES), "%s %s" % (sums.dtype, tuple(sums.shape)) if torch.is_tensor(sums)
                     else type(sums).__name__))
    _chk_dev(sums)
    B, S, dev = int(sums.shape[0]), int(sums.shape[1]), sums.device
    if B > 65535:
        raise err("%s: B=%d (at most 65535 per call)" % (what, B))
    unseen = _colour_bytes(what, "unseen", unseen)
    if isinstance(fill, (bool, float)) or not isinstance(fill, (int, np.integer)) or not 0 <= int(fill) <= COLOUR_MAX_FILL:
        raise err("%s: fill=%r (0..%d passes)" % (what, fill, COLOUR_MAX_FILL))
    fill = int(fill)
    threshold = _finite(what, "threshold", threshold, "number")
    if fill > 0:
        if vox is None:
            raise err("%s: fill=%d needs vox, the grid whose occupied voxels are filled" % (what, fill))
        if not torch.is_tensor(vox):
            raise err("%s: expected vox as a tensor [B,S,S,S,1], got %s" % (what, type(vox).__name__))
        _chk_dev(vox)
        v4 = _grid_view(vox)
        if tuple(v4.shape) != (B, S, S, S) or vox.device != dev:
            raise err("%s: vox %s on %s for sums of %d grids of side %d on %s" % (what, tuple(vox.shape), vox.device, B, S, dev))
    colours = torch.empty((B, S, S, S, 3), dtype=torch.uint8, device=dev)
    known = torch.empty((B, S, S, S), dtype=torch.uint8, device=dev)
    if B == 0:
        return colours, known
    sums = sums.contiguous()
    with torch.no_grad(), torch.cuda.device(dev):
        lib = L.lib()
        L.check(lib.rn_voxel_colour_resolve(_vp(sums), _vp(colours), _vp(known), B, S, unseen[0], unseen[1], unseen[2],
                                            L.stream_ptr()), "rn_voxel_colour_resolve")
        if fill:
            bits, _ = voxel_pack(vox, threshold)
            colours2, known2 = torch.empty_like(colours), torch.empty_like(known)
            for _ in range(fill):                                 # ping-pong: a pass reads the state before it
                L.check(lib.rn_voxel_colour_fill(_vp(colours), _vp(known), _vp(bits), _vp(colours2), _vp(known2), B, S,
                                                 L.stream_ptr()), "rn_voxel_colour_fill")
                colours, colours2, known, known2 = colours2, colours, known2, known
    return colours, known


def colour_from_hits(hit, colours, S, smooth=0, background=(0, 0, 0)):
    """The picture of coloured grids on given hits (rn_colour_from_hits, then rn_albedo_encode when smooth > 0): hit int32
    [B,ph,pw] as `albedo_from_hits` takes it, colours uint8 [B,S,S,S,3] -> uint8 [B,ph,pw,3]: the colour of the hit voxel, and
    `background` for a miss.  smooth = 1..8 averages the colours over the hit pixels within that many pixels, as the albedo
    does (the window of the mean is clipped to the picture); the misses keep the background.  No autograd."""
    what, err = "colour_from_hits", L.RenderNetHipError
    S = _grid_side(what, S)
    if not torch.is_tensor(hit) or hit.dim() != 3 or hit.dtype is not torch.int32:
        raise err("%s: expected hit int32 [B,ph,pw], got %s"
                  % (what, "%s %s" % (hit.dtype, tuple(hit.shape)) if torch.is_tensor(hit) else type(hit).__name__))
    _chk_dev(hit)
    colours, _, B, Sc = _colour_grids(what, colours)
    ph, pw = int(hit.shape[1]), int(hit.shape[2])
    if Sc != S or int(hit.shape[0]) != B or colours.device != hit.device:
        raise err("%s: colours %s on %s for hits %s on %s in grids of side %d"
                  % (what, tuple(colours.shape), colours.device, tuple(hit.shape), hit.device, S))
    if not (1 <= ph <= COLOUR_MAX_SIDE and 1 <= pw <= COLOUR_MAX_SIDE):
        raise err("%s: hits of %d x %d pixels (1..%d each way)" % (what, ph, pw, COLOUR_MAX_SIDE))
    if isinstance(smooth, (bool, float)) or not isinstance(smooth, (int, np.integer)) or not 0 <= int(smooth) <= 8:
        raise err("%s: smooth=%r (0..8 pixels)" % (what, smooth))
    background = _colour_bytes(what, "background", background)
    out = torch.empty((B, ph, pw, 3), dtype=torch.uint8, device=hit.device)
    if B == 0:
        return out
    hit = hit.contiguous()
    with torch.no_grad(), torch.cuda.device(hit.device):
        L.check(L.lib().rn_colour_from_hits(_vp(hit), _vp(colours), _vp(out), B, S, ph, pw, background[0], background[1],
                                            background[2], L.stream_ptr()), "rn_colour_from_hits")
        if int(smooth) == 0:
            return out
        soft = torch.empty_like(out)
        L.check(L.lib().rn_albedo_encode(_vp(out), _vp(hit), _vp(soft), B, S, ph, pw, int(smooth), L.stream_ptr()),
                "rn_albedo_encode")
        if background != (0, 0, 0):                               # the encode stage blackens a miss: give it its colour back
            miss = ((hit < 0) | (hit >= S ** 3)).unsqueeze(-1)
            soft = torch.where(miss, out, soft)
    return soft


def raycast_colour(vox, colours, pose_or_m_inv, new_size=128, pixels_per_cell=4, window=None, affine=False, threshold=0.5,
                   normal_radius=2, smooth=0, view_from_low_x=False, background=(0, 0, 0), return_hits=False):
    """The picture of coloured grids at a pose, from one pack and one cast (rn_voxel_pack + rn_raycast_fwd with hits +
    `colour_from_hits`): vox [B,S,S,S,1], pose [B,3] and the geometry arguments as `raycast_albedo` takes them, colours uint8
    [B,S,S,S,3] as `voxel_colours` returns them -> uint8 [B,ph,pw,3].  With the colours that `voxel_colours` recovered from
    unsmoothed pictures it returns those pictures at their poses, pixel for pixel.  return_hits=True also returns the hits
    int32 [B,ph,pw].  No autograd."""
    what = "raycast_colour"
    if not torch.is_tensor(vox):
        raise L.RenderNetHipError("%s: expected vox as a tensor [B,S,S,S,1], got %s" % (what, type(vox).__name__))
    _chk_dev(vox)
    _, B, S = _occupancy(what, vox, GRID_SIDES)
    colours, _, Bc, Sc = _colour_grids(what, colours)
    if (Bc, Sc) != (B, S) or colours.device != vox.device:
        raise L.RenderNetHipError("%s: colours %s on %s for grids %s on %s"
                                  % (what, tuple(colours.shape), colours.device, tuple(vox.shape), vox.device))
    if isinstance(smooth, (bool, float)) or not isinstance(smooth, (int, np.integer)) or not 0 <= int(smooth) <= 8:
        raise L.RenderNetHipError("%s: smooth=%r (0..8 pixels)" % (what, smooth))
    background = _colour_bytes(what, "background", background)
    N, f, row0, col0, ph, pw = _frame_window(what, window, new_size, pixels_per_cell)
    if B == 0:
        out = torch.empty((0, ph, pw, 3), dtype=torch.uint8, device=vox.device)
        return (out, torch.empty((0, ph, pw), dtype=torch.int32, device=vox.device)) if return_hits else out
    with torch.cuda.device(vox.device):
        _, _, _, _, hit, _ = _raycast(what, vox, pose_or_m_inv, N, f, (row0, col0, ph, pw), affine, threshold, normal_radius,
                                      view_from_low_x, True)
        out = colour_from_hits(hit, colours, S, smooth, background)
    return (out, hit) if return_hits else out


def mesh_vertex_colours(mesh, colours, known, unseen=(128, 128, 128)):
    """The colour of every vertex of an `ExtractedMesh` (rn_mesh_vertex_colours): colours uint8 [B,S,S,S,3] and known uint8
    [B,S,S,S] as `voxel_colours` returns them for the B grids the mesh was extracted from -> uint8 [V,3], the rounded mean of
    the known ones of the 2^3 voxels around the vertex's cell, `unseen` where none is known.  No autograd."""
    what, err = "mesh_vertex_colours", L.RenderNetHipError
    if not isinstance(mesh, ExtractedMesh):
        raise err("%s: expected an ExtractedMesh (ops.extract_mesh), got %s" % (what, type(mesh).__name__))
    colours, known, B, S = _colour_grids(what, colours, known)
    unseen = _colour_bytes(what, "unseen", unseen)
    q, vo = mesh.q, mesh.vert_offsets
    if q.dtype is not torch.int32 or q.dim() != 2 or q.shape[1] != 3 or vo.dtype is not torch.int64 or tuple(vo.shape) != (B + 1,) \
            or q.device != colours.device or vo.device != colours.device:
        raise err("%s: a mesh of %s vertices %s and offsets %s on %s for %d coloured grids on %s"
                  % (what, q.dtype, tuple(q.shape), tuple(vo.shape), q.device, B, colours.device))
    V = int(q.shape[0])
    out = torch.empty((V, 3), dtype=torch.uint8, device=q.device)
    if V and B:
        q, vo = q.contiguous(), vo.contiguous()
        with torch.cuda.device(q.device):
            L.check(L.lib().rn_mesh_vertex_colours(_vp(q), V, _vp(vo), _vp(colours), _vp(known), _vp(out), B, S, unseen[0],
                                                   unseen[1], unseen[2], L.stream_ptr()), "rn_mesh_vertex_colours")
    return out


# ---- Coloured meshes drawn (rn_mesh_face_voxels, rn_mesh_colour_from_ids; include/rendernet_hip.h states the two rules).

def mesh_face_voxels(mesh, vol, threshold=0.5):
    """The solid voxel every face of a surface net bounds (rn_mesh_face_voxels): `mesh` an `ExtractedMesh` with quads or
    triangles, relaxed or not, and vol [B,S,S,S,1] (or [B,S,S,S]) float32 or uint8 with the `threshold` it was extracted at
    -> int32 [F]: the flat index (zs S + ys) S + xs, within its grid, of the inside sample of the sample edge the face was
    emitted for -- what the ray caster calls the hit of a ray that enters through that side -- or -1 for a face that is none of
    this grid's.  No autograd."""
    what, err = "mesh_face_voxels", L.RenderNetHipError
    if not isinstance(mesh, ExtractedMesh):
        raise err("%s: expected an ExtractedMesh (ops.extract_mesh), got %s" % (what, type(mesh).__name__))
    if not torch.is_tensor(vol) or vol.dtype not in (torch.float32, torch.uint8):
        raise err("%s: expected vol as a float32 or uint8 tensor [B,S,S,S,1], got %s"
                  % (what, vol.dtype if torch.is_tensor(vol) else type(vol).__name__))
    if not vol.is_cuda:
        raise err("%s: vol is on %s; there is no CPU path" % (what, vol.device))
    vol, B, S = _occupancy(what, vol, GRID_SIDES)
    if B > 65535:
        raise err("%s: B=%d (at most 65535 per call)" % (what, B))
    threshold = _finite(what, "threshold", threshold, "number")
    q, faces, vo, fo = mesh.q, mesh.faces, mesh.vert_offsets, mesh.face_offsets
    dev = vol.device
    if not all(torch.is_tensor(t) and t.device == dev for t in (q, faces, vo, fo)):
        raise err("%s: the mesh and the grids must be tensors on one device (%s)" % (what, dev))
    if q.dtype is not torch.int32 or q.dim() != 2 or q.shape[1] != 3 or faces.dtype is not torch.int32 or faces.dim() != 2 \
            or faces.shape[1] not in (3, 4):
        raise err("%s: expected q int32 [V,3] and faces int32 [F,3] or [F,4], got %s %s and %s %s"
                  % (what, q.dtype, tuple(q.shape), faces.dtype, tuple(faces.shape)))
    if vo.dtype is not torch.int64 or fo.dtype is not torch.int64 or tuple(vo.shape) != (B + 1,) or tuple(fo.shape) != (B + 1,):
        raise err("%s: offsets %s %s and %s %s for %d grids (int64 [%d] each)"
                  % (what, vo.dtype, tuple(vo.shape), fo.dtype, tuple(fo.shape), B, B + 1))
    V, F, width = int(q.shape[0]), int(faces.shape[0]), int(faces.shape[1])
    if V > RASTER_MAX_ROWS or F > RASTER_MAX_ROWS or (F and not B):
        raise err("%s: %d vertices and %d faces of %d grids (at most 2^28 each, none without a grid)" % (what, V, F, B))
    out = torch.empty((F,), dtype=torch.int32, device=dev)
    if F and B:
        q, faces, vo, fo, vol = q.contiguous(), faces.contiguous(), vo.contiguous(), fo.contiguous(), vol.detach().contiguous()
        with torch.cuda.device(dev):
            L.check(L.lib().rn_mesh_face_voxels(_vp(q) if V else None, V, _vp(vo), _vp(faces), F, width, _vp(fo), _vp(vol),
                                                1 if vol.dtype is torch.uint8 else 0, threshold, _vp(out), B, S, L.stream_ptr()),
                    "rn_mesh_face_voxels")
    return out


def mesh_face_colours(mesh, vol, colours, known=None, threshold=0.5, unseen=(128, 128, 128)):
    """The colour of every face of a surface net: that of the voxel `mesh_face_voxels` names, from colours uint8 [B,S,S,S,3]
    (and known uint8 [B,S,S,S]) as `voxel_colours` returns them for the grids `vol` the mesh was extracted from -> uint8 [F,3],
    `unseen` where the face names no voxel or `known` is 0 there.  On the blocky mesh this is the colour `raycast_colour` shows
    through that voxel side.  A torch gather on top of the ids.  No autograd."""
    what = "mesh_face_colours"
    colours, known, B, S = _colour_grids(what, colours, known)
    unseen = _colour_bytes(what, "unseen", unseen)
    if torch.is_tensor(vol) and (tuple(_grid_view(vol).shape) != (B, S, S, S) or vol.device != colours.device):
        raise L.RenderNetHipError("%s: colours %s on %s for grids %s on %s"
                                  % (what, tuple(colours.shape), colours.device, tuple(vol.shape), vol.device))
    ids = mesh_face_voxels(mesh, vol, threshold)
    F, dev = int(ids.shape[0]), ids.device
    if F == 0:
        return torch.empty((0, 3), dtype=torch.uint8, device=dev)
    with torch.no_grad():
        fo = mesh.face_offsets
        grid = torch.searchsorted(fo[1:].contiguous(), torch.arange(F, dtype=torch.int64, device=dev), right=True).clamp_(max=B - 1)
        flat = grid * S ** 3 + ids.clamp(min=0).long()
        seen = ids >= 0
        if known is not None:
            seen = seen & (known.reshape(-1)[flat] != 0)
        fill = torch.tensor(unseen, dtype=torch.uint8, device=dev)
        return torch.where(seen[:, None], colours.reshape(-1, 3)[flat], fill[None]).contiguous()


def _mesh_colour_args(what, vertex_colours, face_colours, background):
    """The checks of the colour arguments that need no mesh: (the one given, per_face, background).  Shapes come later."""
    err = L.RenderNetHipError
    if (vertex_colours is None) == (face_colours is None):
        raise err("%s: exactly one of vertex_colours and face_colours" % what)
    per_face = face_colours is not None
    c, name = (face_colours, "face_colours") if per_face else (vertex_colours, "vertex_colours")
    if not torch.is_tensor(c) or c.dtype is not torch.uint8 or c.dim() != 2 or c.shape[1] != 3:
        raise err("%s: expected %s as a uint8 tensor [n,3], got %s"
                  % (what, name, "%s %s" % (c.dtype, tuple(c.shape)) if torch.is_tensor(c) else type(c).__name__))
    if not c.is_cuda:
        raise err("%s: %s is on %s; there is no CPU path" % (what, name, c.device))
    return c, per_face, _colour_bytes(what, "background", background)


def _mesh_colour_rows(what, c, per_face, V, T, dev):
    """A colour per vertex of q, or per triangle of tris, on the mesh's device."""
    n, name, of = (T, "face_colours", "triangles (a quad drawn through its fan has two)") if per_face else (V, "vertex_colours", "vertices")
    if int(c.shape[0]) != n or c.device != dev:
        raise L.RenderNetHipError("%s: %s %s on %s for %d %s on %s" % (what, name, tuple(c.shape), c.device, n, of, dev))


def _mesh_colour_resolve(tri_id, setup, S, view_from_low_x, c, per_face, background):
    """The one rn_mesh_colour_from_ids call, on what `_rasterize_mesh` set up (or `mesh_colour_from_ids` checked)."""
    q, tris, vo, to, M, mesh_of_item, cam, N, f, (row0, col0, ph, pw) = setup
    B, V, T, dev = int(cam.shape[0]), int(q.shape[0]), int(tris.shape[0]), q.device
    out = torch.empty((B, ph, pw, 3), dtype=torch.uint8, device=dev)
    if B:
        # exactly one colour pointer is non-NULL; of an empty array the entry never reads a byte, so any address will do
        c = c.contiguous() if int(c.shape[0]) else torch.zeros((1, 3), dtype=torch.uint8, device=dev)
        with torch.cuda.device(dev):
            L.check(L.lib().rn_mesh_colour_from_ids(
                _vp(q) if V else None, V, _vp(tris) if T else None, T, _vp(vo), _vp(to), M, _vp(mesh_of_item), _vp(cam),
                _vp(tri_id), None if per_face else _vp(c), _vp(c) if per_face else None, _vp(out), B, int(S), N, f, row0, col0,
                ph, pw, 1 if view_from_low_x else 0, background[0], background[1], background[2], L.stream_ptr()),
                "rn_mesh_colour_from_ids")
    return out


def mesh_colour_from_ids(tri_id, q, tris, pose_or_m_inv, S, new_size=128, pixels_per_cell=4, window=None, affine=False,
                         view_from_low_x=False, vert_offsets=None, tri_offsets=None, mesh_of_item=None, vertex_colours=None,
                         face_colours=None, background=(0, 0, 0)):
    """The colour picture of triangle meshes on given triangle ids (rn_mesh_camera + rn_mesh_colour_from_ids;
    include/rendernet_hip.h states the rule): tri_id int32 [B,ph,pw] as `rasterize_mesh(..., return_ids=True)` returned it for
    the same mesh set, poses, window and ray end, and the set and geometry arguments as `rasterize_mesh` takes them -> uint8
    [B,ph,pw,3].  Exactly one of `vertex_colours` uint8 [V,3] (a row per row of q: interpolated over the triangle with the
    rasteriser's own integer edge functions, rounded half up) and `face_colours` uint8 [T,3] (a row per row of tris: flat).  A
    quad-faced `ExtractedMesh` is drawn through its fan, two triangles per quad in order, so the colours of its quads go in as
    `face_colours.repeat_interleave(2, 0)`.  A pixel whose id is negative or not a triangle of the item's mesh gets
    `background`; any int32 content is safe.  Everything is checked before anything is launched.  No autograd."""
    what, err = "mesh_colour_from_ids", L.RenderNetHipError
    c, per_face, background = _mesh_colour_args(what, vertex_colours, face_colours, background)
    q, tris, vo, to, M, host_to = _mesh_set_args(what, q, tris, S, vert_offsets, tri_offsets)
    m, B, N, f = _raster_camera_args(what, pose_or_m_inv, S, new_size, pixels_per_cell, affine)
    V, T, dev = int(q.shape[0]), int(tris.shape[0]), q.device
    if m.device != dev:
        raise err("%s: the mesh is on %s and the poses on %s" % (what, dev, m.device))
    if V > RASTER_MAX_ROWS or T > RASTER_MAX_ROWS:
        raise err("%s: %d vertices and %d triangles (at most 2^28 each)" % (what, V, T))
    _, _, row0, col0, ph, pw = _frame_window(what, window, N, f)
    if not torch.is_tensor(tri_id) or tri_id.dtype is not torch.int32 or tuple(tri_id.shape) != (B, ph, pw) or tri_id.device != dev:
        raise err("%s: expected tri_id int32 [%d,%d,%d] on %s, got %s"
                  % (what, B, ph, pw, dev, "%s %s on %s" % (tri_id.dtype, tuple(tri_id.shape), tri_id.device)
                     if torch.is_tensor(tri_id) else type(tri_id).__name__))
    _mesh_colour_rows(what, c, per_face, V, T, dev)
    if mesh_of_item is None:
        if M != 1:
            raise err("%s: %d meshes need mesh_of_item [B]" % (what, M))
        mesh_of_item = torch.zeros((B,), dtype=torch.int32, device=dev)
    if not torch.is_tensor(mesh_of_item) or mesh_of_item.dtype is not torch.int32 or tuple(mesh_of_item.shape) != (B,):
        raise err("%s: mesh_of_item must be an int32 tensor [%d]" % (what, B))
    _chk_dev(mesh_of_item)
    if host_to is None:
        _check_offsets(what, vo, to, V, T)
    if B and M > 1:
        lo, hi = (int(v) for v in torch.aminmax(mesh_of_item))
        if lo < 0 or hi >= M:
            raise err("%s: mesh_of_item names a mesh outside [0, %d)" % (what, M))
    cam = torch.empty((B, 3, 4), dtype=torch.int64, device=dev)
    if B:
        with torch.cuda.device(dev):
            L.check(L.lib().rn_mesh_camera(L.ptr(m), _vp(cam), B, N, f, 1 if view_from_low_x else 0, L.stream_ptr()), "rn_mesh_camera")
    setup = (q, tris, vo, to, M, mesh_of_item.contiguous(), cam, N, f, (row0, col0, ph, pw))
    return _mesh_colour_resolve(tri_id.contiguous(), setup, S, view_from_low_x, c, per_face, background)


def rasterize_mesh_colour(q, tris, pose_or_m_inv, S, new_size=128, pixels_per_cell=4, window=None, affine=False, smooth=True,
                          cull="back", view_from_low_x=False, vert_offsets=None, tri_offsets=None, mesh_of_item=None,
                          vertex_normals=None, vertex_colours=None, face_colours=None, background=(0, 0, 0),
                          return_normals=False, return_ids=False):
    """The colour picture of triangle meshes under the ray caster's camera: ONE raster pass (rn_mesh_rasterize), then the colour
    resolve on its triangle ids (rn_mesh_colour_from_ids).  The mesh set, geometry, culling and mesh-set arguments are
    `rasterize_mesh`'s, the colour arguments `mesh_colour_from_ids`' -- exactly one of `vertex_colours` uint8 [V,3]
    (interpolated) and `face_colours` uint8 [T,3] (flat, a row per row of tris; for the quads of an `ExtractedMesh` drawn
    through their fan pass `face_colours.repeat_interleave(2, 0)`) -> uint8 [B,ph,pw,3], `background` where nothing is hit.
    return_normals=True also returns the normal map of the same pass, bit-equal to `rasterize_mesh` (`smooth` and
    `vertex_normals` matter only then: without it the pass shades flat and its bytes are dropped); return_ids=True the triangle
    ids and depths.  The result is the picture alone, or a tuple (colour[, normals][, tri_id, depth]).  Every byte is an integer
    function of the input: the same bits on every call.  Everything is checked before anything is launched.  No autograd."""
    what = "rasterize_mesh_colour"
    c, per_face, background = _mesh_colour_args(what, vertex_colours, face_colours, background)
    if not isinstance(return_normals, bool) or not isinstance(smooth, bool):
        raise L.RenderNetHipError("%s: smooth=%r return_normals=%r (True or False)" % (what, smooth, return_normals))
    normals, tri_id, depth, setup = _rasterize_mesh(
        what, q, tris, pose_or_m_inv, S, new_size, pixels_per_cell, window, affine, smooth and return_normals, cull, view_from_low_x,
        vert_offsets, tri_offsets, mesh_of_item, vertex_normals, True,
        before_launch=lambda V, T, B, dev: _mesh_colour_rows(what, c, per_face, V, T, dev))
    out = _mesh_colour_resolve(tri_id, setup, S, view_from_low_x, c, per_face, background)
    res = (out,) + ((normals,) if return_normals else ()) + ((tri_id, depth) if return_ids else ())
    return res if len(res) > 1 else out


# ---- Silhouette pose search: the pose of a grid in a picture (rn_mask_pack, rn_pose_score, rn_pose_best; include/rendernet_hip.h
# ---- states the rule and the hole argument behind the footprint).

POSE_MAX_SIDE = L.RN_POSE_MAX_SIDE                # ph, pw: the splat image lives in LDS
POSE_MAX_FOOTPRINT = L.RN_POSE_MAX_FOOTPRINT
POSE_MAX_CANDIDATES = L.RN_POSE_MAX_CANDIDATES    # P per call; mesh_camera's batch too, so cameras are made in chunks of it


def pose_footprint(pixels_per_voxel):
    """The smallest footprint in 1..4 whose splat of a face-on sheet has no holes at `pixels_per_voxel`: the smallest fp with
    pixels_per_voxel < fp / sqrt 2 (include/rendernet_hip.h has the argument).  Refused when none does."""
    ppv = _finite("pose_footprint", "pixels_per_voxel", pixels_per_voxel, "number")
    for fp in range(1, POSE_MAX_FOOTPRINT + 1):
        if ppv < fp / math.sqrt(2.0):
            return fp
    raise L.RenderNetHipError("pose_footprint: %.3f pixels per voxel is at or above %d / sqrt 2, the largest footprint's bound: "
                              "use a coarser frame" % (ppv, POSE_MAX_FOOTPRINT))


def pose_pixels_per_voxel(cam):
    """Pixels per voxel of integer cameras int64 [...,3,4] for the footprint: the LARGER of |row 0| and |row 1| (the Euclidean
    norm of the three coefficients) over 2^20, float64 [...] -- f * scale for a pose."""
    if not torch.is_tensor(cam) or cam.dtype is not torch.int64 or cam.dim() < 2 or tuple(cam.shape[-2:]) != (3, 4):
        raise L.RenderNetHipError("pose_pixels_per_voxel: expected int64 cameras [...,3,4]")
    a = cam[..., :2, :3].to(torch.float64)
    return torch.sqrt((a * a).sum(-1)).amax(-1) / float(1 << 20)


def _pose_window(what, window, new_size, pixels_per_cell):
    N, f, row0, col0, ph, pw = _frame_window(what, window, new_size, pixels_per_cell)
    if ph > POSE_MAX_SIDE or pw > POSE_MAX_SIDE:
        raise L.RenderNetHipError("%s: a window of %d x %d pixels (at most %d each): use a coarser frame or a window"
                                  % (what, ph, pw, POSE_MAX_SIDE))
    return N, f, row0, col0, ph, pw


def _pose_fp_arg(what, footprint):
    if footprint is None:
        return None
    if isinstance(footprint, (bool, float)) or not isinstance(footprint, (int, np.integer)) or not 1 <= int(footprint) <= POSE_MAX_FOOTPRINT:
        raise L.RenderNetHipError("%s: footprint=%r (None, or an integer 1..%d)" % (what, footprint, POSE_MAX_FOOTPRINT))
    return int(footprint)


def _pose_candidates(what, poses, B, affine):
    """Candidates [P,...] shared by all items or [B,P,...] per item, poses [..,3] or matrices [..,3,4] with affine=True: (the
    tensor flattened over its leading axes, P, whether they are shared), checked before anything is launched."""
    err = L.RenderNetHipError
    if not torch.is_tensor(poses) or not poses.is_floating_point():
        raise err("%s: expected a float tensor for the poses, got %s"
                  % (what, poses.dtype if torch.is_tensor(poses) else type(poses).__name__))
    _chk_dev(poses)
    tail = (3, 4) if affine else (3,)
    lead = poses.dim() - len(tail)
    if lead not in (1, 2) or tuple(poses.shape[lead:]) != tail or (lead == 2 and int(poses.shape[0]) != B):
        raise err("%s: expected %s [P,%s] or [%d,P,%s], got %s" % (what, "matrices" if affine else "poses", ",".join(map(str, tail)), B,
                                                                   ",".join(map(str, tail)), tuple(poses.shape)))
    P = int(poses.shape[lead - 1])
    if not 1 <= P <= POSE_MAX_CANDIDATES:
        raise err("%s: P=%d candidates (1..%d per call)" % (what, P, POSE_MAX_CANDIDATES))
    return poses.detach().reshape((-1,) + tail), P, lead == 1


def _pose_cameras(flat, P, shared, B, S, N, f, affine):
    """int64 [B,P,3,4]: `mesh_camera` of the flattened candidates, in chunks of its batch limit.  The ray end is the default one:
    it changes the depth row only, which the score does not read."""
    n = int(flat.shape[0])
    cam = torch.cat([mesh_camera(flat[i:i + POSE_MAX_CANDIDATES], S, N, f, affine) for i in range(0, n, POSE_MAX_CANDIDATES)]) \
        if n else torch.empty((0, 3, 4), dtype=torch.int64, device=flat.device)
    return (cam.view(1, P, 3, 4).expand(B, P, 3, 4) if shared else cam.view(B, P, 3, 4)).contiguous()


def _pose_masks(what, masks, B, ph, pw, dev):
    """masks uint8 or bool [B,ph,pw] on `dev` -> (mask_bits int32 [B,ph,ceil(pw/32)], n_mask int32 [B]) (rn_mask_pack)."""
    err = L.RenderNetHipError
    if not torch.is_tensor(masks) or masks.dtype not in (torch.uint8, torch.bool):
        raise err("%s: expected masks as a uint8 or bool tensor [B,ph,pw], got %s"
                  % (what, masks.dtype if torch.is_tensor(masks) else type(masks).__name__))
    _chk_dev(masks)
    if tuple(masks.shape) != (B, ph, pw) or masks.device != dev:
        raise err("%s: masks %s on %s for %d grids on %s and a window of %d x %d" % (what, tuple(masks.shape), masks.device, B, dev, ph, pw))
    m = masks.to(torch.uint8).contiguous()
    mask_bits = torch.empty((B, ph, (pw + 31) // 32), dtype=torch.int32, device=dev)
    n_mask = torch.empty((B,), dtype=torch.int32, device=dev)
    if B:
        with torch.cuda.device(dev):
            L.check(L.lib().rn_mask_pack(_vp(m), _vp(mask_bits), _vp(n_mask), B, ph, pw, L.stream_ptr()), "rn_mask_pack")
    return mask_bits, n_mask


class PoseScores(object):
    """What `voxel_pose_scores` returns, on the device.  `scores` int32 [B,P,2] is the table (n_splat, n_inter) of every
    candidate, `n_splat` and `n_inter` int32 [B,P] are views of it; `n_mask` int32 [B]; `best` int64 [B] is the winner's index
    under the exact order (the larger n_inter / union by int64 cross-multiplication, equal scores to the lower index) and
    `best_counts` int32 [B,3] its n_splat, n_inter and n_mask (rn_pose_best: no float argmax is involved); `iou()` is float64
    [B,P], n_inter / (n_splat + n_mask - n_inter), 0 where the union is empty; `footprint` is the fp that was used, `cam` the
    integer cameras int64 [B,P,3,4], and `splats` uint8 [B,P,ph,pw] when they were asked for, otherwise None."""
    __slots__ = ("scores", "n_mask", "best", "best_counts", "footprint", "cam", "splats")

    def __init__(self, scores, n_mask, best, best_counts, footprint, cam, splats):
        self.scores, self.n_mask, self.best, self.best_counts = scores, n_mask, best, best_counts
        self.footprint, self.cam, self.splats = int(footprint), cam, splats

    n_splat = property(lambda self: self.scores[..., 0])
    n_inter = property(lambda self: self.scores[..., 1])

    def iou(self):
        n = self.scores[..., 1].double()
        n_or = self.scores[..., 0].double() + self.n_mask.double()[:, None] - n
        return torch.where(n_or > 0, n / n_or.clamp(min=1.0), torch.zeros_like(n))

    def best_iou(self):
        """float64 [B]: the winner's IoU."""
        c = self.best_counts.double()
        n_or = c[:, 0] + c[:, 2] - c[:, 1]
        return torch.where(n_or > 0, c[:, 1] / n_or.clamp(min=1.0), torch.zeros_like(n_or))


def pose_best(scores, n_mask):
    """The winner of a score table under the exact order (rn_pose_best): scores int32 [B,P,2] of (n_splat, n_inter), n_mask int32
    [B], on the device -> (best int64 [B], best_counts int32 [B,3] = the winner's n_splat, n_inter, and n_mask).  The larger
    n_inter / (n_splat + n_mask - n_inter) by int64 cross-multiplication, an empty union counting as 0 / 1, equal scores to the
    lower index.  What `voxel_pose_scores` calls after the scores."""
    what, err = "pose_best", L.RenderNetHipError
    if not torch.is_tensor(scores) or not torch.is_tensor(n_mask) or scores.dtype is not torch.int32 or n_mask.dtype is not torch.int32 \
            or scores.dim() != 3 or scores.shape[2] != 2 or tuple(n_mask.shape) != (scores.shape[0],):
        raise err("%s: expected scores int32 [B,P,2] and n_mask int32 [B]" % what)
    _chk_dev(scores, n_mask)
    B, P = int(scores.shape[0]), int(scores.shape[1])
    if not 1 <= P <= POSE_MAX_CANDIDATES or B > 65535 or scores.device != n_mask.device:
        raise err("%s: scores %s on %s, n_mask on %s (1 <= P <= %d, B <= 65535, one device)"
                  % (what, tuple(scores.shape), scores.device, n_mask.device, POSE_MAX_CANDIDATES))
    scores, n_mask = scores.contiguous(), n_mask.contiguous()
    best = torch.empty((B,), dtype=torch.int32, device=scores.device)
    counts = torch.empty((B, 3), dtype=torch.int32, device=scores.device)
    if B:
        with torch.cuda.device(scores.device):
            L.check(L.lib().rn_pose_best(_vp(scores), _vp(n_mask), _vp(best), _vp(counts), B, P, L.stream_ptr()), "rn_pose_best")
    return best.long(), counts


def _pose_score(what, masks, vox, poses, new_size, pixels_per_cell, window, footprint, threshold, affine, want_splats):
    """The shared body of `voxel_silhouette` (masks=None: empty masks) and `voxel_pose_scores`."""
    err = L.RenderNetHipError
    if not torch.is_tensor(vox):
        raise err("%s: expected a float32 or uint8 tensor [B,S,S,S,1], got %s" % (what, type(vox).__name__))
    _chk_dev(vox)
    _, B, S = _occupancy(what, vox, GRID_SIDES)
    fp = _pose_fp_arg(what, footprint)
    thr = _finite(what, "threshold", threshold, "number")
    N, f, row0, col0, ph, pw = _pose_window(what, window, new_size, pixels_per_cell)
    flat, P, shared = _pose_candidates(what, poses, B, affine)
    dev = vox.device
    if flat.device != dev:
        raise err("%s: poses on %s for grids on %s" % (what, flat.device, dev))
    if masks is None:
        mask_bits = torch.zeros((B, ph, (pw + 31) // 32), dtype=torch.int32, device=dev)
        n_mask = torch.zeros((B,), dtype=torch.int32, device=dev)
    else:
        mask_bits, n_mask = _pose_masks(what, masks, B, ph, pw, dev)
    with torch.no_grad():
        bits, _, _ = _packed_grids(what, vox, thr)
        cam = _pose_cameras(flat.float().contiguous(), P, shared, B, S, N, f, affine)
        if fp is None:
            fp = pose_footprint(float(pose_pixels_per_voxel(cam).max()) if cam.numel() else 0.0)
        scores = torch.empty((B, P, 2), dtype=torch.int32, device=dev)
        splats = torch.empty((B, P, ph, pw), dtype=torch.uint8, device=dev) if want_splats else None
        if B:
            lib = L.lib()
            ws, nws = _workspace(lib.rn_pose_score_workspace_bytes, dev, B, S)      # the list of each item's occupied words
            with torch.cuda.device(dev):
                L.check(lib.rn_pose_score(_vp(bits), _vp(mask_bits), _vp(cam), _vp(scores), _vp(splats), B, P, S, N, f, row0, col0,
                                          ph, pw, fp, _vp(ws), nws, L.stream_ptr()), "rn_pose_score")
        best, counts = pose_best(scores, n_mask)
    return PoseScores(scores, n_mask, best, counts, fp, cam, splats)


def voxel_silhouette(vox, poses, new_size=128, pixels_per_cell=1, window=None, footprint=None, threshold=0.5, affine=False):
    """The splats of grids under candidate poses (rn_pose_score; include/rendernet_hip.h states the rule): vox [B,S,S,S,1] (or
    [B,S,S,S]) float32 or uint8 as `voxel_pack` takes it, S = 32, 64 or 128; poses [P,3] shared by all items or [B,P,3] per item
    (matrices [..,3,4] with affine=True) -> uint8 [B,P,ph,pw], 1 where a voxel's footprint covers the pixel.  Every occupied
    voxel's centre is projected with `mesh_camera`'s integer camera, as `voxel_carve` projects, and covers footprint x footprint
    pixels about it; footprint=None picks the smallest of 1..4 that leaves a face-on sheet without holes at the call's largest
    camera (`pose_footprint`) and refuses a call that none suits.  The window is at most 256 x 256 pixels; pixels_per_cell
    defaults to 1 here, not 4.  B P ph pw bytes are returned: ask for few candidates at a time.  No autograd."""
    return _pose_score("voxel_silhouette", None, vox, poses, new_size, pixels_per_cell, window, footprint, threshold, affine, True).splats


def voxel_pose_scores(masks, vox, poses, new_size=128, pixels_per_cell=1, window=None, footprint=None, threshold=0.5,
                      affine=False, return_splats=False):
    """Every candidate pose of a grid scored against a silhouette, on the device: masks uint8 or bool [B,ph,pw] (nonzero =
    foreground; for depth views pass `views >= 0`), vox and poses as `voxel_silhouette` takes them -> PoseScores: the integer
    table (n_splat, n_inter) [B,P], n_mask [B], and the winner of every item under the exact order -- the larger IoU
    n_inter / (n_splat + n_mask - n_inter) by int64 cross-multiplication, equal scores to the LOWER INDEX, so the order of the
    candidates (`synth.pose_lattice` states its own) is part of the answer.  The table is a function of the input bits alone:
    two calls give the same bits.  Shapes, dtypes, devices, the window and the options are checked before anything is
    launched.  No autograd."""
    return _pose_score("voxel_pose_scores", masks, vox, poses, new_size, pixels_per_cell, window, footprint, threshold, affine,
                       bool(return_splats))


class PoseEstimate(object):
    """What `voxel_pose_search` returns.  `pose` float32 [B,3] on the device: the winner of the last level; `n_splat`, `n_inter`,
    `n_mask` int32 [B] its three integers and `iou` float64 [B] their quotient; `footprint` the fp every level used; `levels` a
    list with one dict per level: "lattice" (float32 [P,3] for level 0, [B,75,3] after it, on the host), "best" (int64 [B], on
    the host) and "pose" (float32 [B,3], the level's winners, on the host)."""
    __slots__ = ("pose", "n_splat", "n_inter", "n_mask", "iou", "footprint", "levels")

    def __init__(self, pose, counts, iou, footprint, levels):
        self.pose, self.iou, self.footprint, self.levels = pose, iou, int(footprint), levels
        self.n_splat, self.n_inter, self.n_mask = counts[:, 0], counts[:, 1], counts[:, 2]

    def as_dicts(self):
        """One dict per item for JSON output."""
        cols = zip(self.pose.cpu().tolist(), self.iou.cpu().tolist(), self.n_splat.cpu().tolist(), self.n_inter.cpu().tolist(),
                   self.n_mask.cpu().tolist())
        return [{"pose": p, "iou": i, "n_splat": a, "n_inter": b, "n_mask": c, "footprint": self.footprint} for p, i, a, b, c in cols]


def voxel_pose_search(masks, vox, n_azimuth=24, elevations=None, scales=None, refine=2, new_size=128, pixels_per_cell=1,
                      window=None, footprint=None, threshold=0.5):
    """From where was each picture of its grid taken?  A coarse-to-fine search over pose hypotheses, the reference's
    reconstruction search on plain silhouettes: masks and vox as `voxel_pose_scores` takes them -> PoseEstimate.  Level 0
    scores `synth.pose_lattice(n_azimuth, elevations, scales)` (defaults synth.POSE_ELEVATIONS and synth.POSE_SCALES), shared by
    all items; each of the `refine` levels after it halves the three steps and scores the 5 x 5 x 3 neighbourhood of each
    item's winner (`synth.pose_refine_lattice`: azimuth wraps, elevation and scale are clipped to the level-0 range), per item,
    in one call.  Every level's winner is the exact one of `voxel_pose_scores`; a level's centre is its candidate 37, so a level
    that finds nothing better than a LOWER-indexed neighbour of equal score moves there.  footprint=None is chosen once, for the
    level-0 lattice, and kept: the footprint is a constant bias only while it is constant.  No autograd."""
    from . import synth
    what, err = "voxel_pose_search", L.RenderNetHipError
    if isinstance(refine, (bool, float)) or not isinstance(refine, (int, np.integer)) or not 0 <= int(refine) <= 8:
        raise err("%s: refine=%r (an integer, 0..8)" % (what, refine))
    elevations = synth.POSE_ELEVATIONS if elevations is None else elevations
    scales = synth.POSE_SCALES if scales is None else scales
    try:
        lattice = synth.pose_lattice(n_azimuth, elevations, scales)
        steps = synth.pose_lattice_steps(n_azimuth, elevations, scales)
    except ValueError as e:
        raise err("%s: %s" % (what, e))
    elevations, scales = [float(v) for v in elevations], [float(v) for v in scales]
    if not torch.is_tensor(vox):
        raise err("%s: expected a float32 or uint8 tensor [B,S,S,S,1], got %s" % (what, type(vox).__name__))
    _chk_dev(vox)
    dev = vox.device
    kw = dict(new_size=new_size, pixels_per_cell=pixels_per_cell, window=window, threshold=threshold)
    found = _pose_score(what, masks, vox, torch.from_numpy(lattice).to(dev), footprint=footprint, affine=False, want_splats=False, **kw)
    fp, B = found.footprint, int(found.best.shape[0])
    best = found.best.cpu().numpy()
    pose = lattice[best] if B else np.zeros((0, 3), np.float32)
    levels = [{"lattice": lattice, "best": best, "pose": pose}]
    for level in range(1, int(refine) + 1):
        if B == 0:
            break
        cand = np.stack([synth.pose_refine_lattice(pose[b], steps, level, elevations, scales) for b in range(B)])
        found = _pose_score(what, masks, vox, torch.from_numpy(cand).to(dev), footprint=fp, affine=False, want_splats=False, **kw)
        best = found.best.cpu().numpy()
        pose = cand[np.arange(B), best]
        levels.append({"lattice": cand, "best": best, "pose": pose})
    return PoseEstimate(torch.from_numpy(np.ascontiguousarray(pose, np.float32)).to(dev), found.best_counts, found.best_iou(), fp, levels)
