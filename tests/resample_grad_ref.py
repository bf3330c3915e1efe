"""The float64 autograd reference of the resampler gradients and the case table of the tests that use it.  A plain module (no test
in it): tests/test_resample_grad_ref_cpu.py pins the reference and the conditions of the table without a GPU,
tests/test_gpu_resample_grad_edges.py launches the same cases.

The reference restates the OPERATION, not its gradient: the integer tap indices are constants -- floor of the float32 coordinates of
oracle.resample.source_coords(M, N, "ordered"), which are the kernel's bit for bit, clamped to [0, S-1] -- and the eight weights are
float64 functions of M @ (gx, gy, gz, 1).  dvox, dM and (through the float64 matrix chain `pose_to_minv`) dpose all come out of
torch.autograd; no formula of csrc/resample_bwd.hip or of oracle.resample.resampling_affine_bwd is written here.
"""
import math
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from oracle import resample as OR  # noqa: E402

F64 = torch.float64
RTOL_DVOX = 1e-4      # max|got - ref| <= RTOL * max|ref| per batch item, no absolute floor (tests/test_gpu_resample_bwd.py's bars)
RTOL_DM = 2e-4


# ---------------------------------------------------------------------------------------------
# pose -> M_inv in float64 torch

def _mat4(rows):
    return torch.stack([torch.stack([torch.as_tensor(v, dtype=F64) for v in r]) for r in rows])


def pose_to_minv(pose, S, N):
    """[B,3] float64 (azimuth, elevation, scale) -> M_inv [B,3,4]: the chain of oracle.resample.inverse_affine_f64,
    total = T_new_inv @ Sc @ (Rot_Z @ Rot_Y) @ T, inverted factor by factor (a translation by its negative, the rotation by its
    transpose, the scale by its reciprocal), so that it is exact to rounding and differentiable."""
    out = []
    for az, el, s in pose:
        a = az - math.pi * 0.5
        ca, sa, ce, se = torch.cos(a), torch.sin(a), torch.cos(el), torch.sin(el)
        rot_y = _mat4([[ca, 0, -sa, 0], [0, 1, 0, 0], [sa, 0, ca, 0], [0, 0, 0, 1]])
        rot_z = _mat4([[ce, se, 0, 0], [-se, ce, 0, 0], [0, 0, 1, 0], [0, 0, 0, 1]])
        inv_s = 1.0 / s
        sc_inv = _mat4([[inv_s, 0, 0, 0], [0, inv_s, 0, 0], [0, 0, inv_s, 0], [0, 0, 0, 1]])
        t_inv = torch.eye(4, dtype=F64)
        t_inv[:3, 3] = S * 0.5
        tn = torch.eye(4, dtype=F64)
        tn[:3, 3] = -N * 0.5
        out.append((t_inv @ (rot_z @ rot_y).T @ sc_inv @ tn)[:3])
    return torch.stack(out)


def pose_jacobian(pose, S, N):
    """d M_inv[b,r,c] / d pose[b,k] as [B,3,4,3] float64, by autograd over pose_to_minv at the float32 pose cast to double."""
    p = torch.as_tensor(np.asarray(pose, np.float32)).double().requires_grad_(True)
    m = pose_to_minv(p, S, N)
    J = torch.zeros(p.shape[0], 3, 4, 3, dtype=F64)
    for r in range(3):
        for c in range(4):
            J[:, r, c] = torch.autograd.grad(m[:, r, c].sum(), p, retain_graph=True)[0]
    return J.numpy()


def minv_f32(pose, S, N):
    """The float32 matrices the kernels sample with for float32 poses: the float64 chain, rounded once."""
    p = torch.as_tensor(np.asarray(pose, np.float32)).double()
    return pose_to_minv(p, S, N).numpy().astype(np.float32)


# ---------------------------------------------------------------------------------------------
# the operation

def _taps(M32, S, N):
    """Constant tap indices of one item, flat over the raw [z,y,x] output grid: (x0, x1, y0, y1, z0, z1) int64, clamped."""
    xs, ys, zs = OR.source_coords(M32, N, "ordered")
    idx = []
    for v in (xs, ys, zs):
        assert v.dtype == np.float32
        f = np.floor(v).astype(np.int64)
        idx += [np.clip(f, 0, S - 1), np.clip(f + 1, 0, S - 1)]
    return [torch.as_tensor(i) for i in idx]


def to_window(raw, layout, window):
    """raw [N,N,N,C] indexed [z,y,x,c] -> the output the kernel writes for one item: itself, or the image layout (transpose z <-> y,
    reverse the rows) cropped to window = (h0, w0, ph, pw)."""
    if layout == "raw":
        assert window is None
        return raw
    img = raw.permute(1, 0, 2, 3).flip(0)
    if window is not None:
        h0, w0, ph, pw = window
        img = img[h0:h0 + ph, w0:w0 + pw]
    return img


def forward(vox, M, M32, N, layout="raw", window=None, count=None):
    """float64 forward for a batch.  vox [B,S,S,S,C] and M [B,3,4] are float64 tensors (differentiable); M32 [B,3,4] float32 NumPy gives
    the constant tap indices.  Returns the list of per-item outputs; `count`, if a list, receives the active samples inside the
    window per item (no axis clamps both taps onto one index)."""
    B, S, C = vox.shape[0], vox.shape[1], vox.shape[4]
    gx, gy, gz = (torch.as_tensor(g).double() for g in OR.voxel_meshgrid(N, N, N))
    G = torch.stack([gx, gy, gz, torch.ones_like(gx)], 0)                  # [4, N^3]
    outs = []
    for b in range(B):
        x0, x1, y0, y1, z0, z1 = _taps(np.asarray(M32[b], np.float32), S, N)
        x, y, z = M[b] @ G
        flat = vox[b].reshape(-1, C)
        out = 0
        for zz, wz in ((z0, z1 - z), (z1, z - z0)):
            for yy, wy in ((y0, y1 - y), (y1, y - y0)):
                for xx, wx in ((x0, x1 - x), (x1, x - x0)):
                    out = out + (wx * wy * wz)[:, None] * flat[(zz * S + yy) * S + xx]
        outs.append(to_window(out.reshape(N, N, N, C), layout, window))
        if count is not None:
            act = ((x0 != x1) & (y0 != y1) & (z0 != z1)).reshape(N, N, N, 1)
            count.append(int(to_window(act, layout, window).sum()))
    return outs


def gradients(vox, dout, N, M32=None, pose=None, layout="raw", window=None):
    """Reference gradients of L = sum(out * dout).  vox [B,S,S,S,C] and dout (in the kernel's output shape: [B,N,N,N,C] raw, or
    [B,ph,pw,N,C]) are float32 NumPy; give either the float32 matrices M32 [B,3,4] or float32 poses [B,3] (then the taps come from
    minv_f32(pose) and dpose is evaluated at the pose cast to double).  Returns a dict of float64 NumPy arrays: dvox, dM [B,3,4],
    dpose [B,3] or None, active [B] (samples per item), out (the float64 forward)."""
    vox = np.asarray(vox)
    assert vox.dtype == np.float32 and np.asarray(dout).dtype == np.float32
    S = vox.shape[1]
    v = torch.as_tensor(vox).double().requires_grad_(True)
    p = None
    if pose is not None:
        assert M32 is None
        p = torch.as_tensor(np.asarray(pose, np.float32)).double().requires_grad_(True)
        M = pose_to_minv(p, S, N)
        M.retain_grad()
        M32 = M.detach().numpy().astype(np.float32)
    else:
        M32 = np.asarray(M32, np.float32).reshape(-1, 3, 4)
        M = torch.as_tensor(M32).double().requires_grad_(True)
    active = []
    outs = forward(v, M, M32, N, layout, window, active)
    d = torch.as_tensor(np.asarray(dout)).double()
    loss = sum((o * d[b]).sum() for b, o in enumerate(outs))
    loss.backward()
    return {"dvox": v.grad.numpy(), "dM": M.grad.numpy(), "dpose": None if p is None else p.grad.numpy(),
            "active": np.array(active), "out": torch.stack([o.detach() for o in outs]).numpy(), "M32": M32}


def abs_terms(o):
    """For a raw-layout case: sum |w * dout| over the taps that land on each dvox entry, and how many land there ("abs", "count", both
    [B,S,S,S,C]) -- active samples with a non-zero dout only, the ones the kernel adds.  The natural scale of a reordered float32 sum."""
    assert o["layout"] == "raw"
    B, S, N, C = o["B"], o["S"], o["N"], o["C"]
    tot, cnt = np.zeros((B, S * S * S, C)), np.zeros((B, S * S * S, C), np.int64)
    for b in range(B):
        x0, x1, y0, y1, z0, z1 = (t.numpy() for t in _taps(o["M32"][b], S, N))
        x, y, z = (v.astype(np.float64) for v in OR.source_coords(o["M32"][b], N, "ordered"))
        act = (x0 != x1) & (y0 != y1) & (z0 != z1)
        d = np.abs(o["dout"][b].reshape(-1, C).astype(np.float64))
        for zz, wz in ((z0, z1 - z), (z1, z - z0)):
            for yy, wy in ((y0, y1 - y), (y1, y - y0)):
                for xx, wx in ((x0, x1 - x), (x1, x - x0)):
                    i = ((zz * S + yy) * S + xx)[act]
                    np.add.at(tot[b], i, np.abs(wx * wy * wz)[act, None] * d[act])
                    np.add.at(cnt[b], i, (d[act] != 0).astype(np.int64))
    return {"abs": tot.reshape(B, S, S, S, C), "count": cnt.reshape(B, S, S, S, C)}


def raw_dout(dwin, N, layout, window):
    """The kernel-layout output gradient embedded in the raw [B,N,N,N,C] grid (zero outside the window): what
    oracle.resample.resampling_affine_bwd takes."""
    if layout == "raw":
        return dwin
    h0, w0, ph, pw = window or (0, 0, N, N)
    full = np.zeros((dwin.shape[0], N, N, N, dwin.shape[4]), dwin.dtype)
    full[:, h0:h0 + ph, w0:w0 + pw] = dwin
    return np.ascontiguousarray(np.transpose(full[:, ::-1], [0, 2, 1, 3, 4]))


def ratios(got, ref):
    """max|got - ref| / max|ref| per batch item (inf where the reference is all zero but got is not, 0 where both are)."""
    got, ref = np.asarray(got, np.float64), np.asarray(ref, np.float64)
    out = []
    for g, r in zip(got.reshape(len(ref), -1), ref.reshape(len(ref), -1)):
        err, top = np.abs(g - r).max(), np.abs(r).max()
        out.append(err / top if top > 0 else (0.0 if err == 0 else np.inf))
    return np.array(out)


# ---------------------------------------------------------------------------------------------
# the case table

POSES = ((1.0, 0.6, 0.9), (4.0, -0.4, 1.7), (2.5, 0.3, 0.7))      # azimuth, elevation, scale; the third is the zoomed-out item
WINDOW = (5, 4, 7, 5)              # S=8 / N=16: 7*5*16 = 560 samples per item = 3 blocks of 256, the last with 48 live threads
WINDOW_BIG = (2, 5, 30, 27)        # S=16 / N=32: 30*27*32 = 25 920 samples = 101 whole blocks + 64 threads (rows 2..31, columns 5..31)


def _sparse(rng, B, S, C):
    return (rng.random((B, S, S, S, C)) * (rng.random((B, S, S, S, 1)) < 0.4)).astype(np.float32)


def _dense(rng, B, S, C):
    return rng.standard_normal((B, S, S, S, C)).astype(np.float32)


# name -> (S, N, C, B, layout, window, volume, matrix source); the matrix source is a tuple of poses, or a name handled in `case`
_TABLE = {
    "raw_b3": (8, 16, 2, 3, "raw", None, _sparse, POSES),
    "window_b3": (8, 16, 3, 3, "image", WINDOW, _sparse, POSES),
    "window_big": (16, 32, 1, 2, "image", WINDOW_BIG, _sparse, POSES[:2]),
    "lattice": (8, 16, 2, 1, "raw", None, _dense, "lattice"),
    "off_side": (8, 16, 2, 3, "raw", None, _sparse, "off_side"),
    "dense_borders": (8, 16, 4, 2, "image", None, _dense, POSES[:2]),
    "pile_up": (8, 32, 2, 1, "raw", None, _dense, ((1.0, 0.6, 3.0),)),
    "concat_full": (8, 16, 5, 2, "image", None, _dense, POSES[:2]),
    "concat_window": (8, 16, 5, 2, "image", WINDOW, _dense, POSES[:2]),
}
CASES = tuple(_TABLE)
DEGENERATE = ("off_side",)          # no active sample anywhere: every buffer stays at its pre-fill
CONCAT_SPLIT = (1, 4)               # the concat cases: source a has 1 channel, source b has 4


def case(name):
    """The operands of a case: dict(S, N, C, B, layout, window, vox, dout, M32, pose) -- float32 NumPy, deterministic; pose is None
    where the case states its matrix directly."""
    S, N, C, B, layout, window, volume, src = _TABLE[name]
    rng = np.random.default_rng(CASES.index(name) + 100)
    vox = volume(rng, B, S, C)
    if name in ("concat_full", "concat_window"):
        vox[..., 0] = rng.random((B, S, S, S)) < 0.3                    # source a: an occupancy grid, as in the face renderer
    ph, pw = (window[2], window[3]) if window else (N, N)
    dout = rng.standard_normal((B, ph, pw, N, C)).astype(np.float32)
    pose = None
    if src == "lattice":
        M32 = np.zeros((B, 3, 4), np.float32)
        M32[:, :, :3] = np.eye(3)
        M32[:, :, 3] = -S / 2          # every coordinate an integer in [-S/2, N - 1 - S/2]: floor(x) == x, plane S-1 clamps onto itself
    elif src == "off_side":
        M32 = minv_f32(POSES, S, N)
        M32[:, :, 3] += np.float32(90.0)
    else:
        pose = np.array(src, np.float32)
        M32 = minv_f32(pose, S, N)
    if name == "dense_borders":
        dout[..., 2] = 0               # one channel takes the kernel's `d == 0` skip on every sample
    return dict(name=name, S=S, N=N, C=C, B=B, layout=layout, window=window, vox=vox, dout=dout, M32=M32, pose=pose)


def reference(o):
    """gradients() of a case; with poses, the taps come from the same rounded matrices as o["M32"]."""
    if o["pose"] is not None:
        return gradients(o["vox"], o["dout"], o["N"], pose=o["pose"], layout=o["layout"], window=o["window"])
    return gradients(o["vox"], o["dout"], o["N"], M32=o["M32"], layout=o["layout"], window=o["window"])


# poses of the rn_pose_to_affine_bwd test, cycled over the batch: elevation 0, a negative elevation, azimuth exactly float32(pi/2),
# one azimuth per quadrant, scales 0.2 and 3.0
JACOBIAN_POSES = np.array([(1.0, 0.0, 1.0), (2.2, -0.4, 0.9), (np.float32(math.pi / 2), 0.3, 1.1), (0.7, 0.5, 0.2), (2.4, 0.2, 3.0),
                           (3.9, 1.1, 1.3), (5.5, -1.2, 0.8)], np.float32)
JACOBIAN_BATCHES = (1, 64, 65, 130)           # one thread per item in blocks of 64: one block, a full one, a second one, a third
JACOBIAN_SIZES = ((64, 128), (8, 32))


def jacobian_case(B, S, N):
    """pose [B,3], dm [B,12] float32 (N(0,1) times a per-item scale between 1 and 1e3) and the float64 summands
    terms[b,rc,k] = dm[b,rc] * dM_rc/dp_k (translation column included)."""
    rng = np.random.default_rng(B * 1000 + S)
    pose = JACOBIAN_POSES[np.arange(B) % len(JACOBIAN_POSES)].copy()
    dm = (rng.standard_normal((B, 12)) * 10.0 ** rng.uniform(0, 3, (B, 1))).astype(np.float32)
    terms = dm.astype(np.float64).reshape(B, 12, 1) * pose_jacobian(pose, S, N).reshape(B, 12, 3)
    return pose, dm, terms
