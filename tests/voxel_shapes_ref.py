"""NumPy int64 twin of rn_voxel_shapes (include/rendernet_hip.h states the rule): clamps, inside tests and slot order, every
intermediate in int64.  `voxel_shapes` is what the kernel is compared with, voxel for voxel; `track` (a dict) collects the
largest magnitude of each named intermediate so that the header's bounds can be asserted, not just non-overflow.
`inside_exact` evaluates the same formulas on Python integers (unbounded), the yardstick for the twin itself."""
import numpy as np

MAX_PRIMS, NOOP = 8, 255
UNIT = 64 << 14

# the header's bounds: name -> largest magnitude the rule allows
BOUNDS = {"q": 3 * 64 * 127, "wq": (1 << 14) * 3 * 64 * 127, "ellipsoid_sum": 3 * ((1 << 14) * 3 * 64 * 127) ** 2,
          "s": 2 * (3 * 64 * 127) ** 2, "cone_lhs": (1 << 28) * 2 * (3 * 64 * 127) ** 2, "cone_rhs_root": 8192 * (8192 + 3 * 64 * 127),
          "torus_l": 3 * (3 * 64 * 127) ** 2 + 8192 ** 2, "torus_rhs": (1 << 28) * 2 * (3 * 64 * 127) ** 2}


def clamp(prim):
    """One primitive's 16 words -> (type, op, c[3], a[3], R[3,3]) after the kernel's clamps, or None for a no-op slot."""
    w = np.asarray(prim, np.int64).reshape(16)
    t, op = int(w[0] & 255), int(w[0] >> 8)
    if t > 4 or op not in (0, 1):
        return None
    return t, op, np.clip(w[1:4], -64, 64), np.clip(w[4:7], 1, 128), np.clip(w[7:16], -64, 64).reshape(3, 3)


def _note(track, name, v):
    if track is not None:
        track[name] = max(track.get(name, 0), int(np.abs(v).max()))


def inside(t, a, q, track=None):
    """The inside test of type t on local coordinates q = (q0, q1, q2), int64 arrays of one shape."""
    q0, q1, q2 = q
    A, w = 64 * a, (1 << 14) // a
    _note(track, "q", np.stack([q0, q1, q2]))
    if t in (0, 2):
        u = [w[i] * q[i] for i in range(3)]
        _note(track, "wq", np.stack(u[:3 if t == 0 else 2]))
        if t == 0:
            e = u[0] * u[0] + u[1] * u[1] + u[2] * u[2]
            _note(track, "ellipsoid_sum", e)
            return e <= UNIT * UNIT
        return (u[0] * u[0] + u[1] * u[1] <= UNIT * UNIT) & (np.abs(q2) <= A[2])
    if t == 1:
        return (np.abs(q0) <= A[0]) & (np.abs(q1) <= A[1]) & (np.abs(q2) <= A[2])
    s = q0 * q0 + q1 * q1
    _note(track, "s", s)
    if t == 3:
        lhs, root = 4 * A[2] * A[2] * s, A[0] * (A[2] - q2)
        _note(track, "cone_lhs", lhs)
        _note(track, "cone_rhs_root", root)
        return (np.abs(q2) <= A[2]) & (lhs <= root * root)
    l = s + q2 * q2 + A[0] * A[0] - A[1] * A[1]
    rhs = 4 * A[0] * A[0] * s
    _note(track, "torus_l", l)
    _note(track, "torus_rhs", rhs)
    return (l <= 0) | (l * l <= rhs)


def occupancy(item, X, Y, Z, track=None):
    """One item's primitives int [K,16] at the voxel centres (X, Y, Z), int64 arrays of one shape in doubled units -> bool."""
    occ = np.zeros(X.shape, bool)
    for prim in item:
        pr = clamp(prim)
        if pr is None:
            continue
        t, op, c, a, R = pr
        d = (X - c[0], Y - c[1], Z - c[2])
        q = [R[i, 0] * d[0] + R[i, 1] * d[1] + R[i, 2] * d[2] for i in range(3)]
        m = inside(t, a, q, track)
        occ = occ & ~m if op else occ | m
    return occ


def voxel_shapes(prims, S, track=None, stride=1):
    """prims int [B,K,16] -> uint8 [B,S,S,S,1] (stride > 1: only every stride-th voxel of each axis, [B,n,n,n,1])."""
    prims = np.asarray(prims, np.int64)
    B, K = prims.shape[:2]
    assert prims.shape == (B, K, 16) and K <= MAX_PRIMS and S in (32, 64)
    P = (2 * np.arange(S, dtype=np.int64) - (S - 1))[::stride]
    Z, Y, X = np.meshgrid(P, P, P, indexing="ij")                      # flat index (zs*S + ys)*S + xs
    out = np.zeros((B,) + X.shape + (1,), np.uint8)
    for b in range(B):
        out[b, ..., 0] = occupancy(prims[b], X, Y, Z, track)
    return out


def border_occupied(prims, S):
    """prims int [B,K,16] -> bool [B]: is any voxel of the six border layers of the S^3 grid occupied?"""
    prims = np.asarray(prims, np.int64)
    P = 2 * np.arange(S, dtype=np.int64) - (S - 1)
    U, V = np.meshgrid(P, P, indexing="ij")
    out = np.zeros(len(prims), bool)
    for b in range(len(prims)):
        for edge in (np.full_like(U, -(S - 1)), np.full_like(U, S - 1)):
            out[b] |= occupancy(prims[b], edge, U, V).any() | occupancy(prims[b], U, edge, V).any() | \
                occupancy(prims[b], U, V, edge).any()
    return out


def inside_exact(prim, P):
    """Python big integers: is the voxel centre P = (Px, Py, Pz) inside the (clamped) primitive?  None for a no-op slot."""
    w = [int(v) for v in np.asarray(prim).reshape(16)]
    t, op = w[0] & 255, w[0] >> 8
    if t > 4 or op not in (0, 1):
        return None
    c = [min(max(v, -64), 64) for v in w[1:4]]
    a = [min(max(v, 1), 128) for v in w[4:7]]
    R = [min(max(v, -64), 64) for v in w[7:16]]
    q = [sum(R[3 * i + j] * (int(P[j]) - c[j]) for j in range(3)) for i in range(3)]
    A, wt = [64 * v for v in a], [(1 << 14) // v for v in a]
    if t == 0:
        return sum((wt[i] * q[i]) ** 2 for i in range(3)) <= UNIT ** 2
    if t == 1:
        return all(abs(q[i]) <= A[i] for i in range(3))
    if t == 2:
        return (wt[0] * q[0]) ** 2 + (wt[1] * q[1]) ** 2 <= UNIT ** 2 and abs(q[2]) <= A[2]
    s = q[0] ** 2 + q[1] ** 2
    if t == 3:
        return abs(q[2]) <= A[2] and 4 * A[2] ** 2 * s <= (A[0] * (A[2] - q[2])) ** 2
    l = s + q[2] ** 2 + A[0] ** 2 - A[1] ** 2
    return l <= 0 or l ** 2 <= 4 * A[0] ** 2 * s


def voxel_shapes_exact(prims, S, stride):
    """`voxel_shapes(prims, S, stride=stride)` on Python integers, voxel by voxel."""
    prims = np.asarray(prims)
    B, K = prims.shape[:2]
    P = [2 * k - (S - 1) for k in range(0, S, stride)]
    n = len(P)
    out = np.zeros((B, n, n, n, 1), np.uint8)
    for b in range(B):
        for iz, pz in enumerate(P):
            for iy, py in enumerate(P):
                for ix, px in enumerate(P):
                    occ = False
                    for k in range(K):
                        m = inside_exact(prims[b, k], (px, py, pz))
                        if m is None:
                            continue
                        op = (int(prims[b, k, 0]) >> 8)
                        occ = (occ and not m) if op else (occ or m)
                    out[b, iz, iy, ix, 0] = occ
    return out


def make_prim(t, op=0, c=(0, 0, 0), a=(16, 16, 16), R=None):
    """16 words from the parts; R defaults to 64 I."""
    R = 64 * np.eye(3, dtype=np.int64) if R is None else np.asarray(R, np.int64)
    return np.concatenate([[t | op << 8], c, a, R.reshape(-1)]).astype(np.int32)
