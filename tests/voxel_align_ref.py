"""NumPy twin of rn_voxel_orient / rn_voxel_align (include/rendernet_hip.h states the rule): the 48 signed axis permutations in
the header's numbering, the moved grid, the whole table of n_and over (orientation, shift) and the winner under the tie order.
Transpose, flip, slice and count_nonzero; integers only, so kernel and twin agree on every word."""
import itertools
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SETS = {"none": 1, "rotations": 24, "all": 48}
MAX_SHIFT = 16


def _parity(p):
    return sum(1 for i in range(3) for j in range(i + 1, 3) if p[i] > p[j]) & 1


def _table():
    pairs = [(p, f) for p in itertools.permutations(range(3)) for f in itertools.product((0, 1), repeat=3)]   # lexicographic
    det = lambda p, f: -1 if (_parity(p) + sum(f)) & 1 else 1
    return [pf for pf in pairs if det(*pf) == 1] + [pf for pf in pairs if det(*pf) == -1]


TABLE = _table()                                   # o -> ((pi0, pi1, pi2), (f0, f1, f2))


def matrix(o):
    """The 3 x 3 signed permutation M of orientation o about the centre: j - c = M (i - c), c = (S - 1) / 2."""
    p, f = TABLE[o]
    m = np.zeros((3, 3), np.int64)
    for k in range(3):
        m[p[k], k] = -1 if f[k] else 1
    return m


def orient(a, o):
    """orient_o(A)[i0,i1,i2] = A[j], j[pi(k)] = f_k ? S-1-i_k : i_k."""
    p, f = TABLE[o]
    out = np.transpose(np.asarray(a), p)
    for k in range(3):
        if f[k]:
            out = np.flip(out, k)
    return np.ascontiguousarray(out)


def _windows(S, t):
    """(slices of the destination, slices of the source) of a shift by t = (tz, ty, tx) with nothing wrapping."""
    dst = tuple(slice(max(v, 0), S + min(v, 0)) for v in t)
    src = tuple(slice(max(-v, 0), S - max(v, 0)) for v in t)
    return dst, src


def shift(a, t):
    """A'(p) = A(p - t); what leaves the grid is dropped, what enters is empty."""
    a = np.asarray(a)
    out = np.zeros_like(a)
    dst, src = _windows(a.shape[0], t)
    out[dst] = a[src]
    return out


def transform(a, o, t):
    return shift(orient(a, o), t)


def scores(a, b, R, n_orient):
    """int32 [n_orient, 2R+1, 2R+1, 2R+1]: n_and(o, t) = |shift(orient_o(a), t) & b|."""
    a, b = np.asarray(a, bool), np.asarray(b, bool)
    S, T = a.shape[0], 2 * R + 1
    out = np.zeros((n_orient, T, T, T), np.int32)
    if not b.any():
        return out
    # only b's bounding box is looked at: outside it b is empty and adds nothing to any count
    box = [np.flatnonzero(b.any(axis=tuple(k for k in range(3) if k != axis))) for axis in range(3)]
    lo, hi = [int(v[0]) for v in box], [int(v[-1]) + 1 for v in box]
    for o in range(n_orient):
        ao = orient(a, o)
        for t in itertools.product(range(-R, R + 1), repeat=3):
            d0 = [max(lo[k], t[k], 0) for k in range(3)]
            d1 = [min(hi[k], S + t[k], S) for k in range(3)]
            if any(d0[k] >= d1[k] for k in range(3)):
                continue
            dst = tuple(slice(d0[k], d1[k]) for k in range(3))
            src = tuple(slice(d0[k] - t[k], d1[k] - t[k]) for k in range(3))
            out[(o,) + tuple(v + R for v in t)] = np.count_nonzero(ao[src] & b[dst])
    return out


def candidates(table, R):
    """Every candidate as (-n_and, |t|^2, o, tz, ty, tx): the smallest tuple is the winner."""
    idx = np.indices(table.shape).reshape(4, -1)
    t = idx[1:] - R
    rows = np.stack([-table.reshape(-1).astype(np.int64), (t * t).sum(0), idx[0], t[0], t[1], t[2]], 1)
    return rows


def winner(table, R):
    """(o, (tz, ty, tx), n_and, the number of candidates that reach n_and)."""
    rows = candidates(table, R)
    order = np.lexsort(rows.T[::-1])
    best = rows[order[0]]
    return int(best[2]), tuple(int(v) for v in best[3:]), int(-best[0]), int((rows[:, 0] == best[0]).sum())


def align(a, b, R, orientations="rotations"):
    """(the eight words of out_best, the whole table) for one pair of boolean grids."""
    table = scores(a, b, R, SETS[orientations])
    o, t, n, _ = winner(table, R)
    words = np.array([o, t[0], t[1], t[2], n, np.count_nonzero(a), np.count_nonzero(b), table[0, R, R, R]], np.int32)
    return words, table


def iou(n_and, n_a, n_b):
    n_or = n_a + n_b - n_and
    return n_and / n_or if n_or else 1.0


def load_binvox(name):
    """binvox/<name>.binvox of the repository as a boolean array [64,64,64]."""
    from rendernet_amd.tools import binvox_rw
    with open(os.path.join(ROOT, "binvox", name + ".binvox"), "rb") as f:
        return np.ascontiguousarray(binvox_rw.read_as_3d_array(f).data).astype(bool)


def pool(occ, k):
    """Max-pool a boolean grid by k along every axis."""
    S = occ.shape[0] // k
    return occ.reshape(S, k, S, k, S, k).any(axis=(1, 3, 5))


def centred(occ, S):
    """occ in the middle of an empty S^3 grid."""
    out = np.zeros((S, S, S), bool)
    m = (S - occ.shape[0]) // 2
    out[m:m + occ.shape[0], m:m + occ.shape[1], m:m + occ.shape[2]] = occ
    return out


def pack(occ):
    """The words of rn_voxel_pack for boolean grids [B,S,S,S]: int32 [B, S^3/32]."""
    occ = np.asarray(occ, bool)
    flat = occ.reshape(occ.shape[0], -1, 32).astype(np.uint64)
    return (flat << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32).view(np.int32)
