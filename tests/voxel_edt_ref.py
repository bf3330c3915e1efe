"""NumPy twin of rn_voxel_edt / rn_voxel_shape_metrics (include/rendernet_hip.h states the rule): the exact squared Euclidean
distance transform of an occupancy grid for the four seed sets, and the sixteen integer words of a pair of grids with the
values derived from them.  Separable min-plus passes in int64; the EMPTY rule pads the grid with one empty layer -- the nearest
cell outside the grid is always in that layer -- and crops.  Array axes are [zs, ys, xs]; a grid is a boolean array [S,S,S]."""
import math
import os

import numpy as np

NONE = 1 << 30
WORDS = 16
SEEDS = ("solid", "empty", "surface", "signed")
_INF = 1 << 40
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def occupied(vox, threshold=0.5):
    """The occupancy of rn_voxel_pack: value > threshold, compared in float32 (a byte is converted)."""
    v = np.asarray(vox)
    if v.ndim == 4 and v.shape[-1] == 1:
        v = v[..., 0]
    return v.astype(np.float32) > np.float32(threshold)


def _min_plus(f, axis):
    """g(p) = min over p' of f(p') + (p - p')^2 along `axis`."""
    f = np.moveaxis(f, axis, 0)
    n = f.shape[0]
    g = f.copy()
    for d in range(1, n):
        dd = d * d
        np.minimum(g[d:], f[:-d] + dd, out=g[d:])
        np.minimum(g[:-d], f[d:] + dd, out=g[:-d])
    return np.moveaxis(g, 0, axis)


def transform(seeds):
    """Squared distance of every cell of the boolean array `seeds` to the nearest True cell, int64; _INF-sized where there is none."""
    f = np.where(seeds, 0, _INF).astype(np.int64)
    for axis in (2, 1, 0):
        f = _min_plus(f, axis)
    return f


def surface(occ):
    """Occupied voxels with an empty 6-neighbour, outside counting as empty."""
    p = np.pad(occ, 1)
    inner = p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1] & p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1]
    return occ & ~inner


def _finish(f):
    return np.where(f >= _INF // 2, NONE, f).astype(np.int32)


def edt(occ, seeds="solid"):
    """int32 [S,S,S] of one boolean grid, the output of rn_voxel_edt."""
    occ = np.asarray(occ, bool)
    if seeds == "solid":
        return _finish(transform(occ))
    if seeds == "empty":
        return _finish(transform(~np.pad(occ, 1))[1:-1, 1:-1, 1:-1])
    if seeds == "surface":
        return _finish(transform(surface(occ)))
    if seeds == "signed":
        return edt(occ, "solid") - edt(occ, "empty")
    raise ValueError("seeds=%r" % (seeds,))


def brute(occ, seeds="solid"):
    """The definition itself: the minimum over every seed, for small grids."""
    occ = np.asarray(occ, bool)
    S = occ.shape[0]
    if seeds == "empty":
        p = np.pad(occ, 1)
        q = np.argwhere(~p) - 1
    elif seeds == "surface":
        q = np.argwhere(surface(occ))
    else:
        q = np.argwhere(occ)
    v = np.stack(np.meshgrid(np.arange(S), np.arange(S), np.arange(S), indexing="ij"), -1).reshape(-1, 3)
    out = np.full(len(v), NONE, np.int64)
    todo = np.arange(len(v))
    if seeds == "empty":                                          # an empty voxel is its own seed: only the occupied ones are searched
        out[~occ.ravel()] = 0
        todo = np.flatnonzero(occ.ravel())
    for k in range(0, len(q), 256):
        d = ((v[todo, None, :] - q[None, k:k + 256, :]) ** 2).sum(-1).min(1) if len(todo) else np.zeros(0, np.int64)
        out[todo] = np.minimum(out[todo], d)
    return out.reshape(S, S, S).astype(np.int32)


def q_of(D):
    """floor(256 sqrt(D)) = isqrt(D << 16)."""
    return math.isqrt(int(D) << 16)


def shape_fields(a, b):
    """What the words of a pair are made of, the two transforms done once: (words 0..5, D of dA's voxels to dB, D of dB's to dA);
    the distance lists are None when either surface is empty."""
    a, b = np.asarray(a, bool), np.asarray(b, bool)
    sa, sb = surface(a), surface(b)
    head = [a.sum(), b.sum(), (a & b).sum(), (a | b).sum(), sa.sum(), sb.sum()]
    if not head[4] or not head[5]:
        return head, None, None
    return head, transform(sb)[sa], transform(sa)[sb]


def words_of(fields, tau2=1):
    """The sixteen words from `shape_fields` at one tau2, int64 [16]."""
    head, dab, dba = fields
    w = np.zeros(WORDS, np.int64)
    w[:6] = head
    if dab is not None:
        for k, D in enumerate((dab, dba)):
            w[6 + k] = D.sum()
            w[8 + k] = sum(q_of(d) * int(n) for d, n in zip(*np.unique(D, return_counts=True)))
            w[10 + k] = D.max()
            w[12 + k] = (D <= tau2).sum()
    return w


def shape_words(a, b, tau2=1):
    """The sixteen words of rn_voxel_shape_metrics for boolean grids a (prediction) and b (target), int64 [16]."""
    return words_of(shape_fields(a, b), tau2)


def derived(w):
    """float64 values from one row of words, the formulas of ops.ShapeMetrics."""
    w = [float(v) for v in w]
    nan = float("nan")
    ok = w[4] > 0 and w[5] > 0
    precision = w[12] / w[4] if ok else nan
    recall = w[13] / w[5] if ok else nan
    if ok:
        fscore = 2.0 * precision * recall / (precision + recall) if precision + recall > 0 else 0.0
    else:
        fscore = nan
    return {"iou": w[2] / w[3] if w[3] > 0 else 1.0,
            "dice": 2.0 * w[2] / (w[0] + w[1]) if w[0] + w[1] > 0 else 1.0,
            "chamfer": 0.5 * (w[8] / w[4] + w[9] / w[5]) / 256.0 if ok else nan,
            "chamfer_sq": 0.5 * (w[6] / w[4] + w[7] / w[5]) if ok else nan,
            "hausdorff": math.sqrt(max(w[10], w[11])) if ok else nan,
            "precision": precision, "recall": recall, "fscore": fscore}


def load_binvox(name):
    """binvox/<name>.binvox of the repository as a boolean array [64,64,64]."""
    from rendernet_amd.tools import binvox_rw
    with open(os.path.join(ROOT, "binvox", name + ".binvox"), "rb") as f:
        return np.ascontiguousarray(binvox_rw.read_as_3d_array(f).data).astype(bool)


def pack(occ):
    """The words of rn_voxel_pack for boolean grids [B,S,S,S]: int32 [B, S^3/32]."""
    occ = np.asarray(occ, bool)
    B = occ.shape[0]
    b = occ.reshape(B, -1, 32).astype(np.uint64)
    return (b << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32).view(np.int32)


def hard_cases(S):
    """Boolean [B,S,S,S]: word seams, the eight corners one by one, the centre, full, empty, and an empty item between two
    occupied ones (the last three items)."""
    g = []
    seams = np.zeros((S, S, S), bool)
    seams[::5, ::7, [x for x in (31, 32, 63, 64) if x < S]] = True
    g.append(seams)
    for c in range(8):
        one = np.zeros((S, S, S), bool)
        one[(S - 1) * (c >> 2 & 1), (S - 1) * (c >> 1 & 1), (S - 1) * (c & 1)] = True
        g.append(one)
    centre = np.zeros((S, S, S), bool)
    centre[S // 2, S // 2, S // 2] = True
    g.append(centre)
    g.append(np.ones((S, S, S), bool))
    g.append(np.zeros((S, S, S), bool))
    g.append(centre)
    return np.stack(g)
