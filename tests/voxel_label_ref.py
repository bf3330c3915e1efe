"""NumPy twin of rn_voxel_label / rn_voxel_label_stats / rn_voxel_topology (include/rendernet_hip.h states the rule) and of
ops.voxel_clean: a union-find over the runs along xs, the numbering by ascending minimum flat index, the outside rule of the
empty space, the per-component rows, the cell counts of the cubical complex, the eight topology words, and the clean-up.  Pure
NumPy and Python, no scipy.  Array axes are [zs, ys, xs]; a grid is a boolean array [S,S,S]."""
import os

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MODELS = ("bunny", "chair", "suzanne", "table", "teapot")
WORDS = 8
DUAL = {26: 6, 6: 26}


def load_binvox(name):
    """binvox/<name>.binvox of the repository as a boolean array [64,64,64]."""
    from rendernet_amd.tools import binvox_rw
    with open(os.path.join(ROOT, "binvox", name + ".binvox"), "rb") as f:
        return np.ascontiguousarray(binvox_rw.read_as_3d_array(f).data).astype(bool)


def pack(occ):
    """The words of rn_voxel_pack for boolean grids [B,S,S,S]: int32 [B, S^3/32]."""
    occ = np.asarray(occ, bool)
    b = occ.reshape(occ.shape[0], -1, 32).astype(np.uint64)
    return (b << np.arange(32, dtype=np.uint64)).sum(-1).astype(np.uint32).view(np.int32)


def _offsets(connectivity):
    """The earlier neighbours (dz, dy, dx) of a voxel that are not in its own row."""
    if connectivity == 6:
        return [(0, -1, 0), (-1, 0, 0)]
    if connectivity == 26:
        return [(dz, dy, dx) for dz in (-1, 0) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dz, dy) < (0, 0)]
    raise ValueError("connectivity=%r (6 or 26)" % (connectivity,))


def _run_ids(sel):
    """(run number of every selected voxel, -1 elsewhere; flat index of the first voxel of every run), runs in raster order."""
    S = sel.shape[-1]
    flat = sel.reshape(-1, S)
    starts = flat.copy()
    starts[:, 1:] &= ~flat[:, :-1]
    ids = np.cumsum(starts.ravel()).reshape(flat.shape) - 1
    return np.where(flat, ids, -1).reshape(sel.shape), np.flatnonzero(starts.ravel())


def _components(sel, connectivity):
    """(component root run per run, runs' first flat indices, run number per voxel): the root is the component's first run."""
    runs, first = _run_ids(sel)
    S = sel.shape[0]
    pairs = []
    for dz, dy, dx in _offsets(connectivity):
        a = [slice(max(0, -d), S - max(0, d)) for d in (dz, dy, dx)]          # the voxel
        b = [slice(max(0, d), S - max(0, -d)) for d in (dz, dy, dx)]          # its neighbour at +d
        ra, rb = runs[tuple(a)], runs[tuple(b)]
        both = (ra >= 0) & (rb >= 0)
        if both.any():
            pairs.append(np.unique(ra[both].astype(np.int64) * len(first) + rb[both]))
    parent = list(range(len(first)))

    def find(i):
        r = i
        while parent[r] != r:
            r = parent[r]
        while parent[i] != r:
            parent[i], i = r, parent[i]
        return r

    if pairs:
        for key in np.unique(np.concatenate(pairs)).tolist():
            a, b = find(key // len(first)), find(key % len(first))
            if a != b:
                parent[max(a, b)] = min(a, b)
    return np.array([find(i) for i in range(len(first))], np.int64), first, runs


def label(occ, of="solid", connectivity=26):
    """(labels int32 [S,S,S], K) of one boolean grid: the output of rn_voxel_label for one item."""
    occ = np.asarray(occ, bool)
    if of not in ("solid", "empty"):
        raise ValueError("of=%r (solid or empty)" % (of,))
    sel = occ if of == "solid" else ~occ
    root, first, runs = _components(sel, connectivity)
    out = np.zeros(occ.shape, np.int32)
    if not len(first):
        return out, 0
    outside = np.zeros(len(first), bool)
    if of == "empty":                                             # a component with a voxel on the grid border is the outside
        border = np.ones(occ.shape, bool)
        border[1:-1, 1:-1, 1:-1] = False
        outside[root[np.unique(runs[border & sel])]] = True
    numbered = np.flatnonzero((root == np.arange(len(first))) & ~outside)     # ascending run number = ascending minimum flat index
    number = np.zeros(len(first), np.int32)
    number[numbered] = np.arange(len(numbered)) + (2 if of == "empty" else 1)
    number[outside] = 1
    out[sel] = number[root][runs[sel]]
    return out, len(numbered)


def stats(labels, rows):
    """int32 [rows, 8] of one item's labels: size, minimum flat index, (x_lo, y_lo, z_lo, x_hi, y_hi, z_hi); row k is label k + 1."""
    S = labels.shape[0]
    out = np.tile(np.array([0, S ** 3, S, S, S, -1, -1, -1], np.int32), (rows, 1))
    z, y, x = np.nonzero(labels)
    k = labels[z, y, x] - 1
    flat = (z * S + y) * S + x
    np.add.at(out[:, 0], k, 1)
    np.minimum.at(out[:, 1], k, flat.astype(np.int32))
    for col, v in ((2, x), (3, y), (4, z)):
        np.minimum.at(out[:, col], k, v.astype(np.int32))
        np.maximum.at(out[:, col + 3], k, v.astype(np.int32))
    return out


def components(grids, of="solid", connectivity=26):
    """What ops.voxel_components returns for boolean grids [B,S,S,S]: (labels [B,S,S,S], counts [B], offsets int64 [B+1], stats)."""
    labs, counts, rows = [], [], []
    for g in grids:
        lab, k = label(g, of, connectivity)
        labs.append(lab)
        counts.append(k)
        rows.append(stats(lab, k + (1 if of == "empty" else 0)))
    offsets = np.concatenate([[0], np.cumsum([len(r) for r in rows])]).astype(np.int64)
    return (np.stack(labs) if labs else np.zeros((0,) + np.shape(grids)[1:], np.int32), np.array(counts, np.int32), offsets,
            np.concatenate(rows) if rows else np.zeros((0, 8), np.int32))


def cell_counts(occ):
    """(V, E, F) of the union of the closed unit cubes of the occupied voxels."""
    p = np.pad(np.asarray(occ, bool), 1)
    any2 = lambda a, axis: np.logical_or(a.take(range(a.shape[axis] - 1), axis), a.take(range(1, a.shape[axis]), axis))
    fz, fy, fx = any2(p, 0), any2(p, 1), any2(p, 2)              # faces across an axis: either of the 2 voxels
    faces = fz[:, 1:-1, 1:-1].sum() + fy[1:-1, :, 1:-1].sum() + fx[1:-1, 1:-1, :].sum()
    ex, ey, ez = any2(fz, 1), any2(fz, 2), any2(fy, 2)            # edges along xs: the 4 voxels around it in zs and ys; ...
    edges = ex[:, :, 1:-1].sum() + ey[:, 1:-1, :].sum() + ez[1:-1, :, :].sum()
    return int(any2(ex, 2).sum()), int(edges), int(faces)


def topology(occ):
    """The eight words of rn_voxel_topology for one boolean grid, int64 [8]."""
    occ = np.asarray(occ, bool)
    v, e, f = cell_counts(occ)
    n, k, c = int(occ.sum()), label(occ, "solid", 26)[1], label(occ, "empty", 6)[1]
    euler = v - e + f - n
    return np.array([n, k, c, v, e, f, euler, k + c - euler], np.int64)


def clean(occ, keep_largest=1, min_voxels=1, fill_cavities=True, connectivity=26):
    """ops.voxel_clean of one boolean grid: (the cleaned grid, the sizes of the dropped components in label order)."""
    occ = np.asarray(occ, bool)
    lab, k = label(occ, "solid", connectivity)
    size = np.bincount(lab.ravel(), minlength=k + 1)[1:]
    order = sorted(range(k), key=lambda j: (-size[j], j))         # on equal size the lower label wins
    keep = [j for j in order if size[j] >= min_voxels]
    if keep_largest:
        keep = keep[:keep_largest]
    table = np.zeros(k + 1, bool)
    table[[j + 1 for j in keep]] = True
    out = table[lab]
    if fill_cavities:
        out = out | (label(out, "empty", DUAL[connectivity])[0] >= 2)
    return out, [int(size[j]) for j in range(k) if not table[j + 1]]


# ---- the closed forms of the tests, boolean [S,S,S] ----

def box(S, lo, hi, hollow=False):
    g = np.zeros((S, S, S), bool)
    g[lo:hi, lo:hi, lo:hi] = True
    if hollow:
        g[lo + 1:hi - 1, lo + 1:hi - 1, lo + 1:hi - 1] = False
    return g


def checkerboard(S):
    z, y, x = np.meshgrid(np.arange(S), np.arange(S), np.arange(S), indexing="ij")
    return (x + y + z) % 2 == 0


def nested_shells(S=32):
    return box(S, 4, 20, True) | box(S, 8, 16, True) | box(S, 11, 13)


def cube_edges(S=32, lo=3, hi=28):
    """The 12 edges of the cube lo..hi (inclusive)."""
    g = np.zeros((S, S, S), bool)
    ends = (lo, hi)
    for a in ends:
        for b in ends:
            g[a, b, lo:hi + 1] = g[a, lo:hi + 1, b] = g[lo:hi + 1, a, b] = True
    return g


def serpentine(S=32):
    """One path through the rows ys = 0, 2, .. of the planes zs = 0, 2, ..: full rows joined alternately at their ends, the planes
    joined alternately at their last and first row: a union chain through every run."""
    g = np.zeros((S, S, S), bool)
    for pz, z in enumerate(range(0, S, 2)):
        rows = list(range(0, S, 2))
        for py, y in enumerate(rows):
            g[z, y, :] = True
            if y + 2 < S:
                g[z, y + 1, S - 1 if py % 2 == 0 else 0] = True
        if z + 2 < S:
            y_link = rows[-1] if pz % 2 == 0 else rows[0]
            g[z + 1, y_link, 0] = True
    return g


def pair(S, at, step):
    """Two voxels, the second `step` away from `at` = (zs, ys, xs)."""
    g = np.zeros((S, S, S), bool)
    g[at] = True
    g[tuple(np.add(at, step))] = True
    return g


def pitfall(S, z, y, x):
    """A lone voxel at xs = x beside a row holding xs = x - 1 and x + 1 (the row ys = y - 1 of the same plane)."""
    g = np.zeros((S, S, S), bool)
    g[z, y, x] = g[z, y - 1, x - 1] = g[z, y - 1, x + 1] = True
    return g


def random_grids(S=32, densities=(0.05, 0.2, 0.5), seed=0):
    """One grid per density, drawn one after the other from RandomState(seed): at 32^3 and seed 0 they have 800 / 76 / 1 components
    at connectivity 26 and 1451 / 2929 / 362 at 6."""
    rng = np.random.RandomState(seed)
    return [rng.random_sample((S, S, S)) < d for d in densities]


def closed_forms_32():
    """name -> grid: the 32^3 closed forms of the issue, an empty item in the middle."""
    S = 32
    hollow = box(S, 4, 20, True)
    open_corner = hollow.copy()
    open_corner[4, 4, 4] = False
    return [("full", np.ones((S, S, S), bool)), ("corner pair", pair(S, (5, 5, 5), (1, 1, 1))), ("edge pair", pair(S, (5, 5, 5), (0, 1, 1))),
            ("pitfall", pitfall(S, 7, 9, 5)), ("checkerboard", checkerboard(S)), ("empty", np.zeros((S, S, S), bool)),
            ("hollow box", hollow), ("open corner", open_corner), ("nested shells", nested_shells(S)), ("cube edges", cube_edges(S)),
            ("serpentine", serpentine(S))]


def seam_cases(S, seams):
    """Pitfall, corner pair and edge pair across each word seam (xs = s - 1, s, s + 1), on the grid border, on the last row and on
    the last plane, and all of them in one grid."""
    g = []
    for s in seams:
        g += [pitfall(S, 3, 5, s), pair(S, (9, 5, s - 1), (1, 1, 1)), pair(S, (9, 9, s - 1), (0, 1, 1)), pair(S, (9, 13, s), (1, -1, -1))]
    g += [pitfall(S, 0, 1, 1), pitfall(S, S - 1, S - 1, S - 2), pair(S, (S - 2, S - 2, S - 2), (1, 1, 1)), pair(S, (0, 0, 0), (0, 1, 1)),
          pair(S, (S - 1, S - 2, 0), (0, 1, 1)), pair(S, (S - 2, S - 1, S - 1), (1, 0, -1))]
    return g + [np.logical_or.reduce(g)]
