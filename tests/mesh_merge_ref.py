"""NumPy twin of rn_mesh_merge_count / rn_mesh_merge_emit (include/rendernet_hip.h states the rule): the exposed voxel faces of a
grid merged into rectangles, run by run.  Vectorised over every plane, side and row of an axis at once -- run descriptors come
from `maximum.accumulate`, a run continues when its descriptor equals the one in the row above -- so a sparse 128^3 grid takes
seconds.  Order is part of the contract: quads by (a, k, side, u0, v0), vertices by flat corner index.  Also the fields the
tests share beyond mesh_extract_ref.cases32()."""
import numpy as np

from mesh_extract_ref import cases32, fan, sphere_field          # noqa: F401  (the tests take them from here)

U = 256


def merge(vol, threshold=0.5, labels=None):
    """vol [S,S,S] float32 or uint8, labels int32 [S,S,S] or None -> (q int32 [V,3], faces int32 [F,4], face_voxel int32 [F],
    face_dir int32 [F], face_size int32 [F,2]) of one grid."""
    vol = np.asarray(vol)
    S = vol.shape[0]
    assert vol.shape == (S, S, S)
    N = S + 1
    inside = vol.astype(np.float32) > np.float32(threshold)
    lab = np.zeros((S, S, S), np.int64) if labels is None else np.asarray(labels).astype(np.int64)
    assert lab.shape == (S, S, S)
    quads = []                                                   # per axis, already in (k, side, u0, v0) order
    for a in range(3):
        u, v = (a + 1) % 3, (a + 2) % 3
        ins = np.zeros((S + 2, S, S), bool)                      # axes (a, u, v); index k + 1 on a is sample k
        ins[1:-1] = inside.transpose(a, u, v)
        key_of = np.zeros((S + 2, S, S), np.int64)
        key_of[1:-1] = lab.transpose(a, u, v)
        lo, hi = ins[:-1], ins[1:]                               # plane k: samples k - 1 and k
        mask = np.stack([lo & ~hi, hi & ~lo], 1)                 # [k, side, u, v]
        key = np.stack([key_of[:-1], key_of[1:]], 1)             # the inside voxel's label
        same = mask[..., 1:] & mask[..., :-1] & (key[..., 1:] == key[..., :-1])          # v joins v - 1
        first = mask.copy()
        first[..., 1:] &= ~same                                  # the face at v starts a run
        last = mask.copy()
        last[..., :-1] &= ~same                                  # ... ends one
        vv = np.arange(S, dtype=np.int64)
        v1 = np.flip(np.minimum.accumulate(np.flip(np.where(last, vv + 1, S + 1), -1), axis=-1), -1)
        cont = np.zeros_like(first)                              # at a run's first face: the row above holds the identical run
        cont[:, :, 1:] = (first[:, :, 1:] & first[:, :, :-1] & (v1[:, :, 1:] == v1[:, :, :-1]) &
                          (key[:, :, 1:] == key[:, :, :-1]))
        height = np.zeros(first.shape, np.int64)
        below = np.zeros(first[:, :, 0].shape, np.int64)
        for r in range(S - 1, -1, -1):                           # rows upwards: 1 + the rows below that continue
            below = np.where(first[:, :, r], 1 + np.where(cont[:, :, r + 1], below, 0) if r + 1 < S else 1, 0)
            height[:, :, r] = below
        at = np.argwhere(first & ~cont)                          # row-major: (k, side, u0, v0)
        k, side, u0, c0 = at.T
        quads.append((np.full(len(at), a), k, side, u0, c0, u0 + height[k, side, u0, c0], v1[k, side, u0, c0]))
    a, k, side, u0, v0, u1, v1 = (np.concatenate(c) for c in zip(*quads))
    u, v = (a + 1) % 3, (a + 2) % 3
    F = len(a)
    rows = np.arange(F)

    def corner(cu, cv):                                          # flat corner index
        p = np.zeros((F, 3), np.int64)
        p[rows, a], p[rows, u], p[rows, v] = k, cu, cv
        return (p[:, 0] * N + p[:, 1]) * N + p[:, 2]
    ring = np.stack([corner(u0, v0), corner(u1, v0), corner(u1, v1), corner(u0, v1)], 1)
    flip = side == 1
    ring[flip] = ring[flip][:, [0, 3, 2, 1]]
    used = np.zeros(N ** 3, bool)
    used[ring.reshape(-1)] = True
    ids = np.cumsum(used) - 1
    flat = np.flatnonzero(used)
    q = (U * np.stack([flat // (N * N), flat // N % N, flat % N], 1)).astype(np.int32).reshape(-1, 3)
    s = np.zeros((F, 3), np.int64)
    s[rows, a], s[rows, u], s[rows, v] = k - 1 + side, u0, v0
    face_voxel = ((s[:, 0] * S + s[:, 1]) * S + s[:, 2]).astype(np.int32)
    return (q, ids[ring].astype(np.int32).reshape(-1, 4), face_voxel, (2 * a + side).astype(np.int32),
            np.stack([u1 - u0, v1 - v0], 1).astype(np.int32).reshape(-1, 2))


def merge_batch(vol, threshold=0.5, labels=None, triangles=False):
    """vol [B,S,S,S] or [B,S,S,S,1] -> (q, faces, vert_offsets int64 [B+1], face_offsets int64 [B+1], face_voxel, face_dir,
    face_size), what ops.extract_mesh_merged returns; vertex indices are local to their grid, the per-quad fields stay per quad."""
    vol = np.asarray(vol)
    if vol.ndim == 5:
        vol = vol[..., 0]
    qs, fs = [np.zeros((0, 3), np.int32)], [np.zeros((0, 3 if triangles else 4), np.int32)]
    fv, fd, fz = [np.zeros(0, np.int32)], [np.zeros(0, np.int32)], [np.zeros((0, 2), np.int32)]
    for b, g in enumerate(vol):
        q, f, voxel, direction, size = merge(g, threshold, None if labels is None else np.asarray(labels)[b])
        qs.append(q)
        fs.append(fan(f).astype(np.int32) if triangles else f)
        fv.append(voxel)
        fd.append(direction)
        fz.append(size)
    vo = np.cumsum([len(x) for x in qs]).astype(np.int64)
    fo = np.cumsum([len(x) for x in fs]).astype(np.int64)
    return np.concatenate(qs), np.concatenate(fs), vo, fo, np.concatenate(fv), np.concatenate(fd), np.concatenate(fz)


def unshared(q, faces):
    """Four private vertices per quad, what MergedMesh.unshared() gives: (q [4F,3], faces [F,4] = arange)."""
    faces = np.asarray(faces).reshape(-1, 4)
    return np.asarray(q)[faces.reshape(-1)], np.arange(4 * len(faces), dtype=np.int32).reshape(-1, 4)


def blocky_count(vol, threshold=0.5):
    """The number of exposed voxel faces: the quads of the blocky extractor."""
    ins = np.pad(np.asarray(vol).astype(np.float32) > np.float32(threshold), 1)
    return int(sum((np.diff(ins.astype(np.int8), axis=a) != 0).sum() for a in range(3)))


# ---- fields the tests share ----------------------------------------------------------------------------------------------------

def checkerboard(S):
    i = np.indices((S, S, S)).sum(0)
    return (i % 2).astype(np.float32)


def edge_cases(S=32):
    """name -> (vol, threshold): the geometry edges of the rule, each the smallest shape that shows it."""
    out = {}

    def grid():
        return np.zeros((S, S, S), np.float32)
    g = grid()
    g[5, 7, :] = 1.0                                             # a run touching both borders of its row: v0 = 0, v1 = S
    g[9, :, 3:6] = 1.0                                           # a rectangle of full height
    out["row_borders_full_height"] = (g, 0.5)
    g = grid()
    g[0, 3:9, 4:20] = 1.0                                        # faces on plane k = 0
    g[S - 1, 2:5, 1:7] = 1.0                                     # ... and k = S
    g[10:14, 0, 5:9] = g[10:14, S - 1, 5:9] = 1.0
    g[20:22, 6:8, 0] = g[20:22, 6:8, S - 1] = 1.0
    out["border_planes"] = (g, 0.5)
    g = grid()
    g[12, 4, 6:12] = 1.0                                         # two rows with equal v0 and different v1
    g[12, 5, 6:15] = 1.0
    g[12, 6, 8:15] = 1.0                                         # ... and equal v1, different v0
    g[16, 10, 3:9] = g[16, 12, 3:9] = 1.0                        # a run in rows u - 1 and u + 1 but not u
    out["ragged_rows"] = (g, 0.5)
    g = grid()
    g[7, 2:10, 2:10] = 1.0                                       # both sides on one plane: k = 8 has side 0 here ...
    g[8, 12:20, 4:30] = 1.0                                      # ... and side 1 here
    g[8, 5:7, 5:7] = 1.0                                         # a voxel pair across the plane: no face between them
    out["both_sides"] = (g, 0.5)
    return out


def word_cases():
    """name -> (vol uint8, S): a run across the full word at 64^3; at 128^3 (sparse) runs that cross bit 63/64 and runs that do not."""
    g64 = np.zeros((64, 64, 64), np.uint8)
    g64[3, 5:9, :] = 1
    g64[:, 40, 17] = 1
    g64[20:30, :, 60:64] = 1
    g128 = np.zeros((128, 128, 128), np.uint8)
    g128[4, 10:13, 60:70] = 1                                    # crosses bit 63/64
    g128[4, 20:22, 10:30] = 1                                    # low word only
    g128[4, 30:33, 64:90] = 1                                    # high word only, starts on bit 64
    g128[4, 40, 0:64] = 1                                        # ends on bit 63
    g128[9, 50, :] = 1                                           # the whole row
    g128[100:128, 127, 62:66] = 1
    g128[60:70, 60:70, 60:70] = 1
    return {"word64": (g64, 64), "word128": (g128, 128)}
