"""NumPy twin of rn_mesh_extract_count / rn_mesh_extract_emit (include/rendernet_hip.h states the rule): the surface-net mesh of
a voxel grid on the voxeliser's 1/256-voxel lattice.  Vectorised over the (S + 1)^3 cells, so 128^3 takes seconds.  Order is
part of the contract: vertices in cell flat-index order, quads by (owning cell, axis).  Also the fields the tests share."""
import numpy as np

U = 256
DMAX = 1 << 22


def _levels(vol, threshold):
    """(inside bool, |D| int64) of the samples, float32 operations only."""
    v = np.asarray(vol)
    if v.dtype != np.uint8:
        v = v.astype(np.float32, copy=False)
    v = v.astype(np.float32)
    t = np.float32(threshold)
    with np.errstate(over="ignore"):
        d = np.rint((v - t) * np.float32(65536.0))
    return v > t, np.abs(np.clip(d, -DMAX, DMAX).astype(np.int64))


def extract(vol, threshold=0.5, smooth=True):
    """vol [S,S,S] float32 or uint8 -> (q int32 [V,3], faces int32 [F,4]) of one grid."""
    vol = np.asarray(vol)
    S = vol.shape[0]
    assert vol.shape == (S, S, S)
    N = S + 1
    inside = np.zeros((S + 2,) * 3, bool)                        # padded: index k + 1 is sample k, the border is outside
    inside[1:-1, 1:-1, 1:-1], d_in = _levels(vol, threshold)
    D = np.full((S + 2,) * 3, _levels(np.zeros(1, np.float32), threshold)[1][0], np.int64)
    D[1:-1, 1:-1, 1:-1] = d_in

    def corner(a, bits):                                         # the cells' corner (b0, b1, b2): [N,N,N]
        return a[bits[0]:bits[0] + N, bits[1]:bits[1] + N, bits[2]:bits[2] + N]
    count = sum(corner(inside, (i, j, k)).astype(np.int64) for i in (0, 1) for j in (0, 1) for k in (0, 1))
    active = (count > 0) & (count < 8)
    cells = np.argwhere(active)                                  # row-major: cell flat-index order; c + 1
    p = np.full((len(cells), 3), 128, np.int64)
    if smooth and len(cells):
        sigma, n = np.zeros((N, N, N, 3), np.int64), np.zeros((N, N, N), np.int64)
        for a in range(3):
            u, v = (a + 1) % 3, (a + 2) % 3
            for bu in (0, 1):
                for bv in (0, 1):
                    lo, hi = [0, 0, 0], [0, 0, 0]
                    lo[u] = hi[u] = bu
                    lo[v] = hi[v] = bv
                    hi[a] = 1
                    cross = corner(inside, lo) != corner(inside, hi)
                    da, db = corner(D, lo), corner(D, hi)
                    o = np.where(da + db == 0, 128, (U * da) // np.maximum(da + db, 1))
                    sigma[..., a] += np.where(cross, o, 0)
                    sigma[..., u] += np.where(cross, U * bu, 0)
                    sigma[..., v] += np.where(cross, U * bv, 0)
                    n += cross
        sg, nn = sigma[active], n[active][:, None]
        p = np.clip((2 * sg + nn) // (2 * nn), 1, 255)
    q = np.clip(U * (cells - 1) + 128 + p, 0, U * S).astype(np.int32).reshape(-1, 3)
    vid = np.full((N, N, N), -1, np.int64)
    vid[active] = np.arange(len(cells))
    keys, quads = [], []
    flat = np.arange(N ** 3, dtype=np.int64).reshape(N, N, N)
    for a in range(3):
        u, v = (a + 1) % 3, (a + 2) % 3
        lo, hi = [1, 1, 1], [1, 1, 1]
        lo[a] = 0
        s_in, e_in = corner(inside, lo), corner(inside, hi)
        own = s_in != e_in
        idx = np.arange(N)
        for ax in (u, v):                                        # c_ax + 1 <= S - 1: array index (c + 1) <= S - 1
            shape = [1, 1, 1]
            shape[ax] = N
            own = own & (idx <= S - 1).reshape(shape)
        c = np.argwhere(own)

        def at(du, dv):
            t = c.copy()
            t[:, u] += du
            t[:, v] += dv
            return vid[t[:, 0], t[:, 1], t[:, 2]]
        ring = np.stack([at(0, 0), at(1, 0), at(1, 1), at(0, 1)], 1)
        flip = ~s_in[own]                                        # the normal points from the inside end to the outside end
        ring[flip] = ring[flip][:, [0, 3, 2, 1]]
        keys.append(flat[own] * 3 + a)
        quads.append(ring)
    keys, quads = np.concatenate(keys), np.concatenate(quads)
    faces = quads[np.argsort(keys, kind="stable")].astype(np.int32).reshape(-1, 4)
    assert (faces >= 0).all()
    return q, faces


def fan(faces):
    """Quads [F,4] -> triangles [2F,3], (0,1,2),(0,2,3) per quad, as mesh.load_mesh fans polygons."""
    f = np.asarray(faces).reshape(-1, 4)
    return np.stack([f[:, [0, 1, 2]], f[:, [0, 2, 3]]], 1).reshape(-1, 3)


def extract_batch(vol, threshold=0.5, smooth=True, triangles=False):
    """vol [B,S,S,S] or [B,S,S,S,1] -> (q, faces, vert_offsets int64 [B+1], face_offsets int64 [B+1]), what ops.extract_mesh
    returns; vertex indices are local to their grid."""
    vol = np.asarray(vol)
    if vol.ndim == 5:
        vol = vol[..., 0]
    qs, fs = [np.zeros((0, 3), np.int32)], [np.zeros((0, 3 if triangles else 4), np.int32)]
    for g in vol:
        q, f = extract(g, threshold, smooth)
        qs.append(q)
        fs.append(fan(f).astype(np.int32) if triangles else f)
    vo = np.cumsum([len(a) for a in qs]).astype(np.int64)
    fo = np.cumsum([len(a) for a in fs]).astype(np.int64)
    return np.concatenate(qs), np.concatenate(fs), vo, fo


# ---- fields the tests share ----------------------------------------------------------------------------------------------------

def sphere_field(S, radius=None, centre=None):
    """float32 [S,S,S]: 0.5 on a sphere about an off-centre point, rising inwards."""
    radius = 0.37 * S if radius is None else radius
    c = np.array([0.5 * S - 0.3, 0.5 * S + 0.15, 0.5 * S - 0.45]) if centre is None else np.asarray(centre, np.float64)
    x = np.stack(np.meshgrid(*[np.arange(S, dtype=np.float64)] * 3, indexing="ij"), -1)
    return (0.5 + (radius - np.sqrt(((x - c) ** 2).sum(-1))) / 4.0).astype(np.float32)


def cases32():
    """name -> (vol, threshold): the 32^3 fields of the round-trip and device tests."""
    S = 32
    rng = np.random.RandomState(20261019)
    out = {"sphere": (sphere_field(S), 0.5),
           "uniform_noise": (rng.rand(S, S, S).astype(np.float32), 0.5),
           "binary_u8": ((rng.rand(S, S, S) < 0.4).astype(np.uint8), 0.5),
           "full": (np.ones((S, S, S), np.float32), 0.5)}
    ties = rng.rand(S, S, S).astype(np.float32)
    ties[rng.rand(S, S, S) < 0.3] = np.float32(0.5)              # exactly on the threshold: outside
    out["threshold_ties"] = (ties, 0.5)
    edge = np.zeros((S, S, S), np.float32)
    edge[10, 11, 12] = edge[10, 12, 13] = 1.0                    # two voxels sharing one edge only
    out["edge_contact"] = (edge, 0.5)
    corners = np.zeros((S, S, S), np.float32)
    corners[0, 0, 0] = corners[S - 1, S - 1, S - 1] = 0.9
    out["grid_corners"] = (corners, 0.5)
    return out
