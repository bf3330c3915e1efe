"""NumPy twin of rn_mesh_relax (include/rendernet_hip.h states the rule): the second half of SurfaceNets, Jacobi passes that move
every vertex of an extracted mesh towards the mean of its linked neighbours inside its own cell, on the 1/256 lattice.  `relax`
takes its links from the QUAD RINGS (consecutive ring vertices), the device from the 8 corner bits of each cell, so a device
test also checks the corner rule; `corner_links` is that rule in NumPy, for the CPU tests.  Also the measures the tests and
DESIGN.md 5c share (normal errors on a sphere, degenerate quads)."""
import numpy as np

U = 256


def ring_links(faces, V):
    """Quads [F,4] -> the undirected links [L,2] int64 (i < j, sorted, unique): every pair of consecutive ring vertices."""
    f = np.asarray(faces, np.int64).reshape(-1, 4)
    e = np.concatenate([f[:, [k, (k + 1) % 4]] for k in range(4)]) if len(f) else np.zeros((0, 2), np.int64)
    e = np.sort(e, 1)
    assert (e[:, 0] != e[:, 1]).all() and (len(e) == 0 or (e.min() >= 0 and e.max() < V))
    key = np.unique(e[:, 0] * V + e[:, 1])                       # V^2 < 2^63
    return np.stack([key // max(V, 1), key % max(V, 1)], 1)


def cells(q):
    """The cell of every vertex, c = ((q + 128) >> 8) - 1: smooth, blocky and clipped boundary vertices alike."""
    return ((np.asarray(q, np.int64) + 128) >> 8) - 1


def bounds(q, S):
    """(lo, hi) int64 [V,3]: what a vertex may reach, strictly between the sample planes of its cell and inside the grid."""
    c = cells(q)
    return np.maximum(0, U * c + 129), np.minimum(U * S, U * c + 383)


def relax(q, faces, S, passes, weight=256):
    """q int32 [V,3], faces int32 [F,4] of ONE grid -> q after `passes` Jacobi passes at `weight` / 256; faces are not changed."""
    assert 0 <= passes <= 64 and 1 <= weight <= 256
    q = np.asarray(q)
    V = len(q)
    if V == 0 or passes == 0:
        return q.astype(np.int32).copy()
    links = ring_links(faces, V)
    both = np.concatenate([links, links[:, ::-1]])
    n = np.bincount(both[:, 0], minlength=V).astype(np.int64)[:, None]
    lo, hi = bounds(q, S)
    cur = q.astype(np.int64)
    assert (lo <= cur).all() and (cur <= hi).all()
    for _ in range(passes):
        sigma = np.zeros((V, 3), np.int64)
        np.add.at(sigma, both[:, 0], cur[both[:, 1]])
        num = U * n * cur + weight * (sigma - n * cur) + 128 * n
        assert (num >= 0).all() and (num < 1 << 27).all()
        t = num // np.maximum(U * n, 1)
        cur = np.where(n > 0, np.clip(t, lo, hi), cur)
    return cur.astype(np.int32)


def relax_batch(q, faces, vert_offsets, face_offsets, S, passes, weight=256, triangles=False):
    """The batch form: what ops.extract_mesh(..., relax=passes) returns as q, from what it returns with relax=0.  With
    triangles=True the faces are the fans (0,1,2),(0,2,3) of the quads, which are put together again first."""
    out = np.asarray(q).astype(np.int32).copy()
    for b in range(len(vert_offsets) - 1):
        f = np.asarray(faces)[face_offsets[b]:face_offsets[b + 1]]
        if triangles:
            f = np.concatenate([f[0::2], f[1::2, 2:3]], 1)       # (0,1,2) + (0,2,3) -> (0,1,2,3)
        out[vert_offsets[b]:vert_offsets[b + 1]] = relax(out[vert_offsets[b]:vert_offsets[b + 1]], f, S, passes, weight)
    return out


def corner_links(vol, threshold=0.5):
    """The device's link rule in NumPy: vol [S,S,S] -> links [L,2] int64 in ring_links' form, from the 8 corner bits of each
    cell.  Cell c is linked to c + e_a iff its four corners with s_a = c_a + 1 are neither all inside nor all outside."""
    vol = np.asarray(vol)
    S = vol.shape[0]
    N = S + 1
    inside = np.zeros((S + 2,) * 3, bool)                        # padded: index k + 1 is sample k, the border is outside
    inside[1:-1, 1:-1, 1:-1] = vol.astype(np.float32) > np.float32(threshold)

    def corner(bits):
        return inside[bits[0]:bits[0] + N, bits[1]:bits[1] + N, bits[2]:bits[2] + N].astype(np.int64)
    count = sum(corner((i, j, k)) for i in (0, 1) for j in (0, 1) for k in (0, 1))
    active = (count > 0) & (count < 8)
    vid = np.full((N, N, N), -1, np.int64)
    vid[active] = np.arange(int(active.sum()))                   # cell flat-index order, as the extractor numbers them
    out = []
    for a in range(3):
        u, v = (a + 1) % 3, (a + 2) % 3
        face = 0
        for bu in (0, 1):
            for bv in (0, 1):
                bits = [0, 0, 0]
                bits[a], bits[u], bits[v] = 1, bu, bv
                face = face + corner(bits)
        up = (face > 0) & (face < 4)                             # the link c -> c + e_a
        c = np.argwhere(up)
        d = c.copy()
        d[:, a] += 1
        assert (d[:, a] < N).all()                               # the far corners of the last cell are virtual: never mixed
        i, j = vid[c[:, 0], c[:, 1], c[:, 2]], vid[d[:, 0], d[:, 1], d[:, 2]]
        assert (i >= 0).all() and (j >= 0).all()                 # both cells are active
        out.append(np.stack([i, j], 1))
        # the link c -> c - e_a, from c's corners with s_a = c_a, is the same face seen from the other side: check it is
        face0 = 0
        for bu in (0, 1):
            for bv in (0, 1):
                bits = [0, 0, 0]
                bits[u], bits[v] = bu, bv
                face0 = face0 + corner(bits)
        down = (face0 > 0) & (face0 < 4)
        sl_hi, sl_lo = [slice(None)] * 3, [slice(None)] * 3
        sl_hi[a], sl_lo[a] = slice(1, None), slice(0, -1)
        assert np.array_equal(down[tuple(sl_hi)], up[tuple(sl_lo)])
        first = [slice(None)] * 3
        first[a] = 0
        assert not down[tuple(first)].any()
    e = np.sort(np.concatenate(out), 1)
    V = int(active.sum())
    key = np.unique(e[:, 0] * V + e[:, 1])
    return np.stack([key // max(V, 1), key % max(V, 1)], 1)


# ---- measures ------------------------------------------------------------------------------------------------------------------

def quad_normals(q, faces):
    """float64 [F,3]: the cross product of each quad's diagonals (twice its vector area), not normalised."""
    p = np.asarray(q, np.int64)[np.asarray(faces, np.int64).reshape(-1, 4)]
    return np.cross(p[:, 2] - p[:, 0], p[:, 3] - p[:, 1]).astype(np.float64)


def zero_area_quads(q, faces):
    """How many quads have a fan triangle (0,1,2) or (0,2,3) without area."""
    p = np.asarray(q, np.int64)[np.asarray(faces, np.int64).reshape(-1, 4)]
    n1 = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 1])
    n2 = np.cross(p[:, 2] - p[:, 0], p[:, 3] - p[:, 2])
    return int(((n1 == 0).all(1) | (n2 == 0).all(1)).sum())


def _angles(n, radial):
    cos = (n * radial).sum(1) / (np.linalg.norm(n, axis=1) * np.linalg.norm(radial, axis=1))
    return np.degrees(np.arccos(np.clip(cos, -1.0, 1.0)))


def sphere_normal_errors(q, faces, centre):
    """(quad mean, quad max, vertex mean, vertex max) in degrees: the angle between a normal and the radial direction from
    `centre` (sample coordinates: sample k of the lattice is 256 k + 128).  Quad normal: the cross product of the diagonals, at
    the mean of the four vertices.  Vertex normal: the sum of the face normals of the fan triangles (0,1,2),(0,2,3) that use the
    vertex, each of twice its triangle's area, as ops.mesh_vertex_normals sums them."""
    q, f = np.asarray(q, np.int64), np.asarray(faces, np.int64).reshape(-1, 4)
    pos = q / 256.0 - 0.5 - np.asarray(centre, np.float64)
    qa = _angles(quad_normals(q, f), pos[f].mean(1))
    tris = np.stack([f[:, [0, 1, 2]], f[:, [0, 2, 3]]], 1).reshape(-1, 3)
    p = q[tris]
    tn = np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 1])
    vn = np.zeros((len(q), 3), np.int64)
    for k in range(3):
        np.add.at(vn, tris[:, k], tn)
    va = _angles(vn.astype(np.float64), pos)
    return float(qa.mean()), float(qa.max()), float(va.mean()), float(va.max())
