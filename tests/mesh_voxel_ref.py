"""NumPy twin of rn_mesh_voxelize (include/rendernet_hip.h states the rules): the solid (centre parity) and surface (conservative
overlap) grids of a triangle mesh on the 1/256-voxel lattice, in int64 throughout.  One Python loop over the triangles, the
candidates of a triangle vectorised.  Takes the lattice integers, never floats.  Also the meshes the tests share."""
import numpy as np

U = 256
SOLID, SURFACE, BOTH = 1, 2, 3


def _clamped(q, tris, S):
    q = np.clip(np.asarray(q, np.int64), 0, U * S)
    return q[np.asarray(tris, np.int64).reshape(-1, 3)]                       # [T,3 vertices,3 axes]


def solid(q, tris, S):
    """bool [S,S,S]: parity of the crossings of the ray along array axis 2 at every voxel centre."""
    grid = np.zeros((S, S, S), bool)
    depth = np.arange(S, dtype=np.int64)
    for p in _clamped(q, tris, S):
        A = (p[1, 0] - p[0, 0]) * (p[2, 1] - p[0, 1]) - (p[1, 1] - p[0, 1]) * (p[2, 0] - p[0, 0])
        if A == 0:
            continue
        if A < 0:
            p, A = p[[0, 2, 1]], -A
        u, v, w = p[:, 0], p[:, 1], p[:, 2]
        # columns whose centre lies in the projected bounding box, clipped to the grid
        i = np.arange(max(-((128 - u.min()) // U), 0), min((u.max() - 128) // U, S - 1) + 1, dtype=np.int64)
        j = np.arange(max(-((128 - v.min()) // U), 0), min((v.max() - 128) // U, S - 1) + 1, dtype=np.int64)
        if not len(i) or not len(j):
            continue
        cu, cv = np.meshgrid(U * i + 128, U * j + 128, indexing="ij")
        inside = np.ones(cu.shape, bool)
        E = []
        for k in range(3):
            du, dv = u[(k + 1) % 3] - u[k], v[(k + 1) % 3] - v[k]
            e = du * (cv - v[k]) - dv * (cu - u[k])
            owns = dv > 0 or (dv == 0 and du < 0)
            inside &= (e > 0) | ((e == 0) & owns)
            E.append(e)
        N = E[0] * w[2] + E[1] * w[0] + E[2] * w[1]
        k = np.clip((N - 128 * A) // (U * A) + 1, 0, S)                        # // floors towards -inf
        ii, jj = np.nonzero(inside)
        grid[i[ii], j[jj]] ^= depth[None, :] >= k[ii, jj][:, None]
    return grid


def surface(q, tris, S):
    """bool [S,S,S]: every voxel whose closed cube meets a closed triangle."""
    grid = np.zeros((S, S, S), bool)
    for p in _clamped(q, tris, S):
        rng = [np.arange(max(-((-p[:, a].min()) // U) - 1, 0), min(p[:, a].max() // U, S - 1) + 1, dtype=np.int64) for a in range(3)]
        if min(len(r) for r in rng) == 0:
            continue
        x = np.stack(np.meshgrid(*rng, indexing="ij"), -1).reshape(-1, 3)
        qk = p[None, :, :] - (U * x + 128)[:, None, :]                          # [M,3 vertices,3 axes]
        e = np.stack([p[1] - p[0], p[2] - p[1], p[0] - p[2]])
        n = np.cross(e[0], e[1])
        ok = np.abs(qk[:, 0] @ n) <= 128 * np.abs(n).sum()
        for i in range(3):
            for j in range(3):
                a = np.cross(e[i], np.eye(3, dtype=np.int64)[j])
                d = qk @ a                                                      # [M,3]
                r = 128 * np.abs(a).sum()
                ok &= (d.min(1) <= r) & (d.max(1) >= -r)
        x = x[ok]
        grid[x[:, 0], x[:, 1], x[:, 2]] = True
    return grid


def voxelize(q, tris, S, mode=BOTH):
    """uint8 [1,S,S,S,1], what ops.voxelize_mesh returns."""
    grid = np.zeros((S, S, S), bool)
    if mode & SOLID:
        grid |= solid(q, tris, S)
    if mode & SURFACE:
        grid |= surface(q, tris, S)
    return grid.astype(np.uint8)[None, ..., None]


def pack(vox):
    """The mask of rn_voxel_pack: int32 [1, S^3/32], bit (i & 31) of word (i >> 5) = voxel with flat index i."""
    b = np.asarray(vox).reshape(-1, 32).astype(np.uint64)
    return (b << np.arange(32, dtype=np.uint64)).sum(1).astype(np.uint32).view(np.int32)[None]


# ---- meshes on the lattice ---------------------------------------------------------------------------------------------------

def cube(lo, hi):
    """The 12 triangles of the axis-aligned cube [lo, hi]^3, outward orientation."""
    v = np.array([[x, y, z] for x in (lo, hi) for y in (lo, hi) for z in (lo, hi)], np.int32)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return v, np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)


def octahedron(centre, radius):
    c = np.full(3, centre, np.int64)
    v = np.array([c + radius * s * np.eye(3, dtype=np.int64)[a] for a in range(3) for s in (1, -1)], np.int32)
    # vertex 2a is +axis a, 2a+1 is -axis a; the face of the sign triple (sx, sy, sz), outward
    tris = []
    for sx in (0, 1):
        for sy in (0, 1):
            for sz in (0, 1):
                t = (0 + sx, 2 + sy, 4 + sz)
                tris.append(t if (sx + sy + sz) % 2 == 0 else (t[0], t[2], t[1]))
    return v, np.array(tris, np.int32)


def icosahedron():
    """Unit icosahedron: float64 vertices [12,3], triangles [20,3], outward orientation."""
    g = (1 + 5 ** 0.5) / 2
    v = np.array([(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g),
                  (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)], np.float64)
    t = np.array([(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
                  (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
                  (9, 8, 1)], np.int32)
    return v / np.linalg.norm(v[0]), t


def rotation(a, b):
    """Rotation by a about axis 2, then by b about axis 0."""
    ca, sa, cb, sb = np.cos(a), np.sin(a), np.cos(b), np.sin(b)
    return np.array([[1, 0, 0], [0, cb, -sb], [0, sb, cb]]) @ np.array([[ca, -sa, 0], [sa, ca, 0], [0, 0, 1]])


def to_lattice(verts, S, radius, step=4):
    """Unit-sphere float vertices -> lattice int32 about the grid centre, `radius` in voxels, rounded to multiples of `step`."""
    return (np.rint((np.asarray(verts) * radius * U + U * S / 2) / step) * step).astype(np.int32)


def subdivide(v, tris, project=None):
    """Midpoint subdivision: each triangle becomes 4, the orientation kept.  Integer vertices must make integer midpoints (use
    multiples of 4 for two rounds); `project` (float vertices) maps the new vertices, e.g. back onto the unit sphere."""
    v = [tuple(p) for p in np.asarray(v).tolist()]
    index, out = {}, []

    def mid(a, b):
        key = (min(a, b), max(a, b))
        if key not in index:
            s = np.asarray(v[a]) + np.asarray(v[b])
            if project is None:
                assert (s % 2 == 0).all(), "midpoint off the lattice"
                m = s // 2
            else:
                m = project(s / 2.0)
            index[key] = len(v)
            v.append(tuple(m.tolist()))
        return index[key]
    for a, b, c in np.asarray(tris).tolist():
        ab, bc, ca = mid(a, b), mid(b, c), mid(c, a)
        out += [(a, ab, ca), (ab, b, bc), (ca, bc, c), (ab, bc, ca)]
    return np.asarray(v, np.int32 if project is None else np.float64), np.asarray(out, np.int32)


def icosphere(n):
    v, t = icosahedron()
    for _ in range(n):
        v, t = subdivide(v, t, project=lambda p: p / np.linalg.norm(p))
    return v, t


def torus(S, major, minor, nu=24, nv=12, tilt=(0.4, 0.7), step=4):
    """A closed torus about the grid centre (radii in voxels), nu x nv quads split in two, tilted; lattice int32 on multiples of step."""
    a = np.arange(nu) * 2 * np.pi / nu
    b = np.arange(nv) * 2 * np.pi / nv
    A, B = np.meshgrid(a, b, indexing="ij")
    p = np.stack([(major + minor * np.cos(B)) * np.cos(A), (major + minor * np.cos(B)) * np.sin(A), minor * np.sin(B)], -1).reshape(-1, 3)
    p = p @ rotation(*tilt).T
    v = (np.rint((p * U + U * S / 2) / step) * step).astype(np.int32)
    tris = []
    for i in range(nu):
        for j in range(nv):
            k00, k10, k01, k11 = i * nv + j, (i + 1) % nu * nv + j, i * nv + (j + 1) % nv, (i + 1) % nu * nv + (j + 1) % nv
            tris += [(k00, k10, k11), (k00, k11, k01)]
    return v, np.asarray(tris, np.int32)


def plate(S, step=4):
    """A two-sided thin plate: a tilted quad, each of its two triangles once per orientation.  Closed, zero volume."""
    c = U * S // 2
    v = np.array([[c - 2000, c - 1500, c - 700], [c + 2100, c - 1300, c - 100], [c + 1900, c + 1700, c + 900],
                  [c - 2200, c + 1500, c + 300]], np.int64)
    v[3] = v[0] + v[2] - v[1]                                                   # planar: a parallelogram
    v = (v // step * step).astype(np.int32)
    v[3] = v[0] + v[2] - v[1]
    return v, np.array([(0, 1, 2), (0, 2, 3), (0, 2, 1), (0, 3, 2)], np.int32)


def inside_convex(q, tris, S):
    """Independent check for a convex polyhedron with outward faces: (inside bool [S,S,S], on_plane bool [S,S,S]) of the voxel
    centres by the exact integer half-space test."""
    c = U * np.stack(np.meshgrid(*[np.arange(S, dtype=np.int64)] * 3, indexing="ij"), -1) + 128
    inside, on = np.ones((S, S, S), bool), np.zeros((S, S, S), bool)
    for p in np.asarray(q, np.int64)[np.asarray(tris)]:
        d = (c - p[0]) @ np.cross(p[1] - p[0], p[2] - p[1])
        inside &= d < 0
        on |= d == 0
    return inside, on
