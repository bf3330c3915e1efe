"""NumPy twin of rn_mesh_camera / rn_mesh_vertex_normals / rn_mesh_rasterize (include/rendernet_hip.h states the rule): the
normal map of ONE triangle mesh under the ray caster's camera.  TEST INFRASTRUCTURE ONLY.  int64 throughout for visibility and
depth -- a loop over the triangles that draw, vectorised over each one's pixel box -- and float64 for the normal bytes, which the
kernel forms in float32 (+-1 byte).  `rasterize` takes the integer camera as an argument: the device tests hand it the `cam` the
device wrote, as the caster's twin takes the device's m_inv; `camera` is the float64 path that a separate test pins it against."""
import numpy as np

U = 256
FIX = 20
CLAMP_XY, CLAMP_Z = 1 << 20, 1 << 17
CLAMP_A, CLAMP_B = float(1 << 40), float(1 << 60)
MISS_KEY = np.iinfo(np.int64).max


def _rows(m_inv, N, f, view_from_low_x):
    """float64 [3,4]: 256 X, 256 Y, 256 D as affine functions (a0, a1, a2, b) of (q0, q1, q2); None for a singular matrix."""
    M = np.eye(4)
    M[:3] = np.asarray(m_inv, np.float32).astype(np.float64).reshape(3, 4)
    try:
        F = np.linalg.inv(M)
    except np.linalg.LinAlgError:
        return None
    rows = []
    for src, sign, scale in ((2, 1.0, float(f)), (1, -1.0, float(f)), (0, 1.0 if view_from_low_x else -1.0, 1.0)):
        Fr = F[src]
        offs = Fr[3] - 0.5 * (Fr[0] + Fr[1] + Fr[2])            # the camera coordinate is (Fr . (q2, q1, q0)) / 256 + offs
        b = offs + 0.5 if sign > 0 else (N - 0.5) - offs
        rows.append([sign * scale * Fr[2], sign * scale * Fr[1], sign * scale * Fr[0], 256.0 * scale * b])
    return np.array(rows, np.float64)


def camera(m_inv, N, f, view_from_low_x=False):
    """cam int64 [3,4] of one item from its float32 m_inv [3,4], by the float64 path."""
    rows = _rows(m_inv, N, f, view_from_low_x)
    if rows is None or not np.isfinite(rows).all():
        return np.zeros((3, 4), np.int64)
    c = np.rint(rows * float(1 << FIX))
    c[:, :3] = np.clip(c[:, :3], -CLAMP_A, CLAMP_A)
    c[:, 3] = np.clip(c[:, 3], -CLAMP_B, CLAMP_B)
    return c.astype(np.int64)


def project_float(m_inv, q, N, f, view_from_low_x=False):
    """float64 [V,3]: (256 X, 256 Y, 256 D) of lattice vertices q [V,3], no rounding anywhere."""
    rows = _rows(m_inv, N, f, view_from_low_x)
    return np.asarray(q, np.float64) @ rows[:, :3].T + rows[:, 3]


def project(cam, q, S):
    """int64 [V,3]: the projected, clamped (X, Y, Z) of lattice vertices q (clamped to [0, 256 S]) under cam [3,4]."""
    cam = np.asarray(cam, np.int64).reshape(3, 4)
    qc = np.clip(np.asarray(q, np.int64).reshape(-1, 3), 0, U * S)
    P = (qc @ cam[:, :3].T + cam[:, 3] + (1 << (FIX - 1))) >> FIX
    P[:, :2] = np.clip(P[:, :2], -CLAMP_XY, CLAMP_XY)
    P[:, 2] = np.clip(P[:, 2], -CLAMP_Z, CLAMP_Z)
    return P


def _corners(q, tris, S):
    q = np.clip(np.asarray(q, np.int64).reshape(-1, 3), 0, U * S)
    tris = np.asarray(tris, np.int64).reshape(-1, 3)
    if len(tris) and len(q):
        tris = np.clip(tris, 0, len(q) - 1)                      # the kernel clamps a stray index into its mesh
    return q, tris


def face_normals(q, tris, S):
    """int64 [T,3]: (p1 - p0) x (p2 - p1) in array-axis order."""
    q, tris = _corners(q, tris, S)
    if len(tris) == 0 or len(q) == 0:
        return np.zeros((len(tris), 3), np.int64)
    p = q[tris]
    return np.cross(p[:, 1] - p[:, 0], p[:, 2] - p[:, 1])


def vertex_normals(q, tris, S):
    """int64 [V,3]: per vertex the sum of the face normals of the triangles that use it (once per corner)."""
    qc, tc = _corners(q, tris, S)
    out = np.zeros((len(qc), 3), np.int64)
    if len(tc) and len(qc):
        n = face_normals(q, tris, S)
        for k in range(3):
            np.add.at(out, tc[:, k], n)
    return out


def encode(n_arr, m_inv, view_from_low_x=False):
    """bytes of normals in array-axis order [n,3] under m_inv [3,4], the caster's encoding."""
    lin = np.asarray(m_inv, np.float32).astype(np.float64).reshape(3, 4)[:, :3]
    c = np.asarray(n_arr, np.float64)[:, ::-1] @ lin             # n_src = (n2, n1, n0); n_j = sum_k M[k][j] n_src_k
    c = c / np.sqrt(np.sum(c * c, 1, keepdims=True))
    comp = np.stack([c[:, 2], c[:, 1], -c[:, 0] if view_from_low_x else c[:, 0]], 1)
    return np.rint(255.0 * (0.5 + 0.5 * comp)).astype(np.uint8)


def rasterize(q, tris, cam, m_inv, S, N, f, window=None, smooth=True, cull="back", view_from_low_x=False):
    """One mesh, one item.  q int [V,3], tris int [T,3], cam int64 [3,4], m_inv float32 [3,4] (for the encoding only).
    Returns (rgb uint8 [ph,pw,3], tri_id int32 [ph,pw], depth int32 [ph,pw], min_dot): min_dot = the smallest dot product of
    the interpolated normal with the visible side's unit face normal over the hit pixels (1.0 when flat or nothing is hit, at
    most 0.0 when the face-normal fallback decided a pixel)."""
    assert cull in ("back", "none")
    if window is None:
        window = (0, 0, f * N, f * N)
    row0, col0, ph, pw = (int(v) for v in window)
    keys = np.full((ph, pw), MISS_KEY, np.int64)
    rgb = np.zeros((ph, pw, 3), np.uint8)
    qc, tc = _corners(q, tris, S)
    T = len(tc)
    if T == 0 or len(qc) == 0:
        return rgb, np.full((ph, pw), -1, np.int32), np.full((ph, pw), -1, np.int32), 1.0
    nf = face_normals(q, tris, S)
    P = project(cam, qc, S)[tc]                                  # [T,3 vertices,(X, Y, Z)]
    A = (P[:, 1, 0] - P[:, 0, 0]) * (P[:, 2, 1] - P[:, 0, 1]) - (P[:, 1, 1] - P[:, 0, 1]) * (P[:, 2, 0] - P[:, 0, 0])
    front = (A > 0) if view_from_low_x else (A < 0)
    draws = (A != 0) & (nf != 0).any(1)
    if cull == "back":
        draws &= front
    order = np.where((A < 0)[:, None], np.array([0, 2, 1]), np.array([0, 1, 2]))          # wound to A > 0
    W = np.take_along_axis(P, order[:, :, None], 1)
    Aw = np.abs(A)
    X, Y, Z = W[..., 0], W[..., 1], W[..., 2]
    c0 = np.maximum(-((128 - X.min(1)) // U), col0)              # ceil((lo - 128) / 256)
    c1 = np.minimum((X.max(1) - 128) // U, col0 + pw - 1)
    r0 = np.maximum(-((128 - Y.min(1)) // U), row0)
    r1 = np.minimum((Y.max(1) - 128) // U, row0 + ph - 1)
    draws &= (c1 >= c0) & (r1 >= r0)

    def edges(t, cu, cv):
        """E [3, ...] and the inside mask at centres (cu, cv); t an index or an array matching cu."""
        E, inside = [], True
        for k in range(3):
            n = (k + 1) % 3
            du, dv = X[t, n] - X[t, k], Y[t, n] - Y[t, k]
            e = du * (cv - Y[t, k]) - dv * (cu - X[t, k])
            owns = (dv > 0) | ((dv == 0) & (du < 0))
            inside = inside & ((e > 0) | ((e == 0) & owns))
            E.append(e)
        return E, inside

    for t in np.nonzero(draws)[0]:
        rr = np.arange(r0[t], r1[t] + 1, dtype=np.int64)[:, None]
        cc = np.arange(c0[t], c1[t] + 1, dtype=np.int64)[None, :]
        E, inside = edges(t, U * cc + 128, U * rr + 128)
        d = (E[0] * Z[t, 2] + E[1] * Z[t, 0] + E[2] * Z[t, 1]) // Aw[t]                   # floor division
        ok = inside & (d >= 0) & (d <= U * N)
        key = np.where(ok, (d << 32) | int(t), MISS_KEY)
        sl = (slice(r0[t] - row0, r1[t] + 1 - row0), slice(c0[t] - col0, c1[t] + 1 - col0))
        keys[sl] = np.minimum(keys[sl], key)

    hit = keys != MISS_KEY
    tri_id = np.where(hit, keys & 0xffffffff, -1).astype(np.int32)
    depth = np.where(hit, keys >> 32, -1).astype(np.int32)
    min_dot = 1.0
    if hit.any():
        pr, pc = np.nonzero(hit)
        t = tri_id[pr, pc].astype(np.int64)
        flip = np.where(front[t], 1.0, -1.0)[:, None]
        face = flip * nf[t].astype(np.float64)
        n = face
        if smooth:
            E, _ = edges(t, U * (pc + col0) + 128, U * (pr + row0) + 128)
            w = np.stack([E[1], E[2], E[0]], 1).astype(np.float64) / Aw[t].astype(np.float64)[:, None]
            vs = vertex_normals(q, tris, S)
            vid = np.take_along_axis(tc[t], order[t], 1)          # [n,3]: the vertex at wound position k
            sums = vs[vid]                                       # [n,3,3]
            zero = (sums == 0).all(2).any(1)
            with np.errstate(invalid="ignore", divide="ignore"):
                vn = sums.astype(np.float64) / np.sqrt((sums.astype(np.float64) ** 2).sum(2, keepdims=True))
                acc = flip * (w[:, :, None] * vn).sum(1)
                cos = (acc * face).sum(1) / np.sqrt((face * face).sum(1))        # acc: a convex sum of unit vectors
            use = ~zero & (cos > 0)
            n = np.where(use[:, None], acc, face)
            if use.any():
                min_dot = float(cos[use].min())
            if (~use).any():
                min_dot = min(min_dot, 0.0)                      # the fallback decided a pixel
        rgb[pr, pc] = encode(n, m_inv, view_from_low_x)
    return rgb, tri_id, depth, min_dot
