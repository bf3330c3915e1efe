"""Integer reference of the cast-shadow stage of the caster (include/rendernet_hip.h, rn_shadow_light /
rn_raycast_shadow_fwd / rn_shadow_encode).  TEST INFRASTRUCTURE ONLY; NumPy.

Visibility and bytes are integer functions of (hit voxels, entry faces, occupancy, the quantised lights), so this twin is not
an approximation of the kernels: it states the same arithmetic in int64 and the kernels must equal it on EVERY pixel.  The
walk is vectorised over the unique (hit voxel, entry face) pairs of one item.  `light_src_float` is the float64 statement
of rn_shadow_light (the device rounds in float32: within +-1 per component)."""
import numpy as np

LIGHT_ONE = 32767                                                          # rn_shadow_encode's light, as rn_lines_encode's
SRC_ONE = 1023                                                             # the largest component of light_src
MISS = 255


def valid_hits(hits, faces, S):
    """bool: a hit as the kernels read it -- 0 <= hit_id < S^3 and a face in 0..5."""
    hits, faces = np.asarray(hits, np.int64), np.asarray(faces, np.int64)
    return (hits >= 0) & (hits < S ** 3) & (faces >= 0) & (faces < 6)


def occupied_box(occ):
    """(lo[3], hi[3]) in (x, y, z) of occ [S,S,S] bool indexed [z,y,x]; an empty grid gives (S, S, S), (-1, -1, -1)."""
    occ = np.asarray(occ).astype(bool)
    S = occ.shape[0]
    if not occ.any():
        return np.full(3, S, np.int64), np.full(3, -1, np.int64)
    z, y, x = np.nonzero(occ)
    return np.array([x.min(), y.min(), z.min()], np.int64), np.array([x.max(), y.max(), z.max()], np.int64)


def walk(occ, v, a, s, D, bias):
    """lit (int64 [n], 0 | 1) for hit voxels v [n,3] (x, y, z), face axes a [n], outward signs s [n] and ONE light
    direction D (three ints, clamped here to +-1023), by rn_raycast_shadow_fwd's rule."""
    occ = np.asarray(occ).astype(bool)
    S = occ.shape[0]
    v, a, s = np.asarray(v, np.int64).reshape(-1, 3), np.asarray(a, np.int64).reshape(-1), np.asarray(s, np.int64).reshape(-1)
    D = np.clip(np.asarray(D, np.int64).reshape(3), -SRC_ONE, SRC_ONE)
    n = len(v)
    lo, hi = occupied_box(occ)
    sg, ad = np.where(D > 0, 1, -1), np.abs(D)
    e = np.zeros((n, 3), np.int64)
    e[np.arange(n), a] = s
    lit = np.zeros(n, np.int64)
    active = s * D[a] > 0                                                  # turned to the light
    u, C = v + e, 2 * v + e
    lit[active] = 1                                                        # the value were the loop's bound ever reached
    for _ in range(3 * S + 3):
        if not active.any():
            break
        outside = ((u < lo) | (u > hi)).any(1)
        active &= ~outside                                                 # they stay lit
        uc = np.clip(u, 0, S - 1)
        blocked = active & occ[uc[:, 2], uc[:, 1], uc[:, 0]] & (np.abs(u - v).max(1) > int(bias))
        lit[blocked] = 0
        active &= ~blocked
        num = np.abs(2 * u + sg - C)
        m = np.full(n, -1, np.int64)
        bn, bd = np.zeros(n, np.int64), np.ones(n, np.int64)
        for k in range(3):
            if ad[k] == 0:
                continue
            better = (m < 0) | (num[:, k] * bd < bn * ad[k])               # strict: the lowest axis wins a tie
            m, bn, bd = np.where(better, k, m), np.where(better, num[:, k], bn), np.where(better, ad[k], bd)
        idx = np.nonzero(active)[0]
        u[idx, m[idx]] += sg[m[idx]]
    return lit


def shadow_lit(occ, hits, faces, D, bias=1):
    """The bytes of rn_raycast_shadow_fwd for one item: occ [S,S,S] bool [z,y,x], hits / faces [ph,pw], D its light_src."""
    occ = np.asarray(occ).astype(bool)
    S = occ.shape[0]
    hits, faces = np.asarray(hits, np.int64), np.asarray(faces, np.int64)
    ok = valid_hits(hits, faces, S)
    out = np.full(hits.shape, MISS, np.uint8)
    if ok.any():
        keys, inv = np.unique(hits[ok] * 8 + faces[ok], return_inverse=True)
        h, f = keys // 8, keys % 8
        v = np.stack([h % S, (h // S) % S, h // (S * S)], -1)
        out[ok] = walk(occ, v, f >> 1, np.where(f & 1, 1, -1), D, bias)[inv].astype(np.uint8)
    return out


def quantise_light(l):
    """rint(32767 l / |l|) as three Python ints."""
    l = np.asarray(l, np.float64).reshape(3)
    return tuple(int(c) for c in np.rint(LIGHT_ONE * l / np.sqrt(np.sum(l * l))))


def camera_vector(light, view_from_low_x=False):
    """(right, up, towards) -> the camera-grid vector (+-towards, up, right)."""
    l = np.asarray(light, np.float64).reshape(3)
    return np.array([-l[2] if view_from_low_x else l[2], l[1], l[0]])


def light_src_float(m_inv, light, view_from_low_x=False):
    """float64 statement of rn_shadow_light for m_inv [B,3,4]: 1023 d / max|d| with d = M_lin w, NOT rounded."""
    d = np.asarray(m_inv, np.float64)[:, :, :3] @ camera_vector(light, view_from_low_x)
    return SRC_ONE * d / np.abs(d).max(1, keepdims=True)


def encode(normals_u8, lit, smooth=0, ambient_byte=26, light_q=(0, 0, LIGHT_ONE)):
    """The bytes of rn_shadow_encode for ONE call's window: normals_u8 [ph,pw,3], lit [ph,pw] -> uint8 [ph,pw]."""
    b = np.asarray(normals_u8).astype(np.int64)
    lit = np.asarray(lit).astype(np.int64)
    ph, pw = lit.shape
    hit = lit <= 1
    r = int(smooth)
    vals = np.zeros((ph + 2 * r, pw + 2 * r), np.int64)
    cnt = np.zeros_like(vals)
    vals[r:r + ph, r:r + pw] = np.where(hit, lit, 0)
    cnt[r:r + ph, r:r + pw] = hit
    total, n = np.zeros((ph, pw), np.int64), np.zeros((ph, pw), np.int64)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            total += vals[dy:dy + ph, dx:dx + pw]
            n += cnt[dy:dy + ph, dx:dx + pw]
    e = np.maximum(sum(int(light_q[k]) * (2 * b[..., k] - 255) for k in range(3)), 0)
    den = LIGHT_ONE * 255 * np.maximum(n, 1)
    byte = np.minimum(255, int(ambient_byte) + ((255 - int(ambient_byte)) * e * total + den // 2) // den)
    return np.where(hit, byte, 0).astype(np.uint8)


def light_src_f32(m_inv, light, view_from_low_x=False):
    """rn_shadow_light operation by operation in float32 NumPy: int64 [B,3]."""
    M = np.asarray(m_inv, np.float32)
    w = camera_vector(light, view_from_low_x).astype(np.float32)
    d = (M[:, :, 0] * w[0] + M[:, :, 1] * w[1]) + M[:, :, 2] * w[2]
    m = np.abs(d).max(1, keepdims=True)
    ok = np.isfinite(d).all(1, keepdims=True) & (m > 0)
    with np.errstate(all="ignore"):
        q = np.rint(np.float32(SRC_ONE) * (d / m))
    return np.where(ok, q, 0).astype(np.int64)


# -- the closed-form scene: a wall on a floor, on any pair of axes ----------------------------------------------------------

def wall_scene(S, h, a=0, sa=1, b=1, sb=1, p0=8, q0=20):
    """occ [S,S,S] bool [z,y,x].  Canonical coordinates (p, q, r): the floor is the layer p = p0, the wall p0+1 .. p0+h at
    q = q0, both over all r.  p runs along axis a (mirrored when sa < 0), q along axis b (mirrored when sb < 0), r along the
    third axis."""
    can = np.zeros((S, S, S), bool)
    can[p0] = True
    can[p0 + 1:p0 + 1 + h, q0] = True
    if sa < 0:
        can = can[::-1]
    if sb < 0:
        can = can[:, ::-1]
    axes = [0, 0, 0]
    axes[a], axes[b], axes[3 - a - b] = 0, 1, 2
    return np.ascontiguousarray(np.transpose(can, axes).transpose(2, 1, 0))          # [x,y,z] -> [z,y,x]


def wall_floor_hits(S, q, r, a=0, sa=1, b=1, sb=1, p0=8):
    """(hit ids, face) of the floor voxels canonical (p0, q[i], r) entered by the floor's upper face."""
    q = np.asarray(q, np.int64)
    xyz = np.zeros((len(q), 3), np.int64)
    xyz[:, a] = p0 if sa > 0 else S - 1 - p0
    xyz[:, b] = q if sb > 0 else S - 1 - q
    xyz[:, 3 - a - b] = r
    return (xyz[:, 2] * S + xyz[:, 1]) * S + xyz[:, 0], 2 * a + (1 if sa > 0 else 0)


def wall_light(Dc, a=0, sa=1, b=1, sb=1):
    """The canonical direction (Dp, Dq, Dr) in (x, y, z)."""
    D = np.zeros(3, np.int64)
    D[a], D[b], D[3 - a - b] = sa * Dc[0], sb * Dc[1], Dc[2]
    return D


def wall_shadowed(Dc, h, q, a=0, b=1, q0=20):
    """bool per floor voxel at canonical q < q0: the ray from its face centre reaches the plane q0 - 1/2 after climbing
    Dp (2 (q0 - q) - 1) / (2 Dq); it meets the wall when that is below h, i.e. Dp (2 (q0 - q) - 1) < 2 h Dq.  On equality the
    ray passes through the wall's upper edge and the lowest AXIS steps first: over the wall (lit) when a < b, into its top
    voxel (shadowed) when b < a.  Holds with bias 0 and while the ray stays inside the occupied box."""
    q = np.asarray(q, np.int64)
    lhs, rhs = int(Dc[0]) * (2 * (q0 - q) - 1), 2 * int(h) * int(Dc[1])
    return (lhs < rhs) | ((lhs == rhs) & (b < a))
