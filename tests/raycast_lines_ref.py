"""Integer reference of the line-drawing stage of the caster (include/rendernet_hip.h, rn_raycast_edges_fwd /
rn_lines_encode).  TEST INFRASTRUCTURE ONLY; NumPy, vectorised over the pixels of one item.

Both rules are integer functions of (hit voxels, entry faces, occupancy, a quantised light), so this twin is not an
approximation of the kernels: it states the same arithmetic in int64 and the kernels must equal it on EVERY pixel.  The
stencil normal is raycast_ref's (gradient + source_normal), the rule rn_raycast_fwd encodes.  `band_float` is the float64
statement of the band with the light NOT quantised: what the integer band stands for."""
import numpy as np

import raycast_ref as RR

SILHOUETTE, DEPTH, CREASE = 1, 2, 4
LIGHT_ONE = 32767


def valid_hits(hits, faces, S):
    """bool: a hit as the kernels read it -- 0 <= hit_id < S^3 and a face in 0..5."""
    hits, faces = np.asarray(hits, np.int64), np.asarray(faces, np.int64)
    return (hits >= 0) & (hits < S ** 3) & (faces >= 0) & (faces < 6)


def hit_voxels(hits, S):
    """int64 [...,3] in (x, y, z) of flat voxel indices (meaningless where the hit is not valid)."""
    h = np.asarray(hits, np.int64)
    return np.stack([h % S, (h // S) % S, h // (S * S)], -1)


def stencil_normals(occ, hits, faces, R):
    """(ok bool [ph,pw], v int64 [ph,pw,3], n int64 [ph,pw,3]): n = n_src of rn_raycast_fwd's rule, zero where not ok."""
    occ = np.asarray(occ).astype(bool)
    S = occ.shape[0]
    hits, faces = np.asarray(hits, np.int64), np.asarray(faces, np.int64)
    ok = valid_hits(hits, faces, S)
    v = hit_voxels(np.where(ok, hits, 0), S)
    n = np.zeros(hits.shape + (3,), np.int64)
    if ok.any():
        n[ok] = RR.source_normal(RR.gradient(occ, v[ok], int(R)), faces[ok])
    return ok, v, n


def crease(n_p, n_q, crease_q):
    """The crease predicate on integer normals [...,3]: n_p . n_q <= 0 or 8 (n_p . n_q)^2 < crease_q |n_p|^2 |n_q|^2."""
    n_p, n_q = np.asarray(n_p, np.int64), np.asarray(n_q, np.int64)
    d = np.sum(n_p * n_q, -1)
    return (d <= 0) | (8 * d * d < int(crease_q) * np.sum(n_p * n_p, -1) * np.sum(n_q * n_q, -1))


def edge_bits(ok, v, n, line_radius, depth_gap, crease_q):
    """uint8 [ph,pw]: the three bits from (ok, hit voxels, normals) of one call's window; pixels outside it are ignored."""
    ok, v, n = np.asarray(ok, bool), np.asarray(v, np.int64), np.asarray(n, np.int64)
    ph, pw = ok.shape
    r = int(line_radius)
    inside = np.zeros((ph + 2 * r, pw + 2 * r), bool)
    okp = np.zeros_like(inside)
    vp = np.zeros(inside.shape + (3,), np.int64)
    npad = np.zeros_like(vp)
    inside[r:r + ph, r:r + pw] = True
    okp[r:r + ph, r:r + pw] = ok
    vp[r:r + ph, r:r + pw] = v
    npad[r:r + ph, r:r + pw] = n
    out = np.zeros((ph, pw), np.uint8)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            if dy == r and dx == r:
                continue
            q_in, q_ok = inside[dy:dy + ph, dx:dx + pw], okp[dy:dy + ph, dx:dx + pw]
            vq, nq = vp[dy:dy + ph, dx:dx + pw], npad[dy:dy + ph, dx:dx + pw]
            both = ok & q_ok
            out |= np.where(ok & q_in & ~q_ok, SILHOUETTE, 0).astype(np.uint8)
            out |= np.where(both & (np.abs(v - vq).max(-1) > int(depth_gap)), DEPTH, 0).astype(np.uint8)
            out |= np.where(both & crease(n, nq, crease_q), CREASE, 0).astype(np.uint8)
    return out


def edges(occ, hits, faces, normal_radius=2, line_radius=2, depth_gap=2, crease_q=4):
    """The bytes of rn_raycast_edges_fwd for one item: occ [S,S,S] bool [z,y,x], hits / faces [ph,pw]."""
    ok, v, n = stencil_normals(occ, hits, faces, normal_radius)
    return edge_bits(ok, v, n, line_radius, depth_gap, crease_q)


def quantise_light(l):
    """rint(32767 l / |l|) as three Python ints."""
    l = np.asarray(l, np.float64).reshape(3)
    return tuple(int(c) for c in np.rint(LIGHT_ONE * l / np.sqrt(np.sum(l * l))))


def band(normals_u8, light_q, K):
    """The integer band of rn_lines_encode for bytes [...,3]: min(K - 1, (K max(d, 0)) // (32767 * 255))."""
    b = np.asarray(normals_u8).astype(np.int64)
    d = sum(int(light_q[k]) * (2 * b[..., k] - 255) for k in range(3))
    return np.minimum(int(K) - 1, (int(K) * np.maximum(d, 0)) // (LIGHT_ONE * 255))


def band_float(normals_u8, light, K):
    """float64, the light not quantised: (K d, min(K - 1, floor(K max(d, 0)))) with d = l/|l| . (2 b / 255 - 1)."""
    l = np.asarray(light, np.float64).reshape(3)
    l = l / np.sqrt(np.sum(l * l))
    d = (2.0 * np.asarray(normals_u8).astype(np.float64) / 255.0 - 1.0) @ l
    return K * d, np.minimum(int(K) - 1, np.floor(K * np.maximum(d, 0.0))).astype(np.int64)


def tone(band_index, K, shadow_byte):
    """The byte of a band: shadow_byte + ((255 - shadow_byte) * 2 * band + (K - 1)) // (2 (K - 1))."""
    bi = np.asarray(band_index, np.int64)
    return int(shadow_byte) + ((255 - int(shadow_byte)) * 2 * bi + (int(K) - 1)) // (2 * (int(K) - 1))


def encode(normals_u8, edge, edge_mask=7, levels=0, shadow_byte=64, light_q=(0, 0, LIGHT_ONE)):
    """The bytes of rn_lines_encode: normals_u8 [...,3], edge [...] -> uint8 [...]."""
    b = np.asarray(normals_u8)
    e = np.asarray(edge).astype(np.int64)
    miss = ~b.any(-1)
    out = np.full(e.shape, 255, np.int64)
    if int(levels):
        out = tone(band(b, light_q, levels), levels, shadow_byte)
    out = np.where((e & int(edge_mask)) != 0, 0, out)
    return np.where(miss, 255, out).astype(np.uint8)
