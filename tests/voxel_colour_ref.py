"""NumPy int64 twin of the voxel colouring (rn_voxel_colour_accumulate, _resolve, _fill, rn_colour_from_hits,
rn_mesh_vertex_colours), written from the rule stated in include/rendernet_hip.h.  Everything is an integer function of its
inputs, so the kernels must agree with it on every word exactly."""
import numpy as np

import raycast_albedo_ref as AR

MAX_PIXELS = 8421504                     # K ph pw of one call: 255 times it stays below 2^31


def counts(hits, S, mask=None):
    """bool, the shape of hits: the pixels that count."""
    h = np.asarray(hits, np.int64)
    ok = (h >= 0) & (h < S ** 3)
    return ok if mask is None else ok & (np.asarray(mask) != 0)


def accumulate(images, hits, S, mask=None, sums=None):
    """images uint8 [B,K,ph,pw,3], hits int [B,K,ph,pw], mask uint8 [B,K,ph,pw] or None -> int32 [B,S,S,S,4], added to `sums`."""
    images, h = np.asarray(images), np.asarray(hits, np.int64)
    B, K, ph, pw = h.shape
    assert images.shape == (B, K, ph, pw, 3) and images.dtype == np.uint8 and K * ph * pw <= MAX_PIXELS
    out = np.zeros((B, S ** 3, 4), np.int64) if sums is None else np.asarray(sums, np.int64).reshape(B, S ** 3, 4).copy()
    ok = counts(h, S, mask)
    for b in range(B):
        sel = ok[b]
        val = np.concatenate([images[b][sel].astype(np.int64), np.ones((int(sel.sum()), 1), np.int64)], 1)
        np.add.at(out[b], h[b][sel], val)
    assert np.abs(out).max(initial=0) < 2 ** 31
    return out.astype(np.int32).reshape(B, S, S, S, 4)


def _mean(sigma, n):
    """(2 sigma + n) // (2 n) where n > 0 (n broadcast over the channels), clamped to a byte; 0 elsewhere."""
    n1 = np.maximum(n, 1)
    return np.clip((2 * sigma + n1) // (2 * n1), 0, 255)


def resolve(sums, unseen=(128, 128, 128)):
    """sums int32 [...,4] -> (colours uint8 [...,3], known uint8 [...])."""
    s = np.asarray(sums, np.int64)
    n = s[..., 3]
    seen = n > 0
    col = np.where(seen[..., None], _mean(s[..., :3], n[..., None]), np.asarray(unseen, np.int64))
    return col.astype(np.uint8), seen.astype(np.uint8)


def fill_pass(colours, known, occ):
    """One Jacobi pass over ONE grid: colours uint8 [S,S,S,3], known uint8 [S,S,S], occ bool [S,S,S] -> the next state."""
    colours, known, occ = np.asarray(colours), np.asarray(known), np.asarray(occ).astype(bool)
    S = known.shape[0]
    k = np.pad((known != 0).astype(np.int64), 1)
    c = np.pad(colours.astype(np.int64), ((1, 1), (1, 1), (1, 1), (0, 0))) * k[..., None]
    sigma, m = np.zeros((S, S, S, 3), np.int64), np.zeros((S, S, S), np.int64)
    for dz in range(3):
        for dy in range(3):
            for dx in range(3):
                if (dz, dy, dx) == (1, 1, 1):
                    continue
                sigma += c[dz:dz + S, dy:dy + S, dx:dx + S]
                m += k[dz:dz + S, dy:dy + S, dx:dx + S]
    take = (known == 0) & occ & (m > 0)
    out_c = np.where(take[..., None], _mean(sigma, m[..., None]), colours.astype(np.int64)).astype(np.uint8)
    return out_c, np.where(take, 2, known).astype(np.uint8)


def colours_of(sums, occ=None, fill=0, unseen=(128, 128, 128)):
    """What ops.voxel_colours returns: sums [B,S,S,S,4], occ bool [B,S,S,S] -> (colours [B,S,S,S,3], known [B,S,S,S])."""
    col, known = resolve(sums, unseen)
    col, known = col.copy(), known.copy()
    for b in range(col.shape[0]):
        for _ in range(int(fill)):
            col[b], known[b] = fill_pass(col[b], known[b], occ[b])
    return col, known


def from_hits(hit, colours, S, smooth=0, background=(0, 0, 0)):
    """What ops.colour_from_hits returns: hit int [B,ph,pw], colours uint8 [B,S,S,S,3] -> uint8 [B,ph,pw,3]."""
    h = np.asarray(hit, np.int64)
    B = h.shape[0]
    ok = (h >= 0) & (h < S ** 3)
    flat = np.asarray(colours).reshape(B, S ** 3, 3)
    out = np.stack([flat[b][np.where(ok[b], h[b], 0)] for b in range(B)]) if B else np.zeros(h.shape + (3,), np.uint8)
    out = np.where(ok[..., None], out, np.asarray(background, np.uint8)).astype(np.uint8)
    if int(smooth) == 0:
        return out
    return np.where(ok[..., None], AR.encode(out, h, S, smooth), out).astype(np.uint8)


def vertex_cells(q):
    """The cell of lattice vertices q int [V,3]: (q + 128) >> 8; its corner samples are cell - 1 + {0, 1} per axis."""
    return (np.asarray(q, np.int64) + 128) >> 8


def vertex_colours(q, vert_offsets, colours, known, unseen=(128, 128, 128)):
    """q int32 [V,3], vert_offsets int64 [B+1], colours uint8 [B,S,S,S,3], known uint8 [B,S,S,S] -> uint8 [V,3]."""
    q, vo = np.asarray(q, np.int64).reshape(-1, 3), np.asarray(vert_offsets, np.int64)
    colours, known = np.asarray(colours).astype(np.int64), np.asarray(known)
    S = known.shape[1]
    item = np.repeat(np.arange(len(vo) - 1), np.diff(vo))
    assert len(item) == len(q)
    cell = vertex_cells(q)
    sigma, m = np.zeros((len(q), 3), np.int64), np.zeros(len(q), np.int64)
    for c in range(8):
        s = cell - 1 + np.array([c >> 2, (c >> 1) & 1, c & 1])
        inside = ((s >= 0) & (s < S)).all(1)
        sc = np.clip(s, 0, S - 1)
        ok = inside & (known[item, sc[:, 0], sc[:, 1], sc[:, 2]] != 0)
        sigma += np.where(ok[:, None], colours[item, sc[:, 0], sc[:, 1], sc[:, 2]], 0)
        m += ok
    return np.where((m > 0)[:, None], _mean(sigma, m[:, None]), np.asarray(unseen, np.int64)).astype(np.uint8)


def surface_voxels(occ):
    """bool like occ [S,S,S]: occupied with an empty 6-neighbour, the outside being empty."""
    o = np.pad(np.asarray(occ).astype(bool), 1)
    S = o.shape[0] - 2
    core = o[1:-1, 1:-1, 1:-1]
    buried = np.ones_like(core)
    for ax in range(3):
        for d in (0, 2):
            sl = [slice(1, S + 1)] * 3
            sl[ax] = slice(d, d + S)
            buried &= o[tuple(sl)]
    return core & ~buried
