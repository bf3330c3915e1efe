"""NumPy twin of rn_hit_depth / rn_voxel_carve (include/rendernet_hip.h states the rule): a grid carved from silhouettes and
depth maps under the rasteriser's integer camera.  TEST INFRASTRUCTURE ONLY.  `carve` is int64 throughout and takes the `cam` and
the `views` it is handed, as the other twins do: the device tests hand it what the device produced.  `hit_depth` is float64 from
the float32 matrix, every operation rounded on its own.  `scan` makes the views of a grid through the caster's twin
(raycast_ref.cast), and `cameras` the integer cameras through the rasteriser's (mesh_raster_ref.camera)."""
import numpy as np

import mesh_raster_ref as MR
import raycast_ref as RR

U = 256


def hit_depth(hit, face, m_inv, S, N, f, window=None, view_from_low_x=False):
    """hit int32 [ph,pw], face int8 [ph,pw] of one item as the caster wrote them for `window`, m_inv float32 [3,4] ->
    depth int32 [ph,pw]: the entry depth in 1/256 camera cell, -1 for a miss, a hit outside [0, S^3) or a face outside 0..5."""
    if window is None:
        window = (0, 0, f * N, f * N)
    row0, col0, ph, pw = (int(v) for v in window)
    hit = np.asarray(hit).astype(np.int64).reshape(ph, pw)
    face = np.asarray(face).astype(np.int64).reshape(ph, pw)
    M = np.asarray(m_inv, np.float32).astype(np.float64).reshape(3, 4)
    r = np.arange(row0, row0 + ph, dtype=np.float64)[:, None]
    c = np.arange(col0, col0 + pw, dtype=np.float64)[None, :]
    y = np.broadcast_to((N - 1) - ((r + 0.5) / f - 0.5), (ph, pw))
    z = np.broadcast_to((c + 0.5) / f - 0.5, (ph, pw))
    x0 = -0.5 if view_from_low_x else N - 0.5
    valid = (hit >= 0) & (hit < S ** 3) & (face >= 0) & (face <= 5)
    k = np.where(valid, face >> 1, 0)
    h = np.where(valid, hit, 0)
    Mk = M[k]                                                    # [ph,pw,4]
    with np.errstate(all="ignore"):
        ok = ((Mk[..., 0] * x0 + Mk[..., 1] * y) + Mk[..., 2] * z) + Mk[..., 3]
        dk = Mk[..., 0] if view_from_low_x else -Mk[..., 0]
        vk = np.stack([h % S, (h // S) % S, h // (S * S)], -1)
        vk = np.take_along_axis(vk, k[..., None], -1)[..., 0].astype(np.float64)
        plane = np.where(face & 1, vk + 0.5, vk - 0.5)
        t = np.where(dk == 0.0, 0.0, (plane - ok) / np.where(dk == 0.0, 1.0, dk))
        t = np.where(np.isnan(t), 0.0, t)
        u = np.floor(256.0 * np.where(t > 0.0, t, 0.0))
        d = np.where(u < 0.0, 0.0, np.where(u > 256.0 * N, 256.0 * N, u))
    return np.where(valid, d, -1.0).astype(np.int32)


def project_centres(cam, S):
    """int64 (X, Y, D), each [S,S,S] indexed [z,y,x]: the rasteriser's projection of the voxel centres under cam [3,4]."""
    k = U * np.arange(S, dtype=np.int64) + 128
    q = np.stack(np.meshgrid(k, k, k, indexing="ij"), -1).reshape(-1, 3)
    P = MR.project(cam, q, S)                                    # the centres lie inside [0, 256 S]: project's clamp is idle
    return tuple(P[:, i].reshape(S, S, S) for i in range(3))


def carve(views, cam, S, window, use_depth=True, slack=8, outside_keep=True, tolerance=0):
    """views int32 [K,ph,pw], cam int64 [K,3,4] of ONE item -> (votes uint8 [S,S,S], hull bool [S,S,S])."""
    views = np.asarray(views).astype(np.int64)
    K = views.shape[0]
    cam = np.asarray(cam, np.int64).reshape(K, 3, 4)
    row0, col0, ph, pw = (int(v) for v in window)
    assert views.shape == (K, ph, pw) and 1 <= K <= 255
    votes = np.zeros((S, S, S), np.int64)
    for k in range(K):
        X, Y, D = project_centres(cam[k], S)
        r, c = (Y >> 8) - row0, (X >> 8) - col0                  # floor division
        inside = (r >= 0) & (r < ph) & (c >= 0) & (c < pw)
        v = views[k][np.clip(r, 0, ph - 1), np.clip(c, 0, pw - 1)]
        ok = v >= 0
        if use_depth:
            ok &= D + int(slack) >= v
        votes += np.where(inside, ok, bool(outside_keep))
    return votes.astype(np.uint8), votes >= K - int(tolerance)


def cameras(poses, low, S, N, f):
    """cam int64 [K,3,4] and m_inv float32 [K,3,4] of poses [K,3] with the ray ends low [K], by the float64 paths."""
    from oracle import resample as OR
    M = OR.inverse_affine(np.asarray(poses, np.float32).reshape(-1, 3), size=S, new_size=N).astype(np.float32)
    cam = np.stack([MR.camera(M[k], N, f, bool(low[k])) for k in range(len(M))])
    return cam, M


def scan(occ, poses, low, N, f, window=None):
    """occ bool [S,S,S] -> (views int32 [K,ph,pw], cam int64 [K,3,4]): K casts of the caster's twin and their entry depths."""
    occ = np.asarray(occ).astype(bool)
    S = occ.shape[0]
    cam, M = cameras(poses, low, S, N, f)
    views = []
    for k in range(len(M)):
        hit, face, _ = RR.cast(occ, M[k], N, f, window, view_from_low_x=bool(low[k]))
        views.append(hit_depth(hit, face, M[k], S, N, f, window, bool(low[k])))
    return np.stack(views), cam


def pixels_per_voxel(cam):
    """float64 [...]: the smaller of |cam row 0| and |cam row 1| over 2^20."""
    a = np.asarray(cam, np.int64).astype(np.float64)[..., :2, :3]
    return np.sqrt((a * a).sum(-1)).min(-1) / float(1 << 20)


def iou(a, b):
    a, b = np.asarray(a, bool), np.asarray(b, bool)
    return float((a & b).sum()) / float(max((a | b).sum(), 1))
