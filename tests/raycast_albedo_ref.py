"""NumPy int64 reference of the albedo targets (rn_raycast_albedo_fwd, rn_albedo_encode), written from the rule stated in
include/rendernet_hip.h.  Everything is an integer function of (hit voxel, wave table, quantised code), so the kernels must
agree with it on every pixel exactly."""
import math

import numpy as np


def cos_q():
    """COS_Q[i] = rint(127 cos(2 pi i / 256)), int64 [256]."""
    return np.array([int(np.rint(127.0 * math.cos(2.0 * math.pi * i / 256.0))) for i in range(256)], np.int64)


def albedo(hit, waves, code_q, S, base):
    """hit int [B,ph,pw] (flat index of the hit voxel; < 0 or >= S^3 = a miss), waves int16 [K,8], code_q int8 [B,K], base three
    bytes -> uint8 [B,ph,pw,3]."""
    hit = np.asarray(hit, np.int64)
    w = np.asarray(waves, np.int64)
    q = np.asarray(code_q, np.int64)
    B = hit.shape[0]
    assert hit.ndim == 3 and w.ndim == 2 and w.shape[1] == 8 and q.shape == (B, w.shape[0])
    C = cos_q()
    is_hit = (hit >= 0) & (hit < S ** 3)
    i = np.where(is_hit, hit, 0)
    xs, ys, zs = i % S, (i // S) % S, i // (S * S)
    acc = np.zeros(hit.shape + (3,), np.int64)
    for k in range(w.shape[0]):
        fx, fy, fz, phase = w[k, :4]
        idx = (4 * (fx * xs + fy * ys + fz * zs) + phase) & 255
        acc += (q[:, k, None, None] * C[idx])[..., None] * w[k, 4:7]
    assert np.abs(acc).max(initial=0) < 2 ** 31 - 32768                      # the kernel's 32-bit sum does not wrap
    byte = np.clip(np.asarray(base, np.int64) + ((acc + 32768) >> 16), 0, 255)
    return np.where(is_hit[..., None], byte, 0).astype(np.uint8)


def encode(colour, hit, S, smooth):
    """colour uint8 [B,ph,pw,3] and hit [B,ph,pw] -> uint8 [B,ph,pw,3]: per channel (2 Sigma + n) / (2 n) over the hit pixels of
    the (2 smooth + 1)^2 window clipped to the picture; a miss is black.  smooth = 0 keeps the colour of every hit."""
    hit = np.asarray(hit, np.int64)
    r = int(smooth)
    is_hit = (hit >= 0) & (hit < S ** 3)
    B, ph, pw = hit.shape
    val = np.where(is_hit[..., None], np.asarray(colour, np.int64), 0)
    pad = ((0, 0), (r, r), (r, r))
    vp, npad = np.pad(val, pad + ((0, 0),)), np.pad(is_hit.astype(np.int64), pad)
    sigma, n = np.zeros_like(val), np.zeros(hit.shape, np.int64)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            sigma += vp[:, dy:dy + ph, dx:dx + pw]
            n += npad[:, dy:dy + ph, dx:dx + pw]
    n1 = np.maximum(n, 1)[..., None]
    return np.where(is_hit[..., None], (2 * sigma + n1) // (2 * n1), 0).astype(np.uint8)


def picture(hit, waves, code_q, S, base, smooth):
    """What ops.albedo_from_hits returns."""
    return encode(albedo(hit, waves, code_q, S, base), hit, S, smooth)


def flat(xs, ys, zs, S):
    return (zs * S + ys) * S + xs
