"""float64 reference of the ambient-occlusion caster (include/rendernet_hip.h, rn_raycast_ao_fwd / rn_ao_encode).
TEST INFRASTRUCTURE ONLY; NumPy, vectorised over (unique hit face) x (64 rays).

It reads the rule of the header: the float32 directions of scripts/gen_ao_dirs.py upcast to float64, the crossing of axis k
recomputed each step from the integer boundary as (b_k - c_k) * (1 / d_k), integer end tests.  The tie screen of the table
keeps crossings of different axes 1e-3 apart and the kernel's float32 parameters are within 1e-5 of these, so both walk
the same voxels: the kernel must equal this reference on EVERY pixel, no stability screen."""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scripts.gen_ao_dirs import table  # noqa: E402

RAYS = 64
MISS = 255
_TABLE = None


def dirs():
    """The direction table, float32 [64,3], generated once."""
    global _TABLE
    if _TABLE is None:
        _TABLE = table()
    return _TABLE


def face_dirs(face):
    """float64 [64,3] source-space directions for a face 0..5: d[a] = s tx, d[(a+1)%3] = ty, d[(a+2)%3] = tz."""
    T = dirs().astype(np.float64)
    a, s = int(face) >> 1, (1.0 if int(face) & 1 else -1.0)
    d = np.empty((RAYS, 3))
    d[:, a], d[:, (a + 1) % 3], d[:, (a + 2) % 3] = s * T[:, 0], T[:, 1], T[:, 2]
    return d


def occupied_box(occ):
    S = occ.shape[0]
    zz, yy, xx = np.nonzero(occ)
    if len(zz) == 0:
        return np.array([S, S, S]), np.array([-1, -1, -1])
    return np.array([xx.min(), yy.min(), zz.min()]), np.array([xx.max(), yy.max(), zz.max()])


def open_rays(occ, v, face, L, dtype=np.float64):
    """bool [n,64]: which rays of the faces (v [n,3] in (x, y, z), face [n]) end in the open.  occ [S,S,S] bool [z,y,x].
    dtype=np.float32 evaluates the crossings with the kernel's roundings instead (a host check of the tie screen)."""
    occ = np.asarray(occ).astype(bool)
    lo, hi = occupied_box(occ)
    v = np.asarray(v, np.int64).reshape(-1, 3)
    face = np.asarray(face, np.int64).reshape(-1)
    n = len(v)
    a, s = face >> 1, np.where(face & 1, 1, -1)
    fd = np.stack([face_dirs(f) for f in range(6)])                        # [6,64,3]
    d = fd[face].astype(dtype)                                             # [n,64,3]
    with np.errstate(divide="ignore"):
        inv = dtype(1.0) / d
    sg = np.where(d > 0, 1, -1).astype(np.int64)
    off = np.zeros((n, 1, 3), dtype)
    off[np.arange(n), 0, a] = 0.5 * s
    w = np.zeros((n, RAYS, 3), np.int64)
    w[np.arange(n), :, a] = s[:, None]
    is_open = np.ones((n, RAYS), bool)
    live = np.ones((n, RAYS), bool)
    for _ in range(3 * int(L) + 3):
        if not live.any():
            break
        i, j = np.nonzero(live)
        u = v[i] + w[i, j]
        outside = np.any((u < lo) | (u > hi), 1)
        uc = np.clip(u, 0, occ.shape[0] - 1)
        on = ~outside & occ[uc[:, 2], uc[:, 1], uc[:, 0]]
        far = ~outside & ~on & (np.abs(w[i, j]).max(1) > L)
        is_open[i[on], j[on]] = False
        done = outside | on | far
        live[i[done], j[done]] = False
        i, j = i[~done], j[~done]
        if len(i) == 0:
            break
        with np.errstate(invalid="ignore"):
            t = (((w[i, j] + 0.5 * sg[i, j]).astype(dtype)) - off[i, 0]) * inv[i, j]
        t[d[i, j] == 0] = np.inf
        m = np.argmin(t, 1)                                                # the first minimum, as the kernel's strict '<'
        w[i, j, m] += sg[i, j, m]
    assert not live.any()                                                  # a ray visits at most 3L + 1 voxels
    return is_open


def ao_counts(occ, hits, faces, L, dtype=np.float64):
    """uint8 counts like rn_raycast_ao_fwd's: hits int [...] (flat voxel index, < 0 = miss), faces int [...] -> 0..64, 255 = miss."""
    occ = np.asarray(occ).astype(bool)
    S = occ.shape[0]
    hits, faces = np.asarray(hits, np.int64), np.asarray(faces, np.int64)
    out = np.full(hits.shape, MISS, np.uint8)
    ok = (hits >= 0) & (hits < S ** 3) & (faces >= 0) & (faces < 6)
    if not ok.any():
        return out
    keys, back = np.unique(hits[ok] * 8 + faces[ok], return_inverse=True)
    h, f = keys >> 3, keys & 7
    v = np.stack([h % S, (h // S) % S, h // (S * S)], 1)
    out[ok] = open_rays(occ, v, f, L, dtype).sum(1).astype(np.uint8)[back]
    return out


def encode(counts, smooth):
    """The bytes of rn_ao_encode for counts [ph,pw] (or [B,ph,pw]): integer arithmetic, window clipped to the array."""
    c = np.asarray(counts)
    if c.ndim == 3:
        return np.stack([encode(x, smooth) for x in c])
    r = int(smooth)
    hit = c <= RAYS
    ph, pw = c.shape
    val = np.zeros((ph + 2 * r, pw + 2 * r), np.int64)
    num = np.zeros_like(val)
    val[r:r + ph, r:r + pw] = np.where(hit, c, 0)
    num[r:r + ph, r:r + pw] = hit
    tot, n = np.zeros((ph, pw), np.int64), np.zeros((ph, pw), np.int64)
    for dy in range(2 * r + 1):
        for dx in range(2 * r + 1):
            tot += val[dy:dy + ph, dx:dx + pw]
            n += num[dy:dy + ph, dx:dx + pw]
    return np.where(hit, (510 * tot + 64 * n) // np.maximum(128 * n, 1), 0).astype(np.uint8)


# -- the closed-form grids -----------------------------------------------------------------------------------------------

S = 32


def flat(x, y, z, side=S):
    return (z * side + y) * side + x


def axis_grid(fill, axis):
    """A grid described along 'x' moved to `axis` with the face mapping's cyclic order: fill(g) gets g indexed
    [main, second, third] = axes (a, a+1, a+2) mod 3 and the result is occ [z,y,x]."""
    g = np.zeros((S, S, S), bool)
    fill(g)
    # g[i0, i1, i2] lies at source axis a = i0, (a+1)%3 = i1, (a+2)%3 = i2; occ wants [z, y, x] = source axes [2, 1, 0]
    order = [(axis + k) % 3 for k in range(3)]                 # g's dims -> source axes
    to_xyz = np.transpose(g, np.argsort(order))                # dims now (x, y, z)
    return np.ascontiguousarray(np.transpose(to_xyz, (2, 1, 0)))


def voxel_on(axis, main, second, third):
    v = [0, 0, 0]
    v[axis], v[(axis + 1) % 3], v[(axis + 2) % 3] = main, second, third
    return v


def closed_form_cases():
    """(name, occ, hits, faces, L, expected counts): the four closed-form grids, each along every axis and sign where the
    form has one.  Shared by the host and the device tests."""
    T = dirs().astype(np.float64)
    lateral = np.maximum(np.abs(T[:, 1]), np.abs(T[:, 2]))
    cases = []
    # one voxel alone: every ray leaves the box at once
    occ = np.zeros((S, S, S), bool)
    occ[10, 11, 12] = True
    cases.append(("voxel", occ, [flat(12, 11, 10)] * 6, list(range(6)), 8, [64] * 6))
    for axis in range(3):
        for sign in (1, -1):
            face = 2 * axis + (sign > 0)
            # a one-voxel slab that fills the grid laterally: nothing above its top face
            occ = axis_grid(lambda g: g.__setitem__((slice(13, 14),), True), axis)
            cases.append(("slab a%d s%+d" % (axis, sign), occ, [flat(*voxel_on(axis, 13, 16, 15))], [face], 8, [64]))
            # two slabs one empty layer apart: open iff the ray gets L + 1 cells sideways before its second main-axis boundary
            for L in (2, 4, 8):
                lo_slab, hi_slab = (12, 14) if sign > 0 else (14, 12)
                occ = axis_grid(lambda g: (g.__setitem__((slice(lo_slab, lo_slab + 1),), True),
                                           g.__setitem__((slice(hi_slab, hi_slab + 1),), True)), axis)
                want = int(np.sum(T[:, 0] * (L + 0.5) < lateral))
                cases.append(("gap a%d s%+d L%d" % (axis, sign, L), occ, [flat(*voxel_on(axis, lo_slab, 16, 15))], [face], L, [want]))
            # the floor of a 1-wide, h-deep well in a solid half-space: open iff h main-axis boundaries come before the first lateral one
            for h in (1, 3):
                def well(g, h=h, sign=sign):
                    if sign > 0:
                        g[:20] = True
                        g[20 - h:20, 16, 15] = False
                    else:
                        g[12:] = True
                        g[12:12 + h, 16, 15] = False
                floor_main = 20 - h - 1 if sign > 0 else 12 + h
                want = int(np.sum(2 * h * lateral < T[:, 0]))
                cases.append(("well a%d s%+d h%d" % (axis, sign, h), axis_grid(well, axis), [flat(*voxel_on(axis, floor_main, 16, 15))],
                              [face], 8, [want]))
    return cases
