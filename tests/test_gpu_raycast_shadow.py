"""rn_shadow_light / rn_raycast_shadow_fwd / rn_shadow_encode (rendernet_amd/csrc/raycast.hip), ops.raycast_shadow and
SyntheticTargets(shader="shadow") against the integer twin tests/raycast_shadow_ref.py.  -m gpu.

Visibility and bytes are integer functions of (hit voxels, entry faces, occupancy, the quantised lights), so every comparison
is exact and covers every pixel: hits, faces, normal bytes and light_src come from the device's own rn_raycast_fwd and
rn_shadow_light, the twin computes lit and bytes from those arrays and the host copy of the grid.  No pixel is left out."""
import ctypes
import dataclasses

import numpy as np
import pytest

import raycast_shadow_ref as SR
from conftest import FIXTURES
from rendernet_amd._lib import RN_E_INVALID

pytestmark = pytest.mark.gpu
CHAIR_POSE, BUNNY_POSE = (37.0, -20.0, 1.2), (250.0, 30.0, 1.0)             # azimuth, elevation (degrees), scale
WINDOW = (190, 203, 112, 96)                                               # odd origin, no multiple of the 16 x 16 tile
WALL_LIGHTS = ((1, 1, 0), (1, 2, 0), (3, 2, 0), (1023, 511, 0), (2, 1, 1), (2, 1, 0), (2, 3, 0))
AXIS_PAIRS = [(a, sa, b, sb) for a in range(3) for b in range(3) if a != b for sa in (1, -1) for sb in (1, -1)]


def pose_rad(az, el, s):
    return np.array([az * np.pi / 180.0, el * np.pi / 180.0, s], np.float32)


def demo_light():
    from rendernet_amd import synth
    from rendernet_amd.tools.Phong_shading import generate_light_pos
    return np.asarray(generate_light_pos(synth.LIGHT_ELEVATION, synth.LIGHT_AZIMUTH), np.float64).reshape(3)


def cuda_vox(occ):
    import torch
    return torch.as_tensor(np.ascontiguousarray(occ[..., None]).astype(np.uint8)).cuda()


def device_shadow(occ, poses, N, f, window=None, light=None, low_x=False, bias=1, smooth=0, ambient_byte=26, normal_radius=2):
    """bool grids [B,S,S,S] at poses [B,3] -> (m_inv, bytes, normal bytes, hit, face, light_src, lit) as NumPy, all of one
    ops.raycast_shadow call on the matrices of ops.pose_to_affine."""
    import torch
    from rendernet_amd import ops
    m = ops.pose_to_affine(torch.as_tensor(np.asarray(poses, np.float32)).cuda(), occ.shape[1], N)
    got = ops.raycast_shadow(cuda_vox(occ), m, new_size=N, pixels_per_cell=f, window=window, affine=True, light=light, bias=bias,
                             smooth=smooth, ambient_byte=ambient_byte, normal_radius=normal_radius, view_from_low_x=low_x,
                             return_parts=True)
    out, rgb, hit, face, D, lit = got
    assert out.dtype is torch.uint8 and lit.dtype is torch.uint8 and D.dtype is torch.int32
    assert out.shape == hit.shape == lit.shape and D.shape == (len(occ), 3)
    return (m.cpu().numpy(),) + tuple(t.cpu().numpy() for t in got)


def twin_lit(occ, hit, face, D, bias):
    return np.stack([SR.shadow_lit(occ[b], hit[b], face[b], D[b], bias) for b in range(len(occ))])


def twin_bytes(rgb, lit, smooth, ambient_byte, light):
    lq = SR.quantise_light(demo_light() if light is None else light)
    return np.stack([SR.encode(rgb[b], lit[b], smooth, ambient_byte, lq) for b in range(len(lit))])


def assert_same(got, want, what=""):
    bad = got != want
    assert not bad.any(), "%s: %d pixels differ, first at %s: kernel %d twin %d" % (
        what, bad.sum(), np.argwhere(bad)[0], got[bad][0], want[bad][0])


def shares(lit):
    hit = lit <= 1
    return float((lit[hit] == 1).mean()), float((lit[hit] == 0).mean())


@pytest.fixture(scope="module")
def models(fixtures_vox):
    """chair and bunny as bool [2,64,64,64] indexed [z,y,x]."""
    return np.stack([fixtures_vox[FIXTURES.index(m), ..., 0] > 0.5 for m in ("chair", "bunny")])


MODEL_POSES = np.stack([pose_rad(*CHAIR_POSE), pose_rad(*BUNNY_POSE)])


# -- closed forms ---------------------------------------------------------------------------------------------------------

def from_hits(occ, hit, face, D, bias):
    import torch
    from rendernet_amd import ops
    S = occ.shape[1]
    bits, box = ops.voxel_pack(cuda_vox(occ))
    lit = ops.raycast_shadow_from_hits(bits, box, torch.as_tensor(hit.astype(np.int32)).cuda(), torch.as_tensor(face.astype(np.int8)).cuda(),
                                       torch.as_tensor(np.asarray(D, np.int32)).cuda(), S, bias)
    assert lit.dtype is torch.uint8 and tuple(lit.shape) == hit.shape
    return lit.cpu().numpy()


def test_lone_voxel_and_slabs_from_given_hits():
    """S = 32, one item per light: the lone voxel under all 27 sign patterns of D (lit = [s D_a > 0] on its six faces), and a
    laterally filled slab on each axis lit from either side for every D with a component that way."""
    S = 32
    occ, hit, face, Ds, want = [], [], [], [], []
    lone = np.zeros((S, S, S), bool)
    lone[14, 12, 10] = True
    for D in [(x, y, z) for x in (-1023, 0, 7) for y in (-5, 0, 1023) for z in (-1, 0, 512)]:
        occ.append(lone); Ds.append(D)
        hit.append(np.full(6, (14 * S + 12) * S + 10)); face.append(np.arange(6))
        want.append([1 if ((1 if f & 1 else -1) * D[f >> 1]) > 0 else 0 for f in range(6)])
    for a in range(3):
        slab_xyz = np.zeros((S, S, S), bool)
        sl = [slice(None)] * 3
        sl[a] = slice(9, 12)
        slab_xyz[tuple(sl)] = True
        for sgn in (1, -1):
            for lateral in ((0, 0), (1023, -300), (-1, 1023)):
                D = np.zeros(3, np.int64)
                D[a] = sgn * (1 if lateral[0] else 1023)
                D[(a + 1) % 3], D[(a + 2) % 3] = lateral
                v_hi, v_lo = np.array([5, 6, 7]), np.array([5, 6, 7])
                v_hi[a], v_lo[a] = 11, 9
                occ.append(slab_xyz.transpose(2, 1, 0)); Ds.append(tuple(D))
                hit.append([(v[2] * S + v[1]) * S + v[0] for v in (v_hi, v_lo, v_hi, v_lo, v_hi, v_lo)])
                face.append([2 * a + 1, 2 * a, 2 * a, 2 * a + 1, 2 * ((a + 1) % 3), 2 * ((a + 1) % 3) + 1])
                want.append([int(sgn > 0), int(sgn < 0), 0, 0, 0, 0])       # the last four look into the slab (bias 0), or away
    occ, hit, face, want = np.stack(occ), np.array(hit)[:, None, :], np.array(face)[:, None, :], np.array(want, np.uint8)[:, None, :]
    got = from_hits(occ, hit, face, Ds, 0)
    assert_same(got, twin_lit(occ, hit, face, np.array(Ds), 0), "twin")
    assert_same(got, want, "closed form")


@pytest.mark.parametrize("h", [1, 3, 5])
def test_wall_on_a_floor_from_given_hits(h):
    """S = 32, the wall of height h on every (floor axis, wall axis) pair, both signs, one item per (pair, light): the floor
    face at distance q0 - q from the wall is shadowed exactly when D_p (2 (q0 - q) - 1) < 2 h D_q, ties by the axis order."""
    S, q = 32, np.arange(0, 20)
    occ, hit, face, Ds, want = [], [], [], [], []
    for a, sa, b, sb in AXIS_PAIRS:
        scene = SR.wall_scene(S, h, a, sa, b, sb)
        ids, fc = SR.wall_floor_hits(S, q, 5, a, sa, b, sb)
        for Dc in WALL_LIGHTS:
            occ.append(scene); hit.append(ids); face.append(np.full(len(q), fc)); Ds.append(SR.wall_light(Dc, a, sa, b, sb))
            want.append(np.where(SR.wall_shadowed(Dc, h, q, a, b), 0, 1))
    occ, hit, face, want = np.stack(occ), np.array(hit)[:, None, :], np.array(face)[:, None, :], np.array(want, np.uint8)[:, None, :]
    got = from_hits(occ, hit, face, np.array(Ds), 0)
    assert_same(got, want, "closed form")
    assert_same(got, twin_lit(occ, hit, face, np.array(Ds), 0), "twin")
    assert (want == 0).any() and (want == 1).any()
    # bias 3 hides the wall from the three nearest floor voxels at most: still the twin
    assert_same(from_hits(occ, hit, face, np.array(Ds), 3), twin_lit(occ, hit, face, np.array(Ds), 3), "bias 3")


def ragged_planes():
    """Hand-made inputs of rn_shadow_encode, B = 2 at 19 x 37 (two tiles down, three across, both ragged, and narrower than
    the 8-pixel halo on neither side): seeded random normal bytes, lit in {0, 1, 255}; the second item is all misses."""
    rng = np.random.default_rng(20)
    rgb = rng.integers(0, 256, (2, 19, 37, 3), dtype=np.uint8)
    lit = rng.choice(np.array([0, 1, 255], np.uint8), (2, 19, 37))
    lit[1] = 255
    return rgb, lit


@pytest.mark.parametrize("smooth", [0, 1, 8])
def test_encode_of_given_planes_at_a_ragged_window(smooth):
    """ops.shadow_encode alone where tile edges, halo clipping and the largest radius meet, against the twin byte for byte."""
    import torch
    from rendernet_amd import ops
    rgb, lit = ragged_planes()
    got = ops.shadow_encode(torch.as_tensor(rgb).cuda(), torch.as_tensor(lit).cuda(), None, smooth, 26).cpu().numpy()
    want = twin_bytes(rgb, lit, smooth, 26, None)
    assert_same(got, want, "smooth %d" % smooth)
    assert len(np.unique(want[0])) > 8 and (want[0][lit[0] == 255] == 0).all() and (want[1] == 0).all()


@pytest.mark.parametrize("light", [(0.0, 1.0, 1.0), (0.0, 1.0, 2.0)])
def test_wall_through_the_caster(light):
    """Pose (90, 0, 1): M_lin is the identity, the camera looks down -x, so the floor x = 8 faces it and the light (right, up,
    towards) = (0, 1, k) is D = (k, 1, 0) / max in source axes.  N = 64, f = 1, heights 1, 3, 5 as three items, bias 0: the
    shadowed floor rows are those of the formula, evaluated with the device's D."""
    S = 32
    occ = np.stack([SR.wall_scene(S, h) for h in (1, 3, 5)])
    m, out, rgb, hit, face, D, lit = device_shadow(occ, np.tile(pose_rad(90.0, 0.0, 1.0), (3, 1)), 64, 1, light=light, bias=0)
    assert np.abs(m[:, :, :3] - np.eye(3)).max() < 1e-6
    assert (D[:, 2] == 0).all() and (D[:, 0] == 1023).all()
    assert np.isin(D[:, 1], (1022, 1023) if light[2] == 1.0 else (511, 512)).all()      # 511.5 may round either way in float32
    assert_same(lit, twin_lit(occ, hit, face, D, 0))
    assert_same(out, twin_bytes(rgb, lit, 0, 26, light), "bytes")
    for i, h in enumerate((1, 3, 5)):
        x, y = hit[i] % S, (hit[i] // S) % S
        floor = (hit[i] >= 0) & (x == 8)
        assert floor.sum() == 31 * 32 and (face[i][floor] == 1).all()       # every floor voxel but the row under the wall
        near = floor & (y < 20)
        want = SR.wall_shadowed((int(D[i, 0]), int(D[i, 1]), 0), h, y[near])
        assert np.array_equal(lit[i][near] == 0, want) and not want.all()
        if light[2] == 1.0:
            assert want.sum() == 32 * h                                     # h rows of 32 pixels
        else:
            assert want.sum() in (32 * (h // 2), 32 * (h // 2 + 1))         # h / 2 rows; the last one depends on that rounding
        assert (lit[i][floor & (y > 20)] == 1).all()
        top = (hit[i] >= 0) & (x == 8 + h)
        assert top.sum() == 32 and (lit[i][top] == 1).all()                 # the wall's top face
        assert (lit[i][hit[i] < 0] == 255).all() and (out[i][hit[i] < 0] == 0).all()


# -- the mapping of the light ---------------------------------------------------------------------------------------------

MAPPING_POSES = ((250.0, 30.0, 1.0), (37.0, -20.0, 1.2), (0.0, 0.0, 1.0), (120.0, 50.0, 0.9))


@pytest.mark.parametrize("low_x", [False, True])
def test_lit_faces_of_a_cube_are_those_whose_normal_is_turned_to_the_light(low_x):
    """A solid 8^3 cube in S = 32 throws no shadow on itself, so lit = [light . n > 0] with n the float64 camera normal of the
    entry face: M_lin^T e normalised, in the header's channel order (right, up, towards) = (n.z, n.y, +-n.x).  Seen from high x
    all six faces of every pose have |light . n| >= 0.05 (0.186 at the least).  Seen from low x the light's `towards` component
    changes sign and the pose (250, 30, 1.0) puts two face pairs at 0.026 and 0.048 -- both among its visible faces; the floor
    there is 0.02, still twenty times the 1 / 1023 at which rounding D could change the sign of D . e (D_a = 1023 d_a / max|d| and
    |d_a| / max|d| >= |light . n|).  No pixel is excluded under either view, so a wrong sign cannot pass."""
    S = 32
    occ = np.zeros((4, S, S, S), bool)
    occ[:, 12:20, 12:20, 12:20] = True
    poses = np.stack([pose_rad(*p) for p in MAPPING_POSES])
    light = demo_light()
    m, out, rgb, hit, face, D, lit = device_shadow(occ, poses, 64, 2, low_x=low_x, smooth=0)
    lhat = light / np.linalg.norm(light)
    seen = 0
    for b in range(4):
        M = m[b, :, :3].astype(np.float64)
        dots = []
        for fc in range(6):
            e = np.zeros(3)
            e[fc >> 1] = 1.0 if fc & 1 else -1.0
            n = M.T @ e
            n /= np.linalg.norm(n)
            dots.append(float(lhat @ np.array([n[2], n[1], -n[0] if low_x else n[0]])))
        dots = np.array(dots)
        print("pose %s low_x %s: light . n per face %s" % (MAPPING_POSES[b], low_x, np.round(dots, 3).tolist()))
        assert np.abs(dots).min() >= (0.02 if low_x else 0.05)
        ok = hit[b] >= 0
        assert ok.sum() > 200
        assert np.array_equal(lit[b][ok], (dots[face[b][ok]] > 0).astype(np.uint8))
        assert (lit[b][~ok] == 255).all()
        seen += len(np.unique(lit[b][ok]))
    assert seen > 4                                                         # some pose shows a lit and a shadowed face
    assert_same(lit, twin_lit(occ, hit, face, D, 1))
    assert_same(out, twin_bytes(rgb, lit, 0, 26, None), "bytes")


@pytest.mark.parametrize("low_x", [False, True])
def test_shadow_light_against_float64(low_x):
    import torch
    from rendernet_amd import ops
    poses = np.array([[az * np.pi / 180, el * np.pi / 180, s] for az in range(0, 360, 37) for el in (-20, 0, 30, 50)
                      for s in (0.9, 1.0, 1.2)], np.float32)
    m = ops.pose_to_affine(torch.as_tensor(poses).cuda(), 64, 128)
    for light in (None, (0, 1, 1), (0, 1, 2), (-3.0, 0.25, 1e-3)):
        D = ops.shadow_light(m, light, view_from_low_x=low_x)
        assert D.dtype is torch.int32 and D.shape == (len(poses), 3) and D.is_cuda
        want = SR.light_src_float(m.cpu().numpy(), demo_light() if light is None else light, low_x)
        err = np.abs(D.cpu().numpy() - want).max()
        print("light %s low_x %s: max |D - float64| = %.3f" % (light, low_x, err))
        assert err <= 1.0 and (np.abs(D.cpu().numpy()).max(1) == 1023).all()
    assert torch.equal(ops.shadow_light(torch.as_tensor(poses).cuda(), (0, 1, 2), S=64, new_size=128, affine=False, view_from_low_x=low_x),
                       ops.shadow_light(m, (0, 1, 2), view_from_low_x=low_x))
    bad = m[:3].clone()
    bad[0, 1, 2], bad[1, :, :3] = float("nan"), 0.0
    got = ops.shadow_light(bad, (0, 1, 1), view_from_low_x=low_x).cpu().numpy()
    assert got[0].tolist() == [0, 0, 0] and got[1].tolist() == [0, 0, 0] and np.abs(got[2]).max() == 1023


# -- models ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("bias", [0, 3])
def test_models_whole_frame(models, bias):
    """chair at (37, -20, 1.2) and bunny at (250, 30, 1.0), S = 64, N = 128, f = 1, the whole frame, the demo's light: lit on
    every pixel, and the bytes at smooth 0 and 8 -- the four corners of (bias, smooth)."""
    import torch
    from rendernet_amd import ops
    m, out0, rgb, hit, face, D, lit = device_shadow(models, MODEL_POSES, 128, 1, bias=bias, smooth=0)
    want = twin_lit(models, hit, face, D, bias)
    assert_same(lit, want, "lit, bias %d" % bias)
    assert_same(out0, twin_bytes(rgb, want, 0, 26, None), "bytes, smooth 0")
    out8 = ops.shadow_encode(torch.as_tensor(rgb).cuda(), torch.as_tensor(lit).cuda(), None, 8, 26).cpu().numpy()
    assert_same(out8, twin_bytes(rgb, want, 8, 26, None), "bytes, smooth 8")
    assert_same(device_shadow(models, MODEL_POSES, 128, 1, bias=bias, smooth=8)[1], out8, "one call")
    assert (hit >= 0).reshape(2, -1).sum(1).min() > 256
    for b, name in enumerate(("chair", "bunny")):
        s_lit, s_dark = shares(lit[b])
        print("%s bias %d: %.1f %% of the hit pixels lit, %.1f %% shadowed" % (name, bias, 100 * s_lit, 100 * s_dark))
        assert s_lit > 0.05 and s_dark > 0.05
        ok = hit[b] >= 0
        assert (out0[b][~ok] == 0).all() and (out0[b][ok] >= 26).all() and (out0[b][ok & (lit[b] == 0)] == 26).all()
        assert out0[b][ok].max() > 200 and not np.array_equal(out0[b], out8[b])


def test_window_at_the_training_resolution(models):
    """f = 4, rows 190..301 x columns 203..298 of the chair (112 x 96: partial tiles on both sides, an odd origin), default
    smoothing (4) and none.  lit is per pixel, so it equals that region of the whole 512^2 frame; the smoothed bytes do where
    the (2r+1)^2 window does not reach the border of the cast."""
    occ, poses = models[:1], pose_rad(*BUNNY_POSE)[None]
    m, out, rgb, hit, face, D, lit = device_shadow(occ, poses, 128, 4, WINDOW, smooth=4)
    assert out.shape == (1, 112, 96) and (hit >= 0).any() and (hit < 0).any()
    want = twin_lit(occ, hit, face, D, 1)
    assert_same(lit, want)
    assert_same(out, twin_bytes(rgb, want, 4, 26, None), "smooth 4")
    assert_same(device_shadow(occ, poses, 128, 4, WINDOW, smooth=0)[1], twin_bytes(rgb, want, 0, 26, None), "smooth 0")
    full = device_shadow(occ, poses, 128, 4, smooth=4)
    r0, c0, ph, pw = WINDOW
    assert np.array_equal(full[6][:, r0:r0 + ph, c0:c0 + pw], lit)
    assert np.array_equal(full[1][:, r0 + 4:r0 + ph - 4, c0 + 4:c0 + pw - 4], out[:, 4:-4, 4:-4])
    assert (lit == 0).any() and (lit == 1).any()


def test_grid_of_128_reads_the_mask_from_memory(models):
    """S = 128 (no LDS copy of the mask): the chair upsampled x2, N = 256, f = 1, a 64 x 64 window through the silhouette."""
    occ = np.repeat(np.repeat(np.repeat(models[:1], 2, 1), 2, 2), 2, 3)
    m, out, rgb, hit, face, D, lit = device_shadow(occ, pose_rad(*BUNNY_POSE)[None], 256, 1, (96, 112, 64, 64), smooth=2)
    assert (hit >= 0).mean() > 0.1 and (hit < 0).mean() > 0.1
    want = twin_lit(occ, hit, face, D, 1)
    assert_same(lit, want)
    assert_same(out, twin_bytes(rgb, want, 2, 26, None), "bytes")
    assert (lit == 0).any() and (lit == 1).any()


# -- edges of the domain --------------------------------------------------------------------------------------------------

def test_empty_and_full_items_and_an_empty_batch():
    import torch
    from rendernet_amd import ops
    occ = np.stack([np.zeros((32, 32, 32), bool), np.ones((32, 32, 32), bool), np.zeros((32, 32, 32), bool)])
    m, out, rgb, hit, face, D, lit = device_shadow(occ, np.tile(pose_rad(*BUNNY_POSE), (3, 1)), 64, 2, smooth=2)
    assert (lit[0] == 255).all() and (out[0] == 0).all() and (lit[2] == 255).all() and (out[2] == 0).all()
    assert (hit[1] >= 0).sum() > 1000
    want = twin_lit(occ, hit, face, D, 1)
    assert_same(lit, want)
    assert_same(out, twin_bytes(rgb, want, 2, 26, None), "bytes")
    ok = hit[1] >= 0
    for fc in np.unique(face[1][ok]):                                       # a box face sees nothing above it: lit iff turned to D
        turned = (1 if fc & 1 else -1) * D[1, fc >> 1] > 0
        assert (lit[1][ok & (face[1] == fc)] == int(turned)).all()
    vox = torch.zeros((0, 32, 32, 32, 1), device="cuda")
    got = ops.raycast_shadow(vox, torch.zeros((0, 3), device="cuda"), new_size=64, pixels_per_cell=2, return_parts=True)
    assert got[0].shape == (0, 128, 128) and got[5].shape == (0, 128, 128) and got[4].shape == (0, 3) and got[0].dtype is torch.uint8


def test_zero_light_shadows_everything_and_long_lights_are_clamped():
    S, q = 32, np.arange(0, 20)
    occ = np.stack([SR.wall_scene(S, 3)] * 4)
    ids, fc = SR.wall_floor_hits(S, q, 5)
    hit, face = np.tile(ids, (4, 1))[:, None, :], np.full((4, 1, len(q)), fc)
    Ds = np.array([(0, 0, 0), (5000, 4000, 0), (1023, 1023, 0), (1023, 818, 0)])
    got = from_hits(occ, hit, face, Ds, 0)
    assert (got[0] == 0).all()
    assert np.array_equal(got[1], got[2]) and not np.array_equal(got[1], got[3])    # (5000, 4000) clamps to (1023, 1023), not 5 : 4
    assert_same(got, twin_lit(occ, hit, face, Ds, 0))
    big = np.array([(2 ** 31 - 1, -2 ** 31, 7)] * 4)
    assert_same(from_hits(occ, hit, face, big, 0), twin_lit(occ, hit, face, big, 0), "int32 extremes")


def test_out_of_range_hits_and_faces_behave_as_misses(models):
    """A few hit_id >= S^3, hit_id < -1 and face = 7 / -1 entries injected into the chair's planes: 255 in lit, 0 in the bytes,
    and left out of their neighbours' means, for the kernel and the twin alike."""
    import torch
    from rendernet_amd import ops
    m, out, rgb, hit, face, D, lit = device_shadow(models[:1], MODEL_POSES[:1], 128, 1)
    hit, face = hit.copy(), face.copy()
    inside = np.argwhere(hit[0] >= 0)
    assert len(inside) > 200
    picks = inside[:: len(inside) // 8][:8]
    for k, (r, c) in enumerate(picks):
        if k % 4 == 0:
            hit[0, r, c] = 64 ** 3 + k
        elif k % 4 == 1:
            face[0, r, c] = 7
        elif k % 4 == 2:
            hit[0, r, c], face[0, r, c] = np.iinfo(np.int32).max, -1
        else:
            hit[0, r, c] = np.iinfo(np.int32).min
    got = from_hits(models[:1], hit, face, D, 1)
    want = twin_lit(models[:1], hit, face, D, 1)
    assert_same(got, want)
    for r, c in picks:
        assert got[0, r, c] == 255
    enc = ops.shadow_encode(torch.as_tensor(rgb).cuda(), torch.as_tensor(got).cuda(), None, 3, 26).cpu().numpy()
    assert_same(enc, twin_bytes(rgb, want, 3, 26, None), "bytes")
    assert all(enc[0, r, c] == 0 for r, c in picks)
    odd = got.copy()
    odd[0, picks[0][0], picks[0][1]] = 2                                    # neither 0, 1 nor 255: the encoder's miss as well
    enc2 = ops.shadow_encode(torch.as_tensor(rgb).cuda(), torch.as_tensor(odd).cuda(), None, 3, 26).cpu().numpy()
    assert_same(enc2, enc, "lit = 2")


# -- end to end -----------------------------------------------------------------------------------------------------------

def test_raycast_shadow_equals_the_staged_calls(models):
    import torch
    from rendernet_amd import ops
    vox, pose = cuda_vox(models), torch.as_tensor(MODEL_POSES).cuda()
    light = (-1.0, 2.0, 0.5)
    for low_x in (False, True):
        kw = dict(new_size=32, pixels_per_cell=4, window=(3, 5, 101, 77), view_from_low_x=low_x)
        out = ops.raycast_shadow(vox, pose, light=light, bias=2, smooth=None, ambient_byte=40, normal_radius=3, **kw)
        m = ops.pose_to_affine(pose, 64, 32)
        rgb, hit, face = ops.raycast_normals(vox, m, affine=True, normal_radius=3, return_hits=True, **kw)
        bits, box = ops.voxel_pack(vox)
        D = ops.shadow_light(m, light, view_from_low_x=low_x)
        lit = ops.raycast_shadow_from_hits(bits, box, hit, face, D, 64, 2)
        assert torch.equal(out, ops.shadow_encode(rgb, lit, light, 4, 40))   # smooth=None is pixels_per_cell
        assert out.shape == (2, 101, 77) and (lit == 0).any() and (lit == 1).any() and (lit == 255).any()
        parts = ops.raycast_shadow(vox, m, affine=True, light=light, bias=2, ambient_byte=40, normal_radius=3, return_parts=True, **kw)
        for got, want in zip(parts, (out, rgb, hit, face, D, lit)):
            assert torch.equal(got, want)
    assert not torch.equal(ops.raycast_shadow(vox, pose, new_size=32, pixels_per_cell=4),
                           ops.raycast_shadow(vox, pose, new_size=32, pixels_per_cell=4, light=light))


# -- argument checks ------------------------------------------------------------------------------------------------------

def test_invalid_arguments_return_invalid_without_a_launch():
    import torch
    from rendernet_amd import _lib, ops
    from rendernet_amd._lib import RenderNetHipError
    lib, vp, st = _lib.lib(), ctypes.c_void_p, _lib.stream_ptr()
    B, S, ph, pw = 2, 32, 20, 24
    bits, box = ops.voxel_pack(torch.ones((B, S, S, S, 1), dtype=torch.uint8, device="cuda"))
    hit = torch.zeros((B, ph, pw), dtype=torch.int32, device="cuda")       # voxel 0 by its -x face everywhere
    face = torch.zeros((B, ph, pw), dtype=torch.int8, device="cuda")
    rgb = torch.full((B, ph, pw, 3), 200, dtype=torch.uint8, device="cuda")
    m = torch.eye(3, 4, device="cuda").repeat(B, 1, 1).contiguous()
    D = torch.full((B, 4), 77, dtype=torch.int32, device="cuda")           # a spare int so that D + 1 element stays inside
    lit = torch.full((B, ph, pw), 77, dtype=torch.uint8, device="cuda")
    out = torch.full((B, ph, pw), 9, dtype=torch.uint8, device="cuda")
    p = {"bits": bits.data_ptr(), "box": box.data_ptr(), "hit": hit.data_ptr(), "face": face.data_ptr(), "D": D.data_ptr(),
         "lit": lit.data_ptr()}

    def light_fn(B=B, low_x=0, l=(0.0, 1.0, 1.0), m_ptr=m.data_ptr(), d_ptr=D.data_ptr()):
        host = (ctypes.c_float * 3)(*l) if l is not None else None
        return lib.rn_shadow_light(vp(m_ptr), ctypes.cast(host, vp) if host is not None else None, low_x, vp(d_ptr), B, st)

    def shadow(B=B, S=S, ph=ph, pw=pw, bias=1, **ptr):
        a = dict(p, **ptr)
        return lib.rn_raycast_shadow_fwd(vp(a["bits"]), vp(a["box"]), vp(a["hit"]), vp(a["face"]), vp(a["D"]), vp(a["lit"]), B, S, ph,
                                         pw, bias, st)

    def enc(B=B, ph=ph, pw=pw, smooth=2, amb=26, l=(0, 0, 32767), n=rgb.data_ptr(), src=lit.data_ptr(), dst=out.data_ptr()):
        return lib.rn_shadow_encode(vp(n), vp(src), vp(dst), B, ph, pw, smooth, amb, l[0], l[1], l[2], st)

    inf, nan = float("inf"), float("nan")
    for kw in [dict(B=-1), dict(B=65536), dict(low_x=2), dict(low_x=-1), dict(l=None), dict(l=(0.0, 0.0, 0.0)), dict(l=(nan, 1.0, 0.0)),
               dict(l=(0.0, inf, 0.0)), dict(l=(0.0, 1.0, -inf)), dict(m_ptr=None), dict(d_ptr=None), dict(m_ptr=m.data_ptr() + 2),
               dict(d_ptr=D.data_ptr() + 1)]:
        assert light_fn(**kw) == RN_E_INVALID, kw
    assert b"rn_shadow_light" in lib.rn_last_error()
    for kw in [dict(B=-1), dict(B=65536), dict(S=48), dict(S=0), dict(S=160), dict(ph=0), dict(pw=0), dict(ph=4097), dict(pw=-3),
               dict(bias=-1), dict(bias=4), dict(bits=None), dict(box=None), dict(hit=None), dict(face=None), dict(D=None), dict(lit=None),
               dict(bits=p["bits"] + 4), dict(box=p["box"] + 2), dict(hit=p["hit"] + 1), dict(D=p["D"] + 2)]:
        assert shadow(**kw) == RN_E_INVALID, kw
    assert b"rn_raycast_shadow_fwd" in lib.rn_last_error()
    for kw in [dict(B=-1), dict(B=65536), dict(ph=0), dict(pw=0), dict(pw=4097), dict(smooth=-1), dict(smooth=9), dict(amb=-1), dict(amb=255),
               dict(l=(32768, 0, 0)), dict(l=(0, -32768, 0)), dict(l=(0, 0, 1 << 20)), dict(n=None), dict(src=None), dict(dst=None),
               dict(dst=lit.data_ptr()), dict(dst=rgb.data_ptr())]:
        assert enc(**kw) == RN_E_INVALID, kw
    assert b"rn_shadow_encode" in lib.rn_last_error()
    torch.cuda.synchronize()
    assert (D == 77).all() and (lit == 77).all() and (out == 9).all()       # nothing was launched
    assert light_fn(B=0) == 0 and shadow(B=0) == 0 and enc(B=0) == 0 and shadow(B=0, bits=None) == 0 and light_fn(B=0, m_ptr=None) == 0
    assert light_fn(B=0, l=(0.0, 0.0, 0.0)) == RN_E_INVALID                 # the light is checked even for an empty batch
    torch.cuda.synchronize()
    assert (D == 77).all() and (lit == 77).all() and (out == 9).all()
    D3 = torch.full((B, 3), 77, dtype=torch.int32, device="cuda")
    assert light_fn(d_ptr=D3.data_ptr()) == 0 and shadow(D=D3.data_ptr()) == 0      # ... and the same buffers are accepted as they are
    torch.cuda.synchronize()
    assert D3.cpu().tolist() == [[1023, 1023, 0]] * B and (lit == 0).all()          # the -x face of voxel 0 is turned away from +x
    assert enc() == 0
    torch.cuda.synchronize()
    assert (out == 26).all()
    vox = torch.zeros((1, 32, 32, 32, 1), device="cuda")
    pose = torch.as_tensor(pose_rad(*BUNNY_POSE)[None]).cuda()
    for kw, msg in (({"bias": 4}, "bias"), ({"bias": -1}, "bias"), ({"smooth": 9}, "smooth"), ({"ambient_byte": 255}, "ambient_byte"),
                    ({"normal_radius": 0}, "normal_radius"), ({"bias": 1.0}, "not an integer"), ({"light": (0, 0, 0)}, "quantise_light"),
                    ({"light": (1, 2)}, "quantise_light"), ({"window": (0, 0, 0, 16)}, "window")):
        with pytest.raises(RenderNetHipError, match=msg):
            ops.raycast_shadow(vox, pose, new_size=32, pixels_per_cell=2, **kw)
    with pytest.raises(RenderNetHipError, match="hit int32"):
        ops.raycast_shadow_from_hits(bits, box, hit.long(), face, D3, S)
    with pytest.raises(RenderNetHipError, match="light_src int32"):
        ops.raycast_shadow_from_hits(bits, box, hit, face, D, S)
    with pytest.raises(RenderNetHipError, match="uint8 normals"):
        ops.shadow_encode(rgb[..., :2], lit)
    with pytest.raises(RenderNetHipError, match="three finite"):
        ops.shadow_light(m, (0, 0, 0))


# -- the trainer ----------------------------------------------------------------------------------------------------------

def test_shadow_frames_feed_the_trainer(models):
    """Greyscale frames of SyntheticTargets(shader="shadow") are ops.raycast_shadow / 255 bit for bit, colour frames carry the
    byte in three channels, and a reduced greyscale trainer (tiny_spec on 32^3 grids: 32^3 -> 32^3 -> 128^2) takes one step on
    a 32-pixel crop of them in the default multiply mode with a finite loss."""
    import torch
    from rendernet_amd import ops, synth
    from rendernet_amd.shader import init_shader_weights, tiny_spec
    from rendernet_amd.train import Trainer
    small = models.reshape(2, 32, 2, 32, 2, 32, 2).any(axis=(2, 4, 6)).astype(np.uint8)[..., None]       # 2x2x2 max-pool
    spec = dataclasses.replace(tiny_spec(1), size=32).check()
    tr = Trainer(spec, init_shader_weights(spec, seed=1234), device="cuda", e_eta=1e-4, keep_prob=1.0)
    opts = {"bias": 2, "ambient_byte": 40}
    feeds = [synth.SyntheticTargets(small, ["chair", "bunny"], 2, 1, seed=3, device="cuda", greyscale=g, new_size=32,
                                    shader="shadow", shadow_options=opts) for g in (True, False)]
    losses = []
    for (frames, vox, poses, names), (fc, vox_c, poses_c, names_c) in zip(*feeds):
        assert names == names_c and torch.equal(vox, vox_c) and torch.equal(poses, poses_c)
        byte = ops.raycast_shadow(vox, poses, new_size=32, pixels_per_cell=4, **opts).cpu().numpy()
        assert byte.shape == (2, 128, 128) and (byte >= 40).reshape(2, -1).sum(1).min() > 64 and set(np.unique(byte)) - {0, 40}
        assert frames.dtype is torch.float32 and frames.shape == (2, 128, 128, 1) and frames.is_cuda
        assert np.array_equal(frames.cpu().numpy()[..., 0], byte.astype(np.float32) / np.float32(255.0))
        assert fc.dtype is torch.uint8 and fc.shape == (2, 128, 128, 3) and fc.is_contiguous()
        assert np.array_equal(fc.cpu().numpy(), np.repeat(byte[..., None], 3, 3))
        losses.append(float(tr.step(vox, poses, frames, patch_size=8, start_point=(8, 8)).item()))
    print("losses: %s" % losses)
    assert len(losses) == 1 and np.isfinite(losses).all()
