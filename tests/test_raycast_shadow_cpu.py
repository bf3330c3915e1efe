"""The cast-shadow rule of the caster (include/rendernet_hip.h, rn_shadow_light / rn_raycast_shadow_fwd /
rn_shadow_encode) on the host: the integer twin tests/raycast_shadow_ref.py against closed forms, and the layers above the
kernels (options, synth, script, header) with the caster stubbed.  No GPU."""
import itertools
import os
import re

import numpy as np
import pytest

import raycast_shadow_ref as SR
from header_version import states_version

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
S = 32
WALL_LIGHTS = ((1, 1, 0), (1, 2, 0), (3, 2, 0), (1023, 511, 0), (2, 1, 1))
AXIS_PAIRS = [(a, sa, b, sb) for a in range(3) for b in range(3) if a != b for sa in (1, -1) for sb in (1, -1)]


def flat(x, y, z):
    return (z * S + y) * S + x


# -- the walk against closed forms ----------------------------------------------------------------------------------------

def test_lone_voxel_is_lit_on_the_faces_turned_to_the_light():
    """One voxel: nothing can shadow it, so lit = [s D_a > 0] for every D, octants and zero components alike."""
    occ = np.zeros((S, S, S), bool)
    occ[14, 12, 10] = True
    hits, faces = np.full(6, flat(10, 12, 14)), np.arange(6)
    seen = set()
    for D in itertools.product((-1023, -5, 0, 7, 1023), repeat=3):
        want = np.array([1 if ((1 if f & 1 else -1) * D[f >> 1]) > 0 else 0 for f in range(6)], np.uint8)
        for bias in (0, 1):
            assert np.array_equal(SR.shadow_lit(occ, hits, faces, D, bias), want), (D, bias)
        seen.add(tuple(want.tolist()))
    assert len(seen) == 27                                                  # every sign pattern, the all-shadowed one included
    assert not SR.shadow_lit(occ, hits, faces, (0, 0, 0)).any()


@pytest.mark.parametrize("a", [0, 1, 2])
def test_laterally_filled_slab_is_lit_from_its_side(a):
    """A slab three voxels thick that spans the grid in the other two axes: its upper face is lit for every D with D_a > 0
    (the ray leaves the box at once), its lower face for every D with D_a < 0, and neither from the other side."""
    occ_xyz = np.zeros((S, S, S), bool)
    sl = [slice(None)] * 3
    sl[a] = slice(9, 12)
    occ_xyz[tuple(sl)] = True
    occ = occ_xyz.transpose(2, 1, 0)
    other = [k for k in range(3) if k != a]
    for D_other in itertools.product((-1023, -300, 0, 1, 1023), repeat=2):
        for Da in (1, 200, 1023):
            D = np.zeros(3, np.int64)
            D[a], D[other[0]], D[other[1]] = Da, D_other[0], D_other[1]
            v_hi, v_lo = np.array([5, 5, 5]), np.array([5, 5, 5])
            v_hi[a], v_lo[a] = 11, 9
            hits = np.array([flat(*v_hi), flat(*v_lo), flat(*v_hi), flat(*v_lo)])
            faces = np.array([2 * a + 1, 2 * a, 2 * a, 2 * a + 1])          # the last two are not faces a camera ray can enter by
            assert SR.shadow_lit(occ, hits, faces, D, 0)[:2].tolist() == [1, 0], D
            assert SR.shadow_lit(occ, hits, faces, -D, 0)[:2].tolist() == [0, 1], D
            # a face inside the slab turned to the light looks into the slab: shadowed once the bias no longer covers it
            assert SR.shadow_lit(occ, hits, faces, D, 0)[3] == 0 and SR.shadow_lit(occ, hits, faces, D, 0)[2] == 0


@pytest.mark.parametrize("h", [1, 3, 5])
@pytest.mark.parametrize("Dc", WALL_LIGHTS)
def test_wall_on_a_floor(h, Dc):
    """The fifteen cases of the issue on the canonical axes (floor normal +x, wall at y0), bias 0: the floor face at y < y0 is
    shadowed exactly when D_x (2 (y0 - y) - 1) < 2 h D_y; an exact tie leaves the pixel lit."""
    occ = SR.wall_scene(S, h)
    q = np.arange(0, 20)
    hits, face = SR.wall_floor_hits(S, q, 5)
    lit = SR.shadow_lit(occ, hits, np.full(len(q), face), SR.wall_light(Dc), 0)
    want = SR.wall_shadowed(Dc, h, q)
    assert np.array_equal(lit == 0, want), (h, Dc, lit, want)
    if Dc == (1, 1, 0):
        assert want.sum() == h
    if Dc == (1, 2, 0):
        assert want.sum() == 2 * h
    # (1023, 511, 0) clears a wall of 1 (1023 / 1022 > 1) and (2, 1, 1) ties on its upper edge: no shadow at all there
    assert want.sum() < len(q) and (want.sum() > 0) == ((Dc, h) not in (((1023, 511, 0), 1), ((2, 1, 1), 1)))
    # beyond the wall the light comes from behind it: nothing in the way
    far, _ = SR.wall_floor_hits(S, np.arange(21, 32), 5)
    assert (SR.shadow_lit(occ, far, np.full(len(far), face), SR.wall_light(Dc), 0) == 1).all()


@pytest.mark.parametrize("axes", AXIS_PAIRS)
def test_wall_on_every_pair_of_axes(axes):
    """The same scene turned onto every (floor axis, wall axis) pair and mirrored: the formula holds, and an exact tie goes
    the way of the lower AXIS -- over the wall when the floor's axis is the lower one, into its top voxel otherwise."""
    a, sa, b, sb = axes
    q = np.arange(0, 20)
    ties = 0
    for h in (1, 3, 5):
        occ = SR.wall_scene(S, h, a, sa, b, sb)
        hits, face = SR.wall_floor_hits(S, q, 5, a, sa, b, sb)
        for Dc in WALL_LIGHTS + ((2, 1, 0), (2, 3, 0)):
            lit = SR.shadow_lit(occ, hits, np.full(len(q), face), SR.wall_light(Dc, a, sa, b, sb), 0)
            want = SR.wall_shadowed(Dc, h, q, a, b)
            assert np.array_equal(lit == 0, want), (axes, h, Dc)
            ties += int((Dc[0] * (2 * (20 - q) - 1) == 2 * h * Dc[1]).sum())
    assert ties == 9                                                        # (2,1,1), (2,1,0) and (2,3,0) tie once per height; odd D_x never does


def test_bias_ignores_the_staircase_next_to_the_hit():
    """A floor with one voxel on it: from the neighbouring floor voxel, under D = (1, 2, 0), the ray's second voxel is that
    step.  It is one voxel away (Chebyshev): counted at bias 0, ignored at bias 1; a step two voxels high is counted again at
    bias 1 from two voxels away, and ignored at bias 2."""
    occ = np.zeros((S, S, S), bool)
    occ[:, :, 8] = True
    occ[5, 20, 9] = True                                                    # (x, y, z) = (9, 20, 5)
    hit, face = np.array([flat(8, 19, 5)]), np.array([1])
    assert [int(SR.shadow_lit(occ, hit, face, (1, 2, 0), bias)[0]) for bias in (0, 1, 2, 3)] == [0, 1, 1, 1]
    occ[5, 20, 10] = True                                                   # the step is now two voxels high
    hit2 = np.array([flat(8, 18, 5)])                                       # climbs 1/2 per voxel of y: meets (9, 20) 2 away
    assert [int(SR.shadow_lit(occ, hit2, face, (1, 2, 0), bias)[0]) for bias in (0, 1, 2, 3)] == [0, 0, 1, 1]
    assert [int(SR.shadow_lit(occ, hit, face, (2, 2, 0), bias)[0]) for bias in (0, 1, 2)] == [0, 0, 1]   # passes through (9, 20), then (10, 20)


def test_out_of_range_hits_are_misses_and_light_is_clamped():
    occ = SR.wall_scene(S, 3)
    hits, face = SR.wall_floor_hits(S, np.arange(10, 20), 5)
    faces = np.full(10, face)
    want = SR.shadow_lit(occ, hits, faces, (1023, 1023, 0), 0)
    assert np.array_equal(SR.shadow_lit(occ, hits, faces, (5000, 4000, 0), 0), want)           # both clamp to 1023
    assert not np.array_equal(SR.shadow_lit(occ, hits, faces, (1023, 818, 0), 0), want)        # ... which 5 : 4 unclamped is not
    bad_h, bad_f = hits.copy(), faces.copy()
    bad_h[0], bad_h[1], bad_f[2], bad_f[3] = -1, S ** 3, 6, -1
    got = SR.shadow_lit(occ, bad_h, bad_f, (1023, 1023, 0), 0)
    assert (got[:4] == 255).all() and np.array_equal(got[4:], want[4:])
    empty = np.zeros((S, S, S), bool)
    assert (SR.shadow_lit(empty, hits, faces, (1, 1, 0), 0) == 1).all()     # nothing is occupied: every ray is outside the box


# -- the encoder's bytes --------------------------------------------------------------------------------------------------

def test_encoder_bytes():
    """ambient + (255 - ambient) e Sigma / (32767 * 255 n), rounded half up, at Sigma / n = 0, 1/2 and 1; the clamp; misses."""
    facing = np.array([128, 128, 255], np.uint8)                            # the normal towards the camera
    nb = np.tile(facing, (1, 2, 1))
    light = (0, 0, 32767)                                                   # e = 32767 * 255: the diffuse term is exactly 1
    assert SR.encode(nb, [[1, 0]], 0, 26, light).tolist() == [[255, 26]]
    assert SR.encode(nb, [[1, 0]], 1, 26, light).tolist() == [[141, 141]]   # 26 + (229 + 1) / 2
    assert SR.encode(nb, [[1, 0]], 1, 0, light).tolist() == [[128, 128]]    # 127.5 rounds up
    assert SR.encode(nb, [[1, 255]], 1, 26, light).tolist() == [[255, 0]]   # a miss writes 0 and is not counted in n
    assert SR.encode(nb, [[0, 255]], 8, 254, light).tolist() == [[254, 0]]
    assert SR.encode(nb, [[255, 255]], 3, 26, light).tolist() == [[0, 0]]
    away = np.tile(np.array([128, 128, 0], np.uint8), (1, 2, 1))
    assert SR.encode(away, [[1, 1]], 0, 26, light).tolist() == [[26, 26]]   # e = 0: the ambient term alone
    # half-lit diffuse: bytes (128, 128, 191) -> e = 32767 * 127; 26 + round(229 * 127 / 255) = 26 + 114
    half = np.tile(np.array([128, 128, 191], np.uint8), (1, 2, 1))
    assert SR.encode(half, [[1, 1]], 0, 26, light).tolist() == [[140, 140]]
    # the clamp: bytes need not be a unit vector, so e can exceed 32767 * 255
    corner = np.full((1, 2, 3), 255, np.uint8)
    q = SR.quantise_light((1, 1, 1))
    assert q == (18918, 18918, 18918) and 3 * 18918 * 255 > 32767 * 255
    assert SR.encode(corner, [[1, 1]], 0, 26, q).tolist() == [[255, 255]]
    assert SR.encode(corner, [[1, 1]], 0, 0, q).tolist() == [[255, 255]]
    # a window sum: 5 x 5 hits, the centre column shadowed, r = 1, clipped at the border
    lit = np.ones((5, 5), np.uint8)
    lit[:, 2] = 0
    got = SR.encode(np.tile(facing, (5, 5, 1)), lit, 1, 0, light)
    assert got[2].tolist() == [255, 170, 170, 170, 255] and got[0].tolist() == [255, 170, 170, 170, 255]   # 2/3 of 255


def test_light_quantisation_against_float64():
    """rn_shadow_light's float32 arithmetic (the twin's light_src_f32) against float64: within +-1 per component, the largest
    component exactly +-1023, on the pose matrices of a sweep and both view directions; D . e keeps the sign of light . n."""
    from oracle import resample as OR
    from rendernet_amd import synth
    from rendernet_amd.tools.Phong_shading import generate_light_pos
    poses = np.array([[az * np.pi / 180, el * np.pi / 180, s] for az in range(0, 360, 37) for el in (-20, 0, 30, 50)
                      for s in (0.9, 1.0, 1.2)], np.float32)
    M = OR.inverse_affine(poses, 64, 128).astype(np.float32)
    for light in (generate_light_pos(synth.LIGHT_ELEVATION, synth.LIGHT_AZIMUTH), (0, 1, 1), (0, 1, 2), (-3.0, 0.25, 1e-3)):
        for low_x in (False, True):
            got, want = SR.light_src_f32(M, light, low_x), SR.light_src_float(M, light, low_x)
            assert np.abs(got - want).max() <= 1.0 and (np.abs(got).max(1) == 1023).all()
            assert np.abs(got - np.rint(want)).max() <= 1
    ident = OR.inverse_affine(np.array([[np.pi / 2, 0.0, 1.0]], np.float32), 32, 64).astype(np.float32)
    assert SR.light_src_f32(ident, (0, 1, 1)).tolist() == [[1023, 1023, 0]]
    assert SR.light_src_f32(ident, (0, 1, 2)).tolist() == [[1023, 512, 0]]  # 511.5 rounds to even
    assert SR.light_src_f32(ident, (0, 1, 2), True).tolist() == [[-1023, 512, 0]]
    assert SR.light_src_f32(ident * np.float32(np.nan), (0, 1, 1)).tolist() == [[0, 0, 0]]
    assert SR.light_src_f32(ident * 0, (0, 1, 1)).tolist() == [[0, 0, 0]]


# -- options --------------------------------------------------------------------------------------------------------------

def test_ops_ranges_and_option_check():
    from rendernet_amd import ops
    from rendernet_amd._lib import RenderNetHipError
    assert ops.SHADOW_RANGES == {"normal_radius": (1, 3, 2), "bias": (0, 3, 1), "smooth": (0, 8, None), "ambient_byte": (0, 254, 26)}
    assert ops.check_shadow_options("t", bias=np.int64(3), smooth=0) == {"bias": 3, "smooth": 0}
    for bad in ({"bias": -1}, {"bias": 4}, {"smooth": 9}, {"smooth": -1}, {"ambient_byte": 255}, {"ambient_byte": -1},
                {"normal_radius": 0}, {"normal_radius": 4}, {"bias": 1.0}, {"bias": True}, {"smooth": "2"}):
        with pytest.raises(RenderNetHipError, match="|".join(bad)):
            ops.check_shadow_options("t", **bad)


def test_synth_check_shadow_options():
    from rendernet_amd import synth
    assert synth.SHADOW_SHADERS == ("shadow",)
    assert synth.SHADERS == ("normal", "phong", "ao") and synth.LINE_SHADERS == ("outline", "cel")
    assert synth.check_shadow_options(None) == {}
    got = synth.check_shadow_options({"bias": 0, "smooth": 8, "ambient_byte": 254, "normal_radius": 3, "light": [0, 1, 2]})
    assert got == {"bias": 0, "smooth": 8, "ambient_byte": 254, "normal_radius": 3, "light": (0.0, 1.0, 2.0)}
    assert synth.check_shadow_options({"smooth": None, "light": None}) == {"smooth": None}
    for bad in ({"bias": 4}, {"bias": -1}, {"smooth": 9}, {"ambient_byte": 255}, {"normal_radius": 0}, {"bias": 1.5}, {"bias": "1"},
                {"smooth": True}, {"light": [0, 0, 0]}, {"light": [1, 2]}, {"light": [1, float("nan"), 0]}, {"levels": 4},
                {"max_distance": 3}):
        with pytest.raises(ValueError, match="|".join(bad)):
            synth.check_shadow_options(bad)


def test_synthetic_shader_options_accept_shadow():
    import RenderNet_Shader as RS
    so = RS.synthetic_shader_options
    assert RS.SYNTHETIC_SHADOW_SHADERS == ("shadow",) and RS.SYNTHETIC_SHADERS == ("normal", "phong", "ao")
    assert so({}, ["cfg", "--train", "--synthetic", "--synthetic-shader", "shadow"]) == ("shadow", 16)
    assert so({"synthetic_shader": "shadow", "synthetic_ao_distance": 8}, ["cfg", "--synthetic"]) == ("shadow", 8)
    assert so({"is_greyscale": "True"}, ["cfg", "--synthetic", "--synthetic-shader", "shadow"]) == ("shadow", 16)
    assert so({"is_greyscale": "False", "synthetic_shader": "shadow"}, ["cfg", "--synthetic"]) == ("shadow", 16)
    with pytest.raises(SystemExit, match="not one of.*shadow"):
        so({}, ["cfg", "--synthetic", "--synthetic-shader", "shadows"])
    with pytest.raises(SystemExit, match="needs --synthetic"):
        so({}, ["cfg", "--train", "--synthetic-shader", "shadow"])
    assert RS.synthetic_options({}, ["cfg", "--train", "--synthetic", "--synthetic-shader", "shadow"]) == (True, 100)
    with pytest.raises(SystemExit, match=r"normal\|phong\|ao\|outline\|cel\|shadow"):
        RS.main([])


def test_synthetic_shadow_options():
    from RenderNet_Shader import synthetic_shadow_options as sh
    from rendernet_amd import synth
    assert sh({}, ["cfg", "--train", "--synthetic"]) == {}
    cfg = {"synthetic_shadow_bias": 3, "synthetic_shadow_smooth": "0", "synthetic_ambient_byte": 254, "synthetic_light": [0, 1, 2]}
    assert sh(cfg, ["cfg"]) == {"bias": 3, "smooth": 0, "ambient_byte": 254, "light": (0.0, 1.0, 2.0)}
    assert synth.check_shadow_options(sh(cfg, ["cfg"])) == sh(cfg, ["cfg"])                     # what SyntheticTargets accepts
    for key, bad, msg in (("synthetic_shadow_bias", -1, r"0\.\.3"), ("synthetic_shadow_bias", 4, r"0\.\.3"),
                          ("synthetic_shadow_smooth", 9, r"0\.\.8"), ("synthetic_shadow_smooth", -1, r"0\.\.8"),
                          ("synthetic_ambient_byte", 255, r"0\.\.254"), ("synthetic_ambient_byte", -1, r"0\.\.254"),
                          ("synthetic_shadow_bias", 1.5, "not an integer"), ("synthetic_shadow_smooth", "wide", "not an integer"),
                          ("synthetic_ambient_byte", True, "not an integer"), ("synthetic_shadow_bias", None, "not an integer"),
                          ("synthetic_light", [0, 0, 0], "three finite numbers"), ("synthetic_light", [1, 2], "three finite numbers"),
                          ("synthetic_light", "up", "three finite numbers"), ("synthetic_light", [1, "2", 3], "three finite numbers"),
                          ("synthetic_light", [1, float("inf"), 3], "three finite numbers"), ("synthetic_light", 3, "three finite numbers")):
        with pytest.raises(SystemExit, match=msg):
            sh({key: bad}, ["cfg", "--synthetic"])


# -- rendernet_amd.synth with the casters stubbed -------------------------------------------------------------------------

@pytest.fixture
def stub_casters(monkeypatch):
    import torch
    from rendernet_amd import synth
    calls = {"other": [], "shadow": []}

    def other(*args, **kw):
        calls["other"].append(args)
        raise AssertionError("not the shadow caster")

    def fake_shadow(vox, poses, new_size, pixels_per_cell, options):
        calls["shadow"].append((tuple(vox.shape), new_size, pixels_per_cell, dict(options)))
        base = (vox.reshape(vox.shape[0], -1).amax(1).float() * 20 + poses[:, 0] * 10).to(torch.uint8)   # depends on the sample
        return (base[:, None, None] + torch.arange(64, dtype=torch.uint8).reshape(1, 8, 8)).contiguous()
    for name in ("_cast", "_cast_ao", "_cast_lines"):
        monkeypatch.setattr(synth, name, other)
    monkeypatch.setattr(synth, "_cast_shadow", fake_shadow)
    return calls


def _targets(seed, rank=0, world=1, steps=3, bs=4, **kw):
    from rendernet_amd import synth
    models = np.zeros((3, 8, 8, 8, 1), np.uint8)
    models[np.arange(3), np.arange(3), 0, 0, 0] = 1 + np.arange(3)
    return synth.SyntheticTargets(models, ["chair", "teapot", "bunny"], bs, steps, seed, rank=rank, world=world, device="cpu", **kw)


def test_shadow_targets_shape_dtype_and_seed(stub_casters):
    import torch
    opts = {"bias": 2, "smooth": 0, "light": [0, 1, 1]}
    grey = list(_targets(7, shader="shadow", greyscale=True, shadow_options=opts))
    col = list(_targets(7, shader="shadow"))
    other = list(_targets(8, shader="shadow"))
    assert stub_casters["other"] == [] and len(stub_casters["shadow"]) == 9
    assert stub_casters["shadow"][0] == ((4, 8, 8, 8, 1), 128, 4, {"bias": 2, "smooth": 0, "light": (0.0, 1.0, 1.0)})
    assert stub_casters["shadow"][3][3] == {}
    for (fg, vg, pg, ng), (fc, vc, pc, nc) in zip(grey, col):
        assert ng == nc and torch.equal(pg, pc) and torch.equal(vg, vc)
        assert fg.dtype is torch.float32 and fg.shape == (4, 8, 8, 1)
        assert fc.dtype is torch.uint8 and fc.shape == (4, 8, 8, 3) and fc.is_contiguous()
        assert torch.equal(fc[..., 0], fc[..., 1]) and torch.equal(fc[..., 0], fc[..., 2])
        assert np.array_equal(fg.numpy()[..., 0], fc.numpy()[..., 0].astype(np.float32) / np.float32(255.0))   # a float32 division
    assert [n for _, _, _, n in col] != [n for _, _, _, n in other]
    names = [n for _, _, _, n in col]
    assert all(re.fullmatch(r"(chair|teapot|bunny)_p[0-9.]+_t[0-9.]+_r[0-9.]+", x) for batch in names for x in batch)


def test_pose_draw_does_not_depend_on_the_shader(monkeypatch):
    import torch
    from rendernet_amd import synth
    monkeypatch.setattr(synth, "_cast_shadow", lambda vox, *a: torch.zeros((vox.shape[0], 8, 8), dtype=torch.uint8))
    monkeypatch.setattr(synth, "_cast_ao", lambda vox, *a: torch.zeros((vox.shape[0], 8, 8), dtype=torch.uint8))
    assert [n for _, _, _, n in _targets(7, shader="shadow")] == [n for _, _, _, n in _targets(7, shader="ao")]


def test_shadow_target_shards_concatenate(stub_casters):
    whole = list(_targets(11, shader="shadow"))
    parts = [list(_targets(11, rank=r, world=2, shader="shadow")) for r in range(2)]
    for step, (f, v, p, n) in enumerate(whole):
        assert n == parts[0][step][3] + parts[1][step][3]
        assert np.array_equal(f.numpy(), np.concatenate([parts[0][step][0].numpy(), parts[1][step][0].numpy()]))
        assert np.array_equal(v.numpy(), np.concatenate([parts[0][step][1].numpy(), parts[1][step][1].numpy()]))


def test_the_real_cast_hook_routes_the_options(monkeypatch):
    from rendernet_amd import ops, synth
    seen = []
    monkeypatch.setattr(ops, "raycast_shadow", lambda vox, poses, **kw: seen.append(kw))
    opts = synth.check_shadow_options({"bias": 3, "ambient_byte": 0, "light": (1, 0, 0)})
    synth._cast_shadow(None, None, 32, 4, opts)
    assert seen == [dict(opts, new_size=32, pixels_per_cell=4)]


def test_bad_shadow_options_raise_in_the_constructor(stub_casters):
    for bad in ({"bias": 4}, {"smooth": 9}, {"ambient_byte": 255}, {"normal_radius": 4}, {"bias": 2.0}, {"light": [0, 0, 0]},
                {"line_radius": 2}):
        for shader in ("shadow", "cel", "ao"):                               # checked whichever shader draws
            with pytest.raises(ValueError, match="|".join(bad)):
                _targets(3, shader=shader, shadow_options=bad)
    with pytest.raises(ValueError, match="shader"):
        _targets(3, shader="shadows")
    ok = _targets(3, shader="shadow", greyscale=True, shadow_options={"normal_radius": 1, "bias": 0, "smooth": 8, "ambient_byte": 0})
    assert ok.shadow_options["smooth"] == 8 and _targets(3, shader="shadow").shadow_options == {}
    assert stub_casters["shadow"] == []


# -- header, binding, demo and bench --------------------------------------------------------------------------------------

def test_header_declares_and_lib_binds_the_three_entries():
    from rendernet_amd import _lib
    text = open(os.path.join(ROOT, "include", "rendernet_hip.h")).read()
    src = open(os.path.join(ROOT, "rendernet_amd", "csrc", "raycast.hip")).read()
    for name, n_params in (("rn_shadow_light", 6), ("rn_raycast_shadow_fwd", 12), ("rn_shadow_encode", 12)):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        assert params[-1] == "void* stream" and len(params) == n_params
        res, args = _lib.SIGNATURES[name]
        assert res is _lib._c_int and len(args) == n_params
        for p, t in zip(params, args):
            assert t is (_lib._c_vp if "*" in p else _lib._c_int), (name, p)
        assert 'extern "C" int %s(' % name in src
    assert states_version(text)
    for kernel in ("shadow_light_kernel", "shadow_encode_kernel"):
        assert "hipLaunchKernelGGL(%s," % kernel in src, kernel
    # the caster's two instantiations are chosen by the grid side and launched through one pointer
    body = src[src.index('extern "C" int rn_raycast_shadow_fwd('):src.index('extern "C" int rn_shadow_encode(')]
    assert "const auto kernel = S <= 64 ? raycast_shadow_kernel<true> : raycast_shadow_kernel<false>;" in body
    assert body.count("hipLaunchKernelGGL(kernel,") == 1


def test_demo_and_bench_know_the_shadow_picture():
    import importlib.util
    import RenderNet_demo
    args = RenderNet_demo.build_parser().parse_args(["--reference_shadow", "True"])
    assert args.reference_shadow is True and RenderNet_demo.build_parser().parse_args([]).reference_shadow is False
    spec = importlib.util.spec_from_file_location("raycast_bench", os.path.join(ROOT, "scripts", "raycast_bench.py"))
    bench = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(bench)
    assert callable(bench.stage_shadow)
    with pytest.raises(SystemExit):
        bench.main(["shadows"])
