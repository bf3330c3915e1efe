"""Host-side checks of the line-drawing targets: the integer twin (tests/raycast_lines_ref.py) against closed forms, the
encoding, the light quantisation, SyntheticTargets(shader="outline" | "cel") with the caster stubbed, and the script's option
parsing.  No GPU."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import raycast_lines_ref as LR
from header_version import states_version
from conftest import ROOT

S = 16                                                                     # the twin takes any grid side
F = 2                                                                      # image pixels per voxel of the hand-made hits


def flat(x, y, z):
    return (z * S + y) * S + x


def plane_hits(ph, pw, x_of_col, rows=None, cols=None):
    """Hits of a surface facing -x seen head on, F pixels per voxel: pixel (r, c) hits voxel (x_of_col(c), 3 + r // F,
    3 + c // F) by face 0; rows / cols (ranges) restrict the hits, everything else is a miss."""
    hits = np.full((ph, pw), -1, np.int64)
    faces = np.zeros((ph, pw), np.int64)
    for r in (range(ph) if rows is None else rows):
        for c in (range(pw) if cols is None else cols):
            hits[r, c] = flat(x_of_col(c), 3 + r // F, 3 + c // F)
    return hits, faces


# -- the three bits against closed forms ----------------------------------------------------------------------------------

@pytest.mark.parametrize("lr", [1, 2, 4])
def test_square_on_a_flat_slab_has_a_silhouette_ring(lr):
    """A 10 x 10 square of hits on the slab x = 5 in a 20 x 20 call: bit 1 alone, in a ring exactly lr wide on the inside."""
    occ = np.zeros((S, S, S), bool)
    occ[:, :, 5] = True
    hits, faces = plane_hits(20, 20, lambda c: 5, range(5, 15), range(5, 15))
    got = LR.edges(occ, hits, faces, normal_radius=2, line_radius=lr, depth_gap=2, crease_q=4)
    rr, cc = np.mgrid[0:20, 0:20]
    square = (rr >= 5) & (rr < 15) & (cc >= 5) & (cc < 15)
    core = (rr >= 5 + lr) & (rr < 15 - lr) & (cc >= 5 + lr) & (cc < 15 - lr)
    assert np.array_equal(got, np.where(square & ~core, LR.SILHOUETTE, 0))
    assert (got == LR.SILHOUETTE).sum() == 100 - (10 - 2 * lr) ** 2


def test_square_at_the_border_of_the_call_has_no_ring_there():
    """The same square pushed into the top-left corner of the call: pixels outside the call are no misses (the window clip)."""
    occ = np.zeros((S, S, S), bool)
    occ[:, :, 5] = True
    hits, faces = plane_hits(20, 20, lambda c: 5, range(0, 10), range(0, 10))
    got = LR.edges(occ, hits, faces, line_radius=2)
    rr, cc = np.mgrid[0:20, 0:20]
    want = (rr < 10) & (cc < 10) & ((rr >= 8) | (cc >= 8))
    assert np.array_equal(got, np.where(want, LR.SILHOUETTE, 0))
    assert got[0, 0] == 0 and got[0, 9] == LR.SILHOUETTE and got[9, 0] == LR.SILHOUETTE
    # a call that IS the square has no silhouette at all
    assert not LR.edges(occ, hits[:10, :10], faces[:10, :10], line_radius=2).any()


@pytest.mark.parametrize("lr", [1, 3])
def test_depth_step_between_two_slabs(lr):
    """Every pixel hits; the left half lies on x = 4, the right half `step` voxels deeper.  step = depth_gap: no bit 2.
    step = depth_gap + 1: bit 2 alone, lr columns wide on each side of the step."""
    gap = 2
    for step in (gap, gap + 1):
        occ = np.zeros((S, S, S), bool)
        occ[:, :, 4] = occ[:, :, 4 + step] = True                           # parallel slabs: every stencil normal is along x
        hits, faces = plane_hits(12, 16, lambda c: 4 if c < 8 else 4 + step)
        got = LR.edges(occ, hits, faces, normal_radius=1, line_radius=lr, depth_gap=gap, crease_q=4)
        cc = np.mgrid[0:12, 0:16][1]
        want = (cc >= 8 - lr) & (cc < 8 + lr) if step > gap else np.zeros((12, 16), bool)
        assert np.array_equal(got, np.where(want, LR.DEPTH, 0)), step
        assert np.array_equal(LR.edges(occ, hits, faces, normal_radius=2, line_radius=lr, depth_gap=gap), got)   # R = 2 sees the other slab: same sign


def test_crease_between_faces_of_different_axes():
    """Two half-planes entered by faces of different axes on an empty stencil (g == 0: the normal is the face's): bit 4
    within line_radius of the fold at every crease_q; one face throughout: never."""
    occ = np.zeros((S, S, S), bool)
    hits, faces = plane_hits(8, 12, lambda c: 5)
    for other in (2, 3, 4, 5, 1):                                           # 1 is the opposite face: n . n = -1
        faces2 = np.where(np.mgrid[0:8, 0:12][1] < 6, 0, other)
        for q in (0, 4, 8):
            got = LR.edges(occ, hits, faces2, line_radius=2, crease_q=q)
            cc = np.mgrid[0:8, 0:12][1]
            assert np.array_equal(got, np.where((cc >= 4) & (cc < 8), LR.CREASE, 0)), (other, q)
    for q in (0, 4, 8):
        assert not LR.edges(occ, hits, faces, line_radius=2, crease_q=q).any()


def test_crease_angle_on_either_side_of_45_degrees():
    """crease_q / 8 = cos^2 of the crease angle: pairs at 26.6, 45 and 63.4 degrees, at crease_q 0, 4, 8 and 2 (60 degrees)."""
    a = np.array([3, 0, 0])
    near, diag, far = np.array([2, 1, 0]), np.array([5, 5, 0]), np.array([1, 0, 2])
    assert [bool(LR.crease(a, n, 0)) for n in (near, diag, far)] == [False, False, False]
    assert [bool(LR.crease(a, n, 4)) for n in (near, diag, far)] == [False, False, True]      # 45 degrees itself is no crease
    assert [bool(LR.crease(a, n, 2)) for n in (near, diag, far)] == [False, False, True]      # cos^2 = 1/5 < 1/4
    assert [bool(LR.crease(a, n, 8)) for n in (near, diag, far)] == [True, True, True]
    assert not LR.crease(a, 7 * a, 8) and LR.crease(a, -a, 0) and LR.crease(a, np.array([0, 4, 0]), 0)
    big = np.array([294, 294, 294])                                         # the largest stencil normal: no overflow in int64
    assert not LR.crease(big, big, 8) and LR.crease(big, np.array([294, 294, 293]), 8)
    # through edge_bits on hand-made normals: the same answers per pixel pair
    ok = np.ones((1, 2), bool)
    v = np.zeros((1, 2, 3), np.int64)
    for n, q, want in ((near, 4, 0), (far, 4, LR.CREASE), (near, 8, LR.CREASE), (far, 0, 0)):
        got = LR.edge_bits(ok, v, np.stack([a, n])[None], 1, 2, q)
        assert got.tolist() == [[want, want]], (n, q)


def test_stencil_normal_is_the_casters():
    """The twin's normal is raycast_ref's rule: a solid half-space x >= 8 gives -g along -x; invalid hits give none."""
    occ = np.zeros((S, S, S), bool)
    occ[:, :, 8:] = True
    hits = np.array([[flat(8, 7, 7), -1, S ** 3, flat(8, 7, 7)]])
    ok, v, n = LR.stencil_normals(occ, hits, np.array([[0, 0, 0, 6]]), 2)
    assert ok.tolist() == [[True, False, False, False]] and v[0, 0].tolist() == [8, 7, 7]
    assert n[0, 0].tolist() == [-(1 + 2) * 25, 0, 0] and not n[0, 1:].any()
    assert LR.edges(occ, hits, np.array([[0, 0, 0, 6]]), line_radius=4).tolist() == [[LR.SILHOUETTE, 0, 0, 0]]


# -- encoding -------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("shadow", [0, 64])
def test_byte_table_of_every_level_count(shadow):
    """Light straight at the camera: d = 32767 (2 b2 - 255).  Every band occurs; band 0 is shadow_byte, band K - 1 is 255,
    the tones between are the rationals shadow + (255 - shadow) band / (K - 1) rounded half up."""
    b2 = np.arange(256)
    normals = np.stack([np.full(256, 128), np.full(256, 128), b2], 1).astype(np.uint8)
    for K in range(2, 9):
        got = LR.encode(normals, np.zeros(256, np.uint8), levels=K, shadow_byte=shadow, light_q=(0, 0, 32767))
        bands = np.minimum(K - 1, (K * np.maximum(2 * b2 - 255, 0)) // 255)
        assert sorted(set(bands.tolist())) == list(range(K))
        want = [int(shadow + Fraction((255 - shadow) * int(j), K - 1) + Fraction(1, 2)) for j in bands]
        assert got.tolist() == want, K
        assert got[0] == shadow and got[127] == shadow and got[255] == 255
        assert LR.tone(np.arange(K), K, shadow).tolist() == sorted(set(want))
    assert LR.tone(np.arange(4), 4, 64).tolist() == [64, 128, 191, 255]


def test_outline_ink_mask_and_background():
    normals = np.array([[0, 0, 0], [128, 128, 255], [128, 128, 255], [1, 0, 0], [128, 128, 255]], np.uint8)
    edge = np.array([7, 0, 5, 2, 2], np.uint8)
    assert LR.encode(normals, edge, edge_mask=7, levels=0).tolist() == [255, 255, 0, 0, 0]       # a miss stays white whatever its bits
    for bit, want in ((1, [255, 255, 0, 255, 255]), (2, [255, 255, 255, 0, 0]), (4, [255, 255, 0, 255, 255])):
        assert LR.encode(normals, edge, edge_mask=bit, levels=0).tolist() == want, bit
    cel = LR.encode(normals, edge, edge_mask=1, levels=4, shadow_byte=64, light_q=(0, 0, 32767))
    assert cel.tolist() == [255, 255, 0, 64, 255]                           # ink wins over the tone; (1,0,0) faces away: shadow
    away = LR.encode(normals, np.zeros(5, np.uint8), levels=2, shadow_byte=10, light_q=(0, 0, -32767))
    assert away.tolist() == [255, 10, 10, 255, 10]


# -- the light ------------------------------------------------------------------------------------------------------------

def test_quantise_light_against_hand_values():
    from rendernet_amd import ops, synth
    from rendernet_amd._lib import RenderNetHipError
    from rendernet_amd.tools.Phong_shading import generate_light_pos
    for q in (ops.quantise_light, LR.quantise_light):
        assert q([0, 0, 2]) == (0, 0, 32767) and q([0, -5.0, 0]) == (0, -32767, 0)
        assert q([3, 4, 0]) == (19660, 26214, 0)                            # 32767 * 0.6 = 19660.2, * 0.8 = 26213.6
        assert q([1, 1, 1]) == (18918, 18918, 18918)                        # 32767 / sqrt 3 = 18918.03
        assert q(np.array([[1.0, -2.0, 2.0]])) == (10922, -21845, 21845)    # 32767 / 3 = 10922.33, * 2 = 21844.67
    demo = generate_light_pos(synth.LIGHT_ELEVATION, synth.LIGHT_AZIMUTH)
    e, a = np.deg2rad(60.0), np.deg2rad(250.0)
    want = tuple(int(np.rint(32767 * c)) for c in (-np.sin(e) * np.cos(a), np.cos(e), -np.sin(e) * np.sin(a)))
    assert ops.quantise_light(demo) == LR.quantise_light(demo) == want == (9706, 16384, 26666)
    for bad in ([0, 0, 0], [1, 2], [1, np.nan, 0], [np.inf, 0, 0]):
        with pytest.raises(RenderNetHipError, match="quantise_light"):
            ops.quantise_light(bad)


@pytest.mark.parametrize("K", [4, 8])
def test_integer_band_is_the_float_band_away_from_band_edges(K):
    """All 18^3 byte triples of the lattice {0, 15, .., 255}^3 under the demo's light: the integer band (15-bit light) equals
    floor(K max(d, 0)) of the unquantised float64 light wherever K d is further than 1e-3 from an integer.  Quantising the light
    moves K d by less than 8 * 3 * 2^-16 < 4e-4.  The share left out is a condition: at most 1 % of the lattice points with
    d > 0.  Observed: K = 4: 6 of 2916 points (0.21 %); K = 8: 7 of 2916 (0.24 %); no disagreement even among those."""
    from rendernet_amd import synth
    from rendernet_amd.tools.Phong_shading import generate_light_pos
    light = generate_light_pos(synth.LIGHT_ELEVATION, synth.LIGHT_AZIMUTH)
    lat = np.arange(0, 256, 15)
    tri = np.stack(np.meshgrid(lat, lat, lat, indexing="ij"), -1).reshape(-1, 3).astype(np.uint8)
    assert len(tri) == 18 ** 3
    kd, want = LR.band_float(tri, light, K)
    got = LR.band(tri, LR.quantise_light(light), K)
    lit = kd > 0
    near = lit & (np.abs(kd - np.rint(kd)) <= 1e-3)
    print("K=%d: %d of %d lit lattice points within 1e-3 of a band edge (%.3f %%), %d of them disagree"
          % (K, near.sum(), lit.sum(), 100.0 * near.sum() / lit.sum(), (got != want)[near].sum()))
    assert lit.sum() > 2000 and near.sum() <= 0.01 * lit.sum()
    assert np.array_equal(got[~near], want[~near])
    assert set(got.tolist()) == set(range(K))
    qd = sum(LR.quantise_light(light)[k] * (2 * tri[:, k].astype(np.int64) - 255) for k in range(3)) * K / (32767.0 * 255.0)
    assert np.abs(qd - kd).max() < 4e-4


# -- rendernet_amd.synth with the casters stubbed -------------------------------------------------------------------------

@pytest.fixture
def stub_casters(monkeypatch):
    import torch
    from rendernet_amd import synth
    calls = {"normal": [], "ao": [], "lines": []}

    def fake(vox, poses, new_size, pixels_per_cell):
        calls["normal"].append(tuple(vox.shape))
        return torch.zeros((vox.shape[0], 8, 8, 3), dtype=torch.uint8)

    def fake_ao(vox, poses, new_size, pixels_per_cell, max_distance):
        calls["ao"].append(tuple(vox.shape))
        return torch.zeros((vox.shape[0], 8, 8), dtype=torch.uint8)

    def fake_lines(vox, poses, new_size, pixels_per_cell, shader, options):
        calls["lines"].append((tuple(vox.shape), new_size, pixels_per_cell, shader, dict(options)))
        # a picture that depends on the sample (its model tag and pose) and on the shader
        base = (vox.reshape(vox.shape[0], -1).amax(1).float() * 20 + poses[:, 0] * 10).to(torch.uint8) + (64 if shader == "cel" else 0)
        return (base[:, None, None] + torch.arange(64, dtype=torch.uint8).reshape(1, 8, 8)).contiguous()
    monkeypatch.setattr(synth, "_cast", fake)
    monkeypatch.setattr(synth, "_cast_ao", fake_ao)
    monkeypatch.setattr(synth, "_cast_lines", fake_lines)
    return calls


def _targets(seed, rank=0, world=1, steps=3, bs=4, **kw):
    from rendernet_amd import synth
    models = np.zeros((3, 8, 8, 8, 1), np.uint8)
    models[np.arange(3), np.arange(3), 0, 0, 0] = 1 + np.arange(3)
    return synth.SyntheticTargets(models, ["chair", "teapot", "bunny"], bs, steps, seed, rank=rank, world=world, device="cpu", **kw)


@pytest.mark.parametrize("shader", ["outline", "cel"])
def test_line_targets_shape_dtype_and_seed(stub_casters, shader):
    import torch
    opts = {"line_radius": 3, "levels": 5, "light": [0, 1, 1]}
    grey = list(_targets(7, shader=shader, greyscale=True, line_options=opts))
    col = list(_targets(7, shader=shader))
    other = list(_targets(8, shader=shader))
    assert stub_casters["normal"] == [] and stub_casters["ao"] == [] and len(stub_casters["lines"]) == 9
    assert stub_casters["lines"][0] == ((4, 8, 8, 8, 1), 128, 4, shader, {"line_radius": 3, "levels": 5, "light": (0.0, 1.0, 1.0)})
    assert stub_casters["lines"][3][4] == {}
    for (fg, vg, pg, ng), (fc, vc, pc, nc) in zip(grey, col):
        assert ng == nc and torch.equal(pg, pc) and torch.equal(vg, vc)
        assert fg.dtype is torch.float32 and fg.shape == (4, 8, 8, 1)
        assert fc.dtype is torch.uint8 and fc.shape == (4, 8, 8, 3) and fc.is_contiguous()
        assert torch.equal(fc[..., 0], fc[..., 1]) and torch.equal(fc[..., 0], fc[..., 2])
        assert np.array_equal(fg.numpy()[..., 0], fc.numpy()[..., 0].astype(np.float32) / np.float32(255.0))   # a float32 division
    assert [n for _, _, _, n in col] != [n for _, _, _, n in other]
    assert [n for _, _, _, n in col] == [n for _, _, _, n in _targets(7, shader="ao")]           # the pose draw does not depend on the shader


def test_line_target_shards_concatenate(stub_casters):
    whole = list(_targets(11, shader="cel"))
    parts = [list(_targets(11, rank=r, world=2, shader="cel")) for r in range(2)]
    for step, (f, v, p, n) in enumerate(whole):
        assert n == parts[0][step][3] + parts[1][step][3]
        assert np.array_equal(f.numpy(), np.concatenate([parts[0][step][0].numpy(), parts[1][step][0].numpy()]))
        assert np.array_equal(v.numpy(), np.concatenate([parts[0][step][1].numpy(), parts[1][step][1].numpy()]))


def test_the_real_cast_hook_routes_the_options(monkeypatch):
    """synth._cast_lines itself: "cel" passes every option on, "outline" drops the cel-only ones."""
    from rendernet_amd import ops, synth
    seen = []
    monkeypatch.setattr(ops, "raycast_cel", lambda vox, poses, **kw: seen.append(("cel", kw)))
    monkeypatch.setattr(ops, "raycast_outline", lambda vox, poses, **kw: seen.append(("outline", kw)))
    opts = synth.check_line_options({"depth_gap": 3, "levels": 2, "shadow_byte": 0, "light": (1, 0, 0), "edge_mask": 5})
    synth._cast_lines(None, None, 32, 4, "cel", opts)
    synth._cast_lines(None, None, 32, 4, "outline", opts)
    assert seen[0] == ("cel", dict(opts, new_size=32, pixels_per_cell=4))
    assert seen[1] == ("outline", {"depth_gap": 3, "edge_mask": 5, "new_size": 32, "pixels_per_cell": 4})


def test_bad_line_options_raise_in_the_constructor(stub_casters):
    from rendernet_amd import synth
    assert synth.LINE_SHADERS == ("outline", "cel") and synth.SHADERS == ("normal", "phong", "ao")
    for bad in ({"line_radius": 0}, {"line_radius": 5}, {"normal_radius": 4}, {"depth_gap": 0}, {"depth_gap": 128}, {"crease_q": -1},
                {"crease_q": 9}, {"edge_mask": 0}, {"edge_mask": 8}, {"levels": 1}, {"levels": 9}, {"levels": 0}, {"shadow_byte": 255},
                {"shadow_byte": -1}, {"line_radius": 2.0}, {"levels": "4"}, {"crease_q": True}, {"light": [0, 0, 0]},
                {"light": [1, 2]}, {"smooth": 2}):
        for shader in ("outline", "cel", "ao"):                              # checked whichever shader draws
            with pytest.raises(ValueError, match="|".join(bad)):
                _targets(3, shader=shader, line_options=bad)
    with pytest.raises(ValueError, match="shader"):
        _targets(3, shader="toon")
    with pytest.raises(ValueError, match="shader"):
        _targets(3, shader="contour")
    ok = _targets(3, shader="cel", greyscale=True, line_options={"normal_radius": 3, "line_radius": 4, "depth_gap": 127, "crease_q": 0,
                                                                  "edge_mask": 1, "levels": 8, "shadow_byte": 254})
    assert ok.line_options["depth_gap"] == 127 and _targets(3, shader="outline").line_options == {}
    assert stub_casters["lines"] == []


# -- flag and config parsing ----------------------------------------------------------------------------------------------

def test_synthetic_shader_options_accept_the_line_shaders():
    from RenderNet_Shader import synthetic_options, synthetic_shader_options as so
    for name in ("outline", "cel"):
        assert so({}, ["cfg", "--train", "--synthetic", "--synthetic-shader", name]) == (name, 16)
        assert so({"synthetic_shader": name, "synthetic_ao_distance": 8}, ["cfg", "--synthetic"]) == (name, 8)
        assert so({"is_greyscale": "True"}, ["cfg", "--synthetic", "--synthetic-shader", name]) == (name, 16)
        assert so({"is_greyscale": "False", "synthetic_shader": name}, ["cfg", "--synthetic"]) == (name, 16)
    for cfg, argv in (({}, ["cfg", "--synthetic", "--synthetic-shader", "toon"]), ({"synthetic_shader": "contour"}, ["cfg", "--synthetic"]),
                      ({}, ["cfg", "--synthetic", "--synthetic-shader", "lines"])):
        with pytest.raises(SystemExit, match="not one of"):
            so(cfg, argv)
    with pytest.raises(SystemExit, match="needs --synthetic"):
        so({}, ["cfg", "--train", "--synthetic-shader", "cel"])
    assert synthetic_options({}, ["cfg", "--train", "--synthetic", "--synthetic-shader", "cel"]) == (True, 100)


def test_synthetic_line_options():
    from RenderNet_Shader import synthetic_line_options as lo
    from rendernet_amd import synth
    assert lo({}, ["cfg", "--train", "--synthetic"]) == {"line_radius": 2, "depth_gap": 2, "crease_q": 4, "levels": 4}
    cfg = {"synthetic_line_radius": 4, "synthetic_depth_gap": "127", "synthetic_crease_q": 0, "synthetic_cel_levels": 8}
    assert lo(cfg, ["cfg"]) == {"line_radius": 4, "depth_gap": 127, "crease_q": 0, "levels": 8}
    assert synth.check_line_options(lo(cfg, ["cfg"])) == lo(cfg, ["cfg"])                       # what SyntheticTargets accepts
    assert lo({"synthetic_line_radius": 1, "synthetic_depth_gap": 1, "synthetic_crease_q": 8, "synthetic_cel_levels": 2}, [])["levels"] == 2
    for key, bad, msg in (("synthetic_line_radius", 0, r"1\.\.4"), ("synthetic_line_radius", 5, r"1\.\.4"),
                          ("synthetic_depth_gap", 0, r"1\.\.127"), ("synthetic_depth_gap", 128, r"1\.\.127"),
                          ("synthetic_crease_q", -1, r"0\.\.8"), ("synthetic_crease_q", 9, r"0\.\.8"),
                          ("synthetic_cel_levels", 0, r"2\.\.8"), ("synthetic_cel_levels", 1, r"2\.\.8"), ("synthetic_cel_levels", 9, r"2\.\.8"),
                          ("synthetic_line_radius", 2.5, "not an integer"), ("synthetic_depth_gap", "deep", "not an integer"),
                          ("synthetic_crease_q", True, "not an integer"), ("synthetic_cel_levels", None, "not an integer")):
        with pytest.raises(SystemExit, match=msg):
            lo({key: bad}, ["cfg", "--synthetic"])


# -- header and binding ---------------------------------------------------------------------------------------------------

def test_header_declares_and_lib_binds_both_entries():
    from rendernet_amd import _lib
    text = open(os.path.join(ROOT, "include", "rendernet_hip.h")).read()
    for name, n_ptr, n_int in (("rn_raycast_edges_fwd", 5, 8), ("rn_lines_encode", 3, 9)):
        m = re.search(r"\bint\s+%s\s*\(([^;]*)\)\s*;" % name, text)
        assert m, name
        params = [p.strip() for p in m.group(1).split(",")]
        assert params[-1] == "void* stream" and len(params) == n_ptr + n_int + 1
        assert sum("*" in p for p in params[:-1]) == n_ptr and sum(p.startswith("int ") for p in params) == n_int
        res, args = _lib.SIGNATURES[name]
        assert res is _lib._c_int and args == [_lib._c_vp] * n_ptr + [_lib._c_int] * n_int + [_lib._c_vp]
    assert states_version(text)
    src = open(os.path.join(ROOT, "rendernet_amd", "csrc", "raycast.hip")).read()
    assert 'extern "C" int rn_raycast_edges_fwd(' in src and 'extern "C" int rn_lines_encode(' in src
    assert src.count("source_normal<LDS>(") == 2                             # one stencil, called by the caster and by the edge kernel
