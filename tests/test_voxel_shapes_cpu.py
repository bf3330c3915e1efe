"""Procedural voxel shapes without a GPU: the NumPy twin of rn_voxel_shapes (tests/voxel_shapes_ref.py) against Python's
unbounded integers and the header's bounds, closed forms of the rule, the seeded generator (rendernet_amd.synth.shape_prims),
the two synthetic feeds with caster and rasteriser stubbed, and the --synthetic-shapes option."""
import itertools
import os
import re

import numpy as np
import pytest

import voxel_shapes_ref as VR
from conftest import ROOT

BIG = 10 ** 6                                # far outside every clamp


def _grid(prims, S=32):
    return VR.voxel_shapes(np.asarray(prims)[None], S)[0, ..., 0].astype(bool)


def _rot(rng):
    q = rng.standard_normal(4)
    w, x, y, z = q / np.sqrt((q * q).sum())
    R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                  [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                  [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
    return np.rint(64 * R).astype(np.int64)


# -- the twin against unbounded integers, and the header's bounds -------------------------------------------------------

def _adversarial():
    """Single-primitive items whose words lie far outside the clamps: every clamp ends at its limit, rows (64, 64, 64) up to
    sign, semi-axes 1 and 128 in every mix that an inside test tells apart."""
    items = []
    for t in range(5):
        for a in ((0, 0, 0), (BIG, BIG, BIG), (BIG, -5, BIG), (0, BIG, 0), (BIG, BIG, 0)):
            for sc, sr in ((1, 1), (-1, 1), (1, -1)):
                R = np.full((3, 3), sr * BIG)
                items.append([VR.make_prim(t, 0, (sc * BIG,) * 3, a, R)])
    items.append([VR.make_prim(1, 0, (BIG, -BIG, BIG), (BIG, BIG, BIG), [[BIG, -BIG, BIG], [-BIG, BIG, BIG], [BIG, BIG, -BIG]])])
    return np.asarray(items, np.int32)


def test_twin_equals_unbounded_integers_and_meets_the_bounds():
    """8^3 voxels of the 64^3 grid (every ninth along each axis: both extreme layers are among them).  The twin is int64
    NumPy, which wraps silently; equality with Python integers shows that it did not, and the tracked maxima are the
    header's: reached exactly where the header derives them from the clamps, never exceeded."""
    from rendernet_amd import synth
    track = {}
    adv = _adversarial()
    assert np.array_equal(VR.voxel_shapes(adv, 64, track, stride=9), VR.voxel_shapes_exact(adv, 64, 9))
    q = 3 * 64 * 127
    assert VR.BOUNDS["q"] == q == 24384 < 1 << 15 and VR.BOUNDS["wq"] == 399507456 < 1 << 29
    assert VR.BOUNDS["ellipsoid_sum"] < 1 << 60 and VR.BOUNDS["s"] == 1189158912 < 1 << 31
    assert VR.BOUNDS["cone_lhs"] < 1 << 59 and VR.BOUNDS["torus_rhs"] < 1 << 59
    assert VR.BOUNDS["cone_rhs_root"] == 266862592 < 1 << 28 and VR.BOUNDS["cone_rhs_root"] ** 2 < 1 << 57
    assert VR.BOUNDS["torus_l"] == 1850847232 < 1.9e9 < 1 << 31 and VR.BOUNDS["torus_l"] ** 2 < 1 << 62
    assert set(track) == set(VR.BOUNDS)
    for name, bound in VR.BOUNDS.items():
        assert track[name] <= bound, name
    for name in ("q", "wq", "ellipsoid_sum", "s", "cone_lhs", "cone_rhs_root", "torus_rhs"):
        assert track[name] == VR.BOUNDS[name], name                            # the adversarial items reach the bound
    assert track["torus_l"] == VR.BOUNDS["torus_l"] - 64 * 64                    # A_1 is at least 64
    drawn = synth.shape_prims(5, np.arange(6), 64)
    track = {}
    assert np.array_equal(VR.voxel_shapes(drawn, 64, track, stride=9), VR.voxel_shapes_exact(drawn, 64, 9))
    assert track["q"] < 16384                                                  # rows of a rounded rotation: far from the bound
    rng = np.random.default_rng(3)
    garbage = rng.integers(-2 ** 31, 2 ** 31, (4, 8, 16)).astype(np.int32)
    garbage[:, :, 0] = rng.integers(0, 5, (4, 8)) | rng.integers(0, 2, (4, 8)) << 8
    assert np.array_equal(VR.voxel_shapes(garbage, 32, stride=4), VR.voxel_shapes_exact(garbage, 32, 4))


def test_noop_slots_and_word_zero():
    """A type outside 0..4 or an op outside 0..1 leaves the grid as it is; type is the low byte, op everything above it."""
    box = VR.make_prim(1, 0, a=(9, 9, 9))
    want = _grid([box])
    assert want.any()
    for word in (VR.NOOP, 5, 2 << 8, 1 | 2 << 8, -1, -256, 1 | -1 << 8, 1 << 31 - 1):
        dead = VR.make_prim(0, 0, a=(60, 60, 60))
        dead[0] = word
        assert VR.clamp(dead) is None and VR.inside_exact(dead, (1, 1, 1)) is None
        assert np.array_equal(_grid([box, dead]), want)
    assert not _grid(np.zeros((0, 16), np.int32)).any()                          # K = 0


# -- closed forms ---------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("S", [32, 64])
def test_axis_aligned_box_count(S):
    for a in ((5, 12, 2 * S), (1, 1, 1), (2, 3, 4), (S - 1, S - 2, 7)):
        n = [sum(1 for P in range(-(S - 1), S, 2) if abs(P) <= min(ai, 128)) for ai in a]
        assert int(VR.voxel_shapes(VR.make_prim(1, 0, a=a)[None, None], S).sum()) == n[0] * n[1] * n[2]


def test_sphere_is_invariant_under_the_48_signed_axis_permutations():
    g = _grid([VR.make_prim(0, 0, a=(21, 21, 21))])
    assert g.any() and not g.all()
    seen = 0
    for perm in itertools.permutations(range(3)):
        for flips in itertools.product((False, True), repeat=3):
            h = np.transpose(g, perm)
            for ax, f in enumerate(flips):
                h = np.flip(h, ax) if f else h
            assert np.array_equal(h, g)
            seen += 1
    assert seen == 48


def test_subtracting_a_primitive_from_itself_is_empty():
    rng = np.random.default_rng(0)
    for t in range(5):
        R = _rot(rng)
        a, c = (20, 9 if t == 4 else 14, 17), rng.integers(-8, 9, 3)
        assert _grid([VR.make_prim(t, 0, c, a, R)]).any()
        assert not _grid([VR.make_prim(t, 0, c, a, R), VR.make_prim(t, 1, c, a, R)]).any()


def test_slot_order_matters():
    A, B = VR.make_prim(1, 0, (-10, 0, 0), (8, 8, 8)), VR.make_prim(0, 0, (10, 0, 0), (12, 12, 12))
    C = VR.make_prim(2, 1, (12, 0, 0), (6, 6, 20))
    first, second = _grid([A, B, C]), _grid([A, C, B])                           # (A u B) \ C  against  (A \ C) u B
    assert np.array_equal(second, _grid([A, B])) and first.sum() < second.sum() and not (first & ~second).any()


def test_each_type_is_its_shape():
    """Coarse geometry of the five types at c = 0, R = 64 I: extents along the axes in voxels."""
    def extent(g, axis):
        idx = np.flatnonzero(g.any(axis=tuple(k for k in range(3) if k != axis)))
        return int(idx[0]), int(idx[-1])
    S = 32
    cyl = _grid([VR.make_prim(2, 0, a=(10, 10, 20))])                            # grid axes (z, y, x): local axis 2 is grid z = array axis 0
    assert extent(cyl, 0) == (6, 25) and extent(cyl, 1) == extent(cyl, 2) == (11, 20)
    cone = _grid([VR.make_prim(3, 0, a=(12, 12, 20))])
    rows = cone.sum(axis=(1, 2))
    # the radius at height P is 12 (20 - P) / 40; the four centres next to the axis lie sqrt(2) from it: the last layer has P = 15
    assert extent(cone, 0) == (6, 23) and rows[6] > rows[15] > rows[23] and np.all(np.diff(rows[6:26]) <= 0)
    torus = _grid([VR.make_prim(4, 0, a=(20, 6, 1))])
    assert not torus[S // 2 - 1:S // 2 + 1, S // 2 - 1:S // 2 + 1, S // 2 - 1:S // 2 + 1].any()          # the hole
    assert extent(torus, 0) == (13, 18) and extent(torus, 1) == extent(torus, 2) == (3, 28)
    ell = _grid([VR.make_prim(0, 0, a=(6, 12, 24))])
    assert extent(ell, 2) == (13, 18) and extent(ell, 1) == (10, 21) and extent(ell, 0) == (4, 27)


# -- the generator --------------------------------------------------------------------------------------------------------

def test_shape_prims_are_a_function_of_seed_and_id():
    from rendernet_amd import synth
    ids = np.array([0, 1, 0xffffffff, 0x1a2b3c4d], np.uint64)
    a, b = synth.shape_prims(7, ids), synth.shape_prims(7, ids[::-1])
    assert a.dtype == np.int32 and a.shape == (4, 8, 16) and np.array_equal(a, b[::-1])
    assert np.array_equal(synth.shape_prims(7, [0x1a2b3c4d])[0], a[3])
    assert not np.array_equal(a[0], a[1]) and not np.array_equal(synth.shape_prims(8, ids), a)
    assert not np.array_equal(synth.shape_prims(7, ids, 32), a)
    for bad in (1 << 32, -1):
        with pytest.raises((ValueError, OverflowError)):
            synth.shape_prims(7, [bad])
    with pytest.raises(ValueError):
        synth.shape_prims(7, [1], 128)


@pytest.mark.parametrize("S", [32, 64])
def test_drawn_words_lie_inside_the_clamps(S):
    from rendernet_amd import synth
    p = synth.shape_prims(11, np.arange(200), S).astype(np.int64)
    live = p[:, :, 0] != VR.NOOP
    k = live.sum(1)
    assert k.min() >= 2 and k.max() <= 6 and set(np.unique(k)) == {2, 3, 4, 5, 6}
    assert np.all(live[:, :-1] >= live[:, 1:])                                   # the live slots come first
    assert not p[~live][:, 1:].any() and np.all(p[:, 0, 0] >> 8 == 0)            # slot 0 is a union
    w = p[live]
    assert set(np.unique(w[:, 0] & 255)) == {0, 1, 2, 3, 4} and set(np.unique(w[:, 0] >> 8)) == {0, 1}
    assert np.abs(w[:, 1:4]).max() <= 64 and w[:, 4:7].min() >= 1 and w[:, 4:7].max() <= 128 and np.abs(w[:, 7:]).max() <= 64
    for row in w:                                                                # what the kernel reads is what was drawn
        t, op, c, a, R = VR.clamp(row)
        assert np.array_equal(c, row[1:4]) and np.array_equal(a, row[4:7]) and np.array_equal(R.reshape(-1), row[7:])
        assert abs(np.linalg.det(R / 64.0) - 1.0) < 0.06
        if t == 4:
            assert 4 * S // 64 <= a[1] <= max(4 * S // 64, a[0] // 2)


def test_200_drawn_grids_are_not_empty_and_keep_their_border_layers_empty():
    """Conditions on the generator, not measurements.  32^3: every voxel.  64^3: the six border layers, every voxel of
    them, and every second voxel along each axis for the fill (an occupied voxel of those is an occupied voxel)."""
    from rendernet_amd import synth
    ids = np.arange(200)
    g = VR.voxel_shapes(synth.shape_prims(1234, ids, 32), 32)[..., 0]
    assert g.reshape(200, -1).any(1).all()
    for axis in (1, 2, 3):
        assert not np.take(g, [0, 31], axis=axis).any()
    p = synth.shape_prims(1234, ids, 64)
    assert not VR.border_occupied(p, 64).any()
    assert VR.voxel_shapes(p, 64, stride=2).reshape(200, -1).any(1).all()


# -- rendernet_amd.synth with caster and rasteriser stubbed ---------------------------------------------------------------

NAMES = ["chair", "teapot", "bunny"]


@pytest.fixture
def stubs(monkeypatch):
    import torch
    from rendernet_amd import synth
    calls = {"cast": [], "shapes": []}

    def fake_cast(vox, poses, new_size, pixels_per_cell):
        calls["cast"].append(tuple(vox.shape))
        return torch.zeros((vox.shape[0], 8, 8, 3), dtype=torch.uint8)

    def fake_albedo(vox, poses, waves, code_q, base, new_size, pixels_per_cell, smooth):
        calls["cast"].append(tuple(vox.shape))
        z = torch.zeros((vox.shape[0], 8, 8, 3), dtype=torch.uint8)
        return z, z

    def fake_shapes(prims, S, device):
        calls["shapes"].append((np.array(prims), S))
        return torch.as_tensor(VR.voxel_shapes(prims, S)).to(device)
    monkeypatch.setattr(synth, "_cast", fake_cast)
    monkeypatch.setattr(synth, "_cast_albedo", fake_albedo)
    monkeypatch.setattr(synth, "_shapes", fake_shapes)
    return calls


def _models(S=32):
    models = np.zeros((3, S, S, S, 1), np.uint8)
    models[np.arange(3), np.arange(3), 0, 0, 0] = 2 + np.arange(3)               # tells the models apart, and from a shape (0 / 1)
    return models


def _targets(seed, rank=0, world=1, steps=3, bs=4, models="default", **kw):
    from rendernet_amd import synth
    models = _models() if isinstance(models, str) else models
    return synth.SyntheticTargets(models, NAMES if models is not None else (), bs, steps, seed, rank=rank, world=world, device="cpu", **kw)


def test_shapes_zero_is_the_feed_as_it_was(stubs):
    """Names, poses and voxels of shapes = 0 are those of the bare pose generator and the models it indexes; with shapes > 0 the
    poses stay what they were: the second generator leaves the first one's stream alone."""
    from rendernet_amd import synth
    models = _models()
    for seed in (7, [7, 3]):
        rng = np.random.default_rng(seed)
        plain, zero, half = list(_targets(seed)), list(_targets(seed, shapes=0.0, shape_seed=99)), list(_targets(seed, shapes=0.5))
        for (f0, v0, p0, n0), (f1, v1, p1, n1), (_, _, p2, n2) in zip(plain, zero, half):
            idx, names, poses = synth.draw_batch(rng, NAMES, 4)
            assert n0 == n1 == names and np.array_equal(p0.numpy(), poses) and np.array_equal(p1.numpy(), poses)
            assert np.array_equal(v0.numpy(), models[idx]) and np.array_equal(v1.numpy(), models[idx])
            assert np.array_equal(p2.numpy(), poses) and [n.split("_p", 1)[1] for n in n2] == [n.split("_p", 1)[1] for n in names]
    stubs["shapes"].clear()
    list(_targets(7, shapes=0.0))
    assert stubs["shapes"] == []                                                 # shapes = 0 never calls the rasteriser


def test_shapes_one_needs_no_models(stubs):
    import torch
    from rendernet_amd import synth
    batches = list(_targets(5, models=None, shapes=1.0, shape_seed=42, shape_size=32, steps=2))
    assert len(batches) == 2 and len(stubs["shapes"]) == 2                       # one rasteriser call per batch
    for (frames, vox, poses, names), (prims, S) in zip(batches, stubs["shapes"]):
        assert vox.dtype is torch.uint8 and vox.shape == (4, 32, 32, 32, 1) and poses.shape == (4, 3) and S == 32
        assert all(re.fullmatch(r"shape[0-9a-f]{8}_p[0-9.]+_t[0-9.]+_r[0-9.]+", n) for n in names)
        ids = [int(n[5:13], 16) for n in names]
        assert np.array_equal(prims, synth.shape_prims(42, ids, 32))
        assert np.array_equal(vox.numpy(), VR.voxel_shapes(synth.shape_prims(42, ids, 32), 32))
    again = list(_targets(5, models=None, shapes=1.0, shape_seed=42, shape_size=32, steps=2))
    assert [b[3] for b in again] == [b[3] for b in batches]
    other = list(_targets(5, models=None, shapes=1.0, shape_seed=43, shape_size=32, steps=2))
    assert [b[3] for b in other] == [b[3] for b in batches]                      # the ids come from `seed` ...
    assert not np.array_equal(other[0][1].numpy(), batches[0][1].numpy())        # ... the geometry from shape_seed
    assert _targets(5, models=None, shapes=1.0).shape_size == 64 and _targets(5, models=None, shapes=1.0).shape_seed == 5
    for kw in ({"shapes": 0.5}, {"shapes": 0.0}, {}):
        with pytest.raises(ValueError, match="models"):
            _targets(5, models=None, **kw)
    for bad in (-0.1, 1.5, float("nan"), True, "1"):
        with pytest.raises(ValueError, match="shapes"):
            _targets(5, shapes=bad)
    with pytest.raises(ValueError, match="side"):
        _targets(5, models=_models(8), shapes=0.5)
    with pytest.raises(ValueError, match="side"):
        _targets(5, shapes=0.5, shape_size=64)                                   # the models are 32^3


def test_mixed_feed_draws_both_kinds_and_names_round_trip(stubs):
    from rendernet_amd import synth
    from rendernet_amd.tools import data_util
    kinds = {"shape": 0, "model": 0}
    for _, vox, poses, names in _targets(3, steps=12, bs=8, shapes=0.5, shape_seed=9):
        for v, p, n in zip(vox.numpy(), poses.numpy(), names):
            assert np.array_equal(data_util.extract_param_from_names(n)[0].astype(np.float32), p)      # exact in float32
            model = n.split("_p")[0]
            if model.startswith("shape"):
                kinds["shape"] += 1
                assert np.array_equal(v[None], VR.voxel_shapes(synth.shape_prims(9, [int(model[5:], 16)], 32), 32))
            else:
                kinds["model"] += 1
                assert int(v.max()) == 2 + NAMES.index(model)
    assert kinds["shape"] >= 24 and kinds["model"] >= 24                         # 96 fair coins: 24 is 4.9 sigma from the mean


def test_shards_of_world_two_concatenate(stubs):
    for kw in ({"shapes": 0.5}, {"shapes": 1.0, "models": None, "shape_size": 32}):
        whole = list(_targets(11, **kw))
        parts = [list(_targets(11, rank=r, world=2, **kw)) for r in range(2)]
        for step, (_, v, p, n) in enumerate(whole):
            assert n == parts[0][step][3] + parts[1][step][3] and len(parts[0][step][3]) == 2
            assert np.array_equal(p.numpy(), np.concatenate([parts[0][step][2].numpy(), parts[1][step][2].numpy()]))
            assert np.array_equal(v.numpy(), np.concatenate([parts[0][step][1].numpy(), parts[1][step][1].numpy()]))
        assert any(x.startswith("shape") for b in whole for x in b[3])


def test_texture_feed_takes_the_same_arguments(stubs):
    import torch
    from rendernet_amd import synth
    colour = synth.ColourModel(1, 5)
    plain = list(synth.SyntheticTextureTargets(_models(), NAMES, 4, 2, 7, colour, device="cpu"))
    zero = list(synth.SyntheticTextureTargets(_models(), NAMES, 4, 2, 7, colour, device="cpu", shapes=0.0))
    half = list(synth.SyntheticTextureTargets(_models(), NAMES, 4, 2, 7, colour, device="cpu", shapes=0.5, shape_seed=3))
    full = list(synth.SyntheticTextureTargets(None, (), 4, 2, 7, colour, device="cpu", shapes=1.0, shape_seed=3, shape_size=32))
    for a, b, h, c in zip(plain, zero, half, full):
        assert a[5] == b[5] and all(torch.equal(x, y) for x, y in zip(a[:5], b[:5]))
        assert torch.equal(a[3], h[3]) and torch.equal(a[4], h[4])              # codes and poses: the first generator's stream
        assert c[3].shape == (4, 5) and c[4].shape == (4, 3) and c[2].dtype is torch.uint8
        ids = [int(n[5:13], 16) for n in c[5]]
        assert np.array_equal(c[2].numpy(), VR.voxel_shapes(synth.shape_prims(3, ids, 32), 32))
    assert 2 <= len(stubs["shapes"]) <= 4                                        # one call per batch that has a shape


def test_the_real_rasteriser_hook_calls_ops(monkeypatch):
    from rendernet_amd import ops, synth
    seen = []
    monkeypatch.setattr(ops, "voxel_shapes", lambda prims, S: seen.append((prims.dtype, tuple(prims.shape), S)))
    synth._shapes(synth.shape_prims(1, [2, 3], 32), 32, "cpu")
    import torch
    assert seen == [(torch.int32, (2, 8, 16), 32)]


# -- flag and config parsing, header and binding --------------------------------------------------------------------------

def test_synthetic_shape_options():
    from RenderNet_Shader import synthetic_shape_options as so
    assert so({}, ["cfg", "--train"]) == (0.0, 1234)
    assert so({}, ["cfg", "--train", "--synthetic"]) == (0.0, 1234)
    assert so({"synthetic_seed": 5}, ["cfg", "--train", "--synthetic", "--synthetic-shapes", "0.25"]) == (0.25, 5)
    assert so({"synthetic_targets": True, "synthetic_shapes": 1, "synthetic_shape_seed": 77, "synthetic_seed": 5}, ["cfg", "--train"]) == (1.0, 77)
    assert so({"synthetic_shapes": 0.5}, ["cfg", "--synthetic", "--synthetic-shapes", "1"]) == (1.0, 1234)
    assert so({"synthetic_shapes": "0.5"}, ["cfg", "--synthetic"]) == (0.5, 1234)
    for cfg, argv, msg in (({}, ["cfg", "--synthetic", "--synthetic-shapes"], "needs a value"),
                           ({}, ["cfg", "--synthetic", "--synthetic-shapes", "x"], "not a number"),
                           ({"synthetic_shapes": True}, ["cfg", "--synthetic"], "not a number"),
                           ({}, ["cfg", "--synthetic", "--synthetic-shapes", "1.5"], r"\[0, 1\]"),
                           ({}, ["cfg", "--synthetic", "--synthetic-shapes", "-0.1"], r"\[0, 1\]"),
                           ({"synthetic_shapes": float("nan")}, ["cfg", "--synthetic"], r"\[0, 1\]"),
                           ({"synthetic_shape_seed": 1.5}, ["cfg", "--synthetic"], "not an integer"),
                           ({"synthetic_shape_seed": -1}, ["cfg", "--synthetic"], "non-negative"),
                           ({}, ["cfg", "--train", "--synthetic-shapes", "0.5"], "needs --synthetic"),
                           ({"synthetic_shapes": 0.5}, ["cfg", "--train"], "needs --synthetic"),
                           ({"synthetic_shape_seed": 3}, ["cfg", "--train"], "needs --synthetic")):
        with pytest.raises(SystemExit, match=msg):
            so(cfg, argv)


def test_shapes_one_does_not_read_model_path(stubs, tmp_path):
    import RenderNet_Shader as RS
    cfg = {"model_path": str(tmp_path / "missing"), "batch_size": 2}
    got = list(RS._synthetic_batches(cfg, False, 0, 1, "cpu", 1, 3, shapes=1.0, shape_seed=4))
    assert len(got) == 1 and got[0][0].shape == (2, 64, 64, 64, 1) and all(n.startswith("shape") for n in got[0][3])
    with pytest.raises(ValueError, match="binvox"):
        list(RS._synthetic_batches(cfg, False, 0, 1, "cpu", 1, 3, shapes=0.5, shape_seed=4))
    assert "--synthetic-shapes P" in RS.__doc__
    with pytest.raises(SystemExit, match="--synthetic-shapes P"):
        RS.main([])


def test_header_declares_and_lib_binds_the_entry():
    from rendernet_amd import _lib, build
    text = open(os.path.join(ROOT, "include", "rendernet_hip.h")).read()
    src = open(os.path.join(ROOT, "rendernet_amd", "csrc", "voxel_shapes.hip")).read()
    m = re.search(r"\bint\s+rn_voxel_shapes\s*\(([^;]*)\)\s*;", text)
    params = [p.strip() for p in m.group(1).split(",")]
    assert params == ["const int* prims", "unsigned char* vox", "int B", "int K", "int S", "void* stream"]
    res, args = _lib.SIGNATURES["rn_voxel_shapes"]
    assert res is _lib._c_int and [t is _lib._c_vp for t in args] == ["*" in p for p in params]
    assert 'extern "C" int rn_voxel_shapes(' in src and "hipLaunchKernelGGL(voxel_shapes_kernel," in src
    assert "voxel_shapes.hip" in build.SOURCES
    assert re.search(r"#define\s+RN_SHAPES_MAX_PRIMS\s+8\b", text) and _lib.RN_SHAPES_MAX_PRIMS == VR.MAX_PRIMS == 8
    assert re.search(r"#define\s+RN_SHAPES_NOOP\s+255\b", text) and _lib.RN_SHAPES_NOOP == VR.NOOP == 255
    assert not re.search(r"\b(float|double)\b", re.sub(r"//[^\n]*", "", src))     # no float anywhere in the kernel file


def test_ops_voxel_shapes_checks_before_any_launch():
    import torch
    from rendernet_amd import ops
    from rendernet_amd._lib import RenderNetHipError
    for bad in (np.zeros((1, 2, 16), np.int32), torch.zeros((1, 2, 16), dtype=torch.int32)):     # not a tensor; not on the device
        with pytest.raises(RenderNetHipError):
            ops.voxel_shapes(bad, 32)


def test_demo_knows_the_shape_flags():
    import RenderNet_demo
    args = RenderNet_demo.build_parser().parse_args(["--voxel_shape", "1a2b3c4d", "--save_binvox", "x.binvox", "--shape_seed", "9"])
    assert (args.voxel_shape, args.save_binvox, args.shape_seed) == ("1a2b3c4d", "x.binvox", 9)
    none = RenderNet_demo.build_parser().parse_args([])
    assert none.voxel_shape is None and none.save_binvox is None and none.shape_seed == 1234
    for argv in (["--voxel_shape", "xyz"], ["--voxel_shape", "123456789"], ["--save_binvox", "x.binvox"]):
        with pytest.raises(SystemExit):
            RenderNet_demo.main(argv)
