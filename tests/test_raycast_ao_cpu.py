"""Host-side checks of the ambient-occlusion caster: the direction table (scripts/gen_ao_dirs.py, csrc/ao_dirs.h), closed
forms and the encoding on the float64 reference (tests/raycast_ao_ref.py), SyntheticTargets(shader="ao") with the caster
stubbed, and the --synthetic-shader parsing.  No GPU."""
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import raycast_ao_ref as AR
from conftest import BINVOX_DIR, ROOT
from scripts import gen_ao_dirs as GEN

# -- the table ------------------------------------------------------------------------------------------------------------

def test_table_is_a_cosine_weighted_hemisphere():
    T = AR.dirs()
    assert T.shape == (64, 3) and T.dtype == np.float32 and GEN.RAYS == 64
    assert np.abs(np.linalg.norm(T.astype(np.float64), axis=1) - 1.0).max() <= 1e-6
    assert (T[:, 0] > 0).all()
    assert abs(float(T[:, 0].astype(np.float64).mean()) - 2.0 / 3.0) <= 1e-3       # E[cos] under a cosine-weighted density


def test_every_direction_passes_the_tie_screen():
    """Written out here independently of the generator's own screen: all crossings up to 32 / max|T_k| + 1, pairwise."""
    for t in AR.dirs().astype(np.float64):
        a = np.abs(t)
        tmax = 32.0 / a.max() + 1.0
        per_axis = [[j / a[0] for j in range(1, 200) if j / a[0] <= tmax]]
        for k in (1, 2):
            per_axis.append([(j + 0.5) / a[k] for j in range(0, 200) if (j + 0.5) / a[k] <= tmax])
        for p in range(3):
            for q in range(p + 1, 3):
                if not per_axis[p] or not per_axis[q]:                               # a near-zero component never crosses in range
                    continue
                gap = np.abs(np.subtract.outer(per_axis[p], per_axis[q])).min()
                assert gap >= 1e-3, (t, p, q, gap)
        assert GEN.tie_gap(t.astype(np.float32)) >= 1e-3


def test_header_is_bit_equal_to_the_table():
    text = open(os.path.join(ROOT, "rendernet_amd", "csrc", "ao_dirs.h")).read()
    body = text[text.index("rn_ao_dirs[RN_AO_DIRS_COUNT][3] = {"):]
    lits = re.findall(r"(-?0x[0-9a-f.]+p[-+]?\d+)f", body)
    assert len(lits) == 64 * 3
    vals = np.array([float.fromhex(x) for x in lits], np.float64)
    assert np.array_equal(vals.astype(np.float32).astype(np.float64), vals)         # each literal is a float32 exactly
    assert np.array_equal(vals.astype(np.float32).view(np.uint32).reshape(64, 3), AR.dirs().view(np.uint32))
    assert re.search(r"#define\s+RN_AO_RAYS\s+64\b", open(os.path.join(ROOT, "include", "rendernet_hip.h")).read())


# -- closed forms on the reference ----------------------------------------------------------------------------------------

def test_closed_forms():
    seen = set()
    for name, occ, hits, faces, L, want in AR.closed_form_cases():
        for h in hits:
            assert occ.reshape(-1)[h], name                                          # the hit voxel is occupied
        got = AR.ao_counts(occ, np.array(hits), np.array(faces), L)
        assert got.tolist() == want, (name, got.tolist(), want)
        seen.update(want)
    assert len(seen - {0, 64}) >= 4                                                  # the inequalities are not vacuous


def test_misses_and_invalid_hits_have_no_count():
    occ = np.zeros((AR.S,) * 3, bool)
    occ[10, 11, 12] = True
    got = AR.ao_counts(occ, np.array([-1, AR.flat(12, 11, 10), AR.S ** 3, AR.flat(12, 11, 10)]), np.array([0, 3, 0, 6]), 4)
    assert got.tolist() == [255, 64, 255, 255]


def test_float32_walk_visits_the_same_voxels():
    """What the tie screen is for, on a model: the reference evaluated with float32 crossings (the kernel's roundings) gives
    the float64 counts on every face the chair shows at the demo pose."""
    import raycast_ref as RR
    from oracle import resample as OR
    from oracle.io_phong import read_binvox
    occ = read_binvox(os.path.join(BINVOX_DIR, "chair.binvox")).astype(bool)
    M = OR.inverse_affine(np.array([[250.0 * np.pi / 180.0, 30.0 * np.pi / 180.0, 1.0]], np.float32), size=64, new_size=128)[0]
    hit, face, _ = RR.cast(occ, M, 128, 1)
    for L in (16, 32):
        c64 = AR.ao_counts(occ, hit, face, L)
        assert np.array_equal(c64, AR.ao_counts(occ, hit, face, L, np.float32))
        inside = c64[hit >= 0]
        assert (c64[hit < 0] == 255).all() and inside.max() == 64 and inside.min() < 32 and len(np.unique(inside)) > 20


# -- encoding -------------------------------------------------------------------------------------------------------------

def test_encode_smooth_zero():
    assert AR.encode(np.array([[0, 32, 64, 255, 1, 63]], np.uint8), 0).tolist() == [[0, 128, 255, 0, 4, 251]]
    every = AR.encode(np.arange(65, dtype=np.uint8)[None], 0)[0]
    assert every.tolist() == [int(Fraction(255 * c, 64) + Fraction(1, 2)) for c in range(65)]


@pytest.mark.parametrize("r", [1, 2, 8])
def test_encode_against_rationals(r):
    rng = np.random.default_rng(r)
    c = rng.integers(0, 65, (21, 13)).astype(np.uint8)
    c[rng.random(c.shape) < 0.4] = 255
    c[0, 0], c[20, 12] = 7, 255
    got = AR.encode(c, r)
    for y in range(c.shape[0]):
        for x in range(c.shape[1]):
            if c[y, x] > 64:
                assert got[y, x] == 0
                continue
            win = c[max(y - r, 0):y + r + 1, max(x - r, 0):x + r + 1]
            n, tot = int((win <= 64).sum()), int(win[win <= 64].sum())
            assert got[y, x] == int(Fraction(255 * tot, 64 * n) + Fraction(1, 2)), (y, x)     # floor(mean byte + 1/2)
    assert np.array_equal(AR.encode(np.stack([c, c]), r), np.stack([got, got]))


# -- rendernet_amd.synth with both casters stubbed ------------------------------------------------------------------------

@pytest.fixture
def stub_casters(monkeypatch):
    import torch
    from rendernet_amd import synth
    calls = {"normal": [], "ao": []}

    def fake(vox, poses, new_size, pixels_per_cell):
        calls["normal"].append(tuple(vox.shape))
        return torch.zeros((vox.shape[0], 8, 8, 3), dtype=torch.uint8)

    def fake_ao(vox, poses, new_size, pixels_per_cell, max_distance):
        calls["ao"].append((tuple(vox.shape), new_size, pixels_per_cell, max_distance))
        # a picture that depends on the sample: its model tag and pose
        base = (vox.reshape(vox.shape[0], -1).amax(1).float() * 20 + poses[:, 0] * 10).to(torch.uint8)
        return (base[:, None, None] + torch.arange(64, dtype=torch.uint8).reshape(1, 8, 8)).contiguous()
    monkeypatch.setattr(synth, "_cast", fake)
    monkeypatch.setattr(synth, "_cast_ao", fake_ao)
    return calls


def _targets(seed, rank=0, world=1, steps=3, bs=4, **kw):
    from rendernet_amd import synth
    models = np.zeros((3, 8, 8, 8, 1), np.uint8)
    models[np.arange(3), np.arange(3), 0, 0, 0] = 1 + np.arange(3)
    return synth.SyntheticTargets(models, ["chair", "teapot", "bunny"], bs, steps, seed, rank=rank, world=world, device="cpu", **kw)


def test_ao_targets_shape_dtype_and_seed(stub_casters):
    import torch
    grey = list(_targets(7, shader="ao", greyscale=True, ao_distance=9))
    col = list(_targets(7, shader="ao"))
    other = list(_targets(8, shader="ao"))
    assert stub_casters["normal"] == [] and len(stub_casters["ao"]) == 9
    assert stub_casters["ao"][0] == ((4, 8, 8, 8, 1), 128, 4, 9) and stub_casters["ao"][3][3] == 16
    for (fg, vg, pg, ng), (fc, vc, pc, nc) in zip(grey, col):
        assert ng == nc and torch.equal(pg, pc) and torch.equal(vg, vc)
        assert fg.dtype is torch.float32 and fg.shape == (4, 8, 8, 1)
        assert fc.dtype is torch.uint8 and fc.shape == (4, 8, 8, 3) and fc.is_contiguous()
        assert torch.equal(fc[..., 0], fc[..., 1]) and torch.equal(fc[..., 0], fc[..., 2])
        assert np.array_equal(fg.numpy()[..., 0], fc.numpy()[..., 0].astype(np.float32) / np.float32(255.0))   # a float32 division
    assert [n for _, _, _, n in col] != [n for _, _, _, n in other]


def test_ao_target_shards_concatenate(stub_casters):
    whole = list(_targets(11, shader="ao"))
    parts = [list(_targets(11, rank=r, world=2, shader="ao")) for r in range(2)]
    for step, (f, v, p, n) in enumerate(whole):
        assert n == parts[0][step][3] + parts[1][step][3]
        assert np.array_equal(f.numpy(), np.concatenate([parts[0][step][0].numpy(), parts[1][step][0].numpy()]))
        assert np.array_equal(v.numpy(), np.concatenate([parts[0][step][1].numpy(), parts[1][step][1].numpy()]))


def test_default_and_named_shaders_use_only_the_normal_caster(stub_casters):
    import torch
    for kw in ({}, {"shader": None}, {"shader": "normal"}):
        frames = next(_targets(3, steps=1, **kw))[0]
        assert frames.dtype is torch.uint8 and frames.shape == (4, 8, 8, 3)
    assert len(stub_casters["normal"]) == 3 and stub_casters["ao"] == []
    from rendernet_amd import synth
    with pytest.raises(ValueError, match="shader"):
        _targets(3, shader="toon")
    with pytest.raises(ValueError, match="greyscale"):
        _targets(3, shader="phong")
    with pytest.raises(ValueError, match="greyscale"):
        _targets(3, shader="normal", greyscale=True)
    with pytest.raises(ValueError, match="ao_distance"):
        _targets(3, shader="ao", ao_distance=33)
    assert synth.SHADERS == ("normal", "phong", "ao")


# -- flag and config parsing ----------------------------------------------------------------------------------------------

def test_synthetic_shader_options():
    from RenderNet_Shader import synthetic_options, synthetic_shader_options as so
    assert so({}, ["cfg", "--train"]) == (None, 16)
    assert so({}, ["cfg", "--train", "--synthetic"]) == (None, 16)
    assert so({}, ["cfg", "--train", "--synthetic", "--synthetic-shader", "ao"]) == ("ao", 16)
    assert so({"synthetic_targets": True}, ["cfg", "--train", "--synthetic-shader", "normal"]) == ("normal", 16)
    assert so({"synthetic_shader": "ao", "synthetic_ao_distance": 8}, ["cfg", "--synthetic"]) == ("ao", 8)
    assert so({"synthetic_shader": "ao"}, ["cfg", "--synthetic", "--synthetic-shader", "phong"]) == ("phong", 16)
    assert so({"is_greyscale": "True"}, ["cfg", "--synthetic", "--synthetic-shader", "phong"]) == ("phong", 16)
    assert so({"is_greyscale": "False", "synthetic_ao_distance": "32"}, ["cfg", "--synthetic", "--synthetic-shader", "ao"]) == ("ao", 32)
    for cfg, argv, msg in (({}, ["cfg", "--train", "--synthetic-shader", "ao"], "needs --synthetic"),
                           ({}, ["cfg", "--synthetic", "--synthetic-shader"], "needs a value"),
                           ({}, ["cfg", "--synthetic", "--synthetic-shader", "toon"], "not one of"),
                           ({"synthetic_shader": "contour"}, ["cfg", "--synthetic"], "not one of"),
                           ({"is_greyscale": "True"}, ["cfg", "--synthetic", "--synthetic-shader", "normal"], "colour target"),
                           ({"is_greyscale": "False", "synthetic_shader": "phong"}, ["cfg", "--synthetic"], "colour target"),
                           ({"synthetic_ao_distance": 0}, ["cfg", "--synthetic"], "1..32"),
                           ({"synthetic_ao_distance": 33}, ["cfg", "--synthetic"], "1..32"),
                           ({"synthetic_ao_distance": 2.5}, ["cfg", "--synthetic"], "not an integer"),
                           ({"synthetic_ao_distance": "far"}, ["cfg", "--synthetic"], "not an integer")):
        with pytest.raises(SystemExit, match=msg):
            so(cfg, argv)
    assert synthetic_options({}, ["cfg", "--train", "--synthetic", "--synthetic-shader", "ao"]) == (True, 100)     # still a 2-tuple
