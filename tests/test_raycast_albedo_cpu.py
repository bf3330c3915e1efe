"""Host-side checks of the albedo targets: the cosine table (scripts/gen_cos_q.py, csrc/cos_q.h), synth.ColourModel, closed
forms and the smoothing on the integer reference (tests/raycast_albedo_ref.py), SyntheticTextureTargets with the caster
stubbed, and the texture script's --synthetic parsing.  No GPU."""
import json
import os
import re
import zlib
from fractions import Fraction

import numpy as np
import pytest

import raycast_albedo_ref as AL
from conftest import ROOT
from scripts import gen_cos_q as GEN

S = 32
BASE = (144, 128, 112)

# -- the table and the colour model ---------------------------------------------------------------------------------------


def test_header_equals_the_generated_table():
    text = open(os.path.join(ROOT, "rendernet_amd", "csrc", "cos_q.h")).read()
    body = text[text.index("rn_cos_q[RN_COS_Q_COUNT] = {"):]
    vals = [int(v) for v in re.findall(r"-?\d+", body[body.index("{"):body.index("}")])]
    T = GEN.table()
    assert T.dtype == np.int8 and T.shape == (256,) and vals == T.tolist() == AL.cos_q().tolist()
    assert T[0] == 127 and T[64] == 0 and T[128] == -127 and T[192] == 0 and np.array_equal(T[1:], T[:0:-1])


@pytest.mark.parametrize("K,crc", [(199, 492401642), (19, 1532230393)])
def test_colour_model_is_pinned(K, crc):
    """The draw order is part of the format: a changed order would invalidate every checkpoint trained on the field."""
    from rendernet_amd.synth import ColourModel
    a, b = ColourModel(1234, K), ColourModel(1234, K)
    w = a.waves
    assert w.dtype == np.int16 and w.shape == (K, 8) and np.array_equal(w, b.waves) and a.base == BASE
    assert zlib.crc32(w.tobytes()) == crc
    assert np.abs(w[:, :3]).max() <= 3 and w[:, :3].any(axis=1).all() and w[:, 3].min() >= 0 and w[:, 3].max() <= 255
    assert np.abs(w[:, 4:7]).max() <= 127 and not w[:, 7].any()
    assert not np.array_equal(ColourModel(1235, K).waves, w)
    rng = np.random.default_rng([1234, K])                                 # the stated order, drawn again here
    f = rng.integers(-3, 4, (K, 3))
    f[~f.any(axis=1)] = (1, 0, 0)
    assert np.array_equal(w[:, :3], f) and np.array_equal(w[:, 3], rng.integers(0, 256, K))
    assert np.array_equal(w[:, 4:7], rng.integers(-127, 128, (K, 3)))
    for bad in (0, 257):
        with pytest.raises(ValueError, match="z_dim"):
            ColourModel(1234, bad)


def test_quantised_code_round_trips():
    from rendernet_amd.synth import ColourModel as CM
    beta = np.concatenate([np.random.default_rng(0).standard_normal(1000) * 1.5, [5.0, -5.0, 127 / 32, 0.0, 1 / 64, -1 / 64, 3 / 64]])
    q = CM.quantise(beta)
    assert q.dtype == np.int8 and q.min() == -127 and q.max() == 127
    assert q[-7:].tolist() == [127, -127, 127, 0, 0, 0, 2]                  # clipped; ties go to the even integer (rint)
    d = CM.dequantise(q)
    assert d.dtype == np.float32 and np.array_equal(d * 32, q.astype(np.float32))     # 32 d is integral: the division is exact
    assert np.array_equal(CM.quantise(d), q)
    inside = np.abs(beta) < 127 / 32
    assert np.abs(d[inside] - beta[inside]).max() <= 1 / 64

# -- closed forms of the colour rule --------------------------------------------------------------------------------------


def _one_wave(f=(1, 0, 0), phase=0, amp=(127, 0, -127)):
    return np.array([list(f) + [phase] + list(amp) + [0]], np.int16)


def test_zero_code_gives_base_on_every_hit():
    from rendernet_amd.synth import ColourModel
    hit = np.concatenate([[-2, -1], np.arange(0, S ** 3, 997), [S ** 3 - 1, S ** 3, S ** 3 + 5]]).reshape(1, 1, -1)
    out = AL.albedo(hit, ColourModel(1234, 199).waves, np.zeros((1, 199), np.int8), S, BASE)
    is_hit = (hit >= 0) & (hit < S ** 3)
    assert is_hit.sum() == hit.size - 4 and (out[is_hit] == BASE).all() and (out[~is_hit] == 0).all()


def test_one_wave_by_hand():
    """q = 32, amp = (127, 0, -127), f = (1, 0, 0), phase 0: idx = 4 xs.  xs = 0: COS_Q = 127, acc = 32 * 127 * 127 = 516128,
    (516128 + 32768) >> 16 = 8 -> base + (8, 0, -8).  xs = 32 (S = 64): idx = 128, COS_Q = -127, acc = -516128,
    (-516128 + 32768) >> 16 = floor(-7.375) = -8 -> base + (-8, 0, 8).  xs = 16: idx = 64, COS_Q = 0 -> base."""
    hit = np.array([[[AL.flat(0, 5, 9, 64), AL.flat(32, 5, 9, 64), AL.flat(16, 1, 2, 64), -1, 64 ** 3]]])
    out = AL.albedo(hit, _one_wave(), np.array([[32]], np.int8), 64, BASE)
    assert out[0, 0].tolist() == [[152, 128, 104], [136, 128, 120], [144, 128, 112], [0, 0, 0], [0, 0, 0]]
    # the phase and the other axes: f = (0, -1, 2), phase 64 at (xs, ys, zs) = (3, 2, 1): idx = (4 * (-2 + 2) + 64) & 255 = 64
    out = AL.albedo(np.array([[[AL.flat(3, 2, 1, S)]]]), _one_wave((0, -1, 2), 64), np.array([[127]], np.int8), S, BASE)
    assert out[0, 0, 0].tolist() == list(BASE)
    # a negative index wraps in two's complement: f = (-3, 0, 0) at xs = 1: idx = -12 & 255 = 244, COS_Q[244] = COS_Q[12] = 122
    out = AL.albedo(np.array([[[AL.flat(1, 0, 0, S)]]]), _one_wave((-3, 0, 0)), np.array([[64]], np.int8), S, BASE)
    step = (64 * 127 * 122 + 32768) >> 16                                  # 15
    assert AL.cos_q()[244] == 122 and step == 15 and out[0, 0, 0].tolist() == [159, 128, 97]           # B: (-991616 + 32768) >> 16 = -15


def test_saturating_codes_clamp_without_wrapping():
    K = 256
    w = np.zeros((K, 8), np.int16)
    w[:, 0], w[:, 4:7] = 1, (127, -127, 127)                               # every wave the same: acc = +-K 127^2 COS_Q
    hit = np.array([[[AL.flat(0, 0, 0, 64), AL.flat(16, 0, 0, 64), AL.flat(32, 3, 3, 64)]]])     # COS_Q = 127, 0, -127
    out = AL.albedo(hit, w, np.full((1, K), 127, np.int8), 64, BASE)
    assert out[0, 0].tolist() == [[255, 0, 255], [144, 128, 112], [0, 255, 0]]
    assert K * 127 ** 3 < 2 ** 31 - 32768

# -- smoothing ------------------------------------------------------------------------------------------------------------


def test_a_lone_hit_keeps_its_colour():
    hit = np.full((1, 9, 9), -1)
    hit[0, 4, 4] = 7
    colour = np.random.default_rng(0).integers(0, 256, (1, 9, 9, 3)).astype(np.uint8)       # misses carry junk: ignored
    for r in (0, 1, 4, 8):
        out = AL.encode(colour, hit, S, r)
        assert out[0, 4, 4].tolist() == colour[0, 4, 4].tolist() and out.sum() == colour[0, 4, 4].sum()


def test_checker_of_two_colours_averages_with_the_stated_rounding():
    """A 5 x 5 checker of hits in colours a (13 pixels) and b (12), smooth 2: the centre's window is the whole picture."""
    a, b = np.array([10, 200, 255]), np.array([13, 1, 0])
    yy, xx = np.mgrid[0:5, 0:5]
    colour = np.where(((yy + xx) % 2 == 0)[..., None], a, b).astype(np.uint8)[None]
    hit = np.zeros((1, 5, 5), np.int64)
    out = AL.encode(colour, hit, S, 2)
    want = [int(Fraction(int(13 * a[c] + 12 * b[c]), 25) + Fraction(1, 2)) for c in range(3)]
    assert out[0, 2, 2].tolist() == want == [(2 * (13 * a[c] + 12 * b[c]) + 25) // 50 for c in range(3)]
    # the corner sees the 3 x 3 window clipped to the picture: 5 of a, 4 of b
    assert out[0, 0, 0].tolist() == [(2 * (5 * a[c] + 4 * b[c]) + 9) // 18 for c in range(3)]
    # a miss in the middle stays black and drops out of its neighbours' means
    hit[0, 2, 2] = -1
    out = AL.encode(colour, hit, S, 1)
    assert out[0, 2, 2].tolist() == [0, 0, 0]
    assert out[0, 2, 1].tolist() == [(2 * (5 * b[c] + 3 * a[c]) + 8) // 16 for c in range(3)]
    assert np.array_equal(AL.encode(colour, hit, S, 0), np.where((hit >= 0)[..., None], colour, 0))

# -- rendernet_amd.synth with the caster stubbed --------------------------------------------------------------------------


@pytest.fixture
def stub_caster(monkeypatch):
    import torch
    from rendernet_amd import synth
    calls = []

    def fake(vox, poses, waves, code_q, base, new_size, pixels_per_cell, smooth):
        calls.append((tuple(vox.shape), tuple(waves.shape), waves.dtype, code_q.dtype, tuple(base), new_size, pixels_per_cell, smooth))
        # pictures that depend on the sample: its model tag, pose and code
        tag = vox.reshape(vox.shape[0], -1).amax(1).float() * 20 + poses[:, 0] * 10
        img = (tag + code_q[:, 0].float()).to(torch.int64).remainder(256).to(torch.uint8)[:, None, None, None] + torch.arange(192, dtype=torch.uint8).reshape(1, 8, 8, 3)
        return img.contiguous(), (img + 1).contiguous()
    monkeypatch.setattr(synth, "_cast_albedo", fake)
    return calls


def _targets(seed, rank=0, world=1, steps=3, bs=4, K=19, names=("chair", "teapot", "bunny"), **kw):
    from rendernet_amd import synth
    models = np.zeros((3, 8, 8, 8, 1), np.uint8)
    models[np.arange(3), np.arange(3), 0, 0, 0] = 1 + np.arange(3)
    return synth.SyntheticTextureTargets(models, list(names), bs, steps, seed, synth.ColourModel(1234, K), rank=rank, world=world,
                                         device="cpu", **kw)


def test_texture_targets_tuple_seed_and_code(stub_caster):
    import torch
    from rendernet_amd import synth
    from rendernet_amd.tools import data_util
    a, b, other = list(_targets(7, smooth=3)), list(_targets(7, smooth=3)), list(_targets(8))
    assert len(a) == 3 and len(stub_caster) == 9
    assert stub_caster[0] == ((4, 8, 8, 8, 1), (19, 8), torch.int16, torch.int8, BASE, 128, 4, 3) and stub_caster[-1][-1] == 4
    rng = np.random.default_rng(7)
    for (img, nrm, vox, tex, pose, names), (img2, nrm2, vox2, tex2, pose2, names2) in zip(a, b):
        assert names == names2 and all(torch.equal(x, y) for x, y in ((img, img2), (nrm, nrm2), (vox, vox2), (tex, tex2), (pose, pose2)))
        assert img.dtype is torch.uint8 and img.shape == (4, 8, 8, 3) and nrm.dtype is torch.uint8 and nrm.shape == img.shape
        assert vox.dtype is torch.uint8 and vox.shape == (4, 8, 8, 8, 1)
        assert tex.dtype is torch.float32 and tex.shape == (4, 19) and pose.dtype is torch.float32 and pose.shape == (4, 3)
        # the draws: draw_batch first, then the codes of the whole batch on the same generator
        _, want_names, want_poses = synth.draw_batch(rng, ["chair", "teapot", "bunny"], 4)
        q = synth.ColourModel.quantise(rng.standard_normal((4, 19)))
        assert names == want_names and np.array_equal(pose.numpy(), want_poses)
        assert np.array_equal(tex.numpy(), synth.ColourModel.dequantise(q)) and np.array_equal(tex.numpy() * 32, q.astype(np.float32))
        for i, n in enumerate(names):                                       # the names parse back to the poses
            assert np.array_equal(np.float32(data_util.extract_param_from_names(n)[0]), pose.numpy()[i])
    assert [t[5] for t in a] != [t[5] for t in other]


def test_texture_target_shards_concatenate(stub_caster):
    whole = list(_targets(11))
    parts = [list(_targets(11, rank=r, world=2)) for r in range(2)]
    for step, batch in enumerate(whole):
        assert batch[5] == parts[0][step][5] + parts[1][step][5]
        for k in range(5):
            assert np.array_equal(batch[k].numpy(), np.concatenate([parts[0][step][k].numpy(), parts[1][step][k].numpy()]))


def test_texture_targets_validate_like_the_shader_feed(stub_caster):
    from rendernet_amd import synth
    for kw, msg in ((dict(world=3), "non-empty shard"), (dict(rank=2, world=2), "non-empty shard"), (dict(bs=0), "batch_size"),
                    (dict(names=("chair", "tea_pot", "bunny")), "pose tags"), (dict(names=("chair", "bunny")), "names for"),
                    (dict(smooth=9), "smooth"), (dict(smooth=-1), "smooth")):
        with pytest.raises(ValueError, match=msg):
            _targets(3, **kw)
    with pytest.raises(ValueError, match="ColourModel"):
        synth.SyntheticTextureTargets(np.zeros((1, 8, 8, 8, 1), np.uint8), ["chair"], 2, 1, 0, colour=1234, device="cpu")
    assert "noise" in synth.SyntheticTextureTargets.__doc__

# -- flag and config parsing ----------------------------------------------------------------------------------------------


def test_texture_script_synthetic_options(tmp_path):
    import RenderNet_Texture_Face_Normal as script
    so = script.synthetic_texture_options
    assert so({}, ["cfg", "--train"]) == (False, 100, 1234, 1234, 4)
    assert so({}, ["cfg", "--train", "--synthetic", "--synthetic-steps", "7"]) == (True, 7, 1234, 1234, 4)
    assert so({"synthetic_targets": True, "synthetic_steps_per_epoch": 3, "synthetic_seed": 5, "synthetic_colour_seed": 6,
               "synthetic_smooth": 0}, ["cfg", "--train"]) == (True, 3, 5, 6, 0)
    for cfg, argv, msg in (({}, ["cfg", "--train", "--synthetic-steps", "2"], "needs --synthetic"),
                           ({"synthetic_smooth": 9}, ["cfg", "--train", "--synthetic"], "0..8"),
                           ({"synthetic_smooth": -1}, ["cfg", "--train", "--synthetic"], "0..8"),
                           ({"synthetic_smooth": 2.5}, ["cfg", "--synthetic"], "not an integer"),
                           ({"synthetic_colour_seed": "red"}, ["cfg", "--synthetic"], "not an integer"),
                           ({"synthetic_targets": "maybe"}, ["cfg"], "neither true nor false")):
        with pytest.raises(SystemExit, match=msg):
            so(cfg, argv)
    # load_config: --synthetic lifts texture_path alone; without it the requirements are today's
    cfg = {"model_path": "m", "sample_save": str(tmp_path / "out"), "trained_model_name": "n", "batch_size": 2, "keep_prob": 1.0}
    path = str(tmp_path / "config.json")
    json.dump(cfg, open(path, "w"))
    assert script.load_config(path, [path, "--train", "--synthetic"]) == cfg
    with pytest.raises(KeyError, match="texture_path"):
        script.load_config(path, [path, "--train"])
    with pytest.raises(KeyError, match="texture_path"):
        script.load_config(path)
    with pytest.raises(SystemExit, match="needs --synthetic"):
        script.main([path, "--train", "--synthetic-steps", "2"])
    json.dump(dict(cfg, synthetic_smooth=9), open(path, "w"))
    with pytest.raises(SystemExit, match="0..8"):
        script.main([path, "--train", "--synthetic"])
    json.dump({k: v for k, v in cfg.items() if k != "model_path"}, open(path, "w"))
    with pytest.raises(KeyError, match="model_path"):
        script.load_config(path, [path, "--train", "--synthetic"])
