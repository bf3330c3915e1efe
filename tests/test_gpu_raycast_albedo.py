"""rn_raycast_albedo_fwd / rn_albedo_encode (rendernet_amd/csrc/raycast_albedo.hip), ops.raycast_albedo, ops.albedo_from_hits,
synth.SyntheticTextureTargets and `RenderNet_Texture_Face_Normal.py --train --synthetic` against the integer reference
tests/raycast_albedo_ref.py.  -m gpu.

The rule is an integer function of (hit voxel, wave table, quantised code), so every comparison is exact and covers every
pixel: the hits come from the device's own rn_raycast_fwd, the reference picture is computed from that array."""
import ctypes
import json
import os

import numpy as np
import pytest

import raycast_albedo_ref as AL
from conftest import FIXTURES, ROOT
from rendernet_amd._lib import RN_E_INVALID

pytestmark = pytest.mark.gpu
POSE = (250.0, 30.0, 1.0)                                                  # azimuth, elevation (degrees), scale
WINDOW = (190, 203, 112, 96)                                               # no multiple of the 16 x 16 tile
BASE = (144, 128, 112)


def pose_rad(az, el, s):
    return np.array([az * np.pi / 180.0, el * np.pi / 180.0, s], np.float32)


def colour_model(K):
    from rendernet_amd.synth import ColourModel
    return ColourModel(1234, K)


def codes(B, K, seed=5):
    from rendernet_amd.synth import ColourModel
    return ColourModel.quantise(np.random.default_rng(seed).standard_normal((B, K)))


def device_cast(occ, poses, N, f, window=None):
    """bool grids [B,S,S,S] at poses [B,3] -> (vox, m_inv on the device; normals, hit as NumPy) of ops.raycast_normals."""
    import torch
    from rendernet_amd import ops
    vox = torch.as_tensor(np.ascontiguousarray(occ[..., None]).astype(np.uint8)).cuda()
    m = ops.pose_to_affine(torch.as_tensor(np.asarray(poses, np.float32)).cuda(), occ.shape[1], N)
    normals, hit, _ = ops.raycast_normals(vox, m, new_size=N, pixels_per_cell=f, window=window, affine=True, return_hits=True)
    return vox, m, normals.cpu().numpy(), hit.cpu().numpy()


def device_albedo(vox, m, waves, q, N, f, smooth, window=None):
    import torch
    from rendernet_amd import ops
    alb, nrm = ops.raycast_albedo(vox, m, torch.as_tensor(waves).cuda(), torch.as_tensor(q).cuda(), BASE, new_size=N,
                                  pixels_per_cell=f, window=window, affine=True, smooth=smooth)
    assert alb.dtype is torch.uint8 and nrm.dtype is torch.uint8 and alb.shape == nrm.shape and alb.is_contiguous()
    return alb.cpu().numpy(), nrm.cpu().numpy()


def assert_same(got, want, what):
    bad = (got != want).any(axis=-1)
    assert not bad.any(), "%s: %d pixels differ, first at %s: kernel %s reference %s" % (
        what, bad.sum(), np.argwhere(bad)[0], got[bad][0], want[bad][0])


@pytest.fixture(scope="module")
def models(fixtures_vox):
    """chair and bunny as bool [2,64,64,64] indexed [z,y,x]."""
    return np.stack([fixtures_vox[FIXTURES.index(m), ..., 0] > 0.5 for m in ("chair", "bunny")])


@pytest.fixture(scope="module")
def small(models):
    """... cut to 32^3 by a 2x2x2 max-pool."""
    return models.reshape(2, 32, 2, 32, 2, 32, 2).any(axis=(2, 4, 6))


@pytest.fixture(scope="module")
def cast32(small):
    """The 128 x 128 frames of both small models (S = 32, N = 32, f = 4), cast once: (vox, m, normals, hit)."""
    return device_cast(small, np.stack([pose_rad(*POSE), pose_rad(37.0, 25.0, 1.0)]), 32, 4)


# -- the caster -----------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("K", [19, 199])
def test_small_models_whole_frame(cast32, K):
    """S = 32, N = 32, f = 4, B = 2: every pixel at smooth 0, 4 (the default) and 8; the normals are raycast_normals' bytes."""
    vox, m, normals, hit = cast32
    waves, q = colour_model(K).waves, codes(2, K)
    assert (hit >= 0).reshape(2, -1).sum(1).min() > 1000 and (hit < 0).reshape(2, -1).sum(1).min() > 1000
    plain = AL.albedo(hit, waves, q, 32, BASE)
    for smooth in (0, None, 8):
        got, nrm = device_albedo(vox, m, waves, q, 32, 4, smooth)
        assert got.shape == (2, 128, 128, 3) and np.array_equal(nrm, normals)
        assert_same(got, AL.encode(plain, hit, 32, 4 if smooth is None else smooth), "K %d smooth %s" % (K, smooth))
    inside = plain[hit >= 0].astype(np.int64)
    assert inside.std(axis=0).min() > (20 if K == 199 else 5) and (plain[hit < 0] == 0).all()      # a picture, not a flat colour


def test_odd_window(small, cast32):
    """A 37 x 53 window at an odd origin: partial tiles, and the smoothing window clipped to the CALL's window, so the bytes
    equal the crop of the whole frame only further than `smooth` pixels from the border."""
    vox, m, normals, hit_full = cast32
    window = (41, 35, 37, 53)
    r0, c0, ph, pw = window
    _, _, nrm_w, hit = device_cast(small, np.stack([pose_rad(*POSE), pose_rad(37.0, 25.0, 1.0)]), 32, 4, window)
    assert np.array_equal(hit, hit_full[:, r0:r0 + ph, c0:c0 + pw]) and (hit >= 0).any() and (hit < 0).any()
    waves, q = colour_model(199).waves, codes(2, 199)
    for smooth in (0, 3, 8):
        got, nrm = device_albedo(vox, m, waves, q, 32, 4, smooth, window)
        assert got.shape == (2, 37, 53, 3) and np.array_equal(nrm, nrm_w)
        assert_same(got, AL.picture(hit, waves, q, 32, BASE, smooth), "smooth %d" % smooth)
    full = AL.picture(hit_full, waves, q, 32, BASE, 3)
    got, _ = device_albedo(vox, m, waves, q, 32, 4, 3, window)
    assert np.array_equal(got[:, 3:-3, 3:-3], full[:, r0 + 3:r0 + ph - 3, c0 + 3:c0 + pw - 3])


def test_window_at_the_training_resolution(models):
    """S = 64, N = 128, f = 4: rows 190..301 x columns 203..298 of the chair, K = 199, the default smoothing and none."""
    occ, poses = models[:1], pose_rad(*POSE)[None]
    vox, m, normals, hit = device_cast(occ, poses, 128, 4, WINDOW)
    assert hit.shape == (1, 112, 96) and (hit >= 0).any() and (hit < 0).any() and hit.max() >= 32 ** 3
    waves, q = colour_model(199).waves, codes(1, 199, seed=9)
    for smooth in (None, 0):
        got, nrm = device_albedo(vox, m, waves, q, 128, 4, smooth, WINDOW)
        assert np.array_equal(nrm, normals)
        assert_same(got, AL.picture(hit, waves, q, 64, BASE, 4 if smooth is None else smooth), "smooth %s" % smooth)


def test_an_empty_item_is_black_and_saturating_codes_clamp(small):
    occ = np.stack([small[0], np.zeros((32, 32, 32), bool), small[1]])
    vox, m, normals, hit = device_cast(occ, np.tile(pose_rad(*POSE), (3, 1)), 32, 2)
    waves = colour_model(199).waves
    q = np.stack([np.full(199, 127, np.int8), np.full(199, -127, np.int8), np.where(waves[:, 4] >= 0, 127, -127).astype(np.int8)])
    for smooth in (0, 2):
        got, _ = device_albedo(vox, m, waves, q, 32, 2, smooth)
        assert got.shape == (3, 64, 64, 3) and (got[1] == 0).all() and (hit[1] < 0).all()
        assert_same(got, AL.picture(hit, waves, q, 32, BASE, smooth), "smooth %d" % smooth)
    plain = AL.albedo(hit, waves, q, 32, BASE)[hit >= 0]
    assert (plain == 0).any() and (plain == 255).any()                      # the clamp is reached from both sides


def test_albedo_from_given_hits_and_an_empty_batch():
    """Hand-made hits: -1 and ids >= S^3 are misses for both kernels; one block holds hits, misses and pixels outside."""
    import torch
    from rendernet_amd import ops
    S, K = 32, 19
    rng = np.random.default_rng(3)
    hit = rng.integers(0, S ** 3, (2, 21, 19)).astype(np.int32)
    hit[rng.random(hit.shape) < 0.3] = -1
    hit[0, 0, :4] = (S ** 3, S ** 3 + 7, 2 ** 31 - 1, -(2 ** 31))
    hit[1, 20, 18], hit[1, 0, 0] = S ** 3 - 1, 0
    waves, q = colour_model(K).waves, codes(2, K)
    dw, dq, dh = torch.as_tensor(waves).cuda(), torch.as_tensor(q).cuda(), torch.as_tensor(hit).cuda()
    for smooth in (0, 1, 8):
        got = ops.albedo_from_hits(dh, dw, dq, S, BASE, smooth).cpu().numpy()
        assert_same(got, AL.picture(hit, waves, q, S, BASE, smooth), "smooth %d" % smooth)
        assert (got[0, 0, :4] == 0).all()
    zero = ops.albedo_from_hits(dh, dw, torch.zeros_like(dq), S, BASE).cpu().numpy()
    ok = (hit >= 0) & (hit < S ** 3)
    assert (zero[ok] == BASE).all() and (zero[~ok] == 0).all()
    # B = 0
    none = ops.albedo_from_hits(dh[:0], dw, dq[:0], S, BASE, 4)
    assert none.shape == (0, 21, 19, 3) and none.dtype is torch.uint8
    alb, nrm = ops.raycast_albedo(torch.zeros((0, 32, 32, 32, 1), device="cuda"), torch.zeros((0, 3), device="cuda"), dw, dq[:0], BASE,
                                  new_size=32, pixels_per_cell=2)
    assert alb.shape == nrm.shape == (0, 64, 64, 3)


def test_invalid_arguments_return_invalid_without_a_launch():
    import torch
    from rendernet_amd import _lib, ops
    from rendernet_amd._lib import RenderNetHipError
    lib, vp, st = _lib.lib(), ctypes.c_void_p, _lib.stream_ptr()
    B, S, K, ph, pw = 2, 32, 19, 20, 24
    hit = torch.zeros((B, ph, pw), dtype=torch.int32, device="cuda")
    waves = torch.as_tensor(colour_model(K).waves).cuda()
    big = torch.zeros((257, 8), dtype=torch.int16, device="cuda")
    q = torch.zeros((B, 257), dtype=torch.int8, device="cuda")
    col = torch.full((B, ph, pw, 3), 7, dtype=torch.uint8, device="cuda")
    out = torch.full((B, ph, pw, 3), 9, dtype=torch.uint8, device="cuda")
    p = {"hit": hit.data_ptr(), "waves": waves.data_ptr(), "q": q.data_ptr(), "col": col.data_ptr(), "out": out.data_ptr()}

    def fwd(B=B, S=S, K=K, ph=ph, pw=pw, base=BASE, **ptr):
        d = dict(p, **ptr)
        host = ctypes.cast((ctypes.c_int * 3)(*base), vp) if base is not None else None
        return lib.rn_raycast_albedo_fwd(vp(d["hit"]), vp(d["waves"]), vp(d["q"]), host, vp(d["col"]), B, S, K, ph, pw, st)

    def enc(B=B, S=S, ph=ph, pw=pw, smooth=2, **ptr):
        d = dict(p, **ptr)
        return lib.rn_albedo_encode(vp(d["col"]), vp(d["hit"]), vp(d["out"]), B, S, ph, pw, smooth, st)

    bad_fwd = [dict(B=-1), dict(B=65536), dict(S=48), dict(S=0), dict(S=160), dict(K=0), dict(K=257, waves=big.data_ptr()),
               dict(ph=0), dict(pw=0), dict(ph=4097), dict(pw=-3), dict(base=None), dict(base=(256, 0, 0)), dict(base=(0, -1, 0)),
               dict(hit=None), dict(waves=None), dict(q=None), dict(col=None), dict(hit=p["hit"] + 2), dict(waves=p["waves"] + 8),
               dict(col=p["hit"]), dict(col=p["hit"] + 4 * B * ph * pw - 1)]
    for kw in bad_fwd:
        assert fwd(**kw) == RN_E_INVALID, kw
    assert b"overlap" in lib.rn_last_error()
    bad_enc = [dict(B=-1), dict(B=65536), dict(S=48), dict(ph=0), dict(pw=4097), dict(smooth=-1), dict(smooth=9), dict(col=None),
               dict(hit=None), dict(out=None), dict(hit=p["hit"] + 1), dict(out=p["col"]), dict(out=p["col"] + 3 * B * ph * pw - 1),
               dict(out=p["hit"])]
    for kw in bad_enc:
        assert enc(**kw) == RN_E_INVALID, kw
    torch.cuda.synchronize()
    assert (col == 7).all() and (out == 9).all()                            # nothing was launched
    assert fwd(B=0) == 0 and enc(B=0) == 0 and fwd(B=0, hit=None) == 0
    torch.cuda.synchronize()
    assert (col == 7).all() and (out == 9).all()
    assert fwd() == 0 and enc() == 0                                        # ... and the same buffers are accepted as they are
    torch.cuda.synchronize()
    assert (col == torch.tensor(BASE, dtype=torch.uint8, device="cuda")).all() and (out == col).all()      # voxel 0, a zero code
    # ops: shapes and dtypes are refused before the cast is launched
    vox = torch.ones((B, 32, 32, 32, 1), dtype=torch.uint8, device="cuda")
    pose = torch.as_tensor(np.tile(pose_rad(*POSE), (B, 1))).cuda()
    qk = q[:, :K].contiguous()
    for args, kw, msg in (((big, q, BASE), {}, "K in 1..256"), ((waves, qk, BASE), {"smooth": 9}, "smooth"),
                          ((waves, qk.short(), BASE), {}, "code_q int8"), ((waves, qk[:1], BASE), {}, "code_q int8"),
                          ((waves.int(), qk, BASE), {}, "waves int16"), ((waves, qk, (1, 2)), {}, "base"),
                          ((waves, qk, (1, 2, 300)), {}, "base"), ((waves.cpu(), qk, BASE), {}, "HIP tensors")):
        with pytest.raises(RenderNetHipError, match=msg):
            ops.raycast_albedo(vox, pose, *args, new_size=32, pixels_per_cell=2, **kw)
    with pytest.raises(RenderNetHipError, match="S=48"):
        ops.raycast_albedo(torch.ones((B, 48, 48, 48, 1), dtype=torch.uint8, device="cuda"), pose, waves, qk, BASE, new_size=32)
    with pytest.raises(RenderNetHipError, match="S=48"):
        ops.albedo_from_hits(hit, waves, qk, 48, BASE)
    with pytest.raises(RenderNetHipError, match="hit int32"):
        ops.albedo_from_hits(hit.long(), waves, qk, S, BASE)


# -- the trainer ----------------------------------------------------------------------------------------------------------

def test_texture_targets_feed_the_trainer(small, gemm_mode):
    """SyntheticTextureTargets on the two small models feeds a reduced texture trainer (the tiny spec's widths on 32^3 grids:
    32^3 -> 64^3 -> 256^2, z_dim 19 -- the smallest spec the caster's S accepts): one step per multiply mode, crop 16.  The
    loss read from the uint8 frames (rn_target_u8_crop_fwd) equals the loss on the same frames passed as float / 255 from
    identical weights: both paths read the same bytes."""
    import torch
    from rendernet_amd import ops, synth
    from rendernet_amd.texture import TextureSpec, init_texture_weights
    from rendernet_amd.train import TextureTrainer
    spec = TextureSpec(size=32, new_size=64, z_dim=19, tex_res=16, c1=8, c2=16, c3=16, n_res1=2, w_res2=256, n_res2=2, w5=64,
                       n_res3=1, w6=32, w7=32, w8=16, w9=16).check()
    colour = synth.ColourModel(1234, 19)
    feed = synth.SyntheticTextureTargets(small.astype(np.uint8)[..., None], ["chair", "bunny"], 2, 1, seed=3, colour=colour,
                                         device="cuda", new_size=64)
    images, normals, vox, tex, poses, names = next(feed)
    assert images.dtype is torch.uint8 and images.shape == (2, 256, 256, 3) and images.is_cuda and normals.shape == images.shape
    assert vox.dtype is torch.uint8 and vox.shape == (2, 32, 32, 32, 1) and tex.dtype is torch.float32 and tex.shape == (2, 19)
    q = torch.round(tex * 32).to(torch.int8)
    assert torch.equal(q.float() / 32, tex)
    alb, nrm = ops.raycast_albedo(vox, poses, torch.as_tensor(colour.waves).cuda(), q, colour.base, new_size=64)
    assert torch.equal(alb, images) and torch.equal(nrm, normals) and torch.equal(nrm, ops.raycast_normals(vox, poses, new_size=64))
    hits = (normals != 0).any(dim=3)
    assert hits.reshape(2, -1).sum(1).min() > 1000 and images[hits].float().std(0).min() > 2
    losses = []
    for frames in ((images, normals), (images.float() / 255.0, normals.float() / 255.0)):
        tr = TextureTrainer(spec, init_texture_weights(spec, seed=1234), device="cuda", e_eta=1e-4, keep_prob=1.0)
        losses.append(float(tr.step(vox, tex, poses, frames[0], frames[1], patch_size=16, start_point=(24, 24)).item()))
    print("%s losses (uint8 frames, float frames): %s" % (gemm_mode, losses))
    assert np.isfinite(losses).all() and losses[0] > 0
    assert abs(losses[0] - losses[1]) <= 1e-6 * abs(losses[1])


def test_texture_script_trains_on_synthetic_targets(tmp_path, capsys):
    """`RenderNet_Texture_Face_Normal.py <config> --train --synthetic` from the binvox folder alone: no image_path, normal_path
    or texture_path in the config."""
    from PIL import Image
    import RenderNet_Texture_Face_Normal as script
    cfg = {"model_path": os.path.join(ROOT, "binvox"), "gpu": 0, "batch_size": 2, "max_epochs": 1, "batches_chunk": 1,
           "threshold": 0.1, "e_eta": 1e-5, "keep_prob": 0.75, "decay_steps": 100000, "trained_model_name": "3d2d_renderer",
           "sample_save": str(tmp_path / "out"), "checkpoint_secs": 7200}
    cfgp = str(tmp_path / "config.json")
    json.dump(cfg, open(cfgp, "w"))
    script.main([cfgp, "--train", "--synthetic", "--synthetic-steps", "2", "--max-steps", "2"])
    out = capsys.readouterr().out
    losses = [float(l.split("Loss")[1]) for l in out.splitlines() if l.startswith("Step")]
    print("losses: %s" % losses)
    assert len(losses) == 2 and all(np.isfinite(losses)) and losses[0] > 0
    files = set(os.listdir(cfg["sample_save"]))
    assert {"config.json", "3d2d_renderer.npz", "L1 All.txt.npz"} <= files
    ck = np.load(os.path.join(cfg["sample_save"], "3d2d_renderer.npz"))
    assert int(ck["__global_step__"]) == 2 and any(k.startswith("texture_encoder/") for k in ck.files)
    l1 = np.load(os.path.join(cfg["sample_save"], "L1 All.txt.npz"))["arr_0"]
    assert l1.shape == (1,) and np.isfinite(l1).all() and l1[0] > 0
    targets = [f for f in files if f.startswith("VALID_") and f.endswith("_target_0.png")]
    assert len(targets) == 1 and sum(f.endswith("_target_normal_0.png") for f in files) == 1
    img = np.asarray(Image.open(os.path.join(cfg["sample_save"], targets[0])))
    assert img.shape == (512, 512, 3)
    lit = img[(img != 0).any(axis=2)]
    assert len(lit) > 1000 and len(np.unique(lit, axis=0)) > 16            # a coloured picture of the model on black
