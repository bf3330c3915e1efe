"""rn_raycast_ao_fwd / rn_ao_encode (rendernet_amd/csrc/raycast.hip), ops.raycast_ao and SyntheticTargets(shader="ao")
against the float64 reference tests/raycast_ao_ref.py.  -m gpu.

The rule is an integer function of (hit voxel, entry face, occupancy), so every comparison is exact and covers every pixel:
hits and faces come from the device's own rn_raycast_fwd, the reference counts are computed from those arrays."""
import ctypes
import dataclasses

import numpy as np
import pytest

import raycast_ao_ref as AR
from conftest import FIXTURES
from rendernet_amd._lib import RN_E_INVALID

pytestmark = pytest.mark.gpu
POSE = (250.0, 30.0, 1.0)                                                  # azimuth, elevation (degrees), scale
WINDOW = (190, 203, 112, 96)                                               # no multiple of the 16 x 16 tile


def pose_rad(az, el, s):
    return np.array([az * np.pi / 180.0, el * np.pi / 180.0, s], np.float32)


def device_ao(occ, poses, N, f, L, smooth, window=None):
    """bool grids [B,S,S,S] at poses [B,3] -> (hit, face, counts, bytes) as NumPy: the hits of ops.raycast_normals and
    ops.raycast_ao on the same matrices."""
    import torch
    from rendernet_amd import ops
    vox = torch.as_tensor(np.ascontiguousarray(occ[..., None]).astype(np.uint8)).cuda()
    m = ops.pose_to_affine(torch.as_tensor(np.asarray(poses, np.float32)).cuda(), occ.shape[1], N)
    _, hit, face = ops.raycast_normals(vox, m, new_size=N, pixels_per_cell=f, window=window, affine=True, return_hits=True)
    out, cnt = ops.raycast_ao(vox, m, new_size=N, pixels_per_cell=f, window=window, affine=True, max_distance=L,
                              smooth=smooth, return_counts=True)
    assert out.dtype is torch.uint8 and cnt.dtype is torch.uint8 and out.shape == hit.shape == cnt.shape
    return hit.cpu().numpy(), face.cpu().numpy(), cnt.cpu().numpy(), out.cpu().numpy()


def bytes_for(occ, poses, N, f, L, smooth, window=None):
    import torch
    from rendernet_amd import ops
    vox = torch.as_tensor(np.ascontiguousarray(occ[..., None]).astype(np.uint8)).cuda()
    return ops.raycast_ao(vox, torch.as_tensor(np.asarray(poses, np.float32)).cuda(), new_size=N, pixels_per_cell=f,
                          window=window, max_distance=L, smooth=smooth).cpu().numpy()


def reference_counts(occ, hit, face, L):
    return np.stack([AR.ao_counts(occ[b], hit[b], face[b], L) for b in range(len(occ))])


@pytest.fixture(scope="module")
def models(fixtures_vox):
    """chair and bunny as bool [2,64,64,64] indexed [z,y,x]."""
    return np.stack([fixtures_vox[FIXTURES.index(m), ..., 0] > 0.5 for m in ("chair", "bunny")])


# -- closed forms ---------------------------------------------------------------------------------------------------------

def test_closed_forms_from_given_hits():
    """Every closed-form case (all six faces) as one item of one call of the second stage, fed its hit voxel and face."""
    import torch
    from rendernet_amd import ops
    cases = AR.closed_form_cases()
    for L in sorted({c[4] for c in cases}):
        sel = [c for c in cases if c[4] == L]
        occ = np.stack([c[1] for c in sel])
        hit = np.full((len(sel), 1, 6), -1, np.int32)
        face = np.zeros((len(sel), 1, 6), np.int8)
        want = np.full((len(sel), 1, 6), 255, np.uint8)
        for i, (_, _, hits, faces, _, counts) in enumerate(sel):
            hit[i, 0, :len(hits)], face[i, 0, :len(hits)], want[i, 0, :len(hits)] = hits, faces, counts
        bits, box = ops.voxel_pack(torch.as_tensor(occ[..., None].astype(np.uint8)).cuda())
        out, cnt = ops.raycast_ao_from_hits(bits, box, torch.as_tensor(hit).cuda(), torch.as_tensor(face).cuda(), AR.S,
                                            max_distance=L, smooth=0, return_counts=True)
        assert np.array_equal(cnt.cpu().numpy(), want), [c[0] for c in sel]
        assert np.array_equal(out.cpu().numpy(), AR.encode(want, 0))


@pytest.mark.parametrize("smooth", [0, 1, 8])
def test_ragged_picture_from_given_hits(smooth):
    """The two slabs one empty layer apart (S = 32, L = 4) under a seeded 19 x 37 picture of hits on its occupied voxels by
    random faces, about a third of the pixels misses: two tiles down and three across, both ragged, no side narrower than
    the 8-pixel halo.  Counts and bytes against the reference where tile edges, halo clipping and the largest radius meet."""
    import torch
    from rendernet_amd import ops
    occ = {c[0]: c[1] for c in AR.closed_form_cases()}["gap a0 s+1 L4"]
    rng = np.random.default_rng(19)
    hit = rng.choice(np.flatnonzero(occ.reshape(-1)), (1, 19, 37)).astype(np.int32)
    face = rng.integers(0, 6, (1, 19, 37)).astype(np.int8)
    hit[rng.random((1, 19, 37)) < 1.0 / 3.0] = -1
    want = reference_counts(occ[None], hit, face, 4)
    assert len(np.unique(want)) > 8 and 0.25 < (want == 255).mean() < 0.45 and len(np.unique(AR.encode(want, smooth))) > 8
    bits, box = ops.voxel_pack(torch.as_tensor(occ[None, ..., None].astype(np.uint8)).cuda())
    out, cnt = ops.raycast_ao_from_hits(bits, box, torch.as_tensor(hit).cuda(), torch.as_tensor(face).cuda(), AR.S,
                                        max_distance=4, smooth=smooth, return_counts=True)
    assert np.array_equal(cnt.cpu().numpy(), want)
    assert np.array_equal(out.cpu().numpy(), AR.encode(want, smooth))


@pytest.mark.parametrize("pose", [(0.0, 0.0, 1.0), (37.0, 25.0, 1.0)])
def test_closed_form_grids_through_the_caster(pose):
    """The four grids (voxel, slab, two slabs, well) at S = 32, N = 32, f = 2: a 64 x 64 frame, head on and oblique."""
    cases = {c[0]: c[1] for c in AR.closed_form_cases()}
    occ = np.stack([cases["voxel"], cases["slab a0 s+1"], cases["gap a0 s+1 L4"], cases["well a0 s+1 h3"]])
    poses = np.tile(pose_rad(*pose), (4, 1))
    seen_faces = set()
    for smooth in (0, 2):
        hit, face, cnt, out = device_ao(occ, poses, 32, 2, 4, smooth)
        assert out.shape == (4, 64, 64)
        want = reference_counts(occ, hit, face, 4)
        assert np.array_equal(cnt, want)
        assert np.array_equal(out, AR.encode(want, smooth))
        assert ((hit >= 0).reshape(4, -1).sum(1) >= 4).all()
        seen_faces.update(np.unique(face[hit >= 0]).tolist())
        assert (cnt[0][hit[0] >= 0] == 64).all()                            # the lone voxel is open on every face
    if pose[0] != 0.0:
        assert len(seen_faces) >= 3, seen_faces


# -- models ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("L", [16, 32])
def test_models_whole_frame(models, L):
    """chair and bunny, S = 64, N = 128, f = 1, the whole frame: counts and bytes on every pixel."""
    poses = np.tile(pose_rad(*POSE), (2, 1))
    hit, face, cnt, out0 = device_ao(models, poses, 128, 1, L, 0)
    want = reference_counts(models, hit, face, L)
    bad = cnt != want
    assert not bad.any(), "%d pixels differ, first at %s: kernel %d reference %d" % (
        bad.sum(), np.argwhere(bad)[0], cnt[bad][0], want[bad][0])
    assert np.array_equal(out0, AR.encode(want, 0))
    assert np.array_equal(bytes_for(models, poses, 128, 1, L, 2), AR.encode(want, 2))
    inside = want[hit >= 0]
    assert (hit >= 0).reshape(2, -1).sum(1).min() > 256 and inside.min() < 32 and inside.max() == 64


def test_window_at_the_training_resolution(models):
    """f = 4, rows 190..301 x columns 203..298 of the chair (112 x 96: partial tiles, lanes outside the window in the wave
    loop), default smoothing (4) and none.  Counts are per pixel, so they equal that region of the whole 512^2 frame; the
    smoothed bytes do where the (2r+1)^2 window does not reach the border of the cast."""
    occ, poses = models[:1], pose_rad(*POSE)[None]
    hit, face, cnt, out = device_ao(occ, poses, 128, 4, 16, None, WINDOW)
    assert out.shape == (1, 112, 96) and (hit >= 0).any() and (hit < 0).any()
    want = reference_counts(occ, hit, face, 16)
    assert np.array_equal(cnt, want)
    assert np.array_equal(out, AR.encode(want, 4))
    assert np.array_equal(bytes_for(occ, poses, 128, 4, 16, 0, WINDOW), AR.encode(want, 0))
    _, _, cnt_full, out_full = device_ao(occ, poses, 128, 4, 16, None)
    r0, c0, ph, pw = WINDOW
    assert np.array_equal(cnt_full[:, r0:r0 + ph, c0:c0 + pw], cnt)
    assert np.array_equal(out_full[:, r0 + 4:r0 + ph - 4, c0 + 4:c0 + pw - 4], out[:, 4:-4, 4:-4])


def test_grid_of_128_reads_the_mask_from_memory(models):
    """S = 128 (no LDS copy of the mask): the chair upsampled x2, N = 256, f = 1, a 64 x 64 window through the silhouette."""
    occ = np.repeat(np.repeat(np.repeat(models[:1], 2, 1), 2, 2), 2, 3)
    window = (96, 112, 64, 64)
    hit, face, cnt, out = device_ao(occ, pose_rad(*POSE)[None], 256, 1, 16, 2, window)
    assert (hit >= 0).mean() > 0.1 and (hit < 0).mean() > 0.1
    want = reference_counts(occ, hit, face, 16)
    assert np.array_equal(cnt, want) and np.array_equal(out, AR.encode(want, 2))
    assert want[hit >= 0].min() < 48


# -- edges ----------------------------------------------------------------------------------------------------------------

def test_empty_and_full_items_and_an_empty_batch():
    import torch
    from rendernet_amd import ops
    occ = np.stack([np.zeros((32, 32, 32), bool), np.ones((32, 32, 32), bool), np.zeros((32, 32, 32), bool)])
    poses = np.tile(pose_rad(*POSE), (3, 1))
    hit, face, cnt, out = device_ao(occ, poses, 64, 2, 8, 2)
    assert (cnt[0] == 255).all() and (out[0] == 0).all() and (cnt[2] == 255).all() and (out[2] == 0).all()
    assert (hit[1] >= 0).sum() > 1000
    want = reference_counts(occ, hit, face, 8)
    assert np.array_equal(cnt, want) and np.array_equal(out, AR.encode(want, 2))
    assert (cnt[1][hit[1] >= 0] == 64).all() and (out[1][hit[1] >= 0] == 255).all()      # a box face sees nothing above it
    vox = torch.zeros((0, 32, 32, 32, 1), device="cuda")
    got = ops.raycast_ao(vox, torch.zeros((0, 3), device="cuda"), new_size=64, pixels_per_cell=2, return_counts=True)
    assert got[0].shape == (0, 128, 128) and got[1].shape == (0, 128, 128) and got[0].dtype is torch.uint8


def test_invalid_arguments_return_invalid_without_a_launch():
    import torch
    from rendernet_amd import _lib, ops
    from rendernet_amd._lib import RenderNetHipError
    lib, vp, st = _lib.lib(), ctypes.c_void_p, _lib.stream_ptr()
    B, S, ph, pw = 2, 32, 20, 24
    bits, box = ops.voxel_pack(torch.ones((B, S, S, S, 1), dtype=torch.uint8, device="cuda"))
    hit = torch.zeros((B, ph, pw), dtype=torch.int32, device="cuda")
    face = torch.zeros((B, ph, pw), dtype=torch.int8, device="cuda")       # voxel 0 by its -x face: nothing in front of it
    cnt = torch.full((B, ph, pw), 7, dtype=torch.uint8, device="cuda")
    out = torch.full((B, ph, pw), 9, dtype=torch.uint8, device="cuda")
    p = {"bits": bits.data_ptr(), "box": box.data_ptr(), "hit": hit.data_ptr(), "face": face.data_ptr(), "cnt": cnt.data_ptr()}

    def ao(B=B, S=S, ph=ph, pw=pw, L=8, **ptr):
        q = dict(p, **ptr)
        return lib.rn_raycast_ao_fwd(vp(q["bits"]), vp(q["box"]), vp(q["hit"]), vp(q["face"]), vp(q["cnt"]), B, S, ph, pw, L, st)

    def enc(B=B, ph=ph, pw=pw, smooth=2, count=cnt.data_ptr(), dst=out.data_ptr()):
        return lib.rn_ao_encode(vp(count), vp(dst), B, ph, pw, smooth, st)

    bad_ao = [dict(B=-1), dict(B=65536), dict(S=48), dict(S=0), dict(S=160), dict(ph=0), dict(pw=0), dict(ph=4097), dict(pw=-3),
              dict(L=0), dict(L=33), dict(bits=None), dict(box=None), dict(hit=None), dict(face=None), dict(cnt=None),
              dict(bits=p["bits"] + 4), dict(box=p["box"] + 2), dict(hit=p["hit"] + 1)]
    for kw in bad_ao:
        assert ao(**kw) == RN_E_INVALID, kw
    bad_enc = [dict(B=-1), dict(B=65536), dict(ph=0), dict(pw=0), dict(pw=4097), dict(smooth=-1), dict(smooth=9), dict(count=None),
               dict(dst=None), dict(dst=cnt.data_ptr())]
    for kw in bad_enc:
        assert enc(**kw) == RN_E_INVALID, kw
    assert b"smooth=9" in lib.rn_last_error() or b"same buffer" in lib.rn_last_error()
    torch.cuda.synchronize()
    assert (cnt == 7).all() and (out == 9).all()                            # nothing was launched
    assert ao(B=0) == 0 and enc(B=0) == 0 and ao(B=0, bits=None) == 0
    torch.cuda.synchronize()
    assert (cnt == 7).all() and (out == 9).all()
    assert ao() == 0 and enc() == 0                                         # ... and the same buffers are accepted as they are
    torch.cuda.synchronize()
    assert (cnt == 64).all() and (out == 255).all()
    vox = torch.zeros((1, 32, 32, 32, 1), device="cuda")
    pose = torch.as_tensor(pose_rad(*POSE)[None]).cuda()
    for kw, msg in (({"max_distance": 0}, "max_distance"), ({"max_distance": 33}, "max_distance"), ({"smooth": 9}, "smooth"),
                    ({"smooth": -1}, "smooth"), ({"window": (0, 0, 0, 16)}, "window")):
        with pytest.raises(RenderNetHipError, match=msg):
            ops.raycast_ao(vox, pose, new_size=64, pixels_per_cell=2, **kw)
    with pytest.raises(RenderNetHipError, match="hit int32"):
        ops.raycast_ao_from_hits(bits, box, hit.long(), face, S)


# -- the trainer ----------------------------------------------------------------------------------------------------------

def test_ao_frames_feed_the_trainer(models):
    """Greyscale frames of SyntheticTargets(shader="ao") are ops.raycast_ao / 255 bit for bit, and a reduced greyscale
    trainer (tiny_spec on 32^3 grids: 32^3 -> 32^3 -> 128^2) takes two steps on them with finite losses."""
    import torch
    from rendernet_amd import ops, synth
    from rendernet_amd.shader import init_shader_weights, tiny_spec
    from rendernet_amd.train import Trainer
    small = models.reshape(2, 32, 2, 32, 2, 32, 2).any(axis=(2, 4, 6)).astype(np.uint8)[..., None]       # 2x2x2 max-pool
    spec = dataclasses.replace(tiny_spec(1), size=32).check()
    tr = Trainer(spec, init_shader_weights(spec, seed=1234), device="cuda", e_eta=1e-4, keep_prob=1.0)
    feed = synth.SyntheticTargets(small, ["chair", "bunny"], 2, 2, seed=3, device="cuda", greyscale=True, new_size=32,
                                  shader="ao", ao_distance=8)
    losses = []
    for frames, vox, poses, names in feed:
        assert frames.dtype is torch.float32 and frames.shape == (2, 128, 128, 1) and frames.is_cuda
        ao = ops.raycast_ao(vox, poses, new_size=32, pixels_per_cell=4, max_distance=8)
        assert ao.shape == (2, 128, 128) and (ao > 0).reshape(2, -1).sum(1).min() > 64
        assert np.array_equal(frames.cpu().numpy()[..., 0], ao.cpu().numpy().astype(np.float32) / np.float32(255.0))
        losses.append(float(tr.step(vox, poses, frames, patch_size=16, start_point=(8, 8)).item()))
    print("losses: %s" % losses)
    assert len(losses) == 2 and np.isfinite(losses).all()
