"""rn_raycast_edges_fwd / rn_lines_encode (rendernet_amd/csrc/raycast.hip), ops.raycast_outline / raycast_cel and
SyntheticTargets(shader="outline" | "cel") against the integer twin tests/raycast_lines_ref.py.  -m gpu.

Both rules are integer functions of (hit voxels, entry faces, occupancy, the quantised light), so every comparison is exact
and covers every pixel: hits, faces and normal bytes come from the device's own rn_raycast_fwd, the twin computes edges and
bytes from those arrays and the host copy of the grid."""
import ctypes
import dataclasses

import numpy as np
import pytest

import raycast_lines_ref as LR
from conftest import FIXTURES
from rendernet_amd._lib import RN_E_INVALID

pytestmark = pytest.mark.gpu
POSES = ((250.0, 30.0, 1.0), (40.0, 65.0, 1.0))                            # azimuth, elevation (degrees), scale
CROP = (37, 5, 45, 83)                                                     # odd origin, no multiple of the 16 x 16 tile, 3735 pixels
DEFAULTS = dict(normal_radius=2, line_radius=2, depth_gap=2, crease_q=4)


def pose_rad(az, el, s):
    return np.array([az * np.pi / 180.0, el * np.pi / 180.0, s], np.float32)


def device_edges(occ, poses, N, f, window=None, **kw):
    """bool grids [B,S,S,S] at poses [B,3] -> (hit, face, normal bytes, edge bytes) as NumPy: the hits of ops.raycast_normals
    and ops.raycast_edges_from_hits on them."""
    import torch
    from rendernet_amd import ops
    p = dict(DEFAULTS, **kw)
    vox = torch.as_tensor(np.ascontiguousarray(occ[..., None]).astype(np.uint8)).cuda()
    m = ops.pose_to_affine(torch.as_tensor(np.asarray(poses, np.float32)).cuda(), occ.shape[1], N)
    rgb, hit, face = ops.raycast_normals(vox, m, new_size=N, pixels_per_cell=f, window=window, affine=True,
                                         normal_radius=p["normal_radius"], return_hits=True)
    bits, box = ops.voxel_pack(vox)
    edge = ops.raycast_edges_from_hits(bits, box, hit, face, occ.shape[1], **p)
    assert edge.dtype is torch.uint8 and edge.shape == hit.shape
    return hit.cpu().numpy(), face.cpu().numpy(), rgb.cpu().numpy(), edge.cpu().numpy()


def twin_edges(occ, hit, face, **kw):
    return np.stack([LR.edges(occ[b], hit[b], face[b], **dict(DEFAULTS, **kw)) for b in range(len(occ))])


def assert_same(got, want, what=""):
    bad = got != want
    assert not bad.any(), "%s: %d pixels differ, first at %s: kernel %d twin %d" % (
        what, bad.sum(), np.argwhere(bad)[0], got[bad][0], want[bad][0])


@pytest.fixture(scope="module")
def models(fixtures_vox):
    """chair and teapot as bool [2,64,64,64] indexed [z,y,x]."""
    return np.stack([fixtures_vox[FIXTURES.index(m), ..., 0] > 0.5 for m in ("chair", "teapot")])


@pytest.fixture(scope="module")
def full_frame(models):
    """The default-parameter cast of both models at POSES[0], 128^2 frames: (hit, face, rgb, edge), computed once."""
    return device_edges(models, np.tile(pose_rad(*POSES[0]), (2, 1)), 32, 4)


# -- models ---------------------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("pose", POSES)
@pytest.mark.parametrize("radii", [(1, 1), (2, 2), (3, 4)])
def test_models_whole_frame(models, radii, pose):
    """chair and teapot, S = 64, N = 32, f = 4 (128^2 frames, 64 tiles each), every corner of (normal_radius, line_radius)."""
    R, lr = radii
    hit, face, _, edge = device_edges(models, np.tile(pose_rad(*pose), (2, 1)), 32, 4, normal_radius=R, line_radius=lr)
    assert edge.shape == (2, 128, 128) and (hit >= 0).reshape(2, -1).sum(1).min() > 1000
    assert_same(edge, twin_edges(models, hit, face, normal_radius=R, line_radius=lr), str(radii))
    assert not edge[hit < 0].any() and edge.max() <= 7
    for b in range(2):
        for bit in (LR.SILHOUETTE, LR.DEPTH, LR.CREASE):
            assert (edge[b] & bit).any(), (b, bit)                          # not an all-zero plane
        assert (edge[b][hit[b] >= 0] == 0).any()                            # ... and not all ink either


def test_thresholds_change_the_bits(models):
    """depth_gap and crease_q at their ends, chair only: still the twin's bytes, and monotone in the threshold."""
    occ, poses = models[:1], pose_rad(*POSES[0])[None]
    seen = {}
    for gap, q in ((1, 0), (2, 4), (127, 8)):
        hit, face, _, edge = device_edges(occ, poses, 32, 4, depth_gap=gap, crease_q=q)
        assert_same(edge, twin_edges(occ, hit, face, depth_gap=gap, crease_q=q), str((gap, q)))
        seen[gap] = edge
    assert not (seen[127] & LR.DEPTH).any() and (seen[1] & LR.DEPTH).sum() > (seen[2] & LR.DEPTH).sum() > 0
    assert (seen[127] & LR.CREASE).sum() > (seen[2] & LR.CREASE).sum() > (seen[1] & LR.CREASE).sum() > 0


@pytest.mark.parametrize("lr", [2, 4])
def test_cropped_window(models, full_frame, lr):
    """Rows 37..81 x columns 5..87: partial tiles on both sides and the window clip.  The bytes equal the twin on the cropped
    hits, and the whole-frame cast wherever the (2 lr + 1)^2 window does not reach the border of the crop."""
    r0, c0, ph, pw = CROP
    poses = np.tile(pose_rad(*POSES[0]), (2, 1))
    hit, face, _, edge = device_edges(models, poses, 32, 4, CROP, line_radius=lr)
    assert edge.shape == (2, ph, pw) and (hit >= 0).any() and (hit < 0).any()
    assert np.array_equal(hit, full_frame[0][:, r0:r0 + ph, c0:c0 + pw])
    assert_same(edge, twin_edges(models, hit, face, line_radius=lr))
    whole = full_frame[3] if lr == 2 else device_edges(models, poses, 32, 4, line_radius=lr)[3]
    assert_same(edge[:, lr:-lr, lr:-lr], whole[:, r0 + lr:r0 + ph - lr, c0 + lr:c0 + pw - lr], "against the whole frame")
    assert (edge[:, :lr] != whole[:, r0:r0 + lr, c0:c0 + pw]).any()         # the clip shows at the border: a miss outside the crop is not seen


def test_grid_of_128_reads_the_mask_from_memory(models):
    """S = 128 (no LDS copy of the mask): the chair upsampled x2, one item, N = 32, f = 4."""
    occ = np.repeat(np.repeat(np.repeat(models[:1], 2, 1), 2, 2), 2, 3)
    hit, face, _, edge = device_edges(occ, pose_rad(*POSES[0])[None], 32, 4, normal_radius=3)
    assert (hit >= 0).mean() > 0.1 and (hit < 0).mean() > 0.1
    assert_same(edge, twin_edges(occ, hit, face, normal_radius=3))
    assert all((edge & bit).any() for bit in (1, 2, 4))


# -- edges of the domain --------------------------------------------------------------------------------------------------

def test_empty_grid_and_empty_batch():
    import torch
    from rendernet_amd import ops
    occ = np.zeros((2, 32, 32, 32), bool)
    occ[1, 10:20, 10:20, 10:20] = True
    hit, face, _, edge = device_edges(occ, np.tile(pose_rad(*POSES[0]), (2, 1)), 32, 2)
    assert not edge[0].any() and (hit[0] < 0).all() and edge[1].any()
    assert_same(edge, twin_edges(occ, hit, face))
    vox = torch.as_tensor(occ[..., None].astype(np.uint8)).cuda()
    pose = torch.as_tensor(np.tile(pose_rad(*POSES[0]), (2, 1))).cuda()
    assert (ops.raycast_outline(vox, pose, new_size=32, pixels_per_cell=2)[0] == 255).all()
    assert (ops.raycast_cel(vox, pose, new_size=32, pixels_per_cell=2)[0] == 255).all()
    got = ops.raycast_cel(vox[:0], pose[:0], new_size=32, pixels_per_cell=2, return_edges=True)
    assert got[0].shape == (0, 64, 64) and got[1].shape == (0, 64, 64) and got[0].dtype is torch.uint8


def test_out_of_range_hits_behave_as_misses(models, full_frame):
    """A few hit_id >= S^3 and face = 7 (and -1) entries injected into the chair's hit plane: misses to the kernel and the twin."""
    import torch
    from rendernet_amd import ops
    hit, face = full_frame[0][:1].copy(), full_frame[1][:1].copy()
    inside = np.argwhere((hit[0] >= 0) & (full_frame[3][0] == 0))            # interior pixels with no line of their own
    inside = inside[(inside.min(1) >= 1) & (inside.max(1) <= 126)]
    assert len(inside) > 200
    picks = inside[:: len(inside) // 6][:6]
    for k, (r, c) in enumerate(picks):
        if k % 3 == 0:
            hit[0, r, c] = 64 ** 3 + k
        elif k % 3 == 1:
            face[0, r, c] = 7
        else:
            hit[0, r, c], face[0, r, c] = np.iinfo(np.int32).max, -1
    vox = torch.as_tensor(models[:1, ..., None].astype(np.uint8)).cuda()
    bits, box = ops.voxel_pack(vox)
    edge = ops.raycast_edges_from_hits(bits, box, torch.as_tensor(hit).cuda(), torch.as_tensor(face).cuda(), 64).cpu().numpy()
    assert_same(edge, twin_edges(models[:1], hit, face))
    for r, c in picks:
        assert edge[0, r, c] == 0 and edge[0, r, c + 1] & LR.SILHOUETTE and edge[0, r + 1, c] & LR.SILHOUETTE


# -- the two pictures -----------------------------------------------------------------------------------------------------

@pytest.mark.parametrize("window", [None, CROP])
def test_outline_and_cel_bytes(models, window):
    """ops.raycast_outline / raycast_cel = twin-encode(device normal bytes, device edge bytes), exactly: the whole frame (the
    word path of the encoder) and the 3735-pixel crop (its byte path); levels 2, 4 and 8, the demo's light and another."""
    import torch
    from rendernet_amd import ops, synth
    from rendernet_amd.tools.Phong_shading import generate_light_pos
    vox = torch.as_tensor(models[..., None].astype(np.uint8)).cuda()
    pose = torch.as_tensor(np.stack([pose_rad(*p) for p in POSES])).cuda()
    kw = dict(new_size=32, pixels_per_cell=4, window=window)
    rgb = ops.raycast_normals(vox, pose, normal_radius=2, **kw).cpu().numpy()
    out, edge = ops.raycast_outline(vox, pose, return_edges=True, **kw)
    out, edge = out.cpu().numpy(), edge.cpu().numpy()
    _, hit, face = ops.raycast_normals(vox, pose, return_hits=True, **kw)
    assert_same(edge, twin_edges(models, hit.cpu().numpy(), face.cpu().numpy()))
    assert_same(out, LR.encode(rgb, edge, 7, 0), "outline")
    assert set(np.unique(out).tolist()) == {0, 255} and (out[rgb.any(-1)] == 255).any() and (out[~rgb.any(-1)] == 255).all()
    for mask in (1, 2, 4):
        assert_same(ops.raycast_outline(vox, pose, edge_mask=mask, **kw).cpu().numpy(), LR.encode(rgb, edge, mask, 0), "mask %d" % mask)
    demo = generate_light_pos(synth.LIGHT_ELEVATION, synth.LIGHT_AZIMUTH)
    for levels, shadow, light in ((4, 64, None), (2, 0, (-1.0, 0.5, 2.0)), (8, 254, (3.0, -1.0, 0.25)), (8, 31, None)):
        got, e2 = ops.raycast_cel(vox, pose, light=light, levels=levels, shadow_byte=shadow, return_edges=True, **kw)
        lq = LR.quantise_light(demo if light is None else light)
        assert lq == ops.quantise_light(demo if light is None else light)
        assert np.array_equal(e2.cpu().numpy(), edge)
        want = LR.encode(rgb, edge, 7, levels, shadow, lq)
        assert_same(got.cpu().numpy(), want, "cel %d %d %s" % (levels, shadow, light))
        tones = set(np.unique(want[(edge == 0) & rgb.any(-1)]).tolist())
        assert tones <= set(LR.tone(np.arange(levels), levels, shadow).tolist()) and len(tones) >= 2
    # a different normal_radius reaches both the cast and the edge stage
    rgb3, hit3, face3 = ops.raycast_normals(vox, pose, normal_radius=3, return_hits=True, **kw)
    out3, edge3 = ops.raycast_cel(vox, pose, normal_radius=3, line_radius=3, return_edges=True, **kw)
    e3 = twin_edges(models, hit3.cpu().numpy(), face3.cpu().numpy(), normal_radius=3, line_radius=3)
    assert_same(edge3.cpu().numpy(), e3)
    assert_same(out3.cpu().numpy(), LR.encode(rgb3.cpu().numpy(), e3, 7, 4, 64, LR.quantise_light(demo)), "cel R 3")


# -- argument checks ------------------------------------------------------------------------------------------------------

def test_invalid_arguments_return_invalid_without_a_launch():
    import torch
    from rendernet_amd import _lib, ops
    from rendernet_amd._lib import RenderNetHipError
    lib, vp, st = _lib.lib(), ctypes.c_void_p, _lib.stream_ptr()
    B, S, ph, pw = 2, 32, 20, 24
    bits, box = ops.voxel_pack(torch.ones((B, S, S, S, 1), dtype=torch.uint8, device="cuda"))
    hit = torch.zeros((B, ph, pw), dtype=torch.int32, device="cuda")       # voxel 0 by its -x face everywhere: no line
    face = torch.zeros((B, ph, pw), dtype=torch.int8, device="cuda")
    rgb = torch.full((B, ph, pw, 3), 200, dtype=torch.uint8, device="cuda")
    edge = torch.full((B, ph, pw), 77, dtype=torch.uint8, device="cuda")
    out = torch.full((B, ph, pw), 9, dtype=torch.uint8, device="cuda")
    p = {"bits": bits.data_ptr(), "box": box.data_ptr(), "hit": hit.data_ptr(), "face": face.data_ptr(), "edge": edge.data_ptr()}

    def edges(B=B, S=S, ph=ph, pw=pw, R=2, lr=2, gap=2, q=4, **ptr):
        a = dict(p, **ptr)
        return lib.rn_raycast_edges_fwd(vp(a["bits"]), vp(a["box"]), vp(a["hit"]), vp(a["face"]), vp(a["edge"]), B, S, ph, pw,
                                        R, lr, gap, q, st)

    def enc(B=B, ph=ph, pw=pw, mask=7, levels=4, shadow=64, l=(0, 0, 32767), n=rgb.data_ptr(), e=edge.data_ptr(), dst=out.data_ptr()):
        return lib.rn_lines_encode(vp(n), vp(e), vp(dst), B, ph, pw, mask, levels, shadow, l[0], l[1], l[2], st)

    bad_edges = [dict(B=-1), dict(B=65536), dict(S=48), dict(S=0), dict(S=160), dict(ph=0), dict(pw=0), dict(ph=4097), dict(pw=-3),
                 dict(R=0), dict(R=4), dict(lr=0), dict(lr=5), dict(gap=0), dict(gap=128), dict(q=-1), dict(q=9),
                 dict(bits=None), dict(box=None), dict(hit=None), dict(face=None), dict(edge=None),
                 dict(bits=p["bits"] + 4), dict(box=p["box"] + 2), dict(hit=p["hit"] + 1)]
    for kw in bad_edges:
        assert edges(**kw) == RN_E_INVALID, kw
    assert b"rn_raycast_edges_fwd" in lib.rn_last_error()
    bad_enc = [dict(B=-1), dict(B=65536), dict(ph=0), dict(pw=0), dict(pw=4097), dict(mask=0), dict(mask=8), dict(levels=1),
               dict(levels=9), dict(levels=-1), dict(shadow=-1), dict(shadow=255), dict(l=(32768, 0, 0)), dict(l=(0, -32768, 0)),
               dict(l=(0, 0, 1 << 20)), dict(n=None), dict(e=None), dict(dst=None), dict(dst=edge.data_ptr()), dict(dst=rgb.data_ptr())]
    for kw in bad_enc:
        assert enc(**kw) == RN_E_INVALID, kw
    assert b"rn_lines_encode" in lib.rn_last_error()
    torch.cuda.synchronize()
    assert (edge == 77).all() and (out == 9).all()                          # nothing was launched
    assert edges(B=0) == 0 and enc(B=0) == 0 and edges(B=0, bits=None) == 0
    torch.cuda.synchronize()
    assert (edge == 77).all() and (out == 9).all()
    assert edges() == 0                                                     # ... and the same buffers are accepted as they are
    torch.cuda.synchronize()
    assert (edge == 0).all()
    assert enc(levels=0) == 0
    torch.cuda.synchronize()
    assert (out == 255).all()
    vox = torch.zeros((1, 32, 32, 32, 1), device="cuda")
    pose = torch.as_tensor(pose_rad(*POSES[0])[None]).cuda()
    for fn, kw, msg in ((ops.raycast_outline, {"line_radius": 5}, "line_radius"), (ops.raycast_outline, {"normal_radius": 0}, "normal_radius"),
                        (ops.raycast_outline, {"depth_gap": 128}, "depth_gap"), (ops.raycast_outline, {"crease_q": 9}, "crease_q"),
                        (ops.raycast_outline, {"edge_mask": 0}, "edge_mask"), (ops.raycast_outline, {"window": (0, 0, 0, 16)}, "window"),
                        (ops.raycast_cel, {"levels": 0}, "levels"), (ops.raycast_cel, {"levels": 9}, "levels"),
                        (ops.raycast_cel, {"shadow_byte": 255}, "shadow_byte"), (ops.raycast_cel, {"light": (0, 0, 0)}, "quantise_light"),
                        (ops.raycast_cel, {"line_radius": 2.0}, "not an integer")):
        with pytest.raises(RenderNetHipError, match=msg):
            fn(vox, pose, new_size=32, pixels_per_cell=2, **kw)
    with pytest.raises(RenderNetHipError, match="hit int32"):
        ops.raycast_edges_from_hits(bits, box, hit.long(), face, S)


# -- the trainer ----------------------------------------------------------------------------------------------------------

def _small(models):
    return models.reshape(2, 32, 2, 32, 2, 32, 2).any(axis=(2, 4, 6)).astype(np.uint8)[..., None]            # 2x2x2 max-pool


def test_outline_frames_of_synthetic_targets(models):
    """Three steps of SyntheticTargets(shader="outline"): greyscale frames are ops.raycast_outline / 255 as a float32 division,
    colour frames carry the byte in three channels."""
    import torch
    from rendernet_amd import ops, synth
    opts = {"line_radius": 1, "crease_q": 2}
    feeds = [synth.SyntheticTargets(_small(models), ["chair", "teapot"], 2, 3, seed=5, device="cuda", greyscale=g, new_size=32,
                                    shader="outline", line_options=opts) for g in (True, False)]
    steps = 0
    for (fg, vox, poses, names), (fc, vox_c, poses_c, names_c) in zip(*feeds):
        assert names == names_c and torch.equal(vox, vox_c) and torch.equal(poses, poses_c)
        byte = ops.raycast_outline(vox, poses, new_size=32, pixels_per_cell=4, **opts).cpu().numpy()
        assert byte.shape == (2, 128, 128) and (byte == 0).reshape(2, -1).sum(1).min() > 64
        assert fg.dtype is torch.float32 and fg.shape == (2, 128, 128, 1) and fg.is_cuda
        assert np.array_equal(fg.cpu().numpy()[..., 0], byte.astype(np.float32) / np.float32(255.0))
        assert fc.dtype is torch.uint8 and fc.shape == (2, 128, 128, 3) and fc.is_contiguous()
        assert np.array_equal(fc.cpu().numpy(), np.repeat(byte[..., None], 3, 3))
        steps += 1
    assert steps == 3


def test_cel_frames_feed_the_trainer(models):
    """A reduced greyscale trainer (tiny_spec on 32^3 grids: 32^3 -> 32^3 -> 128^2) takes five steps on cel targets in the
    default multiply mode with finite losses."""
    import torch
    from rendernet_amd import synth
    from rendernet_amd.shader import init_shader_weights, tiny_spec
    from rendernet_amd.train import Trainer
    spec = dataclasses.replace(tiny_spec(1), size=32).check()
    tr = Trainer(spec, init_shader_weights(spec, seed=1234), device="cuda", e_eta=1e-4, keep_prob=1.0)
    feed = synth.SyntheticTargets(_small(models), ["chair", "teapot"], 2, 5, seed=3, device="cuda", greyscale=True, new_size=32,
                                  shader="cel", line_options={"levels": 3})
    losses = []
    for frames, vox, poses, names in feed:
        assert frames.dtype is torch.float32 and frames.shape == (2, 128, 128, 1) and frames.is_cuda
        values = set(np.unique(np.rint(frames.cpu().numpy() * 255.0)).astype(int).tolist())
        assert values <= {0, 64, 160, 255} and {0, 255} <= values            # ink, the three tones, the white background
        losses.append(float(tr.step(vox, poses, frames, patch_size=16, start_point=(8, 8)).item()))
    print("losses: %s" % losses)
    assert len(losses) == 5 and np.isfinite(losses).all()
