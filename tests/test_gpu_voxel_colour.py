"""The voxel colouring on the device against the NumPy twin (tests/voxel_colour_ref.py), every word: the sums of scanned views with
and without a mask, the resolved and filled colours, the re-rendered pictures and the vertex colours; hand-made hit patterns that
put runs of equal ids across the edges of a wave, of a view and of an item; the per-call limit; the round trip that returns a
colour field from its unsmoothed pictures; chunks, determinism, the three grid sides, empty input and the argument checks.  -m gpu."""
import numpy as np
import pytest

import mesh_extract_ref as XR
import voxel_colour_ref as CR
from rendernet_amd import synth
from test_gpu_voxel_carve import _dev, grids32, poses_for

pytestmark = pytest.mark.gpu

S, N, F = 32, 64, 2
INT_MIN, INT_MAX = -2 ** 31, 2 ** 31 - 1


def _np(t):
    import torch
    torch.cuda.synchronize()
    return t.cpu().numpy()


def same(got, want, what):
    got, want = np.asarray(got), np.asarray(want)
    assert got.shape == want.shape and got.dtype == want.dtype, (what, got.shape, got.dtype, want.shape, want.dtype)
    bad = got != want
    assert not bad.any(), "%s: %d words differ, first at %s: device %s twin %s" % (
        what, bad.sum(), np.argwhere(bad)[0], got[bad][0], want[bad][0])


_scans = {}


def scan32(window):
    """(vox, hits [3,6,ph,pw], images, mask) of grids32 under scan_poses(6), all on the device, made once per window; the
    pictures and the mask are random bytes: the sums are held to the rule, not to plausible pictures."""
    from rendernet_amd import ops
    if window not in _scans:
        poses, low = poses_for(3, 6)
        vox = _dev(grids32().astype(np.uint8)[..., None])
        _, hits = ops.voxel_scan(vox, _dev(poses), new_size=N, pixels_per_cell=F, window=window, view_from_low_x=low, return_hits=True)
        rng = np.random.default_rng(21)
        shape = tuple(hits.shape)
        images = rng.integers(0, 256, shape + (3,)).astype(np.uint8)
        mask = rng.choice(np.array([0, 0, 1, 255, 7], np.uint8), shape)
        _scans[window] = (vox, hits, _dev(images), _dev(mask))
    return _scans[window]


@pytest.mark.parametrize("window", [None, (5, 9, 101, 77)])
def test_scanned_views_against_the_twin(window):
    import torch
    from rendernet_amd import ops
    vox, hits, images, mask = scan32(window)
    ph, pw = (F * N, F * N) if window is None else window[2:]
    assert hits.dtype is torch.int32 and tuple(hits.shape) == (3, 6, ph, pw)
    h, img, msk, occ = _np(hits), _np(images), _np(mask), grids32()
    assert (h[:2] >= 0).sum() > 1000 and (h[2] == -1).all()
    for use_mask in (False, True):
        sums = ops.voxel_colour_sums(images, hits, S, mask if use_mask else None)
        assert sums.dtype is torch.int32 and tuple(sums.shape) == (3, S, S, S, 4)
        want_sums = CR.accumulate(img, h, S, msk if use_mask else None)
        same(_np(sums), want_sums, "sums")
        assert want_sums[..., 3].max() > 4                               # several pixels per voxel: the means are means
        for fill in (0, 1, 3):
            col, known = ops.voxel_colours(sums, vox if fill else None, fill=fill, unseen=(1, 2, 3))
            want_col, want_known = CR.colours_of(want_sums, occ, fill, (1, 2, 3))
            same(_np(col), want_col, "colours, fill %d" % fill)
            same(_np(known), want_known, "known, fill %d" % fill)
            if fill:
                assert (want_known == 2).sum() > 0
        # colours and known are now those of fill = 3
        for smooth in (0, 2):
            pic = ops.colour_from_hits(hits[:, 1].contiguous(), col, S, smooth=smooth, background=(9, 200, 30))
            same(_np(pic), CR.from_hits(h[:, 1], want_col, S, smooth, (9, 200, 30)), "picture, smooth %d" % smooth)
        for smooth in (True, False):
            m = ops.extract_mesh(vox, smooth=smooth)
            vc = ops.mesh_vertex_colours(m, col, known, unseen=(4, 5, 6))
            assert vc.dtype is torch.uint8 and tuple(vc.shape) == (int(m.q.shape[0]), 3) and int(m.q.shape[0]) > 1000
            want_vc = CR.vertex_colours(_np(m.q), _np(m.vert_offsets), want_col, want_known, (4, 5, 6))
            same(_np(vc), want_vc, "vertex colours, smooth %s" % smooth)
            assert (want_vc == (4, 5, 6)).all(1).sum() > 0 and (want_vc != (4, 5, 6)).any(1).sum() > 1000


# ---- hand-made hits: 101 x 77 = 7777 pixels a view, no multiple of 64, so waves span views and the last wave of an item is ragged

PH, PW, B3, K2 = 101, 77, 3, 2


def pattern(name):
    """(hits int32 [3,2,101,77], mask or None)"""
    rng = np.random.default_rng(sum(name.encode()))
    n = K2 * PH * PW
    p = np.arange(n, dtype=np.int64)
    mask = None
    if name == "one_id":
        h = np.full(n, 12345, np.int64)
    elif name == "two_ids_alternating":
        h = np.where(p % 2 == 0, 77, S ** 3 - 1)
    elif name in ("runs_63", "runs_64", "runs_65"):
        h = (p // int(name[5:])) * 37 % S ** 3
    elif name == "random_and_invalid":
        h = rng.integers(0, S ** 3, n)
        kind = rng.integers(0, 10, n)
        for k, v in ((0, -1), (1, S ** 3), (2, INT_MIN), (3, INT_MAX)):
            h = np.where(kind == k, v, h)
        h = np.where(kind >= 7, 4242, h)                                 # and runs of one id between them
    elif name == "mask_zeros_in_a_run":
        h = (p // 200) % 5 + 1000
        mask = (rng.random((B3, n)) < 0.7).astype(np.uint8) * 255
    else:
        raise KeyError(name)
    h = np.broadcast_to(h, (B3, n)).copy()
    h[1] = np.roll(h[1], 13)                                             # the items' runs do not line up
    return h.reshape(B3, K2, PH, PW).astype(np.int32), None if mask is None else mask.reshape(B3, K2, PH, PW)


@pytest.mark.parametrize("name", ["one_id", "two_ids_alternating", "runs_63", "runs_64", "runs_65", "random_and_invalid",
                                  "mask_zeros_in_a_run"])
def test_hand_made_hits(name):
    from rendernet_amd import ops
    h, mask = pattern(name)
    img = np.random.default_rng(4).integers(0, 256, (B3, K2, PH, PW, 3)).astype(np.uint8)     # every item its own pictures
    sums = ops.voxel_colour_sums(_dev(img), _dev(h), S, None if mask is None else _dev(mask))
    want = CR.accumulate(img, h, S, mask)
    same(_np(sums), want, name)
    assert want[..., 3].sum() == CR.counts(h, S, mask).sum() > 0
    assert not np.array_equal(want[0], want[2])                          # the same hits, other pictures: joined items would show


def test_limit_of_one_call():
    import torch
    from rendernet_amd import ops
    from rendernet_amd._lib import RenderNetHipError
    img = torch.full((1, 128, 256, 256, 3), 255, dtype=torch.uint8, device="cuda")
    hits = torch.full((1, 128, 256, 256), 31337, dtype=torch.int32, device="cuda")
    sums = ops.voxel_colour_sums(img, hits, S)
    torch.cuda.synchronize()
    assert sums.view(-1, 4)[31337].tolist() == [2139095040, 2139095040, 2139095040, 8388608]
    assert int((sums != 0).sum()) == 4
    img = torch.empty((1, 129, 256, 256, 3), dtype=torch.uint8, device="cuda")
    hits = torch.empty((1, 129, 256, 256), dtype=torch.int32, device="cuda")
    with pytest.raises(RenderNetHipError, match="8421504"):
        ops.voxel_colour_sums(img, hits, S)


# ---- the round trip ---------------------------------------------------------------------------------------------------------------

def albedo_views(vox, poses, low, cm, code_q, **kw):
    """uint8 [B,K,ph,pw,3]: raycast_albedo at smooth = 0, view by view."""
    import torch
    from rendernet_amd import ops
    waves = _dev(cm.waves)
    return torch.stack([ops.raycast_albedo(vox, poses[:, k].contiguous(), waves, code_q, cm.base, smooth=0, view_from_low_x=low[k],
                                           **kw)[0] for k in range(poses.shape[1])], 1)


def test_round_trip_returns_the_field():
    import torch
    from rendernet_amd import ops
    p, low = poses_for(3, 6)
    poses, vox = _dev(p), _dev(grids32().astype(np.uint8)[..., None])
    kw = dict(new_size=N, pixels_per_cell=F)
    cm = synth.ColourModel(3, 8)
    code_q = _dev(cm.quantise(np.random.default_rng(3).standard_normal((3, 8))))
    images = albedo_views(vox, poses, low, cm, code_q, **kw)
    _, hits = ops.voxel_scan(vox, poses, view_from_low_x=low, return_hits=True, **kw)
    col, known = ops.voxel_colours(ops.voxel_colour_sums(images, hits, S), unseen=(128, 128, 128))
    every = torch.arange(S ** 3, dtype=torch.int32, device="cuda").view(1, S, S * S).expand(3, -1, -1).contiguous()
    field = ops.albedo_from_hits(every, _dev(cm.waves), code_q, S, cm.base, smooth=0).view(3, S, S, S, 3)
    seen = known == 1
    # the CPU twin caster sees 1333 voxels of the sphere from these six poses (tests/test_voxel_colour_cpu.py prints it): half
    assert int(seen[0].sum()) >= 666 and int(seen[1].sum()) >= 666 and int(seen[2].sum()) == 0
    assert torch.equal(col[seen], field[seen]) and bool((col[~seen] == 128).all()) and int(known.max()) == 1
    for k in range(6):
        again = ops.raycast_colour(vox, col, poses[:, k].contiguous(), view_from_low_x=low[k], **kw)
        assert torch.equal(again, images[:, k]), "view %d" % k
    # a pose that is not in the set: the albedo where the hit voxel is known, `unseen` on the other hits, the background elsewhere
    novel = _dev(np.broadcast_to(np.float32([2.0, 0.6, 1.0]), (3, 3)).copy())
    pic, hit = ops.raycast_colour(vox, col, novel, background=(0, 0, 0), return_hits=True, **kw)
    alb = ops.raycast_albedo(vox, novel, _dev(cm.waves), code_q, cm.base, smooth=0, **kw)[0]
    is_hit = hit >= 0
    kn = torch.zeros_like(is_hit)
    kn[is_hit] = (known.view(3, -1).gather(1, hit.clamp(min=0).view(3, -1).long()).view_as(hit) == 1)[is_hit]
    assert int(kn.sum()) > 1000 and int((is_hit & ~kn).sum()) > 0
    assert torch.equal(pic[kn], alb[kn]) and bool((pic[is_hit & ~kn] == 128).all()) and bool((pic[~is_hit] == 0).all())


def test_chunks_of_views_add_up_and_calls_repeat():
    import torch
    from rendernet_amd import ops
    _, hits, images, mask = scan32((5, 9, 101, 77))
    whole = ops.voxel_colour_sums(images, hits, S, mask)
    part = ops.voxel_colour_sums(images[:, :4].contiguous(), hits[:, :4].contiguous(), S, mask[:, :4].contiguous())
    both = ops.voxel_colour_sums(images[:, 4:].contiguous(), hits[:, 4:].contiguous(), S, mask[:, 4:].contiguous(), sums=part)
    assert both is part and torch.equal(both, whole)
    again = ops.voxel_colour_sums(images, hits, S, mask)
    assert torch.equal(again, whole)                                     # integer adds commute: the same bits
    a = ops.voxel_colours(whole, scan32((5, 9, 101, 77))[0], fill=2)
    b = ops.voxel_colours(again, scan32((5, 9, 101, 77))[0], fill=2)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])


@pytest.mark.parametrize("side", [64, 128])
def test_larger_grids(side):
    from rendernet_amd import ops
    occ = XR.sphere_field(side) > np.float32(0.5)
    vox = _dev(occ.astype(np.uint8)[None, ..., None])
    p, low = poses_for(1, 2)
    _, hits = ops.voxel_scan(vox, _dev(p), new_size=2 * side, pixels_per_cell=F, view_from_low_x=low, return_hits=True)
    h = _np(hits)
    img = np.random.default_rng(side).integers(0, 256, h.shape + (3,)).astype(np.uint8)
    sums = ops.voxel_colour_sums(_dev(img), hits, side)
    want_sums = CR.accumulate(img, h, side)
    same(_np(sums), want_sums, "sums")
    assert (want_sums[..., 3] > 0).sum() > 2000 and h.max() > side ** 3 // 2
    col, known = ops.voxel_colours(sums, vox, fill=1)
    want_col, want_known = CR.colours_of(want_sums, occ[None], 1)
    same(_np(col), want_col, "colours")
    same(_np(known), want_known, "known")
    same(_np(ops.colour_from_hits(hits[:, 0].contiguous(), col, side, background=(1, 1, 1))), CR.from_hits(h[:, 0], want_col, side, 0, (1, 1, 1)),
         "picture")
    m = ops.extract_mesh(vox)
    same(_np(ops.mesh_vertex_colours(m, col, known)), CR.vertex_colours(_np(m.q), _np(m.vert_offsets), want_col, want_known),
         "vertex colours")


def test_empty_batch_is_a_no_op():
    import torch
    from rendernet_amd import ops
    dev = "cuda"
    sums = ops.voxel_colour_sums(torch.empty((0, 2, 8, 8, 3), dtype=torch.uint8, device=dev),
                                 torch.empty((0, 2, 8, 8), dtype=torch.int32, device=dev), S)
    assert tuple(sums.shape) == (0, S, S, S, 4) and sums.dtype is torch.int32
    vox = torch.empty((0, S, S, S, 1), dtype=torch.uint8, device=dev)
    col, known = ops.voxel_colours(sums, vox, fill=2)
    assert tuple(col.shape) == (0, S, S, S, 3) and tuple(known.shape) == (0, S, S, S)
    assert tuple(ops.colour_from_hits(torch.empty((0, 8, 8), dtype=torch.int32, device=dev), col, S, smooth=1).shape) == (0, 8, 8, 3)
    assert tuple(ops.raycast_colour(vox, col, torch.empty((0, 3), device=dev), new_size=N, pixels_per_cell=F).shape) == (0, 128, 128, 3)
    assert tuple(ops.mesh_vertex_colours(ops.extract_mesh(vox), col, known).shape) == (0, 3)
    views, hits = ops.voxel_scan(vox, torch.empty((0, 2, 3), device=dev), new_size=N, pixels_per_cell=F, return_hits=True)
    assert tuple(views.shape) == tuple(hits.shape) == (0, 2, 128, 128)


def test_argument_checks():
    import torch
    from rendernet_amd import ops
    from rendernet_amd._lib import RenderNetHipError as E
    dev = "cuda"
    img = torch.zeros((2, 3, 8, 9, 3), dtype=torch.uint8, device=dev)
    hits = torch.zeros((2, 3, 8, 9), dtype=torch.int32, device=dev)
    mask = torch.ones((2, 3, 8, 9), dtype=torch.uint8, device=dev)
    sums = ops.voxel_colour_sums(img, hits, S, mask)
    vox = torch.zeros((2, S, S, S, 1), dtype=torch.uint8, device=dev)
    col, known = ops.voxel_colours(sums, vox, fill=1)
    mesh = ops.extract_mesh(vox)
    hit = hits[:, 0].contiguous()
    pose = torch.zeros((2, 3), device=dev)
    bad = [
        # voxel_colour_sums
        ("images", lambda: ops.voxel_colour_sums(img.float(), hits, S)),
        ("images", lambda: ops.voxel_colour_sums(img[..., :2], hits, S)),
        ("images", lambda: ops.voxel_colour_sums(img[0], hits, S)),
        ("images", lambda: ops.voxel_colour_sums(img.cpu().numpy(), hits, S)),
        ("HIP tensors", lambda: ops.voxel_colour_sums(img.cpu(), hits, S)),
        ("hits", lambda: ops.voxel_colour_sums(img, hits.long(), S)),
        ("hits", lambda: ops.voxel_colour_sums(img, hits[:, :2], S)),
        ("hits", lambda: ops.voxel_colour_sums(img, hits.cpu(), S)),
        ("hits", lambda: ops.voxel_colour_sums(img, None, S)),
        ("mask", lambda: ops.voxel_colour_sums(img, hits, S, mask.bool())),
        ("mask", lambda: ops.voxel_colour_sums(img, hits, S, mask[..., :8])),
        ("mask", lambda: ops.voxel_colour_sums(img, hits, S, mask.cpu())),
        ("S=", lambda: ops.voxel_colour_sums(img, hits, 48)),
        ("S=", lambda: ops.voxel_colour_sums(img, hits, 32.0)),
        ("sums", lambda: ops.voxel_colour_sums(img, hits, S, sums=sums.float())),
        ("sums", lambda: ops.voxel_colour_sums(img, hits, S, sums=sums[:1])),
        ("sums", lambda: ops.voxel_colour_sums(img, hits, S, sums=sums.cpu())),
        ("sums", lambda: ops.voxel_colour_sums(img, hits, S, sums=torch.zeros((2, S, S, S, 8), dtype=torch.int32, device=dev)[..., ::2])),
        ("pixels", lambda: ops.voxel_colour_sums(torch.zeros((1, 1, 4097, 1, 3), dtype=torch.uint8, device=dev),
                                                 torch.zeros((1, 1, 4097, 1), dtype=torch.int32, device=dev), S)),
        # voxel_colours
        ("sums", lambda: ops.voxel_colours(sums.float())),
        ("sums", lambda: ops.voxel_colours(sums[..., :3])),
        ("sums", lambda: ops.voxel_colours(torch.zeros((1, 48, 48, 48, 4), dtype=torch.int32, device=dev))),
        ("HIP tensors", lambda: ops.voxel_colours(sums.cpu())),
        ("needs vox", lambda: ops.voxel_colours(sums, fill=1)),
        ("fill", lambda: ops.voxel_colours(sums, vox, fill=65)),
        ("fill", lambda: ops.voxel_colours(sums, vox, fill=-1)),
        ("fill", lambda: ops.voxel_colours(sums, vox, fill=1.0)),
        ("vox", lambda: ops.voxel_colours(sums, vox[:1], fill=1)),
        ("HIP tensors", lambda: ops.voxel_colours(sums, vox.cpu(), fill=1)),
        ("unseen", lambda: ops.voxel_colours(sums, unseen=(1, 2))),
        ("unseen", lambda: ops.voxel_colours(sums, unseen=(1, 2, 256))),
        ("threshold", lambda: ops.voxel_colours(sums, vox, threshold=float("nan"), fill=1)),
        # colour_from_hits
        ("hit", lambda: ops.colour_from_hits(hits, col, S)),
        ("hit", lambda: ops.colour_from_hits(hit.long(), col, S)),
        ("colours", lambda: ops.colour_from_hits(hit, col.float(), S)),
        ("colours", lambda: ops.colour_from_hits(hit, col[..., :2], S)),
        ("colours", lambda: ops.colour_from_hits(hit, col[:1], S)),
        ("colours", lambda: ops.colour_from_hits(hit, col, 64)),
        ("HIP tensors", lambda: ops.colour_from_hits(hit, col.cpu(), S)),
        ("smooth", lambda: ops.colour_from_hits(hit, col, S, smooth=9)),
        ("background", lambda: ops.colour_from_hits(hit, col, S, background=(0, 0, -1))),
        # raycast_colour
        ("colours", lambda: ops.raycast_colour(vox, col[:1], pose, new_size=N, pixels_per_cell=F)),
        ("colours", lambda: ops.raycast_colour(vox, known, pose, new_size=N, pixels_per_cell=F)),
        ("smooth", lambda: ops.raycast_colour(vox, col, pose, new_size=N, pixels_per_cell=F, smooth=-1)),
        ("window", lambda: ops.raycast_colour(vox, col, pose, new_size=N, pixels_per_cell=F, window=(0, 0, 129, 8))),
        ("occupancy", lambda: ops.raycast_colour(vox[:, :16], col, pose, new_size=N, pixels_per_cell=F)),
        # mesh_vertex_colours
        ("ExtractedMesh", lambda: ops.mesh_vertex_colours((mesh.q, mesh.faces), col, known)),
        ("known", lambda: ops.mesh_vertex_colours(mesh, col, known.float())),
        ("known", lambda: ops.mesh_vertex_colours(mesh, col, known[:1])),
        ("known", lambda: ops.mesh_vertex_colours(mesh, col, known.cpu())),
        ("colours", lambda: ops.mesh_vertex_colours(mesh, known, known)),
        ("offsets", lambda: ops.mesh_vertex_colours(mesh, col[:1], known[:1])),
        ("unseen", lambda: ops.mesh_vertex_colours(mesh, col, known, unseen="grey")),
        # voxel_scan
        ("return_hits", lambda: ops.voxel_scan(vox, torch.zeros((2, 2, 3), device=dev), new_size=N, pixels_per_cell=F, return_hits=1)),
    ]
    for word, call in bad:
        with pytest.raises(E, match=word):
            call()
    # nothing above touched the sums
    assert torch.equal(sums, ops.voxel_colour_sums(img, hits, S, mask))
