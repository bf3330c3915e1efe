"""rn_voxel_carve / rn_hit_depth on the device against the NumPy twin (tests/voxel_carve_ref.py): votes and hull exactly on every
voxel, the twin fed the `cam` and the `views` the device produced; the entry depth within +-1 unit on hits and -1 exactly on
misses; windows, both `outside` modes, the options, arbitrary view content, the three grid sides, the view-count limits, empty
and singular input, determinism, the scan-and-carve round trip, and the argument checks.  -m gpu."""
import os

import numpy as np
import pytest

import mesh_extract_ref as XR
import voxel_carve_ref as VC
from conftest import BINVOX_DIR
from rendernet_amd import synth

pytestmark = pytest.mark.gpu


def _dev(a, dtype=None):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def chair():
    from oracle.io_phong import read_binvox
    return read_binvox(os.path.join(BINVOX_DIR, "chair.binvox")).astype(bool)


def grids32():
    """sphere, 30 % noise inside an empty 2-voxel border, and an empty grid: bool [3,32,32,32]"""
    noise = np.zeros((32,) * 3, bool)
    noise[2:-2, 2:-2, 2:-2] = np.random.default_rng(5).random((28,) * 3) < 0.3
    return np.stack([XR.sphere_field(32) > np.float32(0.5), noise, np.zeros((32,) * 3, bool)])


def poses_for(B, K, scale=1.0):
    poses, low = synth.scan_poses(K, scale)
    return np.broadcast_to(poses, (B, K, 3)).copy(), low


def carve_against_twin(views, poses, low, S, N, f, window=None, affine=False, **opts):
    """One device call over the batch, the twin per item on the device's cameras: returns the device's (hull, votes) as arrays."""
    import torch
    from rendernet_amd import ops
    kw = dict(new_size=N, pixels_per_cell=f, affine=affine, view_from_low_x=low)
    hull, votes = ops.voxel_carve(views, poses, S, window=window, return_votes=True, **kw, **opts)
    cam = ops.carve_cameras(poses, S, **kw)
    torch.cuda.synchronize()
    B, K = int(views.shape[0]), int(views.shape[1])
    assert hull.dtype is torch.uint8 and tuple(hull.shape) == (B, S, S, S, 1)
    assert votes.dtype is torch.uint8 and tuple(votes.shape) == (B, S, S, S)
    hull, votes, cam, v = hull.cpu().numpy()[..., 0], votes.cpu().numpy(), cam.cpu().numpy(), views.cpu().numpy()
    win = (0, 0, f * N, f * N) if window is None else window
    for b in range(B):
        w_votes, w_hull = VC.carve(v[b], cam[b], S, win, opts.get("use_depth", True), opts.get("slack", 8),
                                   opts.get("outside", "keep") == "keep", opts.get("tolerance", 0))
        bad = votes[b] != w_votes
        assert not bad.any(), "item %d: %d voxels differ, first at %s: device %d twin %d" % (
            b, bad.sum(), np.argwhere(bad)[0], votes[b][bad][0], w_votes[bad][0])
        assert np.array_equal(hull[b].astype(bool), w_hull)
    return hull, votes


_scans = {}


def scan32(window):
    """views [3,6,ph,pw] of grids32 under scan_poses(6) at S = 32, N = 64, f = 2, scanned once per window."""
    from rendernet_amd import ops
    if window not in _scans:
        poses, low = poses_for(3, 6)
        views = ops.voxel_scan(_dev(grids32().astype(np.uint8)[..., None]), _dev(poses), new_size=64, pixels_per_cell=2,
                               window=window, view_from_low_x=low)
        _scans[window] = (views, _dev(poses), low)
    return _scans[window]


@pytest.mark.parametrize("window", [None, (5, 9, 101, 77)])
def test_scanned_views_every_option(window):
    views, poses, low = scan32(window)
    assert int((views >= 0).sum()) > 1000
    seen = set()
    for use_depth in (True, False):
        for slack in (0, 8):
            for tolerance in (0, 2):
                for outside in ("keep", "carve"):
                    hull, _ = carve_against_twin(views, poses, low, 32, 64, 2, window, use_depth=use_depth, slack=slack,
                                                 tolerance=tolerance, outside=outside)
                    seen.add(hull.tobytes())
                    assert not hull[2].any() or (window is not None and outside == "keep")     # the empty grid
    assert len(seen) >= 4                                        # the options do change the answer
    # the sphere is inside every hull that depth carved from the full frame
    if window is None:
        hull, _ = carve_against_twin(views, poses, low, 32, 64, 2, None)
        g = grids32()
        assert not (g[0] & ~hull[0].astype(bool)).any() and not (g[1] & ~hull[1].astype(bool)).any()


@pytest.mark.parametrize("window", [None, (5, 9, 101, 77)])
def test_arbitrary_view_content(window):
    """-1, 0 and values up to 256 N in no pattern: the kernel is held to the rule, not to plausible input."""
    N, f, B, K = 64, 2, 3, 6
    ph, pw = (f * N, f * N) if window is None else window[2:]
    rng = np.random.default_rng(11)
    v = rng.integers(0, 256 * N + 1, size=(B, K, ph, pw))
    kind = rng.random((B, K, ph, pw))
    v = np.where(kind < 0.3, -1, np.where(kind < 0.4, 0, v)).astype(np.int32)
    poses, low = poses_for(B, K)
    for opts in (dict(), dict(slack=0, tolerance=2, outside="carve"), dict(use_depth=False, tolerance=1)):
        _, votes = carve_against_twin(_dev(v), _dev(poses), low, 32, N, f, window, **opts)
    assert 0 < votes.mean() < K


def test_chair_64_in_a_window():
    from rendernet_amd import ops
    window = (190, 203, 112, 96)                                 # rows 190 .. 301, columns 203 .. 298 of the 512^2 frame
    poses, low = poses_for(1, 3)
    vox = _dev(chair().astype(np.uint8)[None, ..., None])
    views = ops.voxel_scan(vox, _dev(poses), new_size=128, pixels_per_cell=4, window=window, view_from_low_x=low)
    assert int((views >= 0).sum()) > 1000
    for outside in ("keep", "carve"):
        carve_against_twin(views, _dev(poses), low, 64, 128, 4, window, outside=outside)


def test_side_128():
    """S = 128 in a frame of N = 128 cells at f = 2: the grid's corners fall outside the 256^2 frame and beyond the rays' ends,
    so only the rule is checked here, not the property."""
    from rendernet_amd import ops
    occ = np.repeat(np.repeat(np.repeat(chair(), 2, 0), 2, 1), 2, 2)
    poses, low = poses_for(1, 2)
    views = ops.voxel_scan(_dev(occ.astype(np.uint8)[None, ..., None]), _dev(poses), new_size=128, pixels_per_cell=2,
                           view_from_low_x=low)
    assert int((views >= 0).sum()) > 10000
    hull, votes = carve_against_twin(views, _dev(poses), low, 128, 128, 2)
    assert 0 < int(hull.sum()) < 128 ** 3
    carve_against_twin(views, _dev(poses), low, 128, 128, 2, outside="carve", slack=0)


@pytest.mark.parametrize("K", [1, 255])
def test_view_count_limits(K):
    """K = 1, and K = 255 copies of one 64 x 64 view (N = 32, f = 2): votes reaches the top of a byte."""
    from rendernet_amd import ops
    occ = XR.sphere_field(32) > np.float32(0.5)
    one = np.asarray([[[0.7, 0.6, 1.0]]], np.float32)
    view = ops.voxel_scan(_dev(occ.astype(np.uint8)[None, ..., None]), _dev(one), new_size=32, pixels_per_cell=2)
    views = view.expand(1, K, 64, 64).contiguous()
    poses = _dev(np.broadcast_to(one, (1, K, 3)).copy())
    hull, votes = carve_against_twin(views, poses, False, 32, 32, 2, tolerance=0)
    assert set(np.unique(votes).tolist()) == {0, K}
    assert not (occ & ~hull[0].astype(bool)).any()


def test_empty_batch():
    import torch
    from rendernet_amd import ops
    views = torch.empty((0, 4, 128, 128), dtype=torch.int32, device="cuda")
    poses = torch.empty((0, 4, 3), dtype=torch.float32, device="cuda")
    hull, votes = ops.voxel_carve(views, poses, 32, new_size=64, pixels_per_cell=2, return_votes=True)
    assert tuple(hull.shape) == (0, 32, 32, 32, 1) and tuple(votes.shape) == (0, 32, 32, 32)
    assert tuple(ops.voxel_scan(torch.empty((0, 32, 32, 32, 1), dtype=torch.uint8, device="cuda"), poses, 64, 2).shape) == (0, 4, 128, 128)


def test_singular_matrix():
    """A matrix without an inverse gives the zero camera, and the rule is applied as written: every voxel looks at pixel (0, 0)
    of the frame with D = 0."""
    from rendernet_amd import ops
    N, f, K = 64, 2, 3
    poses, low = poses_for(1, K)
    m = ops.pose_to_affine(_dev(poses[0]), 32, N).view(1, K, 3, 4).clone()
    m[0, 1] = 0.0
    m[0, 2, :, 0] = m[0, 2, :, 1]                                # two equal columns
    cam = ops.carve_cameras(m, 32, N, f, affine=True, view_from_low_x=low)
    assert int(cam[0, 1].abs().sum()) == 0 and int(cam[0, 2].abs().sum()) == 0 and int(cam[0, 0].abs().sum()) > 0
    v = np.random.default_rng(3).integers(-1, 256 * N + 1, size=(1, K, f * N, f * N)).astype(np.int32)
    for v00 in (-1, 0, 9):
        v[0, 1:, 0, 0] = v00
        carve_against_twin(_dev(v), m, low, 32, N, f, affine=True, slack=8, tolerance=2)
    for window in ((0, 0, 50, 50), (3, 3, 50, 50)):              # pixel (0, 0) inside the window, and outside it
        r0, c0, ph, pw = window
        carve_against_twin(_dev(v[:, :, r0:r0 + ph, c0:c0 + pw]), m, low, 32, N, f, window=window, affine=True, tolerance=2)


def test_two_calls_bit_for_bit():
    import torch
    from rendernet_amd import ops
    views, poses, low = scan32(None)
    kw = dict(new_size=64, pixels_per_cell=2, view_from_low_x=low, return_votes=True)
    a = ops.voxel_carve(views, poses, 32, **kw)
    b = ops.voxel_carve(views, poses, 32, **kw)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    assert torch.equal(ops.voxel_scan(_dev(grids32().astype(np.uint8)[..., None]), poses, 64, 2, view_from_low_x=low), views)
    # the hull as a bit grid: the existing pack on votes
    bits, _ = ops.voxel_pack(a[1], 6 - 0 - 0.5)
    want, _ = ops.voxel_pack(a[0], 0.5)
    assert torch.equal(bits, want)


@pytest.mark.parametrize("window,low", [(None, False), ((37, 11, 83, 109), True)])
def test_hit_depth_against_the_twin(window, low):
    import torch
    from rendernet_amd import ops
    S, N, f = 32, 64, 4
    g = grids32()
    pose = np.asarray([(4.36, 0.52, 1.0), (0.3, 1.2, 0.9), (2.0, 0.4, 1.1)], np.float32)
    m = ops.pose_to_affine(_dev(pose), S, N)
    _, hit, face = ops.raycast_normals(_dev(g.astype(np.uint8)[..., None]), m, new_size=N, pixels_per_cell=f, window=window,
                                       affine=True, view_from_low_x=low, return_hits=True)
    hit, face = hit.clone(), face.clone()
    hit[0, 0, :6] = torch.tensor([-5, S ** 3, 2 ** 31 - 1, -2 ** 31, S ** 3 - 1, 0], dtype=torch.int32)   # not hits, and the two ends
    face[0, 1, :4] = torch.tensor([6, -1, 127, -128], dtype=torch.int8)
    hit[0, 1, :4] = 5
    depth = ops.hit_depth(hit, face, m, S, new_size=N, pixels_per_cell=f, window=window, affine=True, view_from_low_x=low)
    assert depth.dtype is torch.int32 and depth.shape == hit.shape
    depth, hit, face, M = depth.cpu().numpy(), hit.cpu().numpy(), face.cpu().numpy(), m.cpu().numpy()
    assert (depth[0, 0, :4] == -1).all() and (depth[0, 1, :4] == -1).all()
    hits = 0
    for b in range(3):
        want = VC.hit_depth(hit[b], face[b], M[b], S, N, f, window, low)
        miss = want < 0
        assert np.array_equal(depth[b] < 0, miss) and (depth[b][miss] == -1).all()
        diff = depth[b][~miss].astype(np.int64) - want[~miss]
        assert diff.size == 0 or (np.abs(diff).max() <= 1), (b, diff.min(), diff.max())
        assert (depth[b][~miss] >= 0).all() and (depth[b][~miss] <= 256 * N).all()
        hits += int((~miss).sum())
    assert hits > 3000 and (depth[2] == -1).all()


def test_scan_and_carve_returns_the_chair():
    """End to end on the device: the chair at 64^3, scan_poses(24), two pixels per voxel.  The hull contains every voxel of the
    grid, and its IoU with the grid is at least 0.999 (the twin gives 1.0; the margin is for the +-1 unit of the depth)."""
    import torch
    from rendernet_amd import ops
    occ = chair()
    vox = _dev(occ.astype(np.uint8)[None, ..., None])
    poses, low = poses_for(1, 24)
    views = ops.voxel_scan(vox, _dev(poses), new_size=128, pixels_per_cell=2, view_from_low_x=low)
    hull = ops.voxel_carve(views, _dev(poses), 64, new_size=128, pixels_per_cell=2, view_from_low_x=low)
    ppv = ops.carve_pixels_per_voxel(ops.carve_cameras(_dev(poses), 64, 128, 2, view_from_low_x=low))
    assert tuple(ppv.shape) == (1, 24) and float(ppv.min()) >= 1.5 and abs(float(ppv.mean()) - 2.0) < 1e-3
    lost = int(((vox > 0) & (hull == 0)).sum())
    assert lost == 0
    iou = float(ops.voxel_shape_metrics(hull, vox).iou[0])
    print("scan-and-carve of the chair, 24 views: hull %d voxels, grid %d, IoU %.6f" % (int(hull.sum()), int(occ.sum()), iou))
    assert iou >= 0.999


def test_argument_checks(monkeypatch):
    import torch
    from rendernet_amd import ops
    from rendernet_amd._lib import RenderNetHipError as E
    N, f, K = 64, 2, 4
    views = torch.zeros((2, K, 128, 128), dtype=torch.int32, device="cuda")
    poses, low = poses_for(2, K)
    poses = _dev(poses)
    kw = dict(new_size=N, pixels_per_cell=f)
    good = ops.voxel_carve(views, poses, 32, **kw)
    assert int(good.sum()) > 0
    bad = [
        lambda: ops.voxel_carve(views.float(), poses, 32, **kw),                         # dtype
        lambda: ops.voxel_carve(views[:, :, :100], poses, 32, **kw),                     # shape against the window
        lambda: ops.voxel_carve(views[0], poses, 32, **kw),                              # rank
        lambda: ops.voxel_carve(views, poses[:, :3], 32, **kw),                          # K of the poses
        lambda: ops.voxel_carve(views, poses[:1], 32, **kw),                             # B of the poses
        lambda: ops.voxel_carve(views, poses, 48, **kw),                                 # S
        lambda: ops.voxel_carve(views.cpu(), poses, 32, **kw),                           # host tensor
        lambda: ops.voxel_carve(views[:, :0], poses[:, :0], 32, **kw),                   # K = 0
        lambda: ops.voxel_carve(torch.zeros((1, 256, 8, 8), dtype=torch.int32, device="cuda"),
                                torch.zeros((1, 256, 3), device="cuda"), 32, window=(0, 0, 8, 8), **kw),          # K = 256
        lambda: ops.voxel_carve(torch.zeros((400, 200, 1, 1), dtype=torch.int32, device="cuda"),
                                torch.zeros((400, 200, 3), device="cuda"), 32, window=(0, 0, 1, 1), **kw),        # B K > 65535
        lambda: ops.voxel_carve(views, poses, 32, window=(1, 0, 128, 128), **kw),        # window outside the frame
        lambda: ops.voxel_carve(views, poses, 32, window=(0, -1, 128, 128), **kw),
        lambda: ops.voxel_carve(views, poses, 32, new_size=256, pixels_per_cell=16),     # f N > 2048
        lambda: ops.voxel_carve(views, poses, 32, slack=-1, **kw),
        lambda: ops.voxel_carve(views, poses, 32, slack=65536, **kw),
        lambda: ops.voxel_carve(views, poses, 32, slack=1.5, **kw),
        lambda: ops.voxel_carve(views, poses, 32, tolerance=-1, **kw),
        lambda: ops.voxel_carve(views, poses, 32, tolerance=K, **kw),
        lambda: ops.voxel_carve(views, poses, 32, outside="drop", **kw),
        lambda: ops.voxel_carve(views, poses, 32, outside=1, **kw),
        lambda: ops.voxel_carve(views, poses, 32, view_from_low_x=[True, False], **kw),  # wrong length
        lambda: ops.voxel_carve(views, poses, 32, view_from_low_x=[1, 0, 1, 0], **kw),   # not bools
        lambda: ops.voxel_carve(views, poses, 32, use_depth=1, **kw),
        lambda: ops.voxel_scan(torch.zeros((2, 32, 32, 32, 1), device="cuda"), poses[:1], N, f),
        lambda: ops.voxel_scan(torch.zeros((2, 48, 48, 48, 1), device="cuda"), poses, N, f),
        lambda: ops.hit_depth(views[:, 0], views[:, 0].to(torch.int8), poses[:, 0], 32, **kw, window=(0, 0, 64, 64)),
        lambda: ops.hit_depth(views[:, 0].float(), views[:, 0].to(torch.int8), poses[:, 0], 32, **kw),
        lambda: ops.hit_depth(views[:, 0], views[:, 0].to(torch.int8), poses[:1, 0], 32, **kw),
        lambda: ops.carve_pixels_per_voxel(poses),
    ]
    def no_launch():
        raise AssertionError("a refused call reached the library")
    with monkeypatch.context() as mp:
        mp.setattr(ops.L, "lib", no_launch)                       # every launch of the wrappers goes through L.lib()
        for i, call in enumerate(bad):
            with pytest.raises(E):
                call()
                pytest.fail("case %d was accepted" % i)
    # the C entries refuse on their own what the wrapper would have stopped
    from rendernet_amd import _lib as L
    lib, vp = L.lib(), ops._vp
    cam = torch.zeros((2, K, 3, 4), dtype=torch.int64, device="cuda")
    votes = torch.zeros((2, 32, 32, 32), dtype=torch.uint8, device="cuda")
    sp = L.stream_ptr()

    def carve(B=2, K=K, S=32, N=N, f=f, win=(0, 0, 128, 128), ud=1, slack=8, keep=1, v=views, c=cam, o=votes):
        return lib.rn_voxel_carve(vp(v), vp(c), vp(o), B, K, S, N, f, win[0], win[1], win[2], win[3], ud, slack, keep, sp)
    assert carve() == 0
    for kwargs in (dict(K=0), dict(K=256), dict(B=-1), dict(B=65536), dict(B=300, K=255), dict(S=96), dict(N=257), dict(f=17),
                   dict(N=256, f=16), dict(win=(0, 1, 128, 128)), dict(win=(0, 0, 0, 5)), dict(slack=-1), dict(slack=65536),
                   dict(v=None), dict(c=None), dict(o=None)):
        assert carve(**kwargs) == -1, kwargs                      # RN_E_INVALID
    assert carve(B=0, v=None, c=None, o=None) == 0
    hit = torch.zeros((2, 128, 128), dtype=torch.int32, device="cuda")
    face = torch.zeros((2, 128, 128), dtype=torch.int8, device="cuda")
    m = torch.zeros((2, 3, 4), device="cuda")
    d = torch.empty_like(hit)
    assert lib.rn_hit_depth(vp(hit), vp(face), vp(m), vp(d), 2, 32, N, f, 0, 0, 128, 128, 0, sp) == 0
    assert lib.rn_hit_depth(vp(hit), vp(face), vp(m), vp(d), 2, 33, N, f, 0, 0, 128, 128, 0, sp) == -1
    assert lib.rn_hit_depth(vp(hit), vp(face), vp(m), vp(d), 2, 32, N, f, 0, 0, 129, 128, 0, sp) == -1
    assert lib.rn_hit_depth(vp(hit), None, vp(m), vp(d), 2, 32, N, f, 0, 0, 128, 128, 0, sp) == -1
    torch.cuda.synchronize()
