"""rn_mask_pack / rn_pose_score / rn_pose_best on the device against the NumPy twin (tests/voxel_pose_ref.py): the score table,
n_mask, the winner and its integers word for word and the returned splats byte for byte, the twin fed the cameras the device
produced; windows, the three grid sides, pose shapes, matrices, edge inputs, recovery, the search level by level, determinism, the
limits and the argument checks.  -m gpu."""
import numpy as np
import pytest

import voxel_pose_ref as R
from rendernet_amd import synth

pytestmark = pytest.mark.gpu

LATTICE = (12, (0.4, 0.9, 1.4), (0.8, 1.25))
MASK_POSES = (5, 30, 64)                                          # the lattice poses the three masks are scanned at


def _dev(a, dtype=None):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


def chair32():
    return R.pool(R.load_binvox("chair"))


def grids32():
    """the pooled chair, 30 % noise inside an empty 2-voxel border, and an empty grid: bool [3,32,32,32]"""
    noise = np.zeros((32,) * 3, bool)
    noise[2:-2, 2:-2, 2:-2] = np.random.default_rng(5).random((28,) * 3) < 0.3
    return np.stack([chair32(), noise, np.zeros((32,) * 3, bool)])


_cache = {}


def scene(window=None):
    """(vox, lattice, masks) on the device, masks = voxel_scan(...) >= 0 of each grid at one lattice pose, once per window."""
    import torch
    from rendernet_amd import ops
    if window not in _cache:
        lat = synth.pose_lattice(*LATTICE)
        vox = _dev(grids32().astype(np.uint8)[..., None])
        views = ops.voxel_scan(vox, _dev(lat[list(MASK_POSES)][:, None]), new_size=64, pixels_per_cell=1, window=window)
        _cache[window] = (vox, _dev(lat), (views[:, 0] >= 0).to(torch.uint8))
    return _cache[window]


def against_twin(masks, vox, poses, S, N, f, window=None, fp=None, affine=False, threshold=0.5):
    """One device call with the splats, the twin per item on the device's cameras: everything compared, the PoseScores returned."""
    import torch
    from rendernet_amd import ops
    out = ops.voxel_pose_scores(masks, vox, poses, new_size=N, pixels_per_cell=f, window=window, footprint=fp, affine=affine,
                                threshold=threshold, return_splats=True)
    torch.cuda.synchronize()
    B, P = int(out.scores.shape[0]), int(out.scores.shape[1])
    win = (0, 0, f * N, f * N) if window is None else window
    assert out.scores.dtype is torch.int32 and out.n_mask.dtype is torch.int32 and out.best.dtype is torch.int64
    assert out.splats.dtype is torch.uint8 and tuple(out.splats.shape) == (B, P, win[2], win[3]) and tuple(out.cam.shape) == (B, P, 3, 4)
    occ = ops._grid_view(vox).cpu().numpy() > threshold
    cam, m = out.cam.cpu().numpy(), masks.cpu().numpy()
    table, n_mask, best, counts, images = (t.cpu().numpy() for t in (out.scores, out.n_mask, out.best, out.best_counts, out.splats))
    if fp is None:
        assert out.footprint == R.choose_footprint(R.pixels_per_voxel(cam))
    for b in range(B):
        want_images = R.splats(occ[b], cam[b], win, out.footprint)
        bad = images[b].astype(bool) != want_images
        assert not bad.any(), "item %d: %d splat pixels differ, first at %s" % (b, bad.sum(), np.argwhere(bad)[0])
        want, want_n = R.scores(occ[b], cam[b], m[b], win, out.footprint, want_images)
        assert np.array_equal(table[b], want), "item %d: candidates %s differ" % (b, np.argwhere((table[b] != want).any(1))[:4, 0])
        assert n_mask[b] == want_n
        w, w_counts = R.best(want, want_n)
        assert (int(best[b]), tuple(int(v) for v in counts[b])) == (w, w_counts)
    return out


@pytest.mark.parametrize("fp", [1, 2, 3, 4])
def test_score_table(fp):
    vox, lat, masks = scene()
    out = against_twin(masks, vox, lat, 32, 64, 1, fp=fp)
    assert int(out.n_mask[0]) > 100 and int(out.n_mask[2]) == 0 and int(out.scores[2].abs().sum()) == 0 and int(out.best[2]) == 0
    if fp == 2:
        assert int(out.best[0]) == MASK_POSES[0]
        auto = against_twin(masks, vox, lat, 32, 64, 1)
        assert auto.footprint == 2 and bool((auto.scores == out.scores).all())
        q = out.iou().cpu().numpy()
        assert q.dtype == np.float64 and q.shape == (3, 72) and q[2].max() == 0.0 and 0.7 < q[0].max() <= 1.0


@pytest.mark.parametrize("window", [(5, 9, 41, 37), (30, 33, 1, 1)])
def test_windows(window):
    vox, lat, masks = scene(window)
    assert tuple(masks.shape) == (3,) + window[2:]
    out = against_twin(masks, vox, lat, 32, 64, 1, window=window, fp=2)
    assert int(out.scores[0, :, 0].max()) > 0


def test_largest_window():
    """256 x 256 at S = 32, N = 128, f = 2: the whole image of LDS words, and a footprint at two pixels per voxel."""
    import torch
    from rendernet_amd import ops
    vox = _dev(grids32()[:2].astype(np.uint8)[..., None])
    poses = _dev(np.array([[0.7, 0.5, 1.0], [4.0, 1.1, 1.2]], np.float32))
    masks = (ops.voxel_scan(vox, poses[:1].expand(2, 1, 3).contiguous(), new_size=128, pixels_per_cell=2)[:, 0] >= 0).to(torch.uint8)
    out = against_twin(masks, vox, poses, 32, 128, 2)
    assert out.footprint == 4 and int(out.best[0]) == 0


@pytest.mark.parametrize("S", [64, 128])
def test_grid_sides(S):
    import torch
    from rendernet_amd import ops
    occ = R.load_binvox("chair")
    if S == 128:
        occ = np.repeat(np.repeat(np.repeat(occ, 2, 0), 2, 1), 2, 2)
    vox = _dev(occ.astype(np.uint8)[None, ..., None])
    poses = _dev(np.array([[0.3, 0.4, 0.5], [2.0, 0.9, 0.5], [3.3, 1.3, 0.45], [5.0, 0.1, 0.55]], np.float32))
    N = 256 if S == 128 else 128                                   # the largest frame at f = 1; the window is its middle
    window = (0, 0, 128, 128) if S == 64 else (40, 36, 176, 180)
    masks = (ops.voxel_scan(vox, poses[None, 2:3], new_size=N, pixels_per_cell=1, window=window)[:, 0] >= 0).to(torch.uint8)
    out = against_twin(masks, vox, poses, S, N, 1, window=window, fp=2)
    assert int(out.best[0]) == 2


def test_pose_shapes_and_matrices():
    import torch
    from rendernet_amd import ops
    vox, lat, masks = scene()
    shared = against_twin(masks, vox, lat[:24], 32, 64, 1, fp=2)
    per_item = against_twin(masks, vox, lat[:24][None].expand(3, 24, 3).contiguous(), 32, 64, 1, fp=2)
    assert bool((shared.scores == per_item.scores).all()) and bool((shared.best == per_item.best).all())
    rolled = torch.stack([lat[:24], lat[24:48], lat[48:72]])       # different candidates per item
    out = against_twin(masks, vox, rolled, 32, 64, 1, fp=2)
    assert not bool((out.scores == shared.scores).all())
    m = ops.pose_to_affine(lat[:6].contiguous(), 32, 64)
    m[3] = 0.0                                                     # no inverse: a zero camera, scored as the rule says
    m[4, :, :3] *= 0.5                                             # a camera no pose gives: twice the pixels per voxel
    out = against_twin(masks, vox, m, 32, 64, 1, fp=4, affine=True)
    assert int(out.cam[0, 3].abs().sum()) == 0 and out.scores[:, 3, 0].tolist() == [4, 4, 0]     # rows and columns -2..1 of pixel (0, 0)
    assert bool((out.scores[:, :3] == against_twin(masks, vox, lat[:3], 32, 64, 1, fp=4).scores).all())


def test_edge_inputs():
    import torch
    vox, lat, masks = scene()
    # every voxel of every candidate outside the window: the corner of the frame the models never reach
    out = against_twin(torch.ones((3, 4, 4), dtype=torch.uint8, device="cuda"), vox, lat, 32, 64, 1, window=(0, 0, 4, 4), fp=2)
    assert int(out.scores.abs().sum()) == 0 and out.best.tolist() == [0, 0, 0] and out.n_mask.tolist() == [16] * 3
    # a mask of all ones, as bool: n_inter = n_splat, the largest splat wins
    out = against_twin(torch.ones((3, 64, 64), dtype=torch.bool, device="cuda"), vox, lat, 32, 64, 1, fp=2)
    assert bool((out.n_splat == out.n_inter).all()) and out.n_mask.tolist() == [4096] * 3
    assert int(out.best[0]) == int(np.argmax(out.n_splat[0].cpu().numpy()))     # NumPy's argmax: the first of the largest
    # nonzero bytes other than 1 are foreground
    odd = (masks * 37).contiguous()
    assert bool((against_twin(odd, vox, lat[:12], 32, 64, 1, fp=2).scores == against_twin(masks, vox, lat[:12], 32, 64, 1, fp=2).scores).all())


def test_tie_order_of_the_winner():
    import torch
    from rendernet_amd import ops
    rng = np.random.default_rng(9)
    tables = [np.array([[9, 1], [4, 2], [1, 1]]), np.array([[9, 1], [1, 1], [4, 2]]), np.array([[5, 0], [7, 0], [0, 0]]),
              np.array([[0, 0], [3, 0], [2, 0]])]
    n_masks = [2, 2, 3, 0]
    for P in (3, 300, 1000):                                       # below, above and well above one candidate per thread
        big = np.zeros((4, P, 2), np.int32)
        for b, t in enumerate(tables):
            big[b, P - 3:] = t                                     # zeros before: 0 / n, which only an equal 0 ties with
        inter = rng.integers(0, 30, size=(2, P))
        extra = np.stack([inter + rng.integers(0, 30, size=(2, P)), inter], -1).astype(np.int32)
        extra[1] = extra[1, 0]                                     # every candidate equal: index 0
        table, nm = np.concatenate([big, extra]), np.array(n_masks + [17, 17], np.int32)
        best, counts = ops.pose_best(_dev(table), _dev(nm))
        assert best.dtype is torch.int64
        for b in range(len(table)):
            w, w_counts = R.best(table[b], nm[b])
            assert (int(best[b]), tuple(counts[b].tolist())) == (w, w_counts), (P, b)
        assert int(best[5]) == 0 and int(best[0]) == P - 2 and int(best[1]) == P - 2


def test_recovery_on_the_device():
    from rendernet_amd import ops
    import torch
    vox, lat, _ = scene()
    truth = list(range(0, 72, 6))
    views = ops.voxel_scan(vox[:1].expand(12, -1, -1, -1, -1).contiguous(), lat[truth][:, None].contiguous(), new_size=64, pixels_per_cell=1)
    out = ops.voxel_pose_scores((views[:, 0] >= 0).to(torch.uint8), vox[:1].expand(12, -1, -1, -1, -1).contiguous(), lat, new_size=64,
                                footprint=2)
    assert out.best.tolist() == truth


def test_search_level_by_level():
    import torch
    from rendernet_amd import ops
    occ = chair32()
    vox = _dev(np.stack([occ, occ]).astype(np.uint8)[..., None])
    true = _dev(np.array([[[1.13, 0.62, 1.07]], [[4.4, 1.21, 0.86]]], np.float32))
    masks = (ops.voxel_scan(vox, true, new_size=64, pixels_per_cell=1)[:, 0] >= 0).to(torch.uint8)
    lat = (12, (0.4, 0.9, 1.4), (0.8, 1.0, 1.25))
    found = ops.voxel_pose_search(masks, vox, *lat, refine=2, new_size=64, pixels_per_cell=1)
    assert found.footprint == 2 and len(found.levels) == 3 and tuple(found.pose.shape) == (2, 3) and found.pose.dtype is torch.float32
    steps = R.lattice_steps(*lat)
    m = masks.cpu().numpy()
    for b in range(2):
        for level, got in enumerate(found.levels):
            lattice = got["lattice"] if level == 0 else got["lattice"][b]
            if level == 0:
                assert np.array_equal(lattice, R.pose_lattice(*lat))
            else:
                assert np.array_equal(lattice, R.refine_lattice(found.levels[level - 1]["pose"][b], steps, level, lat[1], lat[2]))
            # the twin on the device's cameras of this level's lattice
            cam = ops.mesh_camera(_dev(lattice), 32, 64, 1).cpu().numpy()
            table, n_mask = R.scores(occ, cam, m[b], (0, 0, 64, 64), 2)
            w, counts = R.best(table, n_mask)
            assert int(got["best"][b]) == w and np.array_equal(got["pose"][b], lattice[w])
        assert np.array_equal(found.pose[b].cpu().numpy(), found.levels[-1]["pose"][b])
        assert (int(found.n_splat[b]), int(found.n_inter[b]), int(found.n_mask[b])) == counts
        assert abs(float(found.iou[b]) - R.iou(*counts)) < 1e-15


def test_two_calls_bit_for_bit():
    from rendernet_amd import ops
    vox, lat, masks = scene()
    a = ops.voxel_pose_scores(masks, vox, lat, new_size=64, footprint=3, return_splats=True)
    b = ops.voxel_pose_scores(masks, vox, lat, new_size=64, footprint=3, return_splats=True)
    for x, y in ((a.scores, b.scores), (a.splats, b.splats), (a.best, b.best), (a.best_counts, b.best_counts), (a.n_mask, b.n_mask)):
        assert bool((x == y).all())
    s = ops.voxel_silhouette(vox, lat, new_size=64, footprint=3)
    assert bool((s == a.splats).all())


def test_both_forms_of_the_walk():
    """With the workspace the kernel visits the list of occupied words, without it it walks them all: the same bits, at every side."""
    import torch
    from rendernet_amd import ops
    lib = ops.L.lib()
    rng = np.random.default_rng(12)
    for S, N, B in ((32, 64, 3), (64, 128, 2), (128, 256, 1)):
        occ = rng.random((B, S, S, S)) < np.array([0.3, 0.002, 0.0])[:B, None, None, None]      # dense, nearly empty, empty
        vox = _dev(occ.astype(np.uint8)[..., None])
        poses = _dev(synth.pose_lattice(5, (0.3, 1.2), (0.7,)))
        P, side = 10, min(N - 3, 200)                               # the window starts at (3, 1)
        masks = torch.ones((B, side, side), dtype=torch.uint8, device="cuda")
        listed = ops.voxel_pose_scores(masks, vox, poses, new_size=N, window=(3, 1, side, side), footprint=2, return_splats=True)
        bits = ops.voxel_pack(vox)[0]
        mask_bits, _ = ops._pose_masks("test", masks, B, side, side, vox.device)
        walked = torch.full((B, P, 2), -1, dtype=torch.int32, device="cuda")
        images = torch.full((B, P, side, side), 7, dtype=torch.uint8, device="cuda")
        ops.L.check(lib.rn_pose_score(ops._vp(bits), ops._vp(mask_bits), ops._vp(listed.cam), ops._vp(walked), ops._vp(images), B, P, S, N, 1,
                                      3, 1, side, side, 2, None, 0, ops.L.stream_ptr()), "rn_pose_score")
        assert bool((walked == listed.scores).all()) and bool((images == listed.splats).all())
        assert int(listed.scores[0, :, 0].min()) > 0 and (B < 3 or int(listed.scores[2].abs().sum()) == 0)


def test_limits():
    import torch
    from rendernet_amd import ops
    vox, lat, masks = scene()
    out = ops.voxel_pose_scores(masks[:0], vox[:0], lat, new_size=64, footprint=2, return_splats=True)
    assert tuple(out.scores.shape) == (0, 72, 2) and tuple(out.best.shape) == (0,) and tuple(out.splats.shape) == (0, 72, 64, 64)
    assert tuple(ops.voxel_pose_search(masks[:0], vox[:0], new_size=64).pose.shape) == (0, 3)
    one = against_twin(masks, vox, lat[7:8], 32, 64, 1, fp=2)
    assert one.best.tolist() == [0, 0, 0]


def test_argument_checks(monkeypatch):
    import torch
    from rendernet_amd import ops
    from rendernet_amd._lib import RenderNetHipError as E
    vox, lat, masks = scene()
    kw = dict(new_size=64, pixels_per_cell=1)
    bad = [
        lambda: ops.voxel_pose_scores(masks.float(), vox, lat, **kw),                          # a wrong dtype
        lambda: ops.voxel_pose_scores(masks, vox, lat.long(), **kw),
        lambda: ops.voxel_pose_scores(masks.int(), vox, lat, **kw),
        lambda: ops.voxel_pose_scores(masks[:, :63], vox, lat, **kw),                          # a wrong shape
        lambda: ops.voxel_pose_scores(masks, vox, lat[:, :2], **kw),
        lambda: ops.voxel_pose_scores(masks, vox, lat[None].expand(2, 72, 3), **kw),
        lambda: ops.voxel_pose_scores(masks, vox[:, :16], lat, **kw),
        lambda: ops.voxel_pose_scores(masks, vox, lat, affine=True, **kw),
        lambda: ops.voxel_pose_scores(masks.cpu(), vox, lat, **kw),                            # a wrong device
        lambda: ops.voxel_pose_scores(masks, vox, lat.cpu(), **kw),
        lambda: ops.voxel_pose_scores(masks, vox.cpu(), lat, **kw),
        lambda: ops.voxel_pose_scores(masks, vox, lat, new_size=128, pixels_per_cell=4),       # ph > 256
        lambda: ops.voxel_pose_scores(masks, vox, lat, new_size=128, pixels_per_cell=4, window=(0, 0, 257, 64)),
        lambda: ops.voxel_pose_scores(masks, vox, lat, footprint=0, **kw),
        lambda: ops.voxel_pose_scores(masks, vox, lat, footprint=5, **kw),
        lambda: ops.voxel_pose_scores(masks, vox, lat, footprint=2.0, **kw),
        lambda: ops.voxel_pose_scores(masks, vox, lat[:0], **kw),                              # P = 0
        lambda: ops.voxel_pose_scores(masks, vox, lat, window=(10, 10, 64, 64), **kw),         # a window outside the frame
        lambda: ops.voxel_pose_scores(masks, vox, lat, window=(-1, 0, 64, 64), **kw),
        lambda: ops.voxel_pose_scores(masks, vox, lat, threshold=float("nan"), **kw),
        lambda: ops.voxel_silhouette(vox, lat, footprint=5, **kw),
        lambda: ops.voxel_pose_search(masks, vox, refine=-1, **kw),
        lambda: ops.voxel_pose_search(masks.float(), vox, **kw),
        lambda: ops.pose_best(torch.zeros((1, 0, 2), dtype=torch.int32, device="cuda"), torch.zeros((1,), dtype=torch.int32, device="cuda")),
    ]

    def no_launch():
        raise AssertionError("a refused call reached the library")
    with monkeypatch.context() as mp:
        mp.setattr(ops.L, "lib", no_launch)                       # every launch of the wrappers goes through L.lib()
        for i, call in enumerate(bad):
            with pytest.raises(E):
                call()
    # the footprint that no camera of the call allows is refused too, once the cameras are known: 2 pixels per cell at scale 1.5
    with pytest.raises(E, match="coarser frame"):
        ops.voxel_pose_scores(torch.zeros((3, 128, 128), dtype=torch.uint8, device="cuda"), vox, _dev(np.array([[0.0, 0.5, 1.5]], np.float32)),
                              new_size=64, pixels_per_cell=2)
    # and the library's own checks, behind the wrappers'
    lib = ops.L.lib()
    z = torch.zeros((64,), dtype=torch.int64, device="cuda")
    p = ops._vp(z)
    for args in ((p, p, p, p, None, 1, 1, 48, 64, 1, 0, 0, 64, 64, 2, None, 0, None), (p, p, p, p, None, 1, 0, 32, 64, 1, 0, 0, 64, 64, 2, None, 0, None),
                 (p, p, p, p, None, 1, 65536, 32, 64, 1, 0, 0, 64, 64, 2, None, 0, None), (p, p, p, p, None, 1, 1, 32, 64, 1, 0, 0, 64, 64, 0, None, 0, None),
                 (p, p, p, p, None, 1, 1, 32, 64, 1, 0, 0, 64, 64, 5, None, 0, None), (p, p, p, p, None, 1, 1, 32, 128, 4, 0, 0, 257, 8, 2, None, 0, None),
                 (p, p, p, p, None, 1, 1, 32, 64, 1, 1, 0, 64, 64, 2, None, 0, None), (p, p, p, p, None, -1, 1, 32, 64, 1, 0, 0, 64, 64, 2, None, 0, None),
                 (p, p, None, p, None, 1, 1, 32, 64, 1, 0, 0, 64, 64, 2, None, 0, None), (p, p, ops._vp(z[:8].view(torch.int32)[1:]), p, None, 1, 1, 32, 64, 1, 0, 0, 64, 64, 2, None, 0, None)):
        assert lib.rn_pose_score(*args) == -1 and b"rn_pose_score" in lib.rn_last_error()
    need = lib.rn_pose_score_workspace_bytes(1, 32)
    assert need == (1024 + 1) * 4 + 12 and lib.rn_pose_score_workspace_bytes(1, 48) == 0 and lib.rn_pose_score_workspace_bytes(-1, 32) == 0
    for ws, nws in ((p, need - 16), (ops._vp(z[:8].view(torch.int32)[1:]), need)):      # a workspace too small, or not aligned
        assert lib.rn_pose_score(p, p, p, p, None, 1, 1, 32, 64, 1, 0, 0, 64, 64, 2, ws, nws, None) == -1
    assert lib.rn_mask_pack(p, p, p, 1, 257, 4, None) == -1 and lib.rn_mask_pack(p, p, p, 1, 4, 0, None) == -1
    assert lib.rn_pose_best(p, p, p, p, 1, 0, None) == -1 and lib.rn_pose_best(p, None, p, p, 1, 1, None) == -1
    assert lib.rn_pose_score(None, None, None, None, None, 0, 1, 32, 64, 1, 0, 0, 64, 64, 2, None, 0, None) == 0     # B == 0 is a no-op
