"""The rule of rn_pose_score / rn_pose_best on the NumPy twin (tests/voxel_pose_ref.py): closed forms, the tie order, the
hole-freedom of the automatic footprint, exact recovery of 72 poses of three models, self-consistency, the footprint choice at
its boundaries, the lattice's order; the header, the binding, synth.pose_lattice and ops.pose_footprint against the twin; the
host side of tools/pose_voxels.  No device."""
import functools
import math
import os
import re
from fractions import Fraction

import numpy as np
import pytest

import voxel_carve_ref as VC
import voxel_pose_ref as R

LATTICE = (12, (0.4, 0.9, 1.4), (0.8, 1.25))
N, F = 64, 1
FULL = (0, 0, 64, 64)
ONE = 1 << 20


def flat_camera(offset=16):
    """X = 256 (x + offset) + 128 and Y = 256 (y + offset) + 128 for voxel (z, y, x): one pixel per voxel along the z axis."""
    return np.array([[0, 0, ONE, 256 * offset * ONE], [0, ONE, 0, 256 * offset * ONE], [ONE, 0, 0, 0]], np.int64)


@functools.lru_cache(maxsize=None)
def model(name, S=32):
    g = R.load_binvox(name)
    g = R.pool(g, g.shape[0] // S) if g.shape[0] != S else g
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def lattice_set(name):
    """Once per model and left unchanged: (cams [72,3,4], the caster twin's masks [72,64,64], the splats at fp = 2 [72,64,64])."""
    lat = R.pose_lattice(*LATTICE)
    views, cams = VC.scan(model(name), lat, [False] * len(lat), N, F)
    out = (cams, views >= 0, R.splats(model(name), cams, FULL, 2))
    for a in out:
        a.setflags(write=False)
    return out


def tables(images, masks):
    """int64 [M,P,2] and n_mask [M]: every mask against every splat, by one matrix product."""
    A, M = images.reshape(len(images), -1).astype(np.int64), masks.reshape(len(masks), -1).astype(np.int64)
    inter = M @ A.T
    return np.stack([np.broadcast_to(A.sum(1), inter.shape), inter], -1), M.sum(1)


@pytest.mark.parametrize("fp", [1, 2, 3, 4])
def test_lone_voxel(fp):
    occ = np.zeros((32,) * 3, bool)
    occ[5, 6, 7] = True
    img = R.splat(occ, flat_camera(), FULL, fp)
    assert img.sum() == fp * fp
    lo_r, lo_c = (256 * 22 + 128 - 128 * (fp - 1)) // 256, (256 * 23 + 128 - 128 * (fp - 1)) // 256
    assert (lo_r, lo_c) == {1: (22, 23), 2: (22, 23), 3: (21, 22), 4: (21, 22)}[fp]
    assert img[lo_r:lo_r + fp, lo_c:lo_c + fp].all()
    # on the window's edge the footprint is clipped pixel by pixel: the window's corner sits on the footprint's second pixel
    win = (lo_r + 1, lo_c + 1, 7, 5)
    clipped = R.splat(occ, flat_camera(), win, fp)
    assert clipped.shape == (7, 5) and clipped.sum() == (fp - 1) ** 2 and clipped[:fp - 1, :fp - 1].all()
    table, n_mask = R.scores(occ, flat_camera()[None], np.ones((7, 5), np.uint8), win, fp)
    assert table.tolist() == [[(fp - 1) ** 2, (fp - 1) ** 2]] and n_mask == 35
    far = R.splat(occ, flat_camera(), (40, 40, 8, 8), fp)          # all of it outside: what the rule gives is nothing
    assert far.sum() == 0


def test_full_cube_and_empty_grid():
    cube = np.ones((32,) * 3, bool)
    img = R.splat(cube, flat_camera(), FULL, 1)
    assert img.sum() == 32 * 32 and img[16:48, 16:48].all()
    assert R.splat(cube, flat_camera(), FULL, 2).sum() == 33 * 33
    empty = np.zeros((32,) * 3, bool)
    table, n_mask = R.scores(empty, np.stack([flat_camera()] * 3), np.zeros((64, 64), np.uint8), FULL, 2)
    assert table.tolist() == [[0, 0]] * 3 and n_mask == 0
    assert R.best(table, n_mask) == (0, (0, 0, 0)) and R.iou(0, 0, 0) == 0.0
    zero = R.splat(cube, np.zeros((3, 4), np.int64), FULL, 2)       # a zero camera: every centre at (0, 0), footprint rows -1..0
    assert zero.sum() == 1 and zero[0, 0]


def test_tie_order():
    # equal quotients from different integers, 1/2 and 2/4 with n_mask = 2: the lower index, whichever it holds
    assert R.best([[9, 1], [4, 2], [1, 1]], 2)[0] == 1 and R.best([[9, 1], [1, 1], [4, 2]], 2)[0] == 1
    assert R.best([[1, 1], [4, 2], [2, 2]], 2) == (2, (2, 2, 2))     # 2/2 beats both
    assert R.best([[5, 0], [7, 0]], 3)[0] == 0                        # 0/8 and 0/10 are equal: both are zero
    assert R.best([[0, 0], [3, 0]], 0)[0] == 0                        # the empty union counts as 0/1
    # a ball scores the same under every quarter turn against a mask of all ones
    ball = R.ball(32, 11.5)
    lat = R.pose_lattice(4, (0.0,), (1.0,))
    cams, _ = VC.cameras(lat, [False] * 4, 32, N, F)
    table, n_mask = R.scores(ball, cams, np.ones((64, 64), np.uint8), FULL, 2)
    assert len({tuple(r) for r in table.tolist()}) == 1 and n_mask == 4096
    assert R.best(table, n_mask)[0] == 0 and R.best(table[::-1], n_mask)[0] == 0
    # and against its own splat at turn 0, which turn 3 repeats bit for bit: 1/1 twice, the lower index
    images = R.splats(ball, cams, FULL, 2)
    assert np.array_equal(images[0], images[3])
    table, n_mask = R.scores(ball, cams, images[3], FULL, 2, images)
    assert R.best(table, n_mask)[0] == 0 and R.best(table[1:], n_mask)[0] == 2


def test_the_order_is_the_exact_quotient():
    rng = np.random.default_rng(3)
    for _ in range(50):
        n_mask = int(rng.integers(0, 40))
        inter = rng.integers(0, n_mask + 1, size=12)
        table = np.stack([inter + rng.integers(0, 40, size=12), inter], 1)
        q = [Fraction(int(b), R.union(a, b, n_mask)) if R.union(a, b, n_mask) else Fraction(0) for a, b in table]
        assert R.best(table, n_mask)[0] == q.index(max(q))


@pytest.mark.parametrize("name", ["ball", "chair"])
def test_no_holes_under_the_automatic_footprint(name):
    if name == "ball":
        occ = R.ball(32, 11.5)
        cams, _ = VC.cameras(R.pose_lattice(*LATTICE), [False] * 72, 32, N, F)
    else:
        occ, cams = model("chair"), lattice_set("chair")[0]
    ppv = R.pixels_per_voxel(cams)
    fp = R.choose_footprint(ppv)
    assert abs(ppv - 1.25) < 1e-5 and fp == 2
    images = R.splats(occ, cams, FULL, fp) if name == "ball" else lattice_set("chair")[2]
    assert sum(int(R.holes(s).sum()) for s in images) == 0
    if name == "chair":                                            # the centre splat of its thin parts at 1.25 does have them
        assert sum(int(R.holes(s).sum()) for s in R.splats(occ, cams[36:], FULL, 1)) > 0


def filled(img):
    """A splat that is its whole bounding box."""
    r, c = np.nonzero(img.any(1))[0], np.nonzero(img.any(0))[0]
    return int(img.sum()) == (r[-1] - r[0] + 1) * (c[-1] - c[0] + 1)


@pytest.mark.parametrize("fp,scale", [(1, 0.70), (2, 1.41), (3, 2.12)])
def test_hole_argument_on_sheets(fp, scale):
    """The header's argument, checked just below its bound fp / sqrt 2: a sheet one voxel thick, flat or a staircase, has no hole
    from any of 72 directions, and seen face-on it is a filled rectangle; one footprint less leaves the face-on sheet open."""
    flat = np.zeros((32,) * 3, bool)
    flat[6:26, 6:26, 16] = True
    stairs = np.zeros((32,) * 3, bool)
    for i in range(6, 26):
        for j in range(6, 26):
            stairs[(i + j) // 2, i, j] = True
    lat = R.pose_lattice(24, (0.0, 0.6, 1.3), (scale,))
    cams, _ = VC.cameras(lat, [False] * len(lat), 32, N, F)
    assert R.choose_footprint(R.pixels_per_voxel(cams)) == fp
    for occ in (flat, stairs):
        assert sum(int(R.holes(s).sum()) for s in R.splats(occ, cams, FULL, fp)) == 0
    face_on = cams[[6, 18]]                                        # a quarter and three quarters of a turn, on the horizon
    assert all(filled(s) and s.sum() >= (20 * scale) ** 2 for s in R.splats(flat, face_on, FULL, fp))
    if fp > 1:
        assert not any(filled(s) for s in R.splats(flat, face_on, FULL, fp - 1))


@pytest.mark.parametrize("name", ["chair", "bunny", "suzanne"])
def test_recovery_of_every_lattice_pose(name):
    cams, masks, images = lattice_set(name)
    table, n_mask = tables(images, masks)
    for m in range(72):
        w, counts = R.best(table[m], n_mask[m])
        assert w == m, (name, m, w)
        assert counts == (int(images[m].sum()), int((images[m] & masks[m]).sum()), int(masks[m].sum()))


@pytest.mark.parametrize("name,S", [("chair", 32), ("bunny", 64)])
def test_self_consistency(name, S):
    occ = model(name, S)
    if S == 32:
        cams, _, images = lattice_set(name)
    else:
        lat = R.pose_lattice(6, (0.4, 1.4), (0.8,))
        cams, _ = VC.cameras(lat, [False] * len(lat), S, 2 * S, F)
        images = R.splats(occ, cams, (0, 0, 2 * S, 2 * S), 2)
    table, n_mask = tables(images, images)
    for m in range(len(images)):
        w, (n_splat, n_inter, nm) = R.best(table[m], n_mask[m])
        assert w == m and n_splat == n_inter == nm
        full = [p for p in range(len(images)) if R.union(*table[m][p], n_mask[m]) == table[m][p][1]]
        assert full == [m]                                         # IoU exactly 1, and the only one


def test_footprint_choice():
    r2 = math.sqrt(2.0)
    for fp in (1, 2, 3, 4):
        assert R.choose_footprint(math.nextafter(fp / r2, 0.0)) == fp
        assert R.choose_footprint(fp / r2) == (fp + 1 if fp < 4 else None)
    assert R.choose_footprint(0.0) == 1 and R.choose_footprint(3.0) is None
    from rendernet_amd import _lib, ops
    for ppv in (0.0, 0.5, 0.7071, 0.70711, 1.0, 1.25, 1.4142, 1.41422, 2.0, 2.1213, 2.12133, 2.8284):
        assert ops.pose_footprint(ppv) == R.choose_footprint(ppv)
    for ppv in (4.0 / r2, 3.0, float("nan"), True, "1"):
        with pytest.raises(_lib.RenderNetHipError, match="pose_footprint"):
            ops.pose_footprint(ppv)
    with pytest.raises(_lib.RenderNetHipError, match="coarser frame"):
        ops.pose_footprint(2.9)
    # the figure is the LARGER row norm
    cam = np.zeros((2, 3, 4), np.int64)
    cam[0, 0, :3], cam[0, 1, :3] = (3 * ONE, 4 * ONE, 0), (ONE, 0, 0)
    assert R.pixels_per_voxel(cam) == 5.0


def test_lattice_order_and_values():
    from rendernet_amd import synth
    lat = synth.pose_lattice(*LATTICE)
    assert lat.dtype == np.float32 and lat.shape == (72, 3) and np.array_equal(lat, R.pose_lattice(*LATTICE))
    assert np.array_equal(lat[:12, 0], (2.0 * np.pi * np.arange(12) / 12).astype(np.float32))
    assert (lat[:12, 1] == np.float32(0.4)).all() and (lat[12:24, 1] == np.float32(0.9)).all()
    assert (lat[:36, 2] == np.float32(0.8)).all() and (lat[36:, 2] == np.float32(1.25)).all()
    assert tuple(lat[36 + 12 + 5]) == (np.float32(2.0 * np.pi * 5 / 12), np.float32(0.9), np.float32(1.25))
    steps = synth.pose_lattice_steps(*LATTICE)
    assert steps == R.lattice_steps(*LATTICE) and abs(steps[1] - 0.5) < 1e-12 and abs(steps[2] - 0.45) < 1e-12
    for centre, level in (((0.1, 0.4, 0.8), 1), ((5.9, 1.39, 1.25), 2), ((3.0, 0.9, 1.0), 3)):
        near = synth.pose_refine_lattice(centre, steps, level, LATTICE[1], LATTICE[2])
        assert near.shape == (75, 3) and np.array_equal(near, R.refine_lattice(centre, steps, level, LATTICE[1], LATTICE[2]))
        assert np.allclose(near[37], centre, atol=1e-6)            # the centre is candidate 37
        assert (near[:, 0] >= 0).all() and (near[:, 0] < 2 * np.pi + 1e-6).all()
        assert near[:, 1].min() >= np.float32(0.4) and near[:, 1].max() <= np.float32(1.4)
        assert near[:, 2].min() >= np.float32(0.8) and near[:, 2].max() <= np.float32(1.25)
        assert abs(float(near[38, 0] - near[37, 0]) - steps[0] / 2 ** level) < 1e-5
    for bad in ((0, (0.1,), (1.0,)), (4, (), (1.0,)), (4, (0.1,), (float("inf"),))):
        with pytest.raises(ValueError, match="pose_lattice"):
            synth.pose_lattice(*bad)


def test_search_on_the_twin_lands_near_an_off_lattice_pose():
    """One case of the measurement DESIGN.md 5c tabulates: within one level-0 step on every axis without refinement."""
    occ = model("chair")
    true = np.array([[1.13, 0.62, 1.07]], np.float32)
    views, _ = VC.scan(occ, true, [False], N, F)
    lat = (24, (0.1, 0.4, 0.7, 1.0, 1.3), (0.8, 1.0, 1.25))
    levels = R.search(occ, views[0] >= 0, *lat, refine=1, N=N, f=F, window=FULL, fp=2)
    steps = R.lattice_steps(*lat)
    assert len(levels) == 2 and len(levels[0][0]) == 360 and len(levels[1][0]) == 75
    for _, _, pose in levels:
        d_az = abs((float(pose[0]) - 1.13 + np.pi) % (2 * np.pi) - np.pi)
        assert d_az <= steps[0] and abs(float(pose[1]) - 0.62) <= steps[1] and abs(float(pose[2]) - 1.07) <= steps[2] + 1e-6


def test_header_and_binding():
    hdr = open(os.path.join(R.ROOT, "include", "rendernet_hip.h")).read()
    assert "Silhouette pose search" in hdr and "EQUAL SCORES GO TO THE LOWER INDEX" in hdr
    assert "PIXELS PER VOXEL < fp / sqrt 2" in hdr and "ONLY ROWS 0 AND 1 ARE USED" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    from rendernet_amd import _lib, build, ops
    n_args = {"rn_mask_pack": 7, "rn_pose_score_workspace_bytes": 2, "rn_pose_score": 18, "rn_pose_best": 7}
    for name, n in n_args.items():
        m = re.search(r"\b(int|size_t)\s+%s\s*\(([^)]*)\)" % name, code)
        assert m and len(m.group(2).split(",")) == n and name in _lib.SIGNATURES
        restype = _lib._c_int if m.group(1) == "int" else __import__("ctypes").c_size_t
        assert len(_lib.SIGNATURES[name][1]) == n and _lib.SIGNATURES[name][0] is restype
    assert "MAY BE NULL" in hdr
    assert "voxel_pose.hip" in build.SOURCES
    for name, value in (("RN_POSE_MAX_SIDE", 256), ("RN_POSE_MAX_FOOTPRINT", 4), ("RN_POSE_MAX_CANDIDATES", 65535)):
        assert re.search(r"#define\s+%s\s+%d\b" % (name, value), code) and getattr(_lib, name) == value
    assert ops.POSE_MAX_SIDE == 256 and ops.POSE_MAX_FOOTPRINT == 4 == R.MAX_FOOTPRINT


def test_argument_errors_without_a_device():
    import torch
    from rendernet_amd import _lib, ops
    err = _lib.RenderNetHipError
    g = torch.zeros((1, 32, 32, 32), dtype=torch.uint8)
    m = torch.zeros((1, 64, 64), dtype=torch.uint8)
    p = torch.zeros((4, 3))
    with pytest.raises(err, match="HIP tensors"):
        ops.voxel_pose_scores(m, g, p, new_size=64)
    with pytest.raises(err, match="voxel_pose_scores"):
        ops.voxel_pose_scores(m, g.numpy(), p, new_size=64)
    with pytest.raises(err, match="voxel_silhouette"):
        ops.voxel_silhouette(None, p, new_size=64)
    with pytest.raises(err, match="pose_best"):
        ops.pose_best(torch.zeros((1, 4, 2)), torch.zeros((1,), dtype=torch.int32))
    for kw in ({"refine": -1}, {"refine": 1.0}, {"n_azimuth": 0}, {"scales": ()}):
        with pytest.raises(err, match="voxel_pose_search"):
            ops.voxel_pose_search(m, g, new_size=64, **kw)


def test_tool_arguments_and_names(tmp_path, capsys):
    from rendernet_amd.tools import data_util, pose_voxels as PV
    args = PV.parse_args(["chair.binvox", "a.png", "b.png", "--refine", "1", "--copy-to", "out"])
    assert (args.model, args.images, args.size, args.background, args.threshold, args.azimuths, args.refine, args.copy_to) == \
        ("chair.binvox", ["a.png", "b.png"], 64, "black", 8.0, 24, 1, "out")
    for bad in (["chair.txt", "a.png"], ["chair.binvox"], ["chair.binvox", "a.png", "--size", "48"],
                ["chair.binvox", "a.png", "--refine", "9"], ["chair.binvox", "a.png", "--azimuths", "0"],
                ["chair.binvox", "a.png", "--background", "grey"]):
        with pytest.raises(SystemExit):
            PV.parse_args(bad)
    assert "pose_voxels" in capsys.readouterr().err
    # the name written by --copy-to is the name the reference's reader reads: the pose it stands for is the pose to the name's digits
    for pose in ((0.0, 0.4, 1.0), (2.0 * math.pi * 23 / 24, 1.3, 0.8), (1.2345, -0.2, 1.25), (6.2831, 0.1, 0.5)):
        name = PV.pose_name("/data/my_model.binvox", pose, ".png")
        assert name.startswith("my-model_p") and name.endswith(".png")
        back = data_util.extract_param_from_names(name)[0]
        assert np.array_equal(PV.name_pose(name), back.astype(np.float32))
        d_az = abs((back[0] - pose[0] + math.pi) % (2 * math.pi) - math.pi)
        assert d_az < math.radians(0.006) and abs(back[1] - pose[1]) < math.radians(0.006)
        radius = float("%.1f" % (3.3 / pose[2]))
        assert abs(back[2] - 3.3 / radius) < 1e-12 and abs(3.3 / back[2] - 3.3 / pose[2]) <= 0.05 + 1e-9
    assert PV.pose_name("m.obj", (0.0, 0.0, 0.1), ".jpg") == "m_p0.00_t90.00_r9.9.jpg"       # the radius keeps its three characters
    # a finer picture is OR-pooled by two until it fits
    big = np.zeros((512, 512), bool)
    big[101, 333] = True
    small, f = PV.fit_mask(big, 64, 1.25)
    assert f == 2 and small.shape == (256, 256) and small.sum() == 1 and small[50, 166]
    assert PV.fit_mask(big, 64, 1.65)[1] == 1                      # 2 * 1.65 is past the largest footprint's bound
    assert PV.fit_mask(np.zeros((128, 128), bool), 64, 1.25)[1] == 1
    with pytest.raises(ValueError):
        PV.fit_mask(np.zeros((100, 100), bool), 64, 1.25)
