"""Host-side checks of the carving rule's NumPy twin (tests/voxel_carve_ref.py; include/rendernet_hip.h, rn_voxel_carve and
rn_hit_depth, states the rule): closed forms at an axis-aligned pose, the property that the hull of a scan loses no voxel of the
grid at 1.5 pixels per voxel or more (and the counter-case below it), and the entry depth against the rasteriser's depth of the
blocky mesh.  No GPU."""
import os
import re

import numpy as np
import pytest

import mesh_extract_ref as XR
import mesh_raster_ref as MR
import raycast_ref as RR
import voxel_carve_ref as VC
from conftest import BINVOX_DIR
from header_version import states_version
from rendernet_amd import synth
from test_mesh_raster_cpu import axis_pose, m_inv_of

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

# The axis pose at S = 32, N = 64, f = 4 (M_inv is the translation by -16): in 1/256 pixel X = 1024 z + 16896, Y = 48640 - 1024 y,
# D = 12160 - 256 x, so the centre of voxel (z, y, x) falls into column 4 z + 66 and row 190 - 4 y EXACTLY on the pixel's left
# and top border, which the floor gives to that pixel.
S32, N64, F4 = 32, 64, 4
FRAME = (0, 0, 256, 256)


def axis_cam(low=False):
    cam, _ = VC.cameras([axis_pose()], [low], S32, N64, F4)
    return cam[0]


def col_of(z):
    return 4 * z + 66


def row_of(y):
    return 190 - 4 * y


def test_axis_camera_is_the_closed_form():
    X, Y, D = VC.project_centres(axis_cam(), S32)
    z, y, x = np.meshgrid(*[np.arange(S32)] * 3, indexing="ij")
    assert np.array_equal(X, 1024 * z + 16896) and np.array_equal(Y, 48640 - 1024 * y) and np.array_equal(D, 12160 - 256 * x)
    _, _, Dl = VC.project_centres(axis_cam(True), S32)
    assert np.array_equal(Dl, 256 * x + 4224)
    assert VC.pixels_per_voxel(axis_cam()) == 4.0


def box_view(r_a, r_b, c_a, c_b, value=0, window=FRAME):
    row0, col0, ph, pw = window
    v = np.full((ph, pw), -1, np.int32)
    v[max(r_a - row0, 0):max(r_b - row0, 0), max(c_a - col0, 0):max(c_b - col0, 0)] = value
    return v


def test_box_mask_carves_the_prism():
    """A foreground rectangle of rows r_a .. r_b - 1 and columns c_a .. c_b - 1 keeps exactly the voxels whose centre pixel lies
    in it, whatever x.  The mask's edges are put ON projected centres: the floor rule gives a centre on a pixel border to the
    pixel right of and below it, so the voxel on the rectangle's first column / row stays and the one on the column / row just
    past its end goes."""
    z1, z2, y1, y2 = 5, 20, 7, 25
    c_a, c_b = col_of(z1), col_of(z2)                            # z1 <= z < z2
    r_a, r_b = row_of(y2), row_of(y1)                            # rows run against y: y1 < y <= y2
    views = box_view(r_a, r_b, c_a, c_b)[None]
    votes, hull = VC.carve(views, axis_cam()[None], S32, FRAME, use_depth=False)
    want = np.zeros((S32,) * 3, bool)
    want[z1:z2, y1 + 1:y2 + 1, :] = True
    assert np.array_equal(hull, want) and np.array_equal(votes, want.astype(np.uint8))
    # one pixel further in on every side: the border voxels go
    views = box_view(r_a + 1, r_b, c_a + 1, c_b)[None]
    _, hull = VC.carve(views, axis_cam()[None], S32, FRAME, use_depth=False)
    want[:] = False
    want[z1 + 1:z2, y1 + 1:y2, :] = True
    assert np.array_equal(hull, want)
    # a silhouette is any value >= 0: with use_depth off the value does not matter
    views = box_view(r_a, r_b, c_a, c_b, value=256 * N64)[None]
    _, hull2 = VC.carve(views, axis_cam()[None], S32, FRAME, use_depth=False)
    want[:] = False
    want[z1:z2, y1 + 1:y2 + 1, :] = True
    assert np.array_equal(hull2, want)


def test_outside_keep_against_carve():
    """An all-foreground window smaller than the frame: under "keep" no voxel goes, under "carve" exactly those whose centre pixel
    lies outside the window."""
    window = (row_of(20), col_of(8), row_of(10) - row_of(20), col_of(18) - col_of(8))        # rows of y in (10, 20], columns of z in [8, 18)
    views = np.zeros((1, window[2], window[3]), np.int32)
    _, keep = VC.carve(views, axis_cam()[None], S32, window, use_depth=False, outside_keep=True)
    assert keep.all()
    votes, carved = VC.carve(views, axis_cam()[None], S32, window, use_depth=False, outside_keep=False)
    want = np.zeros((S32,) * 3, bool)
    want[8:18, 11:21, :] = True
    assert np.array_equal(carved, want) and np.array_equal(votes, want.astype(np.uint8))
    # background inside the window carves under both
    views[:] = -1
    for mode in (True, False):
        _, h = VC.carve(views, axis_cam()[None], S32, window, use_depth=False, outside_keep=mode)
        assert np.array_equal(h, ~want if mode else np.zeros_like(want))


def test_tolerance():
    """A voxel column missing from exactly one of K masks survives at tolerance 1 and not at 0."""
    K = 4
    views = np.zeros((K, 256, 256), np.int32)
    views[2, row_of(9), col_of(6)] = -1                          # the centre pixel of the voxels (z, y) = (6, 9) in view 2 alone
    cam = np.stack([axis_cam()] * K)
    votes, hull0 = VC.carve(views, cam, S32, FRAME, use_depth=False, tolerance=0)
    _, hull1 = VC.carve(views, cam, S32, FRAME, use_depth=False, tolerance=1)
    want = np.full((S32,) * 3, K, np.uint8)
    want[6, 9, :] = K - 1
    assert np.array_equal(votes, want)
    assert hull1.all() and not hull0[6, 9].any() and hull0.sum() == S32 ** 3 - S32


@pytest.mark.parametrize("low", [False, True])
def test_depth_plane(low):
    """A plane seen at depth d everywhere: the voxels in front of it go, those with D + slack >= d stay.  d is put 8 units behind
    the centres of the layer x1, so that layer goes at slack 0 and stays at slack 8; at slack 7 it still goes."""
    x1 = 11
    d_layer = 256 * x1 + 4224 if low else 12160 - 256 * x1
    views = np.full((1, 256, 256), d_layer + 8, np.int32)
    x = np.arange(S32)
    behind = (x > x1) if low else (x < x1)                       # deeper than the layer
    for slack, layer_stays in ((0, False), (7, False), (8, True)):
        _, hull = VC.carve(views, axis_cam(low)[None], S32, FRAME, use_depth=True, slack=slack)
        want = np.broadcast_to(behind | ((x == x1) & layer_stays), (S32,) * 3)
        assert np.array_equal(hull, want), slack
    _, hull = VC.carve(views, axis_cam(low)[None], S32, FRAME, use_depth=False)
    assert hull.all()


# ---- the property: a scan's hull loses no voxel of the grid --------------------------------------------------------------------

def model(name):
    from oracle.io_phong import read_binvox
    return read_binvox(os.path.join(BINVOX_DIR, name + ".binvox")).astype(bool)


def scan_and_carve(occ, K, N, f, scale=1.0, slack=8):
    poses, low = synth.scan_poses(K)
    poses = poses.copy()
    poses[:, 2] = np.asarray(scale, np.float32) if np.ndim(scale) == 0 else np.asarray(scale, np.float32)[np.arange(K) % len(scale)]
    views, cam = VC.scan(occ, poses, low, N, f)
    _, hull = VC.carve(views, cam, occ.shape[0], (0, 0, f * N, f * N), use_depth=True, slack=slack)
    return hull, cam


@pytest.mark.parametrize("name,K,bound", [("chair", 24, 1.0), ("bunny", 24, 1.0), ("chair", 12, 0.998), ("chair", 6, 0.97),
                                          ("bunny", 6, 0.98)])
def test_scan_then_carve_loses_nothing(name, K, bound):
    """scan_poses(K), N = 2 S, f = 2, slack 8, two pixels per voxel: no voxel of the grid is missing from the hull, and the hull
    is as tight as the prototype measured (24 views return the grid bit for bit)."""
    occ = model(name)
    hull, cam = scan_and_carve(occ, K, 2 * occ.shape[0], 2)
    assert VC.pixels_per_voxel(cam).min() >= 1.5
    assert (occ & ~hull).sum() == 0
    if bound == 1.0:
        assert np.array_equal(hull, occ)
    else:
        assert VC.iou(hull, occ) >= bound


def test_sphere_at_cycling_scales_loses_nothing():
    occ = XR.sphere_field(32) > np.float32(0.5)
    hull, cam = scan_and_carve(occ, 12, 64, 2, scale=(0.8, 1.0, 1.2))
    assert VC.pixels_per_voxel(cam).min() >= 1.5
    assert (occ & ~hull).sum() == 0 and hull.sum() >= occ.sum()


def test_below_the_documented_condition_voxels_are_lost():
    """The counter-case: the chair at scale 0.73 and f = 1 is seen at 0.73 pixels per voxel, and the hull does lose voxels."""
    occ = model("chair")
    hull, cam = scan_and_carve(occ, 24, 128, 1, scale=0.73)
    assert VC.pixels_per_voxel(cam).max() < 1.5
    assert (occ & ~hull).sum() >= 1


# ---- the entry depth against the rasteriser's ----------------------------------------------------------------------------------

@pytest.mark.parametrize("pose,low", [((4.36, 0.52, 1.0), False), ((0.3, 1.2, 0.9), True)])
def test_hit_depth_against_the_rasterised_blocky_mesh(pose, low):
    """On the stable pixels of the caster's twin, hit_depth is within +-1 unit of the rasteriser's depth of the blocky mesh: the
    two see the same voxel face, one through the float64 ray and one through the integer camera."""
    S, N, f = 32, 64, 4
    occ = XR.sphere_field(S) > np.float32(0.5)
    q, quads = XR.extract(occ.astype(np.uint8), 0.5, smooth=False)
    tris = XR.fan(quads).astype(np.int32)
    M = m_inv_of(pose, S, N)
    cam = MR.camera(M, N, f, low)
    _, tid, depth, _ = MR.rasterize(q, tris, cam, M, S, N, f, smooth=False, cull="back", view_from_low_x=low)
    runs, stable = RR.cast_screened(occ, M, N, f, view_from_low_x=low)
    hit, face, _ = runs[0]
    mine = VC.hit_depth(hit, face, M, S, N, f, view_from_low_x=low)
    assert np.array_equal(mine >= 0, hit >= 0)
    both = stable & (hit >= 0) & (tid >= 0)
    assert both.sum() > 5000
    diff = mine[both].astype(np.int64) - depth[both]
    assert diff.min() >= -1 and diff.max() <= 1, (diff.min(), diff.max())


def test_hit_depth_refuses_what_is_not_a_hit():
    S, N, f = 32, 64, 4
    M = m_inv_of((0.3, 1.2, 0.9), S, N)
    hit = np.array([[-1, S ** 3, S ** 3 - 1, 5, 5, -7]], np.int32)
    face = np.array([[0, 0, 1, 6, -1, 2]], np.int8)
    d = VC.hit_depth(hit, face, M, S, N, f, window=(10, 20, 1, 6))
    assert (d[0, [0, 1, 3, 4, 5]] == -1).all() and 0 <= d[0, 2] <= 256 * N
    # a matrix whose direction has no component on the face's axis: t = 0
    Z = np.zeros((3, 4), np.float32)
    assert VC.hit_depth(hit[:, 2:3], face[:, 2:3], Z, S, N, f, window=(10, 20, 1, 1))[0, 0] == 0


def test_scan_poses():
    poses, low = synth.scan_poses(5, scale=1.25)
    assert poses.dtype == np.float32 and poses.shape == (5, 3) and low == [False, True, False, True, False]
    assert np.allclose(poses[:, 0], 2 * np.pi * np.arange(5) / 5 + 0.1) and np.allclose(poses[:, 1], [0.3, 0.9, 1.4, 0.3, 0.9])
    assert (poses[:, 2] == np.float32(1.25)).all()
    with pytest.raises(ValueError):
        synth.scan_poses(0)


def test_header_states_the_rule():
    hdr = open(os.path.join(ROOT, "include", "rendernet_hip.h")).read()
    assert states_version(hdr)
    assert "Voxel carving" in hdr and "AT LEAST 1.5 PIXELS PER VOXEL" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    assert re.search(r"\brn_voxel_carve\s*\(", code) and re.search(r"\brn_hit_depth\s*\(", code)
