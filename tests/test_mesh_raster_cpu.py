"""Host-side checks of the mesh rasteriser's NumPy twin (tests/mesh_raster_ref.py; include/rendernet_hip.h, rn_mesh_rasterize,
states the rule): closed forms that pin the tie rule and the culling, the integer camera against the float64 projection, and the
cross-check against the ray caster's twin on blocky meshes, where the two must show the same voxel face.  No GPU."""
import os

import numpy as np
import pytest

import mesh_extract_ref as XR
import mesh_raster_ref as MR
import raycast_ref as RR
from conftest import BINVOX_DIR
from oracle import resample as OR

POSES32 = ((4.36, 0.52, 1.0), (0.3, 1.2, 0.9), (2.0, 2.6, 0.8))         # radians: azimuth, elevation; scale


def m_inv_of(pose, S, N):
    return OR.inverse_affine(np.asarray(pose, np.float32)[None], size=S, new_size=N)[0].astype(np.float32)


def axis_pose():
    """Azimuth 90 degrees, elevation 0, scale 1: M_inv is a translation, the camera looks along the source x axis."""
    return (np.float32(np.pi / 2), 0.0, 1.0)


def box_mesh(lo, hi):
    """The 8 corners and 12 outward-wound triangles of the lattice box lo .. hi (array-axis order)."""
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    q = np.array([[(hi if (i >> a) & 1 else lo)[a] for a in range(3)] for i in range(8)], np.int32)
    quads = []
    for a in range(3):
        u, v = (a + 1) % 3, (a + 2) % 3
        for side in (0, 1):
            base = side << a
            ring = [base, base | (1 << u), base | (1 << u) | (1 << v), base | (1 << v)]     # (u, v) counter-clockwise: normal +a
            quads.append(ring if side else ring[::-1])
    return q, XR.fan(np.array(quads)).astype(np.int32)


def test_box_mesh_is_outward():
    q, tris = box_mesh((256, 512, 768), (1024, 2048, 3072))
    n = MR.face_normals(q, tris, 32)
    centre = q.astype(np.float64).mean(0)
    mid = q[tris].astype(np.float64).mean(1)
    assert (np.sum(n * (mid - centre), 1) > 0).all()


def square_meshes(rng, a2=12 * 256 + 77):
    """A square in a plane of constant array axis 2 (source x), normal towards +x, as 2 triangles and as a fan of about 200
    around an interior lattice point with the rim points exactly on its sides."""
    lo0, hi0, lo1, hi1 = 2 * 256 + 31, 27 * 256 + 200, 3 * 256 + 5, 25 * 256 + 131
    corners = np.array([[lo0, lo1, a2], [hi0, lo1, a2], [hi0, hi1, a2], [lo0, hi1, a2]], np.int32)
    two = XR.fan(np.array([[0, 1, 2, 3]])).astype(np.int32)
    rim = []
    for k in range(4):
        p, n = corners[k].astype(np.int64), corners[(k + 1) % 4].astype(np.int64)
        axis = int(np.nonzero(n - p)[0][0])
        steps = np.sort(rng.choice(np.arange(1, abs(int(n[axis] - p[axis]))), 49, replace=False))
        rim.append(p)
        for s in steps:
            r = p.copy()
            r[axis] += np.sign(n[axis] - p[axis]) * s
            rim.append(r)
    rim = np.array(rim, np.int32)
    centre = np.array([[11 * 256 + 3, 17 * 256 + 90, a2]], np.int32)
    q = np.concatenate([centre, rim])
    R = len(rim)
    fan = np.array([[0, 1 + i, 1 + (i + 1) % R] for i in range(R)], np.int32)
    return (corners, two), (q, fan)


@pytest.mark.parametrize("low_x", [False, True])
def test_square_fan_equals_two_triangles(low_x):
    """No pixel is lost or doubled on shared edges: identical coverage and depth however the square is cut."""
    S, N, f = 32, 64, 4
    M = m_inv_of(axis_pose(), S, N)
    cam = MR.camera(M, N, f, low_x)
    (q2, t2), (qf, tf) = square_meshes(np.random.RandomState(7))
    assert len(tf) == 200
    if low_x:                                                   # seen from low x the square must face -x
        t2, tf = t2[:, ::-1], tf[:, ::-1]
    _, id2, d2, _ = MR.rasterize(q2, t2, cam, M, S, N, f, smooth=False, view_from_low_x=low_x)
    _, idf, df, _ = MR.rasterize(qf, tf, cam, M, S, N, f, smooth=False, view_from_low_x=low_x)
    assert (id2 >= 0).sum() > 5000
    assert np.array_equal(id2 >= 0, idf >= 0) and np.array_equal(d2, df)
    assert len(np.unique(idf[idf >= 0])) > 150                   # the fan really shares the pixels out
    P = MR.project(cam, q2, S)
    assert len(set(P[:, 2])) == 1 and (d2[id2 >= 0] == P[0, 2]).all()


def _centres_in(lo, hi):
    """Pixel centres 256 k + 128 in (lo, hi]: the sides the tie rule gives a rectangle wound to A > 0."""
    return int((hi - 128) // 256 - (lo - 128) // 256)


@pytest.mark.parametrize("low_x", [False, True])
@pytest.mark.parametrize("cull", ["back", "none"])
def test_box_at_an_axis_aligned_pose(cull, low_x):
    """The picture of a box seen along x is its facing side: exactly the pixels whose centre lies in the projected lattice
    rectangle, left and top sides open, right and bottom closed, at that side's depth."""
    S, N, f = 32, 64, 4
    M = m_inv_of(axis_pose(), S, N)
    cam = MR.camera(M, N, f, low_x)
    lo, hi = (5 * 256 + 17, 7 * 256 + 128, 9 * 256 + 1), (20 * 256 + 128, 19 * 256 + 250, 22 * 256 + 99)
    q, tris = box_mesh(lo, hi)
    rgb, tid, depth, _ = MR.rasterize(q, tris, cam, M, S, N, f, smooth=False, cull=cull, view_from_low_x=low_x)
    P = MR.project(cam, q, S)
    want = _centres_in(P[:, 0].min(), P[:, 0].max()) * _centres_in(P[:, 1].min(), P[:, 1].max())
    assert want > 2000 and (tid >= 0).sum() == want
    assert (depth[tid >= 0] == P[:, 2].min()).all()
    # the facing side: array axis 2 = source x, its high side unless the view is from low x; straight at the camera
    n = MR.face_normals(q, tris, S)[np.unique(tid[tid >= 0])]
    assert (n[:, :2] == 0).all() and (np.sign(n[:, 2]) == (-1 if low_x else 1)).all()
    assert (rgb[tid >= 0] == np.array([128, 128, 255], np.uint8)).all() and (rgb[tid < 0] == 0).all()


def test_axes_sign_and_the_mirror_swap():
    """fit with axes of negative determinant mirrors the mesh; swapping two triangle columns, as MeshSet.from_files does, winds it
    outwards again in array-axis order."""
    from rendernet_amd import mesh
    assert [mesh.axes_sign(a) for a in ("x,y,z", "z,y,x", "-y,z,x", "y,z,x", "x,-y,-z", "-x,-y,-z")] == [1, -1, -1, 1, 1, -1]
    q, tris = box_mesh((0, 0, 0), (256, 512, 384))
    for axes in ("x,y,z", "z,y,x", "-x,y,z", "y,z,x"):
        fq = mesh.fit(q.astype(np.float64), 32, 1, axes)
        t = tris if mesh.axes_sign(axes) > 0 else tris[:, [0, 2, 1]]
        n = MR.face_normals(fq, t, 32)
        mid = fq[t].astype(np.float64).mean(1)
        assert (np.sum(n * (mid - fq.astype(np.float64).mean(0)), 1) > 0).all(), axes


_sphere = {}


def sphere_net(smooth=True):
    if smooth not in _sphere:
        vol, thr = XR.cases32()["sphere"]
        q, faces = XR.extract(vol, thr, smooth=smooth)
        _sphere[smooth] = (vol > np.float32(thr), q, XR.fan(faces).astype(np.int32))
    return _sphere[smooth]


@pytest.mark.parametrize("low_x", [False, True])
def test_reversed_winding(low_x):
    """Every triangle of the square that faces the camera reversed: nothing under cull "back", the same ids and depths as before
    under "none".  A closed surface has the same ids and depths under "none" whichever way it is wound."""
    S, N, f = 32, 64, 4
    M = m_inv_of(axis_pose(), S, N)
    cam = MR.camera(M, N, f, low_x)
    _, (q, tris) = square_meshes(np.random.RandomState(11))
    if low_x:
        tris = tris[:, ::-1]
    rev = np.ascontiguousarray(tris[:, ::-1])
    _, tid0, depth0, _ = MR.rasterize(q, tris, cam, M, S, N, f, smooth=False, cull="back", view_from_low_x=low_x)
    assert (tid0 >= 0).sum() > 5000
    rgb, tid, depth, _ = MR.rasterize(q, rev, cam, M, S, N, f, smooth=False, cull="back", view_from_low_x=low_x)
    assert (tid == -1).all() and (depth == -1).all() and (rgb == 0).all()
    rgb, tid, depth, _ = MR.rasterize(q, rev, cam, M, S, N, f, smooth=False, cull="none", view_from_low_x=low_x)
    assert np.array_equal(tid, tid0) and np.array_equal(depth, depth0)
    assert (rgb[tid >= 0] == np.array([128, 128, 255], np.uint8)).all()      # the shading normal is turned towards the viewer

    S = N = 32
    _, q, tris = sphere_net()
    M = m_inv_of(POSES32[0], S, N)
    cam = MR.camera(M, N, f, low_x)
    rev = np.ascontiguousarray(tris[:, ::-1])
    _, tid_b, _, _ = MR.rasterize(q, tris, cam, M, S, N, f, cull="back", view_from_low_x=low_x)
    assert (tid_b >= 0).sum() > 3000
    rgb_n, tid_n, depth_n, _ = MR.rasterize(q, tris, cam, M, S, N, f, cull="none", view_from_low_x=low_x)
    rgb_r, tid_r, depth_r, _ = MR.rasterize(q, rev, cam, M, S, N, f, cull="none", view_from_low_x=low_x)
    assert np.array_equal(tid_n, tid_r) and np.array_equal(depth_n, depth_r)
    assert np.array_equal(tid_n >= 0, tid_b >= 0)                # a closed surface: the same silhouette either way


def test_smooth_normals_of_a_sphere_point_away_from_its_centre():
    """The decoded bytes of the smooth sphere are the radial direction seen by the camera, to a few degrees."""
    S = N = 32
    f = 4
    _, q, tris = sphere_net()
    M = m_inv_of(POSES32[0], S, N)
    cam = MR.camera(M, N, f)
    rgb, tid, depth, min_dot = MR.rasterize(q, tris, cam, M, S, N, f)
    assert min_dot > 0.1
    hit = tid >= 0
    n = rgb[hit].astype(np.float64) / 127.5 - 1.0                # (right, up, towards)
    r, c = np.nonzero(hit)
    centre = 0.5 * (MR.project(cam, q, S).max(0) + MR.project(cam, q, S).min(0))
    right, up = (256 * c + 128 - centre[0]), -(256 * r + 128 - centre[1])
    radius = 0.5 * (MR.project(cam, q, S)[:, 0].max() - MR.project(cam, q, S)[:, 0].min())
    want = np.stack([right, up], 1) / radius
    assert np.abs(n[:, :2] - want).max() < 0.12 and (n[:, 2] > -0.05).all()


@pytest.mark.parametrize("f", [4, 8])
def test_integer_camera_against_float64(f):
    """cam reproduces 256 X, 256 Y, 256 D of the float64 projection within 0.51 units on every vertex of a 32^3 surface net."""
    S = N = 32
    _, q, _ = sphere_net()
    for pose in POSES32:
        for low_x in (False, True):
            M = m_inv_of(pose, S, N)
            cam = MR.camera(M, N, f, low_x)
            exact = MR.project_float(M, q, N, f, low_x)
            got = (q.astype(np.int64) @ cam[:, :3].T + cam[:, 3] + (1 << 19)) >> 20
            assert np.abs(got - exact).max() <= 0.51
            assert np.array_equal(got, MR.project(cam, q, S))   # nothing near the clamps
    assert (MR.camera(np.zeros((3, 4), np.float32), N, f) == 0).all()


def blocky_faces(occ):
    """The blocky mesh of occ [S,S,S] and, per triangle, the caster's (hit id, face) of the voxel side it lies on."""
    S = occ.shape[0]
    q, quads = XR.extract(occ.astype(np.uint8), 0.5, smooth=False)
    tris = XR.fan(quads).astype(np.int32)
    n = MR.face_normals(q, tris, S)
    axis = np.argmax(np.abs(n), 1)
    assert ((n != 0).sum(1) == 1).all()
    sign = np.sign(n[np.arange(len(n)), axis])
    centre = np.repeat(q[quads].astype(np.int64).sum(1) // 4, 2, 0)          # the side's centre: 256 k + 128 on its own two axes
    vox = centre // 256
    vox[np.arange(len(n)), axis] = centre[np.arange(len(n)), axis] // 256 - (sign > 0)
    assert occ[vox[:, 0], vox[:, 1], vox[:, 2]].all()
    hit_id = ((vox[:, 0] * S + vox[:, 1]) * S + vox[:, 2]).astype(np.int32)
    face = (2 * (2 - axis) + (sign > 0)).astype(np.int8)                     # array axis a is source axis 2 - a
    return q, tris, hit_id, face


def cross_check(occ, S, N, f, pose, low_x):
    q, tris, hit_of, face_of = blocky_faces(occ)
    M = m_inv_of(pose, S, N)
    cam = MR.camera(M, N, f, low_x)
    _, tid, _, _ = MR.rasterize(q, tris, cam, M, S, N, f, smooth=False, cull="back", view_from_low_x=low_x)
    hit = np.where(tid >= 0, hit_of[np.maximum(tid, 0)], -1)
    face = np.where(tid >= 0, face_of[np.maximum(tid, 0)], 0)
    runs, stable = RR.cast_screened(occ, M, N, f, view_from_low_x=low_x)
    share = 1.0 - float(np.mean(stable))
    assert share <= RR.MAX_UNSTABLE, "the reference's own unstable share is %.4f %%" % (100 * share)
    match = [(hit == h) & (face == fa) for h, fa, _ in runs]
    bad = stable & ~match[0]
    assert not bad.any(), "%d stable pixels differ, first at %s: rasteriser (%d, %d) caster (%d, %d)" % (
        bad.sum(), np.argwhere(bad)[0], hit[bad][0], face[bad][0], runs[0][0][bad][0], runs[0][1][bad][0])
    bad = ~stable & ~np.any(np.stack(match), 0)
    assert not bad.any(), "%d unstable pixels equal none of the five runs, first at %s" % (bad.sum(), np.argwhere(bad)[0])
    assert (hit >= 0).sum() > 0.1 * hit.size
    print("unstable share %.4f, %d hits" % (share, (hit >= 0).sum()))


@pytest.mark.parametrize("pose,low_x", [(POSES32[0], False), (POSES32[1], False), (POSES32[2], False), (POSES32[0], True)])
def test_blocky_sphere_against_the_caster(pose, low_x):
    """The rasterised blocky mesh shows the voxel side the caster's ray enters, pixel for pixel (S = N = 32, f = 8)."""
    occ, _, _ = sphere_net()
    cross_check(occ, 32, 32, 8, pose, low_x)


@pytest.mark.parametrize("pose,low_x", [((4.36, 0.52, 1.0), False), ((1.1, 1.9, 0.85), False), ((4.36, 0.52, 1.0), True)])
def test_blocky_teapot_against_the_caster(pose, low_x):
    """The same on a shipped model (S = N = 64, f = 4)."""
    from oracle.io_phong import read_binvox
    occ = read_binvox(os.path.join(BINVOX_DIR, "teapot.binvox")).astype(bool)
    cross_check(occ, 64, 64, 4, pose, low_x)
