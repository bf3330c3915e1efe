"""Host-side checks of the coloured-mesh twin (tests/mesh_colour_ref.py; include/rendernet_hip.h, rn_mesh_colour_from_ids and
rn_mesh_face_voxels, states the rules): the voxel behind every face of smooth, blocky and relaxed nets, closed forms that pin
the integer interpolation, and the cross-check against the ray caster's twin on the blocky sphere, where the flat face-coloured
mesh and the coloured grid must show the same bytes.  No GPU."""
import os

import numpy as np
import pytest

import mesh_colour_ref as MC
import mesh_extract_ref as XR
import mesh_raster_ref as MR
import mesh_relax_ref as MX
import raycast_ref as RR
from conftest import BINVOX_DIR
from oracle import resample as OR

POSES32 = ((4.36, 0.52, 1.0), (0.3, 1.2, 0.9), (2.0, 2.6, 0.8))         # radians: azimuth, elevation; scale


def m_inv_of(pose, S, N):
    return OR.inverse_affine(np.asarray(pose, np.float32)[None], size=S, new_size=N)[0].astype(np.float32)


def axis_pose():
    """Azimuth 90 degrees, elevation 0, scale 1: at S = N the camera is X = f q0, Y = 256 f N - f q1, D = 256 N - q2, exactly."""
    return (np.float32(np.pi / 2), 0.0, 1.0)


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


def pooled_model(name="teapot"):
    """A shipped 64^3 model max-pooled to 32^3, uint8."""
    from oracle.io_phong import read_binvox
    occ = read_binvox(os.path.join(BINVOX_DIR, name + ".binvox")).astype(np.uint8)
    return occ.reshape(32, 2, 32, 2, 32, 2).max((1, 3, 5))


_fields = {}


def field(name):
    """name -> (vol [32,32,32], threshold): the binary sphere's soft field at its own and at a non-trivial threshold, a model."""
    if not _fields:
        _fields["sphere"] = XR.cases32()["sphere"]
        _fields["soft_sphere"] = (XR.sphere_field(32, radius=10.3), 0.8125)
        _fields["model"] = (pooled_model(), 0.5)
    return _fields[name]


def across(ids, tris_axis_sign, S):
    """The sample on the other side of each face from voxel `ids`, as coordinates [F,3] (it may lie outside the grid)."""
    axis, sign = tris_axis_sign
    vox = np.stack([ids // (S * S), (ids // S) % S, ids % S], 1).astype(np.int64)
    vox[np.arange(len(ids)), axis] += sign
    return vox


@pytest.mark.parametrize("name", ["sphere", "soft_sphere", "model"])
def test_face_voxels_of_smooth_blocky_and_relaxed_nets(name):
    """Every face names the inside sample of its edge and the sample across it is outside -- quads and fans, wherever in their
    cells the vertices sit -- and on the blocky net that is the voxel whose exposed side the face is."""
    vol, thr = field(name)
    S = 32
    inside = vol.astype(np.float32) > np.float32(thr)
    assert 500 < inside.sum() < S ** 3 // 2
    bq, btris, hit_of, _ = blocky_faces(inside)
    n = MR.face_normals(bq, btris, S)
    axis = np.argmax(np.abs(n), 1)
    sign = np.sign(n[np.arange(len(n)), axis]).astype(np.int64)
    q_smooth, faces = XR.extract(vol, thr, smooth=True)
    q_blocky, faces_b = XR.extract(vol, thr, smooth=False)
    assert np.array_equal(faces, faces_b) and np.array_equal(q_blocky, bq) and np.array_equal(XR.fan(faces), btris)
    q_relaxed = MX.relax(q_smooth, faces, S, 4)
    assert not np.array_equal(q_relaxed, q_smooth)
    for q in (q_smooth, q_blocky, q_relaxed):
        for f, want, ax, sg in ((faces, hit_of[::2], axis[::2], sign[::2]), (XR.fan(faces), hit_of, axis, sign)):
            ids = MC.face_voxels(q, f, vol, thr)
            assert ids.dtype == np.int32 and ids.shape == (len(f),) and (ids >= 0).all()
            assert inside.reshape(-1)[ids].all()
            other = across(ids.astype(np.int64), (ax, sg), S)
            real = ((other >= 0) & (other < S)).all(1)
            oc = np.clip(other, 0, S - 1)
            assert not (real & inside[oc[:, 0], oc[:, 1], oc[:, 2]]).any()
            assert np.array_equal(ids, want)


def test_face_voxels_of_a_full_grid_and_of_strangers():
    """A full grid: every face stands against a virtual sample, 6 S^2 of them, each voxel side once.  Faces that are no ring of
    this grid -- a repeated vertex, vertices two cells apart -- and an empty net give -1."""
    S = 32
    vol, thr = XR.cases32()["full"]
    for smooth in (True, False):
        q, faces = XR.extract(vol, thr, smooth=smooth)
        assert len(faces) == 6 * S * S
        for f in (faces, XR.fan(faces)):
            ids = MC.face_voxels(q, f, vol, thr)
            v = np.stack([ids // (S * S), (ids // S) % S, ids % S], 1)
            assert (ids >= 0).all() and ((v == 0) | (v == S - 1)).any(1).all()
            assert np.bincount(ids, minlength=S ** 3).max() == 3 * (f.shape[1] == 4) + 6 * (f.shape[1] == 3)
    q, faces = XR.extract(*XR.cases32()["sphere"])
    bad = faces[:4].copy()
    bad[0, 1] = bad[0, 2] = bad[0, 0]                            # all three in the owning cell: three shared axes
    bad[1, 2] = bad[1, 1]                                        # vertices 1 and 2 the same: two shared axes
    bad[2, 1] = faces[-1, 0]                                     # a vertex from the far side of the sphere
    got = MC.face_voxels(q, bad, *XR.cases32()["sphere"])
    assert (got[:3] == -1).all() and got[3] >= 0
    assert (MC.face_voxels(q, faces, np.zeros((S, S, S), np.float32), 0.5) == -1).all()     # both ends outside
    assert MC.face_voxels(np.zeros((0, 3), np.int32), faces[:5], vol, thr).tolist() == [-1] * 5
    assert MC.face_voxels(q, faces[:0], vol, thr).shape == (0,)


_sphere = {}


def sphere_net(smooth=True):
    if smooth not in _sphere:
        vol, thr = XR.cases32()["sphere"]
        q, faces = XR.extract(vol, thr, smooth=smooth)
        _sphere[smooth] = (vol > np.float32(thr), q, XR.fan(faces).astype(np.int32))
    return _sphere[smooth]


def test_equal_vertex_colours_give_that_colour_and_bytes_stay_inside_the_triangle():
    S = N = 32
    f = 4
    _, q, tris = sphere_net()
    M = m_inv_of(POSES32[0], S, N)
    cam = MR.camera(M, N, f)
    window = (0, 0, f * N, f * N)
    _, tid, _, _ = MR.rasterize(q, tris, cam, M, S, N, f)
    hit = tid >= 0
    assert hit.sum() > 3000
    one = np.tile(np.array([[17, 200, 99]], np.uint8), (len(q), 1))
    got = MC.colour_from_ids(q, tris, cam, tid, S, window, vertex_colours=one, background=(1, 2, 3))
    assert (got[hit] == one[0]).all() and (got[~hit] == np.array([1, 2, 3], np.uint8)).all()
    vcol = np.random.RandomState(3).randint(0, 256, (len(q), 3)).astype(np.uint8)
    got = MC.colour_from_ids(q, tris, cam, tid, S, window, vertex_colours=vcol)
    corner = vcol[tris[tid[hit]]]                                # [n,3 vertices,3 channels]
    assert (got[hit] >= corner.min(1)).all() and (got[hit] <= corner.max(1)).all()
    assert len(np.unique(got[hit].reshape(-1))) > 200            # really interpolated, not one corner's colour
    fcol = np.random.RandomState(4).randint(0, 256, (len(tris), 3)).astype(np.uint8)
    got = MC.colour_from_ids(q, tris, cam, tid, S, window, face_colours=fcol, background=(9, 9, 9))
    assert (got[hit] == fcol[tid[hit]]).all() and (got[~hit] == 9).all()


def test_a_pixel_centre_on_a_vertex_gets_that_vertex_colour():
    """Vertices that project onto pixel centres (X = 4 q0 = 128 mod 256): there one weight is A and two are 0.  The rule needs
    no coverage, so every pixel of the window is asked about triangle 0."""
    S = N = 32
    f = 4
    M = m_inv_of(axis_pose(), S, N)
    cam = MR.camera(M, N, f)
    q = np.array([[64 * 10 + 32, 64 * 50 + 32, 3000], [64 * 90 + 32, 64 * 30 + 32, 3100], [64 * 40 + 32, 64 * 100 + 32, 2900]], np.int32)
    P = MR.project(cam, q, S)
    assert (P[:, :2] % 256 == 128).all()
    vcol = np.array([[255, 0, 31], [0, 255, 77], [128, 3, 250]], np.uint8)
    for tris in (np.array([[0, 1, 2]], np.int32), np.array([[0, 2, 1]], np.int32), np.array([[2, 0, 1]], np.int32)):
        window = (0, 0, f * N, f * N)
        got = MC.colour_from_ids(q, tris, cam, np.zeros((f * N, f * N), np.int32), S, window, vertex_colours=vcol)
        for k in range(3):
            assert (got[(P[k, 1] - 128) // 256, (P[k, 0] - 128) // 256] == vcol[k]).all(), (tris, k)
    # a triangle without area: the plain mean, rounded half up
    flat = np.array([[0, 0, 0]], np.int32)
    got = MC.colour_from_ids(q, flat, cam, np.zeros((4, 4), np.int32), S, (0, 0, 4, 4), vertex_colours=vcol)
    assert (got == vcol[0]).all()
    line = np.array([[1000, 1000, 3000], [2000, 2000, 3000], [3000, 3000, 3000]], np.int32)
    got = MC.colour_from_ids(line, np.array([[0, 1, 2]], np.int32), cam, np.zeros((4, 4), np.int32), S, (0, 0, 4, 4), vertex_colours=vcol)
    assert (got == (2 * vcol.astype(np.int64).sum(0) + 3) // 6).all()


def test_an_affine_colour_field_does_not_see_how_the_square_is_cut():
    """Vertex colours that are an affine integer function of the projected coordinates: the interpolated value at a pixel centre
    is that function there, exactly, in rationals -- the same number whichever triangle covers the pixel -- so the rounded bytes
    of the square cut along either diagonal or as a 4-fan about its centre are identical."""
    S = N = 32
    f = 4
    M = m_inv_of(axis_pose(), S, N)
    cam = MR.camera(M, N, f)
    a2 = 12 * 256 + 77
    lo0, hi0, lo1, hi1 = 64 * 9, 64 * 89, 64 * 13, 64 * 101      # projected sides 80 and 88 pixels
    q = np.array([[lo0, lo1, a2], [hi0, lo1, a2], [hi0, hi1, a2], [lo0, hi1, a2], [(lo0 + hi0) // 2, (lo1 + hi1) // 2, a2]], np.int32)
    P = MR.project(cam, q, S)
    dx, dy = (P[:, 0] - P[:, 0].min()) // 256, (P[:, 1] - P[:, 1].min()) // 256
    assert ((P[:, 0] - P[:, 0].min()) % 256 == 0).all() and ((P[:, 1] - P[:, 1].min()) % 256 == 0).all()
    assert dx.max() == 80 and dy.max() == 88 and dx[4] == 40 and dy[4] == 44
    vcol = np.stack([3 * dx + 7, 2 * dy + 11, 255 - dx - dy], 1)
    assert vcol.min() >= 0 and vcol.max() <= 255
    vcol = vcol.astype(np.uint8)
    cuts = (np.array([[0, 1, 2], [0, 2, 3]], np.int32), np.array([[0, 1, 3], [1, 2, 3]], np.int32),
            np.array([[4, 0, 1], [4, 1, 2], [4, 2, 3], [4, 3, 0]], np.int32))
    window = (0, 0, f * N, f * N)
    pictures = []
    for tris in cuts:
        _, tid, _, _ = MR.rasterize(q, tris, cam, M, S, N, f, smooth=False, cull="none")
        assert (tid >= 0).sum() == 80 * 88 and len(np.unique(tid[tid >= 0])) == len(tris)
        pictures.append(MC.colour_from_ids(q, tris, cam, tid, S, window, vertex_colours=vcol))
    assert np.array_equal(pictures[0], pictures[1]) and np.array_equal(pictures[0], pictures[2])
    # and it is the function itself: at pixel centre 256 k + 128 the field is 3 (k - k0) + 1.5 + 7, rounded half up
    r, c = np.nonzero(pictures[0].any(2))
    k0 = P[:, 0].min() // 256
    assert np.array_equal(pictures[0][r, c, 0], (2 * (3 * (256 * c + 128 - P[:, 0].min()) + 7 * 256) + 256) // 512)
    assert c.min() == k0


@pytest.mark.parametrize("pose,low_x", [(POSES32[0], False), (POSES32[1], False), (POSES32[2], False), (POSES32[0], True)])
def test_blocky_sphere_against_the_caster(pose, low_x):
    """The flat face-coloured blocky mesh shows, on every pixel the caster's twin calls stable, the colour of the voxel the
    caster's ray hits (S = N = 32, f = 8): face_voxels, the rasteriser's ids and colour_from_ids against colours[hit]."""
    S = N = 32
    f = 8
    occ, _, _ = sphere_net()
    q, quads = XR.extract(occ.astype(np.uint8), 0.5, smooth=False)
    tris = XR.fan(quads).astype(np.int32)
    colours = np.random.RandomState(11).randint(1, 256, (S, S, S, 3)).astype(np.uint8)
    voxel = MC.face_voxels(q, tris, occ.astype(np.uint8), 0.5)
    assert (voxel >= 0).all()
    fcol = colours.reshape(-1, 3)[voxel]
    M = m_inv_of(pose, S, N)
    cam = MR.camera(M, N, f, low_x)
    _, tid, _, _ = MR.rasterize(q, tris, cam, M, S, N, f, smooth=False, cull="back", view_from_low_x=low_x)
    got = MC.colour_from_ids(q, tris, cam, tid, S, (0, 0, f * N, f * N), face_colours=fcol)
    runs, stable = RR.cast_screened(occ, M, N, f, view_from_low_x=low_x)
    share = 1.0 - float(np.mean(stable))
    assert share <= RR.MAX_UNSTABLE, "the reference's own unstable share is %.4f %%" % (100 * share)
    hit = runs[0][0]
    want = np.where((hit >= 0)[..., None], colours.reshape(-1, 3)[np.maximum(hit, 0)], 0).astype(np.uint8)
    bad = stable & (got != want).any(2)
    assert not bad.any(), "%d stable pixels differ, first at %s" % (bad.sum(), np.argwhere(bad)[0])
    assert (stable & (hit >= 0)).sum() > 0.1 * hit.size
