"""rn_mesh_camera / rn_mesh_vertex_normals / rn_mesh_rasterize on the device against the NumPy twin (tests/mesh_raster_ref.py):
triangle ids and depths exactly on every pixel with the twin fed the device's integer camera, normal bytes within +-1 (float32
against float64, the tolerance raycast_ref.check_against uses for the same encoding); the camera against the float64 path; both
work paths (lane, wave), windows, degenerate input, empty input, several meshes, stray indices, determinism, the argument
checks.  -m gpu."""
import numpy as np
import pytest

import mesh_extract_ref as XR
import mesh_raster_ref as MR

pytestmark = pytest.mark.gpu
POSES32 = ((4.36, 0.52, 1.0), (0.3, 1.2, 0.9), (2.0, 2.6, 0.8))


def _dev(a, dtype=None):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


@pytest.fixture(scope="module")
def sphere():
    vol, thr = XR.cases32()["sphere"]
    q, faces = XR.extract(vol, thr, smooth=True)
    return q, XR.fan(faces).astype(np.int32)


def box_mesh(lo, hi):
    lo, hi = np.asarray(lo, np.int64), np.asarray(hi, np.int64)
    q = np.array([[(hi if (i >> a) & 1 else lo)[a] for a in range(3)] for i in range(8)], np.int32)
    quads = []
    for a in range(3):
        u, v = (a + 1) % 3, (a + 2) % 3
        for side in (0, 1):
            base = side << a
            ring = [base, base | (1 << u), base | (1 << u) | (1 << v), base | (1 << v)]
            quads.append(ring if side else ring[::-1])
    return q, XR.fan(np.array(quads)).astype(np.int32)


def against_twin(meshes, mesh_of_item, poses, S, N, f, window=None, smooth=True, cull="back", low_x=False, min_hits=1):
    """meshes: [(q, tris)]; runs the device once over the batch and the twin per item; returns the device's (rgb, ids, depth)."""
    import torch
    from rendernet_amd import ops
    vo = np.cumsum([0] + [len(q) for q, _ in meshes]).astype(np.int64)
    to = np.cumsum([0] + [len(t) for _, t in meshes]).astype(np.int64)
    q = np.concatenate([q for q, _ in meshes]).astype(np.int32).reshape(-1, 3)
    tris = np.concatenate([t for _, t in meshes]).astype(np.int32).reshape(-1, 3)
    pose = _dev(np.asarray(poses, np.float32).reshape(-1, 3))
    B = int(pose.shape[0])
    m_inv = ops.pose_to_affine(pose, S, N) if B else pose.new_empty((0, 3, 4))
    kw = dict(new_size=N, pixels_per_cell=f, affine=True, view_from_low_x=low_x)
    many = len(meshes) > 1 or mesh_of_item is not None
    sets = dict(vert_offsets=_dev(vo), tri_offsets=_dev(to),
                mesh_of_item=_dev(np.asarray(mesh_of_item if mesh_of_item is not None else [0] * B, np.int32))) if many else {}
    rgb, ids, depth = ops.rasterize_mesh(_dev(q), _dev(tris), m_inv, S, window=window, smooth=smooth, cull=cull,
                                         return_ids=True, **sets, **kw)
    cam = ops.mesh_camera(m_inv, S, **kw).cpu().numpy()
    torch.cuda.synchronize()
    rgb, ids, depth, M = rgb.cpu().numpy(), ids.cpu().numpy(), depth.cpu().numpy(), m_inv.cpu().numpy()
    assert rgb.dtype == np.uint8 and ids.dtype == np.int32 and depth.dtype == np.int32
    hits = 0
    for b in range(B):
        mq, mt = meshes[mesh_of_item[b] if mesh_of_item is not None else 0]
        want_cam = MR.camera(M[b], N, f, low_x)
        assert np.abs(cam[b] - want_cam).max() <= 1, (b, cam[b], want_cam)
        w_rgb, w_ids, w_depth, min_dot = MR.rasterize(mq, mt, cam[b], M[b], S, N, f, window, smooth, cull, low_x)
        if smooth:
            assert min_dot > 0.1, "the twin's fallback branch is too close to deciding a byte: %g" % min_dot
        assert np.array_equal(ids[b], w_ids), (b, int((ids[b] != w_ids).sum()), np.argwhere(ids[b] != w_ids)[:3])
        assert np.array_equal(depth[b], w_depth), (b, int((depth[b] != w_depth).sum()))
        err = np.abs(rgb[b].astype(np.int64) - w_rgb.astype(np.int64))
        assert err.max() <= 1, (b, int(err.max()), np.argwhere(err > 1)[:3])
        assert (rgb[b][ids[b] < 0] == 0).all() and (depth[b][ids[b] < 0] == -1).all()
        hits += int((ids[b] >= 0).sum())
    assert hits >= min_hits, hits
    return rgb, ids, depth


@pytest.mark.parametrize("cull", ["back", "none"])
@pytest.mark.parametrize("smooth", [True, False])
def test_sphere_net_at_three_poses(sphere, smooth, cull):
    """About 5 000 triangles of a few pixels each: the lane path, three items in one call."""
    assert 4000 < len(sphere[1]) < 8000
    against_twin([sphere], None, POSES32, 32, 32, 4, smooth=smooth, cull=cull, min_hits=9000)


def test_sphere_net_from_low_x(sphere):
    against_twin([sphere], None, POSES32[:1], 32, 32, 4, low_x=True, min_hits=3000)


def test_device_camera_against_float64():
    """cam of the device (float64 adjugate) within one unit of 2^-20 of the NumPy inverse, at f = 4 and 8, both view sides; a
    singular matrix gives the zero camera."""
    import torch
    from rendernet_amd import ops
    pose = _dev(np.asarray(POSES32, np.float32))
    for S, N, f in ((32, 32, 4), (32, 32, 8), (64, 128, 4), (64, 128, 16)):
        M = ops.pose_to_affine(pose, S, N)
        for low_x in (False, True):
            cam = ops.mesh_camera(M, S, new_size=N, pixels_per_cell=f, affine=True, view_from_low_x=low_x).cpu().numpy()
            assert cam.dtype == np.int64 and cam.shape == (3, 3, 4)
            for b in range(3):
                assert np.abs(cam[b] - MR.camera(M[b].cpu().numpy(), N, f, low_x)).max() <= 1
            by_pose = ops.mesh_camera(pose, S, new_size=N, pixels_per_cell=f, view_from_low_x=low_x).cpu().numpy()
            assert np.array_equal(by_pose, cam)
    assert (ops.mesh_camera(torch.zeros((2, 3, 4), device="cuda"), 32, new_size=32, affine=True).cpu().numpy() == 0).all()


def test_vertex_normals_equal_the_twin(sphere):
    from rendernet_amd import ops
    q, tris = sphere
    bq, bt = box_mesh((300, 700, 900), (5000, 6000, 7000))
    got = ops.mesh_vertex_normals(_dev(q), _dev(tris), 32).cpu().numpy()
    assert got.dtype == np.int64 and np.array_equal(got, MR.vertex_normals(q, tris, 32))
    both = ops.mesh_vertex_normals(_dev(np.concatenate([bq, q])), _dev(np.concatenate([bt, tris])), 32,
                                   vert_offsets=_dev(np.array([0, 8, 8 + len(q)], np.int64)),
                                   tri_offsets=_dev(np.array([0, 12, 12 + len(tris)], np.int64))).cpu().numpy()
    assert np.array_equal(both[:8], MR.vertex_normals(bq, bt, 32)) and np.array_equal(both[8:], got)


def test_one_triangle_over_a_whole_window():
    """A 64 x 64 window inside one triangle: 4 096 pixels from one work item, the wave path."""
    q = np.array([[200, 300, 4000], [8000, 250, 4100], [4000, 8000, 4200]], np.int32)
    tris = np.array([[0, 1, 2]], np.int32)
    for cull, low_x in (("none", False), ("none", True)):
        _, ids, _ = against_twin([(q, tris)], None, [(np.pi / 2, 0.0, 1.0)], 32, 32, 8, window=(96, 90, 64, 64), cull=cull,
                                 low_x=low_x, min_hits=4096)
        assert (ids == 0).all()


def test_sub_pixel_triangles():
    """4 096 triangles smaller than a pixel (64 lattice units at f = 4): most cover no centre, none more than one."""
    rng = np.random.RandomState(5)
    centre = rng.randint(6 * 256, 26 * 256, (4096, 1, 3))
    q = (centre + rng.randint(-18, 19, (4096, 3, 3))).reshape(-1, 3).astype(np.int32)
    tris = np.arange(3 * 4096, dtype=np.int32).reshape(-1, 3)
    _, ids, _ = against_twin([(q, tris)], None, POSES32[:2], 32, 32, 4, cull="none", min_hits=30)
    assert np.bincount(ids[ids >= 0]).max() <= 2


def test_vertices_outside_the_frame_and_ragged_windows():
    """Scale 2.5 pushes the corners of lattice-spanning triangles left of, above, right of and below the 128^2 frame; windows
    whose sides are no multiple of 8 or 16, one at each side of the frame and one in its corner, cut the triangles."""
    from rendernet_amd import ops
    S = N = 32
    q = np.array([[0, 0, 4096], [8192, 0, 3000], [8192, 8192, 5000], [0, 8192, 4500], [4096, 4096, 0], [4096, 4096, 8192]], np.int32)
    tris = np.array([[0, 1, 2], [0, 2, 3], [4, 1, 5], [3, 5, 4]], np.int32)
    pose = [(0.4, 0.3, 2.5)]
    cam = ops.mesh_camera(_dev(np.asarray(pose, np.float32)), S, new_size=N, pixels_per_cell=4).cpu().numpy()[0]
    P = MR.project(cam, q, S)
    assert P[:, 0].min() < 0 and P[:, 1].min() < 0 and P[:, 0].max() > 256 * 128 and P[:, 1].max() > 256 * 128
    for window in (None, (0, 0, 37, 21), (91, 0, 37, 53), (0, 75, 45, 53), (13, 29, 99, 70), (127, 127, 1, 1)):
        against_twin([(q, tris)], None, pose, S, N, 4, window=window, smooth=False, cull="none",
                     min_hits=1 if window is None or window[2] > 1 else 0)


def test_degenerate_triangles_draw_nothing():
    """Repeated vertices, collinear corners and a triangle seen edge-on, next to one that draws."""
    q = np.array([[1000, 1000, 4000], [5000, 1200, 4000], [3000, 6000, 4100], [3000, 3600, 4050], [5000, 6200, 4100],
                  [2000, 2000, 1000], [2000, 2000, 7000], [2000, 6000, 4000]], np.int32)
    tris = np.array([[0, 0, 1], [1, 1, 1], [0, 3, 4], [0, 1, 2], [2, 1, 2], [5, 6, 7]], np.int32)
    assert (MR.face_normals(q, tris, 32)[[0, 1, 4]] == 0).all()
    _, ids, _ = against_twin([(q, tris)], None, [(np.pi / 2, 0.0, 1.0)], 32, 32, 4, cull="none", min_hits=500)
    assert set(np.unique(ids)) <= {-1, 3}                     # [5, 6, 7] lies in a plane through the view direction


def test_empty_input(sphere):
    import torch
    from rendernet_amd import ops
    q, tris = sphere
    pose = _dev(np.asarray(POSES32, np.float32))
    none = torch.zeros((0, 3), dtype=torch.int32, device="cuda")
    for qq, tt in ((_dev(q), none), (none, none)):
        rgb, ids, depth = ops.rasterize_mesh(qq, tt, pose, 32, new_size=32, window=(3, 5, 50, 41), return_ids=True)
        assert rgb.shape == (3, 50, 41, 3) and (rgb == 0).all() and (ids == -1).all() and (depth == -1).all()
    rgb, ids, depth = ops.rasterize_mesh(_dev(q), _dev(tris), pose[:0], 32, new_size=32, return_ids=True)
    assert rgb.shape == (0, 128, 128, 3) and ids.shape == (0, 128, 128) and depth.shape == (0, 128, 128)
    assert ops.rasterize_mesh(_dev(q), _dev(tris), pose[:0], 32, new_size=32).shape == (0, 128, 128, 3)


def test_two_meshes_three_items(sphere):
    box = box_mesh((5 * 256 + 17, 7 * 256 + 128, 9 * 256 + 1), (20 * 256 + 128, 19 * 256 + 250, 22 * 256 + 99))
    for smooth in (True, False):
        against_twin([box, sphere], [1, 0, 1], POSES32, 32, 32, 4, smooth=smooth, min_hits=9000)


def test_stray_indices_are_clamped(sphere):
    """Indices far outside the mesh neither fault nor disturb the picture: the kernel clamps them into the mesh, as the twin
    does, and with the strays at the end of the list every other triangle keeps its id."""
    q, tris = sphere
    stray = np.array([[2 ** 31 - 1, 5, 9], [-7, -2 ** 31, 3], [len(q), len(q) + 1, len(q) + 2]], np.int32)
    rgb, ids, depth = against_twin([(q, np.concatenate([tris, stray]))], None, POSES32[:1], 32, 32, 4, smooth=False, min_hits=3000)
    clean = against_twin([(q, tris)], None, POSES32[:1], 32, 32, 4, smooth=False, min_hits=3000)
    same = ids < len(tris)
    assert same.mean() > 0.95
    assert np.array_equal(ids[same], clean[1][same]) and np.array_equal(depth[same], clean[2][same])
    assert np.array_equal(rgb[same], clean[0][same])


def test_two_runs_give_identical_bits(sphere):
    from rendernet_amd import ops
    q, tris = _dev(sphere[0]), _dev(sphere[1])
    pose = _dev(np.asarray(POSES32, np.float32))
    for smooth, cull in ((True, "back"), (False, "none")):
        a = ops.rasterize_mesh(q, tris, pose, 32, new_size=32, smooth=smooth, cull=cull, return_ids=True)
        b = ops.rasterize_mesh(q, tris, pose, 32, new_size=32, smooth=smooth, cull=cull, return_ids=True)
        assert all(bool((x == y).all()) for x, y in zip(a, b))
        assert bool((a[0] == ops.rasterize_mesh(q, tris, pose, 32, new_size=32, smooth=smooth, cull=cull)).all())
    vn = ops.mesh_vertex_normals(q, tris, 32)
    assert bool((ops.rasterize_mesh(q, tris, pose, 32, new_size=32, vertex_normals=vn)
                 == ops.rasterize_mesh(q, tris, pose, 32, new_size=32)).all())


def test_arguments_are_checked_before_launch(sphere):
    import torch
    from rendernet_amd import ops
    from rendernet_amd._lib import RenderNetHipError
    q, tris = _dev(sphere[0]), _dev(sphere[1])
    pose = _dev(np.asarray(POSES32, np.float32))
    i64 = lambda *v: torch.tensor(v, dtype=torch.int64, device="cuda")
    bad = [dict(S=48), dict(cull="front"), dict(smooth=1), dict(window=(0, 0, 129, 10)), dict(window=(-1, 0, 10, 10)),
           dict(window=(0, 0, 0, 10)), dict(new_size=512), dict(pixels_per_cell=17), dict(new_size=256, pixels_per_cell=16),
           dict(vert_offsets=i64(0, len(sphere[0]))), dict(vert_offsets=i64(0, 5), tri_offsets=i64(0, len(sphere[1]))),
           dict(vert_offsets=i64(0, 0, len(sphere[0])), tri_offsets=i64(0, 3, len(sphere[1])),
                mesh_of_item=torch.zeros(3, dtype=torch.int32, device="cuda")),
           dict(vert_offsets=i64(0, 9, len(sphere[0])), tri_offsets=i64(0, 3, len(sphere[1]))),
           dict(vert_offsets=i64(0, 9, len(sphere[0])), tri_offsets=i64(0, 3, len(sphere[1])),
                mesh_of_item=torch.tensor([0, 2, 1], dtype=torch.int32, device="cuda")),
           dict(mesh_of_item=torch.zeros(2, dtype=torch.int32, device="cuda")),
           dict(vertex_normals=torch.zeros((5, 3), dtype=torch.int64, device="cuda"))]
    for kw in bad:
        args = dict(S=32, new_size=32)
        args.update(kw)
        S = args.pop("S")
        with pytest.raises(RenderNetHipError):
            ops.rasterize_mesh(q, tris, pose, S, **args)
    for qq, tt, pp in ((q.float(), tris, pose), (q, tris.long(), pose), (q[:, :2], tris, pose), (q.cpu(), tris, pose),
                       (q, tris, pose[:, :2]), (q[:0], tris, pose)):
        with pytest.raises(RenderNetHipError):
            ops.rasterize_mesh(qq, tt, pp, 32, new_size=32)
    with pytest.raises(RenderNetHipError):
        ops.rasterize_mesh(q, tris, pose, 32, new_size=32, affine=True)
