"""rn_mesh_colour_from_ids / rn_mesh_face_voxels on the device against the NumPy twin (tests/mesh_colour_ref.py): every byte of
every pixel and every id of every face, with the twin fed the device's integer camera as in tests/test_gpu_mesh_raster.py;
interpolated and flat colours, both cull modes, windows, degenerate and stray input, several meshes, empty input, determinism,
the argument checks, and the round trip against the coloured-grid caster on a shipped model.  -m gpu."""
import os

import numpy as np
import pytest

import mesh_colour_ref as MC
import mesh_extract_ref as XR
import mesh_raster_ref as MR
import mesh_relax_ref as MX
from conftest import BINVOX_DIR

pytestmark = pytest.mark.gpu
POSES32 = ((4.36, 0.52, 1.0), (0.3, 1.2, 0.9), (2.0, 2.6, 0.8))


def _dev(a, dtype=None):
    import torch
    t = torch.as_tensor(np.ascontiguousarray(a))
    return (t if dtype is None else t.to(dtype)).cuda()


@pytest.fixture(scope="module")
def sphere():
    """The sphere net of 32^3 relaxed 4 passes, as a fan."""
    vol, thr = XR.cases32()["sphere"]
    q, faces = XR.extract(vol, thr, smooth=True)
    return MX.relax(q, faces, 32, 4).astype(np.int32), XR.fan(faces).astype(np.int32)


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


def colours_of(meshes, per_face, seed):
    rng = np.random.RandomState(seed)
    return [rng.randint(0, 256, (len(t) if per_face else len(q), 3)).astype(np.uint8) for q, t in meshes]


def against_twin(meshes, mesh_of_item, poses, S, N, f, per_face, window=None, cull="back", low_x=False, min_hits=1, seed=1,
                 background=(3, 250, 77)):
    """meshes: [(q, tris)]; one rasterize_mesh_colour call over the batch against the twin per item -- the twin's own raster pass
    on the device's camera, then its colour resolve.  Returns the device's (colour, ids)."""
    import torch
    from rendernet_amd import ops
    cols = colours_of(meshes, per_face, seed)
    vo = np.cumsum([0] + [len(q) for q, _ in meshes]).astype(np.int64)
    to = np.cumsum([0] + [len(t) for _, t in meshes]).astype(np.int64)
    q = np.concatenate([q for q, _ in meshes]).astype(np.int32).reshape(-1, 3)
    tris = np.concatenate([t for _, t in meshes]).astype(np.int32).reshape(-1, 3)
    pose = _dev(np.asarray(poses, np.float32).reshape(-1, 3))
    B = int(pose.shape[0])
    m_inv = ops.pose_to_affine(pose, S, N)
    kw = dict(new_size=N, pixels_per_cell=f, affine=True, view_from_low_x=low_x)
    many = len(meshes) > 1 or mesh_of_item is not None
    sets = dict(vert_offsets=_dev(vo), tri_offsets=_dev(to),
                mesh_of_item=_dev(np.asarray(mesh_of_item if mesh_of_item is not None else [0] * B, np.int32))) if many else {}
    colour = {"face_colours" if per_face else "vertex_colours": _dev(np.concatenate(cols))}
    rgb, ids, depth = ops.rasterize_mesh_colour(_dev(q), _dev(tris), m_inv, S, window=window, cull=cull, background=background,
                                                return_ids=True, **colour, **sets, **kw)
    again = ops.rasterize_mesh_colour(_dev(q), _dev(tris), m_inv, S, window=window, cull=cull, background=background,
                                      **colour, **sets, **kw)
    assert torch.equal(rgb, again)                               # two calls: identical bits
    cam = ops.mesh_camera(m_inv, S, **kw).cpu().numpy()
    rgb, ids, M = rgb.cpu().numpy(), ids.cpu().numpy(), m_inv.cpu().numpy()
    win = window if window is not None else (0, 0, f * N, f * N)
    assert rgb.dtype == np.uint8 and rgb.shape == (B, win[2], win[3], 3)
    hits = 0
    for b in range(B):
        k = mesh_of_item[b] if mesh_of_item is not None else 0
        mq, mt = meshes[k]
        _, w_ids, _, _ = MR.rasterize(mq, mt, cam[b], M[b], S, N, f, window, False, cull, low_x)
        assert np.array_equal(ids[b], w_ids), (b, int((ids[b] != w_ids).sum()))
        want = MC.colour_from_ids(mq, mt, cam[b], w_ids, S, win, background=background,
                                  **{"face_colours" if per_face else "vertex_colours": cols[k]})
        bad = (rgb[b] != want).any(2)
        assert not bad.any(), (b, int(bad.sum()), np.argwhere(bad)[:3], rgb[b][bad][:3], want[bad][:3])
        hits += int((ids[b] >= 0).sum())
    assert hits >= min_hits, hits
    return rgb, ids


@pytest.mark.parametrize("cull", ["back", "none"])
@pytest.mark.parametrize("per_face", [False, True])
def test_relaxed_sphere_net_at_three_poses(sphere, per_face, cull):
    """About 5 000 triangles of a few pixels each, three items in one call, then the view from low x."""
    assert 4000 < len(sphere[1]) < 8000
    against_twin([sphere], None, POSES32, 32, 32, 4, per_face, cull=cull, min_hits=9000)
    against_twin([sphere], None, POSES32[:1], 32, 32, 4, per_face, cull=cull, low_x=True, min_hits=3000, seed=2)


@pytest.mark.parametrize("per_face", [False, True])
def test_a_ragged_window(sphere, per_face):
    """row0, col0 != 0, pw = 45 no multiple of 64, ph pw = 1 665 no multiple of the 256-thread workgroup."""
    against_twin([sphere], None, POSES32[:2], 32, 32, 4, per_face, window=(41, 39, 37, 45), min_hits=2000)


def test_one_triangle_over_a_whole_window():
    """A 64 x 64 window inside one triangle, seen from either side: 4 096 interpolated pixels of one triangle."""
    q = np.array([[200, 300, 4000], [8000, 250, 4100], [4000, 8000, 4200]], np.int32)
    tris = np.array([[0, 1, 2]], np.int32)
    for low_x in (False, True):
        rgb, ids = against_twin([(q, tris)], None, [(np.pi / 2, 0.0, 1.0)], 32, 32, 8, False, window=(96, 90, 64, 64), cull="none",
                                low_x=low_x, min_hits=4096)
        assert (ids == 0).all() and len(np.unique(rgb.reshape(-1, 3), axis=0)) > 500


def test_sub_pixel_triangles():
    """4 096 triangles smaller than a pixel: at most a pixel or two each, weights anywhere in the triangle."""
    rng = np.random.RandomState(5)
    centre = rng.randint(6 * 256, 26 * 256, (4096, 1, 3))
    q = (centre + rng.randint(-18, 19, (4096, 3, 3))).reshape(-1, 3).astype(np.int32)
    tris = np.arange(3 * 4096, dtype=np.int32).reshape(-1, 3)
    against_twin([(q, tris)], None, POSES32[:2], 32, 32, 4, False, cull="none", min_hits=30)


def test_vertices_outside_the_frame():
    """A box of three quarters of the grid under a camera that enlarges it: six of its eight projected vertices lie left of, above
    or beyond the 128 x 128 frame, the near plane cuts it, and the triangles that cover the frame are far larger than it."""
    q, tris = box_mesh((1024, 1024, 1024), (7168, 7168, 7168))
    pose = (0.7, 0.4, 1.3)
    from rendernet_amd import ops
    m_inv = ops.pose_to_affine(_dev(np.asarray([pose], np.float32)), 32, 32)
    cam = ops.mesh_camera(m_inv, 32, new_size=32, pixels_per_cell=4, affine=True).cpu().numpy()[0]
    P = MR.project(cam, q, 32)
    assert ((P[:, :2] < 0) | (P[:, :2] > 256 * 128)).any(1).sum() >= 4
    for cull in ("back", "none"):
        against_twin([(q, tris)], None, [pose], 32, 32, 4, False, cull=cull, min_hits=10000)


@pytest.mark.parametrize("per_face", [False, True])
def test_two_meshes_three_items(sphere, per_face):
    box = box_mesh((300, 700, 900), (5000, 6000, 7000))
    against_twin([box, sphere], [1, 0, 1], POSES32, 32, 32, 4, per_face, min_hits=9000)


def test_from_ids_equals_the_one_pass_form_and_normals_are_the_rasterisers(sphere):
    """mesh_colour_from_ids on the ids rasterize_mesh returned = rasterize_mesh_colour; with return_normals the same pass also
    gives rasterize_mesh's bytes, ids and depths, smooth and flat."""
    import torch
    from rendernet_amd import ops
    q, tris = _dev(sphere[0]), _dev(sphere[1])
    pose = _dev(np.asarray(POSES32, np.float32))
    vcol = _dev(colours_of([sphere], False, 7)[0])
    fcol = _dev(colours_of([sphere], True, 8)[0])
    for smooth, low_x, window in ((True, False, None), (False, True, (10, 20, 70, 90))):
        kw = dict(new_size=32, pixels_per_cell=4, window=window, view_from_low_x=low_x)
        normals, ids, depth = ops.rasterize_mesh(q, tris, pose, 32, smooth=smooth, cull="none", return_ids=True, **kw)
        for colour in (dict(vertex_colours=vcol), dict(face_colours=fcol)):
            one = ops.rasterize_mesh_colour(q, tris, pose, 32, smooth=smooth, cull="none", return_normals=True, return_ids=True,
                                            background=(5, 6, 7), **colour, **kw)
            assert len(one) == 4
            assert torch.equal(one[1], normals) and torch.equal(one[2], ids) and torch.equal(one[3], depth)
            two = ops.mesh_colour_from_ids(ids, q, tris, pose, 32, background=(5, 6, 7), **colour, **kw)
            assert torch.equal(one[0], two) and two.dtype is torch.uint8
            pair = ops.rasterize_mesh_colour(q, tris, pose, 32, cull="none", return_normals=True, smooth=smooth,
                                             background=(5, 6, 7), **colour, **kw)
            assert len(pair) == 2 and torch.equal(pair[0], two) and torch.equal(pair[1], normals)
        assert (ids >= 0).sum() > 5000


def test_any_int32_is_a_triangle_id():
    """Ids the rasteriser never wrote: negative ones, INT_MIN, ids past the mesh's count, INT_MAX (background), ids of triangles
    that do not cover the pixel (the rule, clamped to 0..255) and of triangles without area (the mean)."""
    from rendernet_amd import ops
    S, N, f = 32, 32, 4
    rng = np.random.RandomState(9)
    q = np.array([[500, 600, 4000], [7000, 900, 4100], [4000, 7500, 4200], [2000, 2000, 3000], [4000, 4000, 3000],
                  [6000, 6000, 3000]], np.int32)
    tris = np.array([[0, 1, 2], [0, 2, 1], [3, 4, 5], [1, 1, 1], [2, 5, 0], [0, 0, 4], [9, -3, 2]], np.int32)     # 2: a line; 3, 5: a point, a segment
    T = len(tris)
    window = (16, 8, 50, 70)
    ids = rng.randint(-3, T + 3, (2, 50, 70)).astype(np.int32)
    ids[0, 0, :4] = [np.iinfo(np.int32).min, np.iinfo(np.int32).max, T, -1]
    vcol = rng.randint(0, 256, (len(q), 3)).astype(np.uint8)
    vcol[0], vcol[1] = (255, 0, 255), (0, 255, 0)
    fcol = rng.randint(0, 256, (T, 3)).astype(np.uint8)
    pose = _dev(np.asarray(POSES32[:2], np.float32))
    m_inv = ops.pose_to_affine(pose, S, N)
    cam = ops.mesh_camera(m_inv, S, new_size=N, pixels_per_cell=f, affine=True).cpu().numpy()
    for colour, name in ((vcol, "vertex_colours"), (fcol, "face_colours")):
        got = ops.mesh_colour_from_ids(_dev(ids), _dev(q), _dev(tris), m_inv, S, new_size=N, pixels_per_cell=f, window=window,
                                       affine=True, background=(1, 2, 3), **{name: _dev(colour)}).cpu().numpy()
        for b in range(2):
            want = MC.colour_from_ids(q, tris, cam[b], ids[b], S, window, background=(1, 2, 3), **{name: colour})
            assert np.array_equal(got[b], want), (name, b, np.argwhere((got[b] != want).any(2))[:3])
        assert (got[0, 0, :4] == np.array([1, 2, 3], np.uint8)).all()


@pytest.mark.parametrize("as_u8", [False, True])
@pytest.mark.parametrize("triangles", [False, True])
def test_face_voxels_equal_the_twin(triangles, as_u8):
    """B = 3 -- sphere, empty grid, full grid at 32^3 -- smooth, blocky and relaxed, on the meshes the device extracted."""
    import torch
    from rendernet_amd import ops
    S = 32
    field, thr = XR.cases32()["sphere"]
    vol = np.stack([field, np.zeros((S, S, S), np.float32), np.ones((S, S, S), np.float32)])
    if as_u8:
        vol = (vol > np.float32(thr)).astype(np.uint8)
    dvol = _dev(vol)[..., None]
    for smooth, relax in ((True, 0), (False, 0), (True, 4)):
        mesh = ops.extract_mesh(dvol, threshold=thr, smooth=smooth, triangles=triangles, relax=relax)
        got = ops.mesh_face_voxels(mesh, dvol, threshold=thr)
        assert got.dtype is torch.int32 and tuple(got.shape) == (int(mesh.faces.shape[0]),)
        assert torch.equal(got, ops.mesh_face_voxels(mesh, dvol[..., 0], threshold=thr))
        vo, fo = mesh.vert_offsets.cpu().numpy(), mesh.face_offsets.cpu().numpy()
        want = MC.face_voxels_batch(mesh.q.cpu().numpy(), mesh.faces.cpu().numpy(), vo, fo, vol, thr)
        got = got.cpu().numpy()
        assert np.array_equal(got, want) and (got >= 0).all()
        assert fo[2] == fo[1] and fo[3] - fo[2] == 6 * S * S * (2 if triangles else 1)
        # a mesh that is not this grid's: the sphere's faces against the empty grid, and against the full one
        swapped = ops.mesh_face_voxels(mesh, _dev(vol[[1, 1, 0]])[..., None], threshold=thr).cpu().numpy()
        assert np.array_equal(swapped, MC.face_voxels_batch(mesh.q.cpu().numpy(), mesh.faces.cpu().numpy(), vo, fo, vol[[1, 1, 0]], thr))
        assert (swapped[:fo[1]] == -1).all()


def test_face_colours_gather():
    import torch
    from rendernet_amd import ops
    S = 32
    field, thr = XR.cases32()["sphere"]
    vol = _dev(np.stack([field, np.ones((S, S, S), np.float32)]))[..., None]
    rng = np.random.RandomState(12)
    colours = rng.randint(0, 256, (2, S, S, S, 3)).astype(np.uint8)
    known = (rng.rand(2, S, S, S) < 0.7).astype(np.uint8)
    mesh = ops.extract_mesh(vol, threshold=thr, smooth=False, triangles=True)
    ids = ops.mesh_face_voxels(mesh, vol, threshold=thr).cpu().numpy().astype(np.int64)
    grid = np.searchsorted(mesh.face_offsets.cpu().numpy()[1:], np.arange(len(ids)), side="right")
    flat = grid * S ** 3 + ids
    got = ops.mesh_face_colours(mesh, vol, _dev(colours), threshold=thr).cpu().numpy()
    assert np.array_equal(got, colours.reshape(-1, 3)[flat])
    got = ops.mesh_face_colours(mesh, vol, _dev(colours), _dev(known), threshold=thr, unseen=(1, 2, 3)).cpu().numpy()
    want = np.where(known.reshape(-1)[flat][:, None] != 0, colours.reshape(-1, 3)[flat], np.array([1, 2, 3], np.uint8))
    assert np.array_equal(got, want) and (known.reshape(-1)[flat] == 0).sum() > 100
    none = ops.mesh_face_colours(mesh, torch.zeros_like(vol), _dev(colours), threshold=thr).cpu().numpy()
    assert (none == 128).all()


def test_empty_inputs(sphere):
    import torch
    from rendernet_amd import ops
    q, tris = _dev(sphere[0]), _dev(sphere[1])
    vcol = _dev(colours_of([sphere], False, 1)[0])
    none = torch.zeros((0, 3), dtype=torch.float32, device="cuda")
    out = ops.rasterize_mesh_colour(q, tris, none, 32, new_size=32, vertex_colours=vcol, return_ids=True)
    assert tuple(out[0].shape) == (0, 128, 128, 3) and tuple(out[1].shape) == (0, 128, 128)
    assert tuple(ops.mesh_colour_from_ids(out[1], q, tris, none, 32, new_size=32, vertex_colours=vcol).shape) == (0, 128, 128, 3)
    pose = _dev(np.asarray(POSES32[:2], np.float32))
    e3 = torch.zeros((0, 3), dtype=torch.int32, device="cuda")
    c0 = torch.zeros((0, 3), dtype=torch.uint8, device="cuda")
    ids = torch.zeros((2, 128, 128), dtype=torch.int32, device="cuda")
    for qq, vc in ((q, vcol), (e3, c0)):                         # T = 0, then V = 0 as well
        for colour in (dict(vertex_colours=vc), dict(face_colours=c0)):
            got = ops.rasterize_mesh_colour(qq, e3, pose, 32, new_size=32, background=(4, 5, 6), **colour)
            assert (got.cpu().numpy() == np.array([4, 5, 6], np.uint8)).all()
            got = ops.mesh_colour_from_ids(ids, qq, e3, pose, 32, new_size=32, background=(4, 5, 6), **colour)
            assert (got.cpu().numpy() == np.array([4, 5, 6], np.uint8)).all()
    empty = ops.extract_mesh(torch.zeros((2, 32, 32, 32, 1), device="cuda"))
    assert tuple(ops.mesh_face_voxels(empty, torch.zeros((2, 32, 32, 32, 1), device="cuda")).shape) == (0,)
    nothing = ops.extract_mesh(torch.zeros((0, 32, 32, 32, 1), device="cuda"))
    assert tuple(ops.mesh_face_voxels(nothing, torch.zeros((0, 32, 32, 32, 1), device="cuda")).shape) == (0,)
    assert tuple(ops.mesh_face_colours(nothing, torch.zeros((0, 32, 32, 32, 1), device="cuda"),
                                       torch.zeros((0, 32, 32, 32, 3), dtype=torch.uint8, device="cuda")).shape) == (0, 3)


def test_argument_checks_raise_before_a_launch(sphere):
    import torch
    from rendernet_amd import ops
    from rendernet_amd._lib import RenderNetHipError as Err
    q, tris = _dev(sphere[0]), _dev(sphere[1])
    V, T = int(q.shape[0]), int(tris.shape[0])
    vcol, fcol = _dev(colours_of([sphere], False, 1)[0]), _dev(colours_of([sphere], True, 1)[0])
    pose = _dev(np.asarray(POSES32[:1], np.float32))
    ids = torch.zeros((1, 128, 128), dtype=torch.int32, device="cuda")

    def draw(**kw):
        a = dict(new_size=32, vertex_colours=vcol)
        a.update(kw)
        return ops.rasterize_mesh_colour(q, tris, pose, 32, **a)

    def resolve(i=ids, **kw):
        a = dict(new_size=32, vertex_colours=vcol)
        a.update(kw)
        return ops.mesh_colour_from_ids(i, q, tris, pose, 32, **a)
    for call, name in ((draw, "rasterize_mesh_colour"), (resolve, "mesh_colour_from_ids")):
        for bad in (dict(vertex_colours=None), dict(face_colours=fcol), dict(vertex_colours=vcol[:-1]),
                    dict(vertex_colours=None, face_colours=fcol[:-1]), dict(vertex_colours=None, face_colours=vcol),
                    dict(vertex_colours=vcol.int()), dict(vertex_colours=vcol.cpu()), dict(vertex_colours=vcol.reshape(-1)),
                    dict(vertex_colours=vcol.cpu().numpy()), dict(background=(0, 0, 256)), dict(background=(0, 0)),
                    dict(window=(0, 0, 129, 128)), dict(window=(100, 0, 64, 64)), dict(pixels_per_cell=17), dict(new_size=257),
                    dict(mesh_of_item=torch.zeros((2,), dtype=torch.int32, device="cuda")),
                    dict(vert_offsets=torch.tensor([0, V], device="cuda"))):
            with pytest.raises(Err, match=name):
                call(**bad)
    for bad in (dict(cull="front"), dict(return_normals=1), dict(smooth=None, return_normals=True),
                dict(vertex_normals=torch.zeros((V, 3), device="cuda"))):
        with pytest.raises(Err, match="rasterize_mesh_colour"):
            draw(**bad)
    for bad_ids in (ids.long(), ids[:, :100], ids.cpu(), None, torch.zeros((2, 128, 128), dtype=torch.int32, device="cuda")):
        with pytest.raises(Err, match="mesh_colour_from_ids"):
            resolve(bad_ids)
    vol = torch.zeros((1, 32, 32, 32, 1), device="cuda")
    mesh = ops.extract_mesh(_dev(XR.cases32()["sphere"][0])[None, ..., None])
    colours = torch.zeros((1, 32, 32, 32, 3), dtype=torch.uint8, device="cuda")
    for bad in ((None, vol), (mesh, None), (mesh, vol.double()), (mesh, vol.cpu()), (mesh, vol[:, :16]), (mesh, torch.cat([vol, vol])),
                (ops.ExtractedMesh(mesh.q.long(), mesh.faces, mesh.vert_offsets, mesh.face_offsets), vol),
                (ops.ExtractedMesh(mesh.q, mesh.faces[:, :2], mesh.vert_offsets, mesh.face_offsets), vol),
                (ops.ExtractedMesh(mesh.q, mesh.faces, mesh.vert_offsets.int(), mesh.face_offsets), vol),
                (ops.ExtractedMesh(mesh.q.cpu(), mesh.faces, mesh.vert_offsets, mesh.face_offsets), vol)):
        with pytest.raises(Err, match="mesh_face_voxels"):
            ops.mesh_face_voxels(*bad)
    with pytest.raises(Err, match="mesh_face_voxels"):
        ops.mesh_face_voxels(mesh, vol, threshold=float("nan"))
    for bad in (dict(colours=colours.int()), dict(colours=colours[:, :16]), dict(known=colours), dict(unseen=(0, 0, 300)),
                dict(colours=torch.cat([colours, colours]))):
        a = dict(colours=colours)
        a.update(bad)
        with pytest.raises(Err, match="mesh_face_colours"):
            ops.mesh_face_colours(mesh, vol, **a)


def test_c_entries_refuse_bad_arguments():
    """The C checks behind the Python ones, on the limits Python cannot reach: NULL colour pointers, both colour pointers, width."""
    import ctypes
    import torch
    from rendernet_amd import _lib as L
    lib = L.lib()
    z = torch.zeros((64,), dtype=torch.int64, device="cuda")
    p, nul, st = ctypes.c_void_p(z.data_ptr()), None, L.stream_ptr()

    def colour(vcol=p, fcol=nul, B=1, S=32, N=32, f=4, win=(0, 0, 2, 2), M=1, V=3, T=1, bg=(0, 0, 0)):
        return lib.rn_mesh_colour_from_ids(p, V, p, T, p, p, M, p, p, p, vcol, fcol, p, B, S, N, f, win[0], win[1], win[2], win[3], 0,
                                           bg[0], bg[1], bg[2], st)
    assert colour(B=0) == 0
    for bad in (dict(vcol=nul), dict(fcol=p), dict(B=-1), dict(B=65536), dict(S=48), dict(N=257), dict(f=17), dict(win=(0, 0, 0, 2)),
                dict(win=(127, 0, 2, 2)), dict(M=0), dict(V=-1), dict(T=(1 << 28) + 1), dict(V=0), dict(bg=(0, -1, 0)), dict(bg=(256, 0, 0))):
        assert colour(**bad) != 0, bad
        assert b"rn_mesh_colour_from_ids" in lib.rn_last_error()

    def voxels(B=1, S=32, V=3, F=1, width=4, u8=0, thr=0.5, verts=p, out=p):
        return lib.rn_mesh_face_voxels(verts, V, p, p, F, width, p, p, u8, thr, out, B, S, st)
    assert voxels(B=0, F=0) == 0 and voxels(F=0) == 0
    for bad in (dict(B=-1), dict(B=65536), dict(S=96), dict(V=-1), dict(F=-1), dict(F=(1 << 28) + 1), dict(width=5), dict(width=2),
                dict(u8=2), dict(thr=float("nan")), dict(B=0), dict(verts=nul), dict(out=nul)):
        assert voxels(**bad) != 0, bad
        assert b"rn_mesh_face_voxels" in lib.rn_last_error()
    torch.cuda.synchronize()


def test_round_trip_against_the_coloured_grid_caster():
    """A shipped model max-pooled to 32^3 with random voxel colours: the blocky fan drawn with mesh_face_colours shows, wherever
    the face it shows belongs to the voxel the caster's ray hit, that voxel's bytes -- on more than half of the hit pixels (a
    sanity condition: the CPU cross-check establishes >= 99.5 %)."""
    import torch
    from oracle.io_phong import read_binvox
    from rendernet_amd import ops
    S = 32
    occ = read_binvox(os.path.join(BINVOX_DIR, "teapot.binvox")).astype(np.uint8).reshape(S, 2, S, 2, S, 2).max((1, 3, 5))
    vol = _dev(occ)[None, ..., None]
    colours = _dev(np.random.RandomState(21).randint(1, 256, (1, S, S, S, 3)).astype(np.uint8))
    mesh = ops.extract_mesh(vol, smooth=False, triangles=True)
    voxel = ops.mesh_face_voxels(mesh, vol)
    fcol = ops.mesh_face_colours(mesh, vol, colours)
    assert torch.equal(fcol, colours.reshape(-1, 3)[voxel.long()])
    pose = _dev(np.asarray(POSES32[:1], np.float32))
    kw = dict(new_size=S, pixels_per_cell=4)
    picture, tri_id, _ = ops.rasterize_mesh_colour(mesh.q, mesh.faces, pose, S, face_colours=fcol, return_ids=True, **kw)
    cast, hit = ops.raycast_colour(vol.float(), colours, pose, smooth=0, return_hits=True, **kw)
    seen = torch.where(tri_id >= 0, voxel[tri_id.clamp(min=0).long()], torch.full_like(tri_id, -1))
    same = (seen == hit) & (hit >= 0)
    assert torch.equal(picture[same], cast[same])
    share = float(same.sum()) / float((hit >= 0).sum())
    print("the mesh shows the caster's voxel on %.2f %% of %d hit pixels" % (100 * share, int((hit >= 0).sum())))
    assert (hit >= 0).sum() > 1000 and share > 0.5
