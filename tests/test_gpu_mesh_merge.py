"""rn_mesh_merge_count / _emit on the device against the NumPy twin (tests/mesh_merge_ref.py): every array of
ops.extract_mesh_merged exactly, order included, on the fields of the round-trip tests, the geometry edges of the rule, the row
words of 64^3 and 128^3 and labelled grids; the solid round trip through the device voxeliser; the colour gather."""
import numpy as np
import pytest
import torch

import mesh_merge_ref as M

pytestmark = pytest.mark.gpu
S = 32
NAMES = ("q", "faces", "vert_offsets", "face_offsets", "face_voxel", "face_dir", "face_size")
PINNED = {"sphere": (1189, 1511), "full": (6, 8), "binary_u8": (32989, 30957), "uniform_noise": (33702, 31584),
          "threshold_ties": (31333, 30012), "edge_contact": (12, 14), "grid_corners": (12, 16)}


def _arrays(mesh):
    return [getattr(mesh, n).cpu().numpy() for n in NAMES]


def _same(mesh, want, what):
    for name, got, ref in zip(NAMES, _arrays(mesh), want):
        assert got.dtype == ref.dtype and got.shape == ref.shape, (what, name, got.dtype, got.shape, ref.dtype, ref.shape)
        assert np.array_equal(got, ref), (what, name, int((got != ref).sum()))


def _check(vol, thr=0.5, labels=None):
    from rendernet_amd import ops
    vol = np.asarray(vol)
    dev_vol = torch.as_tensor(vol).cuda()
    dev_lab = None if labels is None else torch.as_tensor(np.asarray(labels, np.int32)).cuda()
    out = None
    for tri in (False, True):
        mesh = ops.extract_mesh_merged(dev_vol, thr, labels=dev_lab, triangles=tri)
        _same(mesh, M.merge_batch(vol, thr, labels, triangles=tri), "triangles=%s" % tri)
        out = out or mesh
    return out


@pytest.mark.parametrize("name", sorted(M.cases32()))
def test_cases32_equal_the_twin_in_float32_and_uint8(name):
    vol, thr = M.cases32()[name]
    mesh = _check(vol[None], thr)
    assert (int(mesh.faces.shape[0]), int(mesh.q.shape[0])) == PINNED[name]
    if vol.dtype != np.uint8:
        _check((vol.astype(np.float32) > np.float32(thr)).astype(np.uint8)[None], 0.5)
    else:
        _check(vol.astype(np.float32)[None], thr)


def test_the_chair_has_the_pinned_counts(fixtures_vox):
    from rendernet_amd import ops
    mesh = ops.extract_mesh_merged(torch.as_tensor(fixtures_vox[:1]).cuda())
    assert (int(mesh.faces.shape[0]), int(mesh.q.shape[0])) == (831, 1180)
    _same(mesh, M.merge_batch(fixtures_vox[:1]), "chair")
    assert int(mesh.face_size.long().prod(1).sum()) == 6780                   # the unit quads of the blocky mesh


def test_a_batch_with_an_empty_grid_in_the_middle():
    cases = M.cases32()
    vol = np.stack([cases["sphere"][0], np.zeros((S, S, S), np.float32), cases["edge_contact"][0], cases["full"][0]])
    mesh = _check(vol, 0.5)
    assert mesh.vert_offsets.tolist()[1] == mesh.vert_offsets.tolist()[2]
    q, faces = mesh.grid(2)
    assert tuple(q.shape) == (14, 3) and tuple(faces.shape) == (12, 4)


@pytest.mark.parametrize("name", sorted(M.edge_cases()))
def test_the_geometry_edges(name):
    vol, thr = M.edge_cases()[name]
    _check(vol[None], thr)
    _check(np.ascontiguousarray(vol.transpose(2, 0, 1))[None], thr)           # the same shapes seen along the other axes
    _check(np.ascontiguousarray(vol.transpose(1, 2, 0))[None], thr)


@pytest.mark.parametrize("name", sorted(M.word_cases()))
def test_the_row_words_of_64_and_128(name):
    vol, side = M.word_cases()[name]
    mesh = _check(vol[None])
    assert int(mesh.face_size.max()) == side                                   # a run across the whole row
    _check(np.ascontiguousarray(vol.transpose(1, 2, 0))[None])


def test_labels():
    sphere, thr = M.cases32()["sphere"]
    rng = np.random.RandomState(7)
    three = rng.randint(0, 3, (S, S, S)).astype(np.int32)
    _check(sphere[None], thr, three[None])
    slab = np.zeros((S, S, S), np.float32)
    slab[10:14, 4:20, 3:29] = 1.0
    halves = np.zeros((S, S, S), np.int32)                                    # equal masks, different labels
    halves[:, :, 16:] = np.iinfo(np.int32).max
    halves[:, 12:, :8] = -5
    halves[12] = np.where(halves[12] == 0, np.iinfo(np.int32).min, halves[12])
    plain, cut = _check(slab[None]), _check(slab[None], 0.5, halves[None])
    assert int(plain.faces.shape[0]) == 6 < int(cut.faces.shape[0])
    both = _check(np.stack([slab, sphere]), thr, np.stack([halves, three]))
    assert both.face_offsets.tolist()[1] == int(cut.faces.shape[0])


def test_two_calls_give_the_same_bits():
    from rendernet_amd import ops
    vol = torch.as_tensor(np.stack([M.cases32()[n][0].astype(np.float32) for n in ("uniform_noise", "binary_u8")])).cuda()
    a, b = ops.extract_mesh_merged(vol), ops.extract_mesh_merged(vol)
    for x, y in zip(_arrays(a), _arrays(b)):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("name", ["sphere", "binary_u8", "grid_corners"])
def test_the_device_mesh_voxelises_to_the_grid(name):
    from rendernet_amd import ops
    vol, thr = M.cases32()[name]
    inside = vol.astype(np.float32) > np.float32(thr)
    mesh = ops.extract_mesh_merged(torch.as_tensor(vol[None]).cuda(), thr, triangles=True)
    for m in (mesh, mesh.unshared()):
        vox = ops.voxelize_mesh(m.q, m.faces, S, mode="solid")
        assert np.array_equal(vox.cpu().numpy()[0, ..., 0] != 0, inside), name


def test_unshared_and_merged_face_colours_equal_the_host_gather():
    from rendernet_amd import ops
    rng = np.random.RandomState(11)
    vol = np.stack([M.cases32()["sphere"][0], M.edge_cases()["both_sides"][0]])
    colours = rng.randint(0, 256, (2, S, S, S, 3)).astype(np.uint8)
    known = (rng.rand(2, S, S, S) < 0.7).astype(np.uint8)
    mesh = ops.extract_mesh_merged(torch.as_tensor(vol).cuda())
    q, faces, vo, fo, fv = (a.astype(np.int64) for a in _arrays(mesh)[:5])
    grid = np.searchsorted(fo[1:], np.arange(len(faces)), side="right")
    want = colours.reshape(2, -1, 3)[grid, fv]
    got = ops.merged_face_colours(mesh, torch.as_tensor(colours).cuda())
    assert got.dtype is torch.uint8 and np.array_equal(got.cpu().numpy(), want)
    got = ops.merged_face_colours(mesh, torch.as_tensor(colours).cuda(), torch.as_tensor(known).cuda(), unseen=(1, 2, 3))
    seen = known.reshape(2, -1)[grid, fv] != 0
    assert np.array_equal(got.cpu().numpy(), np.where(seen[:, None], want, np.array([1, 2, 3], np.uint8)))
    un = mesh.unshared()
    assert np.array_equal(un.q.cpu().numpy(), q[(faces + vo[grid][:, None]).reshape(-1)])
    local = np.arange(len(faces)) - fo[grid]
    assert np.array_equal(un.faces.cpu().numpy(), 4 * local[:, None] + np.arange(4))
    assert un.vert_offsets.tolist() == (4 * fo).tolist() and un.face_offsets.tolist() == fo.tolist()
    uq, uf = un.grid(1)
    mq, mf = mesh.grid(1)
    assert np.array_equal(uq.cpu().numpy()[uf.cpu().numpy()], mq.cpu().numpy()[mf.cpu().numpy()])


def test_no_grids_and_empty_grids_return_empty_arrays():
    from rendernet_amd import ops
    for B in (0, 2):
        for tri in (False, True):
            mesh = ops.extract_mesh_merged(torch.zeros((B, S, S, S, 1), device="cuda"), triangles=tri)
            assert tuple(mesh.q.shape) == (0, 3) and tuple(mesh.faces.shape) == (0, 3 if tri else 4)
            assert tuple(mesh.face_voxel.shape) == (0,) and tuple(mesh.face_dir.shape) == (0,) and tuple(mesh.face_size.shape) == (0, 2)
            assert mesh.vert_offsets.tolist() == [0] * (B + 1) == mesh.face_offsets.tolist()
            assert all(getattr(mesh, n).dtype is (torch.int64 if "offsets" in n else torch.int32) for n in NAMES)
            assert tuple(ops.merged_face_colours(mesh, torch.zeros((B, S, S, S, 3), dtype=torch.uint8, device="cuda")).shape) == (0, 3)


def test_labels_are_checked_on_the_device_too():
    from rendernet_amd import ops
    from rendernet_amd._lib import RenderNetHipError
    vol = torch.zeros((1, S, S, S), device="cuda")
    for bad in (torch.zeros((1, S, S, S), dtype=torch.int32), torch.zeros((2, S, S, S), dtype=torch.int32, device="cuda"),
                torch.zeros((1, S, S, S), dtype=torch.int64, device="cuda"), np.zeros((1, S, S, S), np.int32)):
        with pytest.raises(RenderNetHipError, match="labels"):
            ops.extract_mesh_merged(vol, labels=bad)
