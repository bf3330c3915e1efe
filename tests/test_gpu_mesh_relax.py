"""rn_mesh_relax on the device against the NumPy twin (tests/mesh_relax_ref.py): every coordinate, with the twin taking its
links from the quad rings and the device from the corner bits.  Both dtypes, both starts, odd and even pass counts, three
weights, batches, vertex counts about a wave and a workgroup, 32 / 64 / 128, what must NOT change (faces, offsets, colours, the
solid round trip, relax=0), determinism and the argument checks of the C entry.  -m gpu."""
import ctypes
import os

import numpy as np
import pytest

import mesh_extract_ref as E
import mesh_relax_ref as X

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CASES32 = E.cases32()
PASSES = (1, 2, 5)                                               # the ping-pong ends in q from either buffer
WEIGHTS = (256, 128, 77)


def _as_u8(vol, thr):
    """The same field in bytes: 200 steps per unit, so the values on the threshold 0.5 stay exactly on the threshold 100."""
    if vol.dtype == np.uint8:
        return vol.astype(np.float32), thr                       # the binary case: the other dtype is float32
    return np.clip(np.rint(vol.astype(np.float64) * 200.0), 0, 255).astype(np.uint8), 200.0 * thr


def _device(vol):
    import torch
    return torch.as_tensor(np.ascontiguousarray(vol)).cuda()


def _np(t):
    return t.cpu().numpy()


def _check(m, base, S, passes, weight, what, triangles=False):
    """m: the device's relaxed mesh; base = (q, faces, vo, fo): the TWIN's unrelaxed one.  Everything but q is base's."""
    q, f, vo, fo = base
    want = X.relax_batch(q, f, vo, fo, S, passes, weight, triangles)
    got = _np(m.q)
    assert got.dtype == np.int32 and got.shape == want.shape, (what, got.shape, want.shape)
    assert np.array_equal(got, want), (what, passes, weight, int((got != want).any(1).sum()), len(want))
    assert np.array_equal(_np(m.faces), f) and np.array_equal(_np(m.vert_offsets), vo) and np.array_equal(_np(m.face_offsets), fo), what


def _chair():
    from rendernet_amd.tools import binvox_rw
    with open(os.path.join(ROOT, "binvox", "chair.binvox"), "rb") as f:
        return np.ascontiguousarray(binvox_rw.read_as_3d_array(f).data).astype(np.uint8)


@pytest.mark.parametrize("name", sorted(CASES32))
def test_device_equals_twin_at_32(name):
    from rendernet_amd import ops
    vol, thr = CASES32[name]
    moved = 0
    for v, t in ((vol, thr), _as_u8(vol, thr)):
        dev = _device(v[None, ..., None])
        for smooth in (True, False):
            base = E.extract_batch(v[None], t, smooth)
            for passes in PASSES:
                for weight in WEIGHTS:
                    m = ops.extract_mesh(dev, threshold=t, smooth=smooth, relax=passes, relax_weight=weight)
                    _check(m, base, 32, passes, weight, (name, str(v.dtype), smooth))
                    moved += int((_np(m.q) != base[0]).any())
    assert moved == 2 * 2 * len(PASSES) * len(WEIGHTS)           # and the relaxed mesh is not the unrelaxed one


def test_the_full_grid_meets_both_clamps():
    """Every vertex sits in a clipped boundary cell: lo = 0 on one side, hi = 256 S on the other."""
    from rendernet_amd import ops
    vol, thr = CASES32["full"]
    base = E.extract_batch(vol[None], thr, True)
    m = ops.extract_mesh(_device(vol[None]), relax=4)
    _check(m, base, 32, 4, 256, "full")
    q = _np(m.q)
    assert int(q.min()) == 0 and int(q.max()) == 256 * 32 and len(q) == 33 ** 3 - 31 ** 3


def _box(S, a, b, c):
    vol = np.zeros((S, S, S), np.uint8)
    vol[3:3 + a, 4:4 + b, 5:5 + c] = 1
    return vol


@pytest.mark.parametrize("triangles", [False, True], ids=["quads", "triangles"])
def test_batch_of_four_with_an_empty_grid_second(triangles):
    from rendernet_amd import ops
    vols = np.stack([CASES32["binary_u8"][0], np.zeros((32, 32, 32), np.uint8), _box(32, 1, 1, 1), (E.sphere_field(32) > 0.5).astype(np.uint8)])
    base = E.extract_batch(vols, 0.5, True, triangles)
    counts = np.diff(base[2]).tolist()
    assert counts[1] == 0 and counts[2] == 8 and counts[0] > 10000 and counts[3] > 2000
    for passes in (3, 4):
        m = ops.extract_mesh(_device(vols), triangles=triangles, relax=passes)
        _check(m, base, 32, passes, 256, ("batch", triangles), triangles)
        for b in range(4):                                       # and the same grids one at a time
            one = ops.extract_mesh(_device(vols[b:b + 1]), triangles=triangles, relax=passes)
            q, f = m.grid(b)
            assert np.array_equal(_np(q), _np(one.q)) and np.array_equal(_np(f), _np(one.faces)), b
    none = ops.extract_mesh(_device(vols[:0]), relax=4)
    assert tuple(none.q.shape) == (0, 3) and none.vert_offsets.tolist() == [0]
    empty = ops.extract_mesh(_device(vols[1:2]), relax=4)
    assert tuple(empty.q.shape) == (0, 3) and tuple(empty.faces.shape) == (0, 4)


@pytest.mark.parametrize("box, count", [((1, 1, 1), 8), ((3, 3, 3), 56), ((4, 3, 3), 68), ((6, 6, 7), 242), ((6, 7, 7), 268)])
def test_vertex_counts_about_a_wave_and_a_workgroup(box, count):
    """One thread per vertex: a box of a x b x c voxels has (a+1)(b+1)(c+1) - (a-1)(b-1)(c-1) of them."""
    from rendernet_amd import ops
    vol = _box(32, *box)
    for smooth in (True, False):
        base = E.extract_batch(vol[None], 0.5, smooth)
        assert len(base[0]) == count
        for passes in (1, 4):
            _check(ops.extract_mesh(_device(vol[None]), smooth=smooth, relax=passes), base, 32, passes, 256, (box, smooth))


def test_a_csg_grid_at_64():
    import torch
    from rendernet_amd import ops, synth
    vox = ops.voxel_shapes(torch.as_tensor(synth.shape_prims(1234, [0x1a2b3c4d], 64)).cuda(), 64)
    base = E.extract_batch(_np(vox), 0.5, True)
    assert len(base[0]) > 1000
    for passes, weight in ((4, 256), (5, 128)):
        _check(ops.extract_mesh(vox, relax=passes, relax_weight=weight), base, 64, passes, weight, "csg64")


def test_a_sphere_at_128():
    """129^3 cells and some 40 000 vertices: more than a hundred workgroups a pass."""
    from rendernet_amd import ops
    vol = E.sphere_field(128)
    base = E.extract_batch(vol[None], 0.5, True)
    assert len(base[0]) > 40000
    _check(ops.extract_mesh(_device(vol[None]), relax=4), base, 128, 4, 256, "sphere128")


def test_relax_zero_is_the_mesh_without_it_and_two_calls_agree():
    import torch
    from rendernet_amd import ops
    dev = _device(np.stack([CASES32["uniform_noise"][0], CASES32["threshold_ties"][0]]))
    plain, zero = ops.extract_mesh(dev), ops.extract_mesh(dev, relax=0, relax_weight=77)
    a, b = ops.extract_mesh(dev, relax=5, relax_weight=128), ops.extract_mesh(dev, relax=5, relax_weight=128)
    assert a.q.data_ptr() != b.q.data_ptr()
    for name in ("q", "faces", "vert_offsets", "face_offsets"):
        assert torch.equal(getattr(plain, name), getattr(zero, name)), name
        assert torch.equal(getattr(a, name), getattr(b, name)), name
        if name != "q":
            assert torch.equal(getattr(a, name), getattr(plain, name)), name
    assert not torch.equal(a.q, plain.q)


def test_the_relaxed_chair_voxelises_to_the_chair_and_keeps_its_colours():
    import torch
    from rendernet_amd import ops
    grid = _chair()
    dev = _device(grid.reshape(1, 64, 64, 64, 1))
    want, _ = ops.voxel_pack(dev, 0.5)
    plain = ops.extract_mesh(dev, triangles=True)
    rng = np.random.default_rng(7)
    col = _device(rng.integers(0, 256, (1, 64, 64, 64, 3), dtype=np.uint8))
    known = _device((rng.random((1, 64, 64, 64)) < 0.7).astype(np.uint8))
    colours = ops.mesh_vertex_colours(plain, col, known)
    assert len(torch.unique(colours, dim=0)) > 100
    for smooth in (True, False):
        start = plain if smooth else ops.extract_mesh(dev, smooth=False, triangles=True)
        base = E.extract_batch(grid[None], 0.5, smooth, triangles=True)
        for passes in (1, 4, 64):
            m = ops.extract_mesh(dev, smooth=smooth, triangles=True, relax=passes)
            _, bits = ops.voxelize_mesh(m.q, m.faces, S=64, mode="solid", return_bits=True)
            assert torch.equal(bits, want), (smooth, passes, int((bits != want).sum()))
            assert torch.equal(ops.mesh_vertex_colours(m, col, known), colours), (smooth, passes)
            assert torch.equal(m.faces, plain.faces), (smooth, passes)
            assert not torch.equal(m.q, start.q), (smooth, passes)
            _check(m, base, 64, passes, 256, ("chair", smooth), triangles=True)


def test_argument_checks_through_the_c_abi():
    """Every invalid argument is refused with RN_E_INVALID and the entry's name in the error; nothing is launched, so q and
    the workspace keep the pattern they were filled with.  Then the same buffers with valid arguments: the lone voxel."""
    import torch
    from rendernet_amd import _lib as L
    lib, vp = L.lib(), ctypes.c_void_p
    S, B, V = 32, 1, 8
    vol = torch.zeros((B, S, S, S), device="cuda")
    vol[0, 5, 9, 20] = 1.0
    new = lambda shape, dtype=torch.int32: torch.full(shape, -7, dtype=dtype, device="cuda")
    nws = int(lib.rn_mesh_extract_workspace_bytes(B, S))
    ws, totals, cellvert = new((nws // 4,)), new((B, 2)), new((B, (S + 1) ** 3))
    off = torch.tensor([0, V], dtype=torch.int64, device="cuda")
    q, faces = new((V + 1, 3)), new((6, 4))
    st = L.stream_ptr()
    P = lambda t, byte=0: vp(t.data_ptr() + byte)
    assert lib.rn_mesh_extract_count(P(vol), 0, 0.5, B, S, P(ws), nws, P(totals), st) == 0
    assert lib.rn_mesh_extract_emit(P(vol), 0, 0.5, B, S, 0, 0, P(ws), nws, P(off), P(off), V, 6, P(cellvert), P(q), P(faces), st) == 0
    torch.cuda.synchronize()
    start = q.clone()
    assert totals.tolist() == [[8, 6]] and bool((q[V] == -7).all())
    nrws = int(lib.rn_mesh_relax_workspace_bytes(V))
    assert nrws == 36 * V
    rws = new((nrws // 4 + 4,))

    def relax(vol_p=P(vol), u8=0, thr=0.5, b=B, s=S, cv=P(cellvert), vo=P(off), nv=V, passes=1, weight=256, ws_p=P(rws), n=nrws,
              q_p=P(q)):
        return lib.rn_mesh_relax(vol_p, u8, thr, b, s, cv, vo, nv, passes, weight, ws_p, n, q_p, st)
    bad = [dict(passes=-1), dict(passes=65), dict(weight=0), dict(weight=257), dict(weight=-256), dict(s=48), dict(s=0), dict(s=256),
           dict(b=-1), dict(b=65536), dict(b=0), dict(nv=-1), dict(nv=1 << 31), dict(thr=float("nan")), dict(u8=2),
           dict(vol_p=None), dict(cv=None), dict(vo=None), dict(ws_p=None), dict(q_p=None),
           dict(vol_p=P(vol, 2)), dict(cv=P(cellvert, 2)), dict(vo=P(off, 4)), dict(ws_p=P(rws, 8)), dict(q_p=P(q, 2)),
           dict(n=nrws - 16), dict(n=0),
           dict(passes=0, q_p=None), dict(passes=0, weight=0)]                # passes = 0 launches nothing, and is checked all the same
    for kw in bad:
        assert relax(**kw) == L.RN_E_INVALID, kw
        assert b"rn_mesh_relax:" in lib.rn_last_error(), (kw, lib.rn_last_error())
    assert relax(passes=0) == L.RN_OK and relax(b=0, nv=0) == L.RN_OK and relax(nv=0) == L.RN_OK          # the no-ops
    torch.cuda.synchronize()
    assert torch.equal(q, start) and bool((rws == -7).all())
    # offsets that do not belong to the mesh: vertices 4..7 are given to a second grid that has no such cells.  Nothing is
    # written outside q[:V], whatever the links turn out to be
    off2 = torch.tensor([0, 4, V], dtype=torch.int64, device="cuda")
    vol2 = torch.cat([vol, torch.zeros_like(vol)])
    cv2 = torch.cat([cellvert, new((B, (S + 1) ** 3))])
    q2 = q.clone()
    assert lib.rn_mesh_relax(P(vol2), 0, 0.5, 2, S, P(cv2), P(off2), V, 3, 256, P(rws), nrws, P(q2), st) == L.RN_OK
    torch.cuda.synchronize()
    assert bool((q2[V] == -7).all()) and bool((rws[nrws // 4:] == -7).all())
    assert torch.equal(q2[4:V], start[4:V])                      # an all-outside cell has no links: its vertex stays
    # the valid call: one pass over the lone voxel's corners, a third of the way (tests/test_mesh_relax_cpu.py works it out)
    assert relax() == L.RN_OK
    torch.cuda.synchronize()
    lo = 256 * np.array([5, 9, 20])
    bits = np.array([[i, j, k] for i in (0, 1) for j in (0, 1) for k in (0, 1)])
    assert np.array_equal(_np(q[:V]), np.where(bits == 0, lo + 85, lo + 171)) and bool((q[V] == -7).all())
    assert bool((rws[nrws // 4:] == -7).all())
