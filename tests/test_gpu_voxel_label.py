"""rn_voxel_label / rn_voxel_label_stats / rn_voxel_topology on the device against the NumPy twin (tests/voxel_label_ref.py):
every label, count, offset, statistics row and topology word exactly, for both selected sets and both connectivities at 32, 64
and 128, the closed forms, the word seams, batches with an empty item, the clean-up, the input forms, determinism and the
refusals.  -m gpu."""
import functools

import numpy as np
import pytest

import voxel_label_ref as R

pytestmark = pytest.mark.gpu
RULES = [("solid", 26), ("solid", 6), ("empty", 6), ("empty", 26)]


def _device(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _model(name):
    g = R.load_binvox(name)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def _grids(which):
    """The boolean batches of the tests, built once per session and left unchanged."""
    if which == 32:
        forms = [g for _, g in R.closed_forms_32()]
        g = np.stack(forms[:7] + R.random_grids(32) + forms[7:])
        assert not g[5].any() and g[4].any() and g[6].any()      # the empty item sits between two occupied ones
    elif which == 64:
        g = np.stack([_model(n) for n in R.MODELS] + R.seam_cases(64, [32]))
    else:
        g = np.stack([np.kron(_model("chair"), np.ones((2, 2, 2), bool)), R.seam_cases(128, [64, 96])[-1]])
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def _twin(which, of, connectivity):
    out = R.components(_grids(which), of, connectivity)
    for a in out:
        a.setflags(write=False)
    return out


@functools.lru_cache(maxsize=None)
def _twin_words(which):
    w = np.stack([R.topology(g) for g in _grids(which)])
    w.setflags(write=False)
    return w


def _same(got, want, what):
    import torch
    for name, g, w, dtype in zip(("labels", "counts", "offsets", "stats"), got, want, (torch.int32, torch.int32, torch.int64, torch.int32)):
        assert g.is_cuda and g.dtype is dtype and tuple(g.shape) == w.shape, (what, name, g.dtype, tuple(g.shape), w.shape)
        g = g.cpu().numpy()
        assert np.array_equal(g, w), (what, name, int((g != w).sum()), g[g != w][:6], w[g != w][:6])


@pytest.mark.parametrize("of,connectivity", RULES)
def test_device_equals_twin_at_32(of, connectivity):
    """All closed forms and the three random grids in one batched call; the empty item in the middle tests the offsets."""
    from rendernet_amd import ops
    want = _twin(32, of, connectivity)
    _same(ops.voxel_components(_device(_grids(32).astype(np.uint8)), of=of, connectivity=connectivity), want, (of, connectivity))
    if (of, connectivity) == ("solid", 26):
        assert want[1].tolist()[:7] == [1, 1, 1, 1, 1, 0, 1] and want[1].tolist()[7:10] == [800, 76, 1]
    if (of, connectivity) == ("solid", 6):
        assert want[1].tolist()[:5] == [1, 2, 2, 3, 16384] and want[1].tolist()[7:10] == [1451, 2929, 362]
    if (of, connectivity) == ("empty", 6):
        assert want[1].tolist()[4] == 13500 and want[1].tolist()[6] == 1 and want[1].tolist()[10:13] == [1, 2, 0]


@pytest.mark.parametrize("of,connectivity", RULES)
def test_device_equals_twin_at_64(of, connectivity):
    """The five models; the pitfall pattern and the corner and edge pairs across the word seam at xs 31 / 32 / 33, on the grid
    border, on the last row and on the last plane."""
    from rendernet_amd import ops
    _same(ops.voxel_components(_device(_grids(64).astype(np.uint8)[..., None]), of=of, connectivity=connectivity),
          _twin(64, of, connectivity), (of, connectivity))


@pytest.mark.parametrize("of,connectivity", RULES)
def test_device_equals_twin_at_128(of, connectivity):
    """The doubled chair, and the seam patterns at xs 63 / 64 / 65 and 95 / 96 / 97 in one grid."""
    from rendernet_amd import ops
    _same(ops.voxel_components(_device(_grids(128).astype(np.uint8)), of=of, connectivity=connectivity),
          _twin(128, of, connectivity), (of, connectivity))


@pytest.mark.parametrize("which", [32, 64, 128])
def test_topology_words_equal_the_twin(which):
    import torch
    from rendernet_amd import ops
    want = _twin_words(which)
    t = ops.voxel_topology(_device(_grids(which).astype(np.uint8)))
    assert t.words.is_cuda and t.words.dtype is torch.int64
    got = t.words.cpu().numpy()
    assert np.array_equal(got, want), (got[(got != want).any(1)], want[(got != want).any(1)])
    assert t.components.tolist() == want[:, 1].tolist() and t.cavities.tolist() == want[:, 2].tolist()
    assert t.euler.tolist() == want[:, 6].tolist() and t.handles.tolist() == want[:, 7].tolist()
    rows = t.as_dicts()
    assert [r["words"] for r in rows] == want.tolist() and rows[0]["handles"] == want[0, 7] and rows[0]["voxels"] == want[0, 0]
    if which == 64:
        assert t.handles.tolist()[:5] == [0, 1, 0, 2, 1] and t.components.tolist()[:5] == [1] * 5 and t.cavities.tolist()[:5] == [0] * 5
    if which == 32:
        assert want[4].tolist()[1:3] == [1, 13500] and want[4, 6] == 13501 and want[-2].tolist()[6:] == [-4, 5]


def test_clean_returns_the_chair_and_the_solid_box():
    import torch
    from rendernet_amd import ops
    chair = _model("chair")
    p = np.pad(chair, 1)
    inner = chair & p[1:-1, 1:-1, :-2] & p[1:-1, 1:-1, 2:] & p[1:-1, :-2, 1:-1] & p[1:-1, 2:, 1:-1] & p[:-2, 1:-1, 1:-1] & p[2:, 1:-1, 1:-1]
    dirty = chair.copy()
    dirty[tuple(np.argwhere(inner)[len(np.argwhere(inner)) // 2])] = False       # a bubble: all six neighbours are solid
    assert not dirty[2:5, 2:5, 2:5].any() and not dirty[60, 60, 60] and not dirty[2, 60, 2:4].any()
    dirty[3, 3, 3] = dirty[60, 60, 60] = dirty[2, 60, 2:4] = True                 # three specks
    before = ops.voxel_topology(_device(dirty.astype(np.uint8)[None]))
    assert before.components.tolist() == [4] and before.cavities.tolist() == [1]
    shells = R.nested_shells(32)
    for grid, want in ((dirty, chair), (shells, R.box(32, 4, 20))):
        got = ops.voxel_clean(_device(grid.astype(np.uint8)[None]))
        assert tuple(got.shape) == (1,) + grid.shape + (1,) and got.dtype is torch.uint8 and got.is_cuda
        assert np.array_equal(got.cpu().numpy()[0, ..., 0], want.astype(np.uint8))
        assert np.array_equal(got.cpu().numpy()[0, ..., 0].astype(bool), R.clean(grid)[0])
    # the options against the twin, two items in one call; a soft volume at its own threshold
    both = np.stack([dirty, np.roll(dirty, 1, 2)])
    soft = _device(np.where(both, np.float32(0.3), np.float32(0.1))[..., None])
    for kw in (dict(keep_largest=None, min_voxels=2), dict(keep_largest=0, fill_cavities=False), dict(keep_largest=2, connectivity=6),
               dict(keep_largest=3, min_voxels=2, fill_cavities=False)):
        got = ops.voxel_clean(soft, threshold=0.1, **kw).cpu().numpy()[..., 0].astype(bool)
        for b in range(2):
            assert np.array_equal(got[b], R.clean(both[b], **kw)[0]), (kw, b)
    # the mesh of the cleaned nested shells, voxelised again solid, is the cleaned grid
    cleaned = ops.voxel_clean(_device(shells.astype(np.uint8)[None]))
    m = ops.extract_mesh(cleaned, triangles=True)
    assert torch.equal(ops.voxelize_mesh(m.q, m.faces, S=32, mode="solid"), cleaned)
    assert ops.voxel_topology(cleaned).words.cpu().tolist()[0][1:3] == [1, 0]


def test_input_forms_agree_and_two_calls_give_the_same_bits():
    import torch
    from rendernet_amd import ops
    occ = _grids(32)[[4, 7, 8, 12]].astype(np.uint8)              # the checkerboard, two random grids, the cube's edges
    for of, connectivity in (("solid", 6), ("empty", 6)):
        ref = ops.voxel_components(_device(occ), of=of, connectivity=connectivity)
        soft = _device(np.where(occ > 0, np.float32(0.2), np.float32(0.1))[..., None])
        bits, _ = ops.voxel_pack(_device(occ))
        assert np.array_equal(bits.cpu().numpy(), R.pack(occ.astype(bool)))
        again = ops.voxel_components(_device(occ), of=of, connectivity=connectivity)
        assert again.labels.data_ptr() != ref.labels.data_ptr()
        for other in (ops.voxel_components(soft, 0.1, of, connectivity), ops.voxel_components(bits=bits, S=32, of=of, connectivity=connectivity),
                      again):
            for a, b in zip(ref, other):
                assert torch.equal(a, b)
    t1, t2 = ops.voxel_topology(_device(occ)), ops.voxel_topology(bits=bits, S=32)
    assert t1.words.data_ptr() != t2.words.data_ptr() and torch.equal(t1.words, t2.words)
    none = ops.voxel_components(_device(occ[:0]))
    assert tuple(none.labels.shape) == (0, 32, 32, 32) and tuple(none.stats.shape) == (0, 8) and none.offsets.tolist() == [0]
    assert tuple(ops.voxel_topology(_device(occ[:0])).words.shape) == (0, 8) and ops.voxel_topology(_device(occ[:0])).as_dicts() == []
    assert tuple(ops.voxel_clean(_device(occ[:0])).shape) == (0, 32, 32, 32, 1)
    zero = ops.voxel_components(_device(np.zeros((2, 32, 32, 32), np.uint8)))
    assert zero.counts.tolist() == [0, 0] and tuple(zero.stats.shape) == (0, 8) and not zero.labels.any()
    assert not ops.voxel_clean(_device(np.zeros((2, 32, 32, 32), np.uint8))).any()


def test_refusals_leave_the_device_usable():
    import torch
    from rendernet_amd import ops
    from rendernet_amd._lib import RenderNetHipError
    chair = _device(_model("chair").astype(np.uint8)[None])
    bad = [lambda: ops.voxel_components(torch.zeros((1, 48, 48, 48), device="cuda")),
           lambda: ops.voxel_components(torch.zeros((1, 64, 64, 32), device="cuda")),
           lambda: ops.voxel_components(chair.cpu()),
           lambda: ops.voxel_components(chair, of="inside"),
           lambda: ops.voxel_components(chair, connectivity=18),
           lambda: ops.voxel_components(bits=torch.zeros((1, 100), dtype=torch.int32, device="cuda"), S=64),
           lambda: ops.voxel_components(chair, bits=torch.zeros((1, 8192), dtype=torch.int32, device="cuda"), S=64),
           lambda: ops.voxel_clean(chair, keep_largest=-2),
           lambda: ops.voxel_clean(chair, min_voxels=0),
           lambda: ops.voxel_clean(chair, connectivity=18),
           lambda: ops.voxel_topology(torch.zeros((1, 16, 16, 16), device="cuda")),
           lambda: ops.voxel_topology(chair.cpu())]
    for call in bad:
        with pytest.raises(RenderNetHipError):
            call()
        torch.cuda.synchronize()
    assert ops.voxel_topology(chair).words.cpu().tolist() == [R.topology(_model("chair")).tolist()]
