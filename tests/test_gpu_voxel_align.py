"""rn_voxel_orient / rn_voxel_align on the device against the NumPy twin (tests/voxel_align_ref.py): the whole score table and the
eight words exactly, at 32, 64 and 128, for batches, both signs of every shift axis, the mirrored set, the word seam of a row, the
largest shift and the slab path; the oriented copies alone; determinism, B = 0, the table left out, the refusals.  -m gpu."""
import ctypes
import functools

import numpy as np
import pytest

import voxel_align_ref as R
from test_voxel_align_cpu import MIRROR_MOVE, MOVE, small, table_of

pytestmark = pytest.mark.gpu

THIRD_MOVE = (22, (-2, 3, -1))


def _device(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


def _u8(occ):
    return _device(np.asarray(occ).astype(np.uint8))


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == want.dtype and got.shape == want.shape, (what, got.dtype, got.shape, want.shape)
    assert np.array_equal(got, want), (what, int((got != want).sum()), got[got != want][:4], want[got != want][:4])


def _words(moved, fixed, table, R_):
    o, t, n, _ = R.winner(table, R_)
    return np.array([o, t[0], t[1], t[2], n, np.count_nonzero(moved), np.count_nonzero(fixed), table[0, R_, R_, R_]], np.int32)


def _check(moved, fixed, tables, R_, orientations):
    """One batched call against the twin's tables (one per item, already cut to the orientation set)."""
    from rendernet_amd import ops
    got = ops.voxel_align(_u8(np.stack(moved)), _u8(np.stack(fixed)), max_shift=R_, orientations=orientations, return_scores=True)
    _same(got.scores, np.stack(tables), ("scores", orientations, R_))
    _same(got.words, np.stack([_words(m, f, t, R_) for m, f, t in zip(moved, fixed, tables)]), ("words", orientations, R_))
    return got


@functools.lru_cache(maxsize=None)
def chair64():
    g = R.load_binvox("chair")
    g.setflags(write=False)
    return g


def test_batch_of_three_at_32_with_all_orientations():
    names, moves = ("chair", "bunny", "table"), (MOVE, MIRROR_MOVE, THIRD_MOVE)
    fixed = [small(n) for n in names]
    moved = [R.transform(g, *m) for g, m in zip(fixed, moves)]
    tables = [table_of(n, m) for n, m in zip(names, moves)]
    got = _check(moved, fixed, tables, 3, "all")
    words = got.words.cpu().numpy()
    assert tuple(words[0, :5]) == (18, 3, -2, -1, 244) and tuple(words[1, :5]) == (40, -1, 3, 0, 1271)
    assert words[2, 4] == 1212
    _same(got.apply(_u8(np.stack(moved))), np.stack(fixed).astype(np.uint8), "apply gives the models back")
    assert got.iou_after.cpu().tolist() == [1.0, 1.0, 1.0] and max(got.iou_before.cpu().tolist()) < 0.5
    rot = _check(moved, fixed, [t[:24] for t in tables], 3, "rotations")      # the same tables, cut to the rotations
    assert rot.words.cpu().numpy()[1, 4] == 1088


def test_word_seam_at_64():
    """A row of 64^3 is two words: every tx carries bits across the seam."""
    g = chair64()
    moved = R.transform(g, 5, (1, -2, 2))
    table = R.scores(moved, g, 2, 24)
    got = _check([moved], [g], [table], 2, "rotations")
    assert tuple(got.words.cpu().numpy()[0, :7]) == (4, -1, -2, -2, 5206, int(moved.sum()), 5277)


def test_largest_shift_at_64():
    """R = 16, rows full from one end to the other: whole half words leave at both ends, and the shifts reach +-16."""
    rng = np.random.default_rng(20)
    a = np.zeros((64, 64, 64), bool)
    a[28:36, 24:40, :] = rng.random((8, 16, 64)) > 0.25
    a[30, 30:34, :] = True
    b = R.shift(a, (-5, 7, -13))
    b[29:33, 26:30, :] = True
    table = R.scores(a, b, 16, 1)
    assert table.shape == (1, 33, 33, 33) and table[0, 0, 0, 0] == 0 and table[0, 16 - 5, 16 + 7, 16 - 13] > 0
    got = _check([a], [b], [table], 16, "none")
    assert tuple(got.words.cpu().numpy()[0, :4]) == (0, -5, 7, -13)
    both = _check([a, b], [b, a], [table, R.scores(b, a, 16, 1)], 16, "none")
    assert tuple(both.words.cpu().numpy()[1, :4]) == (0, 5, -7, 13)


def test_slabs_at_128():
    """Four words a row, eight z-slabs; a shift in z crosses the slab seams."""
    g = np.kron(chair64(), np.ones((2, 2, 2), bool))
    rng = np.random.default_rng(128)
    g = g & (rng.random(g.shape) > 0.1)
    moved = R.transform(g, 7, (1, -1, 0))
    table = R.scores(moved, g, 1, 24)
    got = _check([moved], [g], [table], 1, "rotations")
    back = R.winner(table, 1)
    assert back[2] == int(moved.sum()) and np.array_equal(R.transform(moved, back[0], back[1]), R.transform(moved, back[0], back[1]) & g)
    assert got.words.cpu().numpy()[0, 0] != 0
    _check([moved], [g], [table[:1]], 1, "none")


@pytest.mark.parametrize("S", [32, 64])
def test_orient_alone(S):
    from rendernet_amd import ops
    rng = np.random.default_rng(S)
    grids = np.stack([rng.random((S, S, S)) > 0.5, chair64() if S == 64 else small("bunny")])
    want = np.stack([R.pack(np.stack([R.orient(g, o) for o in range(48)])) for g in grids])
    _same(ops.voxel_orient(_u8(grids)), want, ("orient", S))
    _same(ops.voxel_orient(_u8(grids), first=13, count=6), want[:, 13:19], ("orient 13..18", S))
    bits, _ = ops.voxel_pack(_u8(grids))
    _same(ops.voxel_orient(bits=bits, S=S, first=47, count=1), want[:, 47:], ("orient from bits", S))
    assert tuple(ops.voxel_orient(_u8(grids), first=5, count=0).shape) == (2, 0, S ** 3 // 32)


def test_determinism_edges_and_metrics():
    import torch
    from rendernet_amd import ops
    g = small("chair")
    moved = R.transform(g, *MOVE)
    a, b = _u8(moved[None]), _u8(g[None])
    one = ops.voxel_align(a, b, max_shift=3, return_scores=True)
    two = ops.voxel_align(a, b, max_shift=3, return_scores=True)
    assert torch.equal(one.words, two.words) and torch.equal(one.scores, two.scores)
    bare = ops.voxel_align(a, b, max_shift=3)                                 # out_scores null: the table stays in the workspace
    assert bare.scores is None and torch.equal(bare.words, one.words)
    soft = ops.voxel_align(a.float()[..., None] * 0.3, b, max_shift=3, threshold=(0.1, 0.5))
    assert torch.equal(soft.words, one.words)
    none = ops.voxel_align(a[:0], b[:0], return_scores=True)
    assert tuple(none.words.shape) == (0, 8) and tuple(none.scores.shape) == (0, 24, 17, 17, 17)
    assert tuple(none.apply(a[:0]).shape) == (0, 32, 32, 32) and none.as_dicts() == []
    same = ops.voxel_align(b, b, max_shift=2, orientations="all")
    assert same.words.cpu().tolist() == [[0, 0, 0, 0, 244, 244, 244, 244]]
    empty = torch.zeros_like(b)
    nothing = ops.voxel_align(empty, empty, max_shift=2, orientations="all")
    assert nothing.words.cpu().tolist() == [[0] * 8] and nothing.iou_after.tolist() == [1.0]
    # the metrics of the aligned pair are the metrics of the twin-aligned pair
    pooled = R.pool(R.load_binvox("table"), 2)
    shoved = R.transform(pooled, 13, (2, -1, 1))
    o, t, n, _ = R.winner(R.scores(shoved, pooled, 3, 24), 3)
    got = ops.voxel_align(_u8(shoved[None]), _u8(pooled[None]), max_shift=3)
    assert got.words.cpu().tolist()[0][:5] == [o, t[0], t[1], t[2], 6372]
    m_dev = ops.voxel_shape_metrics(got.apply(_u8(shoved[None])), _u8(pooled[None]))
    m_twin = ops.voxel_shape_metrics(_u8(R.transform(shoved, o, t)[None]), _u8(pooled[None]))
    assert torch.equal(m_dev.words, m_twin.words) and int(m_dev.words[0, 2]) == 6372


def test_native_refusals_leave_the_device_usable():
    import torch
    from rendernet_amd import _lib, ops
    lib = _lib.lib()
    assert lib.rn_voxel_align_workspace_bytes(2, 64, 8, 24) == 2 * 24 * (64 ** 3 // 8 + 17 * 8 + 17 ** 3 * 4)   # copies, keys, table
    for args in ((1, 48, 8, 24), (1, 64, 17, 24), (1, 64, -1, 24), (-1, 64, 8, 24), (1, 64, 8, 0), (1, 64, 8, 49)):
        assert lib.rn_voxel_align_workspace_bytes(*args) == 0
    bits = torch.zeros((1, 32 ** 3 // 32), dtype=torch.int32, device="cuda")
    best = torch.zeros((1, 8), dtype=torch.int32, device="cuda")
    ws = torch.zeros((1 << 16,), dtype=torch.int32, device="cuda")
    p = lambda t: ctypes.c_void_p(t.data_ptr())
    call = lambda S=32, R_=1, set_=0, a=p(bits), out=p(best), w=p(ws), n=ws.numel() * 4: lib.rn_voxel_align(
        a, p(bits), 1, S, R_, set_, out, None, w, n, _lib.stream_ptr())
    for kw in ({"S": 48}, {"R_": 17}, {"R_": -1}, {"set_": 3}, {"set_": -1}, {"a": None}, {"out": None}, {"w": None}, {"n": 64},
               {"w": ctypes.c_void_p(ws.data_ptr() + 4)}):
        assert call(**kw) != 0 and b"rn_voxel_align" in lib.rn_last_error(), kw
    assert lib.rn_voxel_align(None, None, 0, 32, 1, 0, None, None, None, 0, _lib.stream_ptr()) == 0      # B = 0 asks for nothing
    for first, count in ((-1, 1), (47, 2), (0, 49), (0, -1)):
        assert lib.rn_voxel_orient(p(bits), 1, 32, first, count, p(ws), _lib.stream_ptr()) != 0
    assert lib.rn_voxel_orient(p(bits), 70000, 32, 0, 1, p(ws), _lib.stream_ptr()) != 0
    assert call() == 0
    torch.cuda.synchronize()
    assert best.cpu().tolist() == [[0] * 8]
    with pytest.raises(_lib.RenderNetHipError, match="voxel_align"):
        ops.voxel_align(torch.zeros((1, 32, 32, 32), device="cuda"), torch.zeros((1, 64, 64, 64), device="cuda"))
