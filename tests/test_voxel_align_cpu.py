"""The rule of rn_voxel_align on the NumPy twin (tests/voxel_align_ref.py): the orientation table and its numbering, exact recovery
of a moved model, the tie order, the mirrored set, voxels pushed out of the grid, the degenerate cases; ops.voxel_transform and
ops.ORIENTATIONS against the twin; the header, the binding and the argument errors that need no device."""
import functools
import os
import re

import numpy as np
import pytest

import voxel_align_ref as R

ROOT = R.ROOT
MOVE = (13, (2, -1, 3))
MIRROR_MOVE = (37, (-3, 0, 1))


@functools.lru_cache(maxsize=None)
def small(name):
    """The model pooled by 4 to 16^3 in the middle of 32^3: a margin of 8, so no move by a shift of up to 3 loses a voxel."""
    g = R.centred(R.pool(R.load_binvox(name), 4), 32)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def table_of(name, move, R_=3):
    """The whole table (48 orientations) of the moved model against the model, computed once and left unchanged."""
    t = R.scores(R.transform(small(name), *move), small(name), R_, 48)
    t.setflags(write=False)
    return t


def test_orientation_table():
    assert len(R.TABLE) == 48 and len(set(R.TABLE)) == 48
    mats = [R.matrix(o) for o in range(48)]
    assert len({m.tobytes() for m in mats}) == 48
    dets = [int(round(np.linalg.det(m))) for m in mats]
    assert dets[:24] == [1] * 24 and dets[24:] == [-1] * 24
    assert R.TABLE[0] == ((0, 1, 2), (0, 0, 0))
    pairs = [pf for pf in R.TABLE[:24]]
    assert pairs == sorted(pairs) and list(R.TABLE[24:]) == sorted(R.TABLE[24:])
    a = np.arange(4 ** 3).reshape(4, 4, 4)
    assert np.array_equal(R.orient(a, 0), a)
    for o, back in ((13, 18), (37, 40)):
        assert np.array_equal(R.orient(R.orient(a, o), back), a) and np.array_equal(R.orient(R.orient(a, back), o), a)
    assert not np.array_equal(R.orient(R.orient(a, 13), 13), a)
    # the definition itself, element by element, on an orientation that permutes and flips
    (p, f), S = R.TABLE[13], 4
    out = R.orient(a, 13)
    for i in np.ndindex(S, S, S):
        j = [0, 0, 0]
        for k in range(3):
            j[p[k]] = S - 1 - i[k] if f[k] else i[k]
        assert out[i] == a[tuple(j)]


def test_ops_table_and_transform_are_the_twins():
    import torch
    from rendernet_amd import ops
    assert len(ops.ORIENTATIONS) == 48
    assert [tuple(r) for r in ops.ORIENTATIONS] == [p + f for p, f in R.TABLE]
    g = small("chair")
    vox = torch.from_numpy(np.stack([g, g, g]).astype(np.uint8))
    moves = [(13, (2, -1, 3)), (37, (-3, 0, 1)), (0, (0, 0, 0))]
    out = ops.voxel_transform(vox, [m[0] for m in moves], [m[1] for m in moves])
    assert out.dtype is torch.uint8 and out.shape == vox.shape
    for b, m in enumerate(moves):
        assert np.array_equal(out[b].numpy().astype(bool), R.transform(g, *m)), m
    soft = torch.from_numpy(np.where(g, np.float32(0.7), np.float32(0.0)))[None, ..., None]
    out = ops.voxel_transform(soft, 13, (2, -1, 3))
    assert out.dtype is torch.float32 and out.shape == soft.shape
    assert np.array_equal(out[0, ..., 0].numpy(), np.where(R.transform(g, *MOVE), np.float32(0.7), np.float32(0.0)))
    far = ops.voxel_transform(vox[:1], 0, (0, 0, 20))                  # zero fill, nothing wraps
    assert np.array_equal(far[0].numpy().astype(bool), R.shift(g, (0, 0, 20))) and far.sum() < vox[:1].sum()


@pytest.mark.parametrize("name,count", [("chair", 244), ("bunny", 1271), ("table", 1212)])
def test_exact_recovery(name, count):
    g = small(name)
    assert int(g.sum()) == count
    moved = R.transform(g, *MOVE)
    assert int(moved.sum()) == count
    table = table_of(name, MOVE)
    for n_orient in (24, 48):
        o, t, n, ties = R.winner(table[:n_orient], 3)
        assert n == count
        assert np.array_equal(R.transform(moved, o, t), g)
        if name == "table":
            assert (o, t) == (16, (-3, -2, 1)) and ties == (2 if n_orient == 24 else 4)
        else:
            assert (o, t) == (18, (3, -2, -1)) and ties == 1


def test_tie_order_field_by_field():
    """|t|^2 before o before (tz, ty, tx), on a table made by hand."""
    t = np.zeros((3, 3, 3, 3), np.int32)
    t[2, 0, 1, 1] = t[1, 1, 1, 2] = t[1, 1, 1, 0] = t[0, 2, 2, 1] = 7       # |t|^2 = 1, 1, 1, 2
    assert R.winner(t, 1)[:3] == (1, (0, 0, -1), 7)
    t[1, 1, 1, 0] = 0
    assert R.winner(t, 1)[:3] == (1, (0, 0, 1), 7)
    t[1, 1, 1, 2] = 0
    assert R.winner(t, 1)[:3] == (2, (-1, 0, 0), 7)
    t[0, 2, 2, 1] = 8
    assert R.winner(t, 1) == (0, (1, 1, 0), 8, 1)


def test_mirror():
    for name, count, reach in (("chair", 244, 230), ("bunny", 1271, 1088)):
        table = table_of(name, MIRROR_MOVE)
        assert R.winner(table[:24], 3)[2] == reach                     # chiral: no rotation matches the mirrored grid
        o, t, n, ties = R.winner(table, 3)
        assert (o, t, n, ties) == (40, (-1, 3, 0), count, 1)
        assert np.array_equal(R.transform(R.transform(small(name), *MIRROR_MOVE), o, t), small(name))


def test_voxels_pushed_out():
    lost = {}
    for name in ("chair", "bunny", "table", "teapot", "suzanne"):
        g = R.pool(R.load_binvox(name), 2)
        moved = R.transform(g, 13, (2, -1, 1))
        lost[name] = int(g.sum() - moved.sum())
        if name in ("chair", "table"):
            words, table = R.align(moved, g, 3, "rotations")
            survivors = int(moved.sum())
            assert words[4] == survivors == {"chair": 1046, "table": 6372}[name]
            assert words[5] == survivors and words[6] == int(g.sum())
            assert words[0] == {"chair": 18, "table": 16}[name]
            assert R.iou(int(words[7]), survivors, int(g.sum())) < 0.2 < R.iou(survivors, survivors, int(g.sum()))
    assert lost["chair"] == 42 and lost["table"] == 1440


def test_degenerate_cases():
    g = small("chair")
    words, table = R.align(g, g, 2, "rotations")
    assert tuple(words[:5]) == (0, 0, 0, 0, 244) and words[7] == 244
    empty = np.zeros_like(g)
    words, table = R.align(empty, empty, 2, "all")
    assert tuple(words) == (0,) * 8 and table.shape == (48, 5, 5, 5) and R.iou(0, 0, 0) == 1.0
    moved = R.transform(g, 13, (0, 0, 0))
    words, table = R.align(moved, g, 0, "rotations")                    # R = 0 scores the orientations alone
    assert table.shape == (24, 1, 1, 1) and tuple(words[:5]) == (18, 0, 0, 0, 244)
    sym = np.zeros((32, 32, 32), bool)
    sym[12:20, 12:20, 12:20] = True                                     # every orientation ties: the identity wins
    assert R.winner(R.scores(sym, sym, 1, 48), 1) == (0, (0, 0, 0), 512, 48)


def test_header_binding_and_argument_errors():
    hdr = open(os.path.join(ROOT, "include", "rendernet_hip.h")).read()
    assert "Voxel registration" in hdr and "WHAT IS SHIFTED OUTSIDE THE GRID IS DROPPED" in hdr
    assert "smallest |t|^2" in hdr and "o = 13 is undone by o = 18" in hdr
    code = re.sub(r"/\*.*?\*/", "", hdr, flags=re.S)
    from rendernet_amd import _lib, build, ops
    for name in ("rn_voxel_orient", "rn_voxel_align_workspace_bytes", "rn_voxel_align"):
        assert re.search(r"\b%s\s*\(" % name, code) and name in _lib.SIGNATURES
    assert "voxel_align.hip" in build.SOURCES
    err = _lib.RenderNetHipError
    import torch
    g = torch.zeros((1, 32, 32, 32), dtype=torch.uint8)
    for kw in ({"max_shift": 17}, {"max_shift": -1}, {"max_shift": 2.0}, {"max_shift": True}, {"orientations": "mirror"},
               {"orientations": 24}, {"threshold": (0.5, 0.5, 0.5)}, {"threshold": float("nan")}):
        with pytest.raises(err, match="voxel_align"):
            ops.voxel_align(g, g, **kw)
    with pytest.raises(err, match="voxel_align"):
        ops.voxel_align(g.numpy(), g)
    with pytest.raises(err, match="HIP tensors"):
        ops.voxel_align(g, g)
    for o, t in ((48, (0, 0, 0)), (-1, (0, 0, 0)), (0, (0, 0)), (0.5, (0, 0, 0)), ([0, 1], (0, 0, 0)), (0, (0, 0, 33))):
        with pytest.raises(err, match="voxel_transform"):
            ops.voxel_transform(g, o, t)
    with pytest.raises(err, match="voxel_transform"):
        ops.voxel_transform(torch.zeros((1, 32, 32, 16)), 0, (0, 0, 0))
