"""The NumPy twin of rn_voxel_label / rn_voxel_label_stats / rn_voxel_topology (tests/voxel_label_ref.py) against what it stands
for: scipy.ndimage.label where scipy is present -- both selected sets, both connectivities, the padding rule of the empty space --
and the closed forms of the rule; and the argument checks of the C entries, which run before any launch and so need no device."""
import ctypes
import functools

import numpy as np
import pytest

import voxel_label_ref as R

# voxels, components, cavities, Euler number, handles (scipy 1.15.3: solid 26-connected, empty 6-connected)
MODEL_WORDS = {"bunny": (57835, 1, 0, 1, 0), "chair": (5277, 1, 0, 0, 1), "suzanne": (30270, 1, 0, 1, 0), "table": (61087, 1, 0, -1, 2),
               "teapot": (27933, 1, 0, 0, 1)}


@functools.lru_cache(maxsize=None)
def _model(name):
    g = R.load_binvox(name)
    g.setflags(write=False)
    return g


def _scipy_solid(ndi, occ, connectivity):
    return ndi.label(occ, np.ones((3, 3, 3), bool) if connectivity == 26 else ndi.generate_binary_structure(3, 1))


def _scipy_empty(ndi, occ, connectivity):
    """scipy's labels of the complement padded by one empty layer, cropped and renumbered: the outside 1, the cavities 2.. in
    scipy's own order (ascending first voxel)."""
    lab, n = _scipy_solid(ndi, np.pad(~occ, 1, constant_values=True), connectivity)
    outside = lab[0, 0, 0]
    lab = lab[1:-1, 1:-1, 1:-1]
    cavities = [k for k in range(1, n + 1) if k != outside]
    number = np.zeros(n + 1, np.int32)
    number[outside] = 1
    number[cavities] = np.arange(len(cavities)) + 2
    return number[lab], len(cavities)


def _against_scipy(ndi, occ, what):
    for connectivity in (26, 6):
        lab, k = R.label(occ, "solid", connectivity)
        want, kw = _scipy_solid(ndi, occ, connectivity)
        assert k == kw and lab.dtype == np.int32 and np.array_equal(lab, want), (what, "solid", connectivity, k, kw)
        lab, k = R.label(occ, "empty", connectivity)
        want, kw = _scipy_empty(ndi, occ, connectivity)
        assert k == kw and np.array_equal(lab, want), (what, "empty", connectivity, k, kw)


@pytest.mark.parametrize("name", R.MODELS)
def test_twin_equals_scipy_on_the_models(name):
    ndi = pytest.importorskip("scipy.ndimage")
    _against_scipy(ndi, _model(name), name)


def test_twin_equals_scipy_on_random_grids():
    ndi = pytest.importorskip("scipy.ndimage")
    counts = []
    for density, g in zip((0.05, 0.2, 0.5), R.random_grids(32)):
        _against_scipy(ndi, g, density)
        counts.append((R.label(g, "solid", 26)[1], R.label(g, "solid", 6)[1]))
        w = R.topology(g)
        assert 0 <= w[7] <= 2371 and w[7] == w[1] + w[2] - w[6]
    assert counts == [(800, 1451), (76, 2929), (1, 362)]


def test_twin_equals_scipy_on_the_closed_forms():
    ndi = pytest.importorskip("scipy.ndimage")
    for name, g in R.closed_forms_32():
        _against_scipy(ndi, g, name)


def test_numbering_is_by_ascending_first_voxel():
    for g in [_model("chair")] + R.random_grids(32):
        for of, connectivity in (("solid", 26), ("solid", 6), ("empty", 6), ("empty", 26)):
            lab, k = R.label(g, of, connectivity)
            low = 2 if of == "empty" else 1
            firsts = [int(np.flatnonzero(lab.ravel() == j)[0]) for j in range(low, low + k)]
            assert firsts == sorted(firsts) and lab.max() <= low + k - 1


def _words(g):
    w = R.topology(g)
    return dict(n=int(w[0]), components=int(w[1]), cavities=int(w[2]), euler=int(w[6]), handles=int(w[7]))


def test_closed_forms_at_32():
    S = 32
    forms = dict(R.closed_forms_32())
    assert R.label(forms["empty"], "solid", 26)[1] == 0 and R.label(forms["empty"], "solid", 6)[1] == 0
    lab, k = R.label(forms["empty"], "empty", 6)
    assert k == 0 and (lab == 1).all()                           # the outside component is label 1
    w = _words(forms["full"])
    assert (w["components"], w["cavities"], w["euler"], w["handles"]) == (1, 0, 1, 0)
    lab, k = R.label(forms["full"], "empty", 6)
    assert k == 0 and not lab.any()                               # label 1 exists also when no empty voxel touches the border
    assert np.array_equal(R.components([forms["full"]], "empty", 6)[3], [[0, S ** 3, S, S, S, -1, -1, -1]])
    for name in ("corner pair", "edge pair"):
        assert R.label(forms[name], "solid", 26)[1] == 1 and R.label(forms[name], "solid", 6)[1] == 2, name
    assert R.label(forms["pitfall"], "solid", 26)[1] == 1 and R.label(forms["pitfall"], "solid", 6)[1] == 3
    w = _words(forms["checkerboard"])
    assert (w["components"], w["cavities"], w["euler"], w["handles"]) == (1, 13500, 13501, 0)
    assert R.label(forms["checkerboard"], "solid", 6)[1] == 16384
    w = _words(forms["hollow box"])
    assert (w["components"], w["cavities"], w["euler"], w["handles"]) == (1, 1, 2, 0)
    assert R.label(forms["open corner"], "empty", 6)[1] == 1 and R.label(forms["open corner"], "empty", 26)[1] == 0
    assert R.label(forms["open corner"], "solid", 26)[1] == 1 and R.label(forms["open corner"], "solid", 6)[1] == 1
    w = _words(forms["nested shells"])
    assert (w["components"], w["cavities"], w["euler"]) == (3, 2, 5)
    labels, counts, offsets, stats = R.components([forms["nested shells"]])
    assert counts.tolist() == [3] and offsets.tolist() == [0, 3] and stats[:, 0].tolist() == [1352, 296, 8]
    assert stats[0].tolist() == [1352, (4 * S + 4) * S + 4, 4, 4, 4, 19, 19, 19] and stats[2, 2:].tolist() == [11, 11, 11, 12, 12, 12]
    cleaned, dropped = R.clean(forms["nested shells"])
    assert np.array_equal(cleaned, R.box(S, 4, 20)) and dropped == [296, 8]
    w = _words(forms["cube edges"])
    assert (w["components"], w["cavities"], w["euler"], w["handles"]) == (1, 0, -4, 5)
    snake = forms["serpentine"]
    assert R.label(snake, "solid", 26)[1] == 1 and R.label(snake, "solid", 6)[1] == 1 and _words(snake)["handles"] == 0
    assert snake.sum() == 16 * 16 * 32 + 16 * 15 + 15           # every second row of every second plane, and the links


@pytest.mark.parametrize("name", R.MODELS)
def test_topology_words_of_the_models(name):
    w = _words(_model(name))
    assert (w["n"], w["components"], w["cavities"], w["euler"], w["handles"]) == MODEL_WORDS[name]


def test_cell_counts_and_clean():
    one = np.zeros((32, 32, 32), bool)
    one[31, 0, 31] = True                                         # a corner voxel: its cube's cells lie on the grid's hull
    assert R.cell_counts(one) == (8, 12, 6) and R.topology(one).tolist() == [1, 1, 0, 8, 12, 6, 1, 0]
    assert R.cell_counts(R.box(32, 0, 32)) == (33 ** 3, 3 * 32 * 33 * 33, 3 * 32 * 32 * 33)
    chair = _model("chair")
    dirty = chair.copy()
    assert not dirty[2:5, 2:5, 2:5].any() and not dirty[60, 60, 60] and not dirty[2, 60, 2:4].any()
    dirty[3, 3, 3] = dirty[60, 60, 60] = dirty[2, 60, 2:4] = True   # three specks
    cleaned, dropped = R.clean(dirty)
    assert np.array_equal(cleaned, chair) and sorted(dropped) == [1, 1, 2]
    assert np.array_equal(R.clean(dirty, keep_largest=None, min_voxels=2)[0], _two(dirty)) and _two(dirty).sum() == chair.sum() + 2
    assert np.array_equal(R.clean(dirty, keep_largest=0, fill_cavities=False)[0], dirty)
    # equal sizes: the lower label wins
    two = R.pair(32, (5, 5, 5), (0, 0, 9))
    assert np.argwhere(R.clean(two)[0]).tolist() == [[5, 5, 5]]


def _two(dirty):
    """The voxels of `dirty` in components of at least two voxels."""
    lab, k = R.label(dirty, "solid", 26)
    size = np.bincount(lab.ravel(), minlength=k + 1)
    return (size[lab] >= 2) & dirty


def test_pack_is_the_bit_order_of_the_header():
    occ = np.zeros((1, 32, 32, 32), bool)
    occ[0, 1, 2, 3] = occ[0, 0, 0, 31] = True
    bits = R.pack(occ).view(np.uint32)
    i = (1 * 32 + 2) * 32 + 3
    assert bits[0, i >> 5] == 1 << (i & 31) and bits[0, 0] == 1 << 31 and int((bits != 0).sum()) == 2


def test_workspace_sizes_and_refusals_without_a_device():
    """rn_voxel_label, rn_voxel_label_stats and rn_voxel_topology check every argument before any launch."""
    from rendernet_amd import _lib as L
    lib = L.lib()
    for B, S in ((1, 32), (24, 64), (1, 128), (3, 128)):
        v = B * S ** 3
        totals = (v // 256 * 4 + 15) // 16 * 16
        assert lib.rn_voxel_label_workspace_bytes(B, S) == 8 * v + totals <= 8 * v + v // 64 + 16
        assert lib.rn_voxel_topology_workspace_bytes(B, S) == 8 * v
    assert lib.rn_voxel_label_workspace_bytes(0, 64) == 0
    assert lib.rn_voxel_label_workspace_bytes(1, 48) == 0 and b"S=48" in lib.rn_last_error()
    assert lib.rn_voxel_label_workspace_bytes(65536, 64) == 0 and b"B=65536" in lib.rn_last_error()
    assert lib.rn_voxel_topology_workspace_bytes(-1, 64) == 0 and b"B=-1" in lib.rn_last_error()
    buf = (ctypes.c_char * 64)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 15) & ~15)
    odd, odd8 = ctypes.c_void_p(p.value + 4), ctypes.c_void_p(p.value + 2)
    big = 1 << 40
    label = lambda B=1, S=32, of=0, c=26, bits=p, labels=p, counts=p, ws=p, n=big: lib.rn_voxel_label(bits, B, S, of, c, labels, counts, ws, n, None)
    need = 8 * 32 ** 3 + 32 ** 3 // 64
    for kw, text in ((dict(S=48), b"S=48"), (dict(S=256), b"S=256"), (dict(B=-1), b"B=-1"), (dict(B=65536), b"B=65536"),
                     (dict(of=2), b"of_empty=2"), (dict(of=-1), b"of_empty=-1"), (dict(c=18), b"connectivity=18"),
                     (dict(c=0), b"connectivity=0"), (dict(bits=None), b"null"), (dict(labels=None), b"null"),
                     (dict(counts=None), b"null"), (dict(ws=None), b"null"), (dict(ws=odd), b"16-byte"), (dict(bits=odd), b"16-byte"),
                     (dict(labels=odd8), b"4-byte"), (dict(n=need - 1), b"%d needed" % need)):
        assert label(**kw) == -1 and b"rn_voxel_label:" in lib.rn_last_error() and text in lib.rn_last_error(), (kw, lib.rn_last_error())
    stats = lambda B=1, S=32, of=0, labels=p, offsets=p, out=p: lib.rn_voxel_label_stats(labels, offsets, B, S, of, out, None)
    for kw, text in ((dict(S=96), b"S=96"), (dict(B=70000), b"B=70000"), (dict(of=3), b"of_empty=3"), (dict(labels=None), b"null"),
                     (dict(offsets=None), b"null"), (dict(out=None), b"null"), (dict(offsets=odd), b"8-byte"), (dict(out=odd), b"16-byte")):
        assert stats(**kw) == -1 and b"rn_voxel_label_stats:" in lib.rn_last_error() and text in lib.rn_last_error(), (kw, lib.rn_last_error())
    topo = lambda B=1, S=32, bits=p, out=p, ws=p, n=big: lib.rn_voxel_topology(bits, B, S, out, ws, n, None)
    for kw, text in ((dict(S=16), b"S=16"), (dict(B=65536), b"B=65536"), (dict(bits=None), b"null"), (dict(out=None), b"null"),
                     (dict(ws=None), b"null"), (dict(out=odd), b"8-byte"), (dict(ws=odd), b"16-byte"), (dict(n=262143), b"262144 needed")):
        assert topo(**kw) == -1 and b"rn_voxel_topology:" in lib.rn_last_error() and text in lib.rn_last_error(), (kw, lib.rn_last_error())
    assert label(B=0, bits=None, labels=None, counts=None, ws=None, n=0) == 0
    assert stats(B=0, labels=None, offsets=None, out=None) == 0 and topo(B=0, bits=None, out=None, ws=None, n=0) == 0


def test_ops_refuse_host_tensors_and_bad_arguments():
    import torch
    from rendernet_amd import ops
    from rendernet_amd._lib import RenderNetHipError
    g = torch.zeros((1, 32, 32, 32, 1))
    for call in (lambda: ops.voxel_components(g), lambda: ops.voxel_clean(g), lambda: ops.voxel_topology(g),
                 lambda: ops.voxel_components(g, of="hollow"), lambda: ops.voxel_components(g, connectivity=18),
                 lambda: ops.voxel_components(g, connectivity=26.0), lambda: ops.voxel_components(),
                 lambda: ops.voxel_clean(g, keep_largest=-1), lambda: ops.voxel_clean(g, min_voxels=0),
                 lambda: ops.voxel_clean(g, min_voxels=1.5), lambda: ops.voxel_clean(g, connectivity=18),
                 lambda: ops.voxel_topology(bits=torch.zeros((1, 1024), dtype=torch.int32), S=32)):
        with pytest.raises(RenderNetHipError):
            call()
