"""rn_voxel_edt / rn_voxel_shape_metrics on the device against the NumPy twin (tests/voxel_edt_ref.py): every voxel and every
word exactly, for the four seed sets at 32, 64 and 128, the word seams, the corners, full and empty grids, batches, the input
forms, determinism, the derived values, the ties to the mesh entries, voxel_offset and the refusals.  -m gpu."""
import functools

import numpy as np
import pytest

import voxel_edt_ref as R

pytestmark = pytest.mark.gpu


def _device(a):
    import torch
    return torch.as_tensor(np.ascontiguousarray(a)).cuda()


@functools.lru_cache(maxsize=None)
def _model(name):
    g = R.load_binvox(name)
    g.setflags(write=False)
    return g


@functools.lru_cache(maxsize=None)
def _twin(name, seeds):
    """The twin's field of a named 64^3 model, computed once per session and left unchanged."""
    if seeds == "signed":
        out = _twin(name, "solid") - _twin(name, "empty")
    else:
        out = R.edt(_model(name), seeds)
    out.setflags(write=False)
    return out


def _same(got, want, what):
    got = got.cpu().numpy()
    assert got.dtype == np.int32 and got.shape == want.shape, (what, got.dtype, got.shape)
    assert np.array_equal(got, want), (what, int((got != want).sum()), got[got != want][:4], want[got != want][:4])


@pytest.mark.parametrize("seeds", R.SEEDS)
def test_device_equals_twin_at_32(seeds):
    import torch
    from rendernet_amd import ops, synth
    csg = ops.voxel_shapes(torch.as_tensor(synth.shape_prims(1234, [0x1a2b3c4d], 32)).cuda(), 32)
    occ = R.occupied(csg.cpu().numpy()[0])
    assert 100 < occ.sum() < 32 ** 3 - 100
    _same(ops.voxel_edt(csg, seeds=seeds), R.edt(occ, seeds)[None], ("csg", seeds))
    small = _model("chair")[::2, ::2, ::2]
    _same(ops.voxel_edt(_device(small.astype(np.uint8)[None]), seeds=seeds), R.edt(small, seeds)[None], ("chair/2", seeds))


@pytest.mark.parametrize("seeds", R.SEEDS)
def test_device_equals_twin_at_64(seeds):
    """Both models in one call, as bytes and as a soft float32 volume at threshold 0.1 whose empty voxels sit ON the threshold."""
    from rendernet_amd import ops
    occ = np.stack([_model("chair"), _model("teapot")])
    want = np.stack([_twin("chair", seeds), _twin("teapot", seeds)])
    _same(ops.voxel_edt(_device(occ.astype(np.uint8)[..., None]), seeds=seeds), want, ("u8", seeds))
    soft = np.where(occ, np.float32(0.2), np.float32(0.1))
    assert np.array_equal(R.occupied(soft, 0.1), occ)
    _same(ops.voxel_edt(_device(soft[..., None]), threshold=0.1, seeds=seeds), want, ("f32", seeds))


@pytest.fixture(scope="module")
def chair128():
    g = np.kron(_model("chair"), np.ones((2, 2, 2), bool))
    g.setflags(write=False)
    return g


@pytest.mark.parametrize("seeds", ["solid", "surface"])
def test_device_equals_twin_at_128(seeds, chair128):
    from rendernet_amd import ops
    _same(ops.voxel_edt(_device(chair128.astype(np.uint8)[None]), seeds=seeds), R.edt(chair128, seeds)[None], seeds)


def _hard_expected(S, seeds):
    """The fields of R.hard_cases(S): closed forms for the lone voxels and the empty grid (tests/test_voxel_edt_cpu.py pins them
    to the twin), the twin for the seams and the full grid."""
    grids = R.hard_cases(S)
    z, y, x = np.meshgrid(np.arange(S), np.arange(S), np.arange(S), indexing="ij")
    out = []
    for g in grids:
        n = int(g.sum())
        if n == 1:
            u = np.argwhere(g)[0]
            d = ((z - u[0]) ** 2 + (y - u[1]) ** 2 + (x - u[2]) ** 2).astype(np.int32)
            out.append({"solid": d, "surface": d, "empty": g.astype(np.int32), "signed": d - g}[seeds])
        elif n == 0:
            out.append(np.full((S, S, S), 0 if seeds == "empty" else R.NONE, np.int32))
        elif n == S ** 3 and seeds == "solid":
            out.append(np.zeros((S, S, S), np.int32))
        else:
            out.append(R.edt(g, seeds))
    return grids, np.stack(out)


@pytest.mark.parametrize("S,seeds", [(64, "solid"), (64, "empty"), (64, "surface"), (64, "signed"), (128, "solid")])
def test_hard_cases_in_one_batched_call(S, seeds):
    """Voxels only at xs 31, 32, 63, 64 (the word seams); a lone voxel in each of the eight corners (the longest scans and the
    largest 16-bit intermediate, 2 (S-1)^2); the centre; full; empty; and the centre again, so that the empty item sits between
    two occupied ones."""
    from rendernet_amd import ops
    grids, want = _hard_expected(S, seeds)
    assert len(grids) == 13 and not grids[-2].any() and grids[-3].all() and grids[-1].any()
    _same(ops.voxel_edt(_device(grids.astype(np.uint8)), seeds=seeds), want, (S, seeds))


def test_input_forms_agree_and_two_calls_give_the_same_bits():
    import torch
    from rendernet_amd import ops
    occ = np.stack([_model("chair"), _model("teapot")]).astype(np.uint8)
    ref = ops.voxel_edt(_device(occ), seeds="signed")
    assert torch.equal(ref, ops.voxel_edt(_device(occ[..., None]), seeds="signed"))
    wide = _device(np.repeat(occ[..., None], 2, axis=4))
    view = wide[..., 1:]                                          # [2,64,64,64,1], stride 2 along xs
    assert not view.is_contiguous() and torch.equal(ref, ops.voxel_edt(view, seeds="signed"))
    swapped = _device(np.ascontiguousarray(occ.transpose(0, 3, 2, 1))).permute(0, 3, 2, 1)
    assert not swapped.is_contiguous() and torch.equal(ref, ops.voxel_edt(swapped, seeds="signed"))
    bits, _ = ops.voxel_pack(_device(occ))
    assert np.array_equal(bits.cpu().numpy(), R.pack(occ.astype(bool)))
    assert torch.equal(ref, ops.voxel_edt(bits=bits, S=64, seeds="signed"))
    again = ops.voxel_edt(_device(occ), seeds="signed")
    assert again.data_ptr() != ref.data_ptr() and torch.equal(ref, again)
    a, b = _device(occ), _device(occ[::-1].copy())
    m1, m2 = ops.voxel_shape_metrics(a, b), ops.voxel_shape_metrics(a, b)
    assert m1.words.data_ptr() != m2.words.data_ptr() and torch.equal(m1.words, m2.words)
    none = ops.voxel_edt(_device(occ[:0]))
    assert tuple(none.shape) == (0, 64, 64, 64) and none.dtype is torch.int32


def _check_metrics(a, b, taus, threshold=0.5):
    from rendernet_amd import ops
    fields = [R.shape_fields(x, y) for x, y in zip(a, b)]
    da, db = _device(a.astype(np.uint8)), _device(b.astype(np.uint8)[..., None])
    for tau in taus:
        tau2 = int(np.floor(tau * tau))
        want = np.stack([R.words_of(f, tau2) for f in fields])
        m = ops.voxel_shape_metrics(da, db, threshold=threshold, tau=tau)
        got = m.words.cpu().numpy()
        assert got.dtype == np.int64 and m.words.is_cuda and m.tau2 == tau2
        assert np.array_equal(got, want), (tau, got, want)
        for name in ("iou", "dice", "chamfer", "chamfer_sq", "hausdorff", "precision", "recall", "fscore"):
            v = getattr(m, name)
            assert v.is_cuda and v.dtype.is_floating_point and v.element_size() == 8
            ref = np.array([R.derived(w)[name] for w in want], np.float64)
            assert np.array_equal(v.cpu().numpy(), ref, equal_nan=True), (tau, name, v.cpu().numpy(), ref)
        assert [d["words"] for d in m.as_dicts()] == want.tolist()
    return want


def test_shape_metrics_of_five_pairs_at_64():
    chair, teapot, nothing = _model("chair"), _model("teapot"), np.zeros((64, 64, 64), bool)
    shifted = np.roll(chair, (2, 1, 0), (0, 1, 2))
    a = np.stack([chair, chair, chair, nothing, chair])
    b = np.stack([teapot, chair, nothing, nothing, shifted])
    want = _check_metrics(a, b, (1.0, 2.5))
    assert want[0, 10] > 6 and 0 < want[0, 2] < want[0, 3]                        # chair against teapot: far apart, overlapping
    assert not want[1, 6:12].any() and want[1, 12] == want[1, 4]                  # against itself
    assert not want[2, 6:].any() and want[2, 4] > 0 and not want[3].any()        # against nothing; nothing against nothing
    assert 0 < want[4, 12] <= want[4, 4] and want[4, 10] >= 1 and want[4, 2] < want[4, 3]   # the shifted copy at tau 2.5


def test_shape_metrics_at_32_and_128(chair128):
    small_c, small_t = _model("chair")[::2, ::2, ::2], _model("teapot")[::2, ::2, ::2]
    _check_metrics(small_c[None], small_t[None], (1.0, 2.5))
    teapot128 = np.kron(_model("teapot"), np.ones((2, 2, 2), bool))
    _check_metrics(chair128[None], teapot128[None], (1.0,))


def test_thresholds_as_a_pair():
    """A reconstruction at 0.1 against a binvox at 0.5."""
    from rendernet_amd import ops
    chair, teapot = _model("chair"), _model("teapot")
    soft = np.where(chair, np.float32(0.3), np.float32(0.05))[None, ..., None]
    m = ops.voxel_shape_metrics(_device(soft), _device(teapot.astype(np.uint8)[None, ..., None]), threshold=(0.1, 0.5))
    assert np.array_equal(m.words.cpu().numpy()[0], R.shape_words(chair, teapot, 1))
    one = ops.voxel_shape_metrics(_device(soft), _device(teapot.astype(np.uint8)[None, ..., None]), threshold=0.5)
    assert int(one.words[0, 0]) == 0                               # at 0.5 the soft chair is empty


def test_mesh_round_trip_scores_one_and_offsets_equal_the_twin():
    from rendernet_amd import ops
    chair = _model("chair")
    dev = _device(chair.astype(np.uint8)[None, ..., None])
    m = ops.extract_mesh(dev, triangles=True)
    back = ops.voxelize_mesh(m.q, m.faces, S=64, mode="solid")
    s = ops.voxel_shape_metrics(back, dev)
    assert s.iou.tolist() == [1.0] and s.hausdorff.tolist() == [0.0] and s.fscore.tolist() == [1.0]
    for radius, want in ((0, chair), (1.5, _twin("chair", "solid") <= 2), (-1, _twin("chair", "empty") > 1)):
        got = ops.voxel_offset(dev, radius)
        assert tuple(got.shape) == (1, 64, 64, 64, 1) and got.dtype.is_floating_point is False and got.element_size() == 1
        assert np.array_equal(got.cpu().numpy()[0, ..., 0].astype(bool), want), radius
    assert ops.voxel_offset(dev, 1.5).sum() > chair.sum() > ops.voxel_offset(dev, -1).sum() > 0


def test_refusals_leave_the_device_usable():
    import torch
    from rendernet_amd import ops
    from rendernet_amd._lib import RenderNetHipError
    chair = _device(_model("chair").astype(np.uint8)[None])
    bad = [lambda: ops.voxel_edt(torch.zeros((1, 48, 48, 48), device="cuda")),
           lambda: ops.voxel_edt(torch.zeros((1, 64, 64, 32), device="cuda")),
           lambda: ops.voxel_edt(chair.cpu()),
           lambda: ops.voxel_edt(chair, seeds="inside"),
           lambda: ops.voxel_edt(bits=torch.zeros((1, 100), dtype=torch.int32, device="cuda"), S=64),
           lambda: ops.voxel_edt(chair, bits=torch.zeros((1, 8192), dtype=torch.int32, device="cuda"), S=64),
           lambda: ops.voxel_shape_metrics(chair, chair[:, ::2, ::2, ::2]),
           lambda: ops.voxel_shape_metrics(chair, torch.cat([chair, chair])),
           lambda: ops.voxel_shape_metrics(chair, chair.cpu()),
           lambda: ops.voxel_shape_metrics(chair, chair, tau=-1.0),
           lambda: ops.voxel_shape_metrics(chair, chair, threshold=(0.1, 0.2, 0.3)),
           lambda: ops.voxel_offset(chair, float("inf"))]
    for k, call in enumerate(bad):
        with pytest.raises(RenderNetHipError):
            call()
        torch.cuda.synchronize()
    m = ops.voxel_shape_metrics(chair[:0], chair[:0])
    assert tuple(m.words.shape) == (0, 16) and tuple(m.iou.shape) == (0,) and m.iou.dtype is torch.float64 and m.as_dicts() == []
    assert tuple(ops.voxel_offset(chair[:0], 1.0).shape) == (0, 64, 64, 64, 1)
    _same(ops.voxel_edt(chair), _twin("chair", "solid")[None], "after the refusals")
