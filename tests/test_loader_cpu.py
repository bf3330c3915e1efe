"""Host layer of the prefetching uint8 loader (rendernet_amd/loader.py) against the composition it replaces:
`tools.data_util.data_loader` + `images / 255.0` + the script's `len(images) // batch_size` slices + the rank's shard.
Synthetic tars at img_res 32; no GPU."""
import io
import os
import shutil
import threading
import time

import numpy as np
import pytest

from conftest import ROOT

RES = 32
CFG = {"batch_size": 4, "batches_chunk": 2}
RANKS = ((0, 1), (0, 2), (1, 2), (3, 4))
# images per tar: exact multiple of the chunk (8) | tail shorter than a batch | tail of exactly one batch |
# tail longer than a batch and not a multiple | fewer images than one batch
COUNTS = (16, 18, 20, 22, 3)
SHAPES = {"L": (RES, RES), "RGB": (RES, RES, 3), "RGBA": (RES, RES, 4)}


def _png(rng, mode):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray((rng.random(SHAPES[mode]) * 255).astype(np.uint8)).save(buf, format="PNG")
    return buf.getvalue()


def _names(n):
    return ["model_chair_%s_p%d_t%d_r3.3" % (("xyz", "abc", "klm")[i % 3], 10 * i, 30 + i) for i in range(n)]


@pytest.fixture()
def models(tmp_path):
    d = tmp_path / "models"
    d.mkdir()
    for ident, src in (("abc", "chair"), ("xyz", "table"), ("klm", "teapot")):
        shutil.copy(os.path.join(ROOT, "binvox", src + ".binvox"), d / ("model_chair_%s_clean.binvox" % ident))
    return str(d)


def _tar(tmp_path, n, mode, spoil=None, seed=0):
    """n PNG members of `mode`; spoil = (index, "garbage" | "truncated") damages one member."""
    from rendernet_amd.tools import utils
    path = str(tmp_path / ("set_%d_%s_%s.tar" % (n, mode, spoil[1] if spoil else "ok")))
    w = utils.NpyTarWriter(path)
    rng = np.random.default_rng(seed)
    for i, name in enumerate(_names(n)):
        payload = _png(rng, mode)
        if spoil and i == spoil[0]:
            payload = b"not an image at all " * 8 if spoil[1] == "garbage" else payload[:len(payload) // 2]
        w.add_bytes(payload, name + ".png")
    w.close()
    return path


def _todays_batches(cfg, tar, models, flatten):
    """What RenderNet_Shader.py trains on today, step by step (global batches, before the rank's shard)."""
    from rendernet_amd.tools import data_util
    bs, out = cfg["batch_size"], []
    for images, mods, params, names in data_util.data_loader(cfg, tar, models, flatten=flatten, img_res=RES):
        images = images / 255.0
        for idx in range(len(images) // bs):
            sl = slice(idx * bs, (idx + 1) * bs)
            out.append((images[sl].copy(), mods[sl].copy(), params[sl].copy(), [str(n) for n in names[sl]]))
    return out


def _assert_same_sequence(got, want, rank, world, flatten):
    from rendernet_amd import ops
    from rendernet_amd.parallel import shard_range
    lo, hi = shard_range(CFG["batch_size"], rank, world)
    assert len(got) == len(want)
    for (gi, gv, gp, gn), (wi, wv, wp, wn) in zip(got, want):
        assert gi.dtype == np.uint8 and gv.dtype == np.uint8 and gp.dtype == np.float32
        assert gv.shape == (hi - lo, 64, 64, 64, 1) and gi.shape[:3] == (hi - lo, RES, RES)
        tgt = ops.target_u8_crop_reference(gi, (0, 0, RES, RES), 1 if flatten else 3)
        assert tgt.dtype == np.float32 and np.array_equal(tgt, wi[lo:hi])
        assert np.array_equal(gv.astype(np.float32), wv[lo:hi])
        assert np.array_equal(gp, wp[lo:hi])
        assert list(gn) == wn[lo:hi]


@pytest.mark.parametrize("mode,flatten", [("RGB", True), ("RGBA", True), ("L", True), ("RGB", False), ("RGBA", False)])
def test_same_batches_same_order(tmp_path, models, mode, flatten):
    from rendernet_amd import loader
    for n in COUNTS:
        tar = _tar(tmp_path, n, mode, seed=n)
        want = _todays_batches(CFG, tar, models, flatten)
        assert len(want) == {16: 4, 18: 5, 20: 5, 22: 5, 3: 1}[n]          # 22: the six-sample tail is cut to one batch
        for rank, world in RANKS:
            got = list(loader.iter_host_batches(CFG, tar, models, flatten, RES, rank=rank, world=world, workers=3))
            _assert_same_sequence(got, want, rank, world, flatten)


def test_skips_agree(tmp_path, models):
    from rendernet_amd import loader
    from rendernet_amd.parallel import shard_range
    # garbage bytes: the header does not open -> skipped on every rank of every world size, as the generator skips it
    tar = _tar(tmp_path, 18, "RGB", spoil=(5, "garbage"))
    want = _todays_batches(CFG, tar, models, True)
    assert all(_names(18)[5] not in names for _, _, _, names in want) and len(want) == 5      # 17 samples: two chunks + a tail of one
    for rank, world in RANKS:
        got = list(loader.iter_host_batches(CFG, tar, models, True, RES, rank=rank, world=world, workers=2))
        _assert_same_sequence(got, want, rank, world, True)
    # valid header, truncated pixels: skipped like today with one rank; with more, the owner raises and names the member
    tar = _tar(tmp_path, 18, "RGB", spoil=(5, "truncated"))
    want = _todays_batches(CFG, tar, models, True)
    assert all(_names(18)[5] not in names for _, _, _, names in want)
    got = list(loader.iter_host_batches(CFG, tar, models, True, RES, workers=2))
    _assert_same_sequence(got, want, 0, 1, True)
    for world in (2, 4):
        owner = [r for r in range(world) if shard_range(4, r, world)[0] <= 5 % 4 < shard_range(4, r, world)[1]][0]
        with pytest.raises(RuntimeError, match=_names(18)[5]):
            list(loader.iter_host_batches(CFG, tar, models, True, RES, rank=owner, world=world, workers=2))


def test_shard_before_decode_and_one_read_per_model(tmp_path, models, monkeypatch):
    from rendernet_amd import loader
    lock, counts = threading.Lock(), {"decode": 0, "binvox": []}
    real_decode, real_binvox = loader._decode_pixels, loader._read_binvox

    def decode(raw):
        with lock:
            counts["decode"] += 1
        return real_decode(raw)

    def binvox(path):
        with lock:
            counts["binvox"].append(path)
        return real_binvox(path)

    monkeypatch.setattr(loader, "_decode_pixels", decode)
    monkeypatch.setattr(loader, "_read_binvox", binvox)
    tar = _tar(tmp_path, 32, "RGB")                      # four full chunks: no tail rule in play
    for rank, world in ((2, 4), (0, 1)):
        counts["decode"], counts["binvox"] = 0, []
        got = list(loader.iter_host_batches(CFG, tar, models, True, RES, rank=rank, world=world, workers=4))
        distinct = set(n for b in got for n in b[3])
        assert len(distinct) == 32 // world
        assert counts["decode"] == len(distinct)         # not world x
        assert len(counts["binvox"]) == len(set(counts["binvox"])) <= 3      # each model file once, 32 images refer to 3
    # a tail may cost the decodes this rank made before the end of the tar re-dealt the batch: bounded by its shard
    tar = _tar(tmp_path, 19, "RGB")                      # two chunks + 3 -> repeated up to one batch
    counts["decode"] = 0
    got = list(loader.iter_host_batches(CFG, tar, models, True, RES, rank=1, world=4, workers=4))
    distinct = set(n for b in got for n in b[3])
    assert len(distinct) <= counts["decode"] <= len(distinct) + 1


def test_reference_twin_is_exhaustive():
    """Every channel sum (0..765 for three channels, 0..1020 for four) and every byte: the twin equals the NumPy expressions
    of data_loader followed by `/ 255.0`, bit for bit."""
    from rendernet_amd import ops
    for cs in (3, 4):
        sums = np.arange(255 * cs + 1)
        img = np.zeros((1, len(sums), cs), np.uint8)
        for k in range(cs):                              # spread each sum over the channels: min(255, what is left)
            img[0, :, k] = np.clip(sums - 255 * k, 0, 255)
        assert np.array_equal(img.astype(np.int64).sum(2)[0], sums)
        f32 = img.astype(np.float32)                     # what NpyTarReader hands data_loader
        want_grey = np.reshape(np.mean(f32, axis=2), (1, len(sums), 1)) / 255.0
        want_rgb = np.reshape(f32[:, :, :3], (1, len(sums), 3)) / 255.0
        for perm in (list(range(cs)), list(range(cs))[::-1]):
            got = ops.target_u8_crop_reference(img[None][..., perm], (0, 0, 1, len(sums)), 1)
            assert got.dtype == np.float32 and np.array_equal(got[0], want_grey)
        assert np.array_equal(ops.target_u8_crop_reference(img[None], (0, 0, 1, len(sums)), 3)[0], want_rgb)
    byte = np.arange(256, dtype=np.uint8).reshape(1, 16, 16, 1)
    want = np.reshape(byte[0, :, :, 0].astype(np.float32), (16, 16, 1)) / 255.0
    assert np.array_equal(ops.target_u8_crop_reference(byte, (0, 0, 16, 16), 1)[0], want)
    # the window is the trainer's slice
    assert np.array_equal(ops.target_u8_crop_reference(byte, (4, 8, 8, 4), 1)[0], want[4:12, 8:12])
    for bad in ((0, 0, 17, 16), (-1, 0, 4, 4), (0, 13, 4, 4), (0, 0, 0, 4)):
        with pytest.raises(ValueError):
            ops.target_u8_crop_reference(byte, bad, 1)
    with pytest.raises(ValueError):
        ops.target_u8_crop_reference(byte, (0, 0, 4, 4), 3)          # colour from a single channel
    with pytest.raises(ValueError):
        ops.target_u8_crop_reference(byte.astype(np.float32), (0, 0, 4, 4), 1)


def _wait_for_threads(base, seconds=10.0):
    t0 = time.time()
    while threading.active_count() > base and time.time() - t0 < seconds:
        time.sleep(0.02)
    return threading.active_count()


def test_shutdown_and_worker_exception(tmp_path, models, monkeypatch):
    import gc
    from rendernet_amd import loader
    tar = _tar(tmp_path, 40, "RGB")
    base = threading.active_count()
    it = loader.iter_host_batches(CFG, tar, models, True, RES, workers=4)
    first = next(it)
    assert first[0].shape == (4, RES, RES, 3) and threading.active_count() > base
    it.close()                                           # what leaving a `with closing(...)` block does
    assert _wait_for_threads(base) == base
    it = loader.iter_host_batches(CFG, tar, models, True, RES, workers=4)
    next(it)
    del it                                               # ... and what dropping the last reference does
    gc.collect()
    assert _wait_for_threads(base) == base

    real = loader._decode_pixels
    seen = []

    def explode(raw):
        seen.append(1)
        if len(seen) == 6:
            raise KeyError("injected into a decode worker")
        return real(raw)

    monkeypatch.setattr(loader, "_decode_pixels", explode)
    with pytest.raises(KeyError, match="injected"):
        list(loader.iter_host_batches(CFG, tar, models, True, RES, workers=4))
    assert _wait_for_threads(base) == base


def test_arguments_are_refused(tmp_path, models):
    from rendernet_amd import loader
    tar = _tar(tmp_path, 8, "RGB")
    with pytest.raises(ValueError, match="add_noise"):
        loader.iter_host_batches(CFG, tar, models, True, RES, add_noise=True)
    for w in (0, 17):
        with pytest.raises(ValueError, match="workers"):
            loader.iter_host_batches(CFG, tar, models, True, RES, workers=w)
    with pytest.raises(ValueError):
        loader.iter_host_batches(CFG, tar, models, True, RES, rank=2, world=2)
    with pytest.raises(ValueError):
        loader.iter_host_batches(CFG, tar, models, True, RES, rank=0, world=3)      # 4 frames over 3 ranks
    # one batch is one channel count
    from rendernet_amd.tools import utils
    mixed = str(tmp_path / "mixed.tar")
    w = utils.NpyTarWriter(mixed)
    rng = np.random.default_rng(3)
    for i, name in enumerate(_names(8)):
        w.add_bytes(_png(rng, "RGBA" if i == 6 else "RGB"), name + ".png")
    w.close()
    with pytest.raises(ValueError, match=_names(8)[6]):
        list(loader.iter_host_batches(CFG, mixed, models, True, RES))
    with pytest.raises(ValueError, match="shape"):
        list(loader.iter_host_batches(CFG, tar, models, True, 2 * RES))


def test_prefetch_flag_parsing_and_default_path(monkeypatch):
    import RenderNet_Shader as script
    from rendernet_amd import loader
    from rendernet_amd.tools import data_util
    assert script.prefetch_options({}, ["cfg.json", "--train"]) == (0, 4)
    assert script.prefetch_options({"prefetch_batches": 3, "loader_workers": 8}, ["cfg.json", "--train"]) == (3, 8)
    assert script.prefetch_options({"prefetch_batches": 3}, ["cfg.json", "--train", "--prefetch", "0"]) == (0, 4)
    assert script.prefetch_options({}, ["cfg.json", "--train", "--prefetch", "2", "--loader-workers", "16"]) == (2, 16)
    for argv in (["--prefetch"], ["--prefetch", "two"], ["--prefetch", "-1"], ["--prefetch", "9"], ["--prefetch", "1.5"],
                 ["--loader-workers", "0"], ["--loader-workers", "17"]):
        with pytest.raises(SystemExit):
            script.prefetch_options({}, ["cfg.json", "--train"] + argv)
    for cfg in ({"prefetch_batches": "many"}, {"prefetch_batches": 2.5}, {"prefetch_batches": True}, {"loader_workers": 64}):
        with pytest.raises(SystemExit):
            script.prefetch_options(cfg, ["cfg.json", "--train"])

    # N = 0 takes the synchronous generator and never touches the new module
    calls = []

    def fake_data_loader(cfg, img_path, model_path, validation_mode=False, flatten=False, img_res=256, add_noise=False):
        calls.append((img_path, flatten, img_res, validation_mode))
        yield (np.full((4, 8, 8, 1), 255.0, np.float32), np.ones((4, 2, 2, 2, 1), np.float32),
               np.arange(12, dtype=np.float32).reshape(4, 3), ["a", "b", "c", "d"])

    def forbidden(*a, **k):
        raise AssertionError("the prefetching loader must not be used without --prefetch")

    monkeypatch.setattr(data_util, "data_loader", fake_data_loader)
    monkeypatch.setattr(loader, "iter_host_batches", forbidden)
    monkeypatch.setattr(loader, "PrefetchLoader", forbidden)
    cfg = {"batch_size": 2, "batches_chunk": 2, "image_path": "train.tar", "model_path": "models"}
    got = list(script._training_batches(cfg, True, 8, 1, 2, "cuda:0", 0, 4))
    assert calls == [("train.tar", True, 8, False)] and len(got) == 2
    models, params, images, names = got[1]                                   # second batch, rank 1 of 2: sample 3
    assert names == ["d"] and np.array_equal(params, [[9.0, 10.0, 11.0]]) and images.dtype == np.float32
    assert np.array_equal(images, np.ones((1, 8, 8, 1), np.float32)) and models.shape == (1, 2, 2, 2, 1)
    with pytest.raises(AssertionError, match="must not be used"):
        list(script._training_batches(cfg, True, 8, 0, 1, "cuda:0", 2, 4))    # and N >= 1 does go there
