"""Device layer of the prefetching loader (rendernet_amd/loader.py::PrefetchLoader: slots, events, shutdown) and the
script surface `RenderNet_Shader.py <config.json> --train --prefetch N`.  -m gpu."""
import io
import json
import os
import shutil
import threading
import time

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _host_batches(n, fail_at=None):
    """n distinct batches shaped like the loader's; raises inside the iterator at `fail_at`."""
    rng = np.random.default_rng(2)
    out = []
    for i in range(n):
        out.append((rng.integers(0, 256, (2, 64, 64, 3), dtype=np.uint8), rng.integers(0, 2, (2, 64, 64, 64, 1), dtype=np.uint8),
                    rng.random((2, 3)).astype(np.float32), ["s%d_a" % i, "s%d_b" % i]))

    def gen():
        for i, b in enumerate(out):
            if fail_at is not None and i == fail_at:
                raise KeyError("injected into the host iterator")
            yield b
    return out, gen()


def _loader_threads():
    return [t.name for t in threading.enumerate() if t.name.startswith("rn-")]


def _settled(base, seconds=10.0):
    t0 = time.time()
    while threading.active_count() > base and time.time() - t0 < seconds:
        time.sleep(0.02)
    return threading.active_count()


@pytest.mark.parametrize("depth", [1, 2, 3])
def test_slot_protocol(depth):
    """Every clone equals its host batch although (pass 1) the consumer's stream is busy long after the producer is ready to
    overwrite the slot, and (pass 2) the consumer asks as fast as it can.  No synchronise between batches."""
    import torch
    from rendernet_amd.loader import PrefetchLoader
    base = threading.active_count()
    a = torch.randn(4096, 4096, device="cuda")
    for slow in (True, False):
        want, it = _host_batches(13)
        clones = []
        with PrefetchLoader(it, "cuda", depth=depth) as feed:
            for images, voxels, poses, names in feed:
                assert images.dtype == torch.uint8 and images.is_cuda and poses.dtype == torch.float32
                if slow:
                    b = a
                    for _ in range(12):                    # tens of milliseconds of queued work ahead of the clones
                        b = (b @ a) * 1e-3
                clones.append((images.clone(), voxels.clone(), poses.clone(), list(names)))
        torch.cuda.synchronize()
        assert len(clones) == len(want)
        for (gi, gv, gp, gn), (wi, wv, wp, wn) in zip(clones, want):
            assert np.array_equal(gi.cpu().numpy(), wi) and np.array_equal(gv.cpu().numpy(), wv)
            assert np.array_equal(gp.cpu().numpy(), wp) and gn == wn
        assert _settled(base) == base and not _loader_threads()


def test_exceptions_surface_and_threads_end():
    import gc
    import torch
    from rendernet_amd.loader import PrefetchLoader
    base = threading.active_count()
    want, it = _host_batches(8, fail_at=3)
    feed = PrefetchLoader(it, "cuda", depth=2)
    got = [next(feed)[3] for _ in range(3)]
    assert got == [w[3] for w in want[:3]]
    with pytest.raises(KeyError, match="injected"):
        next(feed)
    assert _settled(base) == base
    # leaving early: close(), and garbage collection
    _, it = _host_batches(8)
    feed = PrefetchLoader(it, "cuda", depth=2)
    next(feed)
    feed.close()
    assert _settled(base) == base
    with pytest.raises(StopIteration):
        next(feed)
    _, it = _host_batches(8)
    feed = PrefetchLoader(it, "cuda", depth=2)
    next(feed)
    del feed
    gc.collect()
    assert _settled(base) == base
    for depth in (0, 9):
        with pytest.raises(ValueError):
            PrefetchLoader(iter(()), "cuda", depth=depth)
    torch.cuda.synchronize()


def test_shader_script_trains_with_prefetch(tmp_path, capsys):
    """`--train --max-steps 2 --prefetch 2` on the four-image data set of tests/test_gpu_cli.py: the first step's loss equals
    the unflagged run's up to the summation order of the loss kernel (tests/test_gpu_ingest.py: n * 2^-53 relative, asserted
    at 1e-10; the script prints the float's repr), the second is finite, the checkpoint carries the same 166 variables,
    no loader thread is left."""
    import torch
    from PIL import Image
    import RenderNet_Shader
    from rendernet_amd.tools import utils
    models = tmp_path / "models"
    models.mkdir()
    shutil.copy(os.path.join(ROOT, "binvox", "chair.binvox"), models / "model_chair_abc_clean.binvox")
    shutil.copy(os.path.join(ROOT, "binvox", "table.binvox"), models / "model_chair_xyz_clean.binvox")
    tarp = str(tmp_path / "train.tar")
    w = utils.NpyTarWriter(tarp)
    rng = np.random.default_rng(0)
    for name in ("model_chair_abc_p250_t30_r3.3", "model_chair_xyz_p10_t100_r3.3", "model_chair_abc_p90_t60_r3.3",
                 "model_chair_xyz_p300_t45_r3.3"):
        buf = io.BytesIO()
        Image.fromarray((rng.random((512, 512)) * 255).astype(np.uint8)).save(buf, format="PNG")
        w.add_bytes(buf.getvalue(), name + ".png")
    w.close()
    base = threading.active_count()
    losses, variables = {}, {}
    for tag, extra in (("sync", []), ("prefetch", ["--prefetch", "2"])):
        cfg = {"image_path": tarp, "image_path_valid": "", "model_path": str(models), "is_greyscale": "True", "gpu": 0,
               "batch_size": 2, "max_epochs": 1, "batches_chunk": 1, "threshold": 0.1, "e_eta": 1e-5, "keep_prob": 1.0,
               "decay_steps": 100000, "trained_model_name": "3d2d_renderer", "sample_save": str(tmp_path / ("out_" + tag)),
               "checkpoint_secs": 7200}
        cfgp = str(tmp_path / ("config_%s.json" % tag))
        json.dump(cfg, open(cfgp, "w"))
        torch.manual_seed(0)                               # both runs draw the same crop windows
        RenderNet_Shader.main([cfgp, "--train", "--max-steps", "2"] + extra)
        out = capsys.readouterr().out
        losses[tag] = [float(l.split("Loss")[1]) for l in out.splitlines() if l.startswith("Step")]
        ck = np.load(os.path.join(cfg["sample_save"], "3d2d_renderer.npz"))
        variables[tag] = sorted(k for k in ck.files if not k.startswith("__"))
        assert int(ck["__global_step__"]) == 2
    print("losses", losses)
    assert len(losses["sync"]) == 2 and len(losses["prefetch"]) == 2
    assert abs(losses["prefetch"][0] - losses["sync"][0]) / abs(losses["sync"][0]) <= 1e-10
    assert np.isfinite(losses["prefetch"][1]) and losses["prefetch"][1] > 0
    assert len(variables["prefetch"]) == 166 and variables["prefetch"] == variables["sync"]
    assert _settled(base) == base and not _loader_threads()
