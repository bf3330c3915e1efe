#!/usr/bin/env python
"""Where the training script's time goes between the tar and the step: decode rate, delivered rate, loader-fed ms/step
of the synchronous loader against the prefetching uint8 loader, and the ingest kernel.

The data set is built from a seed inside the tree: the five shipped binvox models rendered by the project's own Renderer at
the 72 poses of `RenderNet_demo.py --rotate`, saved as 512^2 greyscale PNGs into a tar (random-noise PNGs would mis-state
the decode cost: they do not compress).

Stages, one process each so that a job can give each its own time limit and chain them with `&&`; every stage writes
<work>/<stage>.json and `report` prints the merged result as ONE JSON line (and writes it to --out):

    python scripts/loader_bench.py dataset --work DIR          # GPU: render + write the tar
    python scripts/loader_bench.py decode  --work DIR          # host: decode-only samples/s, workers 1 / 4 / 8
    python scripts/loader_bench.py deliver --work DIR          # GPU: PrefetchLoader, consumer only waits on the events
    python scripts/loader_bench.py train   --work DIR          # GPU: ms/step of the script's loop, legs a b a b
    python scripts/loader_bench.py ingest  --work DIR          # GPU: the ingest kernel alone (run it under
                                                               #      `rocprofv3 --kernel-trace --stats` for the trace time)
    python scripts/loader_bench.py report  --work DIR [--kernel-stats CSV] [--step-alone-ms MS] --out profiles/loader_bench.json
"""
import argparse
import csv
import io
import json
import os
import shutil
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

MODELS = ("chair", "bunny", "table", "suzanne", "teapot")
BATCH, CROP = 24, 64
HBM_PEAK = 8.0e12                                       # bytes/s, MI355X


def _cfg(work, batches_chunk):
    return {"image_path": os.path.join(work, "train.tar"), "model_path": os.path.join(work, "models"), "batch_size": BATCH,
            "batches_chunk": batches_chunk, "is_greyscale": "True"}


def _save(work, stage, result):
    with open(os.path.join(work, stage + ".json"), "w") as f:
        json.dump(result, f)
    print(json.dumps({stage: result}), flush=True)


def stage_dataset(a):
    from PIL import Image
    from rendernet_amd.shader import Renderer, ShaderSpec, init_shader_weights
    from rendernet_amd.tools import binvox_rw, utils
    mdir = os.path.join(a.work, "models")
    os.makedirs(mdir, exist_ok=True)
    spec = ShaderSpec(out_ch=1).check()
    renderer = Renderer(spec, init_shader_weights(spec, seed=1234))
    members = {}
    for k, m in enumerate(MODELS):
        ident = "k%d" % k                               # not the model's name: "_table" / "_teapot" would read as the "_t" pose field
        shutil.copy(os.path.join(ROOT, "binvox", m + ".binvox"), os.path.join(mdir, "model_chair_%s_clean.binvox" % ident))
        with open(os.path.join(ROOT, "binvox", m + ".binvox"), "rb") as f:
            vox = binvox_rw.read_as_3d_array(f).data.astype(np.float32)[None, ..., None]
        for s in range(0, 72, BATCH):
            az = np.arange(s, s + BATCH) * 5.0
            poses = np.stack([az * np.pi / 180, np.full(BATCH, 30 * np.pi / 180), np.ones(BATCH)], 1).astype(np.float32)
            out = renderer.run("encoder/output:0", {"real_model_in:0": np.repeat(vox, BATCH, 0), "view_name:0": poses,
                                                    "patch_size:0": 128, "is_training:0": False})
            for deg, img in zip(az, out):
                buf = io.BytesIO()
                Image.fromarray(np.squeeze(np.clip(255 * img, 0, 255).astype(np.uint8))).save(buf, format="PNG")
                members["model_chair_%s_p%d_t60_r3.3" % (ident, int(deg))] = buf.getvalue()
    # interleave the models as a shuffled render set would: pose-major order
    names = sorted(members, key=lambda n: (int(n.split("_p")[1].split("_")[0]), n))
    w = utils.NpyTarWriter(os.path.join(a.work, "train.tar"))
    for n in names:
        w.add_bytes(members[n], n + ".png")
    w.close()
    sizes = [len(v) for v in members.values()]
    _save(a.work, "dataset", {"images": len(names), "png_bytes_mean": float(np.mean(sizes)), "png_bytes_max": int(max(sizes))})


def stage_decode(a):
    from rendernet_amd import loader
    cfg, res = _cfg(a.work, a.batches_chunk), {}
    for workers in (0, 1, 4, 8):                        # 0: an untimed first pass (page cache, PIL's plug-ins)
        t0, n = time.perf_counter(), 0
        for images, _, _, _ in loader.iter_host_batches(cfg, cfg["image_path"], cfg["model_path"], True, 512,
                                                        workers=max(1, workers)):
            n += len(images)
        if workers:
            res["workers_%d" % workers] = n / (time.perf_counter() - t0)
    _save(a.work, "decode", {"samples_per_s": res, "samples": n})


def stage_deliver(a):
    import torch
    from rendernet_amd import loader
    cfg = _cfg(a.work, a.batches_chunk)
    res = {}
    for workers in (0, 4, 8):                           # 0: an untimed first pass (runtime start-up, first pinned allocation)
        t0, n = time.perf_counter(), 0
        host = loader.iter_host_batches(cfg, cfg["image_path"], cfg["model_path"], True, 512, workers=max(1, workers))
        with loader.PrefetchLoader(host, "cuda", depth=2) as feed:
            for images, _, _, _ in feed:                # the wait on the slot's event is all the consumer does
                n += images.shape[0]
        torch.cuda.synchronize()
        if workers:
            res["workers_%d" % workers] = n / (time.perf_counter() - t0)
    _save(a.work, "deliver", {"samples_per_s": res, "samples": n, "depth": 2})


def stage_train(a):
    """The loop of RenderNet_Shader.train on one GPU: window draw, Trainer.step, loss.item() -- fed by the script's own
    batch source with --prefetch 0 (a) and --prefetch N (b), alternating a b a b on one trainer; then leg c, the same loop on
    one resident uint8 device batch (no loader at all): what the loop itself costs above bench.py's step, which does not
    read the loss back every step."""
    import torch
    import RenderNet_Shader as script
    from rendernet_amd.shader import ShaderSpec, init_shader_weights
    from rendernet_amd.train import Trainer
    cfg = _cfg(a.work, a.batches_chunk)
    spec = ShaderSpec(out_ch=1).check()
    tr = Trainer(spec, init_shader_weights(spec, seed=1234), keep_prob=0.75)
    legs, resident = [], None

    def replay():
        while True:
            yield resident

    for leg, prefetch in (("a", 0), ("b", a.prefetch), ("a", 0), ("b", a.prefetch), ("c", None)):
        done, t0 = 0, None
        while done < a.warmup + a.steps:
            batches = replay() if leg == "c" else script._training_batches(cfg, True, 512, 0, 1, tr.device, prefetch, a.workers)
            try:
                for models, params, images, names in batches:
                    if done == a.warmup:
                        torch.cuda.synchronize()
                        t0 = time.perf_counter()
                    start = torch.randint(0, spec.new_size - CROP + 1, (2,), device="cuda")
                    loss = tr.step(models, params, images, patch_size=CROP, start_point=start.tolist(), global_batch=BATCH)
                    float(loss.item())
                    if leg == "b" and resident is None:
                        resident = (models.clone(), params.clone(), images.clone(), list(names))
                    done += 1
                    if done >= a.warmup + a.steps:
                        break
            finally:
                batches.close()
        torch.cuda.synchronize()
        ms = (time.perf_counter() - t0) * 1e3 / a.steps
        legs.append({"leg": leg, "prefetch": prefetch, "ms_per_step": ms, "samples_per_s": BATCH * 1e3 / ms})
        print(json.dumps(legs[-1]), flush=True)
    _save(a.work, "train", {"legs": legs, "batch": BATCH, "crop": CROP, "steps": a.steps, "warmup": a.warmup,
                            "loader_workers": a.workers, "batches_chunk": a.batches_chunk})


def stage_ingest(a):
    import torch
    from rendernet_amd import ops
    res = {}
    for cs, co in ((1, 1), (3, 1), (3, 3)):
        frames = torch.randint(0, 256, (BATCH, 512, 512, cs), dtype=torch.uint8, device="cuda")
        window = (4 * 17, 4 * 33, 4 * CROP, 4 * CROP)
        for _ in range(10):
            ops.target_u8_crop(frames, window, co)
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(200):
            ops.target_u8_crop(frames, window, co)
        e1.record()
        torch.cuda.synchronize()
        us = e0.elapsed_time(e1) * 1e3 / 200            # includes the wrapper's allocation and launch: an upper bound
        nbytes = BATCH * (4 * CROP) ** 2 * (cs + 4 * co)
        res["cs%d_co%d" % (cs, co)] = {"bytes": nbytes, "us_per_call_events": us}
    _save(a.work, "ingest", res)


def stage_report(a):
    out = {"bench": "loader_bench", "batch": BATCH, "crop": CROP}
    for stage in ("dataset", "decode", "deliver", "train", "ingest"):
        p = os.path.join(a.work, stage + ".json")
        out[stage] = json.load(open(p)) if os.path.exists(p) else "not measured"
    if a.kernel_stats and os.path.exists(a.kernel_stats):
        rows = [r for r in csv.DictReader(open(a.kernel_stats)) if "ingest_" in r.get("Name", "")]
        out["ingest_kernel_trace"] = rows
        if isinstance(out["ingest"], dict):
            for r in rows:                              # kernel time -> share of the HBM peak, bytes from the shapes
                for key, v in out["ingest"].items():
                    if "ingest_vec_kernel<%s, %s>" % (key[2], key[-1]) in r["Name"]:
                        ns = float(r["AverageNs"])
                        v["kernel_us_trace"] = ns / 1e3
                        v["hbm_share"] = v["bytes"] / (ns * 1e-9) / HBM_PEAK
    if a.step_alone_ms is not None:
        out["step_alone_ms_parent_bench"] = a.step_alone_ms
    line = json.dumps(out)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("stage", choices=("dataset", "decode", "deliver", "train", "ingest", "report"))
    ap.add_argument("--work", required=True, help="directory for the data set and the per-stage results")
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--prefetch", type=int, default=2)
    ap.add_argument("--workers", type=int, default=8, help="decode threads of leg b (1..16)")
    ap.add_argument("--batches-chunk", type=int, default=1, help="config key batches_chunk (the reference's default is 1)")
    ap.add_argument("--kernel-stats", default=None, help="kernel stats CSV of a rocprofv3 --kernel-trace --stats run of `ingest`")
    ap.add_argument("--step-alone-ms", type=float, default=None, help="bench.py --mode train ms/step measured in the same visit")
    ap.add_argument("--out", default=None)
    a = ap.parse_args(argv)
    os.makedirs(a.work, exist_ok=True)
    {"dataset": stage_dataset, "decode": stage_decode, "deliver": stage_deliver, "train": stage_train,
     "ingest": stage_ingest, "report": stage_report}[a.stage](a)


if __name__ == "__main__":
    main()
