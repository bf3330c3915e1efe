#!/usr/bin/env python
"""Headline benchmark: rendered frames/s, 64^3 voxel -> 512x512 Phong-shader forward, batch 24 per
GPU (BASELINE.json configs[1]), on N MI355X of one node.

    python bench.py                                   # N=1, the headline line: set up, warm up, time --steps steps, print
    python bench.py --full                            # ... + the other multiply-stage modes, roofline, parity, cpu_baseline
    python bench.py --dump-outputs DIR                # ... + the last timed step's outputs as DIR/<name>.npy
    python bench.py --gpus N [--scaling weak|strong]  # spawns N ranks itself (torch.distributed.run) ...
    python -m torch.distributed.run --nnodes=1 --nproc-per-node N --master-addr 127.0.0.1 \
           --master-port P bench.py --gpus N --steps K --warmup W      # ... or is launched as N ranks
    python bench.py --mode texture | stress | train   # BASELINE configs[2], [4], [3]

A "step" is one pass of the whole hot path over one batch per rank: fused resampler (pose -> image-aligned grid)
+ the RenderNet forward, inputs already resident in HBM.  Frames are independent, so ranks shard by batch with no
data-path collective.  --scaling weak: every rank renders its own batch (value = all frames / max-over-ranks
time); --scaling strong: ONE batch is split over the ranks in contiguous blocks (24 -> 24/12/6/3 frames per GPU,
SURVEY.md §8e).  Rank 0 prints ONE JSON line (fields: README / DESIGN.md §5).  A plain run (no --full) does only what
that line's headline figure needs; everything else the bench measures or checks runs under --full.
"""
import argparse
import json
import os
import socket
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, ROOT)

FIXTURES = ["chair", "bunny", "table", "suzanne", "teapot"]
PEAK_FP32_MFMA_TFLOPS = 157.3     # MI355X_MICROARCH.md: v_mfma_f32_32x32x2_f32 / 16x16x4_f32, dense, exact fp32
PARITY_TOL = 1e-3                 # north_star: per-pixel L-inf vs the reference render
# SURVEY.md §8(d) / App. B / BASELINE.md §2: algorithmic GMAC per frame (direct-convolution counting rule)
GMAC_PER_FRAME = {"render": 1056.874, "texture": 268.790 + 0.66, "stress": 16280.4}


def fixtures_vox():
    from rendernet_amd.tools import binvox_rw
    vox = []
    for n in FIXTURES:
        with open(os.path.join(ROOT, "binvox", n + ".binvox"), "rb") as f:
            vox.append(binvox_rw.read_as_3d_array(f).data.astype(np.float32)[..., None])
    return vox


def bench_poses(batch):
    az = (250.0 + 15.0 * np.arange(batch)) % 360.0
    poses = np.stack([az * np.pi / 180.0, np.full(batch, (90 - 60) * np.pi / 180.0), np.full(batch, 3.3 / 3.3)], 1)
    return poses.astype(np.float32)


def synthetic_batch(batch, upsample=1):
    """item i = fixture[i mod 5]; pose az=(250+15i) mod 360, el=60, r=3.3.  upsample=2: each fixture
    nearest-neighbour-upsampled to 128^3 (the stress config)."""
    vox = fixtures_vox()
    if upsample > 1:
        vox = [v.repeat(upsample, 0).repeat(upsample, 1).repeat(upsample, 2) for v in vox]
    return np.stack([vox[i % 5] for i in range(batch)]), bench_poses(batch)


def texture_codes(batch, z_dim=199):
    """texture codes ~N(0,1), seed 7 (Reconstruct_RenderNet_Face.py:464 uses randn)."""
    return np.random.default_rng(7).standard_normal((batch, z_dim)).astype(np.float32)


def pick_threads():
    """The thread count that runs the dominant conv fastest on this box (all cores of a large host oversubscribe
    oneDNN on a batch this small)."""
    import torch
    import torch.nn.functional as F
    ncpu = os.cpu_count() or 1
    xx, ww = torch.randn(1, 1024, 64, 64), torch.randn(1024, 1024, 3, 3)
    best, cores = None, 1
    for th in sorted({min(ncpu, t) for t in (8, 16, 32, 64, 128)}):
        torch.set_num_threads(th)
        F.conv2d(xx[:, :, :16], ww, padding=1)
        t0 = time.time()
        F.conv2d(xx, ww, padding=1)
        dt = time.time() - t0
        if best is None or dt < best:
            best, cores = dt, th
    torch.set_num_threads(cores)
    return cores, ncpu


def cpu_baseline(weights, mode="render", frames=4):
    """The oracle (CPU restatement of the TF graph; the reference itself needs TensorFlow 1.x, which is not
    installable -- SURVEY.md F4) timed on this box's host cores on a bounded sample: the first `frames` frames of
    the bench batch as one batched pass, then one single-frame pass (BASELINE.md §3 asks for a B=24 pass and three
    B=1 passes: ~2 min of CPU work, cut to the ~20-30 s the bench contract allows -- `protocol` says so in the line).
    Returns (record, images): the images are the oracle's render of those frames -- the parity reference for the timed
    GPU output (texture mode: both heads concatenated on the channel axis, as the bench's render() returns them)."""
    from oracle import rendernet as ON
    from oracle import resample as OR
    cores, ncpu = pick_threads()
    vox, poses = synthetic_batch(frames, 2 if mode == "stress" else 1)
    single = mode != "stress"              # the stress frame is 15x the work: one pass of one frame IS the bounded sample
    if mode == "stress":
        run = lambda n: np.asarray(ON.rendernet_forward(OR.net_input(vox[:n], poses[:n], 128, 256), weights))
        what = "resampler 128^3 -> 256^3 + the 948M-parameter net"
    elif mode == "texture":
        from oracle import texture_net as OT
        z = texture_codes(24)[:frames]
        run = lambda n: np.concatenate(OT.render_texture(vox[:n], z[:n], poses[:n], weights), axis=3)
        what = "texture decoder + 2 resamplers + two-head net"
    else:
        run = lambda n: np.asarray(ON.rendernet_forward(OR.net_input(vox[:n], poses[:n], 64, 128), weights))
        what = "resampler + full 237M-parameter net"
    t0 = time.time()
    out = run(frames)
    dt = time.time() - t0
    t1 = time.time()
    if single:
        run(1)
    dt1 = time.time() - t1
    assert out.shape[0] == frames and out.shape[1] == out.shape[2]
    rec = {"value": round(frames / dt, 4), "unit": "frames/s", "cores": cores, "host_cores": ncpu, "kind": "port",
           "single_frame_s": round(dt1 if single else dt, 2),
           "protocol": {"batched_pass_frames": frames, "single_frame_passes": 1 if single else 0, "threads": cores,
                        "threads_chosen_by": "fastest of {8,16,32,64,128} on the dominant conv",
                        "baseline_md_protocol": "one B=24 pass + three B=1 passes (~2 min): cut to fit the bench's time budget"},
           "sample": "frames 0-%d of the bench batch as one fp32 pass of the NumPy/torch-CPU oracle (%s) on %d threads of a "
                     "%d-core host: %.1f s%s" % (frames - 1, what, cores, ncpu, dt, "; one more single-frame pass: %.1f s" % dt1 if single else "")}
    return rec, np.asarray(out)


def cpu_baseline_full(weights):
    """BASELINE.md §3, the whole protocol, once (`--cpu-baseline-full`; minutes of CPU -- not part of the default bench line):
    the oracle's forward of the headline workload as ONE B=24 pass and the mean of THREE B=1 passes, with
    torch.set_num_threads(os.cpu_count()) as the plan prescribes AND with the best-of-{8..128} thread count the bench's cut
    protocol uses; core count and CPU model of the box printed.  Returns the record."""
    import platform
    import torch
    from oracle import rendernet as ON
    from oracle import resample as OR
    ncpu = os.cpu_count() or 1
    model = ""
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                model = line.split(":", 1)[1].strip()
                break
    except OSError:
        model = platform.processor()
    vox, poses = synthetic_batch(24)
    run = lambda n: np.asarray(ON.rendernet_forward(OR.net_input(vox[:n], poses[:n], 64, 128), weights))
    best, _ = pick_threads()
    legs = {}
    for name, th in (("all_cores", ncpu), ("best_of_sweep", best)):
        torch.set_num_threads(th)
        run(1)                                   # oneDNN primitive caches, first-touch of the weights
        t0 = time.time()
        run(24)
        t24 = time.time() - t0
        t1s = []
        for _ in range(3):
            t0 = time.time()
            run(1)
            t1s.append(time.time() - t0)
        legs[name] = {"threads": th, "b24_pass_s": round(t24, 2), "b24_frames_per_s": round(24.0 / t24, 4),
                      "b1_passes_s": [round(t, 2) for t in t1s], "b1_mean_frames_per_s": round(3.0 / sum(t1s), 4)}
    return {"protocol": "BASELINE.md §3: one B=24 forward + the mean of three B=1 forwards of the oracle (NumPy resampler + torch-CPU "
                        "oneDNN convs, fp32), headline workload (5 fixtures cycled to 24, bench poses, seed-1234 weights)",
            "kind": "port", "host_cores": ncpu, "cpu_model": model, "legs": legs,
            "value": legs["all_cores"]["b24_frames_per_s"], "unit": "frames/s", "cores": ncpu}


# ----------------------------------------------------------------------------------------------------------------
GOLDEN_DIR = os.path.join(ROOT, "tests", "golden")


def gather_per_rank(value, world, rank):
    """Every rank's scalar on every rank (one SUM all-reduce of a one-hot vector: works over RCCL and over gloo)."""
    import torch
    import torch.distributed as dist
    v = torch.zeros(world, dtype=torch.float64, device="cuda")
    v[rank] = value
    if world > 1:
        dist.all_reduce(v)
    return [float(x) for x in v.tolist()]


def per_rank_fields(elapsed_by_rank, units_by_rank, steps):
    ms = [1e3 * e / steps for e in elapsed_by_rank]
    return {"ms_per_step_per_rank": {"min": round(min(ms), 3), "mean": round(float(np.mean(ms)), 3), "max": round(max(ms), 3)},
            "per_rank": {"ms_per_step": [round(m, 3) for m in ms], "units_per_step": [int(u) for u in units_by_rank]}}


DUMP_LIMIT_BYTES = 64 << 20
DUMP_BLOCK = 1024                 # elements per sampled run: a sample keeps runs of neighbouring pixels / parameters


def dump_sample_index(n, keep):
    """The fixed sample of a flattened array of n elements that --dump-outputs writes when the outputs exceed DUMP_LIMIT_BYTES:
    keep // DUMP_BLOCK blocks of DUMP_BLOCK consecutive elements, chosen without replacement by a seed-0 generator, in order."""
    nblk = max(1, keep // DUMP_BLOCK)
    blocks = np.sort(np.random.default_rng(0).choice(n // DUMP_BLOCK, nblk, replace=False))
    return (blocks[:, None] * DUMP_BLOCK + np.arange(DUMP_BLOCK)).reshape(-1)


def dump_outputs(path, arrays):
    """--dump-outputs: {name: tensor} -- what the timed path returned in its last step -- as path/<name>.npy, float64 kept, anything
    else float32.  At most DUMP_LIMIT_BYTES in all: the smallest arrays are written whole; an array larger than its even share of what
    is left is replaced by the dump_sample_index sample of its flattened elements.  The directory gets a .gitignore of its own so that
    a dump inside a checkout leaves it clean."""
    import torch
    os.makedirs(path, exist_ok=True)
    if not os.path.exists(os.path.join(path, ".gitignore")):
        with open(os.path.join(path, ".gitignore"), "w") as f:
            f.write("*\n")
    items = []
    for name, t in arrays.items():
        t = torch.as_tensor(t).detach()
        items.append((name, t if t.dtype == torch.float64 else t.float()))
    items.sort(key=lambda kv: kv[1].numel() * kv[1].element_size())
    left = DUMP_LIMIT_BYTES
    for i, (name, t) in enumerate(items):
        share = left // (len(items) - i)
        if t.numel() * t.element_size() > share:
            idx = dump_sample_index(t.numel(), share // t.element_size())
            t = t.reshape(-1)[torch.as_tensor(idx, device=t.device)]
        left -= t.numel() * t.element_size()
        np.save(os.path.join(path, name + ".npy"), t.cpu().numpy())


def golden_parity(mode, out, frame_ids):
    """The output of the timed run against the COMMITTED oracle renders of the same frames (tests/golden/*.npz, written by
    tests/golden/make_golden.py with the CPU oracle): used where a live CPU pass is too slow (stress: minutes per frame) or
    not run (N > 1, --no-cpu-baseline).  out: this rank's images [n,H,W,ch] (HIP tensor); frame_ids: the bench-batch index
    of each of them.  Returns the parity record (ok False fails the bench)."""
    rec = {"tol": PARITY_TOL, "reference": "committed oracle renders, tests/golden/%s"}
    errs, used = [], []
    if mode == "render":
        z = np.load(os.path.join(GOLDEN_DIR, "bench_frames.npz"))
        rec["reference"] %= "bench_frames.npz (four 128x128 crops per frame)"
        for k, f in enumerate(z["frames"].tolist()):
            if f in frame_ids:
                img = out[frame_ids.index(f)].cpu().numpy()
                for c, (r0, c0) in enumerate(z["crops"].tolist()):
                    errs.append(float(np.abs(img[r0:r0 + 128, c0:c0 + 128, 0] - z["output_%d" % k][c]).max()))
                used.append(f)
    elif mode == "stress":
        z = np.load(os.path.join(GOLDEN_DIR, "stress_bench_frames.npz"))
        rec["reference"] %= "stress_bench_frames.npz (128x128 centre crop per frame)"
        for f in range(8):
            if f in frame_ids:
                img = out[frame_ids.index(f)].cpu().numpy()
                errs.append(float(np.abs(img[448:576, 448:576, 0] - z["output_%d" % f]).max()))
                used.append(f)
    else:
        z = np.load(os.path.join(GOLDEN_DIR, "texture_bench_frames.npz"))
        rec["reference"] %= "texture_bench_frames.npz (128x128 centre crop of both heads per frame)"
        for k, f in enumerate(z["frames"].tolist()):
            if f in frame_ids:
                img = out[frame_ids.index(f)].cpu().numpy()
                errs.append(float(np.abs(img[192:320, 192:320, 0:3] - z["image_%d" % k]).max()))
                errs.append(float(np.abs(img[192:320, 192:320, 3:6] - z["normal_%d" % k]).max()))
                used.append(f)
    if not used:
        return None
    rec.update({"frames": used, "max_abs_err": max(errs), "ok": max(errs) <= PARITY_TOL})
    return rec


def train_parity(tr, spec, world):
    """BASELINE configs[3] checks itself: loss and sampled gradient entries of EVERY variable of the full-width net (two
    samples of the bench batch, crop 64, BCE) against torch-CPU autograd over the oracle graph, committed as
    tests/golden/train_step_golden.npz.  Runs before the first optimiser step (the golden is for the initial weights), on
    EVERY rank (the backward launches the gradient buckets' all-reduces): all ranks feed the same two samples, so the summed
    gradient is `world` times the golden one -- which also exercises the collective before anything is timed."""
    import torch
    z = np.load(os.path.join(GOLDEN_DIR, "train_step_golden.npz"))
    tr._begin_step()
    start, patch = [int(v) for v in z["start"]], int(z["patch"])
    pred, _ = tr.forward(None, None, patch, start, net_in=z["net_in"])
    tr.loss_and_backward(pred, torch.as_tensor(z["target"]).cuda(), int(z["net_in"].shape[0]))
    loss = float(tr.loss_buf.item())
    loss_rel = abs(loss - float(z["loss"])) / abs(float(z["loss"]))
    pred_err = float(np.abs(pred.detach()[:, 64:192, 64:192, 0].cpu().numpy() - z["pred_crop"]).max())
    tr.buckets.finish()                      # the all-reduces of every bucket have landed
    # Filter gradients are compared at 1e-3 of the tensor's largest entry.  Bias and PReLU-slope gradients are sums of ~10^5
    # mixed-sign terms per channel (sum dz, sum dy*min(z,0)) whose value is 10^2-10^3 times smaller than the sum of the terms'
    # magnitudes: the ~1e-6 relative noise a 60-layer fp32 backward leaves on dz is amplified by that cancellation ratio
    # (a FLOAT32 torch-CPU autograd run of the same graph differs from the float64 golden by 2.4e-3 on e_conv7's bias
    # gradient; this path by 1.4e-3 at most) -- their bar is 5e-3.
    worst = {"filters": 0.0, "bias_alpha": 0.0}
    n, per_var = 0, []
    for k, name in enumerate(z["names"].tolist()):
        g = tr.grad_views[name].reshape(-1)[torch.as_tensor(z["idx"][k]).cuda()].cpu().numpy() / float(world)
        e = float(np.abs(g - z["val"][k]).max() / (float(z["gmax"][k]) + 1e-20))
        per_var.append((e, name))
        kind = "filters" if name.endswith("weights") else "bias_alpha"
        worst[kind] = max(worst[kind], e)
        n += g.size
    per_var.sort(reverse=True)
    tr.grad.zero_()
    tol = {"loss_rel": 1e-4, "filter_grad_rel_to_max": 1e-3, "bias_alpha_grad_rel_to_max": 5e-3, "pred": PARITY_TOL,
           "why_5e-3": "bias / PReLU-slope gradients are sums of ~1e5 mixed-sign terms that cancel to 1e-2..1e-3 of their magnitude sum: a float32 "
                       "torch-CPU autograd of the same graph is 2.4e-3 away from the float64 golden on e_conv7's bias"}
    ok = (loss_rel <= tol["loss_rel"] and worst["filters"] <= tol["filter_grad_rel_to_max"]
          and worst["bias_alpha"] <= tol["bias_alpha_grad_rel_to_max"] and pred_err <= PARITY_TOL)
    return {"loss": loss, "loss_rel_err": loss_rel, "pred_max_abs_err": pred_err, "filter_grad_max_rel_err": worst["filters"],
            "bias_alpha_grad_max_rel_err": worst["bias_alpha"], "grad_entries": n, "variables": int(len(z["names"])),
            "worst_variables": [(nm, float("%.3g" % e)) for e, nm in per_var[:4]], "tol": tol, "ok": bool(ok),
            "reference": "float64 torch-CPU autograd over the oracle graph, tests/golden/train_step_golden.npz "
                         "(2 samples, crop 64 at %s, full-width net)" % (tuple(start),)}


def cpu_baseline_train(weights, patch):
    """The oracle's training step (torch-CPU autograd over the oracle graph + the NumPy restatement of TF's Adam) on ONE sample of
    the train bench's batch at the benched crop: a bounded sample (~10-20 s) of the same workload, `kind` "port" as for the
    render line (TensorFlow itself is not installable)."""
    from oracle import resample as OR
    from oracle import train as OTR
    cores, ncpu = pick_threads()
    vox, poses = synthetic_batch(1)
    target = np.random.default_rng(11).uniform(0, 1, (1, 512, 512, 1)).astype(np.float32)
    t0 = time.time()
    full = OR.net_input(vox, poses, 64, 128)
    net_in, tgt = OTR.crop_voxel_image(full, target, (31, 17), patch)
    loss, grads, _ = OTR.loss_and_grads(np.ascontiguousarray(net_in), np.ascontiguousarray(tgt), weights)
    OTR.Adam().apply(weights, grads)
    dt = time.time() - t0
    return {"value": round(1.0 / dt, 4), "unit": "samples/s", "cores": cores, "host_cores": ncpu, "kind": "port",
            "protocol": {"samples": 1, "patch": patch, "threads": cores},
            "sample": "one sample of the bench batch: resampler + crop %d + forward + BCE + torch-CPU autograd backward + NumPy Adam over "
                      "237M parameters on %d threads of a %d-core host: %.1f s (loss %.1f)" % (patch, cores, ncpu, dt, loss)}


TRAIN_DTYPE = {
    "f32": "f32",
    "split": "f32 (forward and input-gradient multiply stages of the wide 2-D convs and of the 3-D encoder's convs, and the filter gradients of the "
             "layers at least 1024 channels wide: bf16x3-split operands, fp32 accumulate; everything else exact fp32)",
    "split16": "f32 (forward and input-gradient multiply stages of the wide 2-D convs and of the 3-D encoder's convs: fp16x2-split operands of value / "
               "tensor scale, 22-bit, fp32 accumulate; filter gradients of the layers at least 1024 channels wide: bf16x3-split; everything else exact fp32)"}


def train_stage_roofline(events, stage, gemm_mode, width):
    """`roofline` (stage "gemm": the GEMM stage of the forward / input-gradient launches on the res2 layers) or `roofline_wgrad` (stage
    "wgrad": ALL launches of the filter gradient of the same layers) of one timed training pass, priced per mode: exact fp32 against the fp32
    MFMA peak; bf16x3 against bf16 peak / 6; fp16x2 against fp16 peak / 3 (the filter gradient has no fp16x2 form: bf16x3 in both split modes)."""
    if not events:
        return None
    ms = float(np.mean([a.elapsed_time(b) for (a, b), _ in events]))
    T, which = events[0][1][0], events[0][1][3]
    nxi, fname = WINO_SCHEMES.get(which.rstrip("s"), (36, "F(4x4,3x3)"))
    fl = 2.0 * nxi * T * width * width
    if stage == "wgrad":
        nprod = 6 if gemm_mode in ("split", "split16") else 0
        kern = ("rn_conv2d_winograd_split_wgrad: wino_input_bf3t + wino_dout_bf3t + wino_gemm_bf3 (rows = input channels, K = tiles) + wino_dfilter_bf3, "
                "all four launches" if nprod else
                "rn_conv2d_wino43_wgrad: wino_input_kernel + wino_dout_kernel + wino43_wgrad_gemm_kernel (+ reduce) + wino_dfilter_kernel, all launches")
    else:
        nprod = {"f32": 0, "split": 6, "split16": 3}[gemm_mode]
        kern = {"f32": "wino43_gemm_kernel (exact-fp32 MFMA)", "split": "wino_gemm_bf3_kernel<rnf::FmtB3>",
                "split16": "wino_gemm_bf3_kernel<rnf::FmtH2>"}[gemm_mode] + ", GEMM stage of the forward and input-gradient launches"
    peak = PEAK_BF16_MFMA_TFLOPS / nprod if nprod else PEAK_FP32_MFMA_TFLOPS
    ach = fl / (ms * 1e-3) / 1e12
    r = {"kernel": "%s; Winograd %s on the res2 3x3 %d->%d conv, T = %d tiles" % (kern, fname, width, width, T),
         "bound": "mfma", "achieved": round(ach, 2), "peak": round(peak, 2), "unit": "TFLOP/s", "frac": round(ach / peak, 4),
         "avg_ms": round(ms, 4), "calls_timed": len(events), "flop_per_call": fl,
         "flop_basis": ("fp32-equivalent FLOPs = 2*%d*T*Cin*Cout, each executed as %d 16-bit piece products" % (nxi, nprod)) if nprod
                       else "executed MFMA FLOPs = 2*%d*T*Cin*Cout" % nxi,
         "traffic": None}
    if nprod:
        r["peak_name"] = "dense 16-bit MFMA peak / %d (%d piece products per fp32 product)" % (nprod, nprod)
    return r


# ----------------------------------------------------------------------------------------------------------------
def train_main(args, world, rank, local_rank):
    """BASELINE configs[3]: Phong-shader training step, batch 24 per GPU (global batch 24*N), crop `--patch`,
    BCE loss, Adam; gradients summed across ranks with bucketed RCCL all-reduces overlapped with backward."""
    import torch
    import torch.distributed as dist
    from rendernet_amd.shader import ShaderSpec, init_shader_weights
    from rendernet_amd.train import Trainer
    spec = ShaderSpec().check()
    weights = init_shader_weights(spec, seed=1234, perturb=True)
    from rendernet_amd import ops
    tr = Trainer(spec, weights, device="cuda:%d" % local_rank, gemm=args.gemm)   # the primary mode (default: the library default, "split")
    B, p = args.batch, args.patch
    vox_np, poses_np = synthetic_batch(B)
    poses_np[:, 0] = (poses_np[:, 0] + rank * 0.1) % (2 * np.pi)
    vox, poses = torch.as_tensor(vox_np).cuda(), torch.as_tensor(poses_np).cuda()
    gen = torch.Generator(device="cuda").manual_seed(11 + rank)
    targets = torch.rand((B, 512, 512, spec.out_ch), device="cuda", generator=gen)
    starts = np.random.default_rng(3).integers(0, spec.new_size - p + 1, size=(args.warmup + args.steps, 2))

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    from rendernet_amd import ops
    parity = train_parity(tr, spec, world) if args.full else None
    for i in range(args.warmup):
        loss = tr.step(vox, poses, targets, patch_size=p, start_point=starts[i])
    # dominant kernel of the step: the GEMM stage of the F(4x4,3x3) path on the res2 trunk (forward and input-gradient
    # launches, 42 per step), bracketed by HIP events on the launch stream like in the render bench
    gemm_events, wgrad_events = [], []

    def stage_hook(stage, tkn):
        if stage in ("gemm", "wgrad") and tkn[1] == spec.w_res2 and tkn[2] == spec.w_res2 and tkn[3] != "f11":
            ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
            (gemm_events if stage == "gemm" else wgrad_events).append((ev, tkn))
            return ev
        return None

    if args.full:
        ops.STAGE_HOOK = stage_hook
    barrier()
    t0 = time.perf_counter()
    for i in range(args.steps):
        loss = tr.step(vox, poses, targets, patch_size=p, start_point=starts[args.warmup + i])
    barrier()
    elapsed = time.perf_counter() - t0
    ops.STAGE_HOOK = None
    by_rank = gather_per_rank(elapsed, world, rank)
    elapsed = max(by_rank)
    lossv = float(loss.item())
    assert np.isfinite(lossv)
    if args.dump_outputs and rank == 0:
        # what a caller of the step holds after the last one: the loss it returned and the updated parameters
        dump_outputs(args.dump_outputs, {"loss": loss, "params": tr.param})
    # the same steps with the multiply stages of the wide 2-D convs (forward, input gradient and, at >= 1024 channels, filter gradient) and of the 3-D encoder
    # on the bf16 pipe by operand splitting: a second trainer from the same initial weights, checked against the same golden
    alts = {}
    if args.full and not args.no_alt:
        del tr
        for akey, gm in other_modes(args.gemm):
            torch.cuda.empty_cache()
            try:
                tr2 = Trainer(spec, weights, device="cuda:%d" % local_rank, gemm=gm)
                parity2 = train_parity(tr2, spec, world)
                for i in range(max(1, args.warmup)):
                    tr2.step(vox, poses, targets, patch_size=p, start_point=starts[i])
                alt_events = {"gemm": [], "wgrad": []}

                def alt_hook(stage, tkn):
                    if stage in alt_events and tkn[1] == spec.w_res2 and tkn[2] == spec.w_res2 and tkn[3] != "f11":
                        ev = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                        alt_events[stage].append((ev, tkn))
                        return ev
                    return None

                ops.STAGE_HOOK = alt_hook
                barrier()
                t0 = time.perf_counter()
                for i in range(args.steps):
                    loss2 = tr2.step(vox, poses, targets, patch_size=p, start_point=starts[args.warmup + i])
                barrier()
                el2 = max(gather_per_rank(time.perf_counter() - t0, world, rank))
                loss2 = float(loss2.item())
            finally:
                ops.STAGE_HOOK = None
            del tr2
            alt = {"dtype": TRAIN_DTYPE[gm], "gemm_mode": gm,
                   "value": round(B * world * args.steps / el2, 3), "unit": "samples/s", "ms_per_step": round(1e3 * el2 / args.steps, 3),
                   "speedup_vs_value": round(elapsed / el2, 4), "final_loss": loss2, "parity": parity2}
            for stage, key in (("gemm", "roofline"), ("wgrad", "roofline_wgrad")):
                r = train_stage_roofline(alt_events[stage], stage, gm, spec.w_res2)
                if r is not None:
                    alt[key] = r
            alts[akey] = alt
    if rank == 0:
        # forward MACs scale with the crop area; backward = dgrad + wgrad ~ 2x forward
        fwd_tflop = 2e-3 * GMAC_PER_FRAME["render"] * (p / float(spec.new_size)) ** 2
        sps = B * world * args.steps / elapsed
        line = {
            "metric": "training samples/sec, Phong shader forward+backward+Adam, crop %d of 128^3, batch 24 per GPU" % p,
            "value": round(sps, 3), "unit": "samples/s", "n_gpus": world, "steps": args.steps, "warmup": args.warmup,
            "ms_per_step": round(1e3 * elapsed / args.steps, 3), "higher_is_better": True, "scaling": "weak",
            "vs_baseline": None, "dtype": TRAIN_DTYPE[args.gemm], "gemm_mode": args.gemm,
            "data": "synthetic", "rccl_ranks": args.rccl_ranks,
            "config": {"workload": "Phong shader training step (resampler+crop, forward, BCE, dgrad+wgrad, bucketed "
                                   "gradient all-reduce, Adam), 237.3M params", "batch_per_gpu": B,
                       "global_batch": B * world, "patch": p, "parallelism": "data-parallel x%d, RCCL sum all-reduce" % world},
            "direct_equiv_tflops_per_gpu": round(3.0 * fwd_tflop * sps / world, 2), "final_loss": lossv}
        if args.full:
            roof = train_stage_roofline(gemm_events, "gemm", args.gemm, spec.w_res2)
            roof_w = train_stage_roofline(wgrad_events, "wgrad", args.gemm, spec.w_res2)
            line.update({"roofline": roof, **({"roofline_wgrad": roof_w} if roof_w is not None else {}), "parity": parity, **alts,
                         **({"cpu_baseline": cpu_baseline_train(weights, p)} if (world == 1 and not args.no_cpu_baseline) else {})})
        line.update(per_rank_fields(by_rank, [B] * world, args.steps))
        print(json.dumps(line), flush=True)
        if parity is not None and not parity["ok"]:
            raise SystemExit("PARITY FAILURE (training step): %s" % json.dumps(parity))
        for akey, ablk in alts.items():
            if not ablk["parity"]["ok"]:
                raise SystemExit("PARITY FAILURE (training step, %s): %s" % (akey, json.dumps(ablk["parity"])))


# ----------------------------------------------------------------------------------------------------------------
def build_workload(mode, device):
    """-> dict(render(vox, aux, poses) -> image tensor, inputs(batch) -> (vox, aux, poses) numpy, spec, weights, ...)."""
    import torch
    if mode in ("render", "stress"):
        from rendernet_amd.shader import Renderer, ShaderSpec, stress_spec, init_shader_weights
        spec = stress_spec(1) if mode == "stress" else ShaderSpec().check()
        weights = init_shader_weights(spec, seed=1234, perturb=True)
        r = Renderer(spec, weights, device=device)
        up = 2 if mode == "stress" else 1

        def inputs(batch):
            v, p = synthetic_batch(batch, up)
            return v, None, p
        name = ("Phong shader forward (resampler + RenderNet 1-ch head), 5 shipped binvox fixtures cycled, 64^3 -> 128^3 -> "
                "512x512, seeded random weights (237.3M params)") if mode == "render" else \
               ("high-res stress: Phong shader forward, 5 fixtures upsampled to 128^3 -> 256^3 -> 1024x1024, every 2-D "
                "width doubled (projection 64*32 = 2048), seeded random weights (948M params)")
        return {"render": lambda v, a, p: r.render(v, p), "inputs": inputs, "spec": spec, "weights": weights,
                "name": name, "out_hw": 4 * spec.new_size, "out_ch": spec.out_ch, "trunk": (spec.new_size // 2, spec.w_res2)}
    from rendernet_amd.texture import TextureRenderer, TextureSpec, init_texture_weights
    spec = TextureSpec().check()
    weights = init_texture_weights(spec, seed=1234, perturb=True)
    r = TextureRenderer(spec, weights, device=device)

    def inputs(batch):
        v, p = synthetic_batch(batch)
        return v, texture_codes(batch, spec.z_dim), p

    def render(v, a, p):
        return r.render(v, a, p)              # (image, normal map): the two heads stay two tensors, as the reference fetches them
    return {"render": render, "inputs": inputs, "spec": spec, "weights": weights,
            "name": "texture + normal face render (RenderNet_Texture_Face_Normal.py): geometry 64^3 + 199-d texture code -> "
                    "texture decoder -> 2 resamplers (1+4 channels) -> 16-channel net -> two 512x512x3 heads, seeded weights",
            "out_hw": 4 * spec.new_size, "out_ch": 6, "trunk": (spec.new_size // 2, spec.w_res2)}


PEAK_BF16_MFMA_TFLOPS = 2500.0     # MI355X_MICROARCH.md: v_mfma_f32_32x32x16_bf16, dense (fp16: the same rate)
# Every line times the PRIMARY mode (--gemm; default = the library default, "split") and then the other two multiply-stage modes as
# named blocks of the same JSON line: mode -> block key
MODE_BLOCK = {"f32": "exact", "split": "alt", "split16": "alt2"}


def other_modes(primary):
    """(block key, ops.WINO_GEMM mode) of the further timed passes, exact first."""
    return tuple((MODE_BLOCK[m], m) for m in ("f32", "split", "split16") if m != primary)


ALT_DTYPE = {"f32": "exact fp32 everywhere (fp32 MFMA multiply stages)",
             "split": "bf16x3-split operands (three bf16 pieces that sum exactly to the fp32 value: 24-bit operands), fp32 accumulate",
             "split16": "fp16x2-split of value / power-of-two tensor scale (22-bit operands; ONE scale per tensor: a region 2^15 / 2^20 below the "
                        "tensor's max|x| is computed with 2.8x / 88x the exact route's error relative to its OWN magnitude -- profiles/r05_regional_range.md; "
                        "max-norm error below the exact route's on every case), fp32 accumulate"}
LINE_DTYPE = {"f32": "f32", "split": "f32 (multiply stages: bf16x3-split operands, fp32 accumulate)",
              "split16": "f32 (multiply stages: fp16x2-split operands of value / tensor scale -- 22-bit, fp32 accumulate)"}
ALT_WHAT = {
    "f32": "the same steps with every multiply stage on the exact-fp32 MFMA pipe (v_mfma_f32_32x32x2_f32 / 16x16x4_f32; RN_WINO_GEMM=f32): the "
           "fallback mode, the product default until round 4, and what a filter rejected by the F(6x6,3x3) self-check is demoted to",
    "split": "the same steps with the multiply stages of the wide stride-1 2-D convs (res2, res3, *_skip, e_conv5, e_conv6) and of the 3-D "
             "encoder's 32-channel convs on the bf16 matrix pipe: every fp32 operand as three bf16 pieces (exact sum), six piece products "
             "with i + j <= 2, fp32 accumulation (csrc/conv_wino_bf3.hip, conv3d_wino_bf3.hip); every other kernel unchanged (exact fp32)",
    "split16": "as `alt`, but the wide 2-D convs take every operand as TWO fp16 pieces of value / scale (scale = a power of two from max|x| "
               "of the tensor, gathered by the producing launch, and the transform's growth bound) and three piece products (h0h0, h0h1, "
               "h1h0): half the matrix work; operands carry 22 mantissa bits, the fp32 accumulation all routes share dominates the error "
               "(profiles: hostile-statistics table); the 3-D encoder's convs in the same format (csrc/conv3d_wino_bf3.hip, C3H2)",
}


def gemm_roofline(gemm_events, layer_events, wtrunk, hw, nloc, mode, gemm_mode):
    """`roofline` of the dominant kernel from the HIP-event brackets of one timed pass.  gemm_mode "f32": executed fp32 MFMA
    FLOPs over the exact-fp32 MFMA peak; "split": the SAME fp32-equivalent FLOPs, each executed as six bf16 piece products --
    priced against the bf16 peak / 6 (and named so), i.e. frac = (6 x those FLOPs per second) / 2.5 PFLOP/s."""
    from rendernet_amd import ops  # noqa: F401
    if not layer_events:
        return None
    layer_ms = float(np.mean([a.elapsed_time(b) for (a, b), _ in layer_events]))
    kinds = {k for _, k in layer_events}
    kind = kinds.pop() if len(kinds) == 1 else "mixed"
    M = nloc * hw * hw
    direct_flop = 2.0 * M * 9 * wtrunk * wtrunk                    # M*K*N*2
    where = " on the res2 3x3 %d->%d conv @%dx%dx%d" % (wtrunk, wtrunk, hw, hw, nloc)
    peak, peak_name = PEAK_FP32_MFMA_TFLOPS, None
    if kind == "wino43" and gemm_events:
        # three launches per layer; the dominant one is the GEMM stage (36 / 64 GEMMs T x Cin x Cout), timed on its own
        kern_ms = float(np.mean([a.elapsed_time(b) for (a, b), _ in gemm_events]))
        T, which = gemm_events[0][1][0], gemm_events[0][1][3]
        nxi, fname = WINO_SCHEMES[which]
        m = 6 if which == "f63" else 4
        exec_flop = 2.0 * nxi * T * wtrunk * wtrunk
        if gemm_mode == "split16":
            name = ("wino_gemm_bf3_kernel<FmtH2> (GEMM stage of Winograd %s on operands split into two fp16 pieces of value / tensor scale: "
                    "256x256x16 blocks, three 32x32x16 fp16 MFMAs per fp32 product tile, fp32 accumulate, LDS-DMA 3 stages, persistent)" % fname)
            basis = ("fp32-equivalent FLOPs = 2*%d*T*Cin*Cout, T = B*ceil(H/%d)*ceil(W/%d) tiles; every one executed as 3 fp16 "
                     "piece products (h0h0, h0h1, h1h0)" % (nxi, m, m))
            peak, peak_name = PEAK_BF16_MFMA_TFLOPS / 3.0, "fp16 MFMA dense peak / 3 (three fp16 products per fp32 product)"
            tkey = "wino63_gemm_h2_res2" if which == "f63" else "wino43_gemm_h2_res2"
        elif gemm_mode == "split":
            name = ("wino_gemm_bf3_kernel (GEMM stage of Winograd %s on split operands: 256x256x16 blocks, the six bf16 piece products of an fp32 "
                    "product as three 16x16x32 bf16 MFMAs per 16x16 tile (K = 16 channels x 2 pieces), fp32 accumulate, LDS-DMA 3 stages, persistent)" % fname)
            basis = ("fp32-equivalent FLOPs = 2*%d*T*Cin*Cout, T = B*ceil(H/%d)*ceil(W/%d) tiles; every one executed as 6 bf16 "
                     "piece products (x0y0, x0y1, x1y0, x0y2, x1y1, x2y0)" % (nxi, m, m))
            peak, peak_name = PEAK_BF16_MFMA_TFLOPS / 6.0, "bf16 MFMA dense peak / 6 (six bf16 products per fp32 product)"
            tkey = "wino63_gemm_bf3_res2" if which == "f63" else "wino43_gemm_bf3_res2"
        else:
            name = "wino43_gemm_kernel (GEMM stage of Winograd %s: 256x256x32 blocks, 32x32x2 fp32 MFMA, LDS-DMA, persistent)" % fname
            basis = "executed MFMA FLOPs = 2*%d*T*Cin*Cout, T = B*ceil(H/%d)*ceil(W/%d) tiles" % (nxi, m, m)
            tkey = "wino63_gemm_res2" if which == "f63" else "wino43_gemm_res2"
    else:
        kern_ms = layer_ms
        exec_flop = direct_flop * 16.0 / 36.0 if kind == "wino" else direct_flop   # F(2x2,3x3): 16 multiplies per 2x2 tile vs 36
        name = ("conv_wino_kernel (Winograd F(2x2,3x3), 16x16x4 fp32 MFMA, fused transforms)" if kind == "wino" else
                "conv_igemm_glds_kernel (128x128x32 tile, LDS-DMA)")
        basis = "executed MFMA FLOPs = 2*(M/4)*16*Cin*Cout" if kind == "wino" else "2*M*9*Cin*Cout"
        tkey = "conv_wino_res2" if kind == "wino" else "conv_igemm_res2"
    achieved = exec_flop / (kern_ms * 1e-3) / 1e12
    traffic, tsrc = read_traffic(tkey) if (mode == "render" and nloc == 24) else (None, None)
    roof = {
        "kernel": name + where,
        "bound": "mfma", "achieved": round(achieved, 2), "peak": round(peak, 2), "unit": "TFLOP/s",
        "frac": round(achieved / peak, 4), "avg_launch_ms": round(kern_ms, 4),
        "launches_timed": len(gemm_events) if kind == "wino43" and gemm_events else len(layer_events), "flop_per_launch": exec_flop,
        "flop_basis": basis,
        "layer_ms": round(layer_ms, 4),       # the whole layer (wino43: input transform + GEMM + output transform)
        "layer_effective_tflops_direct_equiv": round(direct_flop / (layer_ms * 1e-3) / 1e12, 2),
        "traffic": traffic, "traffic_source": tsrc}
    if peak_name:
        roof["peak_name"] = peak_name
        roof["mfma_tflops_executed"] = round((3.0 if gemm_mode == "split16" else 6.0) * achieved, 1)
    return roof


def render_main(args, world, rank, local_rank):
    import torch
    import torch.distributed as dist
    from rendernet_amd import ops
    from rendernet_amd.parallel import shard_range

    mode = args.mode
    wl = build_workload(mode, "cuda:%d" % local_rank)
    B = args.batch
    hw, wtrunk = wl["trunk"]

    def barrier():
        torch.cuda.synchronize()
        if world > 1:
            dist.barrier()
        torch.cuda.synchronize()

    def shard(scaling):
        """This rank's inputs: weak -- its own batch of B frames (every rank its own pose set); strong -- ONE batch of B frames
        split over the ranks in contiguous blocks (24 -> 24/12/6/3 per GPU)."""
        vox_np, aux_np, poses_np = wl["inputs"](B)
        if scaling == "strong":
            if B < world:
                raise SystemExit("--scaling strong: batch %d < %d ranks" % (B, world))
            lo, hi = shard_range(B, rank, world)
            vox_np, poses_np = vox_np[lo:hi], poses_np[lo:hi]
            aux_np = None if aux_np is None else aux_np[lo:hi]
            total = B
        else:
            poses_np = poses_np.copy()
            poses_np[:, 0] = (poses_np[:, 0] + rank * 0.1) % (2 * np.pi)
            total = B * world
        return (torch.as_tensor(vox_np).cuda(), None if aux_np is None else torch.as_tensor(aux_np).cuda(),
                torch.as_tensor(poses_np).cuda(), total)

    def timed_pass(vox, aux, poses, gemm_mode, steps, warmup, instrument):
        """warmup untimed steps, then exactly `steps` steps between barrier + synchronize on both sides; with `instrument` (--full:
        the rooflines) the dominant layer, its GEMM stage and the resampler bracketed by HIP events on the launch stream.
        -> (out, max-over-ranks seconds, per-rank seconds, events)."""
        ev = {"layer": [], "gemm": [], "resample": []}

        def stage_hook(stage, tkn):
            if stage == "gemm" and tkn[1] == wtrunk and tkn[2] == wtrunk and tkn[3] in ("f43", "f63"):      # (not the projection unit's 1x1 GEMM)
                e = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev["gemm"].append((e, tkn))
                return e
            return None

        def hook(m, xshape, pw):
            if m == "resample":
                e = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev["resample"].append((e, xshape))
                return e
            if m == "conv2d" and pw.cin == wtrunk and pw.cout == wtrunk and pw.kdims[0] == 3:
                e = (torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True))
                ev["layer"].append((e, "wino43" if ops._use_wino43(pw, xshape[1], xshape[2]) else "wino" if pw.wino is not None else "direct"))
                return e
            return None

        # the renderer names no mode of its own (gemm=None): it runs in the mode of this context -- no module state is written
        with torch.no_grad(), ops.gemm_mode(gemm_mode):
            for _ in range(warmup):
                out = wl["render"](vox, aux, poses)
            if instrument:
                ops.LAUNCH_HOOK, ops.STAGE_HOOK = hook, stage_hook
            barrier()
            t0 = time.perf_counter()
            for _ in range(steps):
                out = wl["render"](vox, aux, poses)
            barrier()
            elapsed = time.perf_counter() - t0
            ops.LAUNCH_HOOK = ops.STAGE_HOOK = None
        if isinstance(out, (tuple, list)):
            out = torch.cat(list(out), dim=3)          # after the timed region: the checks below index one [n,H,W,6] tensor
        assert out.shape == (vox.shape[0], wl["out_hw"], wl["out_hw"], wl["out_ch"])
        assert bool(torch.isfinite(out).all())
        by_rank = gather_per_rank(elapsed, world, rank)
        return out, max(by_rank), by_rank, ev

    # ---- the primary pass: the mode of --gemm (default: the product default, the bf16x3 split multiply stages)
    vox, aux, poses, total_frames = shard(args.scaling)
    nloc = vox.shape[0]
    out, elapsed, by_rank, ev = timed_pass(vox, aux, poses, args.gemm, args.steps, args.warmup, args.full)
    if args.dump_outputs and rank == 0:
        # what the renderer returned in the last timed step (texture: its two heads, concatenated by timed_pass)
        dump_outputs(args.dump_outputs, {"image": out} if mode != "texture" else {"image": out[..., :3], "normal": out[..., 3:]})
    frames_by_rank = gather_per_rank(nloc, world, rank)
    # ---- --full: the same steps in the other two multiply-stage modes (exact fp32; the other split format)
    ALT_MODES = other_modes(args.gemm)
    alts = {}
    if args.full and not args.no_alt:
        for key, gm in ALT_MODES:
            alts[key] = timed_pass(vox, aux, poses, gm, args.steps, max(1, args.warmup), True)
    # ---- --full, N > 1: the other scaling regime as well (weak: every rank its own batch; strong: ONE batch split 24 -> 24/N)
    other = None
    if args.full and world > 1 and not args.no_other_scaling:
        oscal = "strong" if args.scaling == "weak" else "weak"
        if not (oscal == "strong" and B < world):
            v2, a2, p2, tot2 = shard(oscal)
            o2, el2, br2, _ = timed_pass(v2, a2, p2, args.gemm, args.steps, 1, True)
            fr2 = gather_per_rank(v2.shape[0], world, rank)
            other = {"scaling": oscal, "value": round(tot2 * args.steps / el2, 3), "unit": "frames/s",
                     "ms_per_step": round(1e3 * el2 / args.steps, 3), "global_batch": tot2,
                     **per_rank_fields(br2, fr2, args.steps)}
            for key, gm in ALT_MODES:
                if key in alts:
                    o3, el3, br3, _ = timed_pass(v2, a2, p2, gm, args.steps, 1, True)
                    other[key + "_value"] = round(tot2 * args.steps / el3, 3)
                    other[key + "_ms_per_step"] = round(1e3 * el3 / args.steps, 3)
            del v2, a2, p2, o2
    if rank != 0:
        return

    fps = total_frames * args.steps / elapsed
    gmac = GMAC_PER_FRAME[mode]
    metric = {"render": "rendered frames/sec, 64^3 voxel->512x512 Phong, batch 24",
              "texture": "rendered frames/sec, texture+normal face render 64^3 -> two 512x512x3 maps, batch 24",
              "stress": "rendered frames/sec, 128^3 voxel->1024x1024 Phong (high-res stress), batch 8"}[mode]
    res = {
        "metric": metric, "value": round(fps, 3), "unit": "frames/s", "n_gpus": world, "steps": args.steps,
        "warmup": args.warmup, "ms_per_step": round(1e3 * elapsed / args.steps, 3), "higher_is_better": True,
        "scaling": args.scaling, "vs_baseline": None, "dtype": LINE_DTYPE[args.gemm], "gemm_mode": args.gemm, "data": "synthetic",
        "rccl_ranks": args.rccl_ranks,
        "config": {"workload": wl["name"], "batch_per_gpu": nloc if args.scaling == "weak" else "%d split over %d" % (B, world),
                   "global_batch": total_frames,
                   "parallelism": "batch-sharded x%d, no data-path collective (RCCL: timing barrier + max-reduce only)" % world},
        # throughput priced as if every conv were a direct convolution (the counting rule of SURVEY.md §8d) over the fp32
        # MFMA peak.  The Winograd kernel executes 2.25x fewer multiplies on 87 % of those FLOPs, so this number is no
        # longer bounded by 1; `roofline` below is on EXECUTED MFMA FLOPs and is.
        "direct_equiv_fraction_of_fp32_peak": round(fps / world * gmac * 2e-3 / PEAK_FP32_MFMA_TFLOPS, 4),
        "effective_tflops_direct_equiv": round(fps / world * gmac * 2e-3, 2),
        **per_rank_fields(by_rank, frames_by_rank, args.steps),
    }
    if not args.full:
        print(json.dumps(res), flush=True)
        return
    if other is not None:
        res["other_scaling"] = other
    roof = gemm_roofline(ev["gemm"], ev["layer"], wtrunk, hw, nloc, mode, args.gemm)
    if roof is not None:
        res["roofline"] = roof
    rs_events = ev["resample"]
    if rs_events:
        # second roofline of the path: the resampler is HBM-bound (per frame and channel 1 MiB (64^3) source
        # read + 8 MiB (128^3) grid written); all its launches of a step are summed
        per_step = len(rs_events) // args.steps
        rs_ms = float(np.sum([a.elapsed_time(b) for (a, b), _ in rs_events])) / args.steps
        rs_bytes = float(sum(4.0 * np.prod(sh) * (1 + 8) for _, sh in rs_events[:per_step]))
        rtraffic, rsrc = read_traffic("resampler") if (mode == "render" and nloc == 24) else (None, None)
        res["roofline_resampler"] = {
            "kernel": "resample_prepare + resample_classify + resample_main (csrc/resample_tiled.hip), %d call(s) per step" % per_step,
            "bound": "hbm", "achieved": round(rs_bytes / (rs_ms * 1e-3) / 1e9, 1), "peak": 8000.0, "unit": "GB/s",
            "frac": round(rs_bytes / (rs_ms * 1e-3) / 1e9 / 8000.0, 4), "avg_ms": round(rs_ms, 4),
            "launches_timed": len(rs_events), "bytes_per_call": rs_bytes, "traffic": rtraffic, "traffic_source": rsrc}
    # rank 0's frames as bench-batch indices (weak: rank 0 renders the un-shifted batch; strong: the first block)
    frame_ids = list(range(nloc))
    failures = []
    want = None
    if world == 1 and not args.no_cpu_baseline:
        rec, want = cpu_baseline(wl["weights"], mode, frames=min({"render": 4, "texture": 2, "stress": 1}[mode], nloc))
        got = out[:want.shape[0]].cpu().numpy()
        err = float(np.abs(got - want).max())
        res["cpu_baseline"] = rec
        # parity ON the benched configuration: the oracle's render of the first frames of this very batch vs the output of the
        # timed run (same sess.run feed as RenderNet_demo.py:47-51: voxels + pose -> encoder/output:0)
        res["parity"] = {"frames": int(want.shape[0]), "max_abs_err": err, "tol": PARITY_TOL, "ok": err <= PARITY_TOL,
                         "reference": "oracle (NumPy/torch-CPU restatement of the TF graph), fp32, run live on this box"}
        if err > PARITY_TOL:
            failures.append("max|gpu - oracle| = %g > %g on the benched frames" % (err, PARITY_TOL))
    # ... and against the committed oracle renders of the same batch: the only check of the stress line (the oracle needs
    # minutes per frame) and of every N > 1 / --no-cpu-baseline line
    gp = golden_parity(mode, out, frame_ids)
    if gp is not None:
        res["parity_golden" if "parity" in res else "parity"] = gp
        if not gp["ok"]:
            failures.append("max|gpu - committed oracle render| = %g > %g (frames %s)" % (gp["max_abs_err"], PARITY_TOL, gp["frames"]))
    for key, gm in ALT_MODES:
        if key not in alts:
            continue
        out_alt, el_alt, by_rank_alt, ev_alt = alts[key]
        fps_alt = total_frames * args.steps / el_alt
        ablk = {"dtype": ALT_DTYPE[gm], "gemm_mode": gm, "what": ALT_WHAT[gm],
                "value": round(fps_alt, 3), "unit": "frames/s", "ms_per_step": round(1e3 * el_alt / args.steps, 3),
                "steps": args.steps, "speedup_vs_value": round(fps_alt / fps, 4),
                **per_rank_fields(by_rank_alt, frames_by_rank, args.steps)}
        aroof = gemm_roofline(ev_alt["gemm"], ev_alt["layer"], wtrunk, hw, nloc, mode, gm)
        if aroof is not None:
            ablk["roofline"] = aroof
        if want is not None:
            aerr = float(np.abs(out_alt[:want.shape[0]].cpu().numpy() - want).max())
            ablk["parity"] = {"frames": int(want.shape[0]), "max_abs_err": aerr, "tol": PARITY_TOL, "ok": aerr <= PARITY_TOL,
                              "reference": "the same live oracle render as `parity`"}
            if aerr > PARITY_TOL:
                failures.append("%s (%s): max|gpu - oracle| = %g > %g" % (key, gm, aerr, PARITY_TOL))
        agp = golden_parity(mode, out_alt, frame_ids)
        if agp is not None:
            ablk["parity_golden" if "parity" in ablk else "parity"] = agp
            if not agp["ok"]:
                failures.append("%s (%s): max|gpu - committed oracle render| = %g > %g" % (key, gm, agp["max_abs_err"], PARITY_TOL))
        ablk["max_abs_diff_vs_primary_output"] = float((out_alt - out).abs().max())
        res[key] = ablk
    print(json.dumps(res), flush=True)
    if failures:
        raise SystemExit("PARITY FAILURE: " + "; ".join(failures))


WINO_SCHEMES = {"f43": (36, "F(4x4,3x3)"), "f44": (49, "F(4x4,4x4)"), "f63": (64, "F(6x6,3x3)")}   # ops._wino_scheme -> (planes, name)


def read_traffic(key):
    """HBM-side bytes per launch from profiles/traffic.json (rocprofv3 --pmc passes, scripts/collect_pmc.sh).  The file
    records the git revision of the kernel sources it was measured on; a stale file yields (None, reason)."""
    path = os.path.join(ROOT, "profiles", "traffic.json")
    try:
        tj = json.load(open(path))
        ent = tj["kernels"][key]
    except Exception:
        return None, "no entry %r in profiles/traffic.json" % key
    want = kernel_sources_digest()
    if ent.get("csrc_digest") != want:
        return None, "stale: profiles/traffic.json[%s] was collected on csrc digest %s, this build is %s" % (key, ent.get("csrc_digest"), want)
    return ent.get("hbm_bytes_per_launch"), "profiles/traffic.json[%s], git %s, csrc digest %s" % (key, ent.get("git"), want)


def kernel_sources_digest():
    """sha256 (first 12 hex) over rendernet_amd/csrc/* -- ties counter evidence to the kernels it was measured on."""
    import hashlib
    h = hashlib.sha256()
    d = os.path.join(ROOT, "rendernet_amd", "csrc")
    for n in sorted(os.listdir(d)):
        with open(os.path.join(d, n), "rb") as f:
            h.update(n.encode())
            h.update(f.read())
    return h.hexdigest()[:12]


def free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=5)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--batch", type=int, default=None, help="frames per GPU per step (weak) / per step in total (strong); "
                                                           "default 24, stress mode 8")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="skip the CPU-oracle leg (and with it the parity check)")
    ap.add_argument("--mode", choices=["render", "train", "texture", "stress"], default="render",
                    help="render = the headline metric (BASELINE configs[1]); texture = configs[2]; stress = configs[4] "
                         "(128^3 -> 1024^2, batch 8); train = the training step of configs[3] (samples/s)")
    ap.add_argument("--scaling", choices=["weak", "strong"], default="weak")
    ap.add_argument("--cpu-baseline-full", action="store_true",
                    help="run ONLY the full CPU-baseline protocol of BASELINE.md §3 (one B=24 pass + three B=1 passes of the oracle, all "
                         "cores and the best-of sweep; minutes) and print its record as one JSON line")
    ap.add_argument("--gemm", choices=["f32", "split", "split16"], default=None,
                    help="multiply-stage mode of the PRIMARY pass (`value`): default = the library default (rendernet_amd.ops.WINO_GEMM: `split`, "
                         "bf16x3 operands, unless RN_WINO_GEMM says otherwise); the other two modes are then timed as the blocks `exact` (f32), "
                         "`alt` (split), `alt2` (split16)")
    ap.add_argument("--no-alt", action="store_true", help="skip the further timed passes (the two other multiply-stage modes)")
    ap.add_argument("--no-other-scaling", action="store_true", help="N > 1: skip the pass in the other scaling regime (`other_scaling`)")
    ap.add_argument("--patch", type=int, default=64, help="train mode: crop size on the 128^3 grid (RenderNet_Shader.py:204-207)")
    ap.add_argument("--full", action="store_true",
                    help="also measure and check everything beyond the headline figure: the other two multiply-stage modes, N > 1 the other "
                         "scaling regime, the rooflines, the CPU-oracle baseline and parity, the committed-render parity.  Without it "
                         "--no-alt, --no-other-scaling and --no-cpu-baseline have nothing to skip")
    ap.add_argument("--dump-outputs", metavar="DIR", default=None,
                    help="after the timed steps, write what the timed path returned in its last step as DIR/<name>.npy (render / stress: "
                         "image; texture: image, normal; train: loss, params), at most 64 MiB in all (larger arrays: a fixed seeded "
                         "sample of their elements); N > 1: rank 0's")
    args = ap.parse_args()
    if args.batch is None:
        args.batch = 8 if args.mode == "stress" else 24
    if args.gpus < 1:
        raise SystemExit("--gpus must be >= 1")
    if args.steps < 1 or args.warmup < 0:
        raise SystemExit("--steps must be >= 1 and --warmup >= 0")

    import torch

    if args.cpu_baseline_full:
        from rendernet_amd.shader import ShaderSpec, init_shader_weights
        spec = ShaderSpec().check()
        print(json.dumps({"cpu_baseline_full": cpu_baseline_full(init_shader_weights(spec, seed=1234, perturb=True))}), flush=True)
        return
    if not torch.cuda.is_available():
        raise SystemExit("bench.py needs a HIP device (no CPU render path)")
    if args.gemm is None:
        from rendernet_amd import ops as _ops
        args.gemm = _ops.WINO_GEMM
    ndev = torch.cuda.device_count()
    env_world = os.environ.get("WORLD_SIZE")
    if env_world is None and args.gpus > 1:
        # launched as ONE process but asked for N GPUs: become the launcher (one rank per GPU over RCCL) instead of silently
        # running a single rank
        if ndev < args.gpus and not os.environ.get("RN_SHARE_GPU"):
            raise SystemExit("--gpus %d but only %d HIP device(s) are visible" % (args.gpus, ndev))
        cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", str(args.gpus),
               "--master-addr", "127.0.0.1", "--master-port", str(free_port()), os.path.abspath(__file__)] + sys.argv[1:]
        # every rank initialises 237M weights with NumPy and packs them on its GPU: give each an equal slice of the host's
        # cores instead of N x all-cores thread pools fighting each other
        env = dict(os.environ, HSA_ENABLE_IPC_MODE_LEGACY="0")
        env.setdefault("OMP_NUM_THREADS", str(max(1, (os.cpu_count() or 8) // args.gpus)))
        raise SystemExit(subprocess.call(cmd, env=env))

    import torch.distributed as dist
    world = int(env_world or "1")
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", "0"))
    if world != args.gpus:
        raise SystemExit("--gpus %d but WORLD_SIZE=%d" % (args.gpus, world))
    # RN_SHARE_GPU=1 + RN_DIST_BACKEND=gloo: several ranks on one device, control collectives over gloo -- only for
    # smoke-testing the multi-rank launch path on a single-GPU box (RCCL refuses two ranks on one device)
    if local_rank >= ndev:
        if not os.environ.get("RN_SHARE_GPU"):
            raise SystemExit("LOCAL_RANK=%d but only %d HIP device(s) visible" % (local_rank, ndev))
        local_rank %= ndev
    torch.cuda.set_device(local_rank)
    if world > 1:
        torch.set_num_threads(max(1, min(torch.get_num_threads(), (os.cpu_count() or 8) // world)))
    args.rccl_ranks = None
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")      # dmabuf IPC (RCCL across processes)
        backend = os.environ.get("RN_DIST_BACKEND", "nccl")
        if backend == "nccl":
            dist.init_process_group("nccl", rank=rank, world_size=world, device_id=torch.device("cuda", local_rank))
        else:
            dist.init_process_group(backend, rank=rank, world_size=world)
        # one real collective over the backend before anything is timed: every rank contributes 1
        one = torch.ones(1, device="cuda" if backend == "nccl" else "cpu")
        dist.all_reduce(one)
        if int(one.item()) != world:
            raise SystemExit("all-reduce over %s returned %g, expected %d" % (backend, float(one.item()), world))
        args.rccl_ranks = world if backend == "nccl" else 0
    try:
        if args.mode == "train":
            train_main(args, world, rank, local_rank)
        else:
            render_main(args, world, rank, local_rank)
    finally:
        if world > 1:
            dist.barrier()
            dist.destroy_process_group()


if __name__ == "__main__":
    main()
