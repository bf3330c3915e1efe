#!/usr/bin/env python
"""What the ray-cast targets cost: the two kernels alone, and the --synthetic training loop against the same loop on a
resident batch.

    python scripts/raycast_bench.py cast  [--calls 40]          # GPU: B 24, 64^3 -> 512^2, the five models cycled, the demo
                                                                #      pose with +-20 degrees of azimuth; run it under
                                                                #      `rocprofv3 --kernel-trace --stats` for the kernel times
    python scripts/raycast_bench.py ao    [--calls 40]          # GPU: ops.raycast_ao (L 16, default smoothing) on the same batch,
                                                                #      legs n a n a against ops.raycast_normals on the same visit;
                                                                #      under rocprofv3 as above for the kernel times
    python scripts/raycast_bench.py lines [--calls 40]          # GPU: ops.raycast_outline and ops.raycast_cel (defaults) on the same
                                                                #      batch, legs n o c n o c against ops.raycast_normals;
                                                                #      under rocprofv3 as above for the kernel times
    python scripts/raycast_bench.py shadow [--calls 40]         # GPU: ops.raycast_shadow (defaults) on the same batch, legs n s n s
                                                                #      against ops.raycast_normals; under rocprofv3 as above for
                                                                #      the kernel times
    python scripts/raycast_bench.py albedo [--calls 40]         # GPU: ops.raycast_albedo (K 199, default smoothing) on the same batch,
                                                                #      legs n a n a against ops.raycast_normals, then the two albedo
                                                                #      kernels alone on the hits of that batch; under rocprofv3 as
                                                                #      above for the kernel times
    python scripts/raycast_bench.py shapes [--calls 40]         # GPU: ops.voxel_shapes (B 24, 64^3, eight live slots per item), legs
                                                                #      s c s c against rn_voxel_pack + rn_raycast_fwd
                                                                #      (ops.raycast_normals) on the grids it made; under rocprofv3
                                                                #      as above for the kernel times
    python scripts/raycast_bench.py train [--steps 30]          # GPU: ms/step of RenderNet_Shader.py's loop, legs s c s c:
                                                                #      s = batches from rendernet_amd.synth (cast every step),
                                                                #      c = one resident batch replayed (no caster at all)
    python scripts/raycast_bench.py train_texture [--steps 30]  # GPU: the same for RenderNet_Texture_Face_Normal.py's loop, fed by
                                                                #      synth.SyntheticTextureTargets against one resident batch

Every stage prints ONE JSON line.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

BATCH, CROP = 24, 64


def _models():
    from rendernet_amd import synth
    return synth.read_models(os.path.join(ROOT, "binvox"))


def _cast_batch():
    import torch
    models, names = _models()
    vox = torch.as_tensor(models[np.arange(BATCH) % len(models)]).cuda()
    az = (250.0 + np.linspace(-20.0, 20.0, BATCH)) * np.pi / 180.0
    poses = torch.as_tensor(np.stack([az, np.full(BATCH, 30.0 * np.pi / 180.0), np.ones(BATCH)], 1).astype(np.float32)).cuda()
    return vox, poses


def stage_cast(a):
    import torch
    from rendernet_amd import ops
    vox, poses = _cast_batch()
    for _ in range(3):
        out = ops.raycast_normals(vox, poses)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.calls):
        out = ops.raycast_normals(vox, poses)
    e1.record()
    torch.cuda.synchronize()
    hit = float((out.amax(dim=3) > 0).float().mean().item())
    print(json.dumps({"cast": {"batch": BATCH, "frame": 512, "calls": a.calls, "hit_share": hit,
                               "us_per_call_events": e0.elapsed_time(e1) * 1e3 / a.calls}}), flush=True)


def stage_ao(a):
    """ops.raycast_ao against ops.raycast_normals, alternating legs of `calls` calls each between device events."""
    import torch
    from rendernet_amd import ops
    vox, poses = _cast_batch()
    fns = {"n": lambda: ops.raycast_normals(vox, poses), "a": lambda: ops.raycast_ao(vox, poses, max_distance=16)}
    for fn in fns.values():
        for _ in range(3):
            out = fn()
    legs = []
    for leg in ("n", "a", "n", "a"):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            out = fns[leg]()
        e1.record()
        torch.cuda.synchronize()
        legs.append({"leg": leg, "us_per_call_events": e0.elapsed_time(e1) * 1e3 / a.calls})
    hit = out > 0
    print(json.dumps({"ao": {"batch": BATCH, "frame": 512, "calls": a.calls, "max_distance": 16, "smooth": 4, "legs": legs,
                             "hit_share": float(hit.float().mean().item()),
                             "mean_byte_of_hits": float(out[hit].float().mean().item())}}), flush=True)


def stage_lines(a):
    """ops.raycast_outline and ops.raycast_cel against ops.raycast_normals, alternating legs of `calls` calls each."""
    import torch
    from rendernet_amd import ops
    vox, poses = _cast_batch()
    fns = {"n": lambda: ops.raycast_normals(vox, poses), "o": lambda: ops.raycast_outline(vox, poses),
           "c": lambda: ops.raycast_cel(vox, poses)}
    last = {}
    for k, fn in fns.items():
        for _ in range(3):
            last[k] = fn()
    legs = []
    for leg in ("n", "o", "c", "n", "o", "c"):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            last[leg] = fns[leg]()
        e1.record()
        torch.cuda.synchronize()
        legs.append({"leg": leg, "us_per_call_events": e0.elapsed_time(e1) * 1e3 / a.calls})
    hit = last["n"].amax(dim=3) > 0
    _, edge = ops.raycast_outline(vox, poses, return_edges=True)
    print(json.dumps({"lines": {"batch": BATCH, "frame": 512, "calls": a.calls, "normal_radius": 2, "line_radius": 2,
                                "depth_gap": 2, "crease_q": 4, "levels": 4, "legs": legs,
                                "hit_share": float(hit.float().mean().item()),
                                "ink_share_of_hits": float((last["o"][hit] == 0).float().mean().item()),
                                "bit_shares_of_hits": [float(((edge[hit] & b) != 0).float().mean().item()) for b in (1, 2, 4)],
                                "mean_cel_byte_of_hits": float(last["c"][hit].float().mean().item())}}), flush=True)


def stage_shadow(a):
    """ops.raycast_shadow against ops.raycast_normals, alternating legs of `calls` calls each."""
    import torch
    from rendernet_amd import ops
    vox, poses = _cast_batch()
    fns = {"n": lambda: ops.raycast_normals(vox, poses), "s": lambda: ops.raycast_shadow(vox, poses)}
    last = {}
    for k, fn in fns.items():
        for _ in range(3):
            last[k] = fn()
    legs = []
    for leg in ("n", "s", "n", "s"):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            last[leg] = fns[leg]()
        e1.record()
        torch.cuda.synchronize()
        legs.append({"leg": leg, "us_per_call_events": e0.elapsed_time(e1) * 1e3 / a.calls})
    out, normals, _, _, _, lit = ops.raycast_shadow(vox, poses, return_parts=True)
    hit = lit <= 1
    lq = ops.quantise_light(ops._demo_light())
    facing = sum(lq[k] * (2 * normals[..., k].int() - 255) for k in range(3)) > 0
    print(json.dumps({"shadow": {"batch": BATCH, "frame": 512, "calls": a.calls, "normal_radius": 2, "bias": 1, "smooth": 4,
                                 "ambient_byte": 26, "legs": legs, "hit_share": float(hit.float().mean().item()),
                                 "lit_share_of_hits": float((lit[hit] == 1).float().mean().item()),
                                 "shadowed_share_of_hits": float((lit[hit] == 0).float().mean().item()),
                                 "shadowed_with_positive_diffuse_share_of_hits": float(((lit == 0) & facing)[hit].float().mean().item()),
                                 "mean_byte_of_hits": float(out[hit].float().mean().item())}}), flush=True)


def stage_albedo(a):
    """ops.raycast_albedo against ops.raycast_normals, alternating legs of `calls` calls each; then rn_raycast_albedo_fwd
    (albedo_from_hits, smooth 0) and that plus rn_albedo_encode (smooth 4) alone on the hits of the batch."""
    import torch
    from rendernet_amd import ops, synth
    vox, poses = _cast_batch()
    colour = synth.ColourModel(1234, 199)
    waves = torch.as_tensor(colour.waves).cuda()
    q = torch.as_tensor(colour.quantise(np.random.default_rng(0).standard_normal((BATCH, 199)))).cuda()
    _, hit, _ = ops.raycast_normals(vox, poses, return_hits=True)
    fns = {"n": lambda: ops.raycast_normals(vox, poses), "a": lambda: ops.raycast_albedo(vox, poses, waves, q, colour.base)[0],
           "fwd": lambda: ops.albedo_from_hits(hit, waves, q, 64, colour.base, 0),
           "fwd+encode": lambda: ops.albedo_from_hits(hit, waves, q, 64, colour.base, 4)}
    last = {}
    for k, fn in fns.items():
        for _ in range(3):
            last[k] = fn()
    legs = []
    for leg in ("n", "a", "n", "a", "fwd", "fwd+encode", "fwd", "fwd+encode"):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            last[leg] = fns[leg]()
        e1.record()
        torch.cuda.synchronize()
        legs.append({"leg": leg, "us_per_call_events": e0.elapsed_time(e1) * 1e3 / a.calls})
    ok = hit >= 0
    plain = last["fwd"][ok].float()
    print(json.dumps({"albedo": {"batch": BATCH, "frame": 512, "calls": a.calls, "waves": 199, "smooth": 4, "legs": legs,
                                 "hit_share": float(ok.float().mean().item()),
                                 "std_of_hits_per_channel": [float(v) for v in plain.std(0).tolist()],
                                 "clamped_share_of_hit_values": float(((plain == 0) | (plain == 255)).float().mean().item()),
                                 "mean_of_hits_per_channel": [float(v) for v in last["a"][ok].float().mean(0).tolist()]}}), flush=True)


def shape_batch():
    """prims int32 [24,8,16] with all eight slots live: the drawn primitives of shapes 0, 1, 2, ... of synth.shape_prims(1234)
    in a row, eight to an item, the first of each item a union."""
    from rendernet_amd import synth
    drawn = synth.shape_prims(1234, np.arange(4 * BATCH), 64)
    live = drawn[drawn[:, :, 0] != synth.SHAPE_NOOP]
    prims = np.ascontiguousarray(live[:8 * BATCH].reshape(BATCH, 8, 16))
    prims[:, 0, 0] &= 255
    return prims


def stage_shapes(a):
    """ops.voxel_shapes against ops.raycast_normals (pack + cast) on the grids it made, alternating legs of `calls` calls each."""
    import torch
    from rendernet_amd import ops
    prims = torch.as_tensor(shape_batch()).cuda()
    _, poses = _cast_batch()
    vox = ops.voxel_shapes(prims, 64)
    fns = {"s": lambda: ops.voxel_shapes(prims, 64), "c": lambda: ops.raycast_normals(vox, poses)}
    last = {}
    for k, fn in fns.items():
        for _ in range(3):
            last[k] = fn()
    legs = []
    for leg in ("s", "c", "s", "c"):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            last[leg] = fns[leg]()
        e1.record()
        torch.cuda.synchronize()
        legs.append({"leg": leg, "us_per_call_events": e0.elapsed_time(e1) * 1e3 / a.calls})
    fill = last["s"].float().mean(dim=(1, 2, 3, 4))
    print(json.dumps({"shapes": {"batch": BATCH, "size": 64, "slots": 8, "calls": a.calls, "legs": legs,
                                 "store_bytes": int(last["s"].numel()),
                                 "fill_share_min_mean_max": [float(fill.min().item()), float(fill.mean().item()), float(fill.max().item())],
                                 "hit_share": float((last["c"].amax(dim=3) > 0).float().mean().item())}}), flush=True)


def stage_train_texture(a):
    """The loop of RenderNet_Texture_Face_Normal.train on one GPU: window draw, TextureTrainer.step, loss.item()."""
    import torch
    from rendernet_amd import synth
    from rendernet_amd.texture import TextureSpec, init_texture_weights
    from rendernet_amd.train import TextureTrainer
    models, names = _models()
    spec = TextureSpec().check()
    tr = TextureTrainer(spec, init_texture_weights(spec, seed=1234), keep_prob=0.75)
    colour = synth.ColourModel(1234, spec.z_dim)
    resident, legs = None, []

    def replay():
        while True:
            yield resident

    for k, leg in enumerate(("s", "c", "s", "c")):
        feed = synth.SyntheticTextureTargets(models, names, BATCH, a.warmup + a.steps, [1234, k], colour, device=tr.device) \
            if leg == "s" else replay()
        done, t0 = 0, None
        for images, normals, vox, tex, poses, _ in feed:
            if done == a.warmup:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            start = torch.randint(0, spec.new_size - CROP + 1, (2,), device="cuda")
            loss = tr.step(vox, tex, poses, images, normals, patch_size=CROP, start_point=start.tolist(), global_batch=BATCH)
            float(loss.item())
            if resident is None:
                resident = (images.clone(), normals.clone(), vox.clone(), tex.clone(), poses.clone(), None)
            done += 1
            if done >= a.warmup + a.steps:
                break
        torch.cuda.synchronize()
        legs.append({"leg": leg, "ms_per_step": (time.perf_counter() - t0) * 1e3 / a.steps})
        print(json.dumps(legs[-1]), flush=True)
    print(json.dumps({"train_texture": {"legs": legs, "batch": BATCH, "crop": CROP, "steps": a.steps, "warmup": a.warmup}}), flush=True)


def stage_train(a):
    """The loop of RenderNet_Shader.train on one GPU: window draw, Trainer.step, loss.item()."""
    import torch
    from rendernet_amd import synth
    from rendernet_amd.shader import ShaderSpec, init_shader_weights
    from rendernet_amd.train import Trainer
    models, names = _models()
    spec = ShaderSpec(out_ch=3).check()
    tr = Trainer(spec, init_shader_weights(spec, seed=1234), keep_prob=0.75)
    resident, legs = None, []

    def replay():
        while True:
            yield resident

    for k, leg in enumerate(("s", "c", "s", "c")):
        feed = synth.SyntheticTargets(models, names, BATCH, a.warmup + a.steps, [1234, k], device=tr.device) if leg == "s" else replay()
        done, t0 = 0, None
        for frames, vox, poses, _ in feed:
            if done == a.warmup:
                torch.cuda.synchronize()
                t0 = time.perf_counter()
            start = torch.randint(0, spec.new_size - CROP + 1, (2,), device="cuda")
            loss = tr.step(vox, poses, frames, patch_size=CROP, start_point=start.tolist(), global_batch=BATCH)
            float(loss.item())
            if resident is None:
                resident = (frames.clone(), vox.clone(), poses.clone(), None)
            done += 1
            if done >= a.warmup + a.steps:
                break
        torch.cuda.synchronize()
        legs.append({"leg": leg, "ms_per_step": (time.perf_counter() - t0) * 1e3 / a.steps})
        print(json.dumps(legs[-1]), flush=True)
    print(json.dumps({"train": {"legs": legs, "batch": BATCH, "crop": CROP, "steps": a.steps, "warmup": a.warmup}}), flush=True)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("stage", choices=("cast", "ao", "lines", "shadow", "albedo", "shapes", "train", "train_texture"))
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--steps", type=int, default=30)
    ap.add_argument("--warmup", type=int, default=5)
    a = ap.parse_args(argv)
    {"cast": stage_cast, "ao": stage_ao, "lines": stage_lines, "shadow": stage_shadow, "albedo": stage_albedo,
     "shapes": stage_shapes, "train": stage_train, "train_texture": stage_train_texture}[a.stage](a)


if __name__ == "__main__":
    main()
