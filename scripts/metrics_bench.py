#!/usr/bin/env python
"""What the validation metrics cost: `ops.image_metrics` on the device against the host L1 of the training scripts' validation
loop, on the same tensors.

    python scripts/metrics_bench.py [--calls 40] [--host-calls 3]    # GPU: B 24, 512 x 512, C 3; legs m h m h:
                                                                     #   m = `calls` ops.image_metrics calls (float32 prediction
                                                                     #       against uint8 target) between device events
                                                                     #   h = what the scripts do today per validation batch: the
                                                                     #       prediction's .cpu().numpy() copy and the mean of
                                                                     #       |target - pred| over float arrays, by the host clock
                                                                     #   then one leg each of the other dtype pairs (u8 u8, f32 f32);
                                                                     #   run it under `rocprofv3 --kernel-trace --stats` for the
                                                                     #   kernel times

Prints ONE JSON line.  The images: a ray-cast normal map of the five shipped models (86 % black background, like a validation
target) as the uint8 target, and as the prediction the same frames plus seeded noise, float32 in [0, 1].
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

BATCH, FRAME = 24, 512


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=40)
    ap.add_argument("--host-calls", type=int, default=3)
    a = ap.parse_args(argv)
    import torch
    from rendernet_amd import ops, synth
    if not torch.cuda.is_available():
        raise SystemExit("metrics_bench.py measures on the GPU; no HIP device found")
    models, _ = synth.read_models(os.path.join(ROOT, "binvox"))
    vox = torch.as_tensor(models[np.arange(BATCH) % len(models)]).cuda()
    az = (250.0 + np.linspace(-20.0, 20.0, BATCH)) * np.pi / 180.0
    poses = torch.as_tensor(np.stack([az, np.full(BATCH, 30.0 * np.pi / 180.0), np.ones(BATCH)], 1).astype(np.float32)).cuda()
    target = ops.raycast_normals(vox, poses, new_size=FRAME // 4, pixels_per_cell=4)          # uint8 [24,512,512,3]
    gen = torch.Generator(device="cuda").manual_seed(1234)
    pred = (target.float() / 255.0 + 0.05 * torch.randn(target.shape, device="cuda", generator=gen)).clamp_(0.0, 1.0)
    pred_u8 = (pred * 255.0).round().to(torch.uint8)
    target_f32 = target.float() / 255.0
    target_host = target.cpu().numpy().astype(np.float32) / np.float32(255.0)                 # what _validation_batches yields

    def host_l1():
        return float(np.mean(np.absolute(target_host - pred.cpu().numpy())))

    pairs = {"m": (pred, target), "u8_u8": (pred_u8, target), "f32_f32": (pred, target_f32)}
    last = None
    for x, y in pairs.values():
        for _ in range(3):
            last = ops.image_metrics(x, y)
    host_l1()
    legs = []
    for leg in ("m", "h", "m", "h", "u8_u8", "f32_f32"):
        if leg == "h":
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(a.host_calls):
                l1_host = host_l1()
            legs.append({"leg": leg, "ms_per_call_host_clock": (time.perf_counter() - t0) * 1e3 / a.host_calls})
            continue
        x, y = pairs[leg]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.calls):
            last = ops.image_metrics(x, y)
        e1.record()
        torch.cuda.synchronize()
        legs.append({"leg": leg, "us_per_call_events": e0.elapsed_time(e1) * 1e3 / a.calls})
    m = ops.image_metrics(pred, target)
    bytes_read = {"m": pred.numel() * 4 + target.numel(), "u8_u8": 2 * target.numel(), "f32_f32": 2 * pred.numel() * 4}
    print(json.dumps({"metrics": {"batch": BATCH, "frame": FRAME, "channels": 3, "calls": a.calls, "host_calls": a.host_calls,
                                  "legs": legs, "bytes_read": bytes_read,
                                  "background_share": float((target.amax(dim=3) == 0).float().mean().item()),
                                  "l1_device": float(m.l1.mean().item()), "l1_host": l1_host,
                                  "psnr_mean": float(m.psnr.mean().item()), "ssim_mean": float(m.ssim.mean().item())}}), flush=True)


if __name__ == "__main__":
    main()
