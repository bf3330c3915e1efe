#!/usr/bin/env python
"""What colouring costs: `ops.voxel_colour_sums` on the device, against the same sums done with torch `index_add_`.

    python scripts/voxel_colour_bench.py [--calls 10] [--rounds 3] [--out profiles/voxel_colour_bench.json]
        GPU.  Legs: B = 24 grids of 64^3 (the five shipped models cycled), K = 24 views of synth.scan_poses in a frame of 128
        cells, at f = 4 (512^2 pictures: 453 MB of pictures, 604 MB of hits) and at f = 2 (256^2).  The hits are
        ops.voxel_scan's; the pictures are random bytes, which cost what real ones cost.  Per leg, `rounds` times in alternation
          accumulate  `calls` calls of ops.voxel_colour_sums into the same sums between device events after 3 warm-up calls,
                      and the same for the bare rn_voxel_colour_accumulate launch
          index_add   the baseline, NOT code of the project: sums.view(-1, 4).index_add_(0, rows, values) with the destination
                      rows (int64) and the (r, g, b, 1) values (int32) of the pixels that count made BEFORE the clock starts --
                      its best case: neither the range test nor the gather of the bytes is timed
          resolve     ops.voxel_colours of the sums (one launch), and with fill = 4 (pack + 4 passes)
        and the median of each over the rounds.  `speedup` = index_add / launch.  `runs_per_pixel` = runs of equal neighbouring
        hit ids in memory order over the pixels that count: the atomics the kernel issues are 4 per run against the baseline's
        4 per pixel.  The two sums are compared word for word before anything is timed.

Writes the JSON result and prints it as ONE JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
MODELS = ("bunny", "chair", "suzanne", "table", "teapot")
LEGS = {"b24_s64_k24_f4": (24, 64, 24, 4), "b24_s64_k24_f2": (24, 64, 24, 2)}


def grids(B):
    from rendernet_amd.tools import binvox_rw
    out = []
    for name in MODELS:
        with open(os.path.join(ROOT, "binvox", name + ".binvox"), "rb") as f:
            out.append(np.ascontiguousarray(binvox_rw.read_as_3d_array(f).data).astype(np.uint8))
    return np.stack([out[b % len(out)] for b in range(B)])


def _events(fn, calls):
    import torch
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def time_leg(leg, calls, rounds):
    import torch
    from rendernet_amd import _lib as L, ops, synth
    B, S, K, f = LEGS[leg]
    N = 2 * S
    vox = torch.as_tensor(grids(B)).cuda().unsqueeze(-1)
    p, low = synth.scan_poses(K)
    poses = torch.as_tensor(np.broadcast_to(p, (B, K, 3)).copy()).cuda()
    _, hits = ops.voxel_scan(vox, poses, new_size=N, pixels_per_cell=f, view_from_low_x=low, return_hits=True)
    ph = pw = f * N
    images = torch.randint(0, 256, (B, K, ph, pw, 3), dtype=torch.uint8, device="cuda",
                           generator=torch.Generator(device="cuda").manual_seed(1))
    lib, sp = L.lib(), L.stream_ptr()
    sums = torch.zeros((B, S, S, S, 4), dtype=torch.int32, device="cuda")

    def launch():
        L.check(lib.rn_voxel_colour_accumulate(ops._vp(images), ops._vp(hits), None, ops._vp(sums), B, K, S, ph, pw, sp))

    # the baseline's inputs, made outside the clock
    counts = (hits >= 0) & (hits < S ** 3)
    item = torch.arange(B, device="cuda").view(B, 1, 1, 1).expand_as(hits)
    rows = (item.long() * S ** 3 + hits.long())[counts]
    values = torch.cat([images[counts].to(torch.int32), torch.ones((rows.numel(), 1), dtype=torch.int32, device="cuda")], 1)
    base = torch.zeros((B * S ** 3, 4), dtype=torch.int32, device="cuda")
    once = ops.voxel_colour_sums(images, hits, S)
    base.index_add_(0, rows, values)
    if not torch.equal(once.view(-1, 4), base):
        raise SystemExit("%s: the kernel's sums differ from index_add_'s" % leg)
    flat = torch.where(counts, hits, torch.full_like(hits, -1)).view(B, -1)
    heads = (flat >= 0) & torch.cat([torch.ones((B, 1), dtype=torch.bool, device="cuda"), flat[:, 1:] != flat[:, :-1]], 1)
    row = {"leg": leg, "B": B, "S": S, "K": K, "pixels_per_cell": f, "calls": calls, "rounds": rounds,
           "pixels": int(hits.numel()), "pixels_that_count": int(rows.numel()), "voxels_seen": int((once[..., 3] > 0).sum()),
           "runs_per_pixel": float(heads.sum()) / max(int(rows.numel()), 1), "sums_equal_to_index_add": True}
    del flat, heads, item, counts
    t = {"accumulate_us": [], "launch_us": [], "index_add_us": [], "resolve_us": [], "resolve_fill4_us": []}
    for _ in range(rounds):
        t["accumulate_us"].append(_events(lambda: ops.voxel_colour_sums(images, hits, S, sums=sums), calls))
        sums.zero_()
        t["launch_us"].append(_events(launch, calls))
        sums.zero_()
        t["index_add_us"].append(_events(lambda: base.index_add_(0, rows, values), calls))
        base.zero_()
        t["resolve_us"].append(_events(lambda: ops.voxel_colours(once), calls))
        t["resolve_fill4_us"].append(_events(lambda: ops.voxel_colours(once, vox, fill=4), calls))
    row["rounds_us"] = t
    for k, v in t.items():
        row[k] = float(np.median(v))
    row["speedup"] = row["index_add_us"] / row["launch_us"]
    row["read_gb_s"] = hits.numel() * 7 / row["launch_us"] / 1e3          # 4 bytes of hit and 3 of colour per pixel, at most
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--legs", nargs="*", choices=sorted(LEGS), default=sorted(LEGS, reverse=True))
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_colour_bench.json"))
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("voxel_colour_bench.py measures on the GPU; no HIP device found")
    result = {"voxel_colour": {"rows": [time_leg(leg, a.calls, a.rounds) for leg in a.legs]}}
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
