#!/usr/bin/env python
"""What carving costs: `ops.voxel_carve` on the device, against the scan that produces its views.

    python scripts/voxel_carve_bench.py [--calls 20] [--rounds 3] [--out profiles/voxel_carve_bench.json]
                                        [--stats profiles/voxel_carve_kernel_stats.csv]
        GPU.  Legs: B = 24 grids of 64^3 (the five shipped models cycled), K = 24 views of synth.scan_poses in a frame of 128
        cells, at f = 4 (512^2 views: 604 MB of views) and at f = 2 (256^2: 151 MB).  Per leg, `rounds` times in alternation
          carve    `calls` calls of ops.voxel_carve (cameras, the one carve launch, the threshold) between device events after 3
                   warm-up calls, and the same for the bare rn_voxel_carve launch on ready cameras
          scan     ops.voxel_scan of the same batch (one pack, 24 x rn_raycast_fwd + rn_hit_depth), `calls` / 4 calls
        and the median of each over the rounds; `share` = carve / (scan + carve), the carve's part of a scan-and-carve round
        trip; `gather_gb_s` = B S^3 (4 K + 1) bytes -- one view word per (voxel, view) and the vote byte -- over the launch time.
          kernels  one `rocprofv3 --kernel-trace --stats` run of its own per leg (a fresh child process: this script with --leg
                   NAME), its kernel table read back
        --no-profile leaves the kernel runs out.  RN_HIP_LIBRARY selects another build of the library (the lane mapping A/B).

Writes the JSON result and the kernel table, and prints the result as ONE JSON line.
"""
import argparse
import csv
import glob
import json
import os
import shutil
import subprocess
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
MODELS = ("bunny", "chair", "suzanne", "table", "teapot")
LEGS = {"b24_s64_k24_f4": (24, 64, 24, 4), "b24_s64_k24_f2": (24, 64, 24, 2)}
KERNELS = ("voxel_carve_kernel", "hit_depth_kernel", "mesh_camera_kernel", "raycast", "voxel_pack")
HBM_PEAK_GB_S = 8000.0


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


def time_leg(leg, calls, rounds, carve_only=False):
    import torch
    from rendernet_amd import _lib as L, ops, synth
    B, S, K, f = LEGS[leg]
    N = 2 * S
    vox = torch.as_tensor(grids(B)).cuda().unsqueeze(-1)
    p, low = synth.scan_poses(K)
    poses = torch.as_tensor(np.broadcast_to(p, (B, K, 3)).copy()).cuda()
    kw = dict(new_size=N, pixels_per_cell=f, view_from_low_x=low)
    views = ops.voxel_scan(vox, poses, **kw)
    cam = ops.carve_cameras(poses, S, **kw)
    votes = torch.empty((B, S, S, S), dtype=torch.uint8, device="cuda")
    lib, sp = L.lib(), L.stream_ptr()

    def launch():
        L.check(lib.rn_voxel_carve(ops._vp(views), ops._vp(cam), ops._vp(votes), B, K, S, N, f, 0, 0, f * N, f * N, 1, 8, 1, sp))
    row = {"leg": leg, "B": B, "S": S, "K": K, "pixels_per_cell": f, "calls": calls, "rounds": rounds,
           "views_mb": views.numel() * 4 / 1e6, "library": os.path.basename(os.path.dirname(L.LIB_PATH))}
    if carve_only:
        row["launch_us"] = _events(launch, calls)
        return row
    hull = ops.voxel_carve(views, poses, S, **kw)
    row["hulls_equal_to_their_grid"] = int((hull == (vox > 0).to(torch.uint8)).flatten(1).all(1).sum())
    row["lost_voxels"] = int(((vox > 0) & (hull == 0)).sum())
    t = {"carve_us": [], "launch_us": [], "scan_us": []}
    for _ in range(rounds):
        t["carve_us"].append(_events(lambda: ops.voxel_carve(views, poses, S, **kw), calls))
        t["launch_us"].append(_events(launch, calls))
        t["scan_us"].append(_events(lambda: ops.voxel_scan(vox, poses, **kw), max(calls // 4, 2)))
    row["rounds_us"] = t
    for k, v in t.items():
        row[k] = float(np.median(v))
    row["share"] = row["carve_us"] / (row["carve_us"] + row["scan_us"])
    nbytes = B * S ** 3 * (4 * K + 1)
    row["gather_gb_s"] = nbytes / row["launch_us"] / 1e3
    row["gather_share_of_hbm_peak"] = row["gather_gb_s"] / HBM_PEAK_GB_S
    return row


def profile_leg(leg, calls, tmp):
    out = os.path.join(tmp, leg)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "p", "--",
           sys.executable, os.path.abspath(__file__), "--leg", leg, "--calls", str(calls)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit("rocprofv3 failed for %s:\n%s" % (leg, r.stderr[-2000:]))
    found = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    if not found:
        raise SystemExit("rocprofv3 left no kernel_stats.csv for %s" % leg)
    with open(found[0]) as f:
        return [r_ for r_ in csv.DictReader(f) if any(k in r_["Name"] for k in KERNELS)]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_carve_bench.json"))
    ap.add_argument("--stats", default=os.path.join(ROOT, "profiles", "voxel_carve_kernel_stats.csv"))
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--leg", choices=sorted(LEGS), default=None, help="the bare launch of one leg only (what the profiled child runs)")
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("voxel_carve_bench.py measures on the GPU; no HIP device found")
    if a.leg:
        print(json.dumps(time_leg(a.leg, a.calls, 1, carve_only=True)), flush=True)
        return
    rows = [time_leg(leg, a.calls, a.rounds) for leg in LEGS]
    stats = []
    if not a.no_profile:
        if shutil.which("rocprofv3") is None:
            raise SystemExit("rocprofv3 not found; --no-profile times the calls only")
        with tempfile.TemporaryDirectory() as tmp:
            for row in rows:
                raw = profile_leg(row["leg"], a.calls, tmp)
                mine = [r for r in raw if "voxel_carve_kernel" in r["Name"]]
                if not mine:
                    raise SystemExit("%s: no voxel_carve_kernel in the kernel table" % row["leg"])
                row["kernel_avg_us"] = float(mine[0]["AverageNs"]) / 1e3
                stats += [dict(r, Leg=row["leg"]) for r in raw]
    result = {"voxel_carve": {"rows": rows}}
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    if stats:
        with open(a.stats, "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=["Leg"] + [k for k in stats[0] if k != "Leg"], quoting=csv.QUOTE_NONNUMERIC)
            w.writeheader()
            w.writerows(stats)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
