#!/usr/bin/env python
"""What the voxel distance transform and the shape metrics cost: `ops.voxel_edt` and `ops.voxel_shape_metrics` on the device.

    python scripts/voxel_edt_bench.py [--calls 50] [--out profiles/voxel_edt_bench.json]
                                      [--stats profiles/voxel_edt_kernel_stats.csv]
        GPU.  Legs: B = 1 and 24 at S = 64 and 128, the five shipped models cycled (at 128 each model doubled), uint8 grids.
        Per leg
          call     `calls` calls between device events after 3 warm-up calls, for ops.voxel_edt in each seed set (the pack
                   included: the op takes voxels) and for ops.voxel_shape_metrics of every grid against its neighbour in the cycle
          host     the path it replaces, on the host clock: scipy.ndimage.distance_transform_edt of one grid when scipy is
                   present, otherwise the NumPy twin (tests/voxel_edt_ref.py), times B
          kernels  one `rocprofv3 --kernel-trace --stats` run of its own (a fresh child process: this script with --leg NAME),
                   its kernel table read back: the plane and the column kernel with the bytes each must move and those bytes
                   over the kernel time as a share of the 8.0 TB/s HBM peak
        --no-profile leaves the kernel runs out.

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
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12              # bytes / s, the specification
MODELS = ("bunny", "chair", "suzanne", "table", "teapot")
SEEDS = ("solid", "empty", "surface", "signed")
LEGS = {"b1s64": (1, 64), "b24s64": (24, 64), "b1s128": (1, 128), "b24s128": (24, 128)}
KERNELS = ("edt_plane_kernel", "edt_column_kernel")


def grids(B, S):
    """uint8 [B,S,S,S] on the host: the models cycled, doubled for S = 128."""
    from rendernet_amd.tools import binvox_rw
    out = []
    for name in MODELS:
        with open(os.path.join(ROOT, "binvox", name + ".binvox"), "rb") as f:
            g = np.ascontiguousarray(binvox_rw.read_as_3d_array(f).data).astype(np.uint8)
        out.append(np.kron(g, np.ones((S // 64,) * 3, np.uint8)) if S > 64 else g)
    return np.stack([out[b % len(out)] for b in range(B)])


def kernel_bytes(B, S, what):
    """Bytes the two launches must move at least: the bits read, the 16-bit intermediate written once and read once, the int32
    field written (the transform) or nothing (the metrics, both directions, which read the bits of both grids again)."""
    vox = B * S ** 3
    if what == "metrics":
        return {"edt_plane_kernel": 2 * (vox // 8 + 2 * vox), "edt_column_kernel": 2 * (2 * vox + 2 * vox // 8)}
    passes = 2 if what == "signed" else 1
    return {"edt_plane_kernel": passes * (vox // 8 + 2 * vox), "edt_column_kernel": passes * (2 * vox + 4 * vox) + (4 * vox if passes == 2 else 0)}


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


def host_seconds(grid):
    """(seconds for one grid's solid transform on the host, which path)."""
    occ = grid.astype(bool)
    try:
        from scipy import ndimage
        fn, how = (lambda: ndimage.distance_transform_edt(~occ)), "scipy.ndimage.distance_transform_edt"
    except ImportError:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import voxel_edt_ref
        fn, how = (lambda: voxel_edt_ref.edt(occ, "solid")), "tests/voxel_edt_ref.py"
    fn()
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0, how


def time_leg(leg, calls, what=None):
    import torch
    from rendernet_amd import ops
    B, S = LEGS[leg]
    host = grids(B, S)
    vox = torch.as_tensor(host).cuda()
    other = torch.roll(vox, 1, 0) if B > 1 else torch.as_tensor(grids(2, S)[1:]).cuda()
    row = {"leg": leg, "B": B, "S": S, "calls": calls, "us_per_call_events": {}}
    for seeds in SEEDS:
        if what in (None, seeds):
            row["us_per_call_events"][seeds] = _events(lambda: ops.voxel_edt(vox, seeds=seeds), calls)
    if what in (None, "metrics"):
        row["us_per_call_events"]["metrics"] = _events(lambda: ops.voxel_shape_metrics(vox, other), calls)
    if what in (None, "pack"):
        row["us_per_call_events"]["pack"] = _events(lambda: ops.voxel_pack(vox), calls)
    if what is None:
        sec, how = host_seconds(host[0])
        row["host"] = {"path": how, "us_per_grid": sec * 1e6, "us_per_batch": sec * 1e6 * B}
    return row


def profile_leg(leg, what, calls, tmp):
    """Kernel rows of a rocprofv3 run of this script's --leg mode: {kernel: (calls, average ns)}, and the raw rows."""
    out = os.path.join(tmp, leg + "_" + what)
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", out, "-o", "p", "--",
           sys.executable, os.path.abspath(__file__), "--leg", leg, "--what", what, "--calls", str(calls)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit("rocprofv3 failed for %s:\n%s" % (leg, r.stderr[-2000:]))
    found = glob.glob(os.path.join(out, "**", "*kernel_stats.csv"), recursive=True)
    if not found:
        raise SystemExit("rocprofv3 left no kernel_stats.csv for %s" % leg)
    with open(found[0]) as f:
        rows = list(csv.DictReader(f))
    table = {}
    for r_ in rows:
        for k in KERNELS:
            if k in r_["Name"]:
                n, avg = table.get(k, (0, 0.0))
                c = int(r_["Calls"])
                table[k] = (n + c, (avg * n + float(r_["AverageNs"]) * c) / (n + c))
    return table, rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_edt_bench.json"))
    ap.add_argument("--stats", default=os.path.join(ROOT, "profiles", "voxel_edt_kernel_stats.csv"))
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--profile-legs", default=",".join(sorted(LEGS)), help="the legs that get a kernel table")
    ap.add_argument("--leg", choices=sorted(LEGS), default=None, help="run one leg only and print its row (what the profiled child runs)")
    ap.add_argument("--what", choices=SEEDS + ("metrics", "pack"), default=None, help="with --leg: one entry only")
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("voxel_edt_bench.py measures on the GPU; no HIP device found")
    if a.leg:
        print(json.dumps(time_leg(a.leg, a.calls, a.what)), flush=True)
        return
    rows = [time_leg(leg, a.calls) for leg in LEGS]
    stats = []
    if not a.no_profile:
        if shutil.which("rocprofv3") is None:
            raise SystemExit("rocprofv3 not found; --no-profile times the calls only")
        with tempfile.TemporaryDirectory() as tmp:
            for row in rows:
                if row["leg"] not in a.profile_legs.split(","):
                    continue
                row["kernels"] = {}
                for what in ("solid", "metrics"):
                    table, raw = profile_leg(row["leg"], what, max(a.calls // 5, 5), tmp)
                    need = kernel_bytes(row["B"], row["S"], what)
                    row["kernels"][what] = {}
                    for k in KERNELS:
                        if k not in table:
                            raise SystemExit("%s %s: no %s in the kernel table" % (row["leg"], what, k))
                        n, avg = table[k]
                        row["kernels"][what][k] = {"calls": n, "avg_us": avg / 1e3, "bytes": need[k],
                                                   "hbm_peak_fraction": need[k] / (avg * 1e-9) / HBM_PEAK}
                    stats += [dict(r, Leg=row["leg"] + " " + what) for r in raw]
    result = {"voxel_edt": {"hbm_peak_bytes_per_s": HBM_PEAK, "rows": rows}}
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
