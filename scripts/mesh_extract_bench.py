#!/usr/bin/env python
"""What the mesh extractor costs: `ops.extract_mesh` on the device, per call and per kernel.

    python scripts/mesh_extract_bench.py [--calls 50] [--out profiles/mesh_extract_bench.json]
                                         [--stats profiles/mesh_extract_kernel_stats.csv]
        GPU.  Shapes: the chair at 64^3 (uint8, B = 1), a 128^3 sphere field (float32, B = 1) and B = 24 procedural CSG grids at
        64^3 (uint8), smooth quads.  Per shape
          call     `calls` ops.extract_mesh calls between device events after 5 warm-up calls: count and scan, the read-back of
                   the totals, the allocations, vertices and quads
          kernels  a `rocprofv3 --kernel-trace --stats` run of its own per shape (a fresh child process: this script with
                   --leg NAME, `calls` / 5 calls), its kernel table read back: the four extract_* kernels with the bytes each must
                   move, computed from the shape and the measured (V, F), and those bytes over the kernel time as a share of the
                   8.0 TB/s HBM peak
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

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
HBM_PEAK = 8.0e12              # bytes / s, the specification (a float4 copy reaches 79 % of it)
KERNELS = ("extract_count_kernel", "extract_scan_kernel", "extract_verts_kernel", "extract_quads_kernel")
LEGS = ("chair64", "sphere128", "csg64x24")


def sphere_field(S):
    c = np.array([0.5 * S - 0.3, 0.5 * S + 0.15, 0.5 * S - 0.45])
    x = np.stack(np.meshgrid(*[np.arange(S, dtype=np.float64)] * 3, indexing="ij"), -1)
    return (0.5 + (0.37 * S - np.sqrt(((x - c) ** 2).sum(-1))) / 4.0).astype(np.float32)


def make(leg):
    """The voxels of a leg on the device: [B,S,S,S]."""
    import torch
    from rendernet_amd import ops, synth
    from rendernet_amd.tools import binvox_rw
    if leg == "chair64":
        with open(os.path.join(ROOT, "binvox", "chair.binvox"), "rb") as f:
            return torch.as_tensor(np.ascontiguousarray(binvox_rw.read_as_3d_array(f).data).astype(np.uint8)[None]).cuda()
    if leg == "sphere128":
        return torch.as_tensor(sphere_field(128)[None]).cuda()
    prims = torch.as_tensor(synth.shape_prims(1234, list(range(0x1000, 0x1000 + 24)), 64)).cuda()
    return ops.voxel_shapes(prims, 64)[..., 0].contiguous()


def kernel_bytes(B, S, item, V, F):
    """Bytes each kernel must move at least: the volume once per pass that reads it, the cell -> vertex volume written and read
    once, the workgroup totals, the outputs."""
    cells, nb = (S + 1) ** 3, ((S + 1) ** 3 + 255) // 256
    vol, ws = B * S ** 3 * item, B * nb * 8
    return {"extract_count_kernel": vol + ws, "extract_scan_kernel": 2 * ws + 8 * B,
            "extract_verts_kernel": vol + ws + 4 * B * cells + 12 * V, "extract_quads_kernel": 4 * B * cells + ws + 16 * F}


def time_leg(leg, calls):
    import torch
    from rendernet_amd import ops
    vol = make(leg)
    for _ in range(5):
        m = ops.extract_mesh(vol)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        m = ops.extract_mesh(vol)
    e1.record()
    torch.cuda.synchronize()
    B, S = int(vol.shape[0]), int(vol.shape[1])
    return {"leg": leg, "B": B, "S": S, "dtype": str(vol.dtype).split(".")[-1], "vertices": int(m.q.shape[0]), "quads": int(m.faces.shape[0]),
            "calls": calls, "us_per_call_events": e0.elapsed_time(e1) * 1e3 / calls}


def profile_leg(leg, calls, tmp):
    """Kernel rows of a rocprofv3 run of this script's --leg mode: {kernel: (calls, average ns, min ns, max ns)}, and the raw rows."""
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
        rows = list(csv.DictReader(f))
    table = {}
    for row in rows:
        for k in KERNELS:
            if k in row["Name"]:
                n, avg, lo, hi = table.get(k, (0, 0.0, float("inf"), 0.0))
                c = int(row["Calls"])
                table[k] = (n + c, (avg * n + float(row["AverageNs"]) * c) / (n + c), min(lo, float(row["MinNs"])), max(hi, float(row["MaxNs"])))
    return table, rows


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_extract_bench.json"))
    ap.add_argument("--stats", default=os.path.join(ROOT, "profiles", "mesh_extract_kernel_stats.csv"))
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--leg", choices=LEGS, default=None, help="run one shape only and print its row (what the profiled child runs)")
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mesh_extract_bench.py measures on the GPU; no HIP device found")
    if a.leg:
        print(json.dumps(time_leg(a.leg, a.calls)), flush=True)
        return
    rows = [time_leg(leg, a.calls) for leg in LEGS]
    stats = []
    if not a.no_profile:
        if shutil.which("rocprofv3") is None:
            raise SystemExit("rocprofv3 not found; --no-profile times the calls only")
        with tempfile.TemporaryDirectory() as tmp:
            for row in rows:
                table, raw = profile_leg(row["leg"], max(a.calls // 5, 5), tmp)
                need = kernel_bytes(row["B"], row["S"], 1 if row["dtype"] == "uint8" else 4, row["vertices"], row["quads"])
                row["kernels"] = {}
                for k in KERNELS:
                    if k not in table:
                        raise SystemExit("%s: no %s in the kernel table" % (row["leg"], k))
                    n, avg, lo, hi = table[k]
                    row["kernels"][k] = {"calls": n, "avg_us": avg / 1e3, "min_us": lo / 1e3, "max_us": hi / 1e3, "bytes": need[k],
                                         "gb_per_s": need[k] / avg, "hbm_peak_fraction": need[k] / (avg * 1e-9) / HBM_PEAK}
                row["kernel_us_sum"] = sum(v["avg_us"] for v in row["kernels"].values())
                stats += [dict(r, Leg=row["leg"]) for r in raw]
    result = {"mesh_extract": {"smooth": True, "triangles": False, "hbm_peak_bytes_per_s": HBM_PEAK, "rows": rows}}
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
