#!/usr/bin/env python
"""What the voxel labelling costs: `ops.voxel_components`, `ops.voxel_clean` and `ops.voxel_topology` on the device.

    python scripts/voxel_label_bench.py [--calls 50] [--out profiles/voxel_label_bench.json]
                                        [--stats profiles/voxel_label_kernel_stats.csv]
        GPU.  Legs: the five shipped models cycled at B = 1 and 24, S = 64, and doubled at S = 128; a random grid of density 0.2
        (many components, long merge chains) at 64 and 128; the 32^3 checkerboard (16384 components at connectivity 6, 13500
        cavities).  uint8 grids.  Per leg
          call     `calls` calls between device events after 3 warm-up calls, for ops.voxel_components of the solid at 26 and at
                   6 and of the empty space at 6 (the pack, the one host read of the counts and the statistics included: that is
                   the op), for ops.voxel_clean with its defaults and for ops.voxel_topology
          host     the path it replaces, on the host clock: scipy.ndimage.label (26-connected) of every grid of the batch when
                   scipy is present, otherwise the NumPy twin (tests/voxel_label_ref.py)
          kernels  one `rocprofv3 --kernel-trace --stats` run of its own (a fresh child process: this script with --leg NAME
                   --what solid26, and again with empty6), its kernel table read back: the launches of one labelling and each one's share of their sum
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
MODELS = ("bunny", "chair", "suzanne", "table", "teapot")
LEGS = {"models_b1s64": ("models", 1, 64), "models_b24s64": ("models", 24, 64), "models_b1s128": ("models", 1, 128),
        "models_b24s128": ("models", 24, 128), "random_b24s64": ("random", 24, 64), "random_b1s128": ("random", 1, 128),
        "checker_b1s32": ("checker", 1, 32)}
WHAT = ("solid26", "solid6", "empty6", "clean", "topology")
KERNELS = ("label_init_kernel", "label_merge_kernel", "label_flatten_kernel", "label_count_kernel", "label_scan_kernel",
           "label_emit_kernel", "label_write_kernel", "label_stats_clear_kernel", "label_stats_kernel")


def grids(kind, B, S):
    """uint8 [B,S,S,S] on the host."""
    if kind == "checker":
        z, y, x = np.meshgrid(np.arange(S), np.arange(S), np.arange(S), indexing="ij")
        return np.stack([((x + y + z) % 2 == 0).astype(np.uint8)] * B)
    if kind == "random":
        rng = np.random.RandomState(0)
        return np.stack([(rng.random_sample((S, S, S)) < 0.2).astype(np.uint8) for _ in range(B)])
    from rendernet_amd.tools import binvox_rw
    out = []
    for name in MODELS:
        with open(os.path.join(ROOT, "binvox", name + ".binvox"), "rb") as f:
            g = np.ascontiguousarray(binvox_rw.read_as_3d_array(f).data).astype(np.uint8)
        out.append(np.kron(g, np.ones((S // 64,) * 3, np.uint8)) if S > 64 else g)
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


def host_seconds(batch):
    """(seconds for the 26-connected labelling of the whole batch on the host, which path)."""
    occ = batch.astype(bool)
    try:
        from scipy import ndimage
        full = np.ones((3, 3, 3), bool)
        fn, how = (lambda: [ndimage.label(g, full) for g in occ]), "scipy.ndimage.label"
    except ImportError:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import voxel_label_ref
        fn, how = (lambda: [voxel_label_ref.label(g) for g in occ]), "tests/voxel_label_ref.py"
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0, how


def time_leg(leg, calls, what=None):
    import torch
    from rendernet_amd import ops
    kind, B, S = LEGS[leg]
    host = grids(kind, B, S)
    vox = torch.as_tensor(host).cuda()
    fns = {"solid26": lambda: ops.voxel_components(vox), "solid6": lambda: ops.voxel_components(vox, connectivity=6),
           "empty6": lambda: ops.voxel_components(vox, of="empty", connectivity=6), "clean": lambda: ops.voxel_clean(vox),
           "topology": lambda: ops.voxel_topology(vox)}
    row = {"leg": leg, "kind": kind, "B": B, "S": S, "calls": calls, "us_per_call_events": {}}
    for name in WHAT:
        if what in (None, name):
            row["us_per_call_events"][name] = _events(fns[name], calls)
    if what is None:
        row["components"] = ops.voxel_topology(vox).words[:, 1:3].sum(0).tolist()        # components and cavities over the batch
        sec, how = host_seconds(host)
        row["host"] = {"path": how, "us_per_batch": sec * 1e6}
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_label_bench.json"))
    ap.add_argument("--stats", default=os.path.join(ROOT, "profiles", "voxel_label_kernel_stats.csv"))
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--profile-legs", default=",".join(sorted(LEGS)), help="the legs that get a kernel table")
    ap.add_argument("--leg", choices=sorted(LEGS), default=None, help="run one leg only and print its row (what the profiled child runs)")
    ap.add_argument("--what", choices=WHAT, default=None, help="with --leg: one entry only")
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("voxel_label_bench.py measures on the GPU; no HIP device found")
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
                for what in ("solid26", "empty6"):
                    table, raw = profile_leg(row["leg"], what, max(a.calls // 5, 5), tmp)
                    if "label_merge_kernel" not in table:
                        raise SystemExit("%s %s: no label_merge_kernel in the kernel table" % (row["leg"], what))
                    total = sum(avg for _, avg in table.values())
                    row["kernels"][what] = {k: {"calls": n, "avg_us": avg / 1e3, "share": avg / total} for k, (n, avg) in table.items()}
                    stats += [dict(r, Leg=row["leg"] + " " + what) for r in raw if any(k in r["Name"] for k in KERNELS + ("voxel_pack",))]
    result = {"voxel_label": {"rows": rows}}
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
