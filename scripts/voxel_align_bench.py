#!/usr/bin/env python
"""What registration costs: `ops.voxel_align` on the device, against the NumPy twin and a plain torch formulation.

    python scripts/voxel_align_bench.py [--calls 20] [--rounds 3] [--out profiles/voxel_align_bench.json]
                                        [--stats profiles/voxel_align_kernel_stats.csv]
        GPU.  The workload: B = 24 pairs of 64^3, the five shipped models cycled, each moved by a seeded (o, t) with |t| <= 4 per
        axis; R = 8.  Legs: orientations "rotations" (24) and "all" (48).  Per leg, `rounds` times in alternation
          align    `calls` calls of ops.voxel_align (two packs, orient, correlate, winner) between device events after 3 warm-up
                   calls
          launch   the same for the bare rn_voxel_align entry on packed grids (orient + correlate + winner)
          orient   the same for the bare rn_voxel_orient entry (the oriented copies alone)
        and the median of each over the rounds.  `word_popcounts_per_s` = B n_orient (2R+1)^3 S^3/32 over the launch time.
          torch    one orientation's table of ONE pair as plain torch on the device -- the 2R+1 copies of A shifted along x stacked
                   once, then per (tz, ty) a slice, an & and a sum -- `calls` / 4 calls; `torch_pair_orientation_us`, and
                   `speedup_over_torch` = B n_orient times that over the launch time
          twin     tests/voxel_align_ref.py on the host, one orientation of one pair, once: `twin_pair_orientation_s`
          kernels  one `rocprofv3 --kernel-trace --stats` run of its own per leg (a fresh child process: this script with --leg
                   NAME), its kernel table read back: the correlate, orient and winner launches separately.  No counters.
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
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
MODELS = ("bunny", "chair", "suzanne", "table", "teapot")
LEGS = {"b24_s64_r8_rotations": (24, 64, 8, "rotations"), "b24_s64_r8_all": (24, 64, 8, "all")}
KERNELS = ("correlate_kernel", "orient_kernel", "winner_kernel", "voxel_pack")
SEED = 20


def pairs(B, n_orient):
    """(moving, fixed) uint8 [B,64,64,64]: every model against itself moved by a seeded (o, t)."""
    import voxel_align_ref as R
    rng = np.random.default_rng(SEED)
    fixed = [R.load_binvox(MODELS[b % len(MODELS)]) for b in range(B)]
    moves = [(int(rng.integers(n_orient)), tuple(int(v) for v in rng.integers(-4, 5, 3))) for _ in range(B)]
    moving = [R.transform(g, *m) for g, m in zip(fixed, moves)]
    return np.stack(moving).astype(np.uint8), np.stack(fixed).astype(np.uint8), moves


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


def torch_table(a, b, R):
    """One orientation's table of one pair, a and b bool [S,S,S] on the device: shift, &, sum."""
    import torch
    S, T = a.shape[0], 2 * R + 1
    ax = torch.zeros((T, S, S, S), dtype=torch.bool, device=a.device)
    for k, tx in enumerate(range(-R, R + 1)):
        ax[k, :, :, max(tx, 0):S + min(tx, 0)] = a[:, :, max(-tx, 0):S - max(tx, 0)]
    out = torch.zeros((T, T, T), dtype=torch.int32, device=a.device)
    for i, tz in enumerate(range(-R, R + 1)):
        for j, ty in enumerate(range(-R, R + 1)):
            src = ax[:, max(-tz, 0):S - max(tz, 0), max(-ty, 0):S - max(ty, 0)]
            dst = b[max(tz, 0):S + min(tz, 0), max(ty, 0):S + min(ty, 0)]
            out[i, j] = (src & dst).sum((1, 2, 3))
    return out


def time_leg(leg, calls, rounds, launch_only=False):
    import torch
    import voxel_align_ref as R
    from rendernet_amd import _lib as L, ops
    B, S, Rs, orientations = LEGS[leg]
    n_orient, T = ops.ALIGN_SET_SIZES[orientations], 2 * Rs + 1
    moving, fixed, moves = pairs(B, n_orient)
    a, b = torch.as_tensor(moving).cuda(), torch.as_tensor(fixed).cuda()
    bits_a, bits_b = ops.voxel_pack(a)[0], ops.voxel_pack(b)[0]
    lib, sp = L.lib(), L.stream_ptr()
    ws, nws = ops._workspace(lib.rn_voxel_align_workspace_bytes, a.device, B, S, Rs, n_orient)
    best = torch.empty((B, 8), dtype=torch.int32, device="cuda")
    copies = torch.empty((B, n_orient, S ** 3 // 32), dtype=torch.int32, device="cuda")

    def launch():
        L.check(lib.rn_voxel_align(ops._vp(bits_a), ops._vp(bits_b), B, S, Rs, ops.ALIGN_SETS[orientations], ops._vp(best), None,
                                   ops._vp(ws), nws, sp))

    def orient():
        L.check(lib.rn_voxel_orient(ops._vp(bits_a), B, S, 0, n_orient, ops._vp(copies), sp))
    row = {"leg": leg, "B": B, "S": S, "R": Rs, "orientations": orientations, "n_orient": n_orient, "calls": calls, "rounds": rounds,
           "candidates_per_pair": n_orient * T ** 3, "workspace_mb": nws / 1e6}
    if launch_only:
        row["launch_us"] = _events(launch, calls)
        return row
    found = ops.voxel_align(a, b, max_shift=Rs, orientations=orientations, return_scores=True)
    survivors = torch.as_tensor(moving).flatten(1).sum(1).int().cuda()
    row["pairs_recovered"] = int((found.n_and == survivors).sum())                # every voxel still inside the grid is matched
    t0 = time.time()
    twin = R.scores(moving[0].astype(bool), fixed[0].astype(bool), Rs, 1)
    row["twin_pair_orientation_s"] = time.time() - t0
    row["twin_equal"] = bool(np.array_equal(found.scores[0, :1].cpu().numpy(), twin))
    ab, bb = a[0] > 0, b[0] > 0
    row["torch_equal"] = bool(torch.equal(torch_table(ab, bb, Rs), found.scores[0, 0]))
    t = {"align_us": [], "launch_us": [], "orient_us": [], "torch_pair_orientation_us": []}
    for _ in range(rounds):
        t["align_us"].append(_events(lambda: ops.voxel_align(a, b, max_shift=Rs, orientations=orientations), calls))
        t["launch_us"].append(_events(launch, calls))
        t["orient_us"].append(_events(orient, calls))
        t["torch_pair_orientation_us"].append(_events(lambda: torch_table(ab, bb, Rs), max(calls // 4, 2)))
    row["rounds_us"] = t
    for k, v in t.items():
        row[k] = float(np.median(v))
    words = B * n_orient * T ** 3 * (S ** 3 // 32)
    row["word_popcounts_per_s"] = words / (row["launch_us"] * 1e-6)
    row["speedup_over_torch"] = B * n_orient * row["torch_pair_orientation_us"] / row["launch_us"]
    row["speedup_over_twin"] = B * n_orient * row["twin_pair_orientation_s"] * 1e6 / row["launch_us"]
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
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_align_bench.json"))
    ap.add_argument("--stats", default=os.path.join(ROOT, "profiles", "voxel_align_kernel_stats.csv"))
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--leg", choices=sorted(LEGS), default=None, help="the bare launch of one leg only (what the profiled child runs)")
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("voxel_align_bench.py measures on the GPU; no HIP device found")
    if a.leg:
        print(json.dumps(time_leg(a.leg, a.calls, 1, launch_only=True)), flush=True)
        return
    rows = [time_leg(leg, a.calls, a.rounds) for leg in LEGS]
    stats = []
    if not a.no_profile:
        if shutil.which("rocprofv3") is None:
            raise SystemExit("rocprofv3 not found; --no-profile times the calls only")
        with tempfile.TemporaryDirectory() as tmp:
            for row in rows:
                raw = profile_leg(row["leg"], a.calls, tmp)
                for kernel in ("correlate_kernel", "orient_kernel", "winner_kernel"):
                    mine = [r for r in raw if kernel in r["Name"]]
                    if not mine:
                        raise SystemExit("%s: no %s in the kernel table" % (row["leg"], kernel))
                    row[kernel + "_avg_us"] = float(mine[0]["AverageNs"]) / 1e3
                stats += [dict(r, Leg=row["leg"]) for r in raw]
    result = {"voxel_align": {"rows": rows}}
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
