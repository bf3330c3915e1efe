#!/usr/bin/env python
"""What the silhouette pose search costs: `ops.voxel_pose_scores` on the device, against the plain route and the NumPy twin.

    python scripts/voxel_pose_bench.py [--calls 5] [--rounds 3] [--plain-candidates 48] [--out profiles/voxel_pose_bench.json]
                                       [--stats profiles/voxel_pose_kernel_stats.csv] [--no-profile]
        GPU.  The workload: B = 24 grids of 64^3, the five shipped models cycled, N = 128, f = 1 (a 128 x 128 frame); the lattice
        synth.pose_lattice(72, 18 elevations 0.05 .. 1.5, scales (0.8, 1.0, 1.25)) = 3 888 candidates shared by all items, so
        93 312 (item, candidate) pairs a call; the mask of item b is `voxel_scan(...) >= 0` at lattice pose 161 b + 7; the
        footprint is the automatic one (2).  `rounds` times in alternation
          scores   `calls` calls of ops.voxel_pose_scores (the pack, the mask pack, the cameras, the scores, the winner) between
                   device events after 2 warm-up calls
          launch   the same for the bare rn_pose_score entry on packed grids, packed masks and ready cameras, WITH the workspace:
                   the list of each item's occupied words, then the scores over the list (what ops.voxel_pose_scores calls)
          walk     the same entry WITHOUT the workspace: every workgroup walks all S^3 / 32 words and skips the zero ones
          plain    the plain route on the first `plain-candidates` candidates: one ops.voxel_scan per candidate (B casts and their
                   entry depths) and the IoU against the masks in torch; `plain_pair_us` per (item, candidate), scaled up to the
                   whole lattice as `plain_scaled_s`
        and the median of each over the rounds.  `pairs_per_s` = B P over the launch time, `speedup_over_plain` = the scaled plain
        time over the scores time.  `recovered` counts the items whose winner is the pose their mask was scanned at.
          twin     tests/voxel_pose_ref.py on the host, 8 candidates of one item, once: `twin_pair_s`, and `twin_equal`
          kernels  one `rocprofv3 --kernel-trace --stats` run of its own (a fresh child process: this script with --launch-only),
                   its kernel table read back: pose_score_kernel, pose_best_kernel and mask_pack_kernel.  No counters.
        `occupied_words` is the share of row words that hold a voxel: what the list keeps and the walk does not skip.

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
B, S, N, F = 24, 64, 128, 1
LATTICE = (72, tuple(float(v) for v in np.linspace(0.05, 1.5, 18)), (0.8, 1.0, 1.25))
KERNELS = ("pose_score_kernel", "pose_words_kernel", "pose_best_kernel", "mask_pack_kernel")


def _events(fn, calls, warm=2):
    import torch
    for _ in range(warm):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls


def workload():
    """(vox uint8 [B,S,S,S,1], lattice float32 [P,3], masks uint8 [B,N,N], the true index of every item) on the device."""
    import torch
    import voxel_pose_ref as R
    from rendernet_amd import ops, synth
    grids = np.stack([R.load_binvox(MODELS[b % len(MODELS)]) for b in range(B)]).astype(np.uint8)
    vox = torch.as_tensor(grids[..., None]).cuda()
    lattice = synth.pose_lattice(*LATTICE)
    truth = [(161 * b + 7) % len(lattice) for b in range(B)]
    poses = torch.as_tensor(lattice).cuda()
    views = ops.voxel_scan(vox, poses[truth][:, None].contiguous(), new_size=N, pixels_per_cell=F)
    return vox, poses, (views[:, 0] >= 0).to(torch.uint8), truth, grids


def measure(calls, rounds, plain_candidates, launch_only=False):
    import torch
    import voxel_pose_ref as R
    from rendernet_amd import _lib as L, ops
    vox, poses, masks, truth, grids = workload()
    P = int(poses.shape[0])
    kw = dict(new_size=N, pixels_per_cell=F)
    found = ops.voxel_pose_scores(masks, vox, poses, **kw)
    fp = found.footprint
    bits = ops.voxel_pack(vox)[0]
    mask_bits, n_mask = ops._pose_masks("bench", masks, B, N, N, vox.device)
    scores = torch.empty((B, P, 2), dtype=torch.int32, device="cuda")
    lib, sp = L.lib(), L.stream_ptr()

    ws, nws = ops._workspace(lib.rn_pose_score_workspace_bytes, vox.device, B, S)

    def launch():                                                  # the list of occupied words, then the scores
        L.check(lib.rn_pose_score(ops._vp(bits), ops._vp(mask_bits), ops._vp(found.cam), ops._vp(scores), None, B, P, S, N, F, 0, 0, N, N,
                                  fp, ops._vp(ws), nws, sp))

    def walk():                                                    # no workspace: every workgroup walks every word
        L.check(lib.rn_pose_score(ops._vp(bits), ops._vp(mask_bits), ops._vp(found.cam), ops._vp(scores), None, B, P, S, N, F, 0, 0, N, N,
                                  fp, None, 0, sp))
    row = {"B": B, "S": S, "N": N, "pixels_per_cell": F, "P": P, "pairs": B * P, "footprint": fp, "calls": calls, "rounds": rounds,
           "occupied_words": float((bits != 0).double().mean()), "voxels_per_item": float(grids.reshape(B, -1).sum(1).mean())}
    if launch_only:
        row["launch_us"], row["walk_us"] = _events(launch, calls), _events(walk, calls)
        return row
    walk()
    row["walk_equal"] = bool(torch.equal(scores, found.scores))
    scores.zero_()
    launch()
    row["launch_equal"] = bool(torch.equal(scores, found.scores))
    row["recovered"] = int(sum(int(w) == t for w, t in zip(found.best.tolist(), truth)))
    t0 = time.time()
    twin, _ = R.scores(grids[0].astype(bool), found.cam[0, :8].cpu().numpy(), masks[0].cpu().numpy(), (0, 0, N, N), fp)
    row["twin_pair_s"] = (time.time() - t0) / 8
    row["twin_equal"] = bool(np.array_equal(found.scores[0, :8].cpu().numpy(), twin))
    fg = masks.bool()

    def plain():
        out = torch.empty((B, plain_candidates), dtype=torch.float64, device="cuda")
        for p in range(plain_candidates):
            sil = ops.voxel_scan(vox, poses[p].expand(B, 1, 3).contiguous(), **kw)[:, 0] >= 0
            out[:, p] = (sil & fg).flatten(1).sum(1).double() / (sil | fg).flatten(1).sum(1).clamp(min=1).double()
        return out
    t = {"scores_us": [], "launch_us": [], "walk_us": [], "plain_us": []}
    for _ in range(rounds):
        t["scores_us"].append(_events(lambda: ops.voxel_pose_scores(masks, vox, poses, **kw), calls))
        t["launch_us"].append(_events(launch, calls))
        t["walk_us"].append(_events(walk, calls))
        t["plain_us"].append(_events(plain, max(calls // 2, 1), warm=1))
    row["rounds_us"] = t
    for k, v in t.items():
        row[k] = float(np.median(v))
    row["plain_candidates"] = plain_candidates
    row["plain_pair_us"] = row["plain_us"] / (B * plain_candidates)
    row["plain_scaled_s"] = row["plain_pair_us"] * B * P * 1e-6
    row["pairs_per_s"] = B * P / (row["launch_us"] * 1e-6)
    row["pairs_per_s_end_to_end"] = B * P / (row["scores_us"] * 1e-6)
    row["speedup_over_plain"] = row["plain_scaled_s"] / (row["scores_us"] * 1e-6)
    row["speedup_over_twin"] = B * P * row["twin_pair_s"] * 1e6 / row["scores_us"]
    return row


def profile(calls, tmp):
    cmd = ["rocprofv3", "--kernel-trace", "--stats", "--output-format", "csv", "-d", tmp, "-o", "p", "--",
           sys.executable, os.path.abspath(__file__), "--launch-only", "--calls", str(calls)]
    r = subprocess.run(cmd, cwd=ROOT, capture_output=True, text=True, timeout=600)
    if r.returncode != 0:
        raise SystemExit("rocprofv3 failed:\n%s" % r.stderr[-2000:])
    found = glob.glob(os.path.join(tmp, "**", "*kernel_stats.csv"), recursive=True)
    if not found:
        raise SystemExit("rocprofv3 left no kernel_stats.csv")
    with open(found[0]) as f:
        return [r_ for r_ in csv.DictReader(f) if any(k in r_["Name"] for k in KERNELS)]


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=5)
    ap.add_argument("--rounds", type=int, default=3)
    ap.add_argument("--plain-candidates", type=int, default=48)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_pose_bench.json"))
    ap.add_argument("--stats", default=os.path.join(ROOT, "profiles", "voxel_pose_kernel_stats.csv"))
    ap.add_argument("--no-profile", action="store_true")
    ap.add_argument("--launch-only", action="store_true", help="the bare launch only (what the profiled child runs)")
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("voxel_pose_bench.py measures on the GPU; no HIP device found")
    if a.launch_only:
        print(json.dumps(measure(a.calls, 1, a.plain_candidates, launch_only=True)), flush=True)
        return
    row = measure(a.calls, a.rounds, a.plain_candidates)
    stats = []
    if not a.no_profile:
        if shutil.which("rocprofv3") is None:
            raise SystemExit("rocprofv3 not found; --no-profile times the calls only")
        with tempfile.TemporaryDirectory() as tmp:
            stats = profile(a.calls, tmp)
        for r in stats:                                            # the two forms of pose_score_kernel are two rows
            form = "_walk" if "<false>" in r["Name"] or "ILb0E" in r["Name"] else ""
            kernel = [k for k in KERNELS if k in r["Name"]][0]
            row[kernel + form + "_avg_us"] = float(r["AverageNs"]) / 1e3
    result = {"voxel_pose": row}
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    if stats:
        with open(a.stats, "w", newline="") as f:
            w = csv.DictWriter(f, fieldnames=list(stats[0]), quoting=csv.QUOTE_NONNUMERIC)
            w.writeheader()
            w.writerows(stats)
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
