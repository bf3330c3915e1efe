#!/usr/bin/env python
"""How close the silhouette pose search lands, measured on the NumPy twin (tests/voxel_pose_ref.py), where it can be checked
without a device; the device computes the same tables word for word (tests/test_gpu_voxel_pose.py).

    python scripts/voxel_pose_accuracy.py [--poses 8] [--out profiles/voxel_pose_accuracy.json]

Per model (chair, bunny, suzanne OR-pooled to 32^3, N = 64, f = 1, footprint 2): `poses` seeded off-lattice poses -- azimuth
uniform in [0, 2 pi), elevation in [0.15, 1.25], scale in [0.85, 1.2] -- each scanned by the caster's twin into a mask and
searched over the default lattice (24 azimuths x synth.POSE_ELEVATIONS x synth.POSE_SCALES) with refine = 0, 1, 2.  Reports the
error in azimuth (wrapped), elevation and scale, worst and median per model and refinement, next to the lattice's steps.
Prints ONE JSON line and writes it to --out.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
MODELS = ("chair", "bunny", "suzanne")
LATTICE = (24, (0.1, 0.4, 0.7, 1.0, 1.3), (0.8, 1.0, 1.25))
N, F, FP, REFINE, SEED = 64, 1, 2, 2, 31


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--poses", type=int, default=8)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "voxel_pose_accuracy.json"))
    a = ap.parse_args(argv)
    import voxel_carve_ref as VC
    import voxel_pose_ref as R
    window = (0, 0, F * N, F * N)
    rng = np.random.default_rng(SEED)
    true = np.stack([rng.uniform(0.0, 2.0 * np.pi, a.poses), rng.uniform(0.15, 1.25, a.poses), rng.uniform(0.85, 1.2, a.poses)], 1)
    true = true.astype(np.float32)
    lattice = R.pose_lattice(*LATTICE)
    rows = []
    for name in MODELS:
        occ = R.pool(R.load_binvox(name))
        cams, _ = VC.cameras(lattice, [False] * len(lattice), occ.shape[0], N, F)
        level0 = (cams, R.splats(occ, cams, window, FP))
        views, _ = VC.scan(occ, true, [False] * len(true), N, F)
        err = np.zeros((len(true), REFINE + 1, 3))
        iou = np.zeros((len(true), REFINE + 1))
        for k in range(len(true)):
            mask = views[k] >= 0
            levels = R.search(occ, mask, *LATTICE, refine=REFINE, N=N, f=F, window=window, fp=FP, level0=level0)
            for level, (lat, w, pose) in enumerate(levels):
                d = np.asarray(pose, np.float64) - true[k]
                d[0] = (d[0] + np.pi) % (2.0 * np.pi) - np.pi
                err[k, level] = np.abs(d)
                cam_w, _ = VC.cameras(pose[None], [False], occ.shape[0], N, F)
                table, n_mask = R.scores(occ, cam_w, mask, window, FP)
                iou[k, level] = R.iou(table[0][0], table[0][1], n_mask)
        for level in range(REFINE + 1):
            rows.append({"model": name, "refine": level, "poses": len(true),
                         "worst": [float(v) for v in err[:, level].max(0)], "median": [float(v) for v in np.median(err[:, level], 0)],
                         "lowest_iou": float(iou[:, level].min()), "median_iou": float(np.median(iou[:, level]))})
    result = {"voxel_pose_accuracy": {"lattice": [LATTICE[0], list(LATTICE[1]), list(LATTICE[2])],
                                      "steps": [float(v) for v in R.lattice_steps(*LATTICE)], "seed": SEED, "footprint": FP,
                                      "axes": ["azimuth", "elevation", "scale"], "rows": rows}}
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
