#!/usr/bin/env python
"""What the mesh voxeliser costs: `ops.voxelize_mesh` on the device and the host work in front of it (load_mesh, fit, prepare).

    python scripts/mesh_voxel_bench.py [--calls 20] [--thresholds 64,16,64,16,64,256,64,256]
        GPU.  Meshes: an icosphere of 6 subdivisions (81 920 sub-voxel triangles at these sizes) and the 12-triangle cube that
        fills the grid, each at S = 64 and 128, mode "both".  Each mesh is written as an OBJ once, then
          host    load_mesh, fit and prepare of that file, by the host clock (best of 3)
          device  one leg per entry of --thresholds, in that order (a b a b: the same visit): `calls` ops.voxelize_mesh calls on
                  the prepared dict between device events -- the upload of vertices, triangles and lists included -- with the
                  small / large split of `prepare(..., threshold=T)`
        Run it under `rocprofv3 --kernel-trace --stats -- python scripts/mesh_voxel_bench.py --calls 5 --thresholds 64` for the
        per-kernel rows.

Prints ONE JSON line.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)


def icosphere(n):
    """Unit icosphere after n midpoint subdivisions: (verts float64 [V,3], tris int32 [20 * 4^n, 3])."""
    g = (1 + 5 ** 0.5) / 2
    v = np.array([(-1, g, 0), (1, g, 0), (-1, -g, 0), (1, -g, 0), (0, -1, g), (0, 1, g), (0, -1, -g), (0, 1, -g),
                  (g, 0, -1), (g, 0, 1), (-g, 0, -1), (-g, 0, 1)], np.float64)
    t = np.array([(0, 11, 5), (0, 5, 1), (0, 1, 7), (0, 7, 10), (0, 10, 11), (1, 5, 9), (5, 11, 4), (11, 10, 2), (10, 7, 6),
                  (7, 1, 8), (3, 9, 4), (3, 4, 2), (3, 2, 6), (3, 6, 8), (3, 8, 9), (4, 9, 5), (2, 4, 11), (6, 2, 10), (8, 6, 7),
                  (9, 8, 1)], np.int64)
    v /= np.linalg.norm(v[0])
    for _ in range(n):
        edges = np.sort(np.concatenate([t[:, [0, 1]], t[:, [1, 2]], t[:, [2, 0]]]), 1)
        uniq, inv = np.unique(edges, axis=0, return_inverse=True)
        mid = v[uniq[:, 0]] + v[uniq[:, 1]]
        mid /= np.linalg.norm(mid, axis=1, keepdims=True)
        m = len(v) + inv.reshape(3, -1)                                         # midpoint of edge ab, bc, ca per triangle
        v = np.concatenate([v, mid])
        a, b, c = t.T
        t = np.concatenate([np.stack([a, m[0], m[2]], 1), np.stack([m[0], b, m[1]], 1), np.stack([m[2], m[1], c], 1),
                            np.stack([m[0], m[1], m[2]], 1)])
    return v, t.astype(np.int32)


def cube():
    v = np.array([[x, y, z] for x in (0, 1) for y in (0, 1) for z in (0, 1)], np.float64)
    quads = [(0, 1, 3, 2), (4, 6, 7, 5), (0, 4, 5, 1), (2, 3, 7, 6), (0, 2, 6, 4), (1, 5, 7, 3)]
    return v, np.array([t for a, b, c, d in quads for t in ((a, b, c), (a, c, d))], np.int32)


def write_obj(path, v, t):
    with open(path, "w") as f:
        f.write("".join("v %.9g %.9g %.9g\n" % tuple(p) for p in v))
        f.write("".join("f %d %d %d\n" % tuple(i) for i in t + 1))


def best_of(fn, n=3):
    best, out = None, None
    for _ in range(n):
        t0 = time.perf_counter()
        out = fn()
        dt = time.perf_counter() - t0
        best = dt if best is None else min(best, dt)
    return best * 1e3, out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--thresholds", type=str, default="64,16,64,16,64,256,64,256")
    a = ap.parse_args(argv)
    import torch
    from rendernet_amd import mesh, ops
    if not torch.cuda.is_available():
        raise SystemExit("mesh_voxel_bench.py measures on the GPU; no HIP device found")
    thresholds = [int(x) for x in a.thresholds.split(",")]
    rows = []
    with tempfile.TemporaryDirectory() as tmp:
        for name, (v, t) in (("icosphere6", icosphere(6)), ("cube", cube())):
            path = os.path.join(tmp, name + ".obj")
            write_obj(path, v, t)
            for S in (64, 128):
                load_ms, (verts, tris) = best_of(lambda: mesh.load_mesh(path))
                fit_ms, q = best_of(lambda: mesh.fit(verts, S))
                prep_ms, _ = best_of(lambda: mesh.prepare(q, tris, S))
                row = {"mesh": name, "S": S, "triangles": int(len(tris)), "host_ms": {"load": load_ms, "fit": fit_ms, "prepare": prep_ms},
                       "legs": []}
                for T in thresholds:
                    d = mesh.prepare(q, tris, S, threshold=T)
                    for _ in range(3):
                        vox = ops.voxelize_mesh(d, S=S)
                    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
                    e0.record()
                    for _ in range(a.calls):
                        vox = ops.voxelize_mesh(d, S=S)
                    e1.record()
                    torch.cuda.synchronize()
                    row["legs"].append({"threshold": T, "us_per_call_events": e0.elapsed_time(e1) * 1e3 / a.calls,
                                        "lists": [int(len(d[k])) for k in ops.MESH_LISTS]})
                row["voxels_set"] = int(vox.sum().item())
                rows.append(row)
    print(json.dumps({"mesh_voxel": {"calls": a.calls, "mode": "both", "rows": rows}}), flush=True)


if __name__ == "__main__":
    main()
