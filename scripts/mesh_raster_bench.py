#!/usr/bin/env python
"""What the mesh rasteriser costs beside the voxel ray caster it stands in for: `ops.rasterize_mesh` against
`ops.raycast_normals` on the same objects, at the training feed's shape (B = 24, 64^3 grids, 128^3 camera, 512 x 512 frames).

    python scripts/mesh_raster_bench.py [--calls 20] [--legs 4] [--out profiles/mesh_raster_bench.json]
        GPU.  Two object sets:
          models      the smooth surface nets of the five shipped binvox models (ops.extract_mesh), one mesh set of five, the 24
                      items cycling through them; the caster's leg draws the five grids themselves
          icosphere6  one mesh of 81 920 triangles fitted to the 64^3 grid; the caster's leg draws its voxelisation
        24 seeded poses from the synthetic feed's ranges.  Per set `legs` alternating pairs (raster, cast, raster, cast: the
        same visit), each leg `calls` calls between device events after 3 warm-up calls.  The rasteriser's leg is what the feed
        pays per batch: the vertex normals come from the set (computed once, outside the leg).  Also timed once per set: that
        `ops.mesh_vertex_normals` call.

Prints ONE JSON line and writes it to --out.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

from scripts.mesh_voxel_bench import icosphere  # noqa: E402


def timed(fn, calls):
    import torch
    for _ in range(3):
        fn()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(calls):
        out = fn()
    e1.record()
    torch.cuda.synchronize()
    return e0.elapsed_time(e1) * 1e3 / calls, out


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--legs", type=int, default=4)
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "mesh_raster_bench.json"))
    a = ap.parse_args(argv)
    import torch
    from rendernet_amd import mesh, ops, synth
    if not torch.cuda.is_available():
        raise SystemExit("mesh_raster_bench.py measures on the GPU; no HIP device found")
    B, S, N, f = a.batch, 64, 128, 4
    rng = np.random.default_rng(1234)
    az, el, rad = rng.uniform(0.0, 360.0, B), rng.uniform(10.0, 170.0, B), rng.uniform(2.5, 4.5, B)
    pose = torch.as_tensor(np.stack([az * np.pi / 180.0, el * np.pi / 180.0, 3.3 / rad], 1).astype(np.float32)).cuda()

    models, names = synth.read_models(os.path.join(ROOT, "binvox"))
    grids = torch.as_tensor(models).cuda()
    nets = ops.extract_mesh(grids, smooth=True, triangles=True)
    vo, fo = nets.vert_offsets.tolist(), nets.face_offsets.tolist()
    q, tris = nets.q.cpu().numpy(), nets.faces.cpu().numpy()
    model_set = mesh.MeshSet([(q[vo[m]:vo[m + 1]], tris[fo[m]:fo[m + 1]]) for m in range(len(names))], names, S)
    v, t = icosphere(6)
    ico_q = mesh.fit(v, S)
    ico_set = mesh.MeshSet([(ico_q, t)], ["icosphere6"], S)
    ico_grid = ops.voxelize_mesh(mesh.prepare(ico_q, t, S), S=S)

    rows = []
    for name, ms, ids, vox in (("models", model_set, [b % len(names) for b in range(B)], None), ("icosphere6", ico_set, [0] * B, ico_grid)):
        ids_t = torch.as_tensor(np.asarray(ids, np.int32)).cuda()
        vox = grids[ids_t.long()] if vox is None else vox.expand(B, -1, -1, -1, -1).contiguous()
        normals_us, _ = timed(lambda: ops.mesh_vertex_normals(ms.q, ms.tris, S, ms.vert_offsets, ms.tri_offsets), a.calls)
        legs = []
        for _ in range(a.legs):
            r_us, frames = timed(lambda: ms.rasterize(ids_t, pose, new_size=N, pixels_per_cell=f), a.calls)
            c_us, cast = timed(lambda: ops.raycast_normals(vox, pose, new_size=N, pixels_per_cell=f), a.calls)
            legs.append({"raster_us_per_call_events": r_us, "raycast_us_per_call_events": c_us})
        to = ms.tri_offsets.tolist()
        rows.append({"set": name, "meshes": len(ms), "triangles_per_item": [int(to[m + 1] - to[m]) for m in sorted(set(ids))],
                     "vertex_normals_us_per_call_events": normals_us, "legs": legs,
                     "raster_hit_share": float(frames.any(-1).float().mean().item()),
                     "raycast_hit_share": float(cast.any(-1).float().mean().item())})
    result = {"mesh_raster": {"calls": a.calls, "B": B, "S": S, "new_size": N, "pixels_per_cell": f, "rows": rows}}
    line = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
