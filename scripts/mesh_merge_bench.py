#!/usr/bin/env python
"""What merging the blocky mesh costs, and what drawing a merged mesh loses.

    python scripts/mesh_merge_bench.py [--calls 50] [--out profiles/mesh_merge_bench.json]
        GPU.  Inputs: the chair at 64^3 (uint8, B = 1), B = 24 procedural CSG grids at 64^3 (uint8) and one grid at 128^3 (the
        chair doubled, uint8).  Per input, in the same run, `calls` calls between device events after 5 warm-up calls of
          merged   ops.extract_mesh_merged: pack, count, marks, scan, the read-back of the totals, the allocations, vertices, quads
          blocky   ops.extract_mesh(smooth=False), the yardstick: the same surface as unit quads
        with the vertices and faces of both.
    python scripts/mesh_merge_bench.py --tjunctions
        CPU, the NumPy twins of tests/ only.  The chair at 32^3 (a 2^3 max-pool of the 64^3 grid) drawn flat-shaded by the
        rasteriser's twin under three poses of synth.scan_poses, 64 cells of 2 pixels, once as the blocky mesh and once merged:
        the pixels whose hit mask or normal bytes differ, as a share of the pixels either mesh covers.  A merged mesh has
        T-junctions and the rasteriser keeps every pixel on shared edges only; this is the size of that effect.

Writes the JSON result (the --tjunctions figures are kept when the file already has them) and prints it as ONE JSON line.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
LEGS = ("chair64", "csg64x24", "chair128")


def chair():
    from rendernet_amd.tools import binvox_rw
    with open(os.path.join(ROOT, "binvox", "chair.binvox"), "rb") as f:
        return np.ascontiguousarray(binvox_rw.read_as_3d_array(f).data).astype(np.uint8)


def make(leg):
    """The voxels of a leg on the device: uint8 [B,S,S,S]."""
    import torch
    from rendernet_amd import ops, synth
    if leg == "chair64":
        return torch.as_tensor(chair()[None]).cuda()
    if leg == "chair128":
        return torch.as_tensor(np.ascontiguousarray(chair().repeat(2, 0).repeat(2, 1).repeat(2, 2))[None]).cuda()
    prims = torch.as_tensor(synth.shape_prims(1234, list(range(0x1000, 0x1000 + 24)), 64)).cuda()
    return ops.voxel_shapes(prims, 64)[..., 0].contiguous()


def time_leg(leg, calls):
    import torch
    from rendernet_amd import ops
    vol = make(leg)
    row = {"leg": leg, "B": int(vol.shape[0]), "S": int(vol.shape[1]), "dtype": str(vol.dtype).split(".")[-1], "calls": calls}
    for name, run in (("merged", lambda: ops.extract_mesh_merged(vol)), ("blocky", lambda: ops.extract_mesh(vol, smooth=False))):
        for _ in range(5):
            m = run()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(calls):
            m = run()
        e1.record()
        torch.cuda.synchronize()
        row[name] = {"vertices": int(m.q.shape[0]), "quads": int(m.faces.shape[0]), "us_per_call_events": e0.elapsed_time(e1) * 1e3 / calls}
    row["merged_over_blocky"] = row["merged"]["us_per_call_events"] / row["blocky"]["us_per_call_events"]
    return row


def tjunctions():
    """The blocky and the merged chair at 32^3 under the rasteriser's twin: differing pixels per pose and overall."""
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import mesh_extract_ref as E
    import mesh_merge_ref as M
    import mesh_raster_ref as MR
    from oracle import resample as OR
    from rendernet_amd import synth
    S, N, f = 32, 64, 2
    vol = chair().reshape(32, 2, 32, 2, 32, 2).max(axis=(1, 3, 5))
    bq, bf = E.extract(vol, 0.5, smooth=False)
    mq, mf = M.merge(vol)[:2]
    poses, low = synth.scan_poses(3)
    low = np.broadcast_to(np.asarray(low, bool), (3,))
    rows = []
    for pose, lx in zip(np.asarray(poses, np.float32), low.tolist()):
        m_inv = OR.inverse_affine(pose[None], size=S, new_size=N)[0].astype(np.float32)
        cam = MR.camera(m_inv, N, f, lx)
        pictures = [MR.rasterize(q, E.fan(faces), cam, m_inv, S, N, f, smooth=False, view_from_low_x=lx)[:2] for q, faces in ((bq, bf), (mq, mf))]
        (rgb_b, id_b), (rgb_m, id_m) = pictures
        hit_b, hit_m = id_b >= 0, id_m >= 0
        differ = (hit_b != hit_m) | (rgb_b != rgb_m).any(-1)
        rows.append({"pose": [float(v) for v in pose], "view_from_low_x": bool(lx), "pixels": int(differ.size), "covered": int((hit_b | hit_m).sum()),
                     "mask_differs": int((hit_b != hit_m).sum()), "differ": int(differ.sum())})
    covered, differ = sum(r["covered"] for r in rows), sum(r["differ"] for r in rows)
    return {"grid": "chair, 32^3", "new_size": N, "pixels_per_cell": f, "shading": "flat", "blocky_quads": int(len(bf)), "merged_quads": int(len(mf)),
            "poses": rows, "covered": covered, "differ": differ, "share_of_covered": differ / max(covered, 1)}


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=50)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_merge_bench.json"))
    ap.add_argument("--tjunctions", action="store_true", help="the CPU measurement only")
    a = ap.parse_args(argv)
    result = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            result = json.load(f).get("mesh_merge", {})
    if a.tjunctions:
        result["tjunctions"] = tjunctions()
    else:
        import torch
        if not torch.cuda.is_available():
            raise SystemExit("mesh_merge_bench.py times on the GPU; no HIP device found (--tjunctions is the CPU measurement)")
        result["rows"] = [time_leg(leg, a.calls) for leg in LEGS]
    result = {"mesh_merge": result}
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
