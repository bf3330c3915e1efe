#!/usr/bin/env python
"""What a colour picture of a mesh costs on top of its normal map: `ops.rasterize_mesh_colour` against `ops.rasterize_mesh` alone
on the same objects, at the training feed's shape (B = 24, 64^3 grids, 128^3 camera, 512 x 512 frames), the colour resolve
against the same resolve composed from torch ops, and `ops.mesh_face_voxels` for 24 grids.

    python scripts/mesh_colour_bench.py [--calls 20] [--legs 4] [--out profiles/mesh_colour_bench.json]
        GPU.  The smooth surface nets of the five shipped binvox models (ops.extract_mesh), one mesh set of five, the 24 items
        cycling through them, 24 seeded poses from the synthetic feed's ranges, seeded random colours.  `legs` alternating rounds
        (normal map alone, colour per vertex, colour per face, the two resolves alone, the two torch compositions: the same
        visit), each leg `calls` calls between device events after 3 warm-up calls.
          raster              ops.rasterize_mesh(smooth=False, return_ids=True): what exists without the colour (the baseline)
          colour_vertex/face  ops.rasterize_mesh_colour: the same pass, then rn_mesh_colour_from_ids
          resolve_vertex/face ops.mesh_colour_from_ids on the ids of that pass (rn_mesh_camera + rn_mesh_colour_from_ids)
          torch_vertex/face   the same pictures from torch ops on the returned ids: a gather of face colours; for vertex colours
                              every vertex projected under every camera (int64, ops.mesh_camera's rows), a gather per
                              pixel, the three edge functions and the rounded integer mean -- both are checked equal to the
                              kernel's bytes before anything is timed
        and `ops.mesh_face_voxels` over the quad nets of 24 grids at 64^3 (the five models cycled), once per leg.

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


def torch_face(ids, tri_offsets, mesh_of_item, fcol):
    """colour_from_ids with face colours as torch ops: ids [B,ph,pw] of meshes that all have vertices."""
    import torch
    t0 = tri_offsets[mesh_of_item.long()][:, None, None]
    count = (tri_offsets[1:] - tri_offsets[:-1])[mesh_of_item.long()][:, None, None]
    ok = (ids >= 0) & (ids < count)
    return torch.where(ok[..., None], fcol[(t0 + ids.clamp(min=0)).clamp(max=fcol.shape[0] - 1)], torch.zeros_like(fcol[:1]))


def torch_vertex(ids, q, tris, vert_offsets, tri_offsets, mesh_of_item, cam, vcol, S):
    """colour_from_ids with vertex colours as torch ops, int64 throughout (the rule of include/rendernet_hip.h; the meshes are
    surface nets: no triangle without area, every index in range, the whole frame)."""
    import torch
    B, ph, pw = ids.shape
    m = mesh_of_item.long()
    ok = ids >= 0
    tg = (tri_offsets[m][:, None, None] + ids.clamp(min=0)).reshape(B, -1)                       # [B,P] global triangle
    vid = tris.long()[tg] + vert_offsets[m][:, None, None]                                       # [B,P,3] global vertices
    PV = (q.long().clamp(0, 256 * S)[None, :, None, :] * cam[:, None, :2, :3]).sum(-1) + cam[:, None, :2, 3]   # [B,V,(X,Y)]
    PV = ((PV + (1 << 19)) >> 20).clamp(-(1 << 20), 1 << 20)                                     # every vertex under every camera
    P = PV[torch.arange(B, device=ids.device)[:, None, None], vid]                               # [B,P,3,(X,Y)]
    X, Y = P[..., 0], P[..., 1]
    A = (X[..., 1] - X[..., 0]) * (Y[..., 2] - Y[..., 0]) - (Y[..., 1] - Y[..., 0]) * (X[..., 2] - X[..., 0])
    flip = A < 0                                                                                 # wound to A > 0: swap vertices 1, 2
    order = torch.where(flip[..., None], torch.tensor([0, 2, 1], device=ids.device), torch.tensor([0, 1, 2], device=ids.device))
    X, Y, vid = torch.gather(X, 2, order), torch.gather(Y, 2, order), torch.gather(vid, 2, order)
    r = torch.arange(ph, device=ids.device).repeat_interleave(pw)
    c = torch.arange(pw, device=ids.device).repeat(ph)
    cu, cv = (256 * c + 128)[None], (256 * r + 128)[None]
    E = []
    for k in range(3):
        n = (k + 1) % 3
        E.append((X[..., n] - X[..., k]) * (cv - Y[..., k]) - (Y[..., n] - Y[..., k]) * (cu - X[..., k]))
    w = torch.stack([E[1], E[2], E[0]], -1)                                                      # position k carries E_(k+1)
    num = (w[..., None] * vcol.long()[vid]).sum(2)                                               # [B,P,3 channels]
    Aa = A.abs().clamp(min=1)[..., None]
    byte = torch.div(2 * num + Aa, 2 * Aa, rounding_mode="floor").clamp(0, 255).to(torch.uint8)
    return torch.where(ok.reshape(B, -1, 1), byte, torch.zeros_like(byte)).reshape(B, ph, pw, 3)


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=20)
    ap.add_argument("--legs", type=int, default=4)
    ap.add_argument("--batch", type=int, default=24)
    ap.add_argument("--out", type=str, default=os.path.join(ROOT, "profiles", "mesh_colour_bench.json"))
    a = ap.parse_args(argv)
    import torch
    from rendernet_amd import ops, synth
    if not torch.cuda.is_available():
        raise SystemExit("mesh_colour_bench.py measures on the GPU; no HIP device found")
    B, S, N, f = a.batch, 64, 128, 4
    rng = np.random.default_rng(1234)
    az, el, rad = rng.uniform(0.0, 360.0, B), rng.uniform(10.0, 170.0, B), rng.uniform(2.5, 4.5, B)
    pose = torch.as_tensor(np.stack([az * np.pi / 180.0, el * np.pi / 180.0, 3.3 / rad], 1).astype(np.float32)).cuda()

    models, names = synth.read_models(os.path.join(ROOT, "binvox"))
    grids = torch.as_tensor(models).cuda()
    nets = ops.extract_mesh(grids, smooth=True, triangles=True)
    q, tris, vo, to = nets.q, nets.faces, nets.vert_offsets, nets.face_offsets
    ids_of = torch.as_tensor(np.asarray([b % len(names) for b in range(B)], np.int32)).cuda()
    vcol = torch.as_tensor(rng.integers(0, 256, (int(q.shape[0]), 3)).astype(np.uint8)).cuda()
    fcol = torch.as_tensor(rng.integers(0, 256, (int(tris.shape[0]), 3)).astype(np.uint8)).cuda()
    sets = dict(vert_offsets=vo, tri_offsets=to, mesh_of_item=ids_of)
    kw = dict(new_size=N, pixels_per_cell=f)
    cam = ops.mesh_camera(pose, S, **kw)
    many = grids[ids_of.long()].contiguous()                                                     # 24 grids at 64^3
    quads = ops.extract_mesh(many, smooth=True)

    def raster():
        return ops.rasterize_mesh(q, tris, pose, S, smooth=False, return_ids=True, **sets, **kw)
    _, tri_id, _ = raster()
    want_v = ops.mesh_colour_from_ids(tri_id, q, tris, pose, S, vertex_colours=vcol, **sets, **kw)
    want_f = ops.mesh_colour_from_ids(tri_id, q, tris, pose, S, face_colours=fcol, **sets, **kw)
    same = (bool(torch.equal(want_v, torch_vertex(tri_id, q, tris, vo, to, ids_of, cam, vcol, S))),
            bool(torch.equal(want_f, torch_face(tri_id, to, ids_of, fcol))))
    if not all(same):
        raise SystemExit("mesh_colour_bench.py: the torch composition differs from the kernel (vertex, face) = %s" % (same,))
    legs = []
    for _ in range(a.legs):
        leg = {}
        for key, fn in (("raster", raster),
                        ("colour_vertex", lambda: ops.rasterize_mesh_colour(q, tris, pose, S, vertex_colours=vcol, **sets, **kw)),
                        ("colour_face", lambda: ops.rasterize_mesh_colour(q, tris, pose, S, face_colours=fcol, **sets, **kw)),
                        ("resolve_vertex", lambda: ops.mesh_colour_from_ids(tri_id, q, tris, pose, S, vertex_colours=vcol, **sets, **kw)),
                        ("resolve_face", lambda: ops.mesh_colour_from_ids(tri_id, q, tris, pose, S, face_colours=fcol, **sets, **kw)),
                        ("torch_vertex", lambda: torch_vertex(tri_id, q, tris, vo, to, ids_of, cam, vcol, S)),
                        ("torch_face", lambda: torch_face(tri_id, to, ids_of, fcol)),
                        ("face_voxels", lambda: ops.mesh_face_voxels(quads, many))):
            leg[key + "_us_per_call_events"] = timed(fn, a.calls)[0]
        legs.append(leg)
    tl = to.tolist()
    result = {"mesh_colour": {"calls": a.calls, "B": B, "S": S, "new_size": N, "pixels_per_cell": f, "meshes": len(names),
                              "triangles_per_mesh": [int(tl[m + 1] - tl[m]) for m in range(len(names))],
                              "hit_share": float((tri_id >= 0).float().mean().item()),
                              "face_voxels_grids": B, "face_voxels_faces": int(quads.faces.shape[0]),
                              "torch_equals_kernel": list(same), "legs": legs}}
    line = json.dumps(result)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        fh.write(line + "\n")
    print(line, flush=True)


if __name__ == "__main__":
    main()
