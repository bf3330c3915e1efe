#!/usr/bin/env python
"""What surface-net relaxation costs on the device: 4 passes at weight 256 (the recommended setting), next to the extraction
itself and next to the same passes composed from torch ops.

    python scripts/mesh_relax_bench.py [--calls 200] [--rounds 7] [--out profiles/mesh_relax_bench.json]
        GPU.  Inputs: the chair at 64^3 (uint8, B = 1) and 24 grids of the five shipped models at 64^3 (uint8, B = 24).
        Forms, per input:
          extract        ops.extract_mesh(vol)
          extract_relax  ops.extract_mesh(vol, relax=4): the same call plus rn_mesh_relax (its workspace, the links launch, 4 passes)
          native         rn_mesh_relax alone on a prepared mesh (q restored by a device copy before every call, which is timed
                         with it and on its own as `copy`)
          torch          the same 4 passes from torch ops on a prepared [V,6] table of linked vertex indices: gather, sum, integer
                         divide, clamp.  The table, the link counts and the bounds are prepared outside the timed window, which
                         the native form's links launch is not.  The parent commit has no relaxation, so this is the baseline.
        Every round times `calls` calls of each form in turn between device events, after a warm-up of every form; `rounds` rounds
        alternate the forms, and the result gives the median, the least and the largest round of each, in microseconds per call.
        (a) = extract_relax - extract, per round.  The torch form's result is compared with the native one first: every word.

Writes the JSON result and prints it as ONE JSON line.
"""
import argparse
import ctypes
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
MODELS = ("bunny", "chair", "suzanne", "table", "teapot")
LEGS = ("chair64", "models64x24")
PASSES, WEIGHT = 4, 256


def make(leg):
    """The voxels of an input on the device: uint8 [B,64,64,64]."""
    import torch
    from rendernet_amd.tools import binvox_rw
    grids = {}
    for name in MODELS:
        with open(os.path.join(ROOT, "binvox", name + ".binvox"), "rb") as f:
            grids[name] = np.ascontiguousarray(binvox_rw.read_as_3d_array(f).data).astype(np.uint8)
    vols = [grids["chair"]] if leg == "chair64" else [grids[MODELS[k % len(MODELS)]] for k in range(24)]
    return torch.as_tensor(np.stack(vols)).cuda()


def link_table(faces, vert_offsets, face_offsets):
    """[V,6] int64 of GLOBAL linked vertex indices, V where there is none: the pairs of consecutive vertices of every quad ring."""
    V = int(vert_offsets[-1])
    src, dst = [], []
    for b in range(len(vert_offsets) - 1):
        f = faces[face_offsets[b]:face_offsets[b + 1]].astype(np.int64) + int(vert_offsets[b])
        for k in range(4):
            src += [f[:, k], f[:, (k + 1) % 4]]
            dst += [f[:, (k + 1) % 4], f[:, k]]
    key = np.unique(np.concatenate(src) * V + np.concatenate(dst))
    s, d = key // V, key % V
    start = np.searchsorted(s, np.arange(V))
    slot = np.arange(len(s)) - start[s]
    assert slot.max() < 6
    table = np.full((V, 6), V, np.int64)
    table[s, slot] = d
    return table


def torch_passes(q, table, n, lo, hi, zero_row, passes, weight):
    """The rule of rn_mesh_relax in torch ops; q int32 [V,3] -> int32 [V,3]."""
    import torch
    for _ in range(passes):
        sigma = torch.cat([q, zero_row])[table].sum(1, dtype=torch.int32)
        t = torch.div((256 - weight) * n * q + weight * sigma + 128 * n, 256 * n, rounding_mode="floor")
        q = torch.minimum(torch.maximum(t, lo), hi)
    return q


def prepare(vol):
    """The mesh of `vol` through the C entries, which leave the cell -> vertex volume that rn_mesh_relax reads."""
    import torch
    from rendernet_amd import _lib as L
    lib, vp = L.lib(), lambda t: ctypes.c_void_p(t.data_ptr())
    B, S, dev = int(vol.shape[0]), int(vol.shape[1]), vol.device
    nws = int(lib.rn_mesh_extract_workspace_bytes(B, S))
    ws = torch.empty((nws // 4,), dtype=torch.int32, device=dev)
    totals = torch.empty((B, 2), dtype=torch.int32, device=dev)
    L.check(lib.rn_mesh_extract_count(vp(vol), 1, 0.5, B, S, vp(ws), nws, vp(totals), L.stream_ptr()), "rn_mesh_extract_count")
    sums = torch.cumsum(totals.long(), 0)
    vo, qo = torch.zeros((B + 1,), dtype=torch.int64, device=dev), torch.zeros((B + 1,), dtype=torch.int64, device=dev)
    vo[1:], qo[1:] = sums[:, 0], sums[:, 1]
    V, F = (int(v) for v in sums[-1].tolist())
    q = torch.empty((V, 3), dtype=torch.int32, device=dev)
    faces = torch.empty((F, 4), dtype=torch.int32, device=dev)
    cellvert = torch.empty((B, (S + 1) ** 3), dtype=torch.int32, device=dev)
    L.check(lib.rn_mesh_extract_emit(vp(vol), 1, 0.5, B, S, L.RN_EXTRACT_SMOOTH, 0, vp(ws), nws, vp(vo), vp(qo), V, F, vp(cellvert),
                                     vp(q), vp(faces), L.stream_ptr()), "rn_mesh_extract_emit")
    nrws = int(lib.rn_mesh_relax_workspace_bytes(V))
    rws = torch.empty((nrws // 4,), dtype=torch.int32, device=dev)
    work = q.clone()

    def native():
        work.copy_(q)
        L.check(lib.rn_mesh_relax(vp(vol), 1, 0.5, B, S, vp(cellvert), vp(vo), V, PASSES, WEIGHT, vp(rws), nrws, vp(work),
                                  L.stream_ptr()), "rn_mesh_relax")
        return work
    return q, faces, vo, qo, native, lambda: work.copy_(q)


def time_leg(leg, calls, rounds):
    import torch
    from rendernet_amd import ops
    vol = make(leg)
    q, faces, vo, fo, native, copy = prepare(vol)
    V, S = int(q.shape[0]), int(vol.shape[1])
    table = torch.as_tensor(link_table(faces.cpu().numpy(), vo.cpu().numpy(), fo.cpu().numpy())).cuda()
    n = (table < V).sum(1, dtype=torch.int32)[:, None]
    cell = ((q + 128) >> 8) - 1
    lo, hi = torch.clamp(256 * cell + 129, min=0), torch.clamp(256 * cell + 383, max=256 * S)
    zero_row = torch.zeros((1, 3), dtype=torch.int32, device=q.device)
    forms = {"extract": lambda: ops.extract_mesh(vol),
             "extract_relax": lambda: ops.extract_mesh(vol, relax=PASSES, relax_weight=WEIGHT),
             "native": native, "copy": copy,
             "torch": lambda: torch_passes(q, table, n, lo, hi, zero_row, PASSES, WEIGHT)}
    want = ops.extract_mesh(vol, relax=PASSES, relax_weight=WEIGHT).q
    equal = bool(torch.equal(forms["torch"](), want)) and bool(torch.equal(native(), want)) and bool(torch.equal(ops.extract_mesh(vol).q, q))
    if not equal:
        raise SystemExit("%s: the forms disagree" % leg)
    for f in forms.values():
        for _ in range(10):
            f()
    torch.cuda.synchronize()
    us = {name: [] for name in forms}
    for _ in range(rounds):
        for name, f in forms.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(calls):
                f()
            e1.record()
            torch.cuda.synchronize()
            us[name].append(e0.elapsed_time(e1) * 1e3 / calls)

    def spread(v):
        return {"median": float(np.median(v)), "min": float(min(v)), "max": float(max(v))}
    row = {"leg": leg, "B": int(vol.shape[0]), "S": S, "vertices": V, "quads": int(faces.shape[0]), "calls": calls, "rounds": rounds,
           "forms_equal": equal, "us_per_call": {name: spread(v) for name, v in us.items()}}
    row["us_per_call"]["a_extract_relax_minus_extract"] = spread([r - e for r, e in zip(us["extract_relax"], us["extract"])])
    row["us_per_call"]["native_minus_copy"] = spread([r - e for r, e in zip(us["native"], us["copy"])])
    return row


def main(argv=None):
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("--calls", type=int, default=200)
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "mesh_relax_bench.json"))
    a = ap.parse_args(argv)
    import torch
    if not torch.cuda.is_available():
        raise SystemExit("mesh_relax_bench.py measures on the GPU; no HIP device found")
    result = {"mesh_relax": {"passes": PASSES, "weight": WEIGHT, "rows": [time_leg(leg, a.calls, a.rounds) for leg in LEGS]}}
    with open(a.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result), flush=True)


if __name__ == "__main__":
    main()
