"""How close two shapes are, as voxel grids, on the device (rendernet_amd.ops.voxel_shape_metrics, rn_voxel_shape_metrics):

    python -m rendernet_amd.tools.compare_voxels A B [--size S] [--threshold T[,T]] [--tau V] [--axes STR]
                                                   [--align [R]] [--align-orientations none|rotations|all]

A (the prediction) and B (the target) are each a .binvox grid, an .npz volume as Reconstruct_RenderNet_Face.py writes it
(`<name>_Param.txt.npz`; --threshold matters there, one value for both or "TA,TB"), or an .obj / .ply mesh.  A mesh is voxelised
(rendernet_amd.mesh.voxelize, mode "both", --axes as mesh_to_binvox takes it) at the other argument's size, or at --size when both
are meshes.  Prints one JSON line: the sixteen integer words of the rule (include/rendernet_hip.h) and the values derived from
them -- IoU, Dice, chamfer and Hausdorff distance in voxels, precision / recall / F-score at --tau voxels.  Grids of unequal size
are refused.

With --align (R = 8 when no number follows, at most 16) A is first registered to B (rendernet_amd.ops.voxel_align, rn_voxel_align:
the signed axis permutation out of --align-orientations and the shift of up to R voxels per axis that overlap most) and the line
holds the metrics of the ALIGNED pair, with `align_orientation`, `align_shift` (tz, ty, tx) and `iou_unaligned`, the IoU of the
pair as given.  Without --align the line is what it was.
"""
import argparse
import json
import os

import numpy as np

MESH_EXT = (".obj", ".ply")
ALIGN_ORIENTATIONS = ("none", "rotations", "all")


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m rendernet_amd.tools.compare_voxels", description=__doc__.split("\n")[0],
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("a", help="the prediction: .binvox, .npz, .obj or .ply")
    parser.add_argument("b", help="the target: .binvox, .npz, .obj or .ply")
    parser.add_argument("--size", type=int, default=64, help="grid side for two meshes (32, 64 or 128)")
    parser.add_argument("--threshold", type=str, default="0.5", help="a voxel is occupied above this; T or TA,TB")
    parser.add_argument("--tau", type=float, default=1.0, help="distance in voxels of the precision / recall / F-score")
    parser.add_argument("--axes", type=str, default="x,y,z", help="array axis order of a mesh's axes (signed)")
    parser.add_argument("--align", type=int, nargs="?", const=8, default=None, metavar="R",
                        help="register A to B first, shifts of up to R voxels per axis (0..16)")
    parser.add_argument("--align-orientations", type=str, default="rotations", choices=ALIGN_ORIENTATIONS,
                        help="the signed axis permutations --align tries")
    return parser


def _is_mesh(path):
    return os.path.splitext(path)[1].lower() in MESH_EXT


def load_pair(path_a, path_b, size=64, axes="x,y,z"):
    """The two grids as device tensors [1,S,S,S] (uint8, or float32 for an .npz volume)."""
    import torch
    from rendernet_amd import mesh
    from rendernet_amd.tools.binvox_to_mesh import load_grid
    grids = {}
    for key, path in (("a", path_a), ("b", path_b)):
        if not _is_mesh(path):
            g = load_grid(path)
            if g.ndim != 3 or len(set(g.shape)) != 1 or g.shape[0] not in mesh.SIZES:
                raise ValueError("%s: a grid of shape %s (32^3, 64^3 or 128^3)" % (os.path.basename(path), g.shape))
            grids[key] = torch.from_numpy(np.ascontiguousarray(g)).cuda()[None]
    S = int(next(iter(grids.values())).shape[1]) if grids else int(size)
    for key, path in (("a", path_a), ("b", path_b)):
        if _is_mesh(path):
            grids[key] = mesh.voxelize(path, S=S, mode="both", axes=axes)[..., 0]
    if grids["a"].shape != grids["b"].shape:
        raise ValueError("%s is %d^3 and %s is %d^3: grids of unequal size are not compared"
                         % (os.path.basename(path_a), grids["a"].shape[1], os.path.basename(path_b), grids["b"].shape[1]))
    return grids["a"], grids["b"]


def main(argv=None):
    args = build_parser().parse_args(argv)
    from rendernet_amd import mesh, ops
    from rendernet_amd._lib import RenderNetHipError
    try:
        thr = [float(v) for v in args.threshold.split(",")]
        if len(thr) not in (1, 2):
            raise ValueError("--threshold %r: expected T or TA,TB" % args.threshold)
        mesh.parse_axes(args.axes)
        a, b = load_pair(args.a, args.b, args.size, args.axes)
        found = None
        if args.align is not None:
            found = ops.voxel_align(a, b, max_shift=args.align, orientations=args.align_orientations,
                                    threshold=(thr[0], thr[-1])).as_dicts()[0]
            a = ops.voxel_transform(a, found["orientation"], found["shift"])
        row = ops.voxel_shape_metrics(a, b, threshold=(thr[0], thr[-1]), tau=args.tau).as_dicts()[0]
    except (ValueError, OSError, RenderNetHipError) as e:
        raise SystemExit("compare_voxels: %s" % e)
    row = dict(row, a=args.a, b=args.b, size=int(a.shape[1]), tau=args.tau)
    if found is not None:
        row.update(align_orientation=found["orientation"], align_shift=found["shift"], iou_unaligned=found["iou_before"])
    print(json.dumps(row))                                        # NaN for the distances of an empty surface, as json writes it
    return row


if __name__ == "__main__":
    main()
