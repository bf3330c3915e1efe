"""Puts one shape into the frame of another, as voxel grids, on the device (rendernet_amd.ops.voxel_align, rn_voxel_align):

    python -m rendernet_amd.tools.align_voxels MOVING FIXED OUT [--max-shift R] [--orientations none|rotations|all]
                                                                  [--threshold T[,T]] [--axes STR] [--size S] [--relax N]

MOVING and FIXED are each a .binvox grid, an .npz volume as Reconstruct_RenderNet_Face.py writes it (--threshold matters there,
one value for both or "TM,TF") or an .obj / .ply mesh, read with the loaders of compare_voxels (a mesh is voxelised at the other
argument's size, or at --size when both are meshes; --axes as mesh_to_binvox takes it).  Every signed axis permutation out of
--orientations and every shift of up to --max-shift voxels per axis (at most 16) is scored by the voxels the moved MOVING shares
with FIXED, exhaustively and exactly; include/rendernet_hip.h states the rule and the tie order.  OUT is the moved grid, a .binvox,
or an .obj / .ply mesh of it (rendernet_amd.mesh.extract; --axes as binvox_to_mesh takes it).  --relax N adds N passes of surface-net relaxation to a mesh output (rn_mesh_relax; 4 is the recommended setting).
Prints one JSON line: the
orientation (a row of rendernet_amd.ops.ORIENTATIONS), the shift (tz, ty, tx), the shared voxels and the IoU before and after.
"""
import argparse
import json
import os


def build_parser():
    from rendernet_amd.tools.compare_voxels import ALIGN_ORIENTATIONS
    parser = argparse.ArgumentParser(prog="python -m rendernet_amd.tools.align_voxels", description=__doc__.split("\n")[0],
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("moving", help="the shape that is moved: .binvox, .npz, .obj or .ply")
    parser.add_argument("fixed", help="the shape it is moved onto: .binvox, .npz, .obj or .ply")
    parser.add_argument("output", help=".binvox, .obj or .ply")
    parser.add_argument("--max-shift", type=int, default=8, help="shifts of up to this many voxels per axis (0..16)")
    parser.add_argument("--orientations", type=str, default="rotations", choices=ALIGN_ORIENTATIONS,
                        help="the signed axis permutations that are tried")
    parser.add_argument("--threshold", type=str, default="0.5", help="a voxel is occupied above this; T or TM,TF")
    parser.add_argument("--axes", type=str, default="x,y,z", help="array axis order of a mesh's axes (signed)")
    parser.add_argument("--relax", type=int, default=0, help="passes of surface-net relaxation over a mesh output (0..64; 4 is the recommended setting)")
    parser.add_argument("--size", type=int, default=64, help="grid side for two meshes (32, 64 or 128)")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    from rendernet_amd import mesh, ops
    from rendernet_amd._lib import RenderNetHipError
    from rendernet_amd.tools import binvox_rw, compare_voxels
    try:
        thr = [float(v) for v in args.threshold.split(",")]
        if len(thr) not in (1, 2):
            raise ValueError("--threshold %r: expected T or TM,TF" % args.threshold)
        mesh.parse_axes(args.axes)
        out_ext = os.path.splitext(args.output)[1].lower()
        if out_ext not in (".binvox", ".obj", ".ply"):
            raise ValueError("%s: expected a .binvox, .obj or .ply file" % os.path.basename(args.output))
        moving, fixed = compare_voxels.load_pair(args.moving, args.fixed, args.size, args.axes)
        found = ops.voxel_align(moving, fixed, max_shift=args.max_shift, orientations=args.orientations, threshold=(thr[0], thr[-1]))
        moved = found.apply((moving.float() > thr[0]).byte())       # the occupancy rn_voxel_pack saw
        host = moved[0].cpu().numpy()
        if out_ext == ".binvox":
            binvox_rw.save_binvox(host > 0, args.output)
        else:
            mesh.save_mesh(args.output, *mesh.extract(host, relax=args.relax), axes=args.axes)
    except (ValueError, OSError, RenderNetHipError) as e:
        raise SystemExit("align_voxels: %s" % e)
    row = dict(found.as_dicts()[0], moving=args.moving, fixed=args.fixed, output=args.output, size=int(host.shape[0]),
               max_shift=args.max_shift, orientations=args.orientations)
    print(json.dumps(row))
    return row


if __name__ == "__main__":
    main()
