"""Removes the floaters and closes the bubbles of a voxel grid, on the device (rendernet_amd.ops.voxel_clean, rn_voxel_label):

    python -m rendernet_amd.tools.clean_voxels IN OUT [--keep N] [--min-voxels M] [--no-fill] [--connectivity 6|26]
                                                      [--threshold T] [--axes STR] [--size S] [--relax N]

IN is a .binvox grid, an .npz volume as Reconstruct_RenderNet_Face.py writes it (`<name>_Param.txt.npz`; --threshold matters
there) or an .obj / .ply mesh, read with the loaders of compare_voxels (a mesh is voxelised at --size, mode "both", --axes as
mesh_to_binvox takes it).  The components of at least --min-voxels voxels are kept, of those the --keep largest (0 keeps all),
and then every closed cavity is filled unless --no-fill.  OUT is a .binvox grid, or an .obj / .ply mesh of the cleaned grid
(rendernet_amd.mesh.extract; --axes as binvox_to_mesh takes it).  --relax N adds N passes of surface-net relaxation to a mesh output (rn_mesh_relax; 4 is the recommended setting).
Prints one JSON line: the topology words (voxels, components,
cavities, V, E, F, Euler number, handles; include/rendernet_hip.h) before and after, and the sizes of the dropped components in
label order.
"""
import argparse
import json
import os

import numpy as np


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m rendernet_amd.tools.clean_voxels", description=__doc__.split("\n")[0],
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("input", help=".binvox, .npz, .obj or .ply")
    parser.add_argument("output", help=".binvox, .obj or .ply")
    parser.add_argument("--keep", type=int, default=1, help="keep the N largest components (0: all)")
    parser.add_argument("--min-voxels", type=int, default=1, help="drop components smaller than this")
    parser.add_argument("--no-fill", action="store_true", help="leave the closed cavities open")
    parser.add_argument("--connectivity", type=int, default=26, choices=(6, 26), help="of the solid; the cavities take the dual")
    parser.add_argument("--threshold", type=float, default=0.5, help="a voxel is occupied above this")
    parser.add_argument("--axes", type=str, default="x,y,z", help="array axis order of a mesh's axes (signed)")
    parser.add_argument("--relax", type=int, default=0, help="passes of surface-net relaxation over a mesh output (0..64; 4 is the recommended setting)")
    parser.add_argument("--size", type=int, default=64, help="grid side for a mesh input (32, 64 or 128)")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    import torch
    from rendernet_amd import mesh, ops
    from rendernet_amd._lib import RenderNetHipError
    from rendernet_amd.tools import binvox_rw, compare_voxels
    from rendernet_amd.tools.binvox_to_mesh import load_grid
    try:
        mesh.parse_axes(args.axes)
        out_ext = os.path.splitext(args.output)[1].lower()
        if out_ext not in (".binvox", ".obj", ".ply"):
            raise ValueError("%s: expected a .binvox, .obj or .ply file" % os.path.basename(args.output))
        if compare_voxels._is_mesh(args.input):
            if args.size not in mesh.SIZES:
                raise ValueError("--size %d (32, 64 or 128)" % args.size)
            grid = mesh.voxelize(args.input, S=args.size, mode="both", axes=args.axes)[..., 0]
        else:
            g = load_grid(args.input)
            if g.ndim != 3 or len(set(g.shape)) != 1 or g.shape[0] not in mesh.SIZES:
                raise ValueError("%s: a grid of shape %s (32^3, 64^3 or 128^3)" % (os.path.basename(args.input), g.shape))
            grid = torch.from_numpy(np.ascontiguousarray(g)).cuda()[None]
        before = ops.voxel_topology(grid, args.threshold).as_dicts()[0]
        cleaned, dropped = ops._clean(grid, args.threshold, args.keep, args.min_voxels, not args.no_fill, args.connectivity)
        after = ops.voxel_topology(cleaned).as_dicts()[0]
        host = cleaned[0, ..., 0].cpu().numpy()
        if out_ext == ".binvox":
            binvox_rw.save_binvox(host > 0, args.output)
        else:
            mesh.save_mesh(args.output, *mesh.extract(host, relax=args.relax), axes=args.axes)
    except (ValueError, OSError, RenderNetHipError) as e:
        raise SystemExit("clean_voxels: %s" % e)
    row = {"input": args.input, "output": args.output, "size": int(host.shape[0]), "before": before, "after": after,
           "dropped": dropped[0]}
    print(json.dumps(row))
    return row


if __name__ == "__main__":
    main()
