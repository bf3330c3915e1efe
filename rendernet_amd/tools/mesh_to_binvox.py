"""Triangle mesh -> binvox file, on the device (rendernet_amd.mesh.voxelize, rn_mesh_voxelize):

    python -m rendernet_amd.tools.mesh_to_binvox in.obj out.binvox [--size 32|64|128] [--mode solid|surface|both]
                                                                   [--margin N] [--axes STR]

The file holds the grid as `binvox_rw.read_as_3d_array` returns it, which at --size 64 is what RenderNet_demo.py --voxel_path and
the training scripts read.  --axes is a signed permutation of the mesh axes, one per array axis; array axis 1 is up in the
shipped models ("z,y,x" stands a y-up mesh upright, "-y,z,x" a z-up one; rendernet_amd/mesh.py).
"""
import argparse

import numpy as np


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m rendernet_amd.tools.mesh_to_binvox", description=__doc__.split("\n")[0],
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("mesh", help="input .obj or .ply")
    parser.add_argument("binvox", help="output .binvox")
    parser.add_argument("--size", type=int, choices=[32, 64, 128], default=64, help="grid side")
    parser.add_argument("--mode", choices=["solid", "surface", "both"], default="both",
                        help="solid: voxel centres inside the mesh; surface: voxels a triangle touches; both: their union")
    parser.add_argument("--margin", type=int, default=1, help="empty voxels left on each side")
    parser.add_argument("--axes", type=str, default="x,y,z", help="mesh axis (signed) taken by each array axis")
    return parser


def main(argv=None):
    args = build_parser().parse_args(argv)
    from rendernet_amd import mesh
    from rendernet_amd.tools import binvox_rw
    try:
        vox = mesh.voxelize(args.mesh, S=args.size, mode=args.mode, margin=args.margin, axes=args.axes)
    except (ValueError, OSError) as e:
        raise SystemExit("mesh_to_binvox: %s" % e)
    grid = vox.cpu().numpy()[0, ..., 0] > 0
    binvox_rw.save_binvox(grid, args.binvox)
    print("%s: %d of %d^3 voxels" % (args.binvox, int(np.count_nonzero(grid)), args.size))


if __name__ == "__main__":
    main()
