"""Voxel grid -> surface-net mesh file, on the device (rendernet_amd.mesh.extract, rn_mesh_extract_count / _emit):

    python -m rendernet_amd.tools.binvox_to_mesh in.binvox|in.npz out.obj|out.ply [--threshold T] [--blocky [--merge]] [--axes STR] [--relax N] [--relax-weight W]

A .binvox grid is read as `binvox_rw.read_as_3d_array` returns it; an .npz is the raw volume Reconstruct_RenderNet_Face.py writes
(`<name>_Param.txt.npz`, its first array, [S,S,S] float32), so --threshold matters there: a sample is inside when its value is
above it.  S is 32, 64 or 128.  The mesh is in voxel units; --blocky writes the exposed voxel faces instead of the smoothed
surface; --relax N relaxes the vertices inside their cells for N passes at weight --relax-weight / 256 (rn_mesh_relax; 4 passes at
the default 256 is the recommended setting and takes the terraces off a binary grid).  --axes is the signed permutation mesh_to_binvox takes, applied backwards, so the same string brings the mesh back onto
the grid.  Voxelised again with --mode solid the mesh is the grid voxel for voxel.
--blocky --merge merges the coplanar voxel faces into rectangles (rn_mesh_merge_count / _emit): the same surface, and the same
grid when voxelised again, in far fewer quads -- the chair at 64^3 in 831 instead of 6780.  It goes with --blocky only and
not with --relax.  The merged file is for export; it has T-junctions, so the unit-quad file is the one to draw.
"""
import argparse
import os

import numpy as np


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m rendernet_amd.tools.binvox_to_mesh", description=__doc__.split("\n")[0],
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("grid", help="input .binvox, or .npz holding one [S,S,S] volume")
    parser.add_argument("mesh", help="output .obj or .ply")
    parser.add_argument("--threshold", type=float, default=0.5, help="a sample is inside when its value is above this")
    parser.add_argument("--blocky", action="store_true", help="vertices on voxel corners: exactly the exposed voxel faces")
    parser.add_argument("--merge", action="store_true", help="with --blocky: coplanar voxel faces merged into rectangles")
    parser.add_argument("--axes", type=str, default="x,y,z", help="mesh axis (signed) that each array axis is written to")
    parser.add_argument("--relax", type=int, default=0, help="passes of surface-net relaxation over the mesh (0..64; 4 is the recommended setting)")
    parser.add_argument("--relax-weight", type=int, default=256, help="how far a pass moves a vertex towards its neighbours' mean, in 1/256 (1..256)")
    return parser


def load_grid(path):
    """[S,S,S] uint8 (binvox) or float32 (npz) of the file."""
    ext = os.path.splitext(path)[1].lower()
    if ext == ".binvox":
        from rendernet_amd.tools import binvox_rw
        with open(path, "rb") as f:
            return np.ascontiguousarray(binvox_rw.read_as_3d_array(f).data).astype(np.uint8)
    if ext == ".npz":
        with np.load(path) as z:
            if not z.files:
                raise ValueError("%s holds no array" % os.path.basename(path))
            vol = np.asarray(z[z.files[0]])
        if vol.dtype.kind not in "fiub":
            raise ValueError("%s: a volume of %s" % (os.path.basename(path), vol.dtype))
        return np.squeeze(vol).astype(np.float32)
    raise ValueError("%s: expected a .binvox or .npz file" % os.path.basename(path))


def main(argv=None):
    args = build_parser().parse_args(argv)
    from rendernet_amd import mesh
    from rendernet_amd._lib import RenderNetHipError
    try:
        mesh.parse_axes(args.axes)
        if args.merge and (not args.blocky or args.relax):
            raise ValueError("--merge goes with --blocky and without --relax")
        if os.path.splitext(args.mesh)[1].lower() not in (".obj", ".ply"):
            raise ValueError("%s: expected an .obj or .ply file" % os.path.basename(args.mesh))
        grid = load_grid(args.grid)
        if grid.ndim != 3 or len(set(grid.shape)) != 1 or grid.shape[0] not in mesh.SIZES:
            raise ValueError("%s: a grid of shape %s (32^3, 64^3 or 128^3)" % (os.path.basename(args.grid), grid.shape))
        q, faces = mesh.extract(grid, threshold=args.threshold, smooth=not args.blocky, relax=args.relax, relax_weight=args.relax_weight,
                                merge=args.merge)
        mesh.save_mesh(args.mesh, q, faces, axes=args.axes)
    except (ValueError, OSError, RenderNetHipError) as e:
        raise SystemExit("binvox_to_mesh: %s" % e)
    print("%s: %d vertices, %d quads" % (args.mesh, len(q), len(faces)))


if __name__ == "__main__":
    main()
