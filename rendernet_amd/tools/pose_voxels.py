"""Finds the pose each picture of a model was taken at, on the device (rendernet_amd.ops.voxel_pose_search, rn_pose_score):

    python -m rendernet_amd.tools.pose_voxels MODEL IMAGE... [--size S] [--background black|white] [--threshold T]
                                                            [--azimuths N] [--refine L] [--copy-to DIR]

MODEL is a .binvox grid, an .npz volume or an .obj / .ply mesh, loaded as compare_voxels loads them (a mesh is voxelised at
--size).  Every IMAGE is thresholded into a silhouette as carve_voxels thresholds it (--background, --threshold in bytes) and is
square with a side that is a multiple of twice the grid's side: pixels_per_cell = side / (2 size) in a frame of 2 size cells.  A
picture finer than the search takes -- more than 256 pixels a side, or more pixels per voxel than the largest footprint covers
without holes -- is OR-pooled by two until it fits.  The search is exhaustive over --azimuths x synth.POSE_ELEVATIONS x
synth.POSE_SCALES and then refined --refine times around the winner.  Prints one JSON line per image: the pose (azimuth, elevation in
radians from the horizon, scale), its IoU, the three integers of the rule (include/rendernet_hip.h) and the footprint.
--copy-to DIR writes a copy of each image named `<model>_p<azimuth>_t<elevation>_r<radius>`, the name carve_voxels and
tools/data_util.extract_param_from_names read; the name keeps two decimals of the angles (degrees) and ONE of the radius, so the
line also gives `name_pose`, the pose the name stands for, and `name_iou`, the IoU re-scored at it.
"""
import argparse
import json
import math
import os
import shutil

import numpy as np

MAX_SIDE = 256
MAX_PIXELS_PER_VOXEL = 4.0 / math.sqrt(2.0)      # the bound of the largest footprint


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m rendernet_amd.tools.pose_voxels", description=__doc__.split("\n")[0],
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("model", metavar="MODEL", help=".binvox, .npz, .obj or .ply")
    parser.add_argument("images", nargs="+", metavar="IMAGE", help="pictures of the model")
    parser.add_argument("--size", type=int, default=64, help="grid side for a mesh (32, 64 or 128)")
    parser.add_argument("--background", type=str, default="black", choices=("black", "white"), help="of the images")
    parser.add_argument("--threshold", type=float, default=8.0, help="foreground differs from the background by more than this many bytes")
    parser.add_argument("--azimuths", type=int, default=24, help="azimuths of the level-0 lattice")
    parser.add_argument("--refine", type=int, default=2, help="refinement levels after the lattice (0..8)")
    parser.add_argument("--copy-to", type=str, default=None, metavar="DIR", help="write each image under a name that carries its pose")
    return parser


def parse_args(argv=None):
    parser = build_parser()
    args = parser.parse_args(argv)
    if os.path.splitext(args.model)[1].lower() not in (".binvox", ".npz", ".obj", ".ply"):
        parser.error("%s: expected a .binvox, .npz, .obj or .ply model" % os.path.basename(args.model))
    if args.size not in (32, 64, 128):
        parser.error("--size %d (32, 64 or 128)" % args.size)
    if args.azimuths < 1:
        parser.error("--azimuths %d (at least 1)" % args.azimuths)
    if not 0 <= args.refine <= 8:
        parser.error("--refine %d (0..8)" % args.refine)
    return args


def pose_name(model, pose, ext):
    """`<model>_p<azimuth>_t<elevation>_r<radius><ext>` of a pose (azimuth, elevation from the horizon, scale): degrees with two
    decimals, the file's elevation running from the up axis, the radius 3.3 / scale with ONE decimal -- the three characters
    extract_param_from_names reads, so it is kept inside 1.0..9.9.  Underscores of the model's name become dashes: the reader
    finds the fields by their first `_p`, `_t` and `_r`."""
    az, el, sc = (float(v) for v in pose)
    stem = os.path.splitext(os.path.basename(model))[0].replace("_", "-")
    radius = min(max(3.3 / sc if sc > 0 else 9.9, 1.0), 9.9)
    return "%s_p%.2f_t%.2f_r%.1f%s" % (stem, math.degrees(az) % 360.0, 90.0 - math.degrees(el), radius, ext)


def name_pose(name):
    """(azimuth, elevation, scale) float32 [3] the name stands for, by the reference's reader."""
    from rendernet_amd.tools import data_util
    return np.asarray(data_util.extract_param_from_names(os.path.basename(name))[0], np.float32)


def fit_mask(mask, size, max_scale):
    """(mask, f): the silhouette OR-pooled by two until it is at most 256 pixels a side and its f = side / (2 size) times
    `max_scale` is below the largest footprint's bound."""
    from rendernet_amd.tools.carve_voxels import pixels_per_cell_of
    m = np.asarray(mask, bool)
    f = pixels_per_cell_of(m.shape, size)
    while m.shape[0] > MAX_SIDE or f * max_scale >= MAX_PIXELS_PER_VOXEL:
        if f % 2:
            raise ValueError("an image of %d pixels a side for a %d^3 grid cannot be halved to fit the search" % (m.shape[0], size))
        h = m.shape[0] // 2
        m, f = m.reshape(h, 2, h, 2).any((1, 3)), f // 2
    return m, f


def load_model(path, size):
    """The grid as a device tensor [1,S,S,S] (uint8, or float32 for an .npz volume)."""
    import torch
    from rendernet_amd import mesh
    from rendernet_amd.tools.binvox_to_mesh import load_grid
    from rendernet_amd.tools.compare_voxels import _is_mesh
    if _is_mesh(path):
        return mesh.voxelize(path, S=size, mode="both")[..., 0]
    g = load_grid(path)
    if g.ndim != 3 or len(set(g.shape)) != 1 or g.shape[0] not in mesh.SIZES:
        raise ValueError("%s: a grid of shape %s (32^3, 64^3 or 128^3)" % (os.path.basename(path), g.shape))
    return torch.from_numpy(np.ascontiguousarray(g)).cuda()[None]


def read_mask(path, size, background, threshold, max_scale):
    from PIL import Image
    from rendernet_amd.tools.carve_voxels import silhouette
    with Image.open(path) as im:
        a = np.asarray(im.convert("RGB") if im.mode not in ("L", "RGB", "RGBA") else im)
    return fit_mask(silhouette(a, background, threshold), size, max_scale)


def main(argv=None):
    args = parse_args(argv)
    import torch
    from rendernet_amd import ops, synth
    from rendernet_amd._lib import RenderNetHipError
    rows = []
    try:
        grid = load_model(args.model, args.size)
        S = int(grid.shape[1])
        vox_thr = 0.5
        if args.copy_to is not None:
            os.makedirs(args.copy_to, exist_ok=True)
        for path in args.images:
            mask, f = read_mask(path, S, args.background, args.threshold, max(synth.POSE_SCALES))
            kw = dict(new_size=2 * S, pixels_per_cell=f, threshold=vox_thr)
            m = torch.from_numpy(mask.astype(np.uint8)).cuda()[None]
            found = ops.voxel_pose_search(m, grid.unsqueeze(-1), n_azimuth=args.azimuths, refine=args.refine, **kw)
            row = dict(found.as_dicts()[0], image=path, model=args.model, size=S, pixels_per_cell=f)
            if args.copy_to is not None:
                name = pose_name(args.model, row["pose"], os.path.splitext(path)[1])
                shutil.copyfile(path, os.path.join(args.copy_to, name))
                at = name_pose(name)
                again = ops.voxel_pose_scores(m, grid.unsqueeze(-1), torch.from_numpy(at[None]).cuda(), footprint=found.footprint, **kw)
                row.update(name=name, name_pose=[float(v) for v in at], name_iou=float(again.best_iou()[0]))
            print(json.dumps(row))
            rows.append(row)
    except (ValueError, OSError, RenderNetHipError) as e:
        raise SystemExit("pose_voxels: %s" % e)
    return rows


if __name__ == "__main__":
    main()
