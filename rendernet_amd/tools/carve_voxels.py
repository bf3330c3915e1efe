"""Carves a voxel grid from pictures, on the device (rendernet_amd.ops.voxel_carve, rn_voxel_carve), in two forms:

    python -m rendernet_amd.tools.carve_voxels IMAGES_DIR OUT [--size 32|64|128] [--background black|white] [--threshold T]
                                                              [--tolerance V] [--axes STR] [--relax N]
    python -m rendernet_amd.tools.carve_voxels --from-voxels IN --views K OUT [--threshold T] [--tolerance V] [--axes STR] [--relax N]

The first form takes a folder of rendered images whose names carry the pose, `<model>_p<azimuth>_t<elevation>_r<radius>` as
tools/data_util.extract_param_from_names reads it -- the reference's data convention -- one view per image (at most 255), and
carves the visual hull from their silhouettes: a pixel is foreground when any of its colour channels differs from the
--background by more than --threshold (in bytes; alpha is ignored).  The images are square with a side that is a multiple of
twice --size: pixels_per_cell = side / (2 size) in a frame of 2 size cells, the reference's 512^2 pictures of 64^3 grids at 4.
The second form scans the grid IN (.binvox, .npz, or an .obj / .ply mesh voxelised at --size) from the K views of
rendernet_amd.synth.scan_poses at two pixels per voxel and carves it back WITH depth: the round trip that returns a model bit for
bit from 24 views.  --tolerance V keeps a voxel that up to V views disagree with.  OUT is a .binvox grid, or an .obj / .ply mesh
of the hull (rendernet_amd.mesh.extract; --axes as binvox_to_mesh takes it).  --relax N adds N passes of surface-net relaxation to a mesh output (rn_mesh_relax; 4 is the recommended setting).
Prints one JSON line: the view count, the hull's
voxel count, the smallest pixels-per-voxel of the cameras and, when that is below 1.5, a warning (the hull may then miss thin
parts: include/rendernet_hip.h has the condition); the second form adds IoU, chamfer and Hausdorff distance against IN
(rendernet_amd.ops.voxel_shape_metrics).
"""
import argparse
import json
import os

import numpy as np

IMAGE_EXT = (".png", ".jpg", ".jpeg")
BACKGROUND = {"black": 0, "white": 255}
MAX_VIEWS = 255
MIN_PIXELS_PER_VOXEL = 1.5
SCAN_PIXELS_PER_CELL = 2


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m rendernet_amd.tools.carve_voxels", description=__doc__.split("\n")[0],
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("paths", nargs="+", metavar="PATH", help="IMAGES_DIR OUT, or OUT alone with --from-voxels")
    parser.add_argument("--from-voxels", type=str, default=None, metavar="IN", help="scan this grid instead of reading images")
    parser.add_argument("--views", type=int, default=24, help="views of the scan (--from-voxels)")
    parser.add_argument("--size", type=int, default=64, help="grid side (32, 64 or 128)")
    parser.add_argument("--background", type=str, default="black", choices=sorted(BACKGROUND), help="of the images")
    parser.add_argument("--threshold", type=float, default=None,
                        help="images: foreground differs from the background by more than this many bytes (default 8); "
                             "--from-voxels: a voxel is occupied above this (default 0.5)")
    parser.add_argument("--tolerance", type=int, default=0, help="views that may disagree with a voxel of the hull")
    parser.add_argument("--axes", type=str, default="x,y,z", help="array axis order of a mesh's axes (signed)")
    parser.add_argument("--relax", type=int, default=0, help="passes of surface-net relaxation over a mesh output (0..64; 4 is the recommended setting)")
    return parser


def parse_args(argv=None):
    """The arguments, the two forms told apart: args.images_dir is None for --from-voxels."""
    parser = build_parser()
    args = parser.parse_args(argv)
    want = 1 if args.from_voxels is not None else 2
    if len(args.paths) != want:
        parser.error("expected %s" % ("OUT alone with --from-voxels" if want == 1 else "IMAGES_DIR and OUT"))
    args.images_dir = None if want == 1 else args.paths[0]
    args.output = args.paths[-1]
    if os.path.splitext(args.output)[1].lower() not in (".binvox", ".obj", ".ply"):
        parser.error("%s: expected a .binvox, .obj or .ply file" % os.path.basename(args.output))
    if args.size not in (32, 64, 128):
        parser.error("--size %d (32, 64 or 128)" % args.size)
    if args.tolerance < 0:
        parser.error("--tolerance %d (at least 0)" % args.tolerance)
    if args.from_voxels is not None and not 1 <= args.views <= MAX_VIEWS:
        parser.error("--views %d (1..%d)" % (args.views, MAX_VIEWS))
    if args.threshold is None:
        args.threshold = 0.5 if args.from_voxels is not None else 8.0
    return args


def list_images(folder):
    """The image files of a folder in sorted order."""
    names = sorted(n for n in os.listdir(folder) if os.path.splitext(n)[1].lower() in IMAGE_EXT)
    if not names:
        raise ValueError("no %s images under %s" % (" / ".join(IMAGE_EXT), folder))
    if len(names) > MAX_VIEWS:
        raise ValueError("%d images under %s: at most %d views are carved at once" % (len(names), folder, MAX_VIEWS))
    return names


def pose_of_name(name):
    """(azimuth, elevation, scale) float32 [3] of an image name, by the reference's convention."""
    from rendernet_amd.tools import data_util
    return np.asarray(data_util.extract_param_from_names(os.path.basename(name))[0], np.float32)


def silhouette(img, background="black", threshold=8.0):
    """bool [H,W]: where any colour channel of img (uint8 [H,W] or [H,W,C]; of four channels the alpha is ignored) differs from
    the background's byte by more than `threshold`."""
    a = np.asarray(img)
    if a.dtype != np.uint8 or a.ndim not in (2, 3):
        raise ValueError("an image of dtype %s and shape %s (uint8 [H,W] or [H,W,C])" % (a.dtype, a.shape))
    if a.ndim == 2:
        a = a[..., None]
    if a.shape[2] in (2, 4):
        a = a[..., :-1]
    return (np.abs(a.astype(np.int16) - BACKGROUND[background]) > threshold).any(2)


def pixels_per_cell_of(shape, size):
    """f of an image for a grid of `size`: the side over the 2 size cells of the frame; the image is square and f divides."""
    h, w = int(shape[0]), int(shape[1])
    if h != w or h % (2 * size) != 0 or not 1 <= h // (2 * size) <= 16:
        raise ValueError("an image of %d x %d for a %d^3 grid: square, the side a multiple of %d up to %d"
                         % (h, w, size, 2 * size, min(32 * size, 2048)))
    return h // (2 * size)


def views_of_masks(masks):
    """Silhouettes bool [K,H,W] as views int32 [K,H,W]: 0 where foreground, -1 elsewhere."""
    return np.where(np.asarray(masks, bool), 0, -1).astype(np.int32)


def read_views(folder, size, background, threshold):
    """(views int32 [K,H,W], poses float32 [K,3], f, names) of a folder of images, decoded as the loader decodes them (PIL)."""
    from PIL import Image
    names = list_images(folder)
    masks, poses, f = [], [], None
    for n in names:
        with Image.open(os.path.join(folder, n)) as im:
            a = np.asarray(im.convert("RGB") if im.mode not in ("L", "RGB", "RGBA") else im)
        fn = pixels_per_cell_of(a.shape, size)
        if f is not None and fn != f:
            raise ValueError("%s is %d pixels wide and the images before it %d" % (n, a.shape[1], 2 * size * f))
        f = fn
        masks.append(silhouette(a, background, threshold))
        poses.append(pose_of_name(n))
    return views_of_masks(np.stack(masks)), np.stack(poses), f, names


def main(argv=None):
    args = parse_args(argv)
    import torch
    from rendernet_amd import mesh, ops, synth
    from rendernet_amd._lib import RenderNetHipError
    from rendernet_amd.tools import binvox_rw, compare_voxels
    from rendernet_amd.tools.binvox_to_mesh import load_grid
    try:
        mesh.parse_axes(args.axes)
        row = {"output": args.output}
        if args.images_dir is not None:
            views, poses, f, _ = read_views(args.images_dir, args.size, args.background, args.threshold)
            S, K = args.size, len(poses)
            kw = dict(new_size=2 * S, pixels_per_cell=f)
            poses = torch.from_numpy(poses).cuda()[None]
            hull = ops.voxel_carve(torch.from_numpy(views).cuda()[None], poses, S, use_depth=False,
                                   tolerance=args.tolerance, **kw)
            row.update(images=args.images_dir, mode="silhouettes")
        else:
            if compare_voxels._is_mesh(args.from_voxels):
                grid = mesh.voxelize(args.from_voxels, S=args.size, mode="both", axes=args.axes)[..., 0]
            else:
                g = load_grid(args.from_voxels)
                if g.ndim != 3 or len(set(g.shape)) != 1 or g.shape[0] not in mesh.SIZES:
                    raise ValueError("%s: a grid of shape %s (32^3, 64^3 or 128^3)" % (os.path.basename(args.from_voxels), g.shape))
                grid = torch.from_numpy(np.ascontiguousarray(g)).cuda()[None]
            S, K = int(grid.shape[1]), args.views
            kw = dict(new_size=2 * S, pixels_per_cell=SCAN_PIXELS_PER_CELL)
            p, low = synth.scan_poses(K)
            poses = torch.from_numpy(p).cuda()[None]
            kw["view_from_low_x"] = low
            views = ops.voxel_scan(grid.unsqueeze(-1), poses, threshold=args.threshold, **kw)
            hull = ops.voxel_carve(views, poses, S, use_depth=True, tolerance=args.tolerance, **kw)
            m = ops.voxel_shape_metrics(hull, grid, threshold=(0.5, args.threshold)).as_dicts()[0]
            row.update(input=args.from_voxels, mode="depth", iou=m["iou"], chamfer=m["chamfer"], hausdorff=m["hausdorff"])
        ppv = float(ops.carve_pixels_per_voxel(ops.carve_cameras(poses, S, **kw)).min())
        host = hull[0, ..., 0].cpu().numpy()
        if os.path.splitext(args.output)[1].lower() == ".binvox":
            binvox_rw.save_binvox(host > 0, args.output)
        else:
            mesh.save_mesh(args.output, *mesh.extract(host, relax=args.relax), axes=args.axes)
    except (ValueError, OSError, RenderNetHipError) as e:
        raise SystemExit("carve_voxels: %s" % e)
    row.update(views=K, size=S, voxels=int(host.sum()), pixels_per_voxel=ppv)
    if ppv < MIN_PIXELS_PER_VOXEL:
        row["warning"] = "%.2f pixels per voxel is below %.1f: the hull may miss thin parts" % (ppv, MIN_PIXELS_PER_VOXEL)
    print(json.dumps(row))
    return row


if __name__ == "__main__":
    main()
