"""Colours a model from posed pictures, on the device, and writes it as a coloured mesh (rendernet_amd.ops.voxel_colour_sums,
voxel_colours, mesh_vertex_colours; rn_voxel_colour_accumulate), in two forms:

    python -m rendernet_amd.tools.colour_voxels MODEL IMAGES_DIR OUT [--size 32|64|128] [--background black|white] [--threshold T]
                                                                     [--fill N] [--blocky [--merge]] [--axes STR] [--relax N] [--save-colours out.npz]
                                                                     [--preview DIR]
    python -m rendernet_amd.tools.colour_voxels --from-voxels IN --views K [--seed S] OUT [--fill N] [--blocky [--merge]] [--axes STR] [--relax N]
                                                                     [--preview DIR]

MODEL is a .binvox or .npz grid, which keeps its own side, or an .obj / .ply mesh voxelised at --size; OUT is an .obj or .ply.
The first form takes a folder of pictures named `<model>_p<azimuth>_t<elevation>_r<radius>`, the convention carve_voxels reads,
one view per picture, square with a side that is a multiple of twice the grid's.  Each picture's pose is cast through MODEL
for the voxel every pixel sees; the pixels of the silhouette (a colour channel further than --threshold bytes from the
--background) add their colour to that voxel; a voxel's colour is the rounded mean of what it received; --fill N then spreads
colour over N steps to occupied voxels that no picture saw; the surface-net mesh of MODEL (--blocky: the voxel faces) gets a
colour per vertex from the voxels around it; --relax N relaxes that mesh for N passes first (rn_mesh_relax; 4 is the recommended
setting), which moves the vertices inside their cells and leaves their colours as they are.  --save-colours keeps the voxel colours and the known flags as an .npz.
--preview DIR draws the coloured mesh that was just made, once for every input pose (the poses of the pictures; with
--from-voxels the scan poses), in the frame of the pictures, as `<model>_p<azimuth>_t<elevation>_r<radius>_mesh.png` under DIR
(ops.rasterize_mesh_colour; rn_mesh_rasterize + rn_mesh_colour_from_ids): the vertex colours interpolated, or with --blocky each
voxel face in the colour of its voxel (ops.mesh_face_colours), which is what the caster shows of the coloured grid.  The JSON
line then also has "preview": the number of pictures written.
--blocky --merge writes the voxel faces merged into rectangles (ops.extract_mesh_merged) with the packed colour of
`ops.voxel_colours` as the label, the voxels without a colour under a label of their own, so that faces merge only inside one
colour: every rectangle has exactly its voxels' colour, and the file has four private vertices per rectangle in that colour
(two rectangles of different colour may share a corner).  The JSON line then also has "merged_faces", the rectangles written,
beside "faces", the unit voxel faces they cover; --preview still draws the unit faces.  Not with --relax.
The second form is the self-check: it paints the grid IN with the albedo of rendernet_amd.synth.ColourModel(--seed) from the K
views of rendernet_amd.synth.scan_poses at two pixels per voxel, unsmoothed, colours the grid back from those pictures, and
reports "exact": true when every voxel that was seen has the field's colour and every view re-rendered from the coloured grid
equals its picture.  Prints one JSON line: views, size, the surface voxels (occupied with an empty 6-neighbour, the outside
being empty), how many voxels were seen, filled and -- of the surface -- left unseen, vertices and faces.
"""
import argparse
import json
import os

import numpy as np

from rendernet_amd.tools.carve_voxels import BACKGROUND, list_images, pixels_per_cell_of, pose_of_name, silhouette

MAX_VIEWS = 255
MAX_FILL = 64
SCAN_PIXELS_PER_CELL = 2
CHECK_WAVES = 8                          # plane waves of the self-check's colour field


def build_parser():
    parser = argparse.ArgumentParser(prog="python -m rendernet_amd.tools.colour_voxels", description=__doc__.split("\n")[0],
                                     formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    parser.add_argument("paths", nargs="+", metavar="PATH", help="MODEL IMAGES_DIR OUT, or OUT alone with --from-voxels")
    parser.add_argument("--from-voxels", type=str, default=None, metavar="IN", help="the self-check: paint this grid and colour it back")
    parser.add_argument("--views", type=int, default=24, help="views of the self-check (--from-voxels)")
    parser.add_argument("--seed", type=int, default=0, help="of the self-check's colour field (--from-voxels)")
    parser.add_argument("--size", type=int, default=64, help="grid side a mesh is voxelised at (32, 64 or 128)")
    parser.add_argument("--background", type=str, default="black", choices=sorted(BACKGROUND), help="of the pictures")
    parser.add_argument("--threshold", type=float, default=8.0, help="foreground differs from the background by more than this many bytes")
    parser.add_argument("--fill", type=int, default=0, help="steps that spread colour to occupied voxels no picture saw")
    parser.add_argument("--blocky", action="store_true", help="the voxel faces instead of the smooth surface net")
    parser.add_argument("--merge", action="store_true", help="with --blocky: voxel faces of one colour merged into rectangles")
    parser.add_argument("--axes", type=str, default="x,y,z", help="array axis order of a mesh's axes (signed)")
    parser.add_argument("--relax", type=int, default=0, help="passes of surface-net relaxation over the mesh (0..64; 4 is the recommended setting)")
    parser.add_argument("--save-colours", type=str, default=None, metavar="NPZ", help="also write the voxel colours and known flags")
    parser.add_argument("--preview", type=str, default=None, metavar="DIR",
                        help="also draw the coloured mesh at every input pose: <model>_p.._t.._r.._mesh.png under DIR")
    return parser


def parse_args(argv=None):
    """The arguments, the two forms told apart: args.images_dir is None for --from-voxels, and args.model is the grid either way."""
    parser = build_parser()
    args = parser.parse_args(argv)
    want = 1 if args.from_voxels is not None else 3
    if len(args.paths) != want:
        parser.error("expected %s" % ("OUT alone with --from-voxels" if want == 1 else "MODEL, IMAGES_DIR and OUT"))
    args.model = args.from_voxels if want == 1 else args.paths[0]
    args.images_dir = None if want == 1 else args.paths[1]
    args.output = args.paths[-1]
    if os.path.splitext(args.output)[1].lower() not in (".obj", ".ply"):
        parser.error("%s: expected an .obj or .ply file" % os.path.basename(args.output))
    if os.path.splitext(args.model)[1].lower() not in (".binvox", ".npz", ".obj", ".ply"):
        parser.error("%s: expected a .binvox, .npz, .obj or .ply model" % os.path.basename(args.model))
    if args.size not in (32, 64, 128):
        parser.error("--size %d (32, 64 or 128)" % args.size)
    if args.merge and (not args.blocky or args.relax):
        parser.error("--merge goes with --blocky and without --relax")
    if not 0 <= args.fill <= MAX_FILL:
        parser.error("--fill %d (0..%d)" % (args.fill, MAX_FILL))
    if args.from_voxels is not None and not 1 <= args.views <= MAX_VIEWS:
        parser.error("--views %d (1..%d)" % (args.views, MAX_VIEWS))
    if args.save_colours is not None and os.path.splitext(args.save_colours)[1].lower() != ".npz":
        parser.error("%s: expected an .npz file" % os.path.basename(args.save_colours))
    return args


def read_pictures(folder, size, background, threshold):
    """(images uint8 [K,H,W,3], masks uint8 [K,H,W], poses float32 [K,3], f, names) of a folder of pictures in sorted order."""
    from PIL import Image
    names = list_images(folder)
    images, masks, poses, f = [], [], [], None
    for n in names:
        with Image.open(os.path.join(folder, n)) as im:
            a = np.asarray(im.convert("RGB"))
        fn = pixels_per_cell_of(a.shape, size)
        if f is not None and fn != f:
            raise ValueError("%s is %d pixels wide and the pictures before it %d" % (n, a.shape[1], 2 * size * f))
        f = fn
        images.append(a)
        masks.append(silhouette(a, background, threshold).astype(np.uint8))
        poses.append(pose_of_name(n))
    return np.stack(images), np.stack(masks), np.stack(poses), f, names


def surface_voxels(occ):
    """bool like occ [S,S,S]: occupied with an empty 6-neighbour, the outside being empty."""
    o = np.pad(np.asarray(occ).astype(bool), 1)
    core = o[1:-1, 1:-1, 1:-1]
    buried = (o[:-2, 1:-1, 1:-1] & o[2:, 1:-1, 1:-1] & o[1:-1, :-2, 1:-1] & o[1:-1, 2:, 1:-1] & o[1:-1, 1:-1, :-2] & o[1:-1, 1:-1, 2:])
    return core & ~buried


def load_model(path, size, axes):
    """The grid of MODEL on the device, [1,S,S,S] uint8 or float32."""
    import torch
    from rendernet_amd import mesh
    from rendernet_amd.tools.binvox_to_mesh import load_grid
    if os.path.splitext(path)[1].lower() in (".obj", ".ply"):
        return mesh.voxelize(path, S=size, mode="both", axes=axes)[..., 0]
    g = load_grid(path)
    if g.ndim != 3 or len(set(g.shape)) != 1 or g.shape[0] not in mesh.SIZES:
        raise ValueError("%s: a grid of shape %s (32^3, 64^3 or 128^3)" % (os.path.basename(path), g.shape))
    return torch.from_numpy(np.ascontiguousarray(g)).cuda()[None]


def colour_sums(images, hits, S, mask=None):
    """ops.voxel_colour_sums over all K views, K in chunks that stay inside one call's limit."""
    from rendernet_amd import ops
    K, ph, pw = int(images.shape[1]), int(images.shape[2]), int(images.shape[3])
    step = max(ops.COLOUR_MAX_PIXELS // (ph * pw), 1)
    sums = None
    for k in range(0, K, step):
        sums = ops.voxel_colour_sums(images[:, k:k + step].contiguous(), hits[:, k:k + step].contiguous(), S,
                                     None if mask is None else mask[:, k:k + step].contiguous(), sums)
    return sums


PREVIEW_CHUNK = 8                        # poses per raster call of --preview


def write_previews(folder, model, m, vox, colours, known, vertex_colours, poses, low_x, kw, blocky):
    """One picture of the coloured mesh `m` (an ExtractedMesh with quads) per pose [K,3]: how many were written."""
    import torch
    from PIL import Image
    from rendernet_amd import ops
    from rendernet_amd.tools.pose_voxels import pose_name
    os.makedirs(folder, exist_ok=True)
    S = int(vox.shape[1])
    tris = m.faces[:, [0, 1, 2, 0, 2, 3]].reshape(-1, 3).contiguous()       # the fan of every quad, in order
    colour = dict(face_colours=ops.mesh_face_colours(m, vox, colours, known).repeat_interleave(2, 0)) if blocky \
        else dict(vertex_colours=vertex_colours)
    poses = torch.as_tensor(poses, dtype=torch.float32).cuda()
    low_x = [bool(v) for v in low_x]
    written = 0
    for low in (False, True):                                    # the ray end is one per call
        idx = [k for k in range(len(low_x)) if low_x[k] == low]
        for i in range(0, len(idx), PREVIEW_CHUNK):
            part = idx[i:i + PREVIEW_CHUNK]
            pictures = ops.rasterize_mesh_colour(m.q, tris, poses[part], S, view_from_low_x=low, **colour, **kw).cpu().numpy()
            for k, picture in zip(part, pictures):
                Image.fromarray(picture).save(os.path.join(folder, pose_name(model, poses[k].tolist(), "_mesh.png")))
                written += 1
    return written


def main(argv=None):
    args = parse_args(argv)
    import torch
    from rendernet_amd import mesh, ops, synth
    from rendernet_amd._lib import RenderNetHipError
    try:
        mesh.parse_axes(args.axes)
        grid = load_model(args.model, args.size, args.axes)
        vox = grid.unsqueeze(-1)
        S = int(grid.shape[1])
        row = {"output": args.output, "model": args.model}
        if args.images_dir is not None:
            images, masks, poses, f, _ = read_pictures(args.images_dir, S, args.background, args.threshold)
            K = len(poses)
            kw = dict(new_size=2 * S, pixels_per_cell=f)
            _, hits = ops.voxel_scan(vox, torch.from_numpy(poses).cuda()[None], return_hits=True, **kw)
            sums = colour_sums(torch.from_numpy(images).cuda()[None], hits, S, torch.from_numpy(masks).cuda()[None])
            colours, known = ops.voxel_colours(sums, vox, fill=args.fill)
            row.update(images=args.images_dir)
            view_poses, view_low = poses, [False] * K
        else:
            K = args.views
            kw = dict(new_size=2 * S, pixels_per_cell=SCAN_PIXELS_PER_CELL)
            cm = synth.ColourModel(args.seed, CHECK_WAVES)
            waves = torch.from_numpy(cm.waves).cuda()
            code_q = torch.from_numpy(cm.quantise(np.random.default_rng(args.seed).standard_normal((1, CHECK_WAVES)))).cuda()
            p, low = synth.scan_poses(K)
            poses = torch.from_numpy(p).cuda()
            _, hits = ops.voxel_scan(vox, poses[None], view_from_low_x=low, return_hits=True, **kw)
            images = torch.stack([ops.raycast_albedo(vox, poses[k:k + 1], waves, code_q, cm.base, smooth=0, view_from_low_x=low[k],
                                                     **kw)[0][0] for k in range(K)])[None]
            sums = colour_sums(images, hits, S)
            colours, known = ops.voxel_colours(sums, vox, fill=args.fill)
            cells = S ** 3
            rows = 1 << ((cells.bit_length() - 1 + 1) // 2)
            every = torch.arange(cells, dtype=torch.int32, device="cuda").view(1, rows, cells // rows)
            field = ops.albedo_from_hits(every, waves, code_q, S, cm.base, smooth=0).view(1, S, S, S, 3)
            seen = known == 1
            exact = bool((colours[seen] == field[seen]).all()) and int(seen.sum()) > 0
            for k in range(K):
                again = ops.raycast_colour(vox, colours, poses[k:k + 1], view_from_low_x=low[k], **kw)
                exact = exact and bool(torch.equal(again[0], images[0, k]))
            row.update(seed=args.seed, exact=exact)
            view_poses, view_low = p, list(np.broadcast_to(np.asarray(low, bool), (K,)))
        m = ops.extract_mesh(vox, threshold=0.5, smooth=not args.blocky, relax=args.relax)
        vc = ops.mesh_vertex_colours(m, colours, known)
        q, faces = m.q.cpu().numpy(), m.faces.cpu().numpy()
        if args.merge:
            c = colours.to(torch.int32)
            labels = torch.where(known != 0, (c[..., 0] << 16) | (c[..., 1] << 8) | c[..., 2], torch.full_like(c[..., 0], -1))
            merged = ops.extract_mesh_merged(vox, threshold=0.5, labels=labels.contiguous())
            corners = merged.unshared()
            mesh.save_mesh(args.output, corners.q.cpu().numpy(), corners.faces.cpu().numpy(), axes=args.axes,
                           colours=ops.merged_face_colours(merged, colours, known).repeat_interleave(4, 0).cpu().numpy())
            row.update(merged_faces=int(merged.faces.shape[0]))
        else:
            mesh.save_mesh(args.output, q, faces, axes=args.axes, colours=vc.cpu().numpy())
        if args.preview is not None:
            row.update(preview=write_previews(args.preview, args.model, m, vox, colours, known, vc, view_poses, view_low, kw, args.blocky))
        occ = (grid[0] > 0.5).cpu().numpy()
        kn = known[0].cpu().numpy()
        if args.save_colours is not None:
            np.savez_compressed(args.save_colours, colours=colours[0].cpu().numpy(), known=kn)
    except (ValueError, OSError, RenderNetHipError) as e:
        raise SystemExit("colour_voxels: %s" % e)
    surf = surface_voxels(occ)
    row.update(views=K, size=S, surface=int(surf.sum()), seen=int((kn == 1).sum()), filled=int((kn == 2).sum()),
               unseen=int((surf & (kn == 0)).sum()), vertices=int(len(q)), faces=int(len(faces)))
    print(json.dumps(row))
    return row


if __name__ == "__main__":
    main()
