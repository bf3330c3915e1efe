#!/usr/bin/env python
"""RenderNet Phong shading demo on the MI355X path -- same command line as the reference's
RenderNet_demo.py (flags :72-108, pose convention :33-38, output naming :60-64).

The network outputs a normal map from a 3D voxel grid; the normal map is then Phong-shaded with
lighting control.  Differences from the reference, all forced by what the reference ships:
  * no frozen TF graph exists (./model/3d2d_renderer.pb is a Google-Drive link, README.md:185-189):
    weights come from --weights (an .npz keyed by the TF variable names) or, by default, from the
    seeded reference initialisers -- the demo then exercises the full path but renders noise;
  * --voxel_path defaults to ./voxel/Misc/bunny.binvox as in the reference and falls back to the
    shipped ./binvox/bunny.binvox when that path does not exist (reference defect);
  * --rotate renders the 72 poses as batches instead of 72 batch-1 session runs;
  * --reference_render True also writes, beside each output, the ground truth of that pose: the exact normal map of the
    voxel grid from the device ray caster (`<name>_reference_normal.png`, rn_raycast_fwd) and its Phong composite under
    the same light (`<name>_reference_phong.png`) -- the picture a perfectly trained net would give;
  * --reference_ao True writes `<name>_reference_ao.png` beside each output: the ambient occlusion of the voxel grid at the
    pose (rn_raycast_ao_fwd, 16-voxel rays), the non-local shading a normal map cannot give;
  * --reference_lines True writes `<name>_reference_outline.png` and `<name>_reference_cel.png` beside each output: the
    contour drawing of the voxel grid at the pose and its cel shading under the --light_* direction (rn_raycast_edges_fwd,
    rn_lines_encode);
  * --reference_shadow True writes `<name>_reference_shadow.png` beside each output: the diffuse shading of the voxel grid
    under the --light_* direction with the shadows the grid casts on itself (rn_raycast_shadow_fwd, rn_shadow_encode);
  * --voxel_shape ID (hex, with --shape_seed, default 1234) renders, in place of --voxel_path, the procedural shape of that id
    (rendernet_amd/synth.py shape_prims, rn_voxel_shapes): the grid behind a `shape<ID>_p.._t.._r..` sample of
    `RenderNet_Shader.py --train --synthetic --synthetic-shapes P`; --save_binvox PATH also writes that grid as a binvox file;
  * --mesh_path FILE renders, in place of --voxel_path, the triangle mesh in an .obj or .ply file, voxelised on the device at
    64^3 (rendernet_amd/mesh.py, rn_mesh_voxelize): --mesh_mode solid | surface | both (default: both, voxel centres inside the
    mesh plus every voxel a triangle touches), --mesh_margin N empty voxels on each side (default 1) and --mesh_axes STR, the
    signed mesh axis each array axis takes (default "x,y,z"; array axis 1 is up: "z,y,x" stands a y-up mesh upright).
    --save_binvox PATH writes this grid too, and every --reference_* picture is drawn from it;
  * --save_mesh FILE (.obj or .ply) writes the surface-net mesh of the grid that is rendered -- of --voxel_path, --mesh_path or
    --voxel_shape alike -- extracted on the device (rendernet_amd/mesh.py, rn_mesh_extract_count / _emit), in voxel units;
    --mesh_blocky True writes the exposed voxel faces instead of the smoothed surface, and --mesh_relax N [--mesh_relax_weight W]
    relaxes the vertices inside their cells for N passes (rn_mesh_relax; 4 at the default weight 256 is the recommended setting,
    which takes the terraces off a binary grid).  Voxelised again in solid mode the mesh is the grid voxel for voxel either way;
    --mesh_blocky True --mesh_merge True merges the coplanar voxel faces into rectangles (rn_mesh_merge_count / _emit): the same
    surface and the same round trip in far fewer quads, for export (not with --mesh_relax);
  * --mesh_path FILE --reference_mesh True writes `<name>_reference_mesh_normal.png` and `<name>_reference_mesh_phong.png` beside
    each output: the normal map of the MESH ITSELF at the pose, rasterised on the device under the ray caster's camera
    (rendernet_amd/mesh.py MeshSet, rn_mesh_rasterize), and its Phong composite under the same light -- it overlays the
    --reference_render pictures of the mesh's voxelisation pixel for pixel; --mesh_flat True shades with face normals,
    --mesh_cull none keeps triangles seen from inside (for meshes that are open or not wound consistently).  When FILE carries
    vertex colours (a coloured .ply or .obj, as `colour_voxels` and `mesh.save_mesh(..., colours=)` write them) the same raster
    pass also writes `<name>_reference_mesh_colour.png`, the interpolated vertex colours (rn_mesh_colour_from_ids), and
    `<name>_reference_mesh_colour_phong.png`, the Phong composite of the rasterised normal map with that albedo; a file without
    colours writes exactly the files it always did.
"""
import argparse
import math
import os

import numpy as np

# Phong shading parameters (RenderNet_demo.py:17-20)
AMBIENT_IN = (0.1)
K_DIFFUSE = .9
LIGHT_COL = np.array([[1., 1., 1.]])


def compute_pose_param(azimuth, elevation, radius):
    """RenderNet_demo.py:33-38."""
    phi = azimuth * math.pi / 180.0
    theta = (90 - elevation) * math.pi / 180
    param = np.array([phi, theta, 3.3 / radius])
    return np.expand_dims(param, axis=0)


def _str2bool(v):
    # the reference declares `type=bool` (:103-104): any non-empty string is True
    return bool(v)


def build_parser():
    fmt_cls = argparse.ArgumentDefaultsHelpFormatter
    parser = argparse.ArgumentParser(formatter_class=fmt_cls)
    parser.add_argument('--voxel_path', type=str, default="./voxel/Misc/bunny.binvox", help="Path to the input voxel.")
    parser.add_argument('--azimuth', type=float, default=250, help="Value of azimuth, between (0,360)")
    parser.add_argument('--elevation', type=float, default=60, help="Value of elevation, between (0,360)")
    parser.add_argument('--light_azimuth', type=float, default=250, help="Value of azimuth for light, between (0,360)")
    parser.add_argument('--light_elevation', type=float, default=60, help="Value of elevation for light, between (0,360)")
    parser.add_argument('--radius', type=float, default=3.3, help="Value of radius, between (2.5, 4.5)")
    parser.add_argument('--render_dir', type=str, default='./render', help='Path to the rendered images.')
    parser.add_argument('--rotate', type=_str2bool, default=False,
                        help='Flag rotate and render an object by 360 degree in azimuth. Overwrites early settings in azimuth.')
    # additions (not in the reference)
    parser.add_argument('--weights', type=str, default=None,
                        help='.npz of weights keyed by TF variable names, or the reference\'s frozen graph `*.pb` '
                             '(its Const nodes are read without TensorFlow); default: seeded random initialisation')
    parser.add_argument('--batch', type=int, default=24, help='poses rendered per launch with --rotate')
    parser.add_argument('--gemm', choices=['f32', 'split', 'split16'], default=None,
                        help='multiply stage of the wide convs: default = the library default (`split`: every fp32 operand as three '
                             'bf16 pieces that sum exactly to it, six piece products, fp32 accumulation -- fp32-class error on the '
                             '16x faster bf16 matrix pipe; include/rendernet_hip.h, rn_conv2d_winograd_split_fwd; env RN_WINO_GEMM); '
                             '`f32` = exact-fp32 MFMA everywhere; `split16` = two fp16 pieces of value / tensor scale (22-bit operands)')
    parser.add_argument('--no_winograd_check', action='store_true',
                        help='weights given with --weights are checked once against F(4x4,3x3) where the net would take F(6x6,3x3) '
                             '(Renderer.validate_winograd, tolerance 2e-4 of max|y| per layer); this flag skips the check')
    parser.add_argument('--gif', type=str, default=None,
                        help='with --rotate: also write the 72 frames as an animated GIF to this path (the reference ships '
                             'such turntables under images/*.gif, README.md)')
    parser.add_argument('--reference_render', type=_str2bool, default=False,
                        help='also write <name>_reference_normal.png, the ray-cast normal map of the voxel grid at the pose, and '
                             '<name>_reference_phong.png, its Phong composite, beside every output')
    parser.add_argument('--reference_ao', type=_str2bool, default=False,
                        help='also write <name>_reference_ao.png, the ray-cast ambient occlusion of the voxel grid at the pose, '
                             'beside every output')
    parser.add_argument('--reference_lines', type=_str2bool, default=False,
                        help='also write <name>_reference_outline.png, the ray-cast contour drawing of the voxel grid at the pose, '
                             'and <name>_reference_cel.png, its cel shading under the light, beside every output')
    parser.add_argument('--reference_shadow', type=_str2bool, default=False,
                        help='also write <name>_reference_shadow.png, the ray-cast diffuse shading of the voxel grid with its cast '
                             'shadows under the light, beside every output')
    parser.add_argument('--voxel_shape', type=str, default=None,
                        help='render the procedural shape of this 32-bit id (hex, as in the sample names shape<ID>_p.._t.._r.. of '
                             '--synthetic-shapes training) in place of --voxel_path')
    parser.add_argument('--shape_seed', type=int, default=1234,
                        help='seed of the procedural shapes (the training config\'s "synthetic_shape_seed", default its "synthetic_seed")')
    parser.add_argument('--save_binvox', type=str, default=None,
                        help='with --voxel_shape or --mesh_path: also write the grid to this binvox file')
    parser.add_argument('--mesh_path', type=str, default=None,
                        help='render the triangle mesh in this .obj or .ply file, voxelised on the device, in place of --voxel_path')
    parser.add_argument('--mesh_mode', choices=['solid', 'surface', 'both'], default='both',
                        help='with --mesh_path: voxel centres inside the mesh, voxels a triangle touches, or their union')
    parser.add_argument('--mesh_margin', type=int, default=1, help='with --mesh_path: empty voxels left on each side of the grid')
    parser.add_argument('--mesh_axes', type=str, default='x,y,z',
                        help='with --mesh_path: the signed mesh axis each array axis takes (array axis 1 is up; "z,y,x" stands a '
                             'y-up mesh upright)')
    parser.add_argument('--save_mesh', type=str, default=None,
                        help='also write the surface-net mesh of the rendered grid to this .obj or .ply file (voxel units)')
    parser.add_argument('--mesh_blocky', type=_str2bool, default=False,
                        help='with --save_mesh: the exposed voxel faces instead of the smoothed surface')
    parser.add_argument('--mesh_merge', type=_str2bool, default=False,
                        help='with --save_mesh and --mesh_blocky: coplanar voxel faces merged into rectangles')
    parser.add_argument('--mesh_relax', type=int, default=0,
                        help='with --save_mesh: passes of surface-net relaxation (0..64; 4 is the recommended setting)')
    parser.add_argument('--mesh_relax_weight', type=int, default=256,
                        help="with --mesh_relax: how far a pass moves a vertex towards its neighbours' mean, in 1/256 (1..256)")
    parser.add_argument('--reference_mesh', type=_str2bool, default=False,
                        help='with --mesh_path: also write <name>_reference_mesh_normal.png, the rasterised normal map of the mesh '
                             'itself at the pose, and <name>_reference_mesh_phong.png, its Phong composite, beside every output')
    parser.add_argument('--mesh_flat', type=_str2bool, default=False,
                        help='with --reference_mesh: face normals instead of interpolated vertex normals')
    parser.add_argument('--mesh_cull', choices=['back', 'none'], default='back',
                        help='with --reference_mesh: drop or keep triangles seen from inside')
    return parser


def shape_voxels(shape_id, shape_seed, device="cuda"):
    """The 64^3 grid of procedural shape `shape_id` as the demo feeds it, float32 [1,64,64,64,1] on the host."""
    import torch
    from rendernet_amd import ops, synth
    prims = torch.as_tensor(synth.shape_prims(shape_seed, [shape_id], 64)).to(device)
    return ops.voxel_shapes(prims, 64).cpu().numpy().astype(np.float32)


def mesh_voxels(path, mode="both", margin=1, axes="x,y,z", device="cuda"):
    """The 64^3 grid of the mesh file `path` as the demo feeds it, float32 [1,64,64,64,1] on the host."""
    from rendernet_amd import mesh
    return mesh.voxelize(path, S=64, mode=mode, margin=margin, axes=axes, device=device).cpu().numpy().astype(np.float32)


def save_path_for(render_dir, count, model_name, azimuth, elevation, radius, light_azimuth, light_elevation):
    """RenderNet_demo.py:60-64."""
    return os.path.join(render_dir, str(count).zfill(3) + "_" + model_name + "_pose_%f_%f_%f_light_%f_%f.png" %
                        (azimuth, elevation, radius, light_azimuth, light_elevation))


def render(azimuths, elevation, radius, renderer, voxel, light_dir, render_dir, count0, light_azimuth,
           light_elevation, model_name, reference_render=False, reference_ao=False, reference_lines=False,
           reference_shadow=False, reference_mesh=None):
    """RenderNet_demo.py:41-66 for a batch of azimuths."""
    from PIL import Image
    from rendernet_amd.tools import Phong_shading
    params = np.concatenate([compute_pose_param(a, elevation, radius) for a in azimuths], 0)
    vox = np.repeat(voxel, len(azimuths), axis=0)
    normals = renderer.render(vox, params)                              # HIP tensor [B,512,512,3]
    img_phong = Phong_shading.np_phong_composite(normals, light_dir, LIGHT_COL, AMBIENT_IN, K_DIFFUSE).cpu().numpy()
    if reference_render:
        import torch
        from rendernet_amd import ops
        ref_normals = ops.raycast_normals(torch.as_tensor(vox).to(normals.device), torch.as_tensor(params, dtype=torch.float32).to(normals.device))
        ref_phong = Phong_shading.np_phong_composite(ref_normals.float() / 255.0, light_dir, LIGHT_COL, AMBIENT_IN, K_DIFFUSE).cpu().numpy()
        ref_normals = ref_normals.cpu().numpy()
    if reference_ao:
        import torch
        from rendernet_amd import ops
        ref_ao = ops.raycast_ao(torch.as_tensor(vox).to(normals.device), torch.as_tensor(params, dtype=torch.float32).to(normals.device)).cpu().numpy()
    if reference_lines:
        import torch
        from rendernet_amd import ops
        dev_vox, dev_params = torch.as_tensor(vox).to(normals.device), torch.as_tensor(params, dtype=torch.float32).to(normals.device)
        ref_outline = ops.raycast_outline(dev_vox, dev_params).cpu().numpy()
        ref_cel = ops.raycast_cel(dev_vox, dev_params, light=np.asarray(light_dir).reshape(-1)).cpu().numpy()
    if reference_shadow:
        import torch
        from rendernet_amd import ops
        ref_shadow = ops.raycast_shadow(torch.as_tensor(vox).to(normals.device), torch.as_tensor(params, dtype=torch.float32).to(normals.device),
                                        light=np.asarray(light_dir).reshape(-1)).cpu().numpy()
    if reference_mesh is not None:                                      # (MeshSet, smooth, cull)
        import torch
        mesh_set, smooth, cull = reference_mesh
        mesh_colour = None
        if mesh_set.colours is None:
            mesh_normals = mesh_set.rasterize([0] * len(azimuths), torch.as_tensor(params, dtype=torch.float32).to(normals.device),
                                              smooth=smooth, cull=cull)
        else:                                                           # the file carries vertex colours: the albedo of the same pass
            from rendernet_amd import ops
            mesh_colour, mesh_normals = mesh_set.rasterize_colour([0] * len(azimuths), torch.as_tensor(params, dtype=torch.float32).to(normals.device),
                                                                  smooth=smooth, cull=cull, return_normals=True)
            dev_of = lambda v: torch.as_tensor(np.asarray(v, np.float32)).to(normals.device)
            mesh_colour_phong = ops.phong_composite(mesh_normals.float() / 255.0, dev_of(light_dir), dev_of(LIGHT_COL), AMBIENT_IN, K_DIFFUSE,
                                                    "np_black", albedo=mesh_colour.float() / 255.0).cpu().numpy()
            mesh_colour = mesh_colour.cpu().numpy()
        mesh_phong = Phong_shading.np_phong_composite(mesh_normals.float() / 255.0, light_dir, LIGHT_COL, AMBIENT_IN, K_DIFFUSE).cpu().numpy()
        mesh_normals = mesh_normals.cpu().numpy()
    paths = []
    for i, a in enumerate(azimuths):
        image_out = np.clip(255. * img_phong[i], 0, 255).astype(np.uint8)
        p = save_path_for(render_dir, count0 + i, model_name, a, elevation, radius, light_azimuth, light_elevation)
        print(p)
        Image.fromarray(image_out).save(p)
        paths.append(p)
        if reference_render:
            Image.fromarray(ref_normals[i]).save(p[:-len(".png")] + "_reference_normal.png")
            Image.fromarray(np.clip(255. * ref_phong[i], 0, 255).astype(np.uint8)).save(p[:-len(".png")] + "_reference_phong.png")
        if reference_ao:
            Image.fromarray(ref_ao[i]).save(p[:-len(".png")] + "_reference_ao.png")
        if reference_lines:
            Image.fromarray(ref_outline[i]).save(p[:-len(".png")] + "_reference_outline.png")
            Image.fromarray(ref_cel[i]).save(p[:-len(".png")] + "_reference_cel.png")
        if reference_shadow:
            Image.fromarray(ref_shadow[i]).save(p[:-len(".png")] + "_reference_shadow.png")
        if reference_mesh is not None:
            Image.fromarray(mesh_normals[i]).save(p[:-len(".png")] + "_reference_mesh_normal.png")
            Image.fromarray(np.clip(255. * mesh_phong[i], 0, 255).astype(np.uint8)).save(p[:-len(".png")] + "_reference_mesh_phong.png")
            if mesh_colour is not None:
                Image.fromarray(mesh_colour[i]).save(p[:-len(".png")] + "_reference_mesh_colour.png")
                Image.fromarray(np.clip(255. * mesh_colour_phong[i], 0, 255).astype(np.uint8)).save(p[:-len(".png")] + "_reference_mesh_colour_phong.png")
    return paths


def main(argv=None):
    args = build_parser().parse_args(argv)
    shape_id = None
    if args.voxel_shape is not None:
        try:
            shape_id = int(args.voxel_shape, 16)
            if not 0 <= shape_id < 1 << 32:
                raise ValueError(args.voxel_shape)
        except ValueError:
            raise SystemExit("--voxel_shape %r: expected a 32-bit id in hex, such as 1a2b3c4d" % args.voxel_shape)
        if args.mesh_path is not None:
            raise SystemExit("--voxel_shape and --mesh_path both name the grid: give one")
    elif args.mesh_path is not None:
        from rendernet_amd import mesh
        try:                                                      # refused before the net is built
            mesh.parse_axes(args.mesh_axes)
            if not 0 <= args.mesh_margin < 32:
                raise ValueError("--mesh_margin %d: expected 0..31 voxels" % args.mesh_margin)
            if not os.path.exists(args.mesh_path):
                raise ValueError("--mesh_path %s: no such file" % args.mesh_path)
        except ValueError as e:
            raise SystemExit(str(e))
    elif args.save_binvox:
        raise SystemExit("--save_binvox needs --voxel_shape")
    if args.reference_mesh and args.mesh_path is None:
        raise SystemExit("--reference_mesh draws the mesh of --mesh_path: give one")
    if args.save_mesh is not None and os.path.splitext(args.save_mesh)[1].lower() not in (".obj", ".ply"):
        raise SystemExit("--save_mesh %s: expected an .obj or .ply file" % args.save_mesh)
    if args.mesh_merge and (not args.mesh_blocky or args.mesh_relax):
        raise SystemExit("--mesh_merge goes with --mesh_blocky True and without --mesh_relax")
    from rendernet_amd.shader import Renderer, ShaderSpec, init_shader_weights
    from rendernet_amd.tools import binvox_rw, Phong_shading

    spec = ShaderSpec(out_ch=3).check()                       # the demo graph has the 3-channel normal-map head
    if args.weights and args.weights.endswith(".pb"):
        # the reference's frozen graph (RenderNet_demo.py:23-30, :111 `./model/3d2d_renderer.pb`, made by
        # demo/RenderNet_converter.py): its variables are Const nodes under their TF names
        from rendernet_amd.tools.graphdef import load_frozen_weights
        from rendernet_amd.shader import shader_variable_shapes
        weights = load_frozen_weights(args.weights, {name: tuple(shape) for name, shape, _ in shader_variable_shapes(spec)})
    elif args.weights:
        weights = dict(np.load(args.weights))
    else:
        print("no --weights given: using seeded random weights (the reference ships no trained model)")
        weights = init_shader_weights(spec, seed=1234)
    renderer = Renderer(spec, weights, gemm=args.gemm)      # None: the library default (env RN_WINO_GEMM, "split")

    if not os.path.exists(args.render_dir):
        os.makedirs(args.render_dir)
    light_dir = Phong_shading.generate_light_pos(args.light_elevation, args.light_azimuth)
    voxel_path = args.voxel_path
    reference_mesh = None
    if shape_id is not None:
        voxel, model_name = shape_voxels(shape_id, args.shape_seed), "shape%08x" % shape_id
    elif args.mesh_path is not None:
        try:
            voxel = mesh_voxels(args.mesh_path, args.mesh_mode, args.mesh_margin, args.mesh_axes)
        except ValueError as e:
            raise SystemExit("--mesh_path: %s" % e)
        model_name = os.path.splitext(os.path.basename(args.mesh_path))[0]
        if args.reference_mesh:
            from rendernet_amd import mesh
            try:
                reference_mesh = (mesh.MeshSet.from_files([args.mesh_path], S=64, margin=args.mesh_margin, axes=args.mesh_axes),
                                  not args.mesh_flat, args.mesh_cull)
            except ValueError as e:
                raise SystemExit("--reference_mesh: %s" % e)
    if shape_id is not None or args.mesh_path is not None:
        if args.save_binvox:
            binvox_rw.save_binvox(voxel[0, ..., 0] > 0.5, args.save_binvox)
            print(args.save_binvox)
    else:
        if not os.path.exists(voxel_path) and voxel_path == "./voxel/Misc/bunny.binvox":
            voxel_path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "binvox", "bunny.binvox")
        with open(voxel_path, 'rb') as f:
            voxel = np.reshape(binvox_rw.read_as_3d_array(f).data.astype(np.float32), (1, 64, 64, 64, 1))
        model_name = os.path.basename(voxel_path).split('.binvox')[0]
    if args.save_mesh is not None:
        from rendernet_amd import mesh
        q, faces = mesh.extract(voxel, threshold=0.5, smooth=not args.mesh_blocky, relax=args.mesh_relax, relax_weight=args.mesh_relax_weight,
                                merge=args.mesh_merge)
        mesh.save_mesh(args.save_mesh, q, faces)
        print("%s: %d vertices, %d quads" % (args.save_mesh, len(q), len(faces)))
    if args.weights and not args.no_winograd_check:
        # trained weights have statistics nobody has looked at: one render with the F(6x6,3x3) rounding guard on, on the object
        # and a pose of this very run; filters whose F(6x6,3x3) output strays from F(4x4,3x3) are demoted for the session
        demoted = renderer.validate_winograd(voxel, compute_pose_param(args.azimuth, args.elevation, args.radius), tol=2e-4)
        print("winograd check (tolerance 2e-4 of max|conv|): %s" % ("all F(6x6,3x3) layers kept" if not demoted else
              "%d layer(s) demoted to F(4x4,3x3): %s" % (len(demoted), demoted)))

    if args.rotate:
        # RenderNet_demo.py:130-137: 72 poses, 5 degrees apart, numbered 000..071 -- rendered `--batch` poses per launch
        az = list(np.arange(0.0, 360.0, 5.0))
        paths = []
        for s in range(0, len(az), args.batch):
            paths += render(az[s:s + args.batch], args.elevation, args.radius, renderer, voxel, light_dir, args.render_dir, s,
                            args.light_azimuth, args.light_elevation, model_name, args.reference_render, args.reference_ao,
               args.reference_lines, args.reference_shadow, reference_mesh)
        if args.gif:
            from PIL import Image
            frames = [Image.open(p).convert("P", palette=Image.ADAPTIVE) for p in paths]
            frames[0].save(args.gif, save_all=True, append_images=frames[1:], duration=60, loop=0)
            print(args.gif)
    else:
        render([args.azimuth], args.elevation, args.radius, renderer, voxel, light_dir, args.render_dir, 0,
               args.light_azimuth, args.light_elevation, model_name, args.reference_render, args.reference_ao,
               args.reference_lines, args.reference_shadow, reference_mesh)


if __name__ == "__main__":
    main()
