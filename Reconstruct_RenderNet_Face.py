#!/usr/bin/env python
"""`python Reconstruct_RenderNet_Face.py <config.json>` -- the reference's inverse-rendering script
(Reconstruct_RenderNet_Face.py) on the MI355X path, same JSON keys (config_reconstruction_RenderNet.json:1-23).

Reads the target albedo / normal PNGs, shades the target with the NumPy Phong composite at the ground-truth light
(:430-444), then runs the coarse-to-fine latent search of :446-546: `max_epochs` rounds of five pose hypotheses, each
optimised for `inner_step` gradient steps on (shape code, pose, texture code, light azimuth) through the frozen
decoders + renderer (`rendernet_amd.reconstruct.Reconstructor`).  Every 100 steps and at the end the composite JPGs,
the thresholded voxel grids (.binvox), the raw volumes and texture codes (.npz) are written to `sample_save` with the
reference's file names (:508-520).  An addition: with the config key `"save_mesh": true` (default off) each `.binvox` also
gets a `<name>.ply` beside it, the surface-net mesh of the soft volume at the config's threshold, extracted on the device
(rendernet_amd.ops.extract_mesh); voxelised again in `solid` mode it is the `.binvox` grid voxel for voxel; the key
`"mesh_relax": N` (default 0) adds N passes of surface-net relaxation to every `.ply`, the `_clean` one included (4 is the
recommended setting: rn_mesh_relax).  With the key
`"target_shape": "<path>"` (a .binvox, an .npz volume or an .obj / .ply mesh of the decoder's grid size; absent by default) every
dump also scores each hypothesis' thresholded volume against that shape on the device (rendernet_amd.ops.voxel_shape_metrics):
a `<name> Shape IoU <v> chamfer <v> hausdorff <v> F <v>` line per hypothesis, and `shape_metrics.json` in `sample_save` with
`{name: {...}}` for every dump so far.  `"shape_tau"` (default 1.0 voxel) is the F-score's distance and
`"target_shape_threshold"` (default 0.5) the target's threshold.  With `"align_shape": R` beside it (absent by default) each
hypothesis is also registered to the target first (rendernet_amd.ops.voxel_align: the rotation by quarter turns out of
`"align_orientations"`, default "rotations", and the shift of up to R voxels per axis that overlap most) and scored again: a
`<name> Shape aligned o <o> t <tz,ty,tx> IoU <v> ...` line, and the keys `align_orientation`, `align_shift` and `aligned` in
`shape_metrics.json`.  With the key `"clean_shape": true` (default off) every dump also
cleans each thresholded volume on the device (rendernet_amd.ops.voxel_clean: the largest component of at least
`"clean_min_voxels"` voxels, default 1, its cavities filled) and writes `<name>_clean.binvox`, with `save_mesh` also
`<name>_clean.ply`, extracted from the cleaned grid; it logs `<name> Topology components <k> cavities <c> handles <h>` per
hypothesis for the raw thresholded volume (rendernet_amd.ops.voxel_topology), writes `topology.json`, and with `target_shape`
adds a second score line for the cleaned volume, prefixed `Shape(clean)`.

Weights: `weight_dir` / `weight_dir_decoder` are folders of `<tensor>.txt.npz` files (tools/model_util.py:26-39).  The
reference does not ship them; when a folder is missing the seeded initialisers are used and the script says so.
"""
import json
import math
import os
import shutil
import sys

import numpy as np


def _read_png(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"), np.float32)[None] / 255.0


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if not argv:
        raise SystemExit("usage: python Reconstruct_RenderNet_Face.py <config.json> [--max-steps N]")
    with open(argv[0], 'r') as fh:
        cfg = json.load(fh)
    for key in ('target_albedo', 'target_normal', 'target_azimuth_light', 'target_elevation_light', 'batch_size', 'z_dim',
                'inner_step', 'max_epochs', 'shape_eta', 'pose_eta', 'tex_eta', 'light_eta', 'sample_save'):
        if key not in cfg:
            raise KeyError("config is missing %r (see config_reconstruction_RenderNet.json)" % key)
    os.environ.setdefault("HIP_VISIBLE_DEVICES", "{0}".format(cfg.get('gpu', 0)))
    import torch
    from PIL import Image
    from rendernet_amd import reconstruct as RC
    from rendernet_amd.tools import binvox_rw

    sample_save = cfg['sample_save']
    os.makedirs(sample_save, exist_ok=True)
    shutil.copyfile(argv[0], os.path.join(sample_save, 'config.json'))                       # :421
    max_steps = int(argv[argv.index("--max-steps") + 1]) if "--max-steps" in argv else None

    dec_spec = RC.ShapeDecoderSpec(z_dim=int(cfg['z_dim']))
    weight_dict_MLP = weight_dict_decoder = None
    wd, wdd = cfg.get('weight_dir', ''), cfg.get('weight_dir_decoder', '')
    if os.path.isdir(wd) and os.path.isdir(wdd):
        weight_dict_MLP, weight_dict_decoder = RC.load_weights(wd), RC.load_weights(wdd)      # :337-339, by the reference's keys
    else:
        print("weight_dir / weight_dir_decoder not found: using seeded random weights (the reference ships no trained model)")
    ambient_in, k_diffuse, light_col = 0.0, 1.0, (1.0, 1.0, 1.0)                             # :323-325
    rec = RC.Reconstructor(dec_spec=dec_spec, weight_dict_rendernet=weight_dict_MLP, weight_dict_decoder=weight_dict_decoder,
                           batch_size=int(cfg['batch_size']),
                           light_elevation_deg=float(cfg['target_elevation_light']), light_col=light_col,
                           ambient=ambient_in, k_diffuse=k_diffuse, shape_eta=cfg['shape_eta'], pose_eta=cfg['pose_eta'],
                           tex_eta=cfg['tex_eta'], light_eta=cfg['light_eta'])

    target = _read_png(cfg['target_albedo'])                                                 # :430-431
    target_normal = _read_png(cfg['target_normal'])
    res = 4 * rec.tex_spec.new_size
    if target.shape[1:3] != (res, res) or target_normal.shape != target.shape:
        raise SystemExit("targets must be %dx%d RGB images" % (res, res))
    target_compos, target_shading = RC.shaded_target(target, target_normal, float(cfg['target_azimuth_light']),
                                                     float(cfg['target_elevation_light']), light_col, ambient_in, k_diffuse)
    to_u8 = lambda a: np.clip(a * 255., 0, 255).astype(np.uint8)
    Image.fromarray(to_u8(target_compos[0])).save(os.path.join(sample_save, "shaded_target.png"))       # :444-445
    Image.fromarray(to_u8(target_shading[0])).save(os.path.join(sample_save, "shading.png"))

    B, S = rec.B, rec.tex_spec.size
    save_mesh = bool(cfg.get('save_mesh', False))
    if save_mesh and S not in (32, 64, 128):
        raise SystemExit("save_mesh: the mesh extractor takes grids of 32, 64 or 128, not %d" % S)
    mesh_relax = int(cfg.get('mesh_relax', 0))
    if not 0 <= mesh_relax <= 64:
        raise SystemExit("mesh_relax: %d passes (0..64)" % mesh_relax)
    clean_shape, topology_rows = bool(cfg.get('clean_shape', False)), {}
    if clean_shape and S not in (32, 64, 128):
        raise SystemExit("clean_shape: the labelling takes grids of 32, 64 or 128, not %d" % S)
    shape_target, shape_scores = None, {}
    if cfg.get('target_shape'):                                                              # the ground-truth shape, when there is one
        from rendernet_amd import mesh
        from rendernet_amd.tools import compare_voxels
        path = cfg['target_shape']
        try:
            if compare_voxels._is_mesh(path):
                if S not in mesh.SIZES:
                    raise ValueError("the voxeliser takes grids of 32, 64 or 128, not %d" % S)
                shape_target = mesh.voxelize(path, S=S, mode="both")[..., 0]
            else:
                from rendernet_amd.tools.binvox_to_mesh import load_grid
                shape_target = torch.from_numpy(np.ascontiguousarray(load_grid(path))).cuda()[None]
        except (ValueError, OSError) as e:
            raise SystemExit("target_shape: %s" % e)
        if tuple(shape_target.shape) != (1, S, S, S):
            raise SystemExit("target_shape: %s is a grid of %s, the decoder's is %d^3"
                             % (os.path.basename(path), "x".join(str(int(v)) for v in shape_target.shape[1:]), S))
        shape_target = shape_target.expand(B, S, S, S)
    align_shape = cfg.get('align_shape')                                                     # None: score the frame as it is
    if align_shape is not None:
        if shape_target is None:
            raise SystemExit("align_shape: needs a target_shape to align to")
        if isinstance(align_shape, bool) or not isinstance(align_shape, int) or not 0 <= align_shape <= 16:
            raise SystemExit("align_shape: %r (the largest shift per axis in voxels, an integer 0..16)" % (align_shape,))
        if S not in (32, 64, 128):
            raise SystemExit("align_shape: the registration takes grids of 32, 64 or 128, not %d" % S)
    tgt = torch.as_tensor(np.tile(target_compos, (B, 1, 1, 1)), dtype=torch.float32).cuda()
    state = {"step": 0}

    def dump(loss):
        """:497-520: composites, voxels, texture codes of all hypotheses."""
        with torch.no_grad():
            compos, _, _, shape = rec.forward()
        vals = rec.values()
        img, vox = to_u8(compos.cpu().numpy()), shape.cpu().numpy()
        names = []
        for i in range(B):
            name = "{0}_{1}_p{2:.1f}_t_{3:.1f}_los_{4:.5f}".format(i, state["step"], int(vals["param"][i][0] * 180 / math.pi),
                                                                    int(90 - vals["param"][i][1] * 180 / math.pi), loss[i])
            Image.fromarray(img[i]).save(os.path.join(sample_save, name + ".jpg"))
            binvox_rw.save_binvox(vox[i].reshape(S, S, S) > cfg.get('threshold', 0.1), os.path.join(sample_save, name + ".binvox"))
            np.savez(os.path.join(sample_save, name + "_Param.txt"), vox[i].reshape(S, S, S))
            np.savez(os.path.join(sample_save, name + "_TEX.txt"), vals["texture"][i])
            names.append(name)
        if save_mesh:                                                                        # one extraction for all hypotheses
            from rendernet_amd import mesh
            mesh.save_meshes([os.path.join(sample_save, name + ".ply") for name in names], shape.detach().reshape(B, S, S, S),
                             threshold=float(cfg.get('threshold', 0.1)), relax=mesh_relax)
        if shape_target is not None:                                                         # one batched call for all hypotheses
            from rendernet_amd import metrics, ops
            rows = ops.voxel_shape_metrics(shape.detach().reshape(B, S, S, S), shape_target, tau=float(cfg.get('shape_tau', 1.0)),
                                           threshold=(float(cfg.get('threshold', 0.1)), float(cfg.get('target_shape_threshold', 0.5)))
                                           ).as_dicts()
            for name, row in zip(names, rows):
                print(metrics.shape_line(row, prefix=name + " "))
                shape_scores[name] = row
            if align_shape is not None:                                                      # the shape, not the frame: register, then score
                soft, thr = shape.detach().reshape(B, S, S, S), float(cfg.get('threshold', 0.1))
                found = ops.voxel_align(soft, shape_target, max_shift=align_shape, orientations=str(cfg.get('align_orientations', 'rotations')),
                                        threshold=(thr, float(cfg.get('target_shape_threshold', 0.5))))
                moved = found.apply((soft > thr).to(torch.uint8))
                rows = ops.voxel_shape_metrics(moved, shape_target, tau=float(cfg.get('shape_tau', 1.0)),
                                               threshold=(0.5, float(cfg.get('target_shape_threshold', 0.5)))).as_dicts()
                for name, how, row in zip(names, found.as_dicts(), rows):
                    o, t = how["orientation"], how["shift"]
                    print(metrics.shape_line(row, prefix=name + " ").replace(
                        " Shape IoU ", " Shape aligned o %d t %d,%d,%d IoU " % (o, t[0], t[1], t[2]), 1))
                    shape_scores[name] = dict(shape_scores[name], align_orientation=o, align_shift=t, aligned=row)
            with open(os.path.join(sample_save, "shape_metrics.json"), "w") as fh:
                json.dump(shape_scores, fh, indent=1)
        if clean_shape:                                                                      # the floaters and bubbles of the threshold
            from rendernet_amd import metrics, ops
            soft, thr = shape.detach().reshape(B, S, S, S), float(cfg.get('threshold', 0.1))
            cleaned = ops.voxel_clean(soft, thr, min_voxels=int(cfg.get('clean_min_voxels', 1)))
            host = cleaned[..., 0].cpu().numpy()
            for name, row, grid in zip(names, ops.voxel_topology(soft, thr).as_dicts(), host):
                print("{0} Topology components {1} cavities {2} handles {3}".format(name, row["components"], row["cavities"], row["handles"]))
                topology_rows[name] = row
                binvox_rw.save_binvox(grid > 0, os.path.join(sample_save, name + "_clean.binvox"))
            with open(os.path.join(sample_save, "topology.json"), "w") as fh:
                json.dump(topology_rows, fh, indent=1)
            if save_mesh:
                from rendernet_amd import mesh
                mesh.save_meshes([os.path.join(sample_save, name + "_clean.ply") for name in names], cleaned[..., 0], relax=mesh_relax)
            if shape_target is not None:
                rows = ops.voxel_shape_metrics(cleaned, shape_target, tau=float(cfg.get('shape_tau', 1.0)),
                                               threshold=(0.5, float(cfg.get('target_shape_threshold', 0.5)))).as_dicts()
                for name, row in zip(names, rows):
                    print(metrics.shape_line(row, prefix=name + " ").replace(" Shape IoU ", " Shape(clean) IoU ", 1))

    # the search of rendernet_amd.reconstruct.reconstruct, unrolled here for the periodic dumps and the step cap
    phi_range, theta_range, best = 60.0, 30.0, None
    for epoch in range(int(cfg['max_epochs'])):
        if epoch == 0:                                                                       # :456-461
            params = RC.create_param_center(B, phi_mid=270, phi_range=phi_range, theta_mid=90, theta_range=theta_range)
            rec.assign(vector=np.full((B, dec_spec.z_dim), 0.5, np.float32), param=params,
                       texture=np.random.randn(B, rec.tex_spec.z_dim).astype(np.float32),
                       light=(np.linspace(230, 320, num=B) * math.pi / 180.0)[:, None])
        else:                                                                                # :463-473
            phi_range /= 2
            theta_range /= 2
            params = RC.create_param_center(B, phi_mid=best["param_deg"][0], phi_range=phi_range,
                                            theta_mid=best["param_deg"][1], theta_range=theta_range)
            rec.assign(vector=np.tile(best["vector"][None], (B, 1)), param=params,
                       texture=np.tile(best["texture"][None], (B, 1)), light=np.tile(best["light"][None], (B, 1)))
        for _ in range(int(cfg['inner_step'])):
            loss = rec.step(tgt).cpu().numpy()
            state["step"] += 1
            print("{0} {1}".format(state["step"], loss))
            if state["step"] % 100 == 0:
                dump(loss)
            if max_steps is not None and state["step"] >= max_steps:
                break
        with torch.no_grad():                                                                # :523-541
            final = rec.recon_loss(rec.forward()[0], tgt).cpu().numpy()
        vals = rec.values()
        i = int(np.argmin(final))
        deg = vals["param"][i] * 180.0 / math.pi
        best = {"vector": vals["vector"][i], "texture": vals["texture"][i], "light": vals["light"][i],
                "param_deg": np.array([deg[0], 90 - deg[1], 1.0])}
        np.savez(os.path.join(sample_save, "{0}_loss_.txt".format(state["step"])), final)
        print("BEST LOSS " + str(i))
        print("BEST PARAM " + str(best["param_deg"]))
        if max_steps is not None and state["step"] >= max_steps:
            dump(final)
            break


if __name__ == "__main__":
    main()
