#!/usr/bin/env python
"""`python RenderNet_Shader.py <config.json>` -- the reference's Phong-shader script
(RenderNet_Shader.py) on the MI355X path, same JSON keys (config_RenderNet.json:1-17,
README.md:41-70).

Without `--train` the script builds the graph of RenderNet_Shader.py:135-156 (resample -> transform -> crop ->
RenderNet), loads weights from `<sample_save>/<trained_model_name>.npz` when present (else the seeded reference
initialisers), renders every binvox under `model_path` at the demo pose and writes PNGs to `sample_save`.

`--train` runs the reference's training loop (:193-306): epochs over the image tar (`image_path`, poses parsed from
the member names) + binvox folder (`model_path`), crop 32 for the first five epochs then 64 (:204-207), BCE (greyscale)
or MSE loss, Adam(beta1=0.5) with staircase-decayed learning rate, a sample PNG every 600 steps, weights saved as
`<sample_save>/<trained_model_name>.npz` after every epoch and every `checkpoint_secs` (weights + Adam moments +
global_step + epoch, written atomically; a restart resumes from it like the reference's Supervisor), then the
validation pass over `image_path_valid` (:257-301, dropout off).  Under `torch.distributed.run` every rank trains on its shard of each batch and the gradients are
summed with bucketed RCCL all-reduces (rendernet_amd/train.py).

`--train --prefetch N` (config key "prefetch_batches"; `--loader-workers W` / "loader_workers", default 4) feeds the same
batches in the same order through rendernet_amd/loader.py: PNG decode in W threads, uint8 frames through pinned memory with
N batches in flight, crop + mean + /255 on the device.  N = 0, the default, is the synchronous loader of the reference.

`--train --synthetic [--synthetic-steps K]` (config keys "synthetic_targets", "synthetic_steps_per_epoch", default 100) needs
no image set at all: every epoch is K batches of the binvox models under `model_path` at seeded random poses, the target of
each the exact normal map the device ray caster draws of the model at that pose (rendernet_amd/synth.py, rn_raycast_fwd;
greyscale: its Phong composite under the demo's light).  `image_path` is not read; the validation pass is the same L1 loop
over a fixed held-out pose set (seed + 1, two batches).  `--synthetic-shader {normal,phong,ao,outline,cel,shadow}` (config key "synthetic_shader")
names the picture: `normal` (colour) and `phong` (greyscale) are the defaults spelled out; `ao` is the ambient occlusion of the
grid (rn_raycast_ao_fwd; rays end after "synthetic_ao_distance" voxels, default 16); `outline` is the contour drawing of the
grid and `cel` the same contours over flat bands of the diffuse term under the demo's light (rn_raycast_edges_fwd,
rn_lines_encode; config keys "synthetic_line_radius" 1..4 pixels, "synthetic_depth_gap" 1..127 voxels, "synthetic_crease_q"
0..8 and "synthetic_cel_levels" 2..8, defaults 2, 2, 4, 4); `shadow` is the diffuse shading of the grid with the shadows it
casts on itself (rn_raycast_shadow_fwd, rn_shadow_encode; config keys "synthetic_shadow_bias" 0..3 voxels, default 1,
"synthetic_shadow_smooth" 0..8 pixels, default the 4 pixels of a cell, "synthetic_ambient_byte" 0..254, default 26, and
"synthetic_light", three numbers (right, up, towards the camera), default the demo's light).  These four come in either colour
mode, training and validation alike.  `--synthetic-shapes P` (config key "synthetic_shapes", default 0) makes each sample's grid,
with probability P in [0, 1], a procedural shape and not one of the models: a seeded union and subtraction of a few rotated
ellipsoids, boxes, cylinders, cones and tori, rasterised on the device (rendernet_amd/synth.py shape_prims, rn_voxel_shapes;
config key "synthetic_shape_seed", default the value of "synthetic_seed").  With P = 1 `model_path` is not read.  Such a sample
is named `shape<id>` in hex; `RenderNet_demo.py --voxel_shape <id>` renders that grid again.  `--synthetic-meshes DIR` (config
key "synthetic_meshes", off by default) adds the user's own models: every .obj / .ply under DIR is voxelised once at start, on
the device, at 64^3 (rendernet_amd/mesh.py, rn_mesh_voxelize: voxel centres inside the mesh plus every voxel a triangle touches)
and appended to the binvox models of `model_path`; the file stems are the model names, and a stem that holds one of the pose
tags `_p`, `_t`, `_r` is refused at start, since a sample name `<model>_p.._t.._r..` could not be read back.
`--synthetic-mesh-targets` (config key "synthetic_mesh_targets", off by default; needs `--synthetic-meshes`) makes the target
of such a sample the picture of the MESH, not of its voxelisation: the smooth normal map rasterised on the device under the
caster's camera (rendernet_amd/mesh.py MeshSet, rn_mesh_rasterize), which overlays the grid the net is fed pixel for pixel --
the reference's pairing of rendered meshes with their voxel grids.  Binvox and procedural samples keep the caster.  Shaders
normal and phong only (the others need voxel hits).  `--mesh_cull back|none` (config key "mesh_cull", default back) keeps or
drops triangles seen from inside; "none" is for meshes that are not closed or not wound consistently.

`--train --val-metrics` (config key "val_metrics", default off) adds PSNR and SSIM to the validation pass: after every
`Validation accuracy` line a line `Validation PSNR <dB> SSIM <value>`, the batch's means, computed on the device from the
prediction before it is copied to the host (rendernet_amd/metrics.py, rn_image_metrics: both images as bytes, the 11 x 11
Gaussian SSIM on integer moments).  The epoch means are kept as `psnr_all` and `ssim_all` beside `l1_all` in the checkpoint and
written to `<sample_save>/Metrics All.txt` (np.savez).  Without the flag no line, key or file is added.
"""
import glob
import json
import os
import sys
import time

import numpy as np


def load_config(path):
    with open(path, 'r') as fh:
        cfg = json.load(fh)
    for key in ('model_path', 'sample_save', 'trained_model_name', 'is_greyscale', 'batch_size', 'keep_prob'):
        if key not in cfg:
            raise KeyError("config is missing %r (see config_RenderNet.json)" % key)
    return cfg


def _save_png(path, arr01):
    from PIL import Image
    Image.fromarray(np.squeeze(np.clip(255 * arr01, 0, 255).astype(np.uint8))).save(path)


def prefetch_options(cfg, argv):
    """(prefetch_batches, loader_workers): `--prefetch N` / `--loader-workers W` on the command line win over the config
    keys "prefetch_batches" / "loader_workers".  N = 0 (the default) is the synchronous loader of the reference; N >= 1 is
    rendernet_amd.loader with N slots in flight."""
    def pick(flag, key, default):
        if flag in argv:
            if argv.index(flag) + 1 >= len(argv):
                raise SystemExit("%s needs a value" % flag)
            raw = argv[argv.index(flag) + 1]
        else:
            raw = cfg.get(key, default)
        try:
            if isinstance(raw, (bool, float)):
                raise ValueError(raw)
            return int(raw)
        except (TypeError, ValueError):
            raise SystemExit("%s / %r: %r is not an integer" % (flag, key, raw))
    prefetch, workers = pick("--prefetch", "prefetch_batches", 0), pick("--loader-workers", "loader_workers", 4)
    if not 0 <= prefetch <= 8:
        raise SystemExit("--prefetch %d: expected 0 (synchronous loader) or 1..8 batches in flight" % prefetch)
    if not 1 <= workers <= 16:
        raise SystemExit("--loader-workers %d: expected 1..16 decode threads" % workers)
    return prefetch, workers


def synthetic_options(cfg, argv):
    """(synthetic, steps_per_epoch): `--synthetic` on the command line or a true config key "synthetic_targets" turns the
    ray-cast targets on; `--synthetic-steps K` wins over the config key "synthetic_steps_per_epoch" (default 100)."""
    raw = cfg.get("synthetic_targets", False)
    if isinstance(raw, str):
        if raw.lower() not in ("true", "false"):
            raise SystemExit("\"synthetic_targets\": %r is neither true nor false" % raw)
        raw = raw.lower() == "true"
    elif not isinstance(raw, bool):
        raise SystemExit("\"synthetic_targets\": %r is neither true nor false" % (raw,))
    synthetic = raw or "--synthetic" in argv
    flag, key = "--synthetic-steps", "synthetic_steps_per_epoch"
    if flag in argv:
        if argv.index(flag) + 1 >= len(argv):
            raise SystemExit("%s needs a value" % flag)
        steps = argv[argv.index(flag) + 1]
    else:
        steps = cfg.get(key, 100)
    try:
        if isinstance(steps, (bool, float)):
            raise ValueError(steps)
        steps = int(steps)
    except (TypeError, ValueError):
        raise SystemExit("%s / %r: %r is not an integer" % (flag, key, steps))
    if steps < 1:
        raise SystemExit("%s %d: expected at least one batch per epoch" % (flag, steps))
    if flag in argv and not synthetic:
        raise SystemExit("%s needs --synthetic" % flag)
    return synthetic, steps


SYNTHETIC_SHADERS = ("normal", "phong", "ao")
SYNTHETIC_LINE_SHADERS = ("outline", "cel")
SYNTHETIC_SHADOW_SHADERS = ("shadow",)


def synthetic_shader_options(cfg, argv):
    """(shader, ao_distance): `--synthetic-shader NAME` on the command line wins over the config key "synthetic_shader";
    neither given: None, the default picture of the colour mode.  The config key "synthetic_ao_distance" (default 16) is
    the length of the ambient-occlusion rays in voxels, 1..32."""
    flag, key = "--synthetic-shader", "synthetic_shader"
    if flag in argv:
        if not synthetic_options(cfg, argv)[0]:
            raise SystemExit("%s needs --synthetic" % flag)
        if argv.index(flag) + 1 >= len(argv):
            raise SystemExit("%s needs a value" % flag)
        shader = argv[argv.index(flag) + 1]
    else:
        shader = cfg.get(key)
    names = SYNTHETIC_SHADERS + SYNTHETIC_LINE_SHADERS + SYNTHETIC_SHADOW_SHADERS
    if shader is not None and shader not in names:
        raise SystemExit("%s / %r: %r is not one of %s" % (flag, key, shader, ", ".join(names)))
    if shader in ("normal", "phong") and "is_greyscale" in cfg and (shader == "phong") != (cfg["is_greyscale"].lower() == "true"):
        raise SystemExit("%s %s: the normal map is the colour target and its Phong composite the greyscale one "
                         "(\"is_greyscale\": %r)" % (flag, shader, cfg["is_greyscale"]))
    dist = cfg.get("synthetic_ao_distance", 16)
    try:
        if isinstance(dist, (bool, float)):
            raise ValueError(dist)
        dist = int(dist)
    except (TypeError, ValueError):
        raise SystemExit("\"synthetic_ao_distance\": %r is not an integer" % (dist,))
    if not 1 <= dist <= 32:
        raise SystemExit("\"synthetic_ao_distance\": %d, expected 1..32 voxels" % dist)
    return shader, dist


def synthetic_shape_options(cfg, argv):
    """(shapes, shape_seed): `--synthetic-shapes P` on the command line wins over the config key "synthetic_shapes" (default
    0): the probability in [0, 1] that a sample's grid is a procedural shape.  The config key "synthetic_shape_seed" seeds the
    shapes, default the value of "synthetic_seed" (1234)."""
    flag, key = "--synthetic-shapes", "synthetic_shapes"
    given = flag in argv or key in cfg or "synthetic_shape_seed" in cfg
    if flag in argv:
        if argv.index(flag) + 1 >= len(argv):
            raise SystemExit("%s needs a value" % flag)
        raw = argv[argv.index(flag) + 1]
    else:
        raw = cfg.get(key, 0)
    try:
        if isinstance(raw, bool):
            raise ValueError(raw)
        shapes = float(raw)
    except (TypeError, ValueError):
        raise SystemExit("%s / %r: %r is not a number" % (flag, key, raw))
    if not 0.0 <= shapes <= 1.0:                                   # a NaN fails both comparisons
        raise SystemExit("%s / %r: %r, expected a probability in [0, 1]" % (flag, key, raw))
    seed = cfg.get("synthetic_shape_seed", cfg.get("synthetic_seed", 1234))
    try:
        if isinstance(seed, (bool, float)):
            raise ValueError(seed)
        seed = int(seed)
    except (TypeError, ValueError):
        raise SystemExit("\"synthetic_shape_seed\": %r is not an integer" % (seed,))
    if seed < 0:
        raise SystemExit("\"synthetic_shape_seed\": %d, expected a non-negative integer" % seed)
    if given and not synthetic_options(cfg, argv)[0]:
        raise SystemExit("%s needs --synthetic" % flag)
    return shapes, seed


# config key -> (line_options key of rendernet_amd.synth, lowest, highest, default, unit)
def synthetic_mesh_options(cfg, argv):
    """The folder of `--synthetic-meshes DIR` (it wins over the config key "synthetic_meshes"), or None: off by default."""
    flag, key = "--synthetic-meshes", "synthetic_meshes"
    if flag in argv:
        if argv.index(flag) + 1 >= len(argv):
            raise SystemExit("%s needs a value" % flag)
        path = argv[argv.index(flag) + 1]
    else:
        path = cfg.get(key)
    if path is None:
        return None
    if not isinstance(path, str) or not os.path.isdir(path):
        raise SystemExit("%s / %r: %r is not a folder" % (flag, key, path))
    if not synthetic_options(cfg, argv)[0]:
        raise SystemExit("%s needs --synthetic" % flag)
    return path


def synthetic_mesh_target_options(cfg, argv):
    """(mesh_targets, cull): `--synthetic-mesh-targets` or a true config key "synthetic_mesh_targets" (off by default) makes the
    target of a sample whose model came from `--synthetic-meshes` the rasterised normal map of the mesh itself
    (ops.rasterize_mesh), not the ray-cast picture of its voxelisation; `--mesh_cull back|none` (config key "mesh_cull",
    default back) is its culling.  Normal maps only: the shaders normal and phong."""
    flag, key = "--synthetic-mesh-targets", "synthetic_mesh_targets"
    raw = cfg.get(key, False)
    if isinstance(raw, str) and raw.strip().lower() in ("true", "false"):
        raw = raw.strip().lower() == "true"
    if not isinstance(raw, bool):
        raise SystemExit("\"%s\": %r is neither true nor false" % (key, raw))
    on = raw or flag in argv
    cflag, ckey = "--mesh_cull", "mesh_cull"
    if cflag in argv:
        if argv.index(cflag) + 1 >= len(argv):
            raise SystemExit("%s needs a value" % cflag)
        cull = argv[argv.index(cflag) + 1]
    else:
        cull = cfg.get(ckey, "back")
    if cull not in ("back", "none"):
        raise SystemExit("%s / \"%s\": %r, expected back or none" % (cflag, ckey, cull))
    if (cflag in argv or ckey in cfg) and not on:
        raise SystemExit("%s needs %s" % (cflag, flag))
    if on:
        if synthetic_mesh_options(cfg, argv) is None:
            raise SystemExit("%s needs --synthetic-meshes DIR: the targets are drawn from the meshes under it" % flag)
        shader = synthetic_shader_options(cfg, argv)[0]
        if shader not in (None, "normal", "phong"):
            raise SystemExit("%s draws normal maps: the shader %r needs voxel hits, which a mesh does not give; expected normal "
                             "or phong" % (flag, shader))
    return on, cull


def read_meshes(mesh_dir, device, taken=(), with_set=False):
    """Every .obj / .ply under `mesh_dir`, voxelised once on the device at 64^3 (rendernet_amd.mesh.voxelize, mode "both"):
    (uint8 [n,64,64,64,1] on the host, names), the names being the file stems in sorted file order.  A stem is refused when
    `extract_param_from_names` cannot read a pose back from `<stem>_p.._t.._r..` (it holds one of the pose tags), when it
    repeats, or when it is in `taken` (the binvox models' names).  `with_set` appends the fitted meshes themselves, a
    `mesh.MeshSet` on the device (the targets of --synthetic-mesh-targets)."""
    from rendernet_amd import mesh
    from rendernet_amd.tools.data_util import extract_param_from_names
    files = sorted(p for ext in ("obj", "ply", "OBJ", "PLY") for p in glob.glob(os.path.join(mesh_dir, "**", "*." + ext), recursive=True))
    if not files:
        raise SystemExit("--synthetic-meshes %s: no .obj or .ply file under it" % mesh_dir)
    grids, names = [], []
    for p in files:
        stem = os.path.splitext(os.path.basename(p))[0]
        probe = "%s_p123.45_t67.89_r3.3" % stem
        try:
            back = extract_param_from_names(probe)[0]
            want = extract_param_from_names("m_p123.45_t67.89_r3.3")[0]
            if not np.array_equal(back, want):
                raise ValueError(stem)
        except ValueError:
            raise SystemExit("--synthetic-meshes: %s: the name %r holds one of the pose tags _p / _t / _r, so the pose of a sample "
                             "`%s` cannot be read back; rename the file" % (p, stem, probe))
        if stem in names or stem in taken:
            raise SystemExit("--synthetic-meshes: %s: a model named %r is already in the set" % (p, stem))
        try:
            vox = mesh.voxelize(p, S=64, device=device)
        except ValueError as e:
            raise SystemExit("--synthetic-meshes: %s" % e)
        if not bool(vox.any()):
            raise SystemExit("--synthetic-meshes: %s: the grid is empty" % p)
        grids.append(vox[0].cpu().numpy())
        names.append(stem)
    print("synthetic meshes: %s" % ", ".join(names))
    if with_set:
        try:
            return np.stack(grids), names, mesh.MeshSet.from_files(files, S=64, device=device, names=names)
        except ValueError as e:
            raise SystemExit("--synthetic-mesh-targets: %s" % e)
    return np.stack(grids), names


SYNTHETIC_LINE_KEYS = (("synthetic_line_radius", "line_radius", 1, 4, 2, "pixels"),
                       ("synthetic_depth_gap", "depth_gap", 1, 127, 2, "voxels"),
                       ("synthetic_crease_q", "crease_q", 0, 8, 4, "eighths of cos^2 of the crease angle"),
                       ("synthetic_cel_levels", "levels", 2, 8, 4, "tones"))


def synthetic_line_options(cfg, argv):
    """The `line_options` of the outline and cel targets from the config keys "synthetic_line_radius" (default 2),
    "synthetic_depth_gap" (2), "synthetic_crease_q" (4) and "synthetic_cel_levels" (4): a dict for
    rendernet_amd.synth.SyntheticTargets.  They are checked whichever shader is chosen; there are no flags for them."""
    out = {}
    for key, name, lo, hi, default, unit in SYNTHETIC_LINE_KEYS:
        raw = cfg.get(key, default)
        try:
            if isinstance(raw, (bool, float)):
                raise ValueError(raw)
            val = int(raw)
        except (TypeError, ValueError):
            raise SystemExit("\"%s\": %r is not an integer" % (key, raw))
        if not lo <= val <= hi:
            raise SystemExit("\"%s\": %d, expected %d..%d %s" % (key, val, lo, hi, unit))
        out[name] = val
    return out


# config key -> (shadow_options key of rendernet_amd.synth, lowest, highest, unit); a missing key leaves the default to synth
SYNTHETIC_SHADOW_KEYS = (("synthetic_shadow_bias", "bias", 0, 3, "voxels"),
                         ("synthetic_shadow_smooth", "smooth", 0, 8, "pixels"),
                         ("synthetic_ambient_byte", "ambient_byte", 0, 254, "of 255"))


def synthetic_shadow_options(cfg, argv):
    """The `shadow_options` of the shadow targets from the config keys "synthetic_shadow_bias" (default 1),
    "synthetic_shadow_smooth" (default: the 4 pixels of a cell), "synthetic_ambient_byte" (26) and "synthetic_light" (three
    numbers: right, up, towards the camera; default the demo's light): a dict for rendernet_amd.synth.SyntheticTargets with
    the keys that were given.  They are checked whichever shader is chosen; there are no flags for them."""
    out = {}
    for key, name, lo, hi, unit in SYNTHETIC_SHADOW_KEYS:
        if key not in cfg:
            continue
        raw = cfg[key]
        try:
            if isinstance(raw, (bool, float)):
                raise ValueError(raw)
            val = int(raw)
        except (TypeError, ValueError):
            raise SystemExit("\"%s\": %r is not an integer" % (key, raw))
        if not lo <= val <= hi:
            raise SystemExit("\"%s\": %d, expected %d..%d %s" % (key, val, lo, hi, unit))
        out[name] = val
    if "synthetic_light" in cfg:
        raw = cfg["synthetic_light"]
        try:
            if isinstance(raw, str) or any(isinstance(c, (bool, str)) for c in raw):
                raise ValueError(raw)
            light = tuple(float(c) for c in raw)
            if len(light) != 3 or not np.isfinite(light).all() or not np.abs(light).max() > 0.0:
                raise ValueError(raw)
        except (TypeError, ValueError):
            raise SystemExit("\"synthetic_light\": %r is not three finite numbers (right, up, towards), not all zero" % (raw,))
        out["light"] = light
    return out


def _synthetic_batches(cfg, grey, rank, world, device, steps, seed, shader=None, ao_distance=16, line_options=None,
                       shadow_options=None, shapes=0.0, shape_seed=None, meshes=None, mesh_cull="back"):
    """`steps` batches of (voxels, poses, frames, names) from rendernet_amd.synth over every binvox under model_path and, with
    probability `shapes` per sample, procedural grids (shapes = 1: model_path is not read).  `meshes` (grids, names), what
    `read_meshes` returned, are appended to the model set; with a third entry, the MeshSet, the samples of those models get
    the rasterised mesh as their target."""
    from rendernet_amd import synth
    models, names = synth.read_models(cfg['model_path']) if shapes < 1.0 else (None, ())
    mesh_kw = {}
    if meshes is not None and shapes < 1.0:
        if len(meshes) > 2:
            mesh_kw = dict(mesh_set=meshes[2], mesh_models=[-1] * len(names) + list(range(len(meshes[1]))), mesh_cull=mesh_cull)
        models, names = np.concatenate([models, meshes[0]]), list(names) + list(meshes[1])
    for frames, vox, poses, batch_names in synth.SyntheticTargets(models, names, int(cfg['batch_size']), steps, seed, rank=rank,
                                                                  world=world, device=device, greyscale=grey, shader=shader,
                                                                  ao_distance=ao_distance, line_options=line_options,
                                                                  shadow_options=shadow_options, shapes=shapes,
                                                                  shape_seed=shape_seed, **mesh_kw):
        yield vox, poses, frames, batch_names


def _training_batches(cfg, grey, img_res, rank, world, device, prefetch, workers):
    """One epoch of (voxels, poses, frames, names) per optimiser step, this rank's shard of each batch.
    prefetch == 0: the reference's loader -- float32 NumPy frames already divided by 255 (:224), every rank decodes the
    chunk and slices.  prefetch >= 1: the same batches in the same order as uint8 device tensors, decoded by worker
    threads and copied while the previous step runs (rendernet_amd/loader.py); the trainer turns the bytes into the same
    float target on the device."""
    bs = int(cfg['batch_size'])
    if prefetch == 0:
        from rendernet_amd.parallel import shard_range
        from rendernet_amd.tools import data_util
        for images, models, params, names in data_util.data_loader(cfg, img_path=cfg['image_path'], model_path=cfg['model_path'],
                                                                   flatten=grey, validation_mode=False, img_res=img_res):
            images = images / 255.0                                                     # :224
            for idx in range(len(images) // bs):
                sl = slice(idx * bs, (idx + 1) * bs)
                lo, hi = shard_range(bs, rank, world)                                   # this rank's frames of the batch
                yield models[sl][lo:hi], params[sl][lo:hi], images[sl][lo:hi], names[sl][lo:hi]
        return
    from rendernet_amd import loader
    host = loader.iter_host_batches(cfg, cfg['image_path'], cfg['model_path'], flatten=grey, img_res=img_res, rank=rank,
                                    world=world, workers=workers)
    with loader.PrefetchLoader(host, device, depth=prefetch) as feed:
        for images, models, params, names in feed:
            yield models, params, images, names


def _validation_batches(cfg, grey, img_res, device, synthetic, seed, shader=None, ao_distance=16, line_options=None,
                        shadow_options=None, shapes=0.0, shape_seed=None, meshes=None, mesh_cull="back"):
    """(images in [0, 1] as float NumPy, voxels, poses, names) per validation batch: the tar `image_path_valid` (:258-301),
    or with --synthetic a fixed held-out pose set -- seed + 1, two batches, the same every epoch, procedural shapes with the
    training feed's probability."""
    if synthetic:
        for vox, poses, frames, names in _synthetic_batches(cfg, grey, 0, 1, device, 2, seed + 1, shader, ao_distance, line_options,
                                                            shadow_options, shapes, shape_seed, meshes, mesh_cull):
            frames = frames.cpu().numpy()
            yield (frames if grey else frames.astype(np.float32) / np.float32(255.0)), vox, poses, names
        return
    from rendernet_amd.tools.data_util import data_loader
    for images, models, params, names in data_loader(cfg, img_path=cfg['image_path_valid'], model_path=cfg['model_path'],
                                                     flatten=grey, validation_mode=True, img_res=img_res):
        yield images / 255.0, models, params, names


def train(cfg, argv):
    """RenderNet_Shader.py:193-306 on the MI355X training step."""
    import contextlib
    import random
    import torch
    import torch.distributed as dist
    from rendernet_amd.shader import ShaderSpec, init_shader_weights
    from rendernet_amd.metrics import ValidationMetrics, metrics_options
    from rendernet_amd.train import Trainer

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(cfg.get('gpu', 0)) if world == 1 else "0"))
    bs = int(cfg['batch_size'])
    prefetch, workers = prefetch_options(cfg, argv)                # refused before anything is allocated
    synthetic, synth_steps = synthetic_options(cfg, argv)
    synth_shader, ao_distance = synthetic_shader_options(cfg, argv)
    line_options = synthetic_line_options(cfg, argv)
    shadow_options = synthetic_shadow_options(cfg, argv)
    shapes, shape_seed = synthetic_shape_options(cfg, argv)
    mesh_dir = synthetic_mesh_options(cfg, argv)
    mesh_targets, mesh_cull = synthetic_mesh_target_options(cfg, argv)
    val_metrics = metrics_options(cfg, argv)
    synth_seed = int(cfg.get('synthetic_seed', 1234))
    if bs % world != 0:
        # an empty or short shard would leave its rank out of the bucket / loss all-reduces: rank 0 would block for ever
        raise SystemExit("batch_size %d is not a multiple of the %d ranks: every rank needs the same, non-empty shard of "
                         "each batch" % (bs, world))
    torch.cuda.set_device(local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        import datetime
        # generous collective timeout: rank 0 validates alone at the end of an epoch while the others wait at a barrier
        dist.init_process_group("nccl", rank=rank, world_size=world, timeout=datetime.timedelta(hours=6))
    grey = cfg['is_greyscale'].lower() == "true"
    meshes = None
    if mesh_dir is not None and shapes < 1.0:                      # voxelised once, here; every epoch's feed appends the same grids
        from rendernet_amd import synth
        meshes = read_meshes(mesh_dir, "cuda:%d" % local_rank, taken=synth.read_models(cfg['model_path'])[1], with_set=mesh_targets)
    spec = ShaderSpec(out_ch=1 if grey else 3).check()
    sample_save = cfg['sample_save']
    os.makedirs(sample_save, exist_ok=True)
    wpath = os.path.join(sample_save, cfg['trained_model_name'] + ".npz")
    tr = Trainer(spec, init_shader_weights(spec, seed=1234), device="cuda:%d" % local_rank, e_eta=cfg.get('e_eta', 1e-5),
                 decay_steps=cfg.get('decay_steps', 100000), keep_prob=cfg.get('keep_prob', 1.0))
    # resume like the reference's Supervisor (:171-185): weights, Adam moments, global_step and the epoch counter
    first_epoch = tr.load_checkpoint(dict(np.load(wpath))) if os.path.exists(wpath) else 0
    new_res = spec.new_size
    max_steps = int(argv[argv.index("--max-steps") + 1]) if "--max-steps" in argv else None
    ckpt_secs = float(cfg.get('checkpoint_secs', 7200))
    last_ckpt = time.time()
    l1_all = [float(v) for v in np.ravel(tr.checkpoint_extra.get("l1_all", []))]     # the validation history survives a restart
    psnr_all = [float(v) for v in np.ravel(tr.checkpoint_extra.get("psnr_all", []))]
    ssim_all = [float(v) for v in np.ravel(tr.checkpoint_extra.get("ssim_all", []))]

    def history():                                                                   # the checkpoint's extra
        return dict({"l1_all": l1_all}, psnr_all=psnr_all, ssim_all=ssim_all) if val_metrics else {"l1_all": l1_all}
    for epoch in range(first_epoch, int(cfg['max_epochs'])):
        patch = new_res // 4 if epoch < 5 else new_res // 2                           # :204-207
        source = _synthetic_batches(cfg, grey, rank, world, tr.device, synth_steps, [synth_seed, epoch], synth_shader,
                                    ao_distance, line_options, shadow_options, shapes, shape_seed, meshes, mesh_cull) if synthetic else \
            _training_batches(cfg, grey, 4 * new_res, rank, world, tr.device, prefetch, workers)
        with contextlib.closing(source) as batches:
            for models, params, images, names in batches:                               # this rank's frames of one batch
                # one crop window per batch, the same on every rank (tools/model_util.py:92)
                start = torch.randint(0, new_res - patch + 1, (2,), device="cuda")
                if world > 1:
                    dist.broadcast(start, src=0)
                loss = tr.step(models, params, images, patch_size=patch, start_point=start.tolist(), global_batch=bs)
                step = tr.global_step
                if rank == 0:
                    print("Step {0} Loss {1}".format(step, float(loss.item())))
                if rank == 0 and time.time() - last_ckpt >= ckpt_secs:                  # Supervisor(save_model_secs=checkpoint_secs)
                    tr.save_checkpoint(wpath, epoch, history())
                    last_ckpt = time.time()
                if step % 600 == 0 and rank == 0:                                       # :242-253
                    with torch.no_grad():
                        pred, (r, c, p, _) = tr.forward(models, params, patch, start.tolist())
                    i = random.randint(0, len(names) - 1)
                    if torch.is_tensor(images):                         # frames on the device (--prefetch, --synthetic)
                        tgt = tr._target_patch(images[i:i + 1], r, c, p, spec.out_ch)[0].cpu().numpy()
                    else:
                        tgt = images[i, 4 * r:4 * (r + p), 4 * c:4 * (c + p)]
                    _save_png(os.path.join(sample_save, "{0}_train_target_{1}_patch.png".format(names[i], step)), tgt)
                    _save_png(os.path.join(sample_save, "{0}_train_{1}_patch.png".format(names[i], step)),
                              pred[i].detach().cpu().numpy())
                if max_steps is not None and step >= max_steps:
                    break
        if rank == 0:
            tr.save_checkpoint(wpath, epoch + 1, history())                                        # :257 sess_saver.save (atomic)
            last_ckpt = time.time()
        # validation (:258-301): full-resolution render with is_training False (dropout off), mean absolute error; on
        # rank 0 while the other ranks wait at the barrier below (a generous timeout: torch's default is 10 min for nccl)
        if rank == 0 and (synthetic or (cfg.get('image_path_valid') and os.path.exists(cfg['image_path_valid']))):
            l1, cnt = 0.0, 0
            vm = ValidationMetrics() if val_metrics else None
            with torch.no_grad():
                for images, models, params, names in _validation_batches(cfg, grey, 4 * new_res, tr.device, synthetic, synth_seed, synth_shader,
                                                                         ao_distance, line_options, shadow_options, shapes,
                                                                         shape_seed, meshes, mesh_cull):
                    pred, _ = tr.forward(models, params, is_training=False)
                    if vm is not None:
                        vm.add(pred, images)
                    pred = pred.cpu().numpy()
                    if cnt % 600 == 0:
                        _save_png(os.path.join(sample_save, "VALID_{0}_target_{1}.png".format(names[0], epoch)), images[0])
                        _save_png(os.path.join(sample_save, "VALID_{0}_pred_{1}.png".format(names[0], epoch)), pred[0])
                    acc = float(np.mean(np.absolute(images - pred)))
                    print("Validation accuracy {0}".format(acc))
                    if vm is not None:
                        print(vm.line())
                    l1 += acc
                    cnt += 1
            if cnt:
                l1_all.append(l1 / cnt)
                np.savez(os.path.join(sample_save, "L1 All.txt"), l1_all)
                if vm is not None:
                    psnr, ssim = vm.epoch_means()
                    psnr_all.append(psnr)
                    ssim_all.append(ssim)
                    np.savez(os.path.join(sample_save, "Metrics All.txt"), psnr_all=psnr_all, ssim_all=ssim_all)
        if world > 1:
            dist.barrier()                      # nobody starts the next epoch's collectives while rank 0 validates
        if max_steps is not None and tr.global_step >= max_steps:
            break
    if world > 1:
        dist.destroy_process_group()


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if not argv:
        raise SystemExit("usage: python RenderNet_Shader.py <config.json> [--train [--max-steps N] [--prefetch N] [--loader-workers W] "
                         "[--synthetic [--synthetic-steps K] [--synthetic-shader normal|phong|ao|outline|cel|shadow] "
                         "[--synthetic-shapes P] [--synthetic-meshes DIR [--synthetic-mesh-targets [--mesh_cull back|none]]]] [--val-metrics]]")
    cfg = load_config(argv[0])
    if "--train" in argv:
        return train(cfg, argv)
    os.environ.setdefault("HIP_VISIBLE_DEVICES", "{0}".format(cfg.get('gpu', 0)))
    from PIL import Image
    from rendernet_amd.shader import Renderer, ShaderSpec, init_shader_weights
    from rendernet_amd.tools import binvox_rw

    grey = cfg['is_greyscale'].lower() == "true"                       # RenderNet_Shader.py:125
    spec = ShaderSpec(out_ch=1 if grey else 3).check()
    sample_save = cfg['sample_save']
    os.makedirs(sample_save, exist_ok=True)
    wpath = os.path.join(sample_save, cfg['trained_model_name'] + ".npz")
    if os.path.exists(wpath):
        weights = {k: v for k, v in np.load(wpath).items() if not k.startswith("__")}     # drop the optimiser state
    else:
        weights = init_shader_weights(spec, seed=1234)
    renderer = Renderer(spec, weights)

    files = sorted(glob.glob(os.path.join(cfg['model_path'], "*.binvox")))
    if not files:
        raise SystemExit("no .binvox files under model_path=%s" % cfg['model_path'])
    bs = int(cfg['batch_size'])
    for s in range(0, len(files), bs):
        chunk = files[s:s + bs]
        vox = []
        for p in chunk:
            with open(p, 'rb') as f:
                vox.append(binvox_rw.read_as_3d_array(f).data.astype(np.float32)[..., None])
        vox = np.stack(vox)
        poses = np.tile(np.array([[250 * np.pi / 180, 30 * np.pi / 180, 1.0]], np.float32), (len(chunk), 1))
        out = renderer.run("encoder/output:0", {"real_model_in:0": vox, "view_name:0": poses, "patch_size:0": 128,
                                                "is_training:0": False})
        for p, img in zip(chunk, out):
            name = os.path.basename(p).split('.binvox')[0]
            arr = np.clip(255 * img, 0, 255).astype(np.uint8)
            Image.fromarray(np.squeeze(arr)).save(os.path.join(sample_save, "VALID_%s_pred.png" % name))
            print("rendered", name, arr.shape)


if __name__ == "__main__":
    main()
