#!/usr/bin/env python
"""`python RenderNet_Texture_Face_Normal.py <config.json>` -- the reference's texture + normal face renderer
(RenderNet_Texture_Face_Normal.py; BASELINE configs[2]) on the MI355X path, same JSON keys
(config_RenderNet_texture.json:1-18): image_path, image_path_valid, normal_path, texture_path, model_path, gpu,
batch_size, max_epochs, batches_chunk, e_eta, keep_prob, decay_steps, trained_model_name, sample_save,
checkpoint_secs.

`--train` runs the reference's loop (:196-334): epochs over the image tar (poses, model and texture ids parsed from
the member names), crop new_res/4 for the first four epochs then new_res/2 (:226-229), loss = MSE(image) +
MSE(normal) (:182-183), Adam(beta1 = 0.5) with the staircase learning rate, sample PNGs every 600 steps
(`<name>_train_target_<step>_patch.png`, `..._target_normal_...`, `<name>_train_<step>_patch.png`,
`..._patch_normal.png`, :263-278), a checkpoint at the end of every epoch and every `checkpoint_secs`, then the
validation pass (:286-331: full-resolution render with dropout off, `VALID_<name>_{target,target_normal,pred,
pred_normal}_<epoch>.png`, mean absolute error appended to `L1 All.txt`).
`--train --synthetic [--synthetic-steps K]` (config keys "synthetic_targets", "synthetic_steps_per_epoch", default 100) needs
no face set: `image_path`, `normal_path` and `texture_path` are neither read nor required.  Every batch is drawn on the device
from the .binvox models under `model_path` at seeded random poses ("synthetic_seed", default 1234) with seeded random
texture codes (rendernet_amd/synth.py SyntheticTextureTargets): the normal target is the ray-cast normal map, the image target
the ray-cast albedo, a linear colour field over the voxel lattice weighted by the quantised code the net is fed
(rn_raycast_albedo_fwd; the field's own seed is "synthetic_colour_seed", default 1234; "synthetic_smooth" 0..8 pixels, default
4, is the radius of its masked mean).  Validation is the same L1 loop over a fixed held-out set (seed + 1, two batches).
Without `--train` it renders every `<id>.binvox` of `model_path` that has a texture code in `texture_path` at the
demo pose and writes `VALID_<id>_pred.png` / `VALID_<id>_pred_normal.png` (a model without a code, or a config without
`texture_path`, gets the zero code).
`--train --val-metrics` (config key "val_metrics", default off) adds PSNR and SSIM of both heads to the validation pass, computed
on the device from the predictions before they are copied to the host (rendernet_amd/metrics.py, rn_image_metrics): per batch a
line `Validation PSNR <dB> SSIM <value> | normal PSNR <dB> SSIM <value>`, the epoch means as `psnr_all`, `ssim_all`,
`normal_psnr_all` and `normal_ssim_all` beside `l1_all` in the checkpoint and in `<sample_save>/Metrics All.txt` (np.savez).
Without the flag no line, key or file is added.
Under `torch.distributed.run` the batch is sharded over the ranks (gradient all-reduce: rendernet_amd/train.py).
"""
import glob
import json
import os
import random
import shutil
import sys
import time

import numpy as np


def _save_png(path, arr01):
    from PIL import Image
    Image.fromarray(np.squeeze(np.clip(255 * arr01, 0, 255).astype(np.uint8))).save(path)


def load_config(path, argv=()):
    with open(path, 'r') as fh:
        cfg = json.load(fh)
    synthetic = synthetic_texture_options(cfg, argv)[0]
    for key in ('model_path', 'texture_path', 'sample_save', 'trained_model_name', 'batch_size', 'keep_prob'):
        if key not in cfg and not (synthetic and key == 'texture_path'):
            raise KeyError("config is missing %r (see config_RenderNet_texture.json)" % key)
    return cfg


def synthetic_texture_options(cfg, argv):
    """(synthetic, steps_per_epoch, seed, colour_seed, smooth): the first two are the shader script's `--synthetic
    [--synthetic-steps K]` / "synthetic_targets" / "synthetic_steps_per_epoch", parsed by its own function; then the config
    keys "synthetic_seed" (default 1234), "synthetic_colour_seed" (1234) and "synthetic_smooth" (0..8 pixels, default 4)."""
    from RenderNet_Shader import synthetic_options
    synthetic, steps = synthetic_options(cfg, argv)
    out = []
    for key, default in (("synthetic_seed", 1234), ("synthetic_colour_seed", 1234), ("synthetic_smooth", 4)):
        raw = cfg.get(key, default)
        try:
            if isinstance(raw, (bool, float)):
                raise ValueError(raw)
            out.append(int(raw))
        except (TypeError, ValueError):
            raise SystemExit("\"%s\": %r is not an integer" % (key, raw))
    if not 0 <= out[2] <= 8:
        raise SystemExit("\"synthetic_smooth\": %d, expected 0..8 pixels" % out[2])
    return synthetic, steps, out[0], out[1], out[2]


def _synthetic_batches(cfg, spec, rank, world, device, steps, seed, colour_seed, smooth):
    """`steps` batches of (images, normals, voxels, textures, poses, names) from rendernet_amd.synth over every binvox under
    model_path: this rank's shard of each, uint8 frames on the device."""
    from rendernet_amd import synth
    models, names = synth.read_models(cfg['model_path'])
    return synth.SyntheticTextureTargets(models, names, int(cfg['batch_size']), steps, seed, synth.ColourModel(colour_seed, spec.z_dim),
                                         rank=rank, world=world, device=device, new_size=spec.new_size, smooth=smooth)


def _training_batches(cfg, spec, rank, world, device, synthetic, synth_steps, seed, colour_seed, smooth):
    """One epoch of (images, normals, voxels, textures, poses, names) per optimiser step, this rank's shard of each batch: the
    reference's loader over the image tar -- float NumPy frames divided by 255 (:245-246), every rank decodes the chunk and
    slices -- or with --synthetic the ray-cast targets."""
    if synthetic:
        for batch in _synthetic_batches(cfg, spec, rank, world, device, synth_steps, seed, colour_seed, smooth):
            yield batch
        return
    from rendernet_amd.parallel import shard_range
    from rendernet_amd.tools.data_util import data_loader_image_texture_normal_face
    bs = int(cfg['batch_size'])
    lo, hi = shard_range(bs, rank, world)
    loader = data_loader_image_texture_normal_face(cfg, img_path=cfg['image_path'], model_path=cfg['model_path'],
                                                   normal_path=cfg['normal_path'], texture_path=cfg['texture_path'],
                                                   validation_mode=False, img_res=4 * spec.new_size)
    for images, normals, models, textures, params, names in loader:
        images, normals = images / 255.0, normals / 255.0                           # :245-246
        for idx in range(len(images) // bs):
            sl = slice(idx * bs + lo, idx * bs + hi)
            yield images[sl], normals[sl], models[sl], textures[sl], params[sl], names[sl]


def _validation_batches(cfg, spec, device, synthetic, seed, colour_seed, smooth):
    """(images, normals in [0, 1] as float NumPy, voxels, textures, poses, names) per validation batch: the tar
    `image_path_valid` (:287-331), or with --synthetic a fixed held-out set -- seed + 1, two batches, the same every epoch."""
    if synthetic:
        for images, normals, vox, tex, poses, names in _synthetic_batches(cfg, spec, 0, 1, device, 2, seed + 1, colour_seed, smooth):
            yield (images.cpu().numpy().astype(np.float32) / np.float32(255.0),
                   normals.cpu().numpy().astype(np.float32) / np.float32(255.0), vox, tex, poses, names)
        return
    from rendernet_amd.tools.data_util import data_loader_image_texture_normal_face
    loader = data_loader_image_texture_normal_face(cfg, img_path=cfg['image_path_valid'], model_path=cfg['model_path'],
                                                   normal_path=cfg['normal_path'], texture_path=cfg['texture_path'],
                                                   validation_mode=True, img_res=4 * spec.new_size, add_noise=False)
    for images, normals, models, textures, params, names in loader:
        yield images / 255.0, normals / 255.0, models, textures, params, names


def train(cfg, argv):
    import contextlib
    import torch
    import torch.distributed as dist
    from rendernet_amd.metrics import ValidationMetrics, metrics_options
    from rendernet_amd.texture import TextureSpec, init_texture_weights
    from rendernet_amd.train import TextureTrainer

    world = int(os.environ.get("WORLD_SIZE", "1"))
    rank = int(os.environ.get("RANK", "0"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(cfg.get('gpu', 0)) if world == 1 else "0"))
    bs = int(cfg['batch_size'])
    synthetic, synth_steps, synth_seed, colour_seed, synth_smooth = synthetic_texture_options(cfg, argv)   # refused before anything is allocated
    val_metrics = metrics_options(cfg, argv)
    if bs % world != 0:
        raise SystemExit("batch_size %d is not a multiple of the %d ranks: every rank needs the same, non-empty shard "
                         "(an empty shard would leave its rank out of the gradient all-reduce)" % (bs, world))
    torch.cuda.set_device(local_rank)
    if world > 1:
        os.environ.setdefault("MASTER_ADDR", "127.0.0.1")
        import datetime
        # generous collective timeout: rank 0 validates alone at the end of an epoch while the others wait at a barrier
        dist.init_process_group("nccl", rank=rank, world_size=world, timeout=datetime.timedelta(hours=6))
    spec = TextureSpec().check()
    sample_save = cfg['sample_save']
    os.makedirs(sample_save, exist_ok=True)
    if rank == 0:
        shutil.copyfile(argv[0], os.path.join(sample_save, 'config.json'))               # :218
    wpath = os.path.join(sample_save, cfg['trained_model_name'] + ".npz")
    tr = TextureTrainer(spec, init_texture_weights(spec, seed=1234), device="cuda:%d" % local_rank,
                        e_eta=cfg.get('e_eta', 1e-5), decay_steps=cfg.get('decay_steps', 100000), keep_prob=cfg.get('keep_prob', 1.0))
    first_epoch = tr.load_checkpoint(dict(np.load(wpath))) if os.path.exists(wpath) else 0
    new_res = spec.new_size
    max_steps = int(argv[argv.index("--max-steps") + 1]) if "--max-steps" in argv else None
    ckpt_secs = float(cfg.get('checkpoint_secs', 7200))
    last_ckpt = time.time()
    l1_all = [float(v) for v in np.ravel(tr.checkpoint_extra.get("l1_all", []))]     # the validation history survives a restart
    metric_keys = ("psnr_all", "ssim_all", "normal_psnr_all", "normal_ssim_all")
    metrics_all = {k: [float(v) for v in np.ravel(tr.checkpoint_extra.get(k, []))] for k in metric_keys}

    def history():                                                                   # the checkpoint's extra
        return dict({"l1_all": l1_all}, **metrics_all) if val_metrics else {"l1_all": l1_all}
    for epoch in range(first_epoch, int(cfg['max_epochs'])):
        patch = new_res // 4 if epoch < 4 else new_res // 2                            # :226-229
        source = _training_batches(cfg, spec, rank, world, tr.device, synthetic, synth_steps, [synth_seed, epoch], colour_seed,
                                   synth_smooth)
        with contextlib.closing(source) as batches:
            for images, normals, models, textures, params, names in batches:            # this rank's frames of one batch
                start = torch.randint(0, new_res - patch + 1, (2,), device="cuda")      # one window per batch, all ranks
                if world > 1:
                    dist.broadcast(start, src=0)
                loss = tr.step(models, textures, params, images, normals, patch_size=patch, start_point=start.tolist(),
                               global_batch=bs)
                step = tr.global_step
                if rank == 0:
                    print("Step {0} Loss {1}".format(step, float(loss.item())))
                if step % 600 == 0 and rank == 0:                                      # :263-278
                    with torch.no_grad():
                        img, nrm, (r, c, p, _) = tr.forward(models, textures, params, patch, start.tolist())
                    i = random.randint(0, len(names) - 1)
                    nm = names[i]
                    if torch.is_tensor(images):                         # frames on the device (--synthetic)
                        tgt_img = tr._target_patch(images[i:i + 1], r, c, p, 3)[0].cpu().numpy()
                        tgt_nrm = tr._target_patch(normals[i:i + 1], r, c, p, 3)[0].cpu().numpy()
                    else:
                        win = (slice(4 * r, 4 * (r + p)), slice(4 * c, 4 * (c + p)))
                        tgt_img, tgt_nrm = images[i][win], normals[i][win]
                    _save_png(os.path.join(sample_save, "{0}_train_target_{1}_patch.png".format(nm, step)), tgt_img)
                    _save_png(os.path.join(sample_save, "{0}_train_target_normal_{1}_patch.png".format(nm, step)), tgt_nrm)
                    _save_png(os.path.join(sample_save, "{0}_train_{1}_patch.png".format(nm, step)), img[i].cpu().numpy())
                    _save_png(os.path.join(sample_save, "{0}_train_{1}_patch_normal.png".format(nm, step)), nrm[i].cpu().numpy())
                if rank == 0 and time.time() - last_ckpt >= ckpt_secs:                  # Supervisor(save_model_secs=checkpoint_secs)
                    tr.save_checkpoint(wpath, epoch, history())
                    last_ckpt = time.time()
                if max_steps is not None and step >= max_steps:
                    break
        if rank == 0:
            tr.save_checkpoint(wpath, epoch + 1, history())                                        # :285 sess_saver.save
            last_ckpt = time.time()
        # validation (:287-331), on rank 0 while the others wait at the barrier below
        if rank == 0 and (synthetic or (cfg.get('image_path_valid') and os.path.exists(cfg['image_path_valid']))):
            l1, cnt = 0.0, 0
            vm_img, vm_nrm = (ValidationMetrics(), ValidationMetrics()) if val_metrics else (None, None)
            with torch.no_grad():
                for images, normals, models, textures, params, names in _validation_batches(cfg, spec, tr.device, synthetic, synth_seed,
                                                                                            colour_seed, synth_smooth):
                    img, nrm, _ = tr.forward(models, textures, params, is_training=False)
                    if val_metrics:
                        vm_img.add(img, images)
                        vm_nrm.add(nrm, normals)
                        print(vm_img.line() + " | " + vm_nrm.line(prefix="normal "))
                    img, nrm = img.cpu().numpy(), nrm.cpu().numpy()
                    if cnt % 600 == 0:
                        i = random.randint(0, len(names) - 1)
                        _save_png(os.path.join(sample_save, "VALID_{0}_target_{1}.png".format(names[i], epoch)), images[i])
                        _save_png(os.path.join(sample_save, "VALID_{0}_target_normal_{1}.png".format(names[i], epoch)), normals[i])
                        _save_png(os.path.join(sample_save, "VALID_{0}_pred_{1}.png".format(names[i], epoch)), img[i])
                        _save_png(os.path.join(sample_save, "VALID_{0}_pred_normal_{1}.png".format(names[i], epoch)), nrm[i])
                    l1 += float(np.mean(np.absolute(images - img)))
                    cnt += 1
            if cnt:
                l1_all.append(l1 / cnt)
                np.savez(os.path.join(sample_save, "L1 All.txt"), l1_all)
                if val_metrics:
                    for k, v in zip(metric_keys, vm_img.epoch_means() + vm_nrm.epoch_means()):
                        metrics_all[k].append(v)
                    np.savez(os.path.join(sample_save, "Metrics All.txt"), **metrics_all)
        if world > 1:
            dist.barrier()                      # nobody starts the next epoch's collectives while rank 0 validates
        if max_steps is not None and tr.global_step >= max_steps:
            break
    if world > 1:
        dist.destroy_process_group()


def main(argv=None):
    argv = sys.argv[1:] if argv is None else argv
    if not argv:
        raise SystemExit("usage: python RenderNet_Texture_Face_Normal.py <config.json> [--train [--max-steps N] "
                         "[--synthetic [--synthetic-steps K]] [--val-metrics]]")
    cfg = load_config(argv[0], argv)
    if "--train" in argv:
        return train(cfg, argv)
    os.environ.setdefault("HIP_VISIBLE_DEVICES", "{0}".format(cfg.get('gpu', 0)))
    from rendernet_amd.texture import TextureRenderer, TextureSpec, init_texture_weights
    from rendernet_amd.tools import binvox_rw
    from rendernet_amd.tools.data_util import _read_texture_code

    spec = TextureSpec().check()
    sample_save = cfg['sample_save']
    os.makedirs(sample_save, exist_ok=True)
    wpath = os.path.join(sample_save, cfg['trained_model_name'] + ".npz")
    if os.path.exists(wpath):
        weights = {k: v for k, v in np.load(wpath).items() if not k.startswith("__")}
    else:
        weights = init_texture_weights(spec, seed=1234)
    renderer = TextureRenderer(spec, weights)
    files = sorted(glob.glob(os.path.join(cfg['model_path'], "*.binvox")))
    if not files:
        raise SystemExit("no .binvox files under model_path=%s" % cfg['model_path'])
    bs = int(cfg['batch_size'])
    for s in range(0, len(files), bs):
        chunk = files[s:s + bs]
        vox, tex, names = [], [], []
        for p in chunk:
            name = os.path.basename(p).split('.binvox')[0]
            try:
                if 'texture_path' not in cfg:                            # a config for --synthetic: no codes on disk
                    raise OSError("no texture_path")
                code = _read_texture_code(cfg['texture_path'], name.split('ly')[1] if 'ly' in name else name)
            except (OSError, IndexError):
                code = np.zeros(199, np.float32)
            with open(p, 'rb') as f:
                vox.append(binvox_rw.read_as_3d_array(f).data.astype(np.float32)[..., None])
            tex.append(code)
            names.append(name)
        poses = np.tile(np.array([[250 * np.pi / 180, 30 * np.pi / 180, 1.0]], np.float32), (len(chunk), 1))
        img, nrm = renderer.render(np.stack(vox), np.stack(tex), poses)
        for name, a, b in zip(names, img.cpu().numpy(), nrm.cpu().numpy()):
            _save_png(os.path.join(sample_save, "VALID_%s_pred.png" % name), a)
            _save_png(os.path.join(sample_save, "VALID_%s_pred_normal.png" % name), b)
            print("rendered", name, a.shape)


if __name__ == "__main__":
    main()
