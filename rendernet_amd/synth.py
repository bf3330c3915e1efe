"""Synthetic training targets: the loader's batches without an image set.

The reference trained on normal maps that an offline renderer drew of each model at the pose named in the file name.  For
an occupancy grid that picture is computed on the device (`ops.raycast_normals`, rn_raycast_fwd), so `SyntheticTargets`
yields what `loader.PrefetchLoader` yields -- (frames, voxels, poses, names), device tensors -- from the binvox models
alone, at seeded random poses.  `shader="ao"` makes the frames the grid's ambient occlusion instead (`ops.raycast_ao`,
rn_raycast_ao_fwd): a shading that is not a function of the normal at the hit point alone.  `shader="outline"` and
`shader="cel"` are the two line drawings (`ops.raycast_outline`, `ops.raycast_cel`; rn_raycast_edges_fwd, rn_lines_encode):
contours where the hits of neighbouring pixels differ, alone or over flat bands of the diffuse term.  `shader="shadow"` is
the diffuse shading under a directional light WITH cast shadows (`ops.raycast_shadow`; rn_raycast_shadow_fwd,
rn_shadow_encode): the one picture here that depends on occupancy far from the hit and on the light direction.

`SyntheticTextureTargets` does the same for the texture + normal net (train.TextureTrainer), whose loop consumes (images,
normals, voxels, textures, poses, names): the normal head's target is the same normal map, the image head's target an albedo
picture that is a deterministic function of the texture code the net is fed (`ColourModel`, `ops.raycast_albedo`;
rn_raycast_albedo_fwd, rn_albedo_encode) -- a seeded linear colour field over the voxel lattice, as a morphable face model's
albedo is linear in its code.

Poses.  One seeded `numpy.random.Generator` on the host draws, per sample, the model, the azimuth in [0, 360), the file
elevation t in [10, 170] (degrees from the up axis, as the reference's file names carry it) and the radius in [2.5, 4.5].
The draw is formatted into the name `<model>_p<az>_t<t>_r<rad>` the reference's image files have, and the pose the net is
fed is what `tools.data_util.extract_param_from_names` reads back from that name -- so the sample PNGs written under these
names and any later parse of them agree with the yielded poses exactly (the parser reads three characters of the
radius, hence one decimal).  Every rank draws the whole batch and keeps `parallel.shard_range(batch_size, rank, world)`.
"""
import numpy as np

from .tools import data_util

# the demo's shading (RenderNet_demo.py:17-20 and its --light_* defaults)
AMBIENT_IN, K_DIFFUSE, LIGHT_ELEVATION, LIGHT_AZIMUTH = 0.1, 0.9, 60.0, 250.0


def _cast(vox, poses, new_size, pixels_per_cell):
    """The caster behind SyntheticTargets (a module attribute so that host-only tests can replace it)."""
    from . import ops
    return ops.raycast_normals(vox, poses, new_size=new_size, pixels_per_cell=pixels_per_cell)


def _cast_ao(vox, poses, new_size, pixels_per_cell, max_distance):
    """The ambient-occlusion caster behind SyntheticTargets(shader="ao") (a module attribute, like `_cast`)."""
    from . import ops
    return ops.raycast_ao(vox, poses, new_size=new_size, pixels_per_cell=pixels_per_cell, max_distance=max_distance)


def _cast_lines(vox, poses, new_size, pixels_per_cell, shader, options):
    """The line-drawing caster behind SyntheticTargets(shader="outline" | "cel") (a module attribute, like `_cast`):
    `options` is the validated `line_options` dict; "outline" ignores the cel-only keys (light, levels, shadow_byte)."""
    from . import ops
    if shader == "cel":
        return ops.raycast_cel(vox, poses, new_size=new_size, pixels_per_cell=pixels_per_cell, **options)
    options = {k: v for k, v in options.items() if k not in CEL_ONLY_OPTIONS}
    return ops.raycast_outline(vox, poses, new_size=new_size, pixels_per_cell=pixels_per_cell, **options)


def _cast_shadow(vox, poses, new_size, pixels_per_cell, options):
    """The cast-shadow caster behind SyntheticTargets(shader="shadow") (a module attribute, like `_cast`): `options` is the
    validated `shadow_options` dict."""
    from . import ops
    return ops.raycast_shadow(vox, poses, new_size=new_size, pixels_per_cell=pixels_per_cell, **options)


def _cast_albedo(vox, poses, waves, code_q, base, new_size, pixels_per_cell, smooth):
    """The caster behind SyntheticTextureTargets (a module attribute, like `_cast`): (albedo, normals), uint8 [b,H,W,3] each."""
    from . import ops
    return ops.raycast_albedo(vox, poses, waves, code_q, base, new_size=new_size, pixels_per_cell=pixels_per_cell, smooth=smooth)


SHADERS = ("normal", "phong", "ao")
LINE_SHADERS = ("outline", "cel")
SHADOW_SHADERS = ("shadow",)
CEL_ONLY_OPTIONS = ("light", "levels", "shadow_byte")


def check_line_options(line_options):
    """`line_options` of SyntheticTargets -> a dict ready for ops.raycast_outline / raycast_cel: integer keys of
    ops.LINE_RANGES within their ranges (levels 2..8 here: without bands the picture is "outline") and "light", three
    finite components that are not all zero.  Raises ValueError."""
    from . import ops
    from ._lib import RenderNetHipError
    opts = dict(line_options or {})
    unknown = sorted(set(opts) - set(ops.LINE_RANGES) - {"light"})
    if unknown:
        raise ValueError("line_options: unknown key(s) %s; expected some of %s"
                         % (", ".join(unknown), ", ".join(sorted(ops.LINE_RANGES) + ["light"])))
    try:
        out = ops.check_line_options("line_options", **{k: v for k, v in opts.items() if k != "light"})
        if out.get("levels", 1) == 0:
            raise RenderNetHipError("line_options: levels=0 (2..8; the picture without bands is shader=\"outline\")")
        if opts.get("light") is not None:
            ops.quantise_light(opts["light"])
            out["light"] = tuple(float(c) for c in np.asarray(opts["light"], np.float64).reshape(-1))
    except RenderNetHipError as e:
        raise ValueError(str(e))
    return out


def check_shadow_options(shadow_options):
    """`shadow_options` of SyntheticTargets -> a dict ready for ops.raycast_shadow: integer keys of ops.SHADOW_RANGES within
    their ranges ("smooth" may be None: the pixels of a cell) and "light", three finite components that are not all zero.
    Raises ValueError."""
    from . import ops
    from ._lib import RenderNetHipError
    opts = dict(shadow_options or {})
    unknown = sorted(set(opts) - set(ops.SHADOW_RANGES) - {"light"})
    if unknown:
        raise ValueError("shadow_options: unknown key(s) %s; expected some of %s"
                         % (", ".join(unknown), ", ".join(sorted(ops.SHADOW_RANGES) + ["light"])))
    try:
        out = ops.check_shadow_options("shadow_options", **{k: v for k, v in opts.items()
                                                            if k != "light" and not (k == "smooth" and v is None)})
        if "smooth" in opts and opts["smooth"] is None:
            out["smooth"] = None
        if opts.get("light") is not None:
            ops.quantise_light(opts["light"])
            out["light"] = tuple(float(c) for c in np.asarray(opts["light"], np.float64).reshape(-1))
    except RenderNetHipError as e:
        raise ValueError(str(e))
    return out


def read_models(model_path):
    """Every .binvox under `model_path`: (uint8 [n,64,64,64,1], names) in sorted file order."""
    import glob
    import os
    from .tools import binvox_rw
    files = sorted(glob.glob(os.path.join(model_path, "*.binvox")))
    if not files:
        raise ValueError("no .binvox files under %s" % model_path)
    models, names = [], []
    for p in files:
        with open(p, 'rb') as f:
            models.append(np.reshape(binvox_rw.read_as_3d_array(f).data, (64, 64, 64, 1)).astype(np.uint8))
        names.append(os.path.basename(p)[:-len(".binvox")])
    return np.stack(models), names


def draw_batch(rng, names, batch_size):
    """One whole batch: (model indices [bs], names [bs], poses float32 [bs,3])."""
    idx = rng.integers(0, len(names), size=batch_size)
    az = rng.uniform(0.0, 360.0, size=batch_size)
    el = rng.uniform(10.0, 170.0, size=batch_size)
    rad = rng.uniform(2.5, 4.5, size=batch_size)
    out, poses = [], np.empty((batch_size, 3), np.float32)
    for i in range(batch_size):
        a = float("%.2f" % az[i]) % 360.0                       # 359.996 prints as 360.00
        n = "%s_p%.2f_t%.2f_r%.1f" % (names[idx[i]], a, el[i], rad[i])
        out.append(n)
        poses[i] = data_util.extract_param_from_names(n)[0]
    return idx, out, poses


def _init_feed(self, models, names, batch_size, steps, rank, world, device):
    """What the two feeds share: batch, shard and model names checked, the models on the device, this rank's shard range."""
    import torch
    from .parallel import shard_range
    self.batch_size, self.steps = int(batch_size), int(steps)
    world, rank = int(world), int(rank)
    if self.batch_size < 1 or self.steps < 0:
        raise ValueError("batch_size=%d steps=%d" % (self.batch_size, self.steps))
    if world < 1 or not 0 <= rank < world or self.batch_size % world != 0:
        raise ValueError("rank %d of %d ranks for batch_size %d: every rank needs the same, non-empty shard"
                         % (rank, world, self.batch_size))
    self.names = [str(n) for n in names]
    if len(self.names) == 0 or len(self.names) != len(models):
        raise ValueError("%d names for %d models" % (len(self.names), len(models)))
    for n in self.names:
        if "_p" in n or "_t" in n or "_r" in n:
            raise ValueError("model name %r contains one of the pose tags _p / _t / _r" % n)
    self.device = torch.device(device)
    m = models if torch.is_tensor(models) else torch.as_tensor(np.ascontiguousarray(models))
    self.models = (m if m.dtype is torch.uint8 else m.float()).to(self.device)
    self.lo, self.hi = shard_range(self.batch_size, rank, world)


class SyntheticTargets(object):
    """Iterator over `steps` batches of (frames, voxels, poses, names), the tuple of `loader.PrefetchLoader`, for rank
    `rank` of `world`: voxels uint8 [b,S,S,S,1] and poses float32 [b,3] on `device`, and frames

      colour (greyscale=False): the uint8 normal map [b,4N,4N,3] on the device -- `Trainer._target_patch` feeds it to
                                rn_target_u8_crop_fwd like the prefetch loader's frames;
      greyscale=True:           float32 [b,4N,4N,1] on the device, the channel mean of the demo's Phong composite of that
                                normal map (ops.phong_composite, np_black, the demo's light and coefficients) -- what the demo
                                shows for a perfect normal map; it takes the float branch of `_target_patch`.

    `shader` names the picture: None = the two above by colour mode; "normal" (colour only) and "phong" (greyscale only) name
    them explicitly; "ao" = the ambient occlusion of the grid (ops.raycast_ao, whole frames, `ao_distance` voxels, smoothing =
    the 4 pixels of a cell): greyscale float32 [b,4N,4N,1] = byte / 255 as a float32 division, colour uint8 [b,4N,4N,3] with
    the byte in all three channels.  "outline" and "cel" = the line drawings (ops.raycast_outline / raycast_cel, whole frames,
    parameters from `line_options`, a dict with some of normal_radius, line_radius, depth_gap, crease_q, edge_mask, levels,
    shadow_byte, light -- the keywords of those two functions, checked here): frames exactly as for "ao".  "shadow" = the
    diffuse shading with cast shadows (ops.raycast_shadow, whole frames, parameters from `shadow_options`, a dict with some of
    normal_radius, bias, smooth, ambient_byte, light, checked here): frames exactly as for "ao".

    `models` uint8 | float [n,S,S,S,1] (host array or device tensor), `names` the n model names (no "_p", "_t" or "_r" inside:
    the pose parser looks for the first of each).  Same seed, same sequence; the shards of all ranks concatenate to the
    batch of world 1.  `seed` is what numpy.random.default_rng takes: an int, or a sequence of ints."""

    def __init__(self, models, names, batch_size, steps, seed, rank=0, world=1, device="cuda", greyscale=False, new_size=128,
                 shader=None, ao_distance=16, line_options=None, shadow_options=None):
        _init_feed(self, models, names, batch_size, steps, rank, world, device)
        self.greyscale, self.new_size = bool(greyscale), int(new_size)
        if shader is not None and shader not in SHADERS + LINE_SHADERS + SHADOW_SHADERS:
            raise ValueError("shader %r: expected None or one of %s" % (shader, ", ".join(SHADERS + LINE_SHADERS + SHADOW_SHADERS)))
        self.shader = ("phong" if self.greyscale else "normal") if shader is None else shader
        if self.shader in ("normal", "phong") and (self.shader == "phong") != self.greyscale:
            raise ValueError("shader %r gives %s frames: is_greyscale must be %s for it"
                             % (shader, "colour" if self.greyscale else "greyscale", not self.greyscale))
        self.ao_distance = int(ao_distance)
        if not 1 <= self.ao_distance <= 32:
            raise ValueError("ao_distance=%d: expected 1..32 voxels" % self.ao_distance)
        self.line_options = check_line_options(line_options)
        self.shadow_options = check_shadow_options(shadow_options)
        self.rng = np.random.default_rng(seed)                     # an int, or a sequence of ints such as (seed, epoch)
        self.done = 0

    def __iter__(self):
        return self

    def __len__(self):
        return self.steps

    def __next__(self):
        import torch
        if self.done >= self.steps:
            raise StopIteration
        self.done += 1
        idx, names, poses = draw_batch(self.rng, self.names, self.batch_size)          # the whole batch on every rank
        idx, names, poses = idx[self.lo:self.hi], names[self.lo:self.hi], poses[self.lo:self.hi]
        vox = self.models[torch.as_tensor(idx, dtype=torch.long, device=self.device)]
        pose = torch.as_tensor(poses).to(self.device)
        if self.shader == "ao" or self.shader in LINE_SHADERS + SHADOW_SHADERS:            # one byte per pixel
            if self.shader == "ao":
                grey = _cast_ao(vox, pose, self.new_size, 4, self.ao_distance)[..., None]
            elif self.shader in SHADOW_SHADERS:
                grey = _cast_shadow(vox, pose, self.new_size, 4, self.shadow_options)[..., None]
            else:
                grey = _cast_lines(vox, pose, self.new_size, 4, self.shader, self.line_options)[..., None]
            if not self.greyscale:
                return grey.expand(-1, -1, -1, 3).contiguous(), vox, pose, names
            if grey.is_cuda:                # a float32 division: torch's device kernel multiplies by the scalar's reciprocal instead
                from . import ops
                return ops.target_u8_crop(grey, (0, 0, grey.shape[1], grey.shape[2]), 1), vox, pose, names
            return grey.float() / 255.0, vox, pose, names
        frames = _cast(vox, pose, self.new_size, 4)
        if self.shader == "phong":
            frames = shade(frames).mean(dim=3, keepdim=True)
        return frames, vox, pose, names

    next = __next__

    def close(self):
        self.done = self.steps


class ColourModel(object):
    """The seeded linear colour field behind the albedo targets: K = z_dim plane waves over the voxel lattice, weighted by the
    quantised texture code (include/rendernet_hip.h, rn_raycast_albedo_fwd, states the colour rule).  From
    np.random.default_rng([seed, K]), in this order -- a changed order would invalidate every checkpoint trained on the field:

      f     = integers(-3, 4, (K, 3)), an all-zero row replaced by (1, 0, 0): periods of 64/3 voxels and longer;
      phase = integers(0, 256, K);
      amp   = integers(-127, 128, (K, 3)), one amplitude per colour channel.

    `waves` int16 [K,8], rows (fx, fy, fz, phase, aR, aG, aB, 0); `base` = the colour of a zero code.  The code is fed to the
    caster as int8 q = clip(rint(32 beta), -127, 127) (`quantise`) and to the net as float32 q / 32 (`dequantise`, exact), so
    picture and input are functions of the same numbers."""

    base = (144, 128, 112)

    def __init__(self, seed, z_dim):
        self.seed, self.z_dim = int(seed), int(z_dim)
        if not 1 <= self.z_dim <= 256:
            raise ValueError("z_dim=%d: the colour field takes 1..256 waves" % self.z_dim)
        K = self.z_dim
        rng = np.random.default_rng([self.seed, K])
        f = rng.integers(-3, 4, (K, 3))
        f[~f.any(axis=1)] = (1, 0, 0)
        phase = rng.integers(0, 256, K)
        amp = rng.integers(-127, 128, (K, 3))
        self.waves = np.zeros((K, 8), np.int16)
        self.waves[:, 0:3], self.waves[:, 3], self.waves[:, 4:7] = f, phase, amp

    @staticmethod
    def quantise(beta):
        return np.clip(np.rint(32.0 * np.asarray(beta, np.float64)), -127, 127).astype(np.int8)

    @staticmethod
    def dequantise(q):
        return np.asarray(q, np.int8).astype(np.float32) / np.float32(32.0)


class SyntheticTextureTargets(object):
    """Iterator over `steps` batches of (images, normals, voxels, textures, poses, names), the tuple the texture script's loop
    consumes, for rank `rank` of `world`, all on `device`: images and normals uint8 [b,4N,4N,3] (`TextureTrainer._target_patch`
    feeds them to rn_target_u8_crop_fwd), voxels uint8 [b,S,S,S,1], textures float32 [b,z_dim], poses float32 [b,3].

    Models, names and poses are `SyntheticTargets`' (same checks, same `draw_batch`); after those draws the codes of the whole
    batch come from rng.standard_normal((batch_size, z_dim)) on the same generator, quantised by `colour.quantise`: `textures`
    is the dequantised code, the very numbers the albedo was computed from.  `colour` is a `ColourModel` with z_dim waves;
    `smooth` (0..8) is the pixel radius of the albedo's masked mean.  Every rank draws the whole batch and keeps its shard.

    The reference adds uniform noise of one grey level to its 8-bit photographs before the loss, to dequantise them; it is NOT
    added here: the target is an exact function of the net's inputs, and noise would only blur what the tests pin."""

    def __init__(self, models, names, batch_size, steps, seed, colour, rank=0, world=1, device="cuda", new_size=128, smooth=4):
        import torch
        _init_feed(self, models, names, batch_size, steps, rank, world, device)
        if not isinstance(colour, ColourModel):
            raise ValueError("colour: expected a synth.ColourModel, got %s" % type(colour).__name__)
        if isinstance(smooth, (bool, float)) or not 0 <= int(smooth) <= 8:
            raise ValueError("smooth=%r: expected 0..8 pixels" % (smooth,))
        self.colour, self.new_size, self.smooth = colour, int(new_size), int(smooth)
        self.waves = torch.as_tensor(colour.waves).to(self.device)
        self.rng = np.random.default_rng(seed)                     # an int, or a sequence of ints such as (seed, epoch)
        self.done = 0

    def __iter__(self):
        return self

    def __len__(self):
        return self.steps

    def __next__(self):
        import torch
        if self.done >= self.steps:
            raise StopIteration
        self.done += 1
        idx, names, poses = draw_batch(self.rng, self.names, self.batch_size)          # the whole batch on every rank
        q = self.colour.quantise(self.rng.standard_normal((self.batch_size, self.colour.z_dim)))
        idx, names, poses, q = idx[self.lo:self.hi], names[self.lo:self.hi], poses[self.lo:self.hi], q[self.lo:self.hi]
        vox = self.models[torch.as_tensor(idx, dtype=torch.long, device=self.device)]
        pose = torch.as_tensor(poses).to(self.device)
        code_q = torch.as_tensor(q).to(self.device)
        images, normals = _cast_albedo(vox, pose, self.waves, code_q, self.colour.base, self.new_size, 4, self.smooth)
        textures = torch.as_tensor(self.colour.dequantise(q)).to(self.device)
        return images, normals, vox, textures, pose, names

    next = __next__

    def close(self):
        self.done = self.steps


def shade(normals_u8):
    """The demo's Phong composite of a uint8 normal map [b,H,W,3] on the device -> float32 [b,H,W,3]."""
    import torch
    from . import ops
    from .tools.Phong_shading import generate_light_pos
    dev = normals_u8.device
    light = torch.as_tensor(generate_light_pos(LIGHT_ELEVATION, LIGHT_AZIMUTH).astype(np.float32)).to(dev)
    col = torch.ones((1, 3), dtype=torch.float32, device=dev)
    return ops.phong_composite(normals_u8.float() / 255.0, light, col, AMBIENT_IN, K_DIFFUSE, "np_black")
