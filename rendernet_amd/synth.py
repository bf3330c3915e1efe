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

Shapes.  With `shapes` > 0 a sample's grid is, with that probability, not one of the models but a procedural one: a seeded
constructive-solid-geometry description (`shape_prims`: a few rotated ellipsoids, boxes, cylinders, cones and tori, united
and subtracted) rasterised on the device (`ops.voxel_shapes`, rn_voxel_shapes).  The decision and the shape's 32-bit id come
from a SECOND generator, so the pose stream -- and with `shapes` = 0 every batch -- is what it was without them.

Mesh targets.  With `mesh_set` (a `mesh.MeshSet`) the frames of the samples whose model came from a mesh are the picture of the
mesh itself, rasterised under the caster's camera (`ops.rasterize_mesh`, rn_mesh_rasterize), while the voxels stay its
voxelisation: smooth shading as the target of blocky input, the reference's pairing.  Nothing is drawn for it: voxels, poses
and names are what they are without the argument.
"""
import math

import numpy as np

from .tools import data_util

# the demo's shading (RenderNet_demo.py:17-20 and its --light_* defaults)
AMBIENT_IN, K_DIFFUSE, LIGHT_ELEVATION, LIGHT_AZIMUTH = 0.1, 0.9, 60.0, 250.0


def _cast(vox, poses, new_size, pixels_per_cell):
    """The caster behind SyntheticTargets (a module attribute so that host-only tests can replace it)."""
    from . import ops
    return ops.raycast_normals(vox, poses, new_size=new_size, pixels_per_cell=pixels_per_cell)


def _raster(mesh_set, mesh_ids, poses, new_size, pixels_per_cell, cull):
    """The rasteriser behind SyntheticTargets(mesh_set=...) (a module attribute, like `_cast`): the smooth normal map of meshes
    `mesh_ids` of the set at `poses`, uint8 [n,H,W,3]."""
    return mesh_set.rasterize(mesh_ids, poses, new_size=new_size, pixels_per_cell=pixels_per_cell, cull=cull)


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


def _shapes(prims, S, device):
    """The rasteriser behind the feeds' procedural grids (a module attribute, like `_cast`): prims int32 [n,K,16] on the host
    -> uint8 [n,S,S,S,1] on `device`."""
    import torch
    from . import ops
    return ops.voxel_shapes(torch.as_tensor(prims).to(device), S)


SHAPE_SLOTS, SHAPE_NOOP = 8, 255          # RN_SHAPES_MAX_PRIMS, RN_SHAPES_NOOP of include/rendernet_hip.h


def _shape_radius(t, a):
    """A bounding radius of primitive type t with semi-axes a, in the units of a, enlarged 5 % + 1: the rotation is rounded to
    1/64 (its smallest singular value is above 62.5 / 64) and the ellipsoid's weights 2^14 / a are rounded down (below 0.8 %)."""
    if t == 0:
        r = float(max(a))
    elif t == 1:
        r = float(np.sqrt(float(a[0]) ** 2 + float(a[1]) ** 2 + float(a[2]) ** 2))
    elif t == 2:
        r = float(np.hypot(max(a[0], a[1]), a[2]))
    elif t == 3:
        r = float(np.hypot(a[0], a[2]))
    else:
        r = float(a[0] + a[1])
    return int(np.ceil(1.05 * r)) + 1


def shape_prims(shape_seed, ids, S=64):
    """The descriptions of the procedural shapes `ids` (32-bit integers) for grids of side S (32 or 64): int32 [n, 8, 16] on the
    host, rows as rn_voxel_shapes reads them (include/rendernet_hip.h: word 0 = type | op << 8, centre, semi-axes, 64 R),
    unused slots marked with type 255.  Shape i is a pure function of (shape_seed, ids[i], S).  From
    np.random.default_rng([shape_seed, id]), in this order -- a changed order would invalidate every checkpoint trained on
    the shapes (lengths are for S = 64 and scale with S / 64, in half-voxels):

      K = integers(2, 7), the number of primitives; then for slot k = 0 .. K-1, in turn:
        type  = integers(0, 5): ellipsoid, box, cylinder, cone, torus;
        op    = 0 (union) for slot 0, else random() < 0.3 (subtraction);
        a     = integers(lo, hi + 1, 3), the semi-axes: 20..56 for slot 0, 8..40 for the others;
        a[1]  = integers(4, max(4, a[0] // 2) + 1) for a torus only, its minor radius (<= major / 2); a cone takes a[1] = a[0];
        quat  = standard_normal(4), normalised: the rotation R, stored as rint(64 R);
        c     = integers(-m, m + 1, 3), the centre: m = 40 for a subtraction; for a union m = S - 4 - rho with rho the
                bounding radius of the primitive enlarged 5 % + 1 (`_shape_radius`), so that |c_k| + rho <= S - 4 and the
                grid's border layers stay empty (the resampler and the caster agree only on such grids).  A union too large
                for that has its semi-axes multiplied by 3/4 (integer division; a torus keeps a minor radius of at least 4) until it
                fits; that draws nothing."""
    S = int(S)
    if S not in (32, 64):
        raise ValueError("shape_prims: S=%d (32 or 64)" % S)
    ids = np.asarray(ids, dtype=np.uint64).reshape(-1)
    if ids.size and int(ids.max()) >= 1 << 32:
        raise ValueError("shape_prims: ids are 32-bit")
    out = np.zeros((len(ids), SHAPE_SLOTS, 16), np.int32)
    out[:, :, 0] = SHAPE_NOOP

    def scaled(v):
        return v * S // 64
    for n, sid in enumerate(ids):
        rng = np.random.default_rng([int(shape_seed), int(sid)])
        for k in range(int(rng.integers(2, 7))):
            t = int(rng.integers(0, 5))
            op = 0 if k == 0 else int(rng.random() < 0.3)
            lo, hi = (scaled(20), scaled(56)) if k == 0 else (scaled(8), scaled(40))
            a = [int(v) for v in rng.integers(lo, hi + 1, 3)]
            if t == 4:
                a[1] = int(rng.integers(scaled(4), max(scaled(4), a[0] // 2) + 1))
            elif t == 3:
                a[1] = a[0]
            q = rng.standard_normal(4)
            w, x, y, z = q / np.sqrt((q * q).sum())
            R = np.array([[1 - 2 * (y * y + z * z), 2 * (x * y - z * w), 2 * (x * z + y * w)],
                          [2 * (x * y + z * w), 1 - 2 * (x * x + z * z), 2 * (y * z - x * w)],
                          [2 * (x * z - y * w), 2 * (y * z + x * w), 1 - 2 * (x * x + y * y)]])
            if op == 0:
                while _shape_radius(t, a) > S - 4:
                    a = [max(v * 3 // 4, 1) for v in a]
                    if t == 4:
                        a[1] = max(a[1], scaled(4))
                m = S - 4 - _shape_radius(t, a)
            else:
                m = scaled(40)
            c = rng.integers(-m, m + 1, 3)
            out[n, k, 0] = t | op << 8
            out[n, k, 1:4], out[n, k, 4:7], out[n, k, 7:16] = c, a, np.rint(64.0 * R).reshape(-1)
    return out


SHADERS = ("normal", "phong", "ao")
LINE_SHADERS = ("outline", "cel")
SHADOW_SHADERS = ("shadow",)
CEL_ONLY_OPTIONS = ("light", "levels", "shadow_byte")


def _check_options(name, options, ranges, checker, refuse=None):
    """A shader's option dict of SyntheticTargets, called `name` in messages -> a dict ready for its caster: the keys of
    `ranges` through the ops checker, refuse(those) as a message for a combination this feed does not take, and "light",
    three finite components that are not all zero.  Raises ValueError."""
    from . import ops
    from ._lib import RenderNetHipError
    opts = dict(options or {})
    unknown = sorted(set(opts) - set(ranges) - {"light"})
    if unknown:
        raise ValueError("%s: unknown key(s) %s; expected some of %s"
                         % (name, ", ".join(unknown), ", ".join(sorted(ranges) + ["light"])))
    try:
        out = checker(name, **{k: v for k, v in opts.items() if k != "light"})
        if refuse is not None and refuse(out):
            raise RenderNetHipError(refuse(out))
        if opts.get("light") is not None:
            ops.quantise_light(opts["light"])
            out["light"] = tuple(float(c) for c in np.asarray(opts["light"], np.float64).reshape(-1))
    except RenderNetHipError as e:
        raise ValueError(str(e))
    return out


def check_line_options(line_options):
    """`line_options` of SyntheticTargets -> a dict ready for ops.raycast_outline / raycast_cel: integer keys of
    ops.LINE_RANGES within their ranges (levels 2..8 here: without bands the picture is "outline") and "light", three
    finite components that are not all zero.  Raises ValueError."""
    from . import ops

    def refuse(out):
        if out.get("levels", 1) == 0:
            return "line_options: levels=0 (2..8; the picture without bands is shader=\"outline\")"
    return _check_options("line_options", line_options, ops.LINE_RANGES, ops.check_line_options, refuse)


def check_shadow_options(shadow_options):
    """`shadow_options` of SyntheticTargets -> a dict ready for ops.raycast_shadow: integer keys of ops.SHADOW_RANGES within
    their ranges ("smooth" may be None: the pixels of a cell) and "light", three finite components that are not all zero.
    Raises ValueError."""
    from . import ops
    opts = dict(shadow_options or {})
    auto_smooth = "smooth" in opts and opts["smooth"] is None
    if auto_smooth:
        del opts["smooth"]
    out = _check_options("shadow_options", opts, ops.SHADOW_RANGES, ops.check_shadow_options)
    if auto_smooth:
        out["smooth"] = None
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


def draw_batch(rng, names, batch_size, shape_ids=None):
    """One whole batch: (model indices [bs], names [bs], poses float32 [bs,3]).  `shape_ids` (int64 [bs], -1 = a model) names
    the procedural samples: theirs is `shape%08x` of the id in place of the model's name; the draws from `rng` are the same."""
    idx = rng.integers(0, max(len(names), 1), size=batch_size)
    az = rng.uniform(0.0, 360.0, size=batch_size)
    el = rng.uniform(10.0, 170.0, size=batch_size)
    rad = rng.uniform(2.5, 4.5, size=batch_size)
    out, poses = [], np.empty((batch_size, 3), np.float32)
    for i in range(batch_size):
        a = float("%.2f" % az[i]) % 360.0                       # 359.996 prints as 360.00
        model = names[idx[i]] if shape_ids is None or shape_ids[i] < 0 else "shape%08x" % int(shape_ids[i])
        n = "%s_p%.2f_t%.2f_r%.1f" % (model, a, el[i], rad[i])
        out.append(n)
        poses[i] = data_util.extract_param_from_names(n)[0]
    return idx, out, poses


SCAN_ELEVATIONS = (0.3, 0.9, 1.4)        # radians, cycled by `scan_poses`


def scan_poses(K, scale=1.0):
    """The view set of a turntable scan for `ops.voxel_scan` / `ops.voxel_carve`: (poses float32 [K,3], low [K] of bool).  View
    k has azimuth 2 pi k / K + 0.1, elevation SCAN_ELEVATIONS[k % 3] and looks from the low-x end of the ray when k is odd:
    alternating ends is what shows the underside of a seat, a set with only the default end leaves it uncarved."""
    K = int(K)
    if K < 1:
        raise ValueError("scan_poses: K=%d views (at least 1)" % K)
    poses = np.empty((K, 3), np.float32)
    for k in range(K):
        poses[k] = (2.0 * np.pi * k / K + 0.1, SCAN_ELEVATIONS[k % 3], scale)
    return poses, [bool(k % 2) for k in range(K)]


POSE_ELEVATIONS = (0.1, 0.4, 0.7, 1.0, 1.3)   # radians from the horizon: the default lattice of `ops.voxel_pose_search`
POSE_SCALES = (0.8, 1.0, 1.25)
POSE_REFINE_OFFSETS = (5, 5, 3)               # candidates of a refinement level along azimuth, elevation, scale


def _lattice_axis(what, name, values):
    try:
        v = [float(x) for x in values]
    except (TypeError, ValueError):
        v = []
    if not v or not all(math.isfinite(x) for x in v):
        raise ValueError("%s: %s=%r (one or more finite numbers)" % (what, name, values))
    return v


def pose_lattice(n_azimuth, elevations, scales):
    """The candidate poses of a silhouette pose search (`ops.voxel_pose_scores`): float32 [P,3] of (azimuth, elevation, scale),
    P = n_azimuth * len(elevations) * len(scales).  THE AZIMUTH INDEX RUNS FASTEST, THEN ELEVATION, THEN SCALE -- the order is
    part of the contract, because equal scores go to the lower index.  Azimuth a is 2 pi a / n_azimuth; elevations are radians
    from the horizon, as tools/data_util.extract_param_from_names produces them; scale is 3.3 / radius."""
    if isinstance(n_azimuth, (bool, float)) or int(n_azimuth) < 1:
        raise ValueError("pose_lattice: n_azimuth=%r (an integer, at least 1)" % (n_azimuth,))
    el, sc = _lattice_axis("pose_lattice", "elevations", elevations), _lattice_axis("pose_lattice", "scales", scales)
    out = np.empty((len(sc), len(el), int(n_azimuth), 3), np.float64)
    out[..., 0] = 2.0 * math.pi * np.arange(int(n_azimuth)) / int(n_azimuth)
    out[..., 1] = np.asarray(el)[None, :, None]
    out[..., 2] = np.asarray(sc)[:, None, None]
    return out.reshape(-1, 3).astype(np.float32)


def pose_lattice_steps(n_azimuth, elevations, scales):
    """The three steps of `pose_lattice`: 2 pi / n_azimuth, and the range of the elevations and of the scales over their count
    less one (0 for a single value)."""
    def step(v):
        return (max(v) - min(v)) / (len(v) - 1) if len(v) > 1 else 0.0
    return (2.0 * math.pi / int(n_azimuth), step(_lattice_axis("pose_lattice_steps", "elevations", elevations)),
            step(_lattice_axis("pose_lattice_steps", "scales", scales)))


def pose_refine_lattice(centre, steps, level, elevations, scales):
    """The 5 x 5 x 3 neighbourhood of `centre` (azimuth, elevation, scale) at refinement `level` >= 1, float32 [75,3] in the
    order of `pose_lattice`: offsets -2..2 in azimuth and elevation and -1..1 in scale, in units of the level-0 `steps` halved
    `level` times.  Azimuth wraps into [0, 2 pi); elevation and scale are clipped to the level-0 range."""
    az, el, sc = (float(v) for v in centre)
    h = [float(s) / float(2 ** int(level)) for s in steps]
    el_lo, el_hi, sc_lo, sc_hi = min(elevations), max(elevations), min(scales), max(scales)
    na, ne, ns = POSE_REFINE_OFFSETS
    out = np.empty((ns, ne, na, 3), np.float64)
    for k in range(ns):
        for j in range(ne):
            for i in range(na):
                a = math.fmod(math.fmod(az + (i - na // 2) * h[0], 2.0 * math.pi) + 2.0 * math.pi, 2.0 * math.pi)
                out[k, j, i] = (a, min(max(el + (j - ne // 2) * h[1], el_lo), el_hi), min(max(sc + (k - ns // 2) * h[2], sc_lo), sc_hi))
    return out.reshape(-1, 3).astype(np.float32)


SHAPE_STREAM = 0x5AFE                    # appended to the feed's seed: the generator of the shape decisions and ids


def _init_feed(self, models, names, batch_size, steps, rank, world, device, seed=None, shapes=0.0, shape_seed=None, shape_size=None):
    """What the two feeds share: batch, shard and model names checked, the models on the device, this rank's shard range, and
    the procedural shapes: their probability, seed, grid side and generator."""
    import torch
    from .parallel import shard_range
    self.batch_size, self.steps = int(batch_size), int(steps)
    world, rank = int(world), int(rank)
    if self.batch_size < 1 or self.steps < 0:
        raise ValueError("batch_size=%d steps=%d" % (self.batch_size, self.steps))
    if world < 1 or not 0 <= rank < world or self.batch_size % world != 0:
        raise ValueError("rank %d of %d ranks for batch_size %d: every rank needs the same, non-empty shard"
                         % (rank, world, self.batch_size))
    if isinstance(shapes, (bool, str)) or not 0.0 <= float(shapes) <= 1.0:
        raise ValueError("shapes=%r: expected a probability in [0, 1]" % (shapes,))
    self.shapes = float(shapes)
    self.names = [str(n) for n in (names if names is not None else ())]
    n_models = 0 if models is None else len(models)
    if len(self.names) != n_models or (n_models == 0 and self.shapes < 1.0):
        raise ValueError("%d names for %d models%s" % (len(self.names), n_models,
                                                       "" if n_models else " (only shapes=1.0 does without models)"))
    for n in self.names:
        if "_p" in n or "_t" in n or "_r" in n:
            raise ValueError("model name %r contains one of the pose tags _p / _t / _r" % n)
    self.device = torch.device(device)
    self.models = None
    if n_models:
        m = models if torch.is_tensor(models) else torch.as_tensor(np.ascontiguousarray(models))
        self.models = (m if m.dtype is torch.uint8 else m.float()).to(self.device)
    self.lo, self.hi = shard_range(self.batch_size, rank, world)
    self.shape_size = int(shape_size) if shape_size is not None else (int(self.models.shape[1]) if n_models else 64)
    self.shape_rng = self.shape_seed = None
    if self.shapes > 0.0:
        if self.shape_size not in (32, 64) or (n_models and tuple(self.models.shape[1:]) != (self.shape_size,) * 3 + (1,)):
            raise ValueError("shapes: procedural grids have side 32 or 64 and the side of the models, got shape_size=%d and models %s"
                             % (self.shape_size, tuple(self.models.shape) if n_models else None))
        words = [int(v) for v in np.atleast_1d(np.asarray(seed)).reshape(-1)]
        self.shape_seed = words[0] if shape_seed is None else int(shape_seed)
        self.shape_rng = np.random.default_rng(words + [SHAPE_STREAM])


def _draw_shapes(self):
    """The whole batch's shape ids from the second generator, int64 [bs], -1 = a model: random(bs) < shapes decides, then
    integers(0, 2^32, bs) are the ids (both drawn whatever is decided).  None when the feed has no shapes."""
    if self.shape_rng is None:
        return None
    use = self.shape_rng.random(self.batch_size) < self.shapes
    ids = self.shape_rng.integers(0, 1 << 32, size=self.batch_size, dtype=np.uint64).astype(np.int64)
    return np.where(use, ids, -1)


def _feed_grids(self, idx, shape_ids):
    """The voxels of this rank's shard: the models `idx`, and for the samples with a shape id the procedural grid, all of
    them from one `_shapes` call."""
    import torch
    proc = np.zeros(len(idx), bool) if shape_ids is None else shape_ids >= 0
    vox = None if proc.all() and len(idx) else self.models[torch.as_tensor(idx, dtype=torch.long, device=self.device)]
    if proc.any():
        grids = _shapes(shape_prims(self.shape_seed, shape_ids[proc], self.shape_size), self.shape_size, self.device)
        if vox is None:
            return grids
        vox[torch.as_tensor(np.flatnonzero(proc), dtype=torch.long, device=self.device)] = grids.to(vox.dtype)
    return vox


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
    batch of world 1.  `seed` is what numpy.random.default_rng takes: an int, or a sequence of ints.

    `shapes` in [0, 1] is the per-sample probability that the grid is procedural (`shape_prims`, `ops.voxel_shapes`) and not a
    model; 1.0 does without models (`models=None`, `names=()`); `shape_seed` seeds the shapes (None: the first integer of
    `seed`) and `shape_size` is their side, 32 or 64 (None: the models', 64 without models).  The decisions and the 32-bit ids
    come from np.random.default_rng([*seed, 0x5AFE]), per batch random(bs) then integers(0, 2^32, bs): the pose generator's
    stream is untouched, and with shapes = 0 every batch is what it was without these arguments.  A procedural sample is named
    `shape%08x_p.._t.._r..` from its id, so the grid behind a sample PNG can be made again (RenderNet_demo.py --voxel_shape).

    `mesh_set` (a `mesh.MeshSet`) with `mesh_models` (per model of `models` the index of its mesh in the set, -1 for a model that
    is no mesh) makes the target of a sample whose model came from a mesh the picture of the MESH: the rasterised smooth normal
    map at the sample's pose (`ops.rasterize_mesh`, culling `mesh_cull`), which overlays the ray-cast view of the model's grid
    pixel for pixel; "phong" shades it as it shades the caster's.  The voxels stay the voxelised grid; binvox and procedural
    samples keep the caster; shaders "normal" and "phong" only.  No random draw is added: voxels, poses and names are what they
    are without the argument."""

    def __init__(self, models, names, batch_size, steps, seed, rank=0, world=1, device="cuda", greyscale=False, new_size=128,
                 shader=None, ao_distance=16, line_options=None, shadow_options=None, shapes=0.0, shape_seed=None, shape_size=None,
                 mesh_set=None, mesh_models=None, mesh_cull="back"):
        _init_feed(self, models, names, batch_size, steps, rank, world, device, seed, shapes, shape_seed, shape_size)
        self.mesh_set, self.mesh_models, self.mesh_cull = mesh_set, None, mesh_cull
        if (mesh_set is None) != (mesh_models is None):
            raise ValueError("mesh_set and mesh_models come together")
        if mesh_set is not None:
            mm = np.asarray(mesh_models)
            if mm.dtype.kind not in "iu" or mm.shape != (len(self.names),) or (len(mm) and (mm.min() < -1 or mm.max() >= len(mesh_set))):
                raise ValueError("mesh_models: expected one index into the %d meshes of the set, or -1, for each of the %d models"
                                 % (len(mesh_set), len(self.names)))
            if mesh_cull not in ("back", "none"):
                raise ValueError("mesh_cull=%r: expected back or none" % (mesh_cull,))
            if self.models is not None and int(self.models.shape[1]) != int(mesh_set.S):
                raise ValueError("mesh_set was fitted to %d^3 grids, the models are %d^3" % (mesh_set.S, int(self.models.shape[1])))
            self.mesh_models = mm.astype(np.int64)
        self.greyscale, self.new_size = bool(greyscale), int(new_size)
        if shader is not None and shader not in SHADERS + LINE_SHADERS + SHADOW_SHADERS:
            raise ValueError("shader %r: expected None or one of %s" % (shader, ", ".join(SHADERS + LINE_SHADERS + SHADOW_SHADERS)))
        self.shader = ("phong" if self.greyscale else "normal") if shader is None else shader
        if mesh_set is not None and self.shader not in ("normal", "phong"):
            raise ValueError("mesh targets are normal maps: shader %r needs voxel hits; expected normal or phong" % (self.shader,))
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
        ids = _draw_shapes(self)
        idx, names, poses = draw_batch(self.rng, self.names, self.batch_size, ids)     # the whole batch on every rank
        idx, names, poses = idx[self.lo:self.hi], names[self.lo:self.hi], poses[self.lo:self.hi]
        vox = _feed_grids(self, idx, None if ids is None else ids[self.lo:self.hi])
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
        is_mesh = np.zeros(len(idx), bool)
        if self.mesh_models is not None and len(self.mesh_models):
            is_mesh = self.mesh_models[idx] >= 0
            if ids is not None:
                is_mesh &= ids[self.lo:self.hi] < 0                     # a procedural sample is no model
        if not is_mesh.any():
            frames = _cast(vox, pose, self.new_size, 4)
        else:
            frames = _raster(self.mesh_set, self.mesh_models[idx[is_mesh]].astype(np.int32),
                             pose[torch.as_tensor(np.flatnonzero(is_mesh), device=self.device)], self.new_size, 4, self.mesh_cull)
            if not is_mesh.all():
                rest = torch.as_tensor(np.flatnonzero(~is_mesh), device=self.device)
                both = frames.new_empty((len(idx),) + tuple(frames.shape[1:]))
                both[torch.as_tensor(np.flatnonzero(is_mesh), device=self.device)] = frames
                both[rest] = _cast(vox[rest], pose[rest], self.new_size, 4)
                frames = both
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
    `shapes`, `shape_seed` and `shape_size` are `SyntheticTargets`': procedural grids from a second generator.

    The reference adds uniform noise of one grey level to its 8-bit photographs before the loss, to dequantise them; it is NOT
    added here: the target is an exact function of the net's inputs, and noise would only blur what the tests pin."""

    def __init__(self, models, names, batch_size, steps, seed, colour, rank=0, world=1, device="cuda", new_size=128, smooth=4,
                 shapes=0.0, shape_seed=None, shape_size=None):
        import torch
        _init_feed(self, models, names, batch_size, steps, rank, world, device, seed, shapes, shape_seed, shape_size)
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
        ids = _draw_shapes(self)
        idx, names, poses = draw_batch(self.rng, self.names, self.batch_size, ids)     # the whole batch on every rank
        q = self.colour.quantise(self.rng.standard_normal((self.batch_size, self.colour.z_dim)))
        idx, names, poses, q = idx[self.lo:self.hi], names[self.lo:self.hi], poses[self.lo:self.hi], q[self.lo:self.hi]
        vox = _feed_grids(self, idx, None if ids is None else ids[self.lo:self.hi])
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
