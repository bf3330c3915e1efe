"""NumPy twin of rn_mask_pack / rn_pose_score / rn_pose_best (include/rendernet_hip.h states the rule): the splat of a grid under
an integer camera with a footprint, the two counts of every candidate against a mask, and the winner under the int64
cross-multiplied order with ties to the lower index.  TEST INFRASTRUCTURE ONLY.  Built on voxel_carve_ref.project_centres and
cameras (hence mesh_raster_ref): it takes the `cam` it is handed, so the device tests hand it what the device produced.  Also the
pose lattice, the refinement neighbourhood and the footprint choice of the Python layer, restated."""
import math
import os

import numpy as np

import voxel_carve_ref as VC

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MAX_FOOTPRINT = 4


def load_binvox(name):
    from oracle.io_phong import read_binvox
    return read_binvox(os.path.join(ROOT, "binvox", name + ".binvox")).astype(bool)


def pool(g, k=2):
    """OR-pool a cubic bool grid by k on each axis."""
    S = g.shape[0] // k
    return np.asarray(g, bool).reshape(S, k, S, k, S, k).any((1, 3, 5))


def ball(S, radius):
    k = np.arange(S) - (S - 1) / 2.0
    z, y, x = np.meshgrid(k, k, k, indexing="ij")
    return z * z + y * y + x * x <= radius * radius


def splat(occ, cam, window, fp):
    """occ bool [S,S,S], cam int64 [3,4], window (row0, col0, ph, pw), fp in 1..4 -> bool [ph,pw]."""
    assert 1 <= int(fp) <= MAX_FOOTPRINT
    occ = np.asarray(occ, bool)
    S = occ.shape[0]
    row0, col0, ph, pw = (int(v) for v in window)
    X, Y, _ = VC.project_centres(np.asarray(cam, np.int64).reshape(3, 4), S)
    x, y = X[occ], Y[occ]
    lead = 128 * (int(fp) - 1)
    r0, c0 = ((y - lead) >> 8) - row0, ((x - lead) >> 8) - col0       # floor division
    img = np.zeros((ph, pw), bool)
    for i in range(int(fp)):
        for j in range(int(fp)):
            r, c = r0 + i, c0 + j
            ok = (r >= 0) & (r < ph) & (c >= 0) & (c < pw)            # each pixel against the window on its own
            img[r[ok], c[ok]] = True
    return img


def splats(occ, cams, window, fp):
    cams = np.asarray(cams, np.int64).reshape(-1, 3, 4)
    return np.stack([splat(occ, c, window, fp) for c in cams])


def scores(occ, cams, mask, window, fp, images=None):
    """-> (int32 [P,2] of (n_splat, n_inter), n_mask) of one item; `images` are its splats when they are already at hand."""
    m = np.asarray(mask) != 0
    sp = splats(occ, cams, window, fp) if images is None else np.asarray(images, bool)
    out = np.stack([sp.sum((1, 2)), (sp & m[None]).sum((1, 2))], 1).astype(np.int32)
    return out, int(m.sum())


def union(n_splat, n_inter, n_mask):
    return int(n_splat) + int(n_mask) - int(n_inter)


def best(table, n_mask):
    """table int [P,2] -> (the winner's index, (n_splat, n_inter, n_mask)): Python integers, first strict maximum."""
    t = [(int(a), int(b)) for a, b in np.asarray(table).reshape(-1, 2)]
    assert len(t) >= 1

    def frac(p):
        u = union(t[p][0], t[p][1], n_mask)
        return (t[p][1], u) if u > 0 else (0, 1)

    w = 0
    for p in range(1, len(t)):
        (ni, un), (wi, wu) = frac(p), frac(w)
        if ni * wu > wi * un:
            w = p
    return w, (t[w][0], t[w][1], int(n_mask))


def iou(n_splat, n_inter, n_mask):
    u = union(n_splat, n_inter, n_mask)
    return float(n_inter) / u if u > 0 else 0.0


def pose_lattice(n_azimuth, elevations, scales):
    """float32 [P,3]: azimuth index fastest, then elevation, then scale; azimuth 2 pi a / n_azimuth."""
    out = [(2.0 * math.pi * a / n_azimuth, e, s) for s in scales for e in elevations for a in range(n_azimuth)]
    return np.asarray(out, np.float64).astype(np.float32)


def lattice_steps(n_azimuth, elevations, scales):
    def step(v):
        return (max(v) - min(v)) / (len(v) - 1) if len(v) > 1 else 0.0
    return 2.0 * math.pi / n_azimuth, step(elevations), step(scales)


def refine_lattice(centre, steps, level, elevations, scales):
    """float32 [75,3] around `centre` at refinement `level` >= 1: the three steps of the level-0 lattice halved `level` times,
    5 x 5 x 3 offsets (azimuth fastest); azimuth wraps, elevation and scale are clipped to the level-0 range."""
    az, el, sc = (float(v) for v in centre)
    h = [s / float(2 ** level) for s in steps]
    out = []
    for k in (-1, 0, 1):
        for j in (-2, -1, 0, 1, 2):
            for i in (-2, -1, 0, 1, 2):
                out.append((math.fmod(math.fmod(az + i * h[0], 2.0 * math.pi) + 2.0 * math.pi, 2.0 * math.pi),
                            min(max(el + j * h[1], min(elevations)), max(elevations)),
                            min(max(sc + k * h[2], min(scales)), max(scales))))
    return np.asarray(out, np.float64).astype(np.float32)


def search(occ, mask, n_azimuth, elevations, scales, refine, N, f, window, fp, level0=None):
    """The coarse-to-fine search of ONE item on the twin: a list with one (lattice float32 [P,3], winner index, winner pose) per
    level.  `level0` is the (cams, splats) of the level-0 lattice when the caller has them already (they do not depend on the
    mask)."""
    occ = np.asarray(occ, bool)
    S = occ.shape[0]
    lattice = pose_lattice(n_azimuth, elevations, scales)
    steps = lattice_steps(n_azimuth, elevations, scales)
    out = []
    for level in range(int(refine) + 1):
        if level == 0 and level0 is not None:
            cams, images = level0
        else:
            cams, _ = VC.cameras(lattice, [False] * len(lattice), S, N, f)
            images = splats(occ, cams, window, fp)
        table, n_mask = scores(occ, cams, mask, window, fp, images)
        w, _ = best(table, n_mask)
        out.append((lattice, w, lattice[w]))
        lattice = refine_lattice(lattice[w], steps, level + 1, elevations, scales)
    return out


def pixels_per_voxel(cams):
    """The LARGER Euclidean norm of camera rows 0 and 1 over 2^20, the largest over the cameras."""
    a = np.asarray(cams, np.int64).astype(np.float64).reshape(-1, 3, 4)[:, :2, :3]
    return float(np.sqrt((a * a).sum(-1)).max()) / float(1 << 20) if a.size else 0.0


def choose_footprint(ppv):
    """The smallest fp in 1..4 with ppv < fp / sqrt 2; None when there is none."""
    for fp in range(1, MAX_FOOTPRINT + 1):
        if ppv < fp / math.sqrt(2.0):
            return fp
    return None


def holes(img):
    """The background pixels whose four neighbours are all foreground."""
    f = np.pad(np.asarray(img, bool), 1)
    return ~f[1:-1, 1:-1] & f[:-2, 1:-1] & f[2:, 1:-1] & f[1:-1, :-2] & f[1:-1, 2:]
