"""Validation metrics of the training scripts: PSNR and SSIM per image, computed on the device (`ops.image_metrics`,
rn_image_metrics; include/rendernet_hip.h states the rule) from the prediction before it is copied to the host.

    on = metrics_options(cfg, argv)            # --val-metrics / "val_metrics", default off
    vm = ValidationMetrics()
    vm.add(pred, target); print(vm.line())     # per validation batch
    psnr, ssim = vm.epoch_means()

Both images are compared as bytes: a float image is quantised as rint(clip(255 x, 0, 255)).
"""
import numpy as np

# The PSNR of an image pair with ssd = 0 is +inf.  It enters a MEAN as the value at ssd = 0.5, half the smallest non-zero sum
# of squares: 10 log10(65025 n / 0.5), finite and above every PSNR a differing pair of that size can have.  The per-image
# values that `ValidationMetrics` keeps stay +inf.
_SSD_OF_EQUAL_IMAGES = 0.5


def metrics_options(cfg, argv):
    """True when the validation pass also reports PSNR and SSIM: `--val-metrics` on the command line or a true config key
    "val_metrics" (a JSON boolean, or "true" / "false" like "is_greyscale").  Default off: no new line, key or file."""
    raw = cfg.get("val_metrics", False)
    if isinstance(raw, str):
        if raw.lower() not in ("true", "false"):
            raise SystemExit("\"val_metrics\": %r is neither true nor false" % raw)
        raw = raw.lower() == "true"
    elif not isinstance(raw, bool):
        raise SystemExit("\"val_metrics\": %r is neither true nor false" % (raw,))
    if "--val-metrics" in argv and "--train" not in argv:
        raise SystemExit("--val-metrics needs --train")
    return raw or "--val-metrics" in argv


def derive(sad, ssd, ssim_sum, H, W, C):
    """(l1, mse, psnr, ssim) in float64 from the sums of rn_image_metrics, arrays of one value per image:
    l1 = sad / (255 n), mse = ssd / n, psnr = 10 log10(65025 / mse), +inf where ssd = 0, ssim = ssim_sum / n_win, with
    n = H W C and n_win = (H - 10)(W - 10) C."""
    n, n_win = float(H * W * C), float((H - 10) * (W - 10) * C)
    sad, ssd, ssim_sum = (np.asarray(v, np.float64) for v in (sad, ssd, ssim_sum))
    mse = ssd / n
    with np.errstate(divide="ignore"):
        psnr = 10.0 * np.log10(65025.0 / mse)
    return sad / (255.0 * n), mse, psnr, ssim_sum / n_win


def psnr_for_mean(psnr, n):
    """`psnr` with every +inf replaced by the PSNR at ssd = 0.5 of an image of n samples (see _SSD_OF_EQUAL_IMAGES)."""
    psnr = np.asarray(psnr, np.float64)
    return np.where(np.isposinf(psnr), 10.0 * np.log10(65025.0 * float(n) / _SSD_OF_EQUAL_IMAGES), psnr)


class ValidationMetrics(object):
    """Accumulates the per-image PSNR and SSIM of one validation pass."""

    def __init__(self):
        self.psnr, self.ssim = [], []                      # per image, in the order added; PSNR may hold +inf
        self._mean_psnr = []                               # the same with +inf replaced (psnr_for_mean)
        self._last = None

    def add(self, pred, target):
        """pred: the prediction on the device, float32 in [0, 1] or uint8, [B,H,W,C] (or [B,H,W]); target: the same shape as a
        NumPy float array in [0, 1], a NumPy uint8 array or a device tensor.  One `ops.image_metrics` call; returns the
        batch's (psnr, ssim) as float64 arrays."""
        import torch
        from . import ops
        if not torch.is_tensor(target):
            target = np.ascontiguousarray(target)
            if target.dtype != np.uint8:
                target = target.astype(np.float32, copy=False)
            target = torch.from_numpy(target).to(pred.device)
        elif target.dtype not in (torch.uint8, torch.float32):
            target = target.float()
        if pred.dtype not in (torch.uint8, torch.float32):
            pred = pred.float()
        if pred.dim() == 3:
            pred = pred.unsqueeze(-1)
        if target.dim() == 3:
            target = target.unsqueeze(-1)
        m = ops.image_metrics(pred, target)
        B, H, W, C = (int(v) for v in pred.shape)
        sums = torch.stack((m.sad.double(), m.ssd.double(), m.ssim_sum)).cpu().numpy()       # exact: ssd <= 65025 n < 2^53
        _, _, psnr, ssim = derive(sums[0], sums[1], sums[2], H, W, C)
        self.psnr.extend(psnr.tolist())
        self.ssim.extend(ssim.tolist())
        self._mean_psnr.extend(psnr_for_mean(psnr, H * W * C).tolist())
        self._last = (float(np.mean(self._mean_psnr[len(self._mean_psnr) - B:])) if B else float("nan"),
                      float(np.mean(ssim)) if B else float("nan"))
        return psnr, ssim

    def last(self):
        """(mean PSNR, mean SSIM) of the last batch added."""
        if self._last is None:
            raise ValueError("ValidationMetrics: nothing added yet")
        return self._last

    def line(self, prefix="Validation "):
        """The text for the last batch: `Validation PSNR <dB> SSIM <value>`, means over its images; repr precision, so the
        numbers parse back to the values of `last()`."""
        psnr, ssim = self.last()
        return "{0}PSNR {1!r} SSIM {2!r}".format(prefix, psnr, ssim)

    def epoch_means(self):
        """(mean PSNR, mean SSIM) over every image added.  An image pair with ssd = 0 has PSNR +inf; it enters the mean as the
        PSNR at ssd = 0.5 (psnr_for_mean), so the mean stays finite and ordered."""
        if not self.ssim:
            raise ValueError("ValidationMetrics: nothing added yet")
        return float(np.mean(self._mean_psnr)), float(np.mean(self.ssim))


class ShapeMetricsLog(object):
    """Accumulates the shape metrics of voxel grids against their targets (`ops.voxel_shape_metrics`, rn_voxel_shape_metrics):
    IoU, chamfer distance and Hausdorff distance in voxels, and the F-score at `tau` voxels.

        log = ShapeMetricsLog(threshold=(0.1, 0.5)); log.add(pred, target); print(log.line())
    """
    NAMES = ("iou", "chamfer", "hausdorff", "fscore")

    def __init__(self, threshold=0.5, tau=1.0):
        self.threshold, self.tau = threshold, tau
        self.rows = []                                     # one dict per pair, in the order added (ShapeMetrics.as_dicts)

    def add(self, pred, target):
        """pred, target: grids [B,S,S,S,1] (or [B,S,S,S]) on the device, float32 or uint8; the target may be a NumPy array.
        One `ops.voxel_shape_metrics` call; returns the batch's dicts."""
        import torch
        from . import ops
        if not torch.is_tensor(target):
            target = np.ascontiguousarray(target)
            if target.dtype != np.uint8:
                target = target.astype(np.float32, copy=False)
            target = torch.from_numpy(target).to(pred.device)
        rows = ops.voxel_shape_metrics(pred, target, threshold=self.threshold, tau=self.tau).as_dicts()
        self.rows.extend(rows)
        return rows

    def means(self):
        """{name: mean over every pair added}; a pair with an empty surface has NaN distances and leaves those means out (a mean
        over no pair is NaN)."""
        if not self.rows:
            raise ValueError("ShapeMetricsLog: nothing added yet")
        out = {}
        for name in self.NAMES:
            vals = [r[name] for r in self.rows if r[name] == r[name]]
            out[name] = float(np.mean(vals)) if vals else float("nan")
        return out

    def line(self, prefix=""):
        """`Shape IoU <v> chamfer <v> hausdorff <v> F <v>`: the means over what was added, repr precision."""
        return shape_line(self.means(), prefix)


def shape_line(values, prefix=""):
    """The log line of one {name: value} dict of shape metrics."""
    return "{0}Shape IoU {1!r} chamfer {2!r} hausdorff {3!r} F {4!r}".format(
        prefix, float(values["iou"]), float(values["chamfer"]), float(values["hausdorff"]), float(values["fscore"]))
