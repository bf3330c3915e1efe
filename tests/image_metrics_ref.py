"""NumPy twin of rn_image_metrics (include/rendernet_hip.h states the rule): byte quantisation, the exact sums sad and ssd,
the five integer window moments in uint64, the central moments with wrap-around subtraction, and the float64 SSIM quotient.
Also a big-integer evaluation of the moments of one window (Python's unbounded integers) and the standard float64 SSIM with the
unquantised Gaussian that the integer weights are compared against."""
import numpy as np

WEIGHTS = (4, 31, 147, 448, 872, 1092, 872, 448, 147, 31, 4)       # RN_SSIM_WEIGHTS
T = 1 << 24
K1, K2 = 6.5025, 58.5225                                            # RN_SSIM_K1, RN_SSIM_K2
C1, C2 = K1 * 2.0 ** 48, K2 * 2.0 ** 48


def gaussian():
    """The normalised 1-D Gaussian of Wang et al.: 11 taps, sigma = 1.5, float64."""
    d = np.arange(-5, 6, dtype=np.float64)
    g = np.exp(-d * d / (2.0 * 1.5 * 1.5))
    return g / g.sum()


def weights_from_rule():
    """w_d = rint(4096 g_d) for |d| = 1..5, w_0 = 4096 - 2 sum_{d >= 1} w_d."""
    w = [int(v) for v in np.rint(4096.0 * gaussian())]
    w[5] = 4096 - 2 * sum(w[6:])
    return tuple(w)


def quantise(x):
    """float image -> bytes: rint(min(max(255 x, 0), 255)), the multiply in float32, half to even, NaN -> 0.  uint8 passes."""
    x = np.asarray(x)
    if x.dtype == np.uint8:
        return x
    v = np.float32(255.0) * x.astype(np.float32)
    v = np.where(v > 0, v, np.float32(0))                           # a NaN fails the comparison
    v = np.where(v < 255, v, np.float32(255))
    return np.rint(v).astype(np.uint8)


def _window_sums(x):
    """x uint64 [B,H,W,C] -> sum over the 11 x 11 window with weights w_i w_j at the (H-10) x (W-10) valid centres."""
    w = np.asarray(WEIGHTS, np.uint64)
    H, W = x.shape[1], x.shape[2]
    h = sum(w[d] * x[:, :, d:d + W - 10] for d in range(11))
    return sum(w[d] * h[:, d:d + H - 10] for d in range(11))


def moments(a, b):
    """a, b bytes [B,H,W,C] -> (A, B, Saa, Sbb, Sab) uint64 [B,H-10,W-10,C]."""
    a, b = a.astype(np.uint64), b.astype(np.uint64)
    return _window_sums(a), _window_sums(b), _window_sums(a * a), _window_sums(b * b), _window_sums(a * b)


def ssim_map(a, b):
    """The SSIM of every window, float64 [B,H-10,W-10,C], from the integer moments as the header evaluates it."""
    A, B, Saa, Sbb, Sab = moments(a, b)
    Tu = np.uint64(T)
    Va, Vb = Tu * Saa - A * A, Tu * Sbb - B * B                     # uint64, exact (>= 0)
    Cab = (Tu * Sab - A * B).view(np.int64)                         # wraps to the signed value
    dA, dB = A.astype(np.float64), B.astype(np.float64)
    num = (2.0 * dA * dB + C1) * (2.0 * Cab.astype(np.float64) + C2)
    den = (dA * dA + dB * dB + C1) * (Va.astype(np.float64) + Vb.astype(np.float64) + C2)
    return num / den


def image_metrics(a, b):
    """a, b [B,H,W,C] uint8 or float -> dict of per-image arrays: sad, ssd (int64), ssim_sum, l1, mse, psnr, ssim (float64)."""
    a, b = quantise(a), quantise(b)
    assert a.shape == b.shape and a.ndim == 4 and a.shape[3] in (1, 3) and a.shape[1] >= 11 and a.shape[2] >= 11
    Bn, H, W, C = a.shape
    d = a.astype(np.int64) - b.astype(np.int64)
    sad = np.abs(d).reshape(Bn, -1).sum(1)
    ssd = (d * d).reshape(Bn, -1).sum(1)
    ssim_sum = ssim_map(a, b).reshape(Bn, -1).sum(1) if Bn else np.zeros((0,), np.float64)
    n, n_win = float(H * W * C), float((H - 10) * (W - 10) * C)
    mse = ssd / n
    with np.errstate(divide="ignore"):
        psnr = 10.0 * np.log10(65025.0 / mse)
    return {"sad": sad, "ssd": ssd, "ssim_sum": ssim_sum, "l1": sad / (255.0 * n), "mse": mse, "psnr": psnr,
            "ssim": ssim_sum / n_win}


def window_moments_bigint(a, b):
    """The moments of ONE 11 x 11 window (a, b bytes [11,11]) in Python's unbounded integers: a dict with A, B, Saa, Sbb, Sab,
    the products T Saa, T Sbb, T Sab, AA, BB, AB, and Va, Vb, Cab."""
    out = dict(A=0, B=0, Saa=0, Sbb=0, Sab=0)
    for i in range(11):
        for j in range(11):
            w, x, y = WEIGHTS[i] * WEIGHTS[j], int(a[i, j]), int(b[i, j])
            out["A"] += w * x
            out["B"] += w * y
            out["Saa"] += w * x * x
            out["Sbb"] += w * y * y
            out["Sab"] += w * x * y
    out.update(TSaa=T * out["Saa"], TSbb=T * out["Sbb"], TSab=T * out["Sab"], AA=out["A"] ** 2, BB=out["B"] ** 2,
               AB=out["A"] * out["B"])
    out.update(Va=out["TSaa"] - out["AA"], Vb=out["TSbb"] - out["BB"], Cab=out["TSab"] - out["AB"])
    return out


def standard_ssim_mean(a, b):
    """Mean SSIM of two byte images [H,W] in float64 with the unquantised Gaussian window (Wang et al.: valid region, K1 = 0.01,
    K2 = 0.03, L = 255, weighted second moments): what the integer weights approximate."""
    g = gaussian()
    a, b = a.astype(np.float64), b.astype(np.float64)

    def blur(x):
        H, W = x.shape
        h = sum(g[d] * x[:, d:d + W - 10] for d in range(11))
        return sum(g[d] * h[d:d + H - 10] for d in range(11))

    mu_a, mu_b = blur(a), blur(b)
    va, vb, cab = blur(a * a) - mu_a * mu_a, blur(b * b) - mu_b * mu_b, blur(a * b) - mu_a * mu_b
    s = ((2 * mu_a * mu_b + K1) * (2 * cab + K2)) / ((mu_a * mu_a + mu_b * mu_b + K1) * (va + vb + K2))
    return float(s.mean())
