"""float64 NumPy / SciPy restatement of the pixel metrics of vspbfr_amd.metrics from their published definitions -- the oracle of
tests/test_metrics_ref.py (CPU, closed forms) and tests/test_metrics_gpu.py (the HIP kernel).

PSNR: 10 log10(peak^2 / mse), peak = 255 (the reference's my_lpips.psnr(p0, p1, 255.)).

SSIM (Wang, Bovik, Sheikh, Simoncelli 2004), per channel, on 8-bit data, data range L = 255:
    S = ((2 ux uy + C1)(2 vxy + C2)) / ((ux^2 + uy^2 + C1)(vx + vy + C2)),   C1 = (0.01 L)^2, C2 = (0.03 L)^2
with ux = w * x, vx = k (w * x^2 - ux^2), vxy = k (w * xy - ux uy) for a window w that sums to 1, averaged over the window
positions that lie wholly inside the image (scikit-image crops (win - 1) / 2 pixels off every side) and then over the channels:
    "uniform7": 7 x 7 box, k = 49 / 48 (sample covariance)   -- scikit-image's structural_similarity defaults; the box filter is
                scipy.ndimage.uniform_filter, the very function scikit-image calls;
    "gauss11":  11 x 11 separable Gaussian, sigma 1.5, taps exp(-d^2 / (2 sigma^2)) normalised to sum 1, k = 1 -- the paper's
                window; scikit-image with gaussian_weights=True, use_sample_covariance=False (truncate 3.5 -> radius 5)."""
import numpy as np
from scipy import ndimage

C1 = (0.01 * 255.0) ** 2
C2 = (0.03 * 255.0) ** 2
WIN = {"uniform7": 7, "gauss11": 11}


def gauss_taps(size=11, sigma=1.5):
    d = np.arange(size, dtype=np.float64) - (size - 1) / 2
    t = np.exp(-(d * d) / (2.0 * sigma * sigma))
    return t / t.sum()


def _filter(img, window, mode):
    """window-weighted local mean of a 2-D float64 array, same size as the input (the border rows depend on `mode`)."""
    if window == "uniform7":
        return ndimage.uniform_filter(img, size=7, mode=mode)
    t = gauss_taps()
    return ndimage.correlate1d(ndimage.correlate1d(img, t, axis=0, mode=mode), t, axis=1, mode=mode)


def ssim_map(x, y, window="gauss11", mode="reflect"):
    """S at every VALID window position of two 2-D arrays: shape (H - w + 1, W - w + 1)."""
    w = WIN[window]
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    if x.shape != y.shape or x.ndim != 2 or min(x.shape) < w:
        raise ValueError(f"ssim_map: two 2-D arrays of one shape, at least {w} x {w} (got {x.shape}, {y.shape})")
    k = 49.0 / 48.0 if window == "uniform7" else 1.0
    ux, uy = _filter(x, window, mode), _filter(y, window, mode)
    vx = k * (_filter(x * x, window, mode) - ux * ux)
    vy = k * (_filter(y * y, window, mode) - uy * uy)
    vxy = k * (_filter(x * y, window, mode) - ux * uy)
    s = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    p = (w - 1) // 2
    return s[p:s.shape[0] - p, p:s.shape[1] - p]


def ssim(a, b, window="gauss11", mode="reflect"):
    """Mean SSIM of two (H, W) or (H, W, C) uint8 images: mean over the channels of the mean over the valid positions."""
    a, b = np.asarray(a), np.asarray(b)
    if a.ndim == 2:
        a, b = a[..., None], b[..., None]
    return float(np.mean([ssim_map(a[..., c], b[..., c], window, mode).mean() for c in range(a.shape[2])]))


def sse(a, b):
    """Exact integer sum of squared differences of two uint8 arrays."""
    d = np.asarray(a).astype(np.int64) - np.asarray(b).astype(np.int64)
    return int((d * d).sum())


def psnr(a, b):
    """10 log10(255^2 / mse); None for identical images."""
    e = sse(a, b)
    return None if e == 0 else float(10.0 * np.log10(255.0 * 255.0 * np.asarray(a).size / e))


def ssim_fp32_naive(a, b, window="gauss11"):
    """The formulation a user would write with framework ops: five fp32 F.conv2d (x, y, xx, yy, xy, uncentred), evaluated by
    PyTorch on the CPU.  Not an oracle: tests/test_metrics_gpu.py measures ITS error against `ssim` to bound the kernel's."""
    import torch
    import torch.nn.functional as F
    a, b = np.asarray(a), np.asarray(b)
    if a.ndim == 2:
        a, b = a[..., None], b[..., None]
    x = torch.from_numpy(a.astype(np.float32)).permute(2, 0, 1)[:, None]
    y = torch.from_numpy(b.astype(np.float32)).permute(2, 0, 1)[:, None]
    if window == "uniform7":
        k2, cov = torch.full((1, 1, 7, 7), 1.0 / 49.0, dtype=torch.float32), 49.0 / 48.0
    else:
        t = torch.from_numpy(gauss_taps()).to(torch.float32)
        k2, cov = torch.outer(t, t)[None, None], 1.0
    ux, uy = F.conv2d(x, k2), F.conv2d(y, k2)
    vx = cov * (F.conv2d(x * x, k2) - ux * ux)
    vy = cov * (F.conv2d(y * y, k2) - uy * uy)
    vxy = cov * (F.conv2d(x * y, k2) - ux * uy)
    s = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return float(s.double().mean())


# ---------------------------------------------------------------------------------------------- the kernel tests' image pairs
def pair(kind, h, w, c=3, seed=0):
    """Seeded uint8 image pairs (h, w, c), c = 1 gives (h, w, 1):
    smooth      -- a low-frequency picture and a mildly blurred, noisy copy (an ordinary restoration);
    bright_flat -- mean ~230, contrast ~5 levels, the second image with +-12 uniform integer noise: the cancellation case of
                   E[x^2] - E[x]^2 in fp32;
    noise       -- two independent white-noise images;  identical -- a smooth image twice;  negative -- a against 255 - a."""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)

    def smooth():
        ch = []
        for k in range(c):
            f = 127 + 70 * np.sin(xx / (17.0 + 3 * k) + k) * np.cos(yy / (23.0 - 2 * k)) + 30 * np.sin((xx + 2 * yy) / 61.0)
            ch.append(f)
        return np.stack(ch, -1)

    q = lambda f: np.clip(np.rint(f), 0, 255).astype(np.uint8)
    if kind == "smooth":
        a = smooth()
        b = ndimage.gaussian_filter(a, (1.2, 1.2, 0)) + rng.normal(0, 4, a.shape)
        return q(a), q(b)
    if kind == "bright_flat":
        a = 230 + 2.5 * np.sin(xx / 9.0)[..., None] * np.cos(yy / 13.0)[..., None] + rng.uniform(-0.5, 0.5, (h, w, c))
        a = q(a)
        b = q(a.astype(np.int64) + rng.integers(-12, 13, (h, w, c)))
        return a, b
    if kind == "noise":
        return rng.integers(0, 256, (h, w, c), dtype=np.uint8), rng.integers(0, 256, (h, w, c), dtype=np.uint8)
    if kind == "identical":
        a = q(smooth())
        return a, a.copy()
    if kind == "negative":
        a = q(smooth() + rng.normal(0, 6, (h, w, c)))
        return a, (255 - a).astype(np.uint8)
    raise ValueError(kind)
