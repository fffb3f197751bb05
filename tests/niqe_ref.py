"""NumPy float64 restatement of NIQE (Mittal, Soundararajan, Bovik 2013, the form everybody runs) -- the oracle of the device
kernel (vspbfr_amd/csrc/niqe.hip) and of vspbfr_amd/niqe.py.  Written from the definition, slow and plain on purpose.

    luma -> crop to multiples of 96 -> two scales (the second: MATLAB imresize(., 0.5), bicubic, antialiased) -> per scale the
    7 x 7 Gaussian local normalisation (MSCN) -> per block an asymmetric generalised Gaussian (AGGD) fit of the block and of its
    products with four circularly shifted copies -> 36 features per block -> mean / covariance over blocks -> distance to a model.

`plain_fp32` restates the smooth part (MSCN and the raw moments) in torch CPU float32 with no care taken: what the format
costs on a well-conditioned input; the GPU test scales its bound by that error, measured, not assumed."""
import numpy as np
from scipy.special import gamma as G

BLOCK = 96
SHIFTS = ((0, 1), (1, 0), (1, 1), (1, -1))
GAM = 0.2 + 0.001 * np.arange(9801)
R_GAM = G(2.0 / GAM) ** 2 / (G(1.0 / GAM) * G(3.0 / GAM))
HALF_TAPS = np.array([-3, -9, 29, 111, 111, 29, -9, -3], dtype=np.float64) / 256.0
TINY = 1e-9


def luma(u8):
    """(H, W, 3) uint8 -> (H, W) float64 of integers: round-half-even(16 + (65.481 R + 128.553 G + 24.966 B) / 255), exactly"""
    p = u8.astype(np.int64)
    n = 65481 * p[..., 0] + 128553 * p[..., 1] + 24966 * p[..., 2]
    q, rem = np.divmod(n, 255000)
    up = (2 * rem > 255000) | ((2 * rem == 255000) & (q % 2 == 1))
    return (16 + q + up).astype(np.float64)


def crop(y, crop_border=0):
    if crop_border:
        y = y[crop_border:-crop_border, crop_border:-crop_border]
    h, w = y.shape
    return y[:h // BLOCK * BLOCK, :w // BLOCK * BLOCK]


def gauss_taps():
    k = np.arange(7) - 3.0
    g = np.exp(-k * k / (2.0 * (7.0 / 6.0) ** 2))
    return g / g.sum()


def gauss_window():
    """the 7 x 7 window: the normalised outer product of the 1-D taps"""
    g = np.exp(-(np.arange(7) - 3.0) ** 2 / (2.0 * (7.0 / 6.0) ** 2))
    w = np.outer(g, g)
    return w / w.sum()


def gauss_filter(x):
    """7 x 7 Gaussian, edge replicate: separable, rows of the window then columns"""
    g = gauss_taps()
    h, w = x.shape
    p = np.pad(x, 3, mode="edge")
    t = sum(g[k] * p[:, k:k + w] for k in range(7))
    return sum(g[k] * t[k:k + h, :] for k in range(7))


def cubic(x, a=-0.5):
    x = np.abs(x)
    return np.where(x <= 1, (a + 2) * x ** 3 - (a + 3) * x ** 2 + 1, np.where(x < 2, a * x ** 3 - 5 * a * x ** 2 + 8 * a * x - 4 * a, 0.0))


def half_taps_from_cubic():
    """the antialiased bicubic weights of output sample i at scale 1/2: centre u = 2 i + 0.5, support 2 i - 3 .. 2 i + 4, the kernel
    stretched by 2 and normalised -- independent of i"""
    u = 0.5
    idx = np.arange(-3, 5)
    w = 0.5 * cubic(0.5 * (u - idx))
    return w / w.sum()


def _half_axis0(x):
    n = x.shape[0]
    p = np.pad(x, ((3, 4), (0, 0)), mode="symmetric")   # -1 -> 0, -2 -> 1; n -> n - 1
    return sum(HALF_TAPS[k] * p[k:k + n:2, :][:n // 2] for k in range(8))


def imresize_half(x):
    """MATLAB imresize(x, 0.5): rows first, then columns"""
    return _half_axis0(_half_axis0(x).T).T


def mscn(x):
    mu = gauss_filter(x)
    sd = np.sqrt(np.abs(gauss_filter(x * x) - mu * mu))
    return (x - mu) / (sd + 1.0), sd


def lookup(rnorm):
    """index of the first minimum of (r(gamma) - rnorm)^2"""
    return int(np.argmin((R_GAM - rnorm) ** 2))


def smooth_of(v):
    """(left_std, right_std, rnorm) of one map"""
    v = v.ravel()
    with np.errstate(invalid="ignore", divide="ignore"):
        ls = np.sqrt(np.mean(v[v < 0] ** 2)) if (v < 0).any() else np.nan
        rs = np.sqrt(np.mean(v[v > 0] ** 2)) if (v > 0).any() else np.nan
        gh = ls / rs
        rhat = np.mean(np.abs(v)) ** 2 / np.mean(v ** 2)
        rnorm = rhat * (gh ** 3 + 1) * (gh + 1) / (gh ** 2 + 1) ** 2
    return ls, rs, rnorm


def aggd_from(ls, rs, rnorm, k=None):
    """(alpha index, alpha, beta_l, beta_r); k: take this grid point instead of looking rnorm up"""
    if k is None:
        k = 0 if np.isnan(rnorm) else lookup(rnorm)
    a = GAM[k]
    s = np.sqrt(G(1.0 / a) / G(3.0 / a))
    return k, a, ls * s, rs * s


def features_from_smooth(sm, fixed=None):
    """18 features of one block and scale from its (5, 3) smooth quantities, and the 5 alpha indices (`fixed`: given, not looked up)"""
    out, ks = [], []
    for m in range(5):
        k, a, bl, br = aggd_from(*sm[m], k=None if fixed is None else int(fixed[m]))
        ks.append(k)
        out += [a, (bl + br) / 2.0] if m == 0 else [a, (br - bl) * G(2.0 / a) / G(1.0 / a), bl, br]
    return np.array(out), ks


def block_maps(block):
    return [block] + [block * np.roll(block, s, axis=(0, 1)) for s in SHIFTS]


def analyse(u8, crop_border=0):
    """One (H, W, 3) uint8 image -> dict: features (nblk, 36), sharpness (nblk,), smooth (nblk, 2, 5, 3) = left_std, right_std, rnorm,
    alpha_idx (nblk, 2, 5), tiny = the number of MSCN / product samples with |v| < 1e-9."""
    y = crop(luma(u8), crop_border)
    nby, nbx = y.shape[0] // BLOCK, y.shape[1] // BLOCK
    nblk = nby * nbx
    feats = np.zeros((nblk, 36))
    smooth = np.zeros((nblk, 2, 5, 3))
    aidx = np.zeros((nblk, 2, 5), dtype=np.int64)
    sharp = np.zeros(nblk)
    tiny = 0
    for s, img in enumerate((y, imresize_half(y))):
        v, sd = mscn(img)
        n = BLOCK >> s
        for b in range(nblk):
            by, bx = divmod(b, nbx)
            sl = (slice(by * n, by * n + n), slice(bx * n, bx * n + n))
            if s == 0:
                sharp[b] = sd[sl].mean()
            for m, mp in enumerate(block_maps(v[sl])):
                tiny += int((np.abs(mp) < TINY).sum())
                smooth[b, s, m] = smooth_of(mp)
            feats[b, 18 * s:18 * s + 18], aidx[b, s] = features_from_smooth(smooth[b, s])
    return {"features": feats, "sharpness": sharp, "smooth": smooth, "alpha_idx": aidx, "tiny": tiny}


def score(feats, mu_p, cov_p):
    rows = feats[~np.isnan(feats).any(axis=1)]
    mu = rows.mean(axis=0)
    cov = np.cov(rows, rowvar=False)
    d = (np.asarray(mu_p).reshape(-1) - mu)[None, :]
    return float(np.sqrt(d @ np.linalg.pinv((np.asarray(cov_p) + cov) / 2.0) @ d.T)[0, 0])


def features_with_alpha(smooth, alpha_idx):
    """(nblk, 36) features from (nblk, 2, 5, 3) smooth quantities with the shape parameters held at the grid points alpha_idx (nblk, 2, 5)"""
    return np.stack([np.concatenate([features_from_smooth(smooth[b, s], alpha_idx[b, s])[0] for s in range(2)]) for b in range(smooth.shape[0])])


def sharp_mask(sharpness, share=0.75):
    return sharpness > share * sharpness.max()


def fit(analyses, share=0.75):
    """pristine model of a list of `analyse` results: the sharp blocks of every image, NaN rows dropped"""
    rows = []
    for a in analyses:
        keep = a["features"][sharp_mask(a["sharpness"], share)]
        rows.append(keep[~np.isnan(keep).any(axis=1)])
    rows = np.concatenate(rows)
    return rows.mean(axis=0), np.cov(rows, rowvar=False)


def smooth_from_raw(mom, n):
    mom = np.asarray(mom, dtype=np.float64)
    with np.errstate(invalid="ignore", divide="ignore"):
        ls, rs = np.sqrt(mom[..., 1] / mom[..., 0]), np.sqrt(mom[..., 3] / mom[..., 2])
        gh = ls / rs
        rhat = (mom[..., 4] / n) ** 2 / (mom[..., 5] / n)
        rnorm = rhat * (gh ** 3 + 1) * (gh + 1) / (gh ** 2 + 1) ** 2
    return np.stack([ls, rs, rnorm], axis=-1)


def plain_fp32(u8, crop_border=0):
    """The smooth quantities (nblk, 2, 5, 3) from a plain float32 restatement in torch on the CPU: no shift, no float64 anywhere"""
    import torch
    import torch.nn.functional as F
    y = torch.from_numpy(crop(luma(u8), crop_border)).to(torch.float32)
    g = torch.from_numpy(gauss_taps()).to(torch.float32)
    win = torch.outer(g, g)[None, None]
    ht = torch.from_numpy(HALF_TAPS).to(torch.float32)

    def gfilt(x):
        return F.conv2d(F.pad(x[None, None], (3, 3, 3, 3), mode="replicate"), win)[0, 0]

    def half0(x):
        n = x.shape[0]
        p = torch.cat([x[:3].flip(0), x, x[-4:].flip(0)], 0)
        return sum(ht[k] * p[k:k + n:2][:n // 2] for k in range(8))

    nby, nbx = y.shape[0] // BLOCK, y.shape[1] // BLOCK
    out = np.zeros((nby * nbx, 2, 5, 3))
    for s, img in enumerate((y, half0(half0(y).T).T)):
        mu = gfilt(img)
        v = (img - mu) / (torch.sqrt(torch.abs(gfilt(img * img) - mu * mu)) + 1.0)
        n = BLOCK >> s
        for b in range(nby * nbx):
            by, bx = divmod(b, nbx)
            blk = v[by * n:by * n + n, bx * n:bx * n + n]
            for m, mp in enumerate([blk] + [blk * torch.roll(blk, s_, dims=(0, 1)) for s_ in SHIFTS]):
                ls = torch.sqrt(torch.mean(mp[mp < 0] ** 2))
                rs = torch.sqrt(torch.mean(mp[mp > 0] ** 2))
                gh = ls / rs
                rhat = torch.mean(torch.abs(mp)) ** 2 / torch.mean(mp ** 2)
                out[b, s, m] = (float(ls), float(rs), float(rhat * (gh ** 3 + 1) * (gh + 1) / (gh ** 2 + 1) ** 2))
    return out


# ------------------------------------------------------------------------------------------------ the cases of the GPU tests
def case_image(kind, h, w, seed):
    """(h, w, 3) uint8 test image.  white: uniform noise; smooth: low-frequency waves + Gaussian noise; bright: mean 225 +- 4 clipped to
    235; half: the left half constant (100), the right half white noise."""
    rng = np.random.default_rng(seed)
    if kind == "white":
        return rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    if kind == "smooth":
        yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
        base = 128 + 30 * np.sin(2 * np.pi * yy / 211.0 + 0.3) * np.cos(2 * np.pi * xx / 173.0 + 1.1)
        img = base[..., None] + np.array([4.0, -3.0, 7.0]) + rng.normal(0, 12, (h, w, 3))
        return np.clip(np.rint(img), 0, 255).astype(np.uint8)
    if kind == "bright":
        return np.clip(np.rint(225 + rng.normal(0, 4, (h, w, 3))), 0, 235).astype(np.uint8)
    if kind == "half":
        img = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
        img[:, :w // 2] = 100
        return img
    raise ValueError(kind)
