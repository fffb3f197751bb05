"""Training degradations on the device: the low-quality (LQ) synthesis of the reference's training datasets.

The reference makes each LQ face on the host with cv2 / numpy (dataset.py:327-373 `degrade_img` of `ImageFolder_restore_free_form`,
dataset.py:83-127 in `ImageFolder_restore` without the haze step):
    blur (random 39x39 / 41x41 iso / aniso Gaussian) -> haze (p 0.008) -> INTER_LINEAR down by U(0.8, 8) -> + N(0, U(0, 20) / 255),
    clip -> JPEG at int(U(60, 100)) -> INTER_LINEAR back up -> round to 8 bits.
Here:
  * every scalar of that list is drawn on the host from a counter-based generator keyed by (seed, step, global sample index, slot)
    (`sample_rng`, `sample_lq`): no global `random` / `np.random` state, so a sample is degraded the same way on any rank at any world
    size;
  * the taps are built in float64 exactly as `bivariate_Gaussian` does (my_degradations.py:76-98), rounded to fp32 (what cv2.filter2D
    uses for a float32 image) and uploaded with the per-item table in one pinned copy (`DegradePlan`);
  * the chain runs as five launches over the whole ragged batch (csrc/degrade.hip): blur, down + noise, two for the JPEG round trip,
    up + round.  The Gaussian noise is drawn in the kernel (Philox4x32-10 keyed by (seed, sample, step, slot)) unless injected.
`degrade(gt, lqs, ...)` is the explicit-parameter form; vspbfr_amd.trainset serves the reference's two dataset classes on top of it.
"""
import ctypes as C
import dataclasses
import math

import numpy as np
import torch

from . import _lib
from . import hip_ops as H

_RNG_DOMAIN = 0x44454752414445  # second key word of the host draws ("DEGRADE")


@dataclasses.dataclass(frozen=True)
class DegradeParams:
    """The degradation settings of the reference's dataset classes (dataset.py:28-43 / :221-241).  Colour jitter and Poisson noise are
    off in both and not offered; the unused kernel types (generalized, plateau, sinc) neither."""
    blur_kernel_size: tuple = (19, 20)       # K = randint(19, 20) * 2 + 1
    kernel_list: tuple = ("iso", "aniso")
    kernel_prob: tuple = (0.5, 0.5)
    blur_sigma: tuple = (0.1, 10.0)
    downsample_range: tuple = (0.8, 8.0)
    noise_range: tuple = (0.0, 20.0)
    jpeg_range: tuple = (60.0, 100.0)
    gray_prob: float = 0.0                   # ImageFolder_restore: None
    hazy_prob: float = 0.0                   # ImageFolder_restore: no haze step
    hazy_alpha: tuple = (0.75, 0.95)

    @classmethod
    def free_form(cls):
        """ImageFolder_restore_free_form (dataset.py:221-241)"""
        return cls(gray_prob=0.008, hazy_prob=0.008)

    @classmethod
    def restore(cls):
        """ImageFolder_restore (dataset.py:28-43)"""
        return cls()


@dataclasses.dataclass
class LQParams:
    """Every random scalar of one degrade_img call."""
    ksize: int
    iso: bool
    sig_x: float
    sig_y: float
    theta: float
    scale: float
    size: tuple          # (dh, dw) = (int(h // scale), int(w // scale))
    sigma: float         # noise std on the 0..255 scale
    quality: int
    haze: bool = False
    alpha: float = 1.0
    taps: object = None  # explicit (ksize, ksize) taps instead of the Gaussian of (sig_x, sig_y, theta, iso)


def sample_rng(seed, step, index, slot):
    """numpy Generator over Philox4x32-10 with key (seed, domain) and counter (step, index, slot, 0): a pure function of its four
    arguments.  Slot 0 holds a sample's flip / crop / grey draws, slot s >= 1 the parameters of its s-th LQ image."""
    if min(int(seed), int(step), int(index), int(slot)) < 0:
        raise ValueError("sample_rng: seed, step, index and slot are non-negative")
    key = np.array([int(seed) & (2 ** 64 - 1), _RNG_DOMAIN], dtype=np.uint64)
    counter = np.array([int(step), int(index), int(slot), 0], dtype=np.uint64)
    return np.random.Generator(np.random.Philox(counter=counter, key=key))


def sample_lq(params, im_size, rng):
    """The draws of one degrade_img call, in the reference's order (dataset.py:330-352 and the functions it calls)."""
    h, w = int(im_size[0]), int(im_size[1])
    lo, hi = params.blur_kernel_size
    ksize = int(rng.integers(lo, hi + 1)) * 2 + 1
    prob = np.asarray(params.kernel_prob, dtype=np.float64)
    kind = params.kernel_list[int(np.searchsorted(np.cumsum(prob) / prob.sum(), rng.random(), side="right"))]
    if kind not in ("iso", "aniso"):
        raise ValueError(f"kernel type {kind!r} is not supported (iso / aniso only)")
    iso = kind == "iso"
    sig_x = float(rng.uniform(*params.blur_sigma))
    sig_y, theta = (sig_x, 0.0) if iso else (float(rng.uniform(*params.blur_sigma)), float(rng.uniform(-math.pi, math.pi)))
    haze, alpha = False, 1.0
    if params.hazy_prob and rng.random() < params.hazy_prob:
        haze, alpha = True, float(rng.uniform(*params.hazy_alpha))
    scale = float(rng.uniform(*params.downsample_range))
    size = (int(h // scale), int(w // scale))
    sigma = float(rng.uniform(*params.noise_range))
    quality = int(rng.uniform(*params.jpeg_range))
    return LQParams(ksize, iso, sig_x, sig_y, theta, scale, size, sigma, quality, haze, alpha)


def bivariate_gaussian(ksize, sig_x, sig_y, theta, isotropic=True):
    """Normalised K x K Gaussian density in float64, evaluated as my_degradations.py:30-44 (grid), :18-27 (covariance) and :47-59, :76-98
    (density, normalisation) evaluate it, so the result is bit-identical."""
    half = ksize // 2
    ax = np.arange(-half, half + 1.0)
    xx, yy = np.meshgrid(ax, ax)
    grid = np.stack([xx, yy], axis=-1)
    if isotropic:
        cov = np.array([[sig_x ** 2, 0], [0, sig_x ** 2]])
    else:
        rot = np.array([[np.cos(theta), -np.sin(theta)], [np.sin(theta), np.cos(theta)]])
        cov = np.dot(rot, np.dot(np.array([[sig_x ** 2, 0], [0, sig_y ** 2]]), rot.T))
    k = np.exp(-0.5 * np.sum(np.dot(grid, np.linalg.inv(cov)) * grid, 2))
    return k / np.sum(k)


def lq_taps(p):
    return bivariate_gaussian(p.ksize, p.sig_x, p.sig_y, p.theta, p.iso).astype(np.float32)


def _mcus(dh, dw):
    return ((dh + 15) // 16) * ((dw + 15) // 16)


class DegradePlan:
    """Host table of one ragged batch: n items (LQ images), item i made from gt image src[i] with parameters lqs[i].  Holds the sizes
    of every device buffer the stages need and uploads the item table + taps in one pinned copy."""

    def __init__(self, lqs, src, im_size, batch, samples=None, slots=None, grey=None):
        n = len(lqs)
        if not 0 < n <= _lib.DEGRADE_MAX_ITEMS or len(src) != n:
            raise ValueError(f"DegradePlan: 1..{_lib.DEGRADE_MAX_ITEMS} items with one source each")
        self.n, self.H, self.W, self.B = n, int(im_size[0]), int(im_size[1]), int(batch)
        if not (0 < self.H <= _lib.DEGRADE_MAX_SIZE and 0 < self.W <= _lib.DEGRADE_MAX_SIZE):
            raise ValueError(f"DegradePlan: image size {im_size}")
        samples = list(range(n)) if samples is None else [int(s) for s in samples]
        slots = [0] * n if slots is None else [int(s) for s in slots]
        grey = [False] * n if grey is None else [bool(g) for g in grey]
        self.items = (_lib.DegradeItem * n)()
        taps, tap_off, pix, mcu, jpg = [], 0, 0, 0, 0
        self.sizes, self.offsets = [], []
        for i, (p, s) in enumerate(zip(lqs, src)):
            dh, dw = int(p.size[0]), int(p.size[1])
            if not 0 <= int(s) < self.B:
                raise ValueError(f"item {i}: source {s} outside the batch of {self.B}")
            if not (p.ksize % 2 == 1 and 1 <= p.ksize <= _lib.DEGRADE_MAX_KSIZE):
                raise ValueError(f"item {i}: kernel size {p.ksize} (odd, <= {_lib.DEGRADE_MAX_KSIZE})")
            if not (1 <= dh <= _lib.DEGRADE_MAX_SIZE and 1 <= dw <= _lib.DEGRADE_MAX_SIZE):
                raise ValueError(f"item {i}: downsampled size {(dh, dw)}")
            if not 1 <= int(p.quality) <= 100 or not 0 <= slots[i] <= 3 or samples[i] < 0:
                raise ValueError(f"item {i}: quality {p.quality}, slot {slots[i]}, sample {samples[i]}")
            t = lq_taps(p) if p.taps is None else np.asarray(p.taps, dtype=np.float32)
            if t.shape != (p.ksize, p.ksize):
                raise ValueError(f"item {i}: taps {t.shape}")
            it = self.items[i]
            it.tap_off, it.pix_off, it.jpg_off, it.sample = tap_off, pix, jpg, samples[i]
            it.src, it.ksize, it.dh, it.dw, it.quality = int(s), p.ksize, dh, dw, int(p.quality)
            it.flags = (_lib.DEGRADE_HAZE if p.haze else 0) | (_lib.DEGRADE_GREY if grey[i] else 0)
            it.mcu0, it.slot, it.alpha, it.sigma = mcu, slots[i], float(p.alpha), float(p.sigma)
            taps.append(t.reshape(-1))
            self.sizes.append((dh, dw))
            self.offsets.append(pix)
            tap_off += t.size
            pix += 3 * dh * dw
            mcu += _mcus(dh, dw)
            jpg += ((dh + 15) // 16 * 16) * ((dw + 15) // 16 * 16) * 3 // 2
        if pix >= 2 ** 31 or mcu >= 2 ** 31:
            raise ValueError("DegradePlan: batch too large for one launch")
        self.lq_elems, self.total_mcus, self.work_bytes = pix, mcu, jpg
        self.max_pixels = max(dh * dw for dh, dw in self.sizes)
        self.taps = np.concatenate(taps)
        self._dev = None

    def upload(self, device):
        """items + taps -> device in one copy from pinned memory (enqueued on the current stream)."""
        nb = C.sizeof(self.items)
        head = (nb + 15) // 16 * 16
        host = torch.empty(head + self.taps.nbytes, dtype=torch.uint8, pin_memory=True)
        hv = host.numpy()
        hv[:nb] = np.frombuffer(bytes(self.items), dtype=np.uint8)
        hv[head:] = self.taps.view(np.uint8)
        dev = host.to(device, non_blocking=True)
        self._dev = (dev[:nb], dev[head:].view(torch.float32))
        return self._dev

    def split(self, flat, dtype=None):
        """ragged (lq_elems,) -> list of per-item tensors: (3, dh, dw) for the uint8 image, (dh, dw, 3) for noise / pre values"""
        out = []
        for (dh, dw), off in zip(self.sizes, self.offsets):
            v = flat[off:off + 3 * dh * dw]
            out.append(v.view(3, dh, dw) if flat.dtype == torch.uint8 else v.view(dh, dw, 3))
        return out


def pack_noise(plan, noise, device):
    """list of n (dh, dw, 3) arrays / tensors -> ragged fp32 device tensor"""
    flat = torch.empty(plan.lq_elems, dtype=torch.float32)
    for (dh, dw), off, z in zip(plan.sizes, plan.offsets, noise):
        z = torch.as_tensor(np.asarray(z, dtype=np.float32) if not isinstance(z, torch.Tensor) else z.float().cpu())
        if tuple(z.shape) != (dh, dw, 3):
            raise ValueError(f"noise of shape {tuple(z.shape)} for an item of size {(dh, dw)}")
        flat[off:off + 3 * dh * dw] = z.reshape(-1)
    return flat.to(device)


def run_plan(plan, gt, seed=0, step=0, noise=None, stages=False):
    """The five launches of one ragged batch on gt (B, 3, H, W) fp32 in [0, 1] -> (n, 3, H, W).  stages=True also returns the
    intermediates: blurred (n, 3, H, W), pre (ragged fp32 before the noise), down (ragged uint8 before the JPEG), jpeg (after it)."""
    if gt.dim() != 4 or tuple(gt.shape[1:]) != (3, plan.H, plan.W) or gt.shape[0] != plan.B:
        raise ValueError(f"gt {tuple(gt.shape)} does not match the plan ({plan.B}, 3, {plan.H}, {plan.W})")
    items, taps = plan.upload(gt.device)
    blurred = H.degrade_blur(gt, taps, items, plan.n)
    if noise is not None and not isinstance(noise, torch.Tensor):
        noise = pack_noise(plan, noise, gt.device)
    lq = H.degrade_down(blurred, items, plan.n, plan.lq_elems, plan.max_pixels, seed, step, noise=noise, pre=stages)
    if stages:
        lq, pre = lq
        down = lq.clone()
    H.degrade_jpeg(lq, items, plan.n, plan.total_mcus, plan.work_bytes, plan.max_pixels)
    out = H.degrade_up(lq, items, plan.n, plan.H, plan.W)
    if stages:
        return out, {"blurred": blurred, "pre": pre, "down": down, "jpeg": lq}
    return out


def degrade(gt, lqs, src=None, seed=0, step=0, samples=None, slots=None, grey=None, noise=None, stages=False):
    """Explicit-parameter form: gt (B, 3, H, W) fp32 on the device, lqs = one LQParams per output image (src[i]: its gt image, default
    i), noise: optional list of (dh, dw, 3) standard normals per item (else drawn in the kernel keyed by (seed, samples[i], step,
    slots[i])).  Returns (n, 3, H, W) fp32, multiples of 1/255 unless grey."""
    B = gt.shape[0]
    src = list(range(len(lqs))) if src is None else list(src)
    plan = DegradePlan(lqs, src, gt.shape[2:], B, samples=samples, slots=slots, grey=grey)
    return run_plan(plan, gt.contiguous(), seed, step, noise, stages)
