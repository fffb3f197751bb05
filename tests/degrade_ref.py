"""numpy restatements (float64) of the OpenCV operations behind the reference's training degradations, for the tests of
vspbfr_amd/degrade.py.  TEST INFRASTRUCTURE: cv2 is not a dependency of this project; each function names the OpenCV behaviour it follows."""
import io

import numpy as np


def filter2d(plane, taps):
    """cv2.filter2D(img, -1, kernel) on one float plane: CORRELATION (the kernel is not flipped), anchor at the kernel centre
    (anchor=(-1, -1)), border BORDER_REFLECT_101 (the default; numpy's 'reflect' mode is the same rule: ... 2 1 | 0 1 2 ... n-2 | n-1 n-2 ...),
    taps as given (cv2 uses float32 taps for a float32 image), accumulated here in float64."""
    K = taps.shape[0]
    r = K // 2
    pad = np.pad(plane.astype(np.float64), r, mode="reflect")
    h, w = plane.shape
    out = np.zeros((h, w), np.float64)
    t = taps.astype(np.float64)
    for ky in range(K):
        for kx in range(K):
            out += t[ky, kx] * pad[ky:ky + h, kx:kx + w]
    return out


def linear_coeffs(dst, src, clamp_fraction):
    """cv2.resize INTER_LINEAR coefficients (imgproc/src/resize.cpp, resizeGeneric set-up): scale = 1 / (dst / src) in double,
    f = float32((d + 0.5) * scale - 0.5), s = floor(f), f -= s.  Along x, s < 0 and s >= src - 1 pin the fraction to 0 (xofs / alpha
    set-up); along y the fraction stays and the two source rows are clamped into [0, src - 1] (the row fetch of the invoker)."""
    scale = 1.0 / (float(dst) / float(src))
    f = ((np.arange(dst) + 0.5) * scale - 0.5).astype(np.float32)
    s = np.floor(f).astype(np.int64)
    f = (f - s.astype(np.float32)).astype(np.float32)
    if clamp_fraction:
        lo = s < 0
        s[lo], f[lo] = 0, 0
        hi = s >= src - 1
        s[hi], f[hi] = src - 1, 0
    i0 = np.clip(s, 0, src - 1)
    i1 = np.clip(s + 1, 0, src - 1)
    return i0, i1, (np.float32(1) - f).astype(np.float64), f.astype(np.float64)


def resize_linear(img, dh, dw, f32=False):
    """cv2.resize(img, (dw, dh), interpolation=INTER_LINEAR) of a float (C, h, w) array: horizontal pass, then vertical
    (HResizeLinear / VResizeLinear: s0 * w0 + s1 * w1), in float64, or with f32=True in float32 with every product and sum rounded
    as the scalar code of resize.cpp rounds them.  (For an exact 2x reduction cv2 switches to INTER_AREA, whose 2x2 mean is the same
    value up to rounding.)"""
    c, h, w = img.shape
    x0, x1, a0, a1 = linear_coeffs(dw, w, True)
    y0, y1, b0, b1 = linear_coeffs(dh, h, False)
    t = np.float32 if f32 else np.float64
    img, a0, a1, b0, b1 = (v.astype(t) for v in (img, a0, a1, b0, b1))
    hp = img[:, :, x0] * a0 + img[:, :, x1] * a1
    return hp[:, y0, :] * b0[:, None] + hp[:, y1, :] * b1[:, None]


def bgr2gray(img):
    """cv2.cvtColor(img, COLOR_BGR2GRAY) of a (3, h, w) array whose channel 0 cv2 reads as blue: 0.114 c0 + 0.587 c1 + 0.299 c2"""
    return 0.114 * img[0] + 0.587 * img[1] + 0.299 * img[2]


def round_u8(x):
    """saturate_cast<uchar> of a float (cvRound: half to even) and numpy's round: clip(rint(x), 0, 255)"""
    return np.clip(np.rint(x), 0, 255)


def jpeg_cv2(img_chw_u8, quality):
    """cv2.imdecode(cv2.imencode('.jpg', img, [IMWRITE_JPEG_QUALITY, q]), 1) of a (3, h, w) uint8 array cv2 reads as BGR: PIL's
    libjpeg-turbo at the same defaults, with the channels reversed around the codec."""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img_chw_u8.transpose(1, 2, 0)[..., ::-1])).save(buf, "JPEG", quality=int(quality))
    buf.seek(0)
    return np.ascontiguousarray(np.asarray(Image.open(buf).convert("RGB"))[..., ::-1].transpose(2, 0, 1))


def philox_normals(seed, step, slot, sample, n):
    """The item noise of vsp_degrade_down_u8: element e of the (dh, dw, 3) draw = Box-Muller normal e % 4 of Philox4x32-10 with
    key (seed_lo ^ 0x44475244, seed_hi), counter (e / 4, step << 2 | slot, sample_lo, sample_hi).  Returns (float32 values, words)."""
    from oracle.device_rng import _u01, philox4x32_10
    q = (n + 3) // 4
    seed = int(seed) & (2 ** 64 - 1)
    c1 = np.uint32(((int(step) << 2) | (int(slot) & 3)) & 0xFFFFFFFF)
    w = philox4x32_10(np.arange(q, dtype=np.uint32), c1, np.uint32(int(sample) & 0xFFFFFFFF), np.uint32(int(sample) >> 32),
                      (seed & 0xFFFFFFFF) ^ 0x44475244, seed >> 32)
    two_pi = np.float32(6.283185307179586)
    r0 = np.sqrt(np.float32(-2.0) * np.log(_u01(w[0])))
    r1 = np.sqrt(np.float32(-2.0) * np.log(_u01(w[2])))
    t0, t1 = two_pi * _u01(w[1]), two_pi * _u01(w[3])
    v = np.stack([r0 * np.cos(t0), r0 * np.sin(t0), r1 * np.cos(t1), r1 * np.sin(t1)], axis=1).astype(np.float32).reshape(-1)[:n]
    return v, np.stack(w, axis=1).reshape(-1)[:n]


def degrade_chain(gt_chw, p, noise_hwc):
    """The whole of dataset.py:327-373 for one image with the parameters fixed: gt (3, H, W) float in [0, 1], p a
    vspbfr_amd.degrade.LQParams, noise_hwc (dh, dw, 3) standard normals.  Returns (3, H, W) float64, multiples of 1/255."""
    from vspbfr_amd.degrade import lq_taps
    taps = lq_taps(p) if p.taps is None else np.asarray(p.taps, np.float32)
    x = np.stack([filter2d(gt_chw[c], taps) for c in range(3)])
    if p.haze:
        x = x * np.float32(p.alpha) + (1 - np.float32(p.alpha))
    dh, dw = p.size
    x = resize_linear(x, dh, dw)
    x = np.clip(x + noise_hwc.transpose(2, 0, 1).astype(np.float64) * (np.float32(p.sigma) / 255.0), 0, 1)
    u8 = round_u8(x * 255).astype(np.uint8)
    j = jpeg_cv2(u8, p.quality).astype(np.float32) / np.float32(255)
    up = resize_linear(j, gt_chw.shape[1], gt_chw.shape[2])
    return round_u8(up * 255) / 255.0
