"""NumPy restatement of Pillow's 8-bit LANCZOS resize (libImaging/Resample.c): the tables of vspbfr_amd.resample.lanczos_coeffs, a
horizontal and then a vertical pass of clip8((2**21 + sum(pixel * k)) >> 22) with int64 accumulation and a uint8 image between the
passes.  The oracle of the device kernel besides live PIL."""
import numpy as np

from vspbfr_amd.resample import PRECISION_BITS, lanczos_coeffs


def _pass(img, out_size):
    """resample axis 1 of a (rows, in, C) uint8 array"""
    xmin, count, taps = lanczos_coeffs(img.shape[1], out_size)
    ksize = taps.shape[1]
    # gather index (out, ksize); taps beyond count are zero, so their (clamped) pixels do not matter
    idx = np.minimum(xmin[:, None].astype(np.int64) + np.arange(ksize)[None, :], img.shape[1] - 1)
    acc = np.full((img.shape[0], out_size, img.shape[2]), 1 << (PRECISION_BITS - 1), dtype=np.int64)
    for k in range(ksize):
        acc += img[:, idx[:, k], :].astype(np.int64) * taps[:, k].astype(np.int64)[None, :, None]
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def resize(arr, nw, nh):
    """uint8 (h, w, C) -> uint8 (nh, nw, C), Image.resize((nw, nh), LANCZOS)"""
    arr = np.asarray(arr, dtype=np.uint8)
    tmp = _pass(arr, nw)
    return np.ascontiguousarray(_pass(tmp.transpose(1, 0, 2), nh).transpose(1, 0, 2))


def resize_crop(arr, nw, nh, x0, y0, H, W, flip=False):
    arr = np.asarray(arr, dtype=np.uint8)
    if flip:
        arr = arr[:, ::-1]
    if arr.shape[:2] == (nh, nw):
        return np.ascontiguousarray(arr[y0:y0 + H, x0:x0 + W])
    return np.ascontiguousarray(resize(arr, nw, nh)[y0:y0 + H, x0:x0 + W])


def to_tensor_f32(u8):
    """imageio._to_tensor's arithmetic on every element of a uint8 array: three separately rounded fp32 operations"""
    v = np.asarray(u8).astype(np.float32)
    return ((v / np.float32(255.0)) - np.float32(0.5)) / np.float32(0.5)


def test_image(w, h, seed):
    """random uint8 (h, w, 3) with rows of 0 and of 255 mixed in (both ends of clip8 are reached by the filter's overshoot)"""
    rng = np.random.default_rng(seed)
    a = rng.integers(0, 256, (h, w, 3), dtype=np.uint8)
    for r in range(h):
        m = r % 5
        if m == 1:
            a[r] = 0
        elif m == 3:
            a[r] = 255
    if w >= 8:
        a[:, w // 3:w // 3 + 2] = 255
        a[:, w // 3 + 2:w // 3 + 4] = 0
    return a


test_image.__test__ = False   # a helper, not a test

# (source w, h) -> (resized w, h): the size pairs of the issue, shared by the CPU and the GPU tests
SIZE_PAIRS = [((1, 1), (8, 8)), ((7, 5), (16, 16)), ((40, 33), (64, 77)), ((64, 48), (43, 32)), ((97, 61), (64, 64)),
              ((513, 777), (512, 775)), ((300, 200), (768, 512)), ((1024, 1024), (512, 512)), ((1024, 64), (64, 4)), ((64, 64), (64, 64))]
SWEEP = [((w, 8), (32, 8)) for w in range(33, 161)]
