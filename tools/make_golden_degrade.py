"""Writes tests/golden/degrade.npz: fixtures of the training degradation chain (vspbfr_amd/degrade.py, csrc/degrade.hip).

BUILD-CONTAINER ONLY (imports the reference through tools/refshim.py).  Contents:
  kernels        `bivariate_Gaussian` (reference my_basicsr/my_degradations.py:76-98) for a set of (K, sigma_x, sigma_y, theta, iso)
                 cases: kernel_params (n, 5), kernels (n, 41, 41) float64, centred, zero outside the K x K window
  mixed          `random_mixed_kernels(('iso', 'aniso'), [0.5, 0.5], K, [0.1, 10], [0.1, 10], [-pi, pi], noise_range=None)`
                 (my_degradations.py:295-356) drawn after random.seed(s) / np.random.seed(s): mixed_seeds (m,), mixed_ksize (m,),
                 mixed_kernels (m, 41, 41)
  jpeg_*         PIL JPEG round trips of fixed uint8 HWC images with the channels reversed around the codec, i.e. what
                 cv2.imdecode(cv2.imencode('.jpg', img)) returns for an array cv2 reads as BGR (my_degradations.py:681-710):
                 jpeg_in_<h>x<w> (h, w, 3), jpeg_out_<h>x<w>_q<q> (h, w, 3)
PIL's codec is libjpeg-turbo at the defaults cv2 uses (4:2:0, ISLOW, baseline tables, fancy upsampling on decode).
"""
import io
import math
import os
import random
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
sys.path.insert(0, HERE)

KERNEL_CASES = [(41, 2.0, 2.0, 0.0, 1), (39, 0.1, 0.1, 0.0, 1), (41, 10.0, 10.0, 0.0, 1), (41, 3.5, 0.7, 0.6, 0),
                (39, 9.9, 0.2, -2.9, 0), (41, 0.15, 7.0, 3.1, 0), (3, 1.0, 1.0, 0.0, 1), (21, 4.0, 1.5, 1.0, 0)]
MIXED_SEEDS = list(range(12))
JPEG_SIZES = [(64, 64), (65, 91), (100, 57), (640, 640)]
JPEG_QUALITIES = [60, 61, 75, 90, 99]
JPEG_QUALITIES_LARGE = [60, 99]   # 640 x 640: two qualities keep the fixture small; the GPU test adds live PIL round trips


def jpeg_image(h, w, seed):
    """a face-like test pattern: smooth colour field + edges + mild texture; the large image is a mosaic of 20 x 20 flat tiles
    (edges that cross the 8 x 8 blocks and the MCUs), which keeps the fixture small"""
    rng = np.random.default_rng(seed)
    if h * w > 100000:
        tiles = rng.integers(30, 225, (h // 20 + 1, w // 20 + 1, 3)).astype(np.uint8)
        return np.ascontiguousarray(np.kron(tiles, np.ones((20, 20, 1), np.uint8))[:h, :w])
    y, x = np.mgrid[0:h, 0:w].astype(np.float64)
    chans = []
    for c in range(3):
        f = 120 + 70 * np.sin(x / (9.0 + 3 * c) + c) * np.cos(y / (13.0 - 2 * c) - c)
        f += 40 * (((x - w / 2) ** 2 + (y - h / 2) ** 2) < (min(h, w) / 3) ** 2)
        chans.append(f)
    img = np.stack(chans, -1) + rng.normal(0, 6, (h, w, 3))
    return np.clip(img, 0, 255).round().astype(np.uint8)


def pil_cv2_jpeg(img, q):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img[..., ::-1])).save(buf, "JPEG", quality=int(q))
    buf.seek(0)
    return np.ascontiguousarray(np.asarray(Image.open(buf).convert("RGB"))[..., ::-1])


def pad41(k):
    out = np.zeros((41, 41), np.float64)
    o = (41 - k.shape[0]) // 2
    out[o:o + k.shape[0], o:o + k.shape[1]] = k
    return out


def main():
    import refshim
    refshim.install()
    if "torchvision.transforms.functional" not in sys.modules:   # my_degradations.py:8 imports it; the kernels never call it
        tv = sys.modules.get("torchvision") or types.ModuleType("torchvision")
        tr = types.ModuleType("torchvision.transforms")
        fn = types.ModuleType("torchvision.transforms.functional")
        fn.rgb_to_grayscale = None
        tv.transforms, tr.functional = tr, fn
        sys.modules.update({"torchvision": tv, "torchvision.transforms": tr, "torchvision.transforms.functional": fn})
    from my_basicsr import my_degradations as deg
    out = {}
    out["kernel_params"] = np.array(KERNEL_CASES, np.float64)
    out["kernels"] = np.stack([pad41(deg.bivariate_Gaussian(int(k), sx, sy, th, isotropic=bool(iso))) for k, sx, sy, th, iso in KERNEL_CASES])
    ks, mk = [], []
    for s in MIXED_SEEDS:
        random.seed(s)
        np.random.seed(s)
        k = random.randint(19, 20) * 2 + 1
        ks.append(k)
        mk.append(pad41(deg.random_mixed_kernels(('iso', 'aniso'), [0.5, 0.5], k, [0.1, 10], [0.1, 10], [-math.pi, math.pi],
                                                 noise_range=None)))
    out["mixed_seeds"], out["mixed_ksize"], out["mixed_kernels"] = np.array(MIXED_SEEDS), np.array(ks), np.stack(mk)
    for i, (h, w) in enumerate(JPEG_SIZES):
        img = jpeg_image(h, w, 100 + i)
        out[f"jpeg_in_{h}x{w}"] = img
        for q in (JPEG_QUALITIES_LARGE if h * w > 100000 else JPEG_QUALITIES):
            out[f"jpeg_out_{h}x{w}_q{q}"] = pil_cv2_jpeg(img, q)
    path = os.path.join(ROOT, "tests", "golden", "degrade.npz")
    np.savez_compressed(path, **out)
    print("wrote", path, os.path.getsize(path), "bytes", len(out), "arrays")


if __name__ == "__main__":
    main()
