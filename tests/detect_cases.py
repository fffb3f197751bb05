"""The shared cases of the detector tests: built once per process, never written to."""
import functools

import numpy as np
import torch

import detect_ref as R

SEED, CLASS_BIAS = 7, 0.3            # chosen so that the margins of test_detect_ref.test_margins_of_the_gpu_detection_case hold
HC, WC, SIDE = 96, 128, 128
THRESHOLD, NMS = 0.5, 0.4


@functools.lru_cache(maxsize=None)
def model():
    return R.make_model(SEED, CLASS_BIAS)


@functools.lru_cache(maxsize=None)
def detection_case():
    """Two photos, one of them larger than SIDE; the canvas the detector must build (the larger one through Pillow's LANCZOS), the
    network's outputs in float64 and float32 and the restated detections of both -> dict"""
    from PIL import Image
    a, b = R.test_photo(96, 128, 5), R.test_photo(150, 200, 6)
    br = np.asarray(Image.fromarray(b).resize((128, 96), Image.Resampling.LANCZOS))
    x = R.canvas([a, br], HC, WC)
    net = model()
    with torch.no_grad():
        o64 = [t.numpy() for t in net(x)]
        o32 = [t.numpy() for t in R.as_f32(net)(x.float())]
    det = []
    for k in range(2):
        d64 = R.decode(o64[0][k], o64[1][k], o64[2][k], HC, WC, np.float64)
        d32 = R.decode(o32[0][k], o32[1][k], o32[2][k], HC, WC, np.float32)
        det.append({"d64": d64, "d32": d32, "r64": R.select_nms(*d64, THRESHOLD, NMS), "r32": R.select_nms(*d32, THRESHOLD, NMS)})
    return {"photos": [a, b], "canvas_photos": [a, br], "geo": [(96, 128, 96, 128), (150, 200, 96, 128)], "o64": o64, "o32": o32, "det": det}


def synthetic_heads(seed=3):
    """(conf (3, P, 2), loc (3, P, 4), lm (3, P, 10)) float32 for the 96 x 128 canvas.  Image 0: a quiet background with three planted
    clusters of overlapping high-score priors; image 1: logits on a grid of 0.25, so that hundreds of candidates share scores and the
    caps cut through ties; image 2: no candidate."""
    rng = np.random.default_rng(seed)
    P = sum(2 * h * w for h, w in R.level_sizes(HC, WC))
    conf = np.zeros((3, P, 2), dtype=np.float32)
    loc = (0.3 * rng.standard_normal((3, P, 4))).astype(np.float32)
    lm = (0.5 * rng.standard_normal((3, P, 10))).astype(np.float32)
    conf[:, :, 0] = 4.0
    n0 = 2 * 12 * 16                                         # level 1: 6 x 8 cells of step 16
    for ci, cj in ((1, 1), (3, 5), (4, 2)):
        for di in (-1, 0, 1):
            for dj in (-1, 0, 1):
                for a in (0, 1):
                    p = n0 + 2 * ((ci + di) * 8 + cj + dj) + a
                    conf[0, p] = (0.0, rng.uniform(0.5, 4.0))
    conf[1, :, 0] = 0.0
    conf[1, :, 1] = np.rint(rng.uniform(-2.0, 2.0, P) * 4.0) / 4.0
    return conf, loc, lm
