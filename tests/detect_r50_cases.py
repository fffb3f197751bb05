"""The shared cases of the ResNet-50 detector tests: built once per process, never written to."""
import functools

import numpy as np
import torch

import detect_r50_ref as R5
import detect_ref as R

SEED, CLASS_BIAS = 15, 0.8         # chosen so that the margins of test_detect_r50_ref.test_margins_of_the_gpu_detection_case hold
HC, WC, SIDE = 64, 96, 96
THRESHOLD, NMS = 0.5, 0.4


@functools.lru_cache(maxsize=None)
def model():
    return R5.make_model(SEED, CLASS_BIAS)


@functools.lru_cache(maxsize=None)
def state():
    return {k: v.clone() for k, v in model().state_dict().items()}


@functools.lru_cache(maxsize=None)
def folded():
    return R5.fold(state())


@functools.lru_cache(maxsize=None)
def detection_case():
    """Two photos, one of them larger than SIDE; the canvas the detector must build (the larger one through Pillow's LANCZOS), the
    network's outputs with the kernels' rounding points in float64 and float32 and the restated detections of both -> dict"""
    from PIL import Image
    a, b = R.test_photo(64, 96, 5), R.test_photo(100, 150, 6)
    br = np.asarray(Image.fromarray(b).resize((96, 64), Image.Resampling.LANCZOS))
    with torch.no_grad():
        o64 = [t.numpy() for t in R5.forward(folded(), [a, br], HC, WC, torch.float64)]
        o32 = [t.numpy() for t in R5.forward(folded(), [a, br], HC, WC, torch.float32)]
        alone = [t.numpy() for t in R5.forward(folded(), [a], HC, WC, torch.float64)]
    det = []
    for k in range(2):
        d64 = R.decode(o64[0][k], o64[1][k], o64[2][k], HC, WC, np.float64)
        d32 = R.decode(o32[0][k], o32[1][k], o32[2][k], HC, WC, np.float32)
        det.append({"d64": d64, "d32": d32, "r64": R.select_nms(*d64, THRESHOLD, NMS), "r32": R.select_nms(*d32, THRESHOLD, NMS)})
    return {"photos": [a, b], "canvas_photos": [a, br], "geo": [(64, 96, 64, 96), (100, 150, 64, 96)], "o64": o64, "o32": o32, "det": det,
            "alone64": alone}
