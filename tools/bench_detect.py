"""The face detector (vspbfr_amd/detect.py, csrc/detect.hip) on 8 photos of 1024 x 1536 at --side 1024 and 640, random weights:

  network      device time of RetinaFaceDetector.network on a canvas made beforehand (HIP events, median of 30 after a warm-up), and of
               every layer class alone: its launches replayed on the tensors of one forward pass
  eager        the same folded network in torch-ROCm eager fp32 on the same GPU in the same run (tests/detect_ref.folded_forward on the
               uploaded folded weights), whole and per layer class -- the yardstick
  postprocess  vsp_det_decode_nms_f32 on the network's outputs at threshold 0.5 (the random weights give hundreds of candidates)
  detect       one detect() call from a packed device buffer: resize, network, post-processing, the read-back (events and wall time)
  share        of a 39 ms pipeline step
  cli          the loop of vspbfr_amd.restore_photos over the 8 photos with --landmarks against --detect_weights (--batch 8 --timesteps 4
               --no_sample, threshold 0.5, two faces per photo), alternating, three each after a warm run

    python tools/bench_detect.py [--out profiles/detect_bench.json] [--skip-cli]
"""
import argparse
import json
import os
import random
import statistics
import sys
import tempfile
import time
from argparse import Namespace

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
PIPELINE_STEP_MS = 39.0
CLASSES = {"det_entry_u8": "entry", "det_sep": "separable", "det_conv3x3": "dense3x3", "det_lateral": "lateral", "det_heads": "heads"}


def events(fn, n=30, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    med = statistics.median(ms)
    return {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "percent_of_pipeline_step": round(100.0 * med / PIPELINE_STEP_MS, 3)}


def record_launches(det, sources, B, Hc, Wc):
    """one forward pass with every hip_ops.det_* call noted: {class: [closure that repeats the launch]}"""
    from vspbfr_amd import hip_ops as H
    calls, saved = {c: [] for c in CLASSES.values()}, {}
    for name, cls in CLASSES.items():
        fn = saved[name] = getattr(H, name)

        def wrapped(*a, _fn=fn, _cls=cls, **kw):
            calls[_cls].append(lambda: _fn(*a, **kw))
            return _fn(*a, **kw)
        setattr(H, name, wrapped)
    try:
        det.network(sources, B, Hc, Wc)
    finally:
        for name, fn in saved.items():
            setattr(H, name, fn)
    return calls


def eager_classes(folded, x):
    """the same forward pass in torch eager, by layer class: {class: [closure]} on the tensors of one pass"""
    import detect_ref as R
    F = torch.nn.functional
    calls = {c: [] for c in CLASSES.values()}
    saved = {n: getattr(R, n) for n in ("sep_ref", "conv3x3_ref", "lateral_ref", "heads_ref")}
    conv2d = F.conv2d
    first = []

    def note(cls, fn):
        def wrapped(*a, **kw):
            calls[cls].append(lambda: fn(*a, **kw))
            return fn(*a, **kw)
        return wrapped
    R.sep_ref, R.conv3x3_ref = note("separable", saved["sep_ref"]), note("dense3x3", saved["conv3x3_ref"])
    R.lateral_ref, R.heads_ref = note("lateral", saved["lateral_ref"]), note("heads", saved["heads_ref"])

    def entry_conv(inp, w, b=None, stride=1, padding=0, dilation=1, groups=1):
        if inp.shape[1] == 3 and not first:
            first.append(1)
            calls["entry"].append(lambda: R.lrelu(conv2d(inp, w, b, stride, padding), 0.1))
        return conv2d(inp, w, b, stride, padding, dilation, groups)
    F.conv2d = entry_conv
    try:
        with torch.no_grad():
            R.folded_forward(folded, x)
    finally:
        F.conv2d = conv2d
        for n, fn in saved.items():
            setattr(R, n, fn)
    return calls


def bench_side(det, photos, side):
    import detect_ref as R
    from vspbfr_amd import hip_ops as H
    flat = torch.from_numpy(np.concatenate([p.reshape(-1) for p in photos])).cuda()
    offsets = np.concatenate([[0], np.cumsum([p.size for p in photos])])[:-1].tolist()
    sizes = [p.shape[:2] for p in photos]
    sources, B, Hc, Wc, geo = det.canvas(device_photos=(flat, offsets, sizes), side=side)
    res = {"side": side, "photos": len(photos), "photo_hw": list(sizes[0]), "canvas": [B, Hc, Wc], "priors": H.det_priors(Hc, Wc)}
    res["canvas_build"] = events(lambda: det.canvas(device_photos=(flat, offsets, sizes), side=side))
    res["network"] = events(lambda: det.network(sources, B, Hc, Wc))
    conf, loc, lm = det.network(sources, B, Hc, Wc)
    launches = record_launches(det, sources, B, Hc, Wc)
    res["network_by_class"] = {c: dict(events(lambda: [f() for f in fs]), launches=len(fs)) for c, fs in launches.items()}
    # the yardstick: the canvas as a float tensor (the resized photos read back once), the folded weights in fp32 on the device
    x = torch.zeros((B, 3, Hc, Wc), device="cuda")
    mean = torch.tensor(R.MEAN_BGR, device="cuda").view(3, 1, 1)
    for buf, items in sources:
        for off, h, w, slot in items:
            x[slot, :, :h, :w] = buf[off:off + 3 * h * w].view(h, w, 3).permute(2, 0, 1).flip(0).float() - mean
    folded = det.p
    with torch.no_grad():
        ref = R.folded_forward(folded, x)
        res["eager_vs_hip_max_abs"] = [float((a - b).abs().max()) for a, b in zip(ref, (conf, loc, lm))]
        res["eager"] = events(lambda: R.folded_forward(folded, x))
        eager = eager_classes(folded, x)
        res["eager_by_class"] = {c: dict(events(lambda: [f() for f in fs]), launches=len(fs)) for c, fs in eager.items()}
    res["hip_over_eager"] = {c: round(res["network_by_class"][c]["median_ms"] / res["eager_by_class"][c]["median_ms"], 3) for c in launches}
    res["hip_over_eager"]["network"] = round(res["network"]["median_ms"] / res["eager"]["median_ms"], 3)
    res["postprocess"] = events(lambda: H.det_decode_nms(conf, loc, lm, Hc, Wc, 0.5, 0.4, 1024, 256))
    info = H.det_decode_nms(conf, loc, lm, Hc, Wc, 0.5, 0.4, 1024, 256)[1].cpu().numpy()
    res["postprocess"].update(candidates=info[:, 2].tolist(), faces=info[:, 0].tolist(), status=info[:, 1].tolist())
    res["detect_call"] = events(lambda: det.detect(device_photos=(flat, offsets, sizes), side=side, threshold=0.5))
    wall = []
    for _ in range(10):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        det.detect(device_photos=(flat, offsets, sizes), side=side, threshold=0.5)
        wall.append((time.perf_counter() - t0) * 1e3)
    res["detect_call"]["wall_ms_median"] = round(statistics.median(wall), 3)
    return res


def bench_cli(tmp, det, photos):
    import bench_photo
    from vspbfr_amd import restore_photos as RP
    restorer, root, names, landmarks, device = bench_photo.cli_setup(tmp, *bench_photo.workload())
    params = dict(threshold=0.5, nms=0.4, side=1024, max_faces=2, min_face=0.0)
    times, faces = {"landmarks": [], "detect": []}, {}
    for rep in range(4):                       # the first of each is the warm run
        for route in ("landmarks", "detect"):
            args = Namespace(photos=root, out=os.path.join(tmp, f"out_{route}_{rep}"), batch=8, save_faces=False, upscale=1, size=512, inset=8,
                             feather=48, antialias=False)
            torch.manual_seed(123)
            random.seed(123)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            if route == "detect":
                rep_ = RP.restore_photos(args, restorer, names, {}, device, detector=det, detect_params=params)
            else:
                rep_ = RP.restore_photos(args, restorer, names, landmarks, device)
            torch.cuda.synchronize()
            faces[route] = sum(p["faces"] for p in rep_)
            if rep:
                times[route].append(round(time.perf_counter() - t0, 4))
    return {"what": "8 photos of 1024 x 1536, --batch 8 --timesteps 4 --no_sample, decode + (detect) + restore + PNG, writers drained, "
                    "alternating, three each after a warm run", "cpus_used": len(os.sched_getaffinity(0)), "faces": faces,
            "loop_s": times, "loop_median_s": {r: statistics.median(t) for r, t in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-cli", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_detect: no GPU")
    import bench_photo
    import detect_cases as K
    from vspbfr_amd.detect import RetinaFaceDetector
    det = RetinaFaceDetector(K.model().state_dict(), "cuda")
    photos, _ = bench_photo.workload()
    res = {"what": "RetinaFace mobilenet0.25 (random weights) on 8 photos of 1024 x 1536; HIP events, median of 30 after a warm-up; torch eager "
                   "fp32 in the same run", "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "runs": []}
    for side in (1024, 640):
        r = bench_side(det, photos, side)
        print(json.dumps(r), flush=True)
        res["runs"].append(r)
    if not a.skip_cli:
        with tempfile.TemporaryDirectory() as d:
            res["cli"] = bench_cli(d, det, photos)
        print(json.dumps(res["cli"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
