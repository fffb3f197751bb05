"""The ResNet-50 face detector (vspbfr_amd/detect_r50.py, csrc/detect_r50.hip) on 8 photos of 1024 x 1536 at --side 1024 and
640, random weights:

  network      device time of RetinaFaceR50Detector.network on a canvas made beforehand (HIP events, median of 30 after a warm-up), and of
               every layer class alone -- stem (with the pool), 1x1, 3x3 stride 1, 3x3 stride 2, strided 1x1 (the downsamples of layers
               2..4), FPN, SSH, heads -- as its launches replayed on the tensors of one forward pass, with the achieved TFLOP/s and the
               share of the f16 MFMA peak
  eager        the yardstick: the same layers in torch-ROCm eager fp16 channels-last on the same folded weights on the same GPU in the
               same run, per class and summed
  detect       one detect() call from a packed device buffer: resize, network, post-processing, the read-back; the MobileNet-0.25
               detector's detect() on the same photos beside it

    python tools/bench_detect_r50.py [--out profiles/detect_r50_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
F16_MFMA_PEAK_TFLOPS = 2500.0     # dense f16 / bf16 MFMA, MI355X
CLASSES = ("stem", "1x1", "3x3_s1", "3x3_s2", "1x1_s2", "fpn", "ssh", "heads")


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
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def conv_class(name, ksize, stride):
    if name.startswith("fpn."):
        return "fpn"
    if name.startswith("ssh"):
        return "ssh"
    return {(1, 1): "1x1", (1, 2): "1x1_s2", (3, 1): "3x3_s1", (3, 2): "3x3_s2"}[(ksize, stride)]


def record(det, sources, B, Hc, Wc):
    """one forward pass with every launch noted -> ({class: [closure that repeats the launch]}, {class: flop}, [conv descriptions])"""
    from vspbfr_amd import hip_ops as H
    calls, flop, convs, current = {c: [] for c in CLASSES}, {c: 0 for c in CLASSES}, [], [None]
    saved = {n: getattr(H, n) for n in ("det50_stem_u8", "det50_pool_f16", "det50_conv_f16", "det50_heads")}
    inner = det._conv

    def named_conv(name, *a, **kw):
        current[0] = name
        return inner(name, *a, **kw)

    def note(fn, cls_of):
        def wrapped(*a, **kw):
            cls = cls_of(a, kw)
            calls[cls].append(lambda: fn(*a, **kw))
            return fn(*a, **kw)
        return wrapped

    def conv_cls(a, kw):
        w_img, stride = a[9], (a[11] if len(a) > 11 else kw.get("stride", 1))
        k, cin, cout = (1 if w_img.shape[0] == 1 else 3), 32 * w_img.shape[1], 16 * w_img.shape[2]
        oh, ow = H.det50_out_size(a[7], a[8], stride)
        cls = conv_class(current[0], k, stride)
        relu = a[12] if len(a) > 12 else kw.get("relu", False)
        flop[cls] += 2 * a[6] * oh * ow * cout * cin * k * k
        convs.append(dict(cls=cls, name=current[0], B=a[6], H=a[7], W=a[8], cin=cin, cout=cout, k=k, stride=stride, relu=bool(relu),
                          res=kw.get("res") is not None, up=kw.get("up") is not None))
        return cls

    def heads_cls(a, kw):
        flop["heads"] += 2 * a[2] * a[3] * a[4] * 256 * 32
        return "heads"

    def stem_cls(a, kw):
        flop["stem"] += 2 * a[4] * ((a[8] + 1) // 2) * ((a[9] + 1) // 2) * 147 * 64
        return "stem"
    H.det50_stem_u8, H.det50_pool_f16 = note(saved["det50_stem_u8"], stem_cls), note(saved["det50_pool_f16"], lambda a, kw: "stem")
    H.det50_conv_f16, H.det50_heads = note(saved["det50_conv_f16"], conv_cls), note(saved["det50_heads"], heads_cls)
    det._conv = named_conv
    try:
        det.network(sources, B, Hc, Wc)
    finally:
        del det._conv
        for n, fn in saved.items():
            setattr(H, n, fn)
    return calls, flop, convs


def eager_calls(det, convs, B, Hc, Wc):
    """the same layers in torch eager fp16 channels-last on the folded weights: {class: [closure]}"""
    from vspbfr_amd import detect_r50 as D5
    F = torch.nn.functional
    calls = {c: [] for c in CLASSES}
    g = torch.Generator(device="cuda").manual_seed(1)

    def act(b, c, h, w):
        return torch.randn((b, c, h, w), device="cuda", dtype=torch.float16, generator=g).contiguous(memory_format=torch.channels_last)
    for d in convs:
        w = D5.unpack_conv_weight(det.p[d["name"] + ".w"]).contiguous(memory_format=torch.channels_last)
        b = det.p[d["name"] + ".b"].half()
        x = act(d["B"], d["cin"], d["H"], d["W"])
        oh, ow = (d["H"] - 1) // d["stride"] + 1, (d["W"] - 1) // d["stride"] + 1
        r = act(d["B"], d["cout"], oh, ow) if d["res"] else None
        u = act(d["B"], d["cout"], oh // 2, ow // 2) if d["up"] else None

        def run(x=x, w=w, b=b, r=r, u=u, d=d):
            y = F.conv2d(x, w, b, d["stride"], d["k"] // 2)
            if r is not None:
                y = y + r
            if d["relu"]:
                y = torch.relu_(y)
            if u is not None:
                y = y + F.interpolate(u, scale_factor=2, mode="nearest")
            return y
        calls[d["cls"]].append(run)
    x = act(B, 3, Hc, Wc)
    ws = det.p["body.conv1.w"].reshape(7, 7, 3, 64).permute(3, 2, 0, 1).half().contiguous(memory_format=torch.channels_last)
    bs = det.p["body.conv1.b"].half()
    calls["stem"].append(lambda: F.max_pool2d(torch.relu_(F.conv2d(x, ws, bs, 2, 3)), 3, 2, 1))
    for k, s in enumerate((8, 16, 32)):
        f = act(B, 256, Hc // s, Wc // s)
        wh = det.p[f"heads.{k}.w"].t().reshape(32, 256, 1, 1).half().contiguous(memory_format=torch.channels_last)
        bh = det.p[f"heads.{k}.b"].half()
        calls["heads"].append(lambda f=f, wh=wh, bh=bh: F.conv2d(f, wh, bh).permute(0, 2, 3, 1).contiguous())
    return calls


def rate(r, flop):
    tf = flop / r["median_ms"] / 1e9
    r.update(gflop=round(flop / 1e9, 2), tflops=round(tf, 1), percent_of_f16_mfma_peak=round(100 * tf / F16_MFMA_PEAK_TFLOPS, 2))
    return r


def bench_side(det, mnet, photos, side):
    flat = torch.from_numpy(np.concatenate([p.reshape(-1) for p in photos])).cuda()
    offsets = np.concatenate([[0], np.cumsum([p.size for p in photos])])[:-1].tolist()
    sizes = [p.shape[:2] for p in photos]
    dp = (flat, offsets, sizes)
    sources, B, Hc, Wc, _ = det.canvas(device_photos=dp, side=side)
    res = {"side": side, "photos": len(photos), "photo_hw": list(sizes[0]), "canvas": [B, Hc, Wc]}
    calls, flop, convs = record(det, sources, B, Hc, Wc)
    res["network"] = rate(events(lambda: det.network(sources, B, Hc, Wc)), sum(flop.values()))
    res["network"]["launches"] = sum(len(v) for v in calls.values())
    res["network_by_class"] = {c: dict(rate(events(lambda: [f() for f in calls[c]]), flop[c]), launches=len(calls[c])) for c in CLASSES}
    with torch.no_grad():
        eager = eager_calls(det, convs, B, Hc, Wc)
        res["eager_by_class"] = {c: dict(rate(events(lambda: [f() for f in eager[c]]), flop[c]), launches=len(eager[c])) for c in CLASSES}
    res["eager_sum_of_classes_ms"] = round(sum(v["median_ms"] for v in res["eager_by_class"].values()), 4)
    res["hip_sum_of_classes_ms"] = round(sum(v["median_ms"] for v in res["network_by_class"].values()), 4)
    res["hip_over_eager"] = {c: round(res["network_by_class"][c]["median_ms"] / res["eager_by_class"][c]["median_ms"], 3) for c in CLASSES}
    res["hip_over_eager"]["sum_of_classes"] = round(res["hip_sum_of_classes_ms"] / res["eager_sum_of_classes_ms"], 3)
    res["classes_that_lose_to_eager"] = [c for c in CLASSES if res["hip_over_eager"][c] > 1.0]
    res["detect_call"] = events(lambda: det.detect(device_photos=dp, side=side, threshold=0.5))
    res["mobilenet_detect_call"] = events(lambda: mnet.detect(device_photos=dp, side=side, threshold=0.5))
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_detect_r50: no GPU")
    import bench_photo
    import detect_cases as K0
    import detect_r50_cases as K
    from vspbfr_amd.detect import RetinaFaceDetector
    from vspbfr_amd.detect_r50 import RetinaFaceR50Detector
    det, mnet = RetinaFaceR50Detector(K.state(), "cuda"), RetinaFaceDetector(K0.model().state_dict(), "cuda")
    photos, _ = bench_photo.workload()
    res = {"what": "RetinaFace resnet50 (random weights) on 8 photos of 1024 x 1536; HIP events, median of 30 after a warm-up; torch eager fp16 "
                   "channels-last on the same folded weights in the same run; a class is its launches replayed on the tensors of one pass",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "peaks_used": {"f16_mfma_tflops": F16_MFMA_PEAK_TFLOPS}, "runs": []}
    for side in (1024, 640):
        r = bench_side(det, mnet, photos, side)
        print(json.dumps(r), flush=True)
        res["runs"].append(r)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
