"""The landmark network (vspbfr_amd/fan.py, csrc/fan.hip) on 16 pairs of 512 x 512 faces, 2D-FAN-4 with random weights:

  heatmaps     device time of FanLandmarks.heatmaps on the 32 images (HIP events, median of 20 after a warm-up), and of every launch
               class alone -- stem, 3x3 per map size, 1x1, pool, decode -- as its launches replayed on the tensors of one forward pass,
               with the achieved TFLOP/s and the share of the f16 MFMA peak
               (a replay repeats the in-place launches of conv2 and conv4 on one tensor: after some twenty of them those windows no
               longer hold a forward pass's values; the times do not depend on the values)
  eager        the yardstick: the same layers in torch-ROCm eager fp16 channels-last on the same reduced weights on the same GPU in the
               same run, per class and summed (the input affine as a multiply, an add and a ReLU in front of the convolution)
  add          one Evaluator.add of the 16 pairs with lmd set, and without it

    python tools/bench_fan.py [--out profiles/fan_bench.json]
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
F16_MFMA_PEAK_TFLOPS = 2500.0     # dense f16 / bf16 MFMA, MI355X
PAIRS, SIZE = 16, 512


def events(fn, n=20, warm=3):
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


def record(net, u8):
    """one forward pass with every launch noted -> ({class: [closure that repeats the launch]}, {class: flop}, [conv descriptions])"""
    from vspbfr_amd import hip_ops as H
    calls, flop, convs = {}, {}, []
    saved = {n: getattr(H, n) for n in ("fan_stem_u8", "fan_pool_f16", "fan_conv_f16", "fan_decode")}

    def note(fn, cls_of):
        def wrapped(*a, **kw):
            cls = cls_of(a, kw)
            calls.setdefault(cls, []).append(lambda: fn(*a, **kw))
            return fn(*a, **kw)
        return wrapped

    def add(cls, f):
        flop[cls] = flop.get(cls, 0) + f
        return cls

    def conv_cls(a, kw):
        B, h, w, w_img, cout = a[2], a[3], a[4], a[5], a[6]
        k, cin = (1 if w_img.shape[0] == 1 else 3), 32 * w_img.shape[1]
        cls = "1x1" if k == 1 else f"3x3_{h}"
        convs.append(dict(cls=cls, B=B, H=h, W=w, cin=cin, cout=cout, k=k, w=w_img, b=kw.get("b"), affine=kw.get("affine"), relu=kw.get("relu", False),
                          res=sum(kw.get(r) is not None for r in ("res1", "res2")), up=kw.get("up") is not None, raw=kw.get("raw") is not None))
        return add(cls, 2 * B * h * w * cout * cin * k * k)

    H.fan_stem_u8 = note(saved["fan_stem_u8"], lambda a, kw: add("stem", 2 * a[1].shape[0] * (a[5] // 2) ** 2 * 147 * 64))
    H.fan_pool_f16 = note(saved["fan_pool_f16"], lambda a, kw: add("pool", 0))
    H.fan_conv_f16 = note(saved["fan_conv_f16"], conv_cls)
    H.fan_decode = note(saved["fan_decode"], lambda a, kw: add("decode", 0))
    try:
        net.landmarks(u8)
    finally:
        for n, fn in saved.items():
            setattr(H, n, fn)
    return calls, flop, convs


def eager_calls(net, convs, u8):
    """the same layers in torch eager fp16 channels-last on the reduced weights: {class: [closure]}"""
    from vspbfr_amd import fan
    F = torch.nn.functional
    calls = {}
    g = torch.Generator(device="cuda").manual_seed(1)

    def act(b, c, h, w):
        return torch.randn((b, c, h, w), device="cuda", dtype=torch.float16, generator=g).contiguous(memory_format=torch.channels_last)
    for d in convs:
        w = fan.unpack_conv_weight(d["w"], d["cout"]).contiguous(memory_format=torch.channels_last)
        b = None if d["b"] is None else d["b"].half()
        aff = None if d["affine"] is None else tuple(t.half().view(1, -1, 1, 1) for t in d["affine"])
        x = act(d["B"], d["cin"], d["H"], d["W"])
        rs = [act(d["B"], d["cout"], d["H"], d["W"]) for _ in range(d["res"])]
        u = act(d["B"], d["cout"], d["H"] // 2, d["W"] // 2) if d["up"] else None

        def run(x=x, w=w, b=b, aff=aff, rs=rs, u=u, d=d):
            if aff is not None:
                x = torch.relu_(x * aff[0] + aff[1])
            y = F.conv2d(x, w, b, 1, d["k"] // 2)
            if d["relu"]:
                y = torch.relu_(y)
            for r in rs:
                y = y + r
            if u is not None:
                y = y + F.interpolate(u, scale_factor=2, mode="nearest")
            return y
        calls.setdefault(d["cls"], []).append(run)
    B = u8.shape[0]
    x = act(B, 3, net.side, net.side)
    ws = net.p["conv1.w"].reshape(7, 7, 3, 64).permute(3, 2, 0, 1).half().contiguous(memory_format=torch.channels_last)
    bs = net.p["conv1.b"].half()
    big = u8.permute(0, 3, 1, 2)
    calls["stem"] = [lambda: torch.relu_(F.conv2d(F.interpolate(big.half(), size=(net.side, net.side), mode="bilinear", align_corners=False) / 255,
                                                  ws, bs, 2, 3))]
    s2, n = net.side // 2, net.side // 4
    pools = [act(B, 128, s2, s2)] + [act(B, 256, n >> l, n >> l) for l in range(net.depth) for _ in range(net.num_modules)]
    calls["pool"] = [lambda p=p: F.avg_pool2d(p, 2) for p in pools]
    heat = torch.randn((B, 68, n, n), device="cuda", generator=g)
    calls["decode"] = [lambda: heat.view(B, 68, -1).max(dim=2)]
    return calls


def rate(r, flop):
    tf = flop / r["median_ms"] / 1e9
    r.update(gflop=round(flop / 1e9, 2), tflops=round(tf, 1), percent_of_f16_mfma_peak=round(100 * tf / F16_MFMA_PEAK_TFLOPS, 2))
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_fan: no GPU")
    import fan_ref as R
    from vspbfr_amd import metrics as M
    from vspbfr_amd.fan import FanLandmarks
    net = FanLandmarks(R.state_of(R.make_model(0, 4, 4)), "cuda")
    rng = np.random.default_rng(0)
    base = np.stack([R.test_photo(SIZE, SIZE, 100 + i) for i in range(4)])
    restored = torch.from_numpy(base[rng.integers(0, 4, PAIRS)]).cuda()
    gt = torch.from_numpy(np.clip(base[rng.integers(0, 4, PAIRS)].astype(np.int16) + rng.integers(-9, 10, (PAIRS, SIZE, SIZE, 3)), 0, 255).astype(np.uint8)).cuda()
    u8 = torch.cat([restored, gt])
    res = {"what": f"2D-FAN-4 (random weights) on {PAIRS} pairs of {SIZE} x {SIZE}; HIP events, median of 20 after a warm-up; torch eager fp16 "
                   "channels-last on the same reduced weights in the same run; a class is its launches replayed on the tensors of one pass",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "peaks_used": {"f16_mfma_tflops": F16_MFMA_PEAK_TFLOPS},
           "network": net.describe(), "images": int(u8.shape[0])}
    calls, flop, convs = record(net, u8)
    classes = sorted(calls, key=lambda c: (c != "stem", not c.startswith("3x3"), -int(c[4:]) if c.startswith("3x3") else 0, c))
    res["heatmaps"] = rate(events(lambda: net.heatmaps(u8)), sum(flop.values()))
    res["heatmaps"]["launches"] = sum(len(v) for c, v in calls.items() if c != "decode")
    res["gflop_per_image"] = round(sum(flop.values()) / 1e9 / u8.shape[0], 2)
    res["hip_by_class"] = {c: dict(rate(events(lambda: [f() for f in calls[c]]), flop[c]), launches=len(calls[c])) for c in classes}
    with torch.no_grad():
        eager = eager_calls(net, convs, u8)
        res["eager_by_class"] = {c: dict(rate(events(lambda: [f() for f in eager[c]]), flop[c]), launches=len(eager[c])) for c in classes}
    res["eager_sum_of_classes_ms"] = round(sum(v["median_ms"] for v in res["eager_by_class"].values()), 4)
    res["hip_sum_of_classes_ms"] = round(sum(v["median_ms"] for v in res["hip_by_class"].values()), 4)
    res["hip_over_eager"] = {c: round(res["hip_by_class"][c]["median_ms"] / res["eager_by_class"][c]["median_ms"], 3) for c in classes}
    res["hip_over_eager"]["sum_of_classes"] = round(res["hip_sum_of_classes_ms"] / res["eager_sum_of_classes_ms"], 3)
    res["classes_that_lose_to_eager"] = [c for c in classes if res["hip_over_eager"][c] > 1.0]

    def add(lmd):
        ev = M.Evaluator(lmd=lmd)
        ev.add(restored, gt)
    res["evaluator_add_with_lmd"] = events(lambda: add(net))
    res["evaluator_add_without_lmd"] = events(lambda: add(None))
    print(json.dumps(res), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
