"""The background upscaler (vspbfr_amd/upscale.py, csrc/sr.hip) on 8 photos of 1024 x 1536, random weights, 32 convolutions, x4:

  kernels   device time of the head, of ONE body layer and of the tail (x4 and x2) over the whole group (HIP events, median of 30 after a
            warm-up); the body's achieved TFLOP/s against the f16 MFMA peak and its bytes (one read and one write of the activations)
            against the HBM rate
  eager     torch-ROCm eager fp16 conv2d (channels-last) + bias + PReLU on the same weights and the same group in the same run -- the yardstick
  upscale   one SrUpscaler.upscale() call for the group at x4, and at x2 through the ragged LANCZOS resize (upscale_to)
  cli       the loop of vspbfr_amd.restore_photos over the 8 photos (set-up of tools/bench_photo.py: --batch 8 --timesteps 4 --no_sample)
            with and without --bg_weights at --upscale 2 and 4, alternating, three each after a warm run

    python tools/bench_sr.py [--out profiles/sr_bench.json] [--skip-cli | --cli-only]
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
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))
F16_MFMA_PEAK_TFLOPS = 2500.0     # dense f16 / bf16 MFMA, MI355X
HBM_PEAK_TBS = 8.0


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


def bench_kernels(sd, photos):
    from vspbfr_amd import hip_ops as H, upscale as U
    shapes = [p.shape[:2] for p in photos]
    px = sum(h * w for h, w in shapes)
    src = torch.from_numpy(np.concatenate([p.reshape(-1) for p in photos])).cuda()
    src_off = np.concatenate([[0], np.cumsum([p.size for p in photos])])[:-1].tolist()
    units = [(k, 0, h, 0, h) for k, (h, w) in enumerate(shapes)]
    net = U.SrUpscaler(sd, "cuda")
    a, b = (torch.empty(px * 64, dtype=torch.float16, device="cuda") for _ in range(2))
    res = {"group": f"{len(photos)} photos of {shapes[0][0]} x {shapes[0][1]}", "pixels": px}
    n = len(photos)
    tabs = {}
    for s in (2, 4):
        out_off = np.concatenate([[0], np.cumsum([3 * s * s * h * w for h, w in shapes])]).tolist()
        tab, _ = U.item_table(units, shapes, src_off, out_off, s)
        tabs[s] = (tab, torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).cuda(), out_off[-1])
    tab, tab_dev, _ = tabs[4]
    res["head"] = events(lambda: H.sr_head_u8(a, src, tab, tab_dev, n, *net.head))
    img, bias, slope = net.body[0]
    r = events(lambda: H.sr_body_f16(b, a, tab, tab_dev, n, img, bias, slope))
    flop, byts = 2.0 * 576 * 64 * px, 2.0 * 128 * px
    r.update(tflops=round(flop / r["median_ms"] / 1e9, 1), percent_of_f16_mfma_peak=round(100 * flop / r["median_ms"] / 1e9 / F16_MFMA_PEAK_TFLOPS, 2),
             hbm_tb_s=round(byts / r["median_ms"] / 1e9, 3), percent_of_hbm_peak=round(100 * byts / r["median_ms"] / 1e9 / HBM_PEAK_TBS, 1))
    res["body_layer"] = r
    H.sr_body_f16(b, a, tab, tab_dev, n, img, bias, slope)
    info = torch.zeros(n, dtype=torch.int32, device="cuda")
    for s in (4, 2):
        w = torch.randn(3 * s * s, 64, 3, 3) * (0.4 / 576) ** 0.5
        wi, bi = U.pack_body_weight(w).cuda(), torch.zeros(16 * (-(-3 * s * s // 16)), device="cuda")
        tab_s, tab_s_dev, nbytes = tabs[s]
        out = torch.empty(nbytes, dtype=torch.uint8, device="cuda")
        res[f"tail_x{s}"] = events(lambda: H.sr_tail_u8(out, info, b, src, tab_s, tab_s_dev, n, wi, bi, s))
        res[f"tail_x{s}"]["weight"] = w
    del a, b, out
    return res, net


def bench_eager(sd, photos, tails):
    """the same three layer classes in torch eager: fp16 tensors in channels-last memory, conv2d + bias, PReLU as its own op"""
    dev = "cuda"
    x8 = torch.from_numpy(np.stack(photos)).to(dev).permute(0, 3, 1, 2)
    res = {}
    x = (x8.half() / 255).contiguous(memory_format=torch.channels_last)
    w0, b0, a0 = (sd[k].to(dev).half() for k in ("body.0.weight", "body.0.bias", "body.1.weight"))
    w0 = w0.contiguous(memory_format=torch.channels_last)
    res["head_conv_prelu"] = events(lambda: F.prelu(F.conv2d(x, w0, b0, padding=1), a0), n=30, warm=3)
    act = F.prelu(F.conv2d(x, w0, b0, padding=1), a0)
    w1, b1, a1 = (sd[k].to(dev).half() for k in ("body.2.weight", "body.2.bias", "body.3.weight"))
    w1 = w1.contiguous(memory_format=torch.channels_last)
    res["body_conv"] = events(lambda: F.conv2d(act, w1, b1, padding=1), n=30, warm=3)
    res["body_conv_prelu"] = events(lambda: F.prelu(F.conv2d(act, w1, b1, padding=1), a1), n=30, warm=3)
    for s, w in tails.items():
        wt = w.to(dev).half().contiguous(memory_format=torch.channels_last)
        bt = torch.zeros(3 * s * s, device=dev, dtype=torch.float16)
        up = lambda: (F.pixel_shuffle(F.conv2d(act, wt, bt, padding=1), s) + F.interpolate(x, scale_factor=s, mode="nearest")).clamp(0, 1).mul(255).round().to(torch.uint8)
        res[f"tail_x{s}_conv"] = events(lambda: F.conv2d(act, wt, bt, padding=1), n=30, warm=3)
        res[f"tail_x{s}_conv_shuffle_skip_u8"] = events(up, n=10, warm=2)
    return res


def bench_upscale(net, photos):
    src = torch.from_numpy(np.concatenate([p.reshape(-1) for p in photos])).cuda()
    shapes = [p.shape[:2] for p in photos]
    offs = np.concatenate([[0], np.cumsum([p.size for p in photos])])[:-1].tolist()
    dp = (src, offs, shapes)
    out4 = torch.empty(sum(48 * h * w for h, w in shapes), dtype=torch.uint8, device="cuda")
    res = {"x4": events(lambda: net.upscale(device_photos=dp, out=out4), n=10, warm=2)}
    out2 = torch.empty(sum(12 * h * w for h, w in shapes), dtype=torch.uint8, device="cuda")
    res["x2_through_the_resize"] = events(lambda: net.upscale_to(2, device_photos=dp, out=out2), n=10, warm=2)
    res["launches"] = net.num_conv + 2
    return res


def bench_cli(tmp, sd4):
    import bench_photo
    from vspbfr_amd import restore_photos as RP, upscale as U
    restorer, root, names, landmarks, device = bench_photo.cli_setup(tmp, *bench_photo.workload())
    net = U.SrUpscaler(sd4, device)
    res = {"what": "8 photos of 1024 x 1536, 16 faces, --batch 8 --timesteps 4 --no_sample, decode + restore + PNG, writers drained; LANCZOS "
                   "against a 32-convolution x4 network behind --bg_weights, alternating, three each after a warm run",
           "cpus_used": len(os.sched_getaffinity(0))}
    for upscale in (2, 4):
        times = {"lanczos": [], "bg_weights": []}
        restorer.upscale = upscale
        for rep in range(4):                   # the first of each is the warm run
            for route in ("lanczos", "bg_weights"):
                restorer.background = net if route == "bg_weights" else None
                args = Namespace(photos=root, out=os.path.join(tmp, f"out_{upscale}_{route}_{rep}"), batch=8, save_faces=False, upscale=upscale,
                                 size=512, inset=8, feather=48, antialias=False)
                torch.manual_seed(123)
                random.seed(123)
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                RP.restore_photos(args, restorer, names, landmarks, device)
                torch.cuda.synchronize()
                if rep:
                    times[route].append(round(time.perf_counter() - t0, 4))
        res[f"upscale_{upscale}"] = {"loop_s": times, "loop_median_s": {r: statistics.median(t) for r, t in times.items()}}
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-cli", action="store_true")
    ap.add_argument("--cli-only", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sr: no GPU")
    import bench_photo
    import sr_ref as R
    sd = R.make_state(32, 4, seed=1)
    photos, _ = bench_photo.workload()
    res = {"device": torch.cuda.get_device_name(0), "model": "SRVGGNetCompact, 64 features, 32 convolutions, x4, random weights (tests/sr_ref.make_state)",
           "timing": "HIP events around the call, median of 30 after a warm-up (10 for whole calls)",
           "peaks_used": {"f16_mfma_tflops": F16_MFMA_PEAK_TFLOPS, "hbm_tb_s": HBM_PEAK_TBS}}
    if not a.cli_only:
        res["kernels"], net = bench_kernels(sd, photos)
        tails = {s: res["kernels"][f"tail_x{s}"].pop("weight") for s in (4, 2)}
        res["upscale"] = bench_upscale(net, photos)
        del net
        torch.cuda.empty_cache()
        res["eager_fp16_channels_last"] = bench_eager(sd, photos, tails)
        torch.cuda.empty_cache()
    if not a.skip_cli:
        with tempfile.TemporaryDirectory() as tmp:
            res["cli"] = bench_cli(tmp, sd)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
