"""Time vsp_pair_stats_u8 (hip_ops.pair_stats_u8) beside the formulation a user would write today: fp32 F.conv2d moments with
torch ops on the same GPU.  HIP events, warm, B = 16 at 512^2 RGB, both windows, median of >= 20 launches after warm-up.

    python tools/bench_metrics.py [--batch 16] [--size 512] [--iters 30] [--out profiles/metrics_bench.json]

The torch-op baseline takes the same uint8 tensors and returns the same two numbers per image (SSE and mean SSIM over the valid
positions), so both columns time the same job; it is the naive uncentred form, whose accuracy tests/test_metrics_gpu.py measures."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

C1, C2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2


def torch_pair_stats(a, b, window):
    """(B, H, W, 3) uint8 x 2 -> (sse, ssim) with framework ops: depthwise fp32 F.conv2d over x, y, xx, yy, xy."""
    x, y = a.permute(0, 3, 1, 2).float(), b.permute(0, 3, 1, 2).float()
    sse = ((x - y) ** 2).sum((1, 2, 3))       # fp32 sum: not exact at this size (the kernel's is)
    if window == "uniform7":
        k, cov = torch.full((7, 7), 1.0 / 49.0, device=a.device), 49.0 / 48.0
    else:
        d = torch.arange(11, device=a.device, dtype=torch.float64) - 5
        t = torch.exp(-(d * d) / 4.5)
        t = (t / t.sum()).float()
        k, cov = torch.outer(t, t), 1.0
    k = k[None, None].expand(3, 1, -1, -1).contiguous()
    f = lambda v: F.conv2d(v, k, groups=3)
    ux, uy = f(x), f(y)
    vx, vy, vxy = cov * (f(x * x) - ux * ux), cov * (f(y * y) - uy * uy), cov * (f(x * y) - ux * uy)
    s = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return sse, s.double().mean((1, 2, 3))


def time_us(fn, iters, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    times = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        times.append(e0.elapsed_time(e1) * 1e3)
    return {"median_us": statistics.median(times), "min_us": min(times), "max_us": max(times), "launches": iters}


def main(argv=None):
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--iters", type=int, default=30)
    ap.add_argument("--out", default=None)
    args = ap.parse_args(argv)
    if args.iters < 20:
        ap.error("--iters must be at least 20")
    from vspbfr_amd import hip_ops as H
    g = torch.Generator().manual_seed(0)
    a = torch.randint(0, 256, (args.batch, args.size, args.size, 3), generator=g, dtype=torch.uint8).cuda()
    b = (a.int() + torch.randint(-12, 13, a.shape, generator=g).cuda()).clamp(0, 255).to(torch.uint8)
    res = {"device": torch.cuda.get_device_name(0), "batch": args.batch, "size": args.size, "bytes_read": 2 * a.numel(), "windows": {}}
    for window in ("uniform7", "gauss11"):
        hip = time_us(lambda: H.pair_stats_u8(a, b, window), args.iters)
        ref = time_us(lambda: torch_pair_stats(a, b, window), args.iters)
        s0, q0 = H.pair_stats_u8(a, b, window)
        _, q1 = torch_pair_stats(a, b, window)
        exact = ((a.to(torch.int64) - b.to(torch.int64)) ** 2).sum((1, 2, 3))
        res["windows"][window] = {
            "hip_pair_stats_u8": hip, "torch_fp32_conv2d_moments": ref, "speedup_median": ref["median_us"] / hip["median_us"],
            "max_abs_ssim_difference_between_the_two": float((q0 - q1).abs().max()),
            "hip_sse_equals_int64_sum": bool((s0 == exact).all())}
    line = json.dumps(res)
    print(line)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(res, indent=1) + "\n")


if __name__ == "__main__":
    main()
