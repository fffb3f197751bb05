"""Device time of the training degradation chain (vspbfr_amd/degrade.py) for one free-form batch: B samples x 2 LQ images at
size^2 (the reference's ImageFolder_restore_free_form at B = 4, 512^2 makes 8 LQ images + gt), split by stage with device events,
after a warm-up and over >= --seconds of work per measurement; the blur's flops and bytes from the shapes; host decode throughput
(PIL decode + LANCZOS cover resize + crop of a 1024^2 PNG) on --threads threads.  One JSON line on stdout (and in --out).

    python tools/bench_degrade.py [--batch 4] [--size 512] [--seconds 1.0] [--threads 16] [--out FILE]
Kernel times: run it under `rocprofv3 --kernel-trace --stats -- python tools/bench_degrade.py --seconds 0.3 --no-host` in a run of its own.
"""
import argparse
import json
import os
import sys
import tempfile
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

FP32_PEAK_TFLOPS = 157.3   # MI355X vector fp32 (packed FMA)


def smooth_batch(rng, B, size):
    y, x = np.mgrid[0:size, 0:size]
    base = np.stack([0.5 + 0.3 * np.sin(x / (9.0 + c)) * np.cos(y / (13.0 + c)) for c in range(3)])
    return np.clip(base[None] + 0.05 * rng.standard_normal((B, 3, size, size)), 0, 1).astype(np.float32)


def timed(fn, seconds):
    """mean device ms per call of fn over >= `seconds` of work, by events around the whole window"""
    fn()
    torch.cuda.synchronize()
    n, total = 0, 0.0
    while total < seconds * 1000.0:
        reps = max(1, n)
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(reps):
            fn()
        b.record()
        b.synchronize()
        total += a.elapsed_time(b)
        n += reps
    return total / n, n


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=4)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--threads", type=int, default=16)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--no-host", action="store_true", help="skip the host decode measurement")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_degrade: no GPU")
    from vspbfr_amd import hip_ops as H
    from vspbfr_amd.degrade import DegradeParams, DegradePlan, run_plan, sample_lq, sample_rng

    B, S = a.batch, a.size
    rng = np.random.default_rng(a.seed)
    gt = torch.from_numpy(smooth_batch(rng, B, S)).cuda()
    p = DegradeParams.free_form()
    # slot-major as the loader builds it: lq1 of every sample, then lq2
    lqs = [sample_lq(p, (S, S), sample_rng(a.seed, 0, b, s + 1)) for s in range(2) for b in range(B)]
    src = [b for _ in range(2) for b in range(B)]
    t0 = time.perf_counter()
    plan = DegradePlan(lqs, src, (S, S), B, samples=src, slots=[1 + i // B for i in range(2 * B)])
    plan_ms = (time.perf_counter() - t0) * 1000
    items, taps = plan.upload(gt.device)

    total_ms, n_total = timed(lambda: run_plan(plan, gt, seed=1, step=0), a.seconds)
    blurred = H.degrade_blur(gt, taps, items, plan.n)
    lq = H.degrade_down(blurred, items, plan.n, plan.lq_elems, plan.max_pixels, 1, 0)
    lq_keep = lq.clone()
    stages = {
        "blur": lambda: H.degrade_blur(gt, taps, items, plan.n),
        "down_noise": lambda: H.degrade_down(blurred, items, plan.n, plan.lq_elems, plan.max_pixels, 1, 0),
        "jpeg": lambda: H.degrade_jpeg(lq, items, plan.n, plan.total_mcus, plan.work_bytes, plan.max_pixels),
        "up_round": lambda: H.degrade_up(lq_keep, items, plan.n, S, S),
    }
    stage_ms = {k: round(timed(f, a.seconds)[0], 4) for k, f in stages.items()}

    flops = sum(2.0 * q.ksize ** 2 * 3 * S * S for q in lqs)
    blur_bytes = plan.n * 3 * S * S * 4 * 2
    blur_s = stage_ms["blur"] / 1000
    res = {
        "what": f"free-form batch B={B} ({plan.n} LQ + gt) at {S}^2",
        "device_ms_per_batch": round(total_ms, 4), "batches_timed": n_total,
        "stage_ms": stage_ms,
        "plan_host_ms": round(plan_ms, 3),
        "items": [{"k": q.ksize, "size": list(q.size), "q": q.quality, "sigma": round(q.sigma, 2)} for q in lqs],
        "blur_gflop": round(flops / 1e9, 3), "blur_bytes_mb": round(blur_bytes / 1e6, 2),
        "blur_tflops": round(flops / blur_s / 1e12, 2), "blur_share_of_fp32_peak": round(flops / blur_s / 1e12 / FP32_PEAK_TFLOPS, 3),
        "lq_pixels": int(plan.lq_elems // 3), "mcus": plan.total_mcus,
    }
    if not a.no_host:
        from PIL import Image

        from vspbfr_amd.trainset import ImageFolder_restore_free_form
        from concurrent.futures import ThreadPoolExecutor
        with tempfile.TemporaryDirectory() as d:
            big = (np.clip(smooth_batch(rng, 1, 1024)[0].transpose(1, 2, 0), 0, 1) * 255).astype(np.uint8)
            for i in range(8):
                Image.fromarray(np.roll(big, 37 * i, axis=1)).save(os.path.join(d, f"{i}.png"))
            ds = ImageFolder_restore_free_form(d, im_size=(S, S))
            with ThreadPoolExecutor(a.threads) as pool:
                list(pool.map(lambda i: ds.load(i % 8, sample_rng(0, 0, i, 0)), range(a.threads)))
                n, t0 = 0, time.perf_counter()
                while time.perf_counter() - t0 < max(a.seconds, 1.0):
                    list(pool.map(lambda i: ds.load(i % 8, sample_rng(0, 0, i, 0)), range(n, n + 4 * a.threads)))
                    n += 4 * a.threads
                dt = time.perf_counter() - t0
        res["host_decode"] = {"threads": a.threads, "source": "1024^2 RGB PNG -> LANCZOS cover + crop", "images_per_s": round(n / dt, 1),
                              "ms_per_batch": round(B / (n / dt) * 1000, 2)}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
