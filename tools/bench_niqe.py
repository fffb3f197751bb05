"""NIQE features of a batch: the single-launch kernel (hip_ops.niqe_features_u8) against the same job written with torch ops on
the same GPU.  B = 16 at 512^2, HIP events, median of 30 after 5 warm-up calls.  Writes profiles/niqe_bench.json.

    timeout -k 10 120 python tools/bench_niqe.py --step hip   [--batch 16] [--size 512] [--reps 30] [--out profiles/niqe_bench.json]
    timeout -k 10 120 python tools/bench_niqe.py --step torch [the same arguments]

Two steps, each a process of its own under its own time limit, chained with `&&`; each merges its part into --out, and the one
that finds the other's part there adds the ratio.

The torch form stops at the raw moments (the smooth part: luma, both scales, MSCN, the five maps, six masked sums each); the
table lookup that the kernel also does is left out of it, in its favour."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def torch_moments(u8):
    """(B, H, W, 3) uint8 -> (B, nblk, 2, 5, 6) float64 raw moments with torch ops (float32 maps, float64 sums)"""
    p = u8.to(torch.int64)
    n = 65481 * p[..., 0] + 128553 * p[..., 1] + 24966 * p[..., 2]
    q, rem = n // 255000, n % 255000
    y = (16 + q + ((2 * rem > 255000) | ((2 * rem == 255000) & (q % 2 == 1)))).to(torch.float32)
    B, H, W = y.shape
    y = y[:, :H // 96 * 96, :W // 96 * 96]
    k = torch.arange(7, device=y.device, dtype=torch.float64) - 3
    g = torch.exp(-k * k / (2 * (7 / 6) ** 2))
    g = (g / g.sum()).to(torch.float32)
    win = torch.outer(g, g)[None, None]
    ht = torch.tensor([-3, -9, 29, 111, 111, 29, -9, -3], device=y.device, dtype=torch.float32) / 256

    def half(x, dim):
        n_ = x.shape[dim]
        x = torch.cat([x.narrow(dim, 0, 3).flip(dim), x, x.narrow(dim, n_ - 4, 4).flip(dim)], dim)
        return sum(ht[t] * x.narrow(dim, t, n_).index_select(dim, torch.arange(0, n_, 2, device=x.device)) for t in range(8))

    out = []
    for s, img in enumerate((y, half(half(y, 1), 2))):
        x = img[:, None]
        mu = F.conv2d(F.pad(x, (3, 3, 3, 3), mode="replicate"), win)
        sd = torch.sqrt(torch.abs(F.conv2d(F.pad(x * x, (3, 3, 3, 3), mode="replicate"), win) - mu * mu))
        v = ((x - mu) / (sd + 1))[:, 0]
        nb = 96 >> s
        blk = v.reshape(B, v.shape[1] // nb, nb, v.shape[2] // nb, nb).permute(0, 1, 3, 2, 4).reshape(B, -1, nb, nb)
        maps = torch.stack([blk] + [blk * torch.roll(blk, sh, dims=(2, 3)) for sh in ((0, 1), (1, 0), (1, 1), (1, -1))], 2).to(torch.float64)
        neg, pos, sq = maps < 0, maps > 0, maps * maps
        out.append(torch.stack([neg.sum((3, 4)).double(), (sq * neg).sum((3, 4)), pos.sum((3, 4)).double(), (sq * pos).sum((3, 4)),
                                maps.abs().sum((3, 4)), sq.sum((3, 4))], -1))
    return torch.stack(out, 2)


def timed(fn, reps, warmup=5):
    for _ in range(warmup):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return statistics.median(ms), min(ms), max(ms)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join("profiles", "niqe_bench.json"))
    ap.add_argument("--step", choices=["hip", "torch"], required=True, help="which of the two timings this process takes")
    args = ap.parse_args()
    from vspbfr_amd import hip_ops as H
    u8 = torch.randint(0, 256, (args.batch, args.size, args.size, 3), dtype=torch.uint8, generator=torch.Generator().manual_seed(0)).cuda()
    res = {}
    if os.path.exists(args.out):
        with open(args.out) as f:
            res = json.load(f)
    shape = {"batch": args.batch, "size": args.size, "reps": args.reps, "device": torch.cuda.get_device_name(0)}
    if any(res.get(k) != v for k, v in shape.items()):
        res = dict(shape)                                          # another job's file: start again
    if args.step == "hip":
        t = timed(lambda: H.niqe_features_u8(u8, 0), args.reps)
        res["hip_ms"] = {"median": t[0], "min": t[1], "max": t[2]}
        res["hip_images_per_s"] = args.batch / t[0] * 1e3
    else:
        _, _, mom = H.niqe_features_u8(u8, 0, with_moments=True)
        ref = torch_moments(u8)
        res["moments_max_rel_diff_vs_torch_ops"] = float(((mom - ref).abs() / ref.abs().clamp_min(1e-30)).max())
        t = timed(lambda: torch_moments(u8), args.reps)
        res["torch_ops_ms"] = {"median": t[0], "min": t[1], "max": t[2]}
    if "hip_ms" in res and "torch_ops_ms" in res:
        res["torch_over_hip"] = res["torch_ops_ms"]["median"] / res["hip_ms"]["median"]
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    print(json.dumps(res))


if __name__ == "__main__":
    main()
