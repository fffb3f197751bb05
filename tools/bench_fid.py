"""FID Inception on the device: B = 16 images of 512 x 512, HIP events, median of 30.  Times the stem, the convolutions by
class (the 35 x 35, 17 x 17 and 8 x 8 blocks, and the stem chain), the pools and one features() call, each beside torch eager fp32 on the
same folded weights in the same run, and reports TFLOP/s against the 157.3 TF fp32 matrix peak.  Writes profiles/fid_bench.json.

    python tools/bench_fid.py [--batch 16] [--size 512] [--reps 30] [--out profiles/fid_bench.json]

The weights are random (He-style): the timing does not depend on their values."""
import argparse
import json
import os
import statistics
import sys

import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
PEAK_TF = 157.3


def random_state(fid, seed=0):
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for k, shape in fid.expected_state().items():
        if k.endswith("conv.weight"):
            sd[k] = torch.randn(shape, generator=g) * (2.0 / (shape[1] * shape[2] * shape[3])) ** 0.5
        elif k.endswith(("bn.weight", "running_var")):
            sd[k] = 0.75 + 0.5 * torch.rand(shape, generator=g)
        else:
            sd[k] = 0.05 * torch.randn(shape, generator=g)
    return sd


def timed(fn, reps):
    for _ in range(3):
        fn()
    torch.cuda.synchronize()
    out = []
    for _ in range(reps):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        out.append(a.elapsed_time(b))
    return statistics.median(out)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--size", type=int, default=512)
    ap.add_argument("--reps", type=int, default=30)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fid_bench.json"))
    args = ap.parse_args()
    from vspbfr_amd import fid
    from vspbfr_amd import hip_ops as H
    dev = torch.device("cuda", 0)
    B = args.batch
    state = fid.check_state_dict(random_state(fid))
    net = fid.FidInception(state, dev)
    folded = {k: (w.float().to(dev), b.float().to(dev)) for k, (w, b) in fid.fold_state(state).items()}
    g = torch.Generator().manual_seed(1)
    images = torch.randint(0, 256, (B, args.size, args.size, 3), generator=g, dtype=torch.uint8).to(dev)
    plan = net._plan(fid.SIZE, fid.SIZE)
    net.features(images)                                     # the workspace
    bufs = net._buffers(plan, B)
    bufs["feat"] = torch.empty((B, fid.DIMS), dtype=torch.float32, device=dev)

    def klass(op):
        if op[0] == "pool":
            return "pools"
        side = op[4]
        return {35: "conv_35", 17: "conv_17", 8: "conv_8"}.get(side, "conv_stem") if op[1].startswith("Mixed") else "conv_stem"

    groups = {}
    for op in plan.ops:
        groups.setdefault(klass(op), []).append(op)
    # eager: every launch on its own contiguous NCHW input of the right shape
    eager = {}
    for name, ops in groups.items():
        calls = []
        for op in ops:
            if op[0] == "conv":
                c = plan.specs[op[1]]
                x = torch.randn((B, c.cin, op[4], op[5]), device=dev)
                w, b = folded[op[1]]
                calls.append(lambda x=x, w=w, b=b, c=c: F.relu_(F.conv2d(x, w, b, stride=c.stride, padding=(c.ph, c.pw))))
            else:
                x = torch.randn((B, op[6], op[4], op[5]), device=dev)
                calls.append({H.FID_POOL_MAX_S2: lambda x=x: F.max_pool2d(x, 3, 2), H.FID_POOL_AVG_S1: lambda x=x: F.avg_pool2d(x, 3, 1, 1, count_include_pad=False),
                              H.FID_POOL_MAX_S1: lambda x=x: F.max_pool2d(x, 3, 1, 1), H.FID_POOL_GLOBAL_AVG: lambda x=x: x.mean(dim=(2, 3))}[op[1]])
        eager[name] = calls

    def flops(ops):
        total = 0
        for op in ops:
            if op[0] == "conv":
                c = plan.specs[op[1]]
                oh, ow = H.fid_conv_out(op[4], op[5], c.kh, c.kw, c.ph, c.pw, c.stride)
                total += 2 * B * oh * ow * c.cout * c.cin * c.kh * c.kw
        return total

    rows = {}
    w1, b1 = folded["Conv2d_1a_3x3"]

    def eager_stem():
        x = F.interpolate(images.permute(0, 3, 1, 2).float(), size=(fid.SIZE, fid.SIZE), mode="bilinear", align_corners=False) / 127.5 - 1
        return F.relu_(F.conv2d(x, w1, b1, stride=2))

    with torch.no_grad():
        hip_ms = timed(lambda: _stem(net, plan, bufs, images, B), args.reps)
        rows["stem"] = {"launches": 1, "hip_ms": hip_ms, "eager_ms": timed(eager_stem, args.reps), "gflop": 2 * B * 149 * 149 * 32 * 27 / 1e9}
        for name, ops in sorted(groups.items()):
            hip_ms = timed(lambda ops=ops: [net.launch(plan, op, bufs, B) for op in ops], args.reps)
            eager_ms = timed(lambda calls=eager[name]: [c() for c in calls], args.reps)
            rows[name] = {"launches": len(ops), "hip_ms": hip_ms, "eager_ms": eager_ms, "gflop": flops(ops) / 1e9}
        whole = timed(lambda: net.features(images), args.reps)
    total_gflop = sum(r["gflop"] for r in rows.values())
    for r in rows.values():
        r["hip_over_eager"] = r["hip_ms"] / r["eager_ms"]
        if r["gflop"]:
            r["hip_tflops"] = r["gflop"] / r["hip_ms"]
            r["eager_tflops"] = r["gflop"] / r["eager_ms"]
            r["hip_share_of_peak"] = r["hip_tflops"] / PEAK_TF
    result = {"what": f"FID Inception-v3, fp32, B = {B} u8 images of {args.size} x {args.size}; HIP events, median of {args.reps}; eager = torch "
                      "fp32 on the same folded weights, every launch on its own contiguous NCHW input (no concatenation cost)",
              "device": torch.cuda.get_device_name(0), "peak_fp32_matrix_tflops": PEAK_TF, "classes": rows,
              "features": {"hip_ms": whole, "ms_per_image": whole / B, "gflop": total_gflop, "hip_tflops": total_gflop / whole,
                           "share_of_peak": total_gflop / whole / PEAK_TF, "eager_sum_of_classes_ms": sum(r["eager_ms"] for r in rows.values()),
                           "hip_sum_of_classes_ms": sum(r["hip_ms"] for r in rows.values())}}
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(result, f, indent=1)
        f.write("\n")
    print(json.dumps(result["features"]))
    for k, r in rows.items():
        print(k, json.dumps(r))


def _stem(net, plan, bufs, images, B):
    from vspbfr_amd import _lib
    from vspbfr_amd import hip_ops as H
    from vspbfr_amd import fid
    if not hasattr(_stem, "items"):
        n = images.shape[1] * images.shape[2] * 3
        items = (_lib.DetSrc * B)()
        for i in range(B):
            items[i].off, items[i].h, items[i].w, items[i].slot = i * n, images.shape[1], images.shape[2], i
        _stem.items = items
        _stem.dev = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(images.device)
    w, b = net.weights["Conv2d_1a_3x3"]
    sh, sw = plan.stem
    H.fid_stem_u8(bufs["x"][:B * sh * sw * 32], images.view(-1), _stem.items, _stem.dev, B, B, fid.SIZE, fid.SIZE, w, b)


if __name__ == "__main__":
    main()
