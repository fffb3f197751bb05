"""Per-launch A/B of the up-convs of the path at batch B (default 8): the direct transposed launch of vsp_conv2d_f32 (conv_pipe.hip MODE 1, the
tuned tile) against the fused Winograd phase kernel (conv_tconv_wino.hip), same process, same operands, interleaved.  One child process per
shape, each under its own time limit; median and minimum of N launches after warm-up go to the JSON file, and --allow derives
vspbfr_amd/tconv_wino_allow.json from it (a shape goes in only where the new kernel's median is >= 5 % below the direct one's, and not where HOLD
names it).

    python tools/bench_tconv_wino.py [--out profiles/tconv_wino_launch_ab.json] [--n 30] [--allow]
"""
import argparse
import json
import math
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
# Measured >= 5 % faster and still held back: at batch 8 each of these 512-channel up-convs moves `style_sample` of the configs[1] step by
# 1.0-1.1e-5 against the direct kernel (all six shapes together 1.5e-5; the two that stay in: 6.9e-6), and tests/test_hip_models.py
# test_config_c2_full_size holds every image of the batch to 1e-5 of its batch-1 run, which keeps the direct kernel (exact-key rule)
HOLD = {"8,512,64,64,1,256,3,3,1,1,65,65,t", "8,512,32,32,1,512,3,3,1,1,33,33,t", "8,512,16,16,1,512,3,3,1,1,17,17,t", "8,512,8,8,1,512,3,3,1,1,9,9,t"}
SHAPES = [(64, 32, 512), (128, 64, 256), (256, 128, 128), (512, 256, 64), (512, 512, 32), (512, 512, 16), (512, 512, 8), (512, 512, 4)]   # Cin, Cout, H = W


def one_shape(i, B, n):
    import torch
    from vspbfr_amd import hip_ops as H
    cin, cout, hw = SHAPES[i]
    g = torch.Generator().manual_seed(1)
    x = torch.randn(B, cin, hw, hw, generator=g).cuda()
    w = (torch.randn(cout, cin, 3, 3, generator=g) / math.sqrt(cin * 9)).cuda()
    s_in = (torch.rand(B, cin, generator=g) + 0.5).cuda()
    demod = (torch.rand(B, cout, generator=g) + 0.5).cuda()
    pc = H.PackedConv(H.pack_weight(w), 1, cout, cin, 3, 3, 1, (1,), (1,))
    out = torch.empty(B, cout, 2 * hw + 1, 2 * hw + 1, device="cuda")
    key = H.conv_key(B, cin, hw, hw, pc, hw + 1, hw + 1) + ",t"

    def launch(mode):
        H.TCONV_WINO = mode
        return H.conv2d_packed(x, pc, transposed=True, out=out, in_scale=s_in, out_scale=demod)
    yd = launch(False).clone()
    diff = (launch("all") - yd).abs().max().item()
    times = {False: [], "all": []}
    for it in range(n + 5):
        for mode in (False, "all"):
            s, e = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            s.record()
            launch(mode)
            e.record()
            e.synchronize()
            if it >= 5:
                times[mode].append(s.elapsed_time(e) * 1000)
    med = lambda v: sorted(v)[len(v) // 2]   # noqa: E731
    d, wn = times[False], times["all"]
    return {"key": key, "cin": cin, "cout": cout, "hw": hw, "B": B, "launches": n, "direct_us": {"median": med(d), "min": min(d)},
            "tconvw_us": {"median": med(wn), "min": min(wn)}, "speedup_median": med(d) / med(wn), "max_abs_diff": diff,
            "gflop_direct_count": 2.0 * B * cout * hw * hw * cin * 9 / 1e9}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tconv_wino_launch_ab.json"))
    ap.add_argument("--n", type=int, default=30)
    ap.add_argument("--B", type=int, default=8)
    ap.add_argument("--shape", type=int, default=-1, help="(child) measure this shape and print its JSON line")
    ap.add_argument("--allow", action="store_true", help="derive vspbfr_amd/tconv_wino_allow.json from --out instead of measuring")
    a = ap.parse_args()
    if a.allow:
        rows = json.load(open(a.out))["shapes"]
        keys = sorted(r["key"] for r in rows if r["speedup_median"] >= 1.05 and r["key"] not in HOLD)
        with open(os.path.join(ROOT, "vspbfr_amd", "tconv_wino_allow.json"), "w") as f:
            json.dump(keys, f, indent=0)
            f.write("\n")
        print("allow-list:", keys)
        return
    if a.shape >= 0:
        print("RESULT " + json.dumps(one_shape(a.shape, a.B, a.n)), flush=True)
        return
    rows = []
    for i in range(len(SHAPES)):
        r = subprocess.run([sys.executable, os.path.abspath(__file__), "--shape", str(i), "--n", str(a.n), "--B", str(a.B)], capture_output=True,
                           text=True, timeout=120)
        if r.returncode != 0:   # a fault, abort or time limit: nothing more is started on the device
            sys.stderr.write(r.stdout + r.stderr)
            raise SystemExit(f"shape {SHAPES[i]} ended with status {r.returncode}")
        row = json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("RESULT ")][-1][7:])
        rows.append(row)
        print(f"{row['cin']:4d} -> {row['cout']:3d} at {row['hw'] + 1}^2: direct {row['direct_us']['median']:8.1f} us (min {row['direct_us']['min']:.1f}) | "
              f"tconvw {row['tconvw_us']['median']:8.1f} us (min {row['tconvw_us']['min']:.1f}) | x{row['speedup_median']:.3f} | max diff {row['max_abs_diff']:.1e}",
              flush=True)
    os.makedirs(os.path.dirname(a.out), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump({"what": "per-launch A/B, direct transposed launch vs fused Winograd phase kernel, microseconds", "shapes": rows}, f, indent=1)
        f.write("\n")


if __name__ == "__main__":
    main()
