"""The RRDBNet background upscaler (vspbfr_amd/rrdb.py, csrc/rrdb.hip) on one photo of 1024 x 1536, random weights, 23 blocks:

  kernels   device time (HIP events, median of 30 after a warm-up) of the head (x4 and x2), of the five dense shapes 64 | 96 | 128 | 160 ->
            32 (into their slice of the 192-channel tensor) and 192 -> 64 with one and with two residuals, of conv_up1 (nearest x2 fused), and
            of conv_up2, conv_hr and the tail over one band of 512 rows of the 2x map; TFLOP/s as a share of the f16 MFMA peak
  eager     torch-ROCm eager fp16 channels-last conv2d on the same weights in the same run, each on a contiguous input of its own (eager
            pays no concatenation; the LeakyReLU, the residuals and the upsampling are NOT in its figure) -- the yardstick of each class
  upscale   one RrdbUpscaler.upscale() of the photo with a x4 and with a x2 network

    python tools/bench_rrdb.py [--out profiles/rrdb_bench.json]
"""
import argparse
import json
import os
import statistics
import sys

import numpy as np
import torch
import torch.nn.functional as F

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
F16_MFMA_PEAK_TFLOPS = 2500.0     # dense f16 / bf16 MFMA, MI355X
H0, W0 = 1024, 1536
BAND = 512                        # rows of the 2x map in the band that conv_up2, conv_hr and the tail are timed on


def events(fn, n=30, warm=3):
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


def rate(r, cin, cout, px):
    flop = 2.0 * 9 * cin * cout * px
    r.update(tflops=round(flop / r["median_ms"] / 1e9, 1), percent_of_f16_mfma_peak=round(100 * flop / r["median_ms"] / 1e9 / F16_MFMA_PEAK_TFLOPS, 2))
    return r


def eager_conv(w, b, h, w_, cin):
    x = torch.randn(1, cin, h, w_, device="cuda", dtype=torch.float16).contiguous(memory_format=torch.channels_last)
    wt, bt = w.cuda().half().contiguous(memory_format=torch.channels_last), b.cuda().half()
    r = events(lambda: F.conv2d(x, wt, bt, padding=1), n=30, warm=3)
    del x
    return r


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rrdb: no GPU")
    import rrdb_ref as R
    from vspbfr_amd import hip_ops as H, rrdb
    photo = R.make_photo(H0, W0, seed=1)
    src = torch.from_numpy(photo.reshape(-1)).cuda()
    res = {"device": torch.cuda.get_device_name(0), "photo": f"{H0} x {W0}",
           "model": "RRDBNet, 64 features, growth 32, 23 blocks, random weights (tests/rrdb_ref.make_state, gain 0.5)",
           "timing": "HIP events around the call, median of 30 after a warm-up", "peaks_used": {"f16_mfma_tflops": F16_MFMA_PEAK_TFLOPS}}
    sd4 = R.make_state(23, 4, seed=1, gain=R.DEPTH_GAIN)
    net = rrdb.RrdbUpscaler(sd4, "cuda")
    px = H0 * W0
    k, e = {}, {}
    dense = torch.randn(px * 192, device="cuda").mul_(0.5).half()
    other = torch.zeros(px * 192, dtype=torch.float16, device="cuda")
    feat = torch.zeros(px * 64, dtype=torch.float16, device="cuda")
    k["head_x4"] = events(lambda: H.rrdb_head_u8(feat, 64, src, 0, H0, W0, 4, *net.head))
    for j in (1, 2, 3, 4):
        cin = 32 + 32 * j
        wimg, b = net.convs[f"body.0.rdb1.conv{j}"]
        k[f"dense_{cin}_to_32"] = rate(events(lambda: H.rrdb_conv_f16(dense, 192, cin, dense, 192, H0, W0, wimg, b, act=True)), cin, 32, px)
        e[f"dense_{cin}_to_32"] = rate(eager_conv(sd4[f"body.0.rdb1.conv{j}.weight"], sd4[f"body.0.rdb1.conv{j}.bias"], H0, W0, cin), cin, 32, px)
    wimg, b = net.convs["body.0.rdb1.conv5"]
    k["dense_192_to_64_one_residual"] = rate(events(lambda: H.rrdb_conv_f16(other, 192, 0, dense, 192, H0, W0, wimg, b, res1=(dense, 192, 0.2))), 192, 64, px)
    k["dense_192_to_64_two_residuals"] = rate(events(lambda: H.rrdb_conv_f16(other, 192, 0, dense, 192, H0, W0, wimg, b, res1=(dense, 192, 0.2),
                                                                           res2=(feat, 64, 0.2))), 192, 64, px)
    e["dense_192_to_64"] = rate(eager_conv(sd4["body.0.rdb1.conv5.weight"], sd4["body.0.rdb1.conv5.bias"], H0, W0, 192), 192, 64, px)
    del other
    up1 = torch.empty(4 * px * 64, dtype=torch.float16, device="cuda")
    k["conv_up1"] = rate(events(lambda: H.rrdb_conv_f16(up1, 64, 0, feat, 64, H0, W0, *net.convs["conv_up1"], act=True, up=True)), 64, 64, 4 * px)
    e["conv_up1_on_an_upsampled_input"] = rate(eager_conv(sd4["conv_up1.weight"], sd4["conv_up1.bias"], 2 * H0, 2 * W0, 64), 64, 64, 4 * px)
    W2 = 2 * W0
    bpx = 2 * BAND * 2 * W2
    v1, v2 = (torch.empty(bpx * 64, dtype=torch.float16, device="cuda") for _ in range(2))
    band = up1[:BAND * W2 * 64].normal_(0, 0.5)
    k["conv_up2_band"] = rate(events(lambda: H.rrdb_conv_f16(v1, 64, 0, band, 64, BAND, W2, *net.convs["conv_up2"], act=True, up=True)), 64, 64, bpx)
    k["conv_hr_band"] = rate(events(lambda: H.rrdb_conv_f16(v2, 64, 0, v1, 64, 2 * BAND, 2 * W2, *net.convs["conv_hr"], act=True)), 64, 64, bpx)
    out = torch.empty(3 * bpx, dtype=torch.uint8, device="cuda")
    info = torch.zeros(1, dtype=torch.int32, device="cuda")
    k["tail_band"] = rate(events(lambda: H.rrdb_tail_u8(out, 0, 3 * 2 * W2, 2 * W2, info, v2, 64, 2 * BAND, 2 * W2, 0, 2 * BAND, *net.tail)), 64, 3, bpx)
    del v1, v2, up1, band, out, dense, feat
    torch.cuda.empty_cache()
    e["conv_64_to_64_band"] = rate(eager_conv(sd4["conv_hr.weight"], sd4["conv_hr.bias"], 2 * BAND, 2 * W2, 64), 64, 64, bpx)
    e["tail_conv_64_to_3_band"] = rate(eager_conv(sd4["conv_last.weight"], sd4["conv_last.bias"], 2 * BAND, 2 * W2, 64), 64, 3, bpx)
    torch.cuda.empty_cache()
    res["kernels"], res["eager_fp16_channels_last"] = k, e
    dp = (src, [0], [(H0, W0)])
    flop4 = sum(2.0 * 9 * c[0] * c[1] * m for c, m in
                [((64, 3), px)] + [((32 if j < 5 else 64, 32 + 32 * j), px) for _ in range(69) for j in (1, 2, 3, 4, 5)]
                + [((64, 64), px), ((64, 64), 4 * px), ((64, 64), 16 * px), ((64, 64), 16 * px), ((3, 64), 16 * px)])
    out4 = torch.empty(48 * px, dtype=torch.uint8, device="cuda")
    r = events(lambda: net.upscale(device_photos=dp, out=out4), n=30, warm=2)
    r.update(tflop=round(flop4 / 1e12, 2), tflops=round(flop4 / r["median_ms"] / 1e9, 1),
             percent_of_f16_mfma_peak=round(100 * flop4 / r["median_ms"] / 1e9 / F16_MFMA_PEAK_TFLOPS, 2), launches=net.upscale(device_photos=dp, out=out4)[1]["launches"])
    res["upscale_x4"] = r
    del net, out4
    torch.cuda.empty_cache()
    net2 = rrdb.RrdbUpscaler(R.make_state(23, 2, seed=2, gain=R.DEPTH_GAIN), "cuda")
    k["head_x2"] = events(lambda: H.rrdb_head_u8(net2._buf("feat", px // 4 * 64), 64, src, 0, H0, W0, 2, *net2.head))
    out2 = torch.empty(12 * px, dtype=torch.uint8, device="cuda")
    r = events(lambda: net2.upscale(device_photos=dp, out=out2), n=30, warm=2)
    r.update(tflop=round(flop4 / 4e12, 2), tflops=round(flop4 / 4 / r["median_ms"] / 1e9, 1), launches=net2.upscale(device_photos=dp, out=out2)[1]["launches"])
    res["upscale_x2"] = r
    res["loses_to_eager"] = sorted(n for n, m in (("dense_64_to_32", "dense_64_to_32"), ("dense_96_to_32", "dense_96_to_32"), ("dense_128_to_32", "dense_128_to_32"),
                                                  ("dense_160_to_32", "dense_160_to_32"), ("dense_192_to_64_one_residual", "dense_192_to_64"),
                                                  ("dense_192_to_64_two_residuals", "dense_192_to_64"), ("conv_up1", "conv_up1_on_an_upsampled_input"),
                                                  ("conv_up2_band", "conv_64_to_64_band"), ("conv_hr_band", "conv_64_to_64_band"),
                                                  ("tail_band", "tail_conv_64_to_3_band")) if k[n]["median_ms"] > e[m]["median_ms"])
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
