"""The face parser (vspbfr_amd/parse.py, csrc/parse.hip) at S = 512 with random weights:

  kernels   device time of the head, of every convolution class between head and tail by (Cin, Cout, input map, stride, up), of the tail
            and of the blur, for --faces faces in one launch (default 16: the chunk FaceParser uses at 512) -- HIP events, median of 30 after a warm-up; TFLOP/s and the share of the f16 MFMA peak per class
  paste     paste_faces over 8 photos of 1024 x 1536 with 16 faces, through a mask and without one
  eager     torch-ROCm eager fp16 conv2d on channels-last tensors with the same folded weights in the same run -- the yardstick; the
            reflection padding (and the nearest x2) are made beforehand and not timed, the bias is in the call, LeakyReLU and residuals
            are not (they would be further eager launches)
  mask      one FaceParser.mask() call for 16 faces (one chunk: 46 launches, and the blur's 4)
  restorer  one PhotoRestorer call over 8 photos of 1024 x 1536 with 16 faces and a stand-in pipeline, with and without the parser

  cli       the loop of vspbfr_amd.restore_photos over the 8 photos (set-up of tools/bench_photo.py: --batch 8 --timesteps 4 --no_sample)
            with and without the parser, alternating, three each after a warm run

    python tools/bench_parse.py [--out profiles/parse_bench.json] [--faces 16] [--skip-cli]
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
PIPELINE_STEP_MS = 39.0           # one restoration pipeline step at batch 8
S = 512


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


def layer_classes():
    """[(label, layer name, cin, cout, input map, stride, up, count in the network)] of the convolutions between head and tail"""
    from vspbfr_amd import parse as P
    out, h = [], S
    for prefix, ci, co, scale in P.blocks():
        if scale == "down":
            out += [(f"{prefix}.shortcut", ci, co, h, 2, False), (f"{prefix}.conv1", ci, co, h, 1, False), (f"{prefix}.conv2", co, co, h, 2, False)]
            h //= 2
        elif scale == "up":
            out += [(f"{prefix}.shortcut", ci, co, h, 1, True), (f"{prefix}.conv1", ci, co, h, 1, True), (f"{prefix}.conv2", co, co, 2 * h, 1, False)]
            h *= 2
        else:
            out += [(f"{prefix}.conv1", ci, co, h, 1, False), (f"{prefix}.conv2", co, co, h, 1, False)]
    classes = {}
    for name, ci, co, hh, st, up in out:
        key = (ci, co, hh, st, up)
        classes.setdefault(key, [name, 0])[1] += 1
    return [(f"{ci}->{co} at {hh}^2" + (" stride 2" if st == 2 else "") + (" up" if up else ""), name, ci, co, hh, st, up, cnt)
            for (ci, co, hh, st, up), (name, cnt) in classes.items()]


def bench_kernels(net, folded, faces):
    from vspbfr_amd import hip_ops as H
    dev = "cuda"
    rows = []
    crops = torch.randint(0, 256, (faces, S, S, 3), dtype=torch.uint8, device=dev)
    big = faces * S * S * 128
    a, b = (torch.randn(big, device=dev).mul_(0.5).half() for _ in range(2))
    r = events(lambda: H.parse_head_u8(a[:faces * S * S * 64], crops, *net.head))
    flop = 2.0 * 27 * 64 * faces * S * S
    rows.append(dict(r, layer="head 3->64 at 512^2", count=1, gflop=round(flop / 1e9, 2)))
    total = r["median_ms"]
    for label, name, ci, co, hh, st, up, cnt in layer_classes():
        oh, _ = H.parse_conv_out(hh, hh, st, up)
        w_img, bias = net.layers[name]
        x, y = a[:faces * hh * hh * ci], b[:faces * oh * oh * co]
        r = events(lambda: H.parse_conv_f16(y, x, faces, hh, hh, w_img, bias, stride=st, up=up, act=True, res1=y))
        flop = 2.0 * 9 * ci * co * faces * oh * oh
        tf = flop / r["median_ms"] / 1e9
        row = dict(r, layer=label, count=cnt, gflop=round(flop / 1e9, 2), tflops=round(tf, 1),
                   percent_of_f16_mfma_peak=round(100 * tf / F16_MFMA_PEAK_TFLOPS, 2))
        # the yardstick: eager fp16 channels-last on the same folded weights; padding and upsampling made beforehand
        wt = folded[name][0].to(dev).half().contiguous(memory_format=torch.channels_last)
        bt = folded[name][1].to(dev).half()
        xe = torch.randn(faces, ci, hh, hh, device=dev).mul_(0.5).half()
        if up:
            xe = F.interpolate(xe, scale_factor=2, mode="nearest")
        xe = F.pad(xe, (1, 1, 1, 1), mode="reflect").contiguous(memory_format=torch.channels_last)
        e = events(lambda: F.conv2d(xe, wt, bt, stride=st), n=30, warm=3)
        row.update(eager_median_ms=e["median_ms"], hip_over_eager=round(r["median_ms"] / e["median_ms"], 3))
        del xe, wt
        rows.append(row)
        total += cnt * r["median_ms"]
    feats = a[:faces * S * S * 64]
    r = events(lambda: H.parse_mask_u8(feats, faces, S, S, *net.tail))
    rows.append(dict(r, layer="tail 64->19 at 512^2, argmax, keep", count=1, gflop=round(2.0 * 576 * 19 * faces * S * S / 1e9, 2)))
    total += r["median_ms"]
    from vspbfr_amd import parse as P
    keep = (torch.rand(faces, S, S, device=dev) < 0.5).to(torch.uint8)
    taps, border = P.default_taps(S), P.default_border(S)
    work = torch.empty(2 * faces * S * S, dtype=torch.uint16, device=dev)
    out = torch.empty((faces, S, S), dtype=torch.uint16, device=dev)
    r = events(lambda: H.parse_blur_u16(keep, taps, border, out=out, work=work))
    rows.append(dict(r, layer="blur (4 passes, R = 50) at 512^2", count=1))
    total += r["median_ms"]
    return rows, round(total, 3)


def bench_paste():
    import bench_photo
    from vspbfr_amd import photo as PH
    photos, landmarks = bench_photo.workload()
    faces = [(k, pts) for k, per in enumerate(landmarks) for pts in per]
    res = {"what": "paste_faces, 8 photos of 1024 x 1536, 16 faces of 512^2, in place on one output buffer"}
    for tag, aa in (("bilinear", False), ("antialias", True)):
        plan = PH.FacePlan(photos, faces, size=S, antialias=aa)
        out = plan.background("cuda")
        restored = torch.randint(0, 256, (plan.n, S, S, 3), dtype=torch.uint8, device="cuda")
        mask = torch.from_numpy(np.random.default_rng(1).integers(0, 257, (plan.n, S, S)).astype(np.uint16)).cuda()
        res[tag] = {"unmasked": events(lambda: PH.paste_faces(plan, restored, "cuda", out=out)),
                    "masked": events(lambda: PH.paste_faces(plan, restored, "cuda", out=out, mask=mask))}
    return res


class _Pipe:
    def __call__(self, low):
        return {"restored": low * 0.9}


def bench_restorer(net):
    import bench_photo
    from vspbfr_amd import photo as PH
    photos, landmarks = bench_photo.workload()
    res = {"what": "8 photos of 1024 x 1536, 16 faces, a pointwise stand-in for the pipeline: crop + quantise + [parser +] paste"}
    for tag, parser in (("without_parser", None), ("with_parser", net)):
        rest = PH.PhotoRestorer(_Pipe(), 8, upscale=1, size=S, parser=parser)
        res[tag] = events(lambda: rest(photos, landmarks, "cuda"), n=10, warm=2)
    return res


def bench_cli(tmp, net):
    import bench_photo
    from vspbfr_amd import restore_photos as RP
    restorer, root, names, landmarks, device = bench_photo.cli_setup(tmp, *bench_photo.workload())
    times = {"plain": [], "parse_weights": []}
    for rep in range(4):                       # the first of each is the warm run
        for route in ("plain", "parse_weights"):
            restorer.parser = net if route == "parse_weights" else None
            args = Namespace(photos=root, out=os.path.join(tmp, f"out_{route}_{rep}"), batch=8, save_faces=False, upscale=1, size=S, inset=8,
                             feather=48, antialias=False)
            torch.manual_seed(123)
            random.seed(123)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            RP.restore_photos(args, restorer, names, landmarks, device)
            torch.cuda.synchronize()
            if rep:
                times[route].append(round(time.perf_counter() - t0, 4))
    return {"what": "8 photos of 1024 x 1536, 16 faces, --batch 8 --timesteps 4 --no_sample, decode + restore + PNG files by Pillow, writers "
                    "drained; without and with a parser, alternating, three each after a warm run",
            "cpus_used": len(os.sched_getaffinity(0)), "loop_s": times, "loop_median_s": {r: statistics.median(t) for r, t in times.items()}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--faces", type=int, default=16)
    ap.add_argument("--skip-cli", action="store_true")
    ap.add_argument("--skip-restorer", action="store_true")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_parse: no GPU")
    import parse_ref as R
    from vspbfr_amd import parse as P
    sd = R.make_state(seed=1)
    folded = P.fold_state(sd)
    net = P.FaceParser(sd, "cuda")
    res = {"device": torch.cuda.get_device_name(0), "model": "ParseNet at S = 512, random weights (tests/parse_ref.make_state)",
           "timing": "HIP events around the call, median of 30 after a warm-up (10 for whole calls)",
           "faces_per_launch": a.faces, "peaks_used": {"f16_mfma_tflops": F16_MFMA_PEAK_TFLOPS}}
    res["kernels"], res["sum_over_the_network_ms"] = bench_kernels(net, folded, a.faces)
    torch.cuda.empty_cache()
    crops = torch.randint(0, 256, (16, S, S, 3), dtype=torch.uint8, device="cuda")
    res["mask_call_16_faces"] = events(lambda: net.mask(crops), n=10, warm=2)
    res["mask_call_16_faces"]["share_of_a_39_ms_pipeline_step_per_8_faces"] = round(res["mask_call_16_faces"]["median_ms"] / 2 / PIPELINE_STEP_MS, 3)
    if not a.skip_restorer:
        res["paste"] = bench_paste()
        res["restorer"] = bench_restorer(net)
    if not a.skip_cli:
        torch.cuda.empty_cache()
        with tempfile.TemporaryDirectory() as tmp:
            res["cli"] = bench_cli(tmp, net)
    text = json.dumps(res, indent=1)
    print(text)
    if a.out:
        with open(a.out, "w") as f:
            f.write(text + "\n")


if __name__ == "__main__":
    main()
