"""Host ingest against device ingest (vspbfr_amd/resample.py, csrc/resample.hip), on sources synthesised in a temporary directory:

  restore    images/s of RestoreTestSet stacked on the main thread (what the inference CLIs do) and of imageio.DeviceRestoreLoader, for
             1024^2 PNG and JPEG sources to 512^2, B = 8, each window ending in a device synchronise; for the JPEG sources also the
             loader with decode="device" (the device JPEG decoder feeding the resize) beside decode="host", at 8 pool
             threads and at 2 (a rank's share of 16 CPUs with 8 ranks on a node)
  train      images/s of trainset.DegradeLoader(resize="host") and (resize="device") over the same PNG sources (degradation included)
  host_split one thread: decode alone and decode + LANCZOS cover resize + crop per image (what the resize is of the host cost)
  resize     device time of one vsp_lanczos_resize_u8 call for 8 images 1024^2 -> 512^2 (both launches, upload excluded): HIP events,
             median of 30 after a warm-up; bytes moved from the shapes
  cli        the dataset loop of vspbfr_amd.restoration_metrics (tester_restore_ddpm between device synchronisations) with --ingest host
             and --ingest device over 64 pairs of 512^2 PNGs, --batch 8 --timesteps 4 --no_sample (the settings of
             profiles/metrics_cli_overhead.json; sources of the target size, so this one moves only the decode), alternating, five each
  cli_jpg    the same loop over JPEG pairs with --ingest host, --ingest device and --ingest device --decode device

    python tools/bench_ingest.py [--out profiles/ingest_bench.json] [--skip-cli] [--only restore_jpg,resize,cli_jpg]
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

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def face_like(rng, size):
    y, x = np.mgrid[0:size, 0:size]
    base = np.stack([0.5 + 0.3 * np.sin(x / (19.0 + c) + rng.random() * 6) * np.cos(y / (27.0 + c)) for c in range(3)], axis=2)
    return (np.clip(base + 0.04 * rng.standard_normal((size, size, 3)), 0, 1) * 255).astype(np.uint8)


def write_images(d, n, size, ext, rng):
    from PIL import Image
    os.makedirs(d, exist_ok=True)
    big = face_like(rng, size)
    for i in range(n):
        Image.fromarray(np.roll(big, 37 * i, axis=1)).save(os.path.join(d, f"{i:03d}.{ext}"), **({"quality": 95} if ext == "jpg" else {}))


def rate(fn, n_images, repeats=3):
    """images/s of fn() (which ends in a device synchronise): best and all of `repeats` runs after one warm run"""
    fn()
    runs = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        runs.append(n_images / (time.perf_counter() - t0))
    return {"images_per_s": round(statistics.median(runs), 1), "runs": [round(r, 1) for r in runs]}


def bench_restore(root, B, size, device_decode=False):
    from vspbfr_amd.imageio import DeviceRestoreLoader, RestoreTestSet
    data = RestoreTestSet(root, None, (size, size))
    n = len(data)

    def host():
        for s in range(0, n, B):
            low = torch.stack([data[i] for i in range(s, min(s + B, n))]).cuda(non_blocking=True)
        torch.cuda.synchronize()
        return low

    def device():
        for _, low, _ in DeviceRestoreLoader(data, B, "cuda"):
            pass
        torch.cuda.synchronize()
        return low

    assert torch.equal(host(), device())
    res = {"main_thread_stack": rate(host, n), "device_loader": rate(device, n)}
    if device_decode:
        def loader(threads, decode):
            def run():
                it = DeviceRestoreLoader(data, B, "cuda", threads=threads, decode=decode)
                for _, low, _ in it:
                    pass
                torch.cuda.synchronize()
                run.how = it.how
                return low
            return run
        last = host()
        for threads in (8, 2):
            for decode in ("host", "device"):
                fn = loader(threads, decode)
                assert torch.equal(last, fn())
                res[f"device_loader_decode_{decode}_threads_{threads}"] = rate(fn, n)
        res["files_decoded_on_the_device"] = sum(v == "device" for v in fn.how.values())
    return res


def bench_train(root, B, size):
    from vspbfr_amd.trainset import DegradeLoader, ImageFolder_restore_free_form
    ds = ImageFolder_restore_free_form(root, im_size=(size, size))
    out = {}
    for mode in ("host", "device"):
        loader = DegradeLoader(ds, B, device="cuda", resize=mode, threads=4)

        def run(loader=loader):
            for e in range(2):
                for batch in loader.epoch(e):
                    pass
            torch.cuda.synchronize()

        out[mode] = rate(run, 2 * (len(ds) // B) * B)
    return out


def bench_host_split(root, size, n=8):
    from PIL import Image
    from vspbfr_amd.imageio import list_images, load_image
    paths = list_images(root)[:n]
    out = {}
    for name, fn in (("decode_ms", lambda p: Image.open(p).convert("RGB")), ("decode_resize_crop_ms", lambda p: load_image(p, (size, size)))):
        fn(paths[0])
        t0 = time.perf_counter()
        for p in paths:
            fn(p)
        out[name] = round((time.perf_counter() - t0) / len(paths) * 1000, 2)
    return out


def bench_resize_call(B, src_size, size, rng):
    from vspbfr_amd import hip_ops as H
    from vspbfr_amd.resample import ResamplePlan
    srcs = [face_like(rng, src_size) for _ in range(2)]
    plan = ResamplePlan([srcs[i % 2] for i in range(B)], [(size, size)] * B, [(0, 0)] * B, (size, size))
    host, nb, c0, s0 = plan.pack()
    dev = host.cuda()
    sect = (dev[:nb], dev[c0:c0 + plan.coef.nbytes], dev[s0:])
    res = {}
    for name, kw in (("f32_nchw", dict(u8=False, f32=True)), ("u8_nhwc", dict(u8=True, f32=False))):
        for _ in range(5):
            H.lanczos_resize_u8(plan, *sect, **kw)
        torch.cuda.synchronize()
        ms = []
        for _ in range(30):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record()
            H.lanczos_resize_u8(plan, *sect, **kw)
            b.record()
            b.synchronize()
            ms.append(a.elapsed_time(b))
        out_bytes = B * size * size * 3 * (4 if kw["f32"] else 1)
        moved = plan.src_bytes + 2 * plan.work_bytes + out_bytes          # source read, intermediate written and read, output written
        med = statistics.median(ms)
        res[name] = {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
                     "bytes_moved_mb": round(moved / 1e6, 2), "gb_per_s": round(moved / med / 1e6, 1)}
    res["what"] = f"{B} images {src_size}^2 -> {size}^2, one call = horizontal + vertical launch; ksize {plan.items[0].hk}"
    return res


def bench_cli(tmp, rng, pairs=64, size=512, B=8, ext="png", modes=(("host", "host", None), ("device", "device", None))):
    """modes: (name, --ingest, --decode)"""
    from PIL import Image
    from vspbfr_amd import restoration_metrics as RM
    from vspbfr_amd.diffusion import Code_diffuser
    from vspbfr_amd.e4e import E4e_embedding, Encoder4Editing, Generator
    from vspbfr_amd.pipeline import RestorationPipeline, load_ddpm
    from vspbfr_amd.restorenet import Restoration_net
    torch.manual_seed(0)
    ck = os.path.join(tmp, "ckpt_" + ext)
    os.makedirs(ck)
    torch.save({"att_mapper": Code_diffuser(timesteps=4).state_dict()}, os.path.join(ck, "code_diffuser.pt"))
    enc, dec = Encoder4Editing(50, "ir_se", Namespace(input_channel=3, stylegan_size=1024)), Generator(1024, 512, 8)
    sd = {"encoder." + k: v for k, v in enc.state_dict().items()}
    sd.update({"decoder." + k: v for k, v in dec.state_dict().items()})
    torch.save({"state_dict": sd, "latent_avg": torch.zeros(18, 512),
                "opts": {"encoder_type": "Encoder4Editing", "stylegan_size": 1024, "start_from_latent_avg": True}},
               os.path.join(ck, "psp.pt"))
    del enc, dec, sd
    lq, hq = os.path.join(tmp, "cli_lq_" + ext), os.path.join(tmp, "cli_hq_" + ext)
    write_images(lq, pairs, size, ext, rng)
    write_images(hq, pairs, size, ext, rng)
    device = torch.device("cuda", 0)
    g_ema = Restoration_net(size, 512, 8).to(device).eval()
    psp = E4e_embedding(os.path.join(ck, "psp.pt"), out_size=size, size=1024, device=device, use_generator=True)
    pipe = RestorationPipeline(g_ema, psp, load_ddpm(os.path.join(ck, "code_diffuser.pt"), device=device, timesteps=4), mixing=0.5,
                               with_sample=False)
    times = {name: [] for name, _, _ in modes}
    for rep in range(6):                       # the first of each is the warm run
        for mode, ingest, decode in modes:
            args = Namespace(batch=B, size=size, debug=False, metrics=False, ingest=ingest, decode=decode)
            torch.manual_seed(123)
            random.seed(123)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            RM.tester_restore_ddpm(args, pipe, lq, hq, os.path.join(tmp, f"eval_{ext}_{mode}_{rep}"), "demo", device)
            torch.cuda.synchronize()
            if rep:
                times[mode].append(time.perf_counter() - t0)
    res = {"what": f"{pairs} pairs of {size}^2 {ext.upper()}, --batch {B} --timesteps 4 --no_sample, dataset loop between synchronisations, "
                   "alternating"}
    for name, _, _ in modes:
        res[f"{name}_loop_s"] = times[name]
        res[f"{name}_loop_median_s"] = statistics.median(times[name])
    return res


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--images", type=int, default=32, help="sources per format")
    ap.add_argument("--skip-cli", action="store_true")
    ap.add_argument("--only", default=None, help="comma-separated sections: restore_png, restore_jpg, train, resize, cli, cli_jpg")
    a = ap.parse_args()
    want = None if a.only is None else set(a.only.split(","))

    def on(name):
        return want is None or name in want
    if not torch.cuda.is_available():
        raise SystemExit("bench_ingest: no GPU")
    import PIL
    rng = np.random.default_rng(0)
    B, S = 8, 512
    res = {"what": "1024^2 sources -> 512^2, B = 8; host = PIL on this machine's CPUs", "pillow": PIL.__version__,
           "cpus_used": len(os.sched_getaffinity(0))}
    with tempfile.TemporaryDirectory() as d:
        for ext in ("png", "jpg"):
            if on(f"restore_{ext}") or (ext == "png" and on("train")):
                write_images(os.path.join(d, ext), a.images, 1024, ext, rng)
            if on(f"restore_{ext}"):
                res[f"restore_{ext}"] = bench_restore(os.path.join(d, ext), B, S, device_decode=ext == "jpg")
                res[f"host_split_{ext}"] = bench_host_split(os.path.join(d, ext), S)
        if on("train"):
            res["train_png"] = bench_train(os.path.join(d, "png"), B, S)
        if on("resize"):
            res["resize_call"] = bench_resize_call(B, 1024, S, rng)
        if not a.skip_cli and on("cli"):
            res["cli"] = bench_cli(d, rng)
        if not a.skip_cli and on("cli_jpg"):
            res["cli_jpg"] = bench_cli(d, rng, ext="jpg", modes=(("host", "host", None), ("device", "device", None),
                                                                 ("device_decode", "device", "device")))
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
