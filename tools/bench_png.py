"""The device PNG encoder (vspbfr_amd/png.py, csrc/png.hip) against PIL on the same host:

  encode_call  device time of one vsp_png_encode_u8 call, B = 8 at 512^2 RGB, HIP events, median of 30 after a warm-up, for three kinds of
               image: smooth (a 16x-upsampled Gaussian field + N(0, 3^2)), white noise, two-level
  pil          Image.save of the same images with 1 thread and with the writer's 8 (ms per image)
  sizes        file sizes against PIL's default
  cli          the dataset loop of vspbfr_amd.restoration_metrics (tester_restore_ddpm between device synchronisations) with --encode host
               and --encode device over 64 pairs of 512^2 PNGs, --batch 8 --timesteps 4 --no_sample --ingest device, alternating, five
               each after a warm run (the protocol of profiles/ingest_bench.json)

    python tools/bench_png.py [--out profiles/png_bench.json] [--skip-cli]

--ragged: the ragged encoder for whole photos (vsp_png_encode_ragged_u8) instead:

  kernels      the three kernels of one call alone -- the entry on buffers allocated and an item table uploaded beforehand -- for 8 photos
               of 1024 x 1536 and of 2048 x 3072, smooth, white noise and two-level, HIP events, median of 30 after a warm-up
  call         the same window around hip_ops.png_encode_ragged: the layout, the allocations, the item table's upload and the kernels
  files        wall time of png.encode_ragged (the call, the copies of the used bytes, the host framing)
  pil          Image.save of the same photos on 1 and on 8 threads in the same run, and the file sizes against PIL's default
  uniform      the smooth row of the default mode again (vsp_png_encode_u8, B = 8 at 512^2): the compress stage is shared
  cli          the dataset loop of vspbfr_amd.restore_photos over the 8 photos of tools/bench_photo.py's CLI loop, --batch 8
               --timesteps 4 --no_sample: --format png (host), --png_encode device and --format jpg --encode device, alternating,
               three each after a warm run, writers drained

    python tools/bench_png.py --ragged [--out profiles/png_ragged_bench.json] [--skip-cli] [--uniform-only]
"""
import argparse
import io
import json
import os
import random
import statistics
import sys
import tempfile
import time
from argparse import Namespace
from concurrent.futures import ThreadPoolExecutor

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))
sys.path.insert(0, os.path.join(ROOT, "tools"))


def pil_bytes(arr):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="PNG")
    return buf.getvalue()


def bench_kind(kind, B=8, S=512):
    import png_ref as R
    from vspbfr_amd import hip_ops as H, png
    imgs = np.ascontiguousarray(np.stack([R.named_image(kind, S, S, 3, seed=i) for i in range(B)]))
    dev = torch.from_numpy(imgs).cuda()
    files = png.encode_batch(dev)
    assert files[0] == R.encode_png(imgs[0])
    for _ in range(5):
        H.png_encode(dev)
    torch.cuda.synchronize()
    ms = []
    for _ in range(30):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        H.png_encode(dev)
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    t0 = time.perf_counter()
    for _ in range(3):
        job = png.enqueue(dev)
        job.files()
    end_to_end = (time.perf_counter() - t0) / 3
    pil = {}
    for threads in (1, 8):
        with ThreadPoolExecutor(max_workers=threads) as pool:
            list(pool.map(pil_bytes, imgs))
            t0 = time.perf_counter()
            ref = list(pool.map(pil_bytes, imgs))
            pil[f"threads_{threads}_ms_per_image"] = round((time.perf_counter() - t0) / B * 1000, 2)
    return {"device_call_median_ms": round(statistics.median(ms), 4), "device_call_min_ms": round(min(ms), 4),
            "device_call_max_ms": round(max(ms), 4), "enqueue_to_files_ms_per_batch": round(end_to_end * 1000, 2), "pil_save": pil,
            "file_bytes_device": [len(f) for f in files], "file_bytes_pil": [len(f) for f in ref]}


def bench_cli(tmp, pairs=64, size=512, B=8):
    from bench_ingest import write_images
    from vspbfr_amd import restoration_metrics as RM
    from vspbfr_amd.diffusion import Code_diffuser
    from vspbfr_amd.e4e import E4e_embedding, Encoder4Editing, Generator
    from vspbfr_amd.pipeline import RestorationPipeline, load_ddpm
    from vspbfr_amd.restorenet import Restoration_net
    rng = np.random.default_rng(0)
    torch.manual_seed(0)
    ck = os.path.join(tmp, "ckpt")
    os.makedirs(ck)
    torch.save({"att_mapper": Code_diffuser(timesteps=4).state_dict()}, os.path.join(ck, "code_diffuser.pt"))
    enc, dec = Encoder4Editing(50, "ir_se", Namespace(input_channel=3, stylegan_size=1024)), Generator(1024, 512, 8)
    sd = {"encoder." + k: v for k, v in enc.state_dict().items()}
    sd.update({"decoder." + k: v for k, v in dec.state_dict().items()})
    torch.save({"state_dict": sd, "latent_avg": torch.zeros(18, 512),
                "opts": {"encoder_type": "Encoder4Editing", "stylegan_size": 1024, "start_from_latent_avg": True}}, os.path.join(ck, "psp.pt"))
    del enc, dec, sd
    lq, hq = os.path.join(tmp, "cli_lq"), os.path.join(tmp, "cli_hq")
    write_images(lq, pairs, size, "png", rng)
    write_images(hq, pairs, size, "png", rng)
    device = torch.device("cuda", 0)
    g_ema = Restoration_net(size, 512, 8).to(device).eval()
    psp = E4e_embedding(os.path.join(ck, "psp.pt"), out_size=size, size=1024, device=device, use_generator=True)
    pipe = RestorationPipeline(g_ema, psp, load_ddpm(os.path.join(ck, "code_diffuser.pt"), device=device, timesteps=4), mixing=0.5,
                               with_sample=False)
    times, sizes = {"host": [], "device": []}, {}
    for rep in range(6):                       # the first of each is the warm run
        for mode in ("host", "device"):
            args = Namespace(batch=B, size=size, debug=False, metrics=False, ingest="device", encode=mode)
            torch.manual_seed(123)
            random.seed(123)
            out = os.path.join(tmp, f"eval_{mode}_{rep}")
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            RM.tester_restore_ddpm(args, pipe, lq, hq, out, "demo", device)
            torch.cuda.synchronize()
            if rep:
                times[mode].append(time.perf_counter() - t0)
            sizes[mode] = sum(os.path.getsize(os.path.join(out, f)) for f in os.listdir(out))
    return {"what": f"{pairs} pairs of {size}^2 PNG, --batch {B} --timesteps 4 --no_sample --ingest device, dataset loop between "
                    "synchronisations (the writer drained), alternating",
            "encode_host_loop_s": times["host"], "encode_device_loop_s": times["device"],
            "encode_host_median_s": statistics.median(times["host"]), "encode_device_median_s": statistics.median(times["device"]),
            "output_bytes": sizes}


def events(fn, n=30, warm=5):
    for _ in range(warm):
        fn()
    torch.cuda.synchronize()
    ms = []
    for _ in range(n):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        torch.cuda.synchronize()
        a.record()
        fn()
        b.record()
        b.synchronize()
        ms.append(a.elapsed_time(b))
    return {"median_ms": round(statistics.median(ms), 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4)}


def ragged_entry_alone(flat, sizes):
    """the entry on buffers made beforehand: what the window around it holds is the three launches"""
    import ctypes as Ct
    from vspbfr_amd import hip_ops as H
    from vspbfr_amd._lib import PngItem, lib
    rows, out_bytes, work_bytes, segs = H.png_ragged_layout(sizes, None, 3)
    n = len(rows)
    items = (PngItem * n)(*[PngItem(*r) for r in rows])
    items_dev = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).cuda()
    out, work = (torch.empty(k, device="cuda", dtype=torch.uint8) for k in (out_bytes, work_bytes))
    idat, adler = torch.empty(n, device="cuda", dtype=torch.int32), torch.empty(2 * segs, device="cuda", dtype=torch.int32)

    def call():
        rc = lib.vsp_png_encode_ragged_u8(H._ptr(out), out_bytes, H._ptr(idat), H._ptr(adler), H._ptr(work), work_bytes, H._ptr(flat),
                                          flat.numel(), Ct.cast(items, Ct.c_void_p), H._ptr(items_dev), n, 3, H._stream())
        assert rc == 0, rc
    return call


def bench_ragged(kind, B, h, w):
    import png_ragged_ref as RR
    import png_ref as R
    from PIL import Image
    from vspbfr_amd import hip_ops as H, png
    imgs = np.ascontiguousarray(np.stack([R.named_image(kind, h, w, 3, seed=i) for i in range(B)]))
    flat, sizes = torch.from_numpy(imgs).cuda().reshape(-1), [(h, w)] * B
    files = png.encode_ragged(flat, sizes)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(files[-1]))), imgs[-1])
    head = imgs[0, :64]                                  # the restatement on a strip: the whole photo takes it seconds
    assert png.encode_ragged(torch.from_numpy(head.copy()).cuda().reshape(-1), [(64, w)]) == [RR.encode_png(head)]
    kernels = events(ragged_entry_alone(flat, sizes))
    call = events(lambda: H.png_encode_ragged(flat, sizes))
    wall = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        png.encode_ragged(flat, sizes)
        wall.append((time.perf_counter() - t0) * 1e3)
    pil = {}
    for threads in (1, 8):
        with ThreadPoolExecutor(max_workers=threads) as pool:
            t0 = time.perf_counter()
            ref = list(pool.map(pil_bytes, imgs))
            pil[f"threads_{threads}_ms_per_batch"] = round((time.perf_counter() - t0) * 1000, 2)
    return {"kind": kind, "batch": B, "h": h, "w": w, "kernels": kernels, "call": call, "files_wall_ms_median": round(statistics.median(wall), 3),
            "pil_save": pil, "file_bytes_device": [len(f) for f in files], "file_bytes_pil": [len(f) for f in ref]}


def bench_ragged_cli(tmp):
    import bench_photo
    from vspbfr_amd import restore_photos as RP
    restorer, root, names, landmarks, device = bench_photo.cli_setup(tmp, *bench_photo.workload())
    routes = {"png_host": dict(format="png"), "png_device": dict(format="png", png_encode="device"),
              "jpg_device": dict(format="jpg", quality=90, subsampling="420", encode="device")}
    times = {r: [] for r in routes}
    for rep in range(4):                       # the first of each is the warm run
        for route, flags in routes.items():
            args = Namespace(photos=root, out=os.path.join(tmp, f"out_{route}_{rep}"), batch=8, save_faces=False, upscale=1, size=512, inset=8,
                             feather=48, **flags)
            torch.manual_seed(123)
            random.seed(123)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            RP.restore_photos(args, restorer, names, landmarks, device)
            torch.cuda.synchronize()
            if rep:
                times[route].append(round(time.perf_counter() - t0, 4))
    sizes = {r: sum(os.path.getsize(os.path.join(tmp, f"out_{r}_3", f)) for f in os.listdir(os.path.join(tmp, f"out_{r}_3")) if f[:2].isdigit())
             for r in routes}
    return {"what": "8 photos of 1024 x 1536, 16 faces, --batch 8 --timesteps 4 --no_sample, decode + restore + write, writers drained, "
                    "alternating, three each after a warm run", "cpus_used": len(os.sched_getaffinity(0)),
            "loop_s": times, "loop_median_s": {r: statistics.median(t) for r, t in times.items()}, "photo_bytes": sizes}


def main_ragged(a):
    import PIL
    res = {"what": "vsp_png_encode_ragged_u8 against PIL on this machine's CPUs", "device": torch.cuda.get_device_name(0),
           "pillow": PIL.__version__, "cpus_used": len(os.sched_getaffinity(0)), "runs": []}
    res["uniform_smooth_512"] = bench_kind("smooth")
    print(json.dumps({"uniform_smooth_512": {k: v for k, v in res["uniform_smooth_512"].items() if k.startswith("device")}}), flush=True)
    if not a.uniform_only:
        for h, w in ((1024, 1536), (2048, 3072)):
            for kind in ("smooth", "noise", "twolevel"):
                r = bench_ragged(kind, 8, h, w)
                print(json.dumps(r), flush=True)
                res["runs"].append(r)
        if not a.skip_cli:
            with tempfile.TemporaryDirectory() as d:
                res["cli"] = bench_ragged_cli(d)
            print(json.dumps(res["cli"]), flush=True)
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-cli", action="store_true")
    ap.add_argument("--ragged", action="store_true", help="the ragged encoder for whole photos instead of the uniform one")
    ap.add_argument("--uniform-only", action="store_true", help="--ragged: only the uniform smooth row (the parent-commit comparison)")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_png: no GPU")
    if a.ragged:
        return main_ragged(a)
    import PIL
    res = {"what": "B = 8 at 512^2 RGB; host = PIL on this machine's CPUs", "pillow": PIL.__version__, "cpus_used": len(os.sched_getaffinity(0))}
    for kind in ("smooth", "noise", "twolevel"):
        res[kind] = bench_kind(kind)
    if not a.skip_cli:
        with tempfile.TemporaryDirectory() as d:
            res["cli"] = bench_cli(d)
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
