"""The device JPEG encoder (vspbfr_amd/jpeg.py, csrc/jpeg.hip) against Pillow on the same host:

  kernels      the three kernels of one vsp_jpeg_encode_u8 call alone: the entry called on buffers allocated and an item table uploaded
               beforehand, HIP events, median of 30 after a warm-up, quality 90, 4:2:0, restart 8: 8 photos of 1024 x 1536 and 16 crops
               of 512 x 512, for a smooth image (an upsampled Gaussian field + N(0, 3^2)) and for white noise (the bit packer's worst
               case: long codes everywhere)
  call         the same window around hip_ops.jpeg_encode: the layout on the host, four allocations, the item table's upload and the
               kernels -- what a caller's stream sees per call
  files        wall time of jpeg.encode_batch (the call, the copies of the used bytes, the host framing)
  pillow       Pillow's JPEG (same parameters) and PNG encoders over the same images on 8 threads, ms per batch
  cli          the dataset loop of vspbfr_amd.restore_photos (between device synchronisations, the writers drained inside) over the 8
               photos of tools/bench_photo.py's CLI loop, --batch 8 --timesteps 4 --no_sample, random weights: --format png against
               --format jpg --encode device and --encode host, alternating, three each after a warm run

    python tools/bench_jpeg.py [--out profiles/jpeg_bench.json] [--skip-cli]
"""
import argparse
import io
import json
import os
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


def image(kind, h, w, seed):
    rng = np.random.RandomState(seed)
    if kind == "noise":
        return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    low = rng.randn(h // 16 + 2, w // 16 + 2, 3) * 50 + 128
    up = np.kron(low, np.ones((16, 16, 1)))[:h, :w]
    k = np.ones(9) / 9
    for ax in (0, 1):
        up = np.apply_along_axis(lambda v: np.convolve(v, k, mode="same"), ax, up)
    return np.clip(np.rint(up + rng.randn(h, w, 3) * 3), 0, 255).astype(np.uint8)


def pil_png(arr):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr).save(buf, format="PNG")
    return len(buf.getvalue())


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


def entry_alone(flat, sizes):
    """the entry on buffers made beforehand: what the window around it holds is the three launches"""
    import ctypes as Ct
    from vspbfr_amd import hip_ops as H
    from vspbfr_amd._lib import JpegItem, lib
    rows, src_bytes, out_bytes, work_bytes, total = H.jpeg_layout(sizes, "420", 8)
    n = len(rows)
    items = (JpegItem * n)(*[JpegItem(*r, 0) for r in rows])
    items_dev = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).cuda()
    out, work = (torch.empty(k, device="cuda", dtype=torch.uint8) for k in (out_bytes, work_bytes))
    ws, totals = (torch.empty(k, device="cuda", dtype=torch.int32) for k in (2 * total, n))

    def call():
        rc = lib.vsp_jpeg_encode_u8(H._ptr(out), out_bytes, H._ptr(totals), H._ptr(work), work_bytes, H._ptr(ws), H._ptr(flat), src_bytes,
                                    Ct.cast(items, Ct.c_void_p), H._ptr(items_dev), n, 90, 2, 8, H._stream())
        assert rc == 0, rc
    return call


def bench(kind, B, h, w):
    import jpeg_ref as R
    from vspbfr_amd import hip_ops as H, jpeg
    imgs = np.stack([image(kind, h, w, i) for i in range(B)])
    dev = torch.from_numpy(imgs).cuda()
    flat, sizes = dev.reshape(-1), [(h, w)] * B
    files = jpeg.encode_batch(dev)
    assert files[0] == R.pillow_file(imgs[0], 90, "420", 8) and files[-1] == R.pillow_file(imgs[-1], 90, "420", 8)
    kernels = events(entry_alone(flat, sizes))
    call = events(lambda: H.jpeg_encode(flat, sizes))
    wall = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        jpeg.encode_batch(dev)
        wall.append((time.perf_counter() - t0) * 1e3)
    pil = {}
    with ThreadPoolExecutor(max_workers=8) as pool:
        for name, fn in (("jpeg", lambda a: len(R.pillow_file(a, 90, "420", 8))), ("png", pil_png)):
            t = []
            for _ in range(3):
                t0 = time.perf_counter()
                nbytes = sum(pool.map(fn, list(imgs)))
                t.append((time.perf_counter() - t0) * 1e3)
            pil[name] = {"ms_per_batch_8_threads": round(min(t), 3), "bytes": int(nbytes)}
    return {"kind": kind, "batch": B, "h": h, "w": w, "kernels": kernels, "call": call, "files_wall_ms_median": round(statistics.median(wall), 3),
            "bytes": int(sum(len(f) for f in files)), "pillow": pil}


def bench_cli(tmp):
    import random
    import bench_photo
    from vspbfr_amd import restore_photos as RP
    restorer, root, names, landmarks, device = bench_photo.cli_setup(tmp, *bench_photo.workload())
    routes = {"png": dict(format="png"), "jpg_device": dict(format="jpg", quality=90, subsampling="420", encode="device"),
              "jpg_host": dict(format="jpg", quality=90, subsampling="420", encode="host")}
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_bench.json"))
    ap.add_argument("--skip-cli", action="store_true")
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "quality": 90, "subsampling": "420", "restart": 8, "runs": []}
    for kind in ("smooth", "noise"):
        for B, h, w in ((8, 1024, 1536), (16, 512, 512)):
            r = bench(kind, B, h, w)
            print(json.dumps(r))
            res["runs"].append(r)
    if not args.skip_cli:
        with tempfile.TemporaryDirectory() as d:
            res["cli"] = bench_cli(d)
        print(json.dumps(res["cli"]))
    os.makedirs(os.path.dirname(args.out), exist_ok=True)
    with open(args.out, "w") as f:
        json.dump(res, f, indent=1)


if __name__ == "__main__":
    main()
