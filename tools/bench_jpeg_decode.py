"""The device JPEG decoder (vspbfr_amd/jpeg.py, csrc/jpeg_decode.hip) against Pillow on the same host.  Contents: 8 photos of
1024 x 1536, smooth (an upsampled Gaussian field + N(0, 3^2)) and white noise, quality 90, 4:2:0, without a restart interval and with
one of 8 MCUs.

  kernels      the launches of one vsp_jpeg_decode_u8 call alone: the entry called on buffers allocated and tables uploaded beforehand,
               HIP events, median of 30 after a warm-up, at the default sub_bytes; `rounds` = the entry's round counts
  call         the same window around hip_ops.jpeg_decode: layout, allocations, the pinned block's upload and the launches
  files        wall time of jpeg.decode_files (reading, parsing, upload, the call, the status words)
  pillow       Image.open(f).convert("RGB") over the same files, serially and on 8 threads, ms per batch
  sweep        `kernels` over sub_bytes 16 .. 512: the default (hip_ops.JPEG_DEC_SUB_BYTES) is taken from here
  cli          the dataset loop of vspbfr_amd.restore_photos over the 8 photos of tools/bench_photo.py's CLI loop written as JPEG
               (quality 90, 4:2:0), --batch 8 --timesteps 4 --no_sample, random weights: --decode host against --decode device,
               alternating, three each after a warm run; `host_decode_s` is the `_decode` line of that loop alone

    python tools/bench_jpeg_decode.py [--out profiles/jpeg_dec_bench.json] [--skip-cli] [--skip-sweep]
"""
import argparse
import ctypes as Ct
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
sys.path.insert(0, os.path.join(ROOT, "tools"))

from bench_jpeg import events, image  # noqa: E402

SWEEP = (16, 32, 64, 128, 256, 512)


def jpeg_bytes(arr, restart):
    from PIL import Image
    buf = io.BytesIO()
    kw = dict(restart_marker_blocks=restart) if restart else {}
    Image.fromarray(arr).save(buf, format="JPEG", quality=90, subsampling=2, **kw)
    return buf.getvalue()


def entry_alone(datas, sub_bytes):
    """the entry on buffers made beforehand -> (call, status, rounds)"""
    from vspbfr_amd import hip_ops as H, jpeg
    from vspbfr_amd._lib import JpegDecItem, lib
    scans = [jpeg.parse(d)[0] for d in datas]
    comp = torch.from_numpy(np.concatenate([np.frombuffer(d, dtype=np.uint8, offset=s.offset) for d, s in zip(datas, scans)])).cuda()
    specs, at = [], 0
    for s in scans:
        specs.append((at, s.length, s.h, s.w, jpeg.SUBSAMPLING[s.subsampling], s.restart))
        at += s.length
    rows, out_bytes, work_bytes = H.jpeg_decode_layout(specs, sub_bytes)
    n = len(rows)
    items = (JpegDecItem * n)(*[JpegDecItem(*r) for r in rows])
    tables = np.concatenate([s.tables() for s in scans])
    items_dev = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).cuda()
    tables_dev = torch.from_numpy(tables).cuda()
    out, work = (torch.empty(k, device="cuda", dtype=torch.uint8) for k in (out_bytes, work_bytes))
    status, rounds = (torch.empty(n, device="cuda", dtype=torch.int32) for _ in range(2))

    def call():
        rc = lib.vsp_jpeg_decode_u8(H._ptr(out), out_bytes, H._ptr(status), H._ptr(rounds), H._ptr(work), work_bytes, H._ptr(comp), comp.numel(),
                                    Ct.cast(items, Ct.c_void_p), H._ptr(items_dev), tables.ctypes.data, H._ptr(tables_dev), n, sub_bytes, H._stream())
        assert rc == 0, rc
    return call, status, rounds, (comp, specs, tables)


def bench(kind, restart, tmp, sweep):
    from PIL import Image
    from vspbfr_amd import hip_ops as H, jpeg
    imgs = [image(kind, 1024, 1536, i) for i in range(8)]
    datas = [jpeg_bytes(a, restart) for a in imgs]
    paths = []
    for i, d in enumerate(datas):
        paths.append(os.path.join(tmp, f"{kind}_{restart}_{i}.jpg"))
        with open(paths[-1], "wb") as f:
            f.write(d)

    def pil(p):
        return np.asarray(Image.open(p).convert("RGB"))

    ref = [pil(p) for p in paths]
    packed, sizes, offsets, how = jpeg.decode_files(paths, "cuda")
    host = packed.cpu().numpy()
    assert how == ["device"] * 8 and all(np.array_equal(host[o:o + r.size].reshape(r.shape), r) for o, r in zip(offsets, ref))
    call, status, rounds, (comp, specs, tables) = entry_alone(datas, H.JPEG_DEC_SUB_BYTES)
    res = {"kind": kind, "restart": restart, "file_bytes": sum(len(d) for d in datas), "sub_bytes": H.JPEG_DEC_SUB_BYTES, "kernels": events(call)}
    assert status.cpu().abs().sum().item() == 0
    res["rounds"] = rounds.cpu().tolist()
    res["call"] = events(lambda: H.jpeg_decode(comp, specs, tables))
    wall = []
    for _ in range(5):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        jpeg.decode_files(paths, "cuda")
        torch.cuda.synchronize()
        wall.append((time.perf_counter() - t0) * 1e3)
    res["files_wall_ms_median"] = round(statistics.median(wall), 3)
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        for p in paths:
            pil(p)
        t.append((time.perf_counter() - t0) * 1e3)
    res["pillow_serial_ms"] = round(min(t), 3)
    with ThreadPoolExecutor(max_workers=8) as pool:
        t = []
        for _ in range(3):
            t0 = time.perf_counter()
            list(pool.map(pil, paths))
            t.append((time.perf_counter() - t0) * 1e3)
    res["pillow_8_threads_ms"] = round(min(t), 3)
    if sweep:
        res["sweep"] = {}
        for sb in SWEEP:
            c, _, r, _ = entry_alone(datas, sb)
            res["sweep"][str(sb)] = dict(events(c, n=10, warm=2), max_rounds=int(r.cpu().max()))
    return res


def bench_cli(tmp):
    import random
    from PIL import Image
    import bench_photo
    from vspbfr_amd import hip_ops as H, restore_photos as RP
    restorer, root, names, landmarks, device = bench_photo.cli_setup(tmp, *bench_photo.workload())
    jroot = os.path.join(tmp, "photos_jpg")
    os.makedirs(jroot)
    jnames = [os.path.splitext(n)[0] + ".jpg" for n in names]
    for n, j in zip(names, jnames):
        Image.open(os.path.join(root, n)).save(os.path.join(jroot, j), quality=90, subsampling=2)
    marks = {j: landmarks[n] for n, j in zip(names, jnames)}
    t = []
    for _ in range(3):
        t0 = time.perf_counter()
        for j in jnames:
            RP._decode(os.path.join(jroot, j))
        t.append(time.perf_counter() - t0)
    times = {"host": [], "device": []}
    for rep in range(4):                       # the first of each is the warm run
        for route in times:
            args = Namespace(photos=jroot, out=os.path.join(tmp, f"out_{route}_{rep}"), batch=8, save_faces=False, upscale=1, size=512, inset=8,
                             feather=48, format="png", decode=route)
            torch.manual_seed(123)
            random.seed(123)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            RP.restore_photos(args, restorer, jnames, marks, device)
            torch.cuda.synchronize()
            if rep:
                times[route].append(round(time.perf_counter() - t0, 4))
    same = all(open(os.path.join(tmp, "out_host_3", f), "rb").read() == open(os.path.join(tmp, "out_device_3", f), "rb").read()
               for f in os.listdir(os.path.join(tmp, "out_host_3")) if f.endswith(".png"))
    return {"what": "8 JPEG photos of 1024 x 1536 (quality 90, 4:2:0), 16 faces, --batch 8 --timesteps 4 --no_sample, decode + restore + PNG, "
                    "writers drained, alternating, three each after a warm run", "sub_bytes": H.JPEG_DEC_SUB_BYTES,
            "host_decode_s": round(min(t), 4), "loop_s": times, "loop_median_s": {r: statistics.median(v) for r, v in times.items()},
            "equal_files": bool(same)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "jpeg_dec_bench.json"))
    ap.add_argument("--skip-cli", action="store_true")
    ap.add_argument("--skip-sweep", action="store_true")
    args = ap.parse_args()
    res = {"device": torch.cuda.get_device_name(0), "quality": 90, "subsampling": "420", "runs": []}

    def save():
        os.makedirs(os.path.dirname(args.out), exist_ok=True)
        with open(args.out, "w") as f:
            json.dump(res, f, indent=1)

    with tempfile.TemporaryDirectory() as d:
        for kind in ("smooth", "noise"):
            for restart in (0, 8):
                r = bench(kind, restart, d, not args.skip_sweep)
                print(json.dumps(r), flush=True)
                res["runs"].append(r)
                save()
    if not args.skip_cli:
        with tempfile.TemporaryDirectory() as d:
            res["cli"] = bench_cli(d)
        print(json.dumps(res["cli"]), flush=True)
    save()


if __name__ == "__main__":
    main()
