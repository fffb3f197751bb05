"""Device time of the whole-photo face kernels (vspbfr_amd/photo.py, csrc/face_warp.hip) against the same job on the host:

  kernels    16 faces from 8 photos of 1024 x 1536 (two per photo, overlapping, turned and scaled), S = 512, at upscale 1 and 2: one
             vsp_face_crop_u8 call (uint8 + fp32 outputs) and one vsp_face_paste_u8 call, HIP events, median of 30 after a warm-up
             (the paste runs in place on the same buffer every time: its work does not depend on the bytes); bytes written from the shapes
  host       the same crops and pastes by tests/photo_ref.py (NumPy, one thread), once; outputs compared with the device's
  cli        the dataset loop of vspbfr_amd.restore_photos (restore_photos between device synchronisations) over those 8 photos with and
             without --save_faces, --batch 8 --timesteps 4 --no_sample, random weights, alternating, three each after a warm run

    python tools/bench_photo.py [--out profiles/photo_bench.json] [--skip-cli]

  --antialias   instead: the anti-aliased kernels (vsp_face_crop_aa_u8 / vsp_face_paste_aa_u8) against the bilinear ones on the
             same faces -- 16 faces from 8 photos at the same turns, with faces of 256, 1024 and 2048 px (crop minification 0.5 / 2 / 4,
             paste minification 2 / 0.5 / 0.25; the photos grow to 2560 x 3072 for the 2048 px faces), S = 512, upscale 1.  Per size:
             both crops and both pastes, median of 30, the ratio filtered / bilinear and the share of one pipeline step; the first
             face's crop and the first photo's paste are compared with tests/photo_aa_ref.py on the host.

    python tools/bench_photo.py --antialias [--out profiles/photo_aa_bench.json]

  --color_fix MODE   instead: the colour fix (vsp_color_fix_u8; MODE stats, wavelet or both) on the 16 crops of the `kernels`
             workload at upscale 1, beside the crop and the paste of the same run, median of 30; the NumPy restatement
             (tests/color_fix_ref.py) on the host, timed once (its integer elementwise operations run on the calling thread), and
             whether the bytes are equal; the bytes each mode must move -- every buffer counted once, halo re-reads not counted, so
             `effective_gb_per_s` is a floor of the traffic, not a bandwidth measurement.

    python tools/bench_photo.py --color_fix both [--out profiles/color_fix_bench.json]

  --background   instead: FacePlan.background() (the LANCZOS-upscaled photos a group's faces are pasted into) for the 8 photos
             of 1024 x 1536 at upscale 2 and 4, from a plan built from arrays and from one built beside a device buffer
             (device_photos, what `restore_photos --decode device` has): HIP events around the call and the wall time up to a device
             synchronise, median of 30 after a warm-up; the first photo is compared with Pillow's resize.

    python tools/bench_photo.py --background [--out FILE]
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

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

PIPELINE_STEP_MS = 39.0      # one 8-image pipeline step of the flagship benchmark: what "well under 1 %" is measured against


def workload():
    import photo_ref as R
    photos = [R.test_photo(1024, 1536, seed=40 + k) for k in range(8)]
    marks = [[R.landmarks_for(1.4 + 0.1 * k, 9.0 * k - 30.0, (400.0, 600.0)), R.landmarks_for(0.9 + 0.05 * k, 20.0 - 7.0 * k, (620.0, 820.0))]
             for k in range(8)]
    return photos, marks


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
    med = statistics.median(ms)
    return {"median_ms": round(med, 4), "min_ms": round(min(ms), 4), "max_ms": round(max(ms), 4),
            "percent_of_pipeline_step": round(100.0 * med / PIPELINE_STEP_MS, 3)}


def bench_kernels(photos, marks, upscale):
    import photo_ref as R
    from vspbfr_amd import photo as P
    faces = [(k, pts) for k, per in enumerate(marks) for pts in per]
    plan = P.FacePlan(photos, faces, size=512, upscale=upscale)
    plan.upload("cuda")
    rng = np.random.default_rng(1)
    restored = rng.integers(0, 256, (plan.n, 512, 512, 3), dtype=np.uint8)
    rdev = torch.from_numpy(restored).cuda()
    base = plan.background("cuda")
    base_host = [b.cpu().numpy() for b in plan.split(base)]
    res = {"faces": plan.n, "tiles": plan.ntiles, "output_photo": list(plan.out_shape[0])}
    res["crop_u8_f32"] = events(lambda: P.crop_faces(plan, "cuda", u8=True, f32=True))
    res["crop_u8_f32"]["bytes_written_mb"] = round(plan.n * 512 * 512 * 3 * 5 / 1e6, 2)
    out = base.clone()
    res["paste"] = events(lambda: P.paste_faces(plan, rdev, "cuda", out=out))
    res["paste"]["pixels_in_tiles_m"] = round(plan.ntiles * 1024 / 1e6, 3)
    # the host's time for the same job, and the same bytes
    t0 = time.perf_counter()
    ref_c = [R.crop(photos[k], R.invert(R.similarity(pts)), 512) for k, pts in faces]
    t1 = time.perf_counter()
    ref_p = [R.paste(base_host[k], [(restored[i], R.paste_matrix(R.similarity(pts), upscale)) for i, (kk, pts) in enumerate(faces) if kk == k], 512)
             for k in range(len(photos))]
    t2 = time.perf_counter()
    res["host_numpy_one_thread"] = {"crop_ms": round((t1 - t0) * 1000, 1), "paste_ms": round((t2 - t1) * 1000, 1)}
    u8, _ = P.crop_faces(plan, "cuda")
    fresh = P.paste_faces(plan, rdev, "cuda", out=base.clone())
    res["bytes_equal_host"] = bool(np.array_equal(u8.cpu().numpy(), np.stack(ref_c))
                                   and all(np.array_equal(g.cpu().numpy(), r) for g, r in zip(plan.split(fresh), ref_p)))
    return res


def workload_aa(face_px):
    import photo_ref as R
    w, h = (1024, 1536) if face_px <= 1024 else (2560, 3072)
    scale = 512.0 / face_px
    photos = [R.test_photo(w, h, seed=40 + k) for k in range(8)]
    marks = [[R.landmarks_for(scale, 9.0 * k - 30.0, (0.39 * w, 0.39 * h)), R.landmarks_for(scale, 20.0 - 7.0 * k, (0.6 * w, 0.53 * h))]
             for k in range(8)]
    return photos, marks


def bench_antialias(face_px):
    import photo_aa_ref as AA
    import photo_ref as R
    from vspbfr_amd import photo as P
    photos, marks = workload_aa(face_px)
    faces = [(k, pts) for k, per in enumerate(marks) for pts in per]
    plans = {"bilinear": P.FacePlan(photos, faces, size=512), "filtered": P.FacePlan(photos, faces, size=512, antialias=True)}
    aa = plans["filtered"]
    rng = np.random.default_rng(1)
    restored = rng.integers(0, 256, (aa.n, 512, 512, 3), dtype=np.uint8)
    rdev = torch.from_numpy(restored).cuda()
    res = {"face_px": face_px, "photo": [photos[0].shape[1], photos[0].shape[0]], "faces": aa.n, "tiles": aa.ntiles,
           "crop_minify": round(aa.crop_minify[0], 4), "paste_minify": round(aa.paste_minify[0], 4),
           "crop_reach": sorted({aa.crop_aa_items[i].reach for i in range(aa.n)}),
           "paste_reach": sorted({aa.paste_aa_items[i].reach for i in range(aa.n)})}
    for name, plan in plans.items():
        plan.upload("cuda")
        out = plan.background("cuda")
        res[f"crop_{name}"] = events(lambda: P.crop_faces(plan, "cuda", u8=True, f32=True))
        res[f"paste_{name}"] = events(lambda: P.paste_faces(plan, rdev, "cuda", out=out))
    for k in ("crop", "paste"):
        res[f"{k}_ratio_filtered_over_bilinear"] = round(res[f"{k}_filtered"]["median_ms"] / res[f"{k}_bilinear"]["median_ms"], 2)
    u8, _ = P.crop_faces(aa, "cuda")
    k0, pts0 = faces[0]
    ok = np.array_equal(u8[0].cpu().numpy(), AA.crop(photos[k0], R.similarity(pts0), 512))
    base = aa.background("cuda")
    fresh = P.paste_faces(aa, rdev, "cuda", out=base.clone())
    mine = [(restored[i], R.similarity(pts)) for i, (kk, pts) in enumerate(faces) if kk == 0]
    ok = ok and np.array_equal(aa.split(fresh)[0].cpu().numpy(), AA.paste(photos[0], mine, 512))
    res["bytes_equal_host_first_face_and_photo"] = bool(ok)
    return res


def bench_color_fix(photos, marks, modes, levels=5):
    import color_fix_ref as CF
    from vspbfr_amd import photo as P
    faces = [(k, pts) for k, per in enumerate(marks) for pts in per]
    plan = P.FacePlan(photos, faces, size=512)
    plan.upload("cuda")
    crops = P.crop_faces(plan, "cuda")[0]
    c = crops.cpu().numpy()
    rng = np.random.default_rng(1)
    restored = np.clip(np.rint(0.7 * c.astype(np.float64) + 40 + rng.normal(0, 8, c.shape)), 0, 255).astype(np.uint8)   # a tone shift plus noise
    rdev = torch.from_numpy(restored).cuda()
    out = plan.background("cuda")
    fixed = torch.empty_like(rdev)
    res = {"faces": plan.n, "S": 512, "levels": levels}
    res["crop_u8_f32"] = events(lambda: P.crop_faces(plan, "cuda", u8=True, f32=True))
    res["paste"] = events(lambda: P.paste_faces(plan, rdev, "cuda", out=out))
    valid = [CF.validity_from_landmarks(pts, 512, photos[k].shape[1], photos[k].shape[0]) for k, pts in faces]
    res["valid_share"] = round(float(np.mean([v.mean() for v in valid])), 4)
    u8 = plan.n * 512 * 512 * 3
    # wavelet: first level reads c and r and writes an int16 plane, the levels between read and write one, the last reads one and r and
    # writes uint8; stats: the reduction reads c and r, the apply reads r and writes uint8
    moved = {"wavelet": u8 * (2 + 2) + (levels - 2) * 4 * u8 + u8 * (2 + 1 + 1), "stats": 4 * u8}
    for mode in modes:
        r = events(lambda: P.color_fix(crops, rdev, mode, plan=plan, device="cuda", levels=levels, out=fixed))
        r["bytes_moved_mb"] = round(moved[mode] / 1e6, 1)       # each buffer once: halo re-reads are not counted
        r["effective_gb_per_s"] = round(moved[mode] / 1e6 / r["median_ms"], 1)
        r["ratio_to_crop"] = round(r["median_ms"] / res["crop_u8_f32"]["median_ms"], 2)
        r["ratio_to_paste"] = round(r["median_ms"] / res["paste"]["median_ms"], 2)
        t0 = time.perf_counter()
        ref = CF.fix_batch(c, restored, mode, valid, levels)
        r["host_numpy_ms"] = round((time.perf_counter() - t0) * 1000, 1)
        got = P.color_fix(crops, rdev, mode, plan=plan, device="cuda", levels=levels).cpu().numpy()
        r["bytes_equal_host"] = bool(np.array_equal(got, ref))
        r["bytes_moved_by_the_fix_share"] = round(float((ref != restored).mean()), 4)
        res[mode] = r
    return res


def bench_background(photos, marks, upscale):
    from PIL import Image
    from vspbfr_amd import photo as P
    faces = [(k, pts) for k, per in enumerate(marks) for pts in per]
    flat = torch.from_numpy(np.concatenate([a.reshape(-1) for a in photos])).cuda()
    plans = {"arrays": P.FacePlan(photos, faces, size=512, upscale=upscale),
             "device_photos": P.FacePlan([a.shape[:2] for a in photos], faces, size=512, upscale=upscale, device_photos=flat)}
    want = np.asarray(Image.fromarray(photos[0]).resize((photos[0].shape[1] * upscale, photos[0].shape[0] * upscale), Image.Resampling.LANCZOS))
    res = {"output_photo": list(plans["arrays"].out_shape[0]), "output_mb": round(plans["arrays"].out_bytes / 1e6, 1)}
    for name, plan in plans.items():
        plan.upload("cuda")
        r = events(lambda: plan.background("cuda"), n=30, warm=3)
        del r["percent_of_pipeline_step"]
        wall = []
        for _ in range(30):
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            plan.background("cuda")
            torch.cuda.synchronize()
            wall.append((time.perf_counter() - t0) * 1000)
        r["wall_median_ms"] = round(statistics.median(wall), 3)
        r["first_photo_equals_pillow"] = bool(np.array_equal(plan.split(plan.background("cuda"))[0].cpu().numpy(), want))
        res[name] = r
    return res


def cli_setup(tmp, photos, marks):
    """random checkpoints, the photos as PNG files under tmp/photos and a PhotoRestorer at --batch 8 --timesteps 4 --no_sample: what a CLI
    loop needs besides its args -> (restorer, root, names, landmarks, device); tools/bench_jpeg.py times its loop on the same set-up"""
    from PIL import Image
    from vspbfr_amd.diffusion import Code_diffuser
    from vspbfr_amd.e4e import E4e_embedding, Encoder4Editing, Generator
    from vspbfr_amd.photo import PhotoRestorer
    from vspbfr_amd.pipeline import RestorationPipeline, load_ddpm
    from vspbfr_amd.restorenet import Restoration_net
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
    root = os.path.join(tmp, "photos")
    os.makedirs(root)
    names = [f"{k:02d}.png" for k in range(len(photos))]
    for n, a in zip(names, photos):
        Image.fromarray(a).save(os.path.join(root, n))
    landmarks = {n: m for n, m in zip(names, marks)}
    device = torch.device("cuda", 0)
    g_ema = Restoration_net(512, 512, 8).to(device).eval()
    psp = E4e_embedding(os.path.join(ck, "psp.pt"), out_size=512, size=1024, device=device, use_generator=True)
    pipe = RestorationPipeline(g_ema, psp, load_ddpm(os.path.join(ck, "code_diffuser.pt"), device=device, timesteps=4), mixing=0.5, with_sample=False)
    return PhotoRestorer(pipe, 8), root, names, landmarks, device


def bench_cli(tmp, photos, marks):
    from vspbfr_amd import restore_photos as RP
    restorer, root, names, landmarks, device = cli_setup(tmp, photos, marks)
    times = {False: [], True: []}
    for rep in range(4):                       # the first of each is the warm run
        for save in (False, True):
            args = Namespace(photos=root, out=os.path.join(tmp, f"out_{int(save)}_{rep}"), batch=8, save_faces=save, upscale=1, size=512, inset=8,
                             feather=48)
            torch.manual_seed(123)
            random.seed(123)
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            RP.restore_photos(args, restorer, names, landmarks, device)
            torch.cuda.synchronize()
            if rep:
                times[save].append(round(time.perf_counter() - t0, 4))
    return {"what": "8 photos of 1024 x 1536, 16 faces, --batch 8 --timesteps 4 --no_sample, decode + restore + PNG, alternating",
            "loop_s": times[False], "loop_save_faces_s": times[True], "loop_median_s": statistics.median(times[False]),
            "loop_save_faces_median_s": statistics.median(times[True])}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=None)
    ap.add_argument("--skip-cli", action="store_true")
    ap.add_argument("--antialias", action="store_true", help="the anti-aliased kernels against the bilinear ones at three face sizes")
    ap.add_argument("--color_fix", choices=["stats", "wavelet", "both"], default=None, help="the colour fix beside crop and paste")
    ap.add_argument("--background", action="store_true", help="FacePlan.background() at upscale 2 and 4, with and without device_photos")
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_photo: no GPU")
    if a.background:
        photos, marks = workload()
        res = {"what": "FacePlan.background() of 8 photos of 1024 x 1536 (w x h): HIP events around the call and wall time to a device "
                       "synchronise, median of 30", "cpus_used": len(os.sched_getaffinity(0))}
        for s in (2, 4):
            res[f"upscale_{s}"] = bench_background(photos, marks, s)
        line = json.dumps(res, indent=1)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    if a.color_fix:
        photos, marks = workload()
        res = {"what": "16 faces from 8 photos of 1024 x 1536 (w x h), S = 512, upscale 1: colour fix (DESIGN 17) beside crop and paste; HIP "
                       "events, median of 30", "pipeline_step_ms": PIPELINE_STEP_MS, "cpus_used": len(os.sched_getaffinity(0))}
        res.update(bench_color_fix(photos, marks, ["wavelet", "stats"] if a.color_fix == "both" else [a.color_fix]))
        line = json.dumps(res, indent=1)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    if a.antialias:
        res = {"what": "16 faces from 8 photos, S = 512, upscale 1: filtered (DESIGN 16) against bilinear kernels; HIP events, median of 30",
               "pipeline_step_ms": PIPELINE_STEP_MS, "cpus_used": len(os.sched_getaffinity(0)),
               "sizes": [bench_antialias(px) for px in (256, 1024, 2048)]}
        line = json.dumps(res, indent=1)
        print(line)
        if a.out:
            with open(a.out, "w") as f:
                f.write(line + "\n")
        return
    photos, marks = workload()
    res = {"what": "16 faces from 8 photos of 1024 x 1536 (w x h), S = 512; HIP events, median of 30", "pipeline_step_ms": PIPELINE_STEP_MS,
           "cpus_used": len(os.sched_getaffinity(0))}
    for s in (1, 2):
        res[f"upscale_{s}"] = bench_kernels(photos, marks, s)
    if not a.skip_cli:
        with tempfile.TemporaryDirectory() as d:
            res["cli"] = bench_cli(d, photos, marks)
    line = json.dumps(res, indent=1)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
