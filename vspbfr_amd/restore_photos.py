"""Restore the faces inside whole photos and give the photos back.

    python -m vspbfr_amd.restore_photos --photos DIR (--landmarks FILE.json | --detect_weights W) --out DIR [--upscale {1,2,4}]
        [--save_faces] [--inset PX] [--feather PX] [--antialias] [--color_fix {none,stats,wavelet}] [--color_levels L]
        [--detect_threshold 0.8] [--detect_nms 0.4] [--detect_side 1024] [--detect_max_faces N] [--detect_min_face PX]
        [--format {png,jpg}] [--quality Q] [--subsampling {420,444}] [--encode {host,device}] [--decode {host,device}]
        [--png_encode {host,device}] [--bg_weights W [--bg_band_rows N]] [--parse_weights W [--parse_sigma F] [--parse_border PX]] <the model flags of vspbfr_amd.restoration_test: --ckpt --ddpm_ckpt --psp_checkpoint_path --size
        --mixing --channel_multiplier --timesteps --no_sample --conv_dtype --batch>

`vspbfr_amd.restoration_test` takes aligned 512 x 512 faces; this CLI takes photos of any size with any number of faces.  Exactly one of
--landmarks and --detect_weights says where the faces are.  FILE.json maps a photo's path relative to DIR to its faces, each five
(x, y) landmarks in photo pixels (pixel centres) --
left eye, right eye, nose, left and right mouth corner:

    {"relative/name.png": [[[x, y], [x, y], [x, y], [x, y], [x, y]], ...one entry per face], ...}

Per face: the least-squares similarity onto the FFHQ template, an aligned crop on the device, the restoration pipeline (faces of
several photos share a batch), quantisation to 8 bits as the other CLIs' PNG writer does, and a feathered paste-back in list order
(vspbfr_amd.photo, csrc/face_warp.hip).  With --upscale 2 or 4 the photo is first resized by Pillow's LANCZOS filter and the
faces are pasted at that scale.  Output: OUT/<relative stem>.png for every photo -- one without an entry or with no face is written
through (resized if asked) -- with --save_faces also <stem>_<k>_crop.png and <stem>_<k>_restore.png per face, and report.json
(report_<rank>.json in a multi-GPU run) listing every photo with its face count.

--antialias: a face larger than the crop is shrunk, and a restored crop larger than its face in the output photo is pasted, through a
tent filter one destination pixel wide instead of four bilinear taps; report.json then lists per face `crop_minify` and
`paste_minify`.  A minification above 16 is refused while the landmarks are validated.

--color_fix stats | wavelet: before the paste the restored crop takes its colours back from the crop (vspbfr_amd.photo.color_fix,
csrc/color_fix.hip) -- `stats` moves its per-channel mean and deviation onto the crop's, `wavelet` keeps its high frequencies
and takes the low ones (--color_levels dilated blurs, default 5, 1..6) from the crop; crop pixels outside the photo take no part.  The
fixed crop is what is pasted; with --save_faces it is written as <stem>_<k>_fixed.png beside _crop.png and _restore.png, which stay the
crop and the network's output.  report.json then lists `color_fix` and `color_levels`.  Default none: nothing changes.

--format jpg: the output photo is OUT/<relative stem>.jpg, a baseline JPEG of --quality (1..100, default 90) and --subsampling (420,
the default, or 444) with a restart interval of vspbfr_amd.jpeg.DEFAULT_RESTART MCUs.  --encode device (the default of this route)
codes it on the device (vspbfr_amd.jpeg, csrc/jpeg.hip), --encode host hands the pixels to Pillow with the same parameters;
both write the bytes Pillow writes for the pixels of the png route.  The --save_faces files stay PNG.  report.json then names the .jpg
files and lists `format`, `quality` and `subsampling`.  Default png: nothing changes.

--decode device: the group's files are read as bytes and baseline JPEGs are decoded on the device (vspbfr_amd.jpeg.decode_files,
csrc/jpeg_decode.hip) into the buffer the crop kernel reads; a PNG, a progressive or otherwise refused JPEG and a file whose
scan the kernels flag take Pillow's decode inside the same group.  Equal output bytes either way.  With the flag (host or device)
report.json lists `decode` per photo.  Default: Pillow, nothing changes.

--png_encode device: the PNG files are coded on the device.  A group's output photos go through one call of the ragged encoder on the
packed buffer they lie in (imageio.PngWriter.submit_photos, vsp_png_encode_ragged_u8, DESIGN 21: any width, every photo its own size),
the --save_faces files through the uniform encoder (vsp_png_encode_u8).  The files hold the pixels of the host route; their bytes differ
from Pillow's, as any two PNG encoders' do.  report.json then lists `png_encode`.  With --format jpg the flag needs --save_faces (no
other file is a PNG).  Default host: Pillow, nothing changes.

--detect_weights W: the faces are found on the device by RetinaFace from the checkpoint W: the MobileNet-0.25 network (vspbfr_amd.detect,
csrc/detect.hip) or, for a file that holds `body.layer1.0.conv1.weight`, the ResNet-50 network (vspbfr_amd.detect_r50,
csrc/detect_r50.hip; report.json's `detect` then lists `backbone`) -- no weights are shipped, and the key layouts the loaders
expect are unverified against a real file.  Every group of
photos goes through one detect() call (with --decode device on the decoder's buffer); a detected face that the validation of --landmarks
would refuse (degenerate landmarks, with --antialias a minification above 16) is dropped and listed with its reason.  report.json then
lists `detect` (the parameters) and per photo `score`, `box` and, if any, `dropped`; OUT/landmarks.json (landmarks_<rank>.json in a
multi-GPU run) holds the faces that were used, in the format --landmarks reads.  Without the flag nothing changes.

--bg_weights W: with --upscale 2 or 4 the photo under the faces is upscaled by Real-ESRGAN's compact network (vspbfr_amd.upscale,
csrc/sr.hip) from the checkpoint W instead of the LANCZOS resize -- no weights are shipped, and the key layout the loader
expects is unverified against a real file.  A x4 network at --upscale 2 goes through the device LANCZOS resize down from its x4 output;
a x2 network at --upscale 4 is refused.  --bg_band_rows N processes every photo in bands of N rows (the same bytes).  report.json then
lists `background` = {model, num_conv, scale, banded, nonfinite}; `nonfinite` names the photos in which a value was not finite before the
clamp (written as 0): a warning, not an abort.  Without the flag nothing changes.  A checkpoint with RRDBNet's keys (`conv_first.weight`:
RealESRGAN_x4plus, RealESRGAN_x2plus, the 6-block anime model) runs that network instead (vspbfr_amd.rrdb, csrc/rrdb.hip) under
the same rules; `background` is then {model: "RRDBNet", num_block, scale, banded, nonfinite}.

--parse_weights W: the paste goes through a face-parsing mask (vspbfr_amd.parse, csrc/parse.hip): facexlib's ParseNet from the
checkpoint W runs on the network's restored crop, the face classes are kept (everything but background, neck, clothes, hair and hat), the
binary map is blurred twice (--parse_sigma F, default 11 size / 512) and its outermost --parse_border PX rows and columns (default
round(10 size / 512)) are set to 0; the blend weight is the feather ramp times that mask.  No weights are shipped, and the key layout the
loader expects is unverified against a real file.  With --save_faces also <stem>_<k>_mask.png (grey, (weight 255 + 128) >> 8) and
<stem>_<k>_parse.png (class indices).  report.json then lists `parse` = {model, sigma, radius, border, nonfinite} and per photo
`mask_mean`, one value per face; `nonfinite` names the photos with a face that had a non-finite logit (those pixels keep the photo): a
warning, not an abort.  Without the flag nothing changes.

Multi-GPU as the other CLIs: `python -m torch.distributed.run --nproc-per-node N -m vspbfr_amd.restore_photos ...`; every rank takes a
contiguous shard of the sorted photo list, no collective."""
import argparse
import json
import os

import numpy as np
import torch

from .detect import add_detect_arguments, check_detect_arguments, load_detector
from .e4e import E4e_embedding
from .imageio import JpegWriter, PngWriter, list_images
from .photo import DEFAULT_FEATHER, DEFAULT_INSET, PhotoRestorer, check_color_fix, check_minify, similarity_from_landmarks
from .pipeline import RestorationPipeline, load_ddpm, shard_range
from .restorenet import Restoration_net

MAX_PHOTOS_PER_CALL = 8      # photos decoded and kept on the device together while their faces fill a batch


def load_landmarks(path, names, size=512, upscale=1, antialias=False):
    """FILE.json -> {relative name: [(5, 2) float64, ...]}; every face is validated here (ValueError names the photo and the face), an
    entry for a photo that is not in the list is an error too.  antialias: a minification above photo.MAX_MINIFY at crop side `size`
    and `upscale` is refused here as well."""
    with open(path) as f:
        raw = json.load(f)
    if not isinstance(raw, dict):
        raise ValueError(f"{path}: expected an object that maps photo names to lists of faces")
    unknown = sorted(set(raw) - set(names))
    if unknown:
        raise ValueError(f"{path}: no such photo under --photos: {', '.join(unknown[:5])}")
    out = {}
    for name, faces in raw.items():
        if not isinstance(faces, list):
            raise ValueError(f"photo {name!r}: expected a list of faces")
        for k, pts in enumerate(faces):
            A = similarity_from_landmarks(pts, size=size, photo=name, face=k)
            if antialias:
                check_minify(A, upscale, name, k)
        out[name] = [np.asarray(p, dtype=np.float64) for p in faces]
    return out


def _decode(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"), dtype=np.uint8)


def _groups(names, landmarks, batch):
    """consecutive photos whose faces fill at least one batch, at most MAX_PHOTOS_PER_CALL of them"""
    group, nfaces = [], 0
    for n in names:
        group.append(n)
        nfaces += len(landmarks.get(n, ()))
        if nfaces >= batch or len(group) == MAX_PHOTOS_PER_CALL:
            yield group
            group, nfaces = [], 0
    if group:
        yield group


def list_photos(root):
    """the photos under `root` as sorted paths relative to it"""
    return [os.path.relpath(p, root) for p in list_images(root)]


def detect_report(detector, detect_params):
    """report.json's `detect` entry: the parameters, and `backbone` for a detector that names one (the ResNet-50 route alone)"""
    backbone = getattr(detector, "backbone", None)
    return dict(detect_params, backbone=backbone) if backbone else detect_params


def detect_group(detector, params, group, landmarks, found, photos=None, device_photos=None, size=512, upscale=1, antialias=False):
    """One detect() call over a group of photos: the faces that pass the validation of load_landmarks go to landmarks[name] (as the
    float64 values a landmarks file gives back), every face's score and box and the dropped ones with their reason to found[name]."""
    from .detect import as_json_floats
    res = detector.detect(photos=photos, device_photos=device_photos, **params)
    for n, d in zip(group, res):
        used, info = [], {"score": [], "box": [], "dropped": [], "status": d["status"]}
        for j in range(len(d["landmarks"])):
            pts = as_json_floats(d["landmarks"][j])
            score, box = float(d["score"][j]), [float(v) for v in d["box"][j]]
            try:
                A = similarity_from_landmarks(pts, size=size, photo=n, face=j)
                if antialias:
                    check_minify(A, upscale, n, j)
            except ValueError as e:
                info["dropped"].append({"face": j, "reason": str(e), "score": score, "box": box})
                continue
            used.append(pts)
            info["score"].append(score)
            info["box"].append(box)
        landmarks[n], found[n] = used, info


def restore_photos(args, restorer, names, landmarks, device, rank=0, world=1, detector=None, detect_params=None):
    lo, hi = shard_range(len(names), rank, world)
    os.makedirs(args.out, exist_ok=True)
    png_device = getattr(args, "png_encode", None) == "device"
    writer = PngWriter(encode="device") if png_device else PngWriter()
    jpg = getattr(args, "format", "png") == "jpg"
    photo_writer = JpegWriter(quality=args.quality, subsampling=args.subsampling, encode=args.encode) if jpg else writer
    ext = ".jpg" if jpg else ".png"
    ragged = png_device and not jpg          # a group's photos go through one call of the ragged PNG encoder
    report, found = [], {}
    bg_banded, bg_nonfinite = False, []
    parser, parse_nonfinite = getattr(restorer, "parser", None), []
    if detector is not None:
        landmarks = {}
    print("restoring photos: %d (rank %d handles %d..%d)" % (len(names), rank, lo, hi))
    for group in _groups(names[lo:hi], landmarks, args.batch):
        decode = getattr(args, "decode", None)
        if decode == "device":
            from .jpeg import decode_files
            packed, sizes, offsets, how = decode_files([os.path.join(args.photos, n) for n in group], device)
            if detector is not None:
                detect_group(detector, detect_params, group, landmarks, found, device_photos=(packed, offsets, sizes), size=args.size,
                             upscale=args.upscale, antialias=getattr(args, "antialias", False))
            outs, crops, restored, plan, *fixed = restorer(sizes, [landmarks.get(n) for n in group], device, names=group, device_photos=packed)
        else:
            photos, how = [_decode(os.path.join(args.photos, n)) for n in group], ["host"] * len(group)
            if detector is not None:
                detect_group(detector, detect_params, group, landmarks, found, photos=photos, size=args.size, upscale=args.upscale,
                             antialias=getattr(args, "antialias", False))
            outs, crops, restored, plan, *fixed = restorer(photos, [landmarks.get(n) for n in group], device, names=group)
        if restorer.background is not None:
            info = plan.background_info
            bg_banded = bg_banded or any(info["banded"])
            bg_nonfinite += [n for n, f in zip(group, info["flags"].cpu().tolist()) if f]
        pinfo = restorer.parse_info if parser is not None else None
        if pinfo is not None:
            from .parse import mask_png
            mask_mean = (pinfo["mask"].view(torch.int16).to(torch.float32).mean(dim=(1, 2)) / 256).cpu().tolist()
            parse_flags = pinfo["flags"].cpu().tolist()
            if args.save_faces:
                from PIL import Image
                mask_grey, parse_cls = mask_png(pinfo["mask"]).cpu().numpy(), pinfo["classes"].cpu().numpy()
        stems = [os.path.join(args.out, os.path.splitext(n)[0]) for n in group]
        for stem in stems:
            os.makedirs(os.path.dirname(stem) or ".", exist_ok=True)
        if ragged:
            writer.submit_photos(plan.out_packed, plan.out_shape, plan.out_off, [stem + ext for stem in stems])
        for k, n in enumerate(group):
            stem = stems[k]
            if not ragged:
                photo_writer.submit(outs[k][None], [stem + ext])
            mine = [i for i, kk in enumerate(plan.face_photo) if kk == k]
            if args.save_faces:
                for j, i in enumerate(mine):
                    writer.submit(crops[i:i + 1], [f"{stem}_{j}_crop.png"])
                    writer.submit(restored[i:i + 1], [f"{stem}_{j}_restore.png"])
                    if fixed:
                        writer.submit(fixed[0][i:i + 1], [f"{stem}_{j}_fixed.png"])
                    if pinfo is not None:       # two small single-channel files per face: the RGB writers do not take them
                        Image.fromarray(mask_grey[i]).save(f"{stem}_{j}_mask.png")
                        Image.fromarray(parse_cls[i]).save(f"{stem}_{j}_parse.png")
            report.append({"photo": n, "faces": len(mine), "output": os.path.relpath(stem + ext, args.out),
                           "size": [int(outs[k].shape[1]), int(outs[k].shape[0])]})
            if decode is not None:
                report[-1]["decode"] = how[k]
            if detector is not None:
                report[-1].update(score=found[n]["score"], box=found[n]["box"])
                if found[n]["dropped"]:
                    report[-1]["dropped"] = found[n]["dropped"]
                if found[n]["status"]:
                    report[-1]["detect_status"] = found[n]["status"]
            if pinfo is not None:
                report[-1]["mask_mean"] = [round(mask_mean[i], 6) for i in mine]
                if any(parse_flags[i] for i in mine):
                    parse_nonfinite.append(n)
            if plan.antialias:
                report[-1]["crop_minify"] = [round(plan.crop_minify[i], 6) for i in mine]
                report[-1]["paste_minify"] = [round(plan.paste_minify[i], 6) for i in mine]
    writer.drain()
    photo_writer.drain()
    name = "report.json" if world == 1 else "report_%d.json" % rank
    head = {"upscale": args.upscale, "crop_size": args.size, "inset": args.inset, "feather": args.feather}
    if restorer.color_fix is not None:
        head.update(color_fix=restorer.color_fix, color_levels=restorer.color_levels)
    if jpg:
        head.update(format="jpg", quality=args.quality, subsampling=args.subsampling)
    if getattr(args, "png_encode", None) is not None:
        head.update(png_encode=args.png_encode)
    if restorer.background is not None:
        head.update(background=restorer.background.describe(bg_banded, bg_nonfinite))
        if bg_nonfinite:
            print("warning: non-finite background values were written as 0 in: " + ", ".join(bg_nonfinite))
    if parser is not None:
        head.update(parse=parser.describe(args.size, sigma=getattr(args, "parse_sigma", None), border=restorer.parse_border,
                                          nonfinite=parse_nonfinite))
        if parse_nonfinite:
            print("warning: non-finite parsing logits (those pixels are class 0 and keep the photo) in: " + ", ".join(parse_nonfinite))
    if detector is not None:
        from .detect import write_landmarks
        head.update(detect=detect_report(detector, detect_params))
        write_landmarks(os.path.join(args.out, "landmarks.json" if world == 1 else "landmarks_%d.json" % rank),
                        {n: landmarks[n] for n in names[lo:hi] if landmarks.get(n)})
    with open(os.path.join(args.out, name), "w") as f:
        json.dump(dict(head, photos=report), f, indent=1)
    return report


def main(argv=None):
    ap = argparse.ArgumentParser(description="Restore the faces inside whole photos (MI355X path)")
    ap.add_argument("--batch", type=int, default=1, help="faces per pipeline batch; faces of several photos share a batch")
    ap.add_argument("--size", type=int, default=512, help="image sizes for the models: the side of the aligned crop")
    ap.add_argument("--mixing", type=float, default=0.5, help="probability of latent code mixing")
    ap.add_argument("--channel_multiplier", type=int, default=2)
    ap.add_argument("--ckpt", type=str, default=None)
    ap.add_argument("--ddpm_ckpt", type=str, default="pre-train/code_diffuser.pt")
    ap.add_argument("--psp_checkpoint_path", type=str, default="pre-train/style_encoder_decoder.pt")
    ap.add_argument("--timesteps", type=int, default=4, help="DDPM steps")
    ap.add_argument("--no_sample", action="store_true", help="skip the 1024^2 style-sample tail of the pipeline (it is not written here)")
    ap.add_argument("--conv_dtype", choices=["f32", "bf16", "bf16x3"], default="f32",
                    help="bf16 = the bf16-kernel configuration (vsp_conv2d_bf16; not the parity path); "
                         "bf16x3 = split-precision operands on the bf16 pipe (fp32-grade)")
    ap.add_argument("--photos", type=str, required=True, help="directory of photos (searched recursively)")
    ap.add_argument("--landmarks", type=str, default=None, help='JSON: {"relative/name.png": [[[x, y] x 5], ...one entry per face]}')
    ap.add_argument("--detect_weights", type=str, default=None,
                    help="RetinaFace checkpoint, mobilenet0.25 or resnet50 (not shipped): find the faces on the device instead of reading --landmarks")
    add_detect_arguments(ap, "detect_")
    ap.add_argument("--out", type=str, required=True, help="output directory")
    ap.add_argument("--upscale", type=int, choices=[1, 2, 4], default=1, help="resize the photo (Pillow LANCZOS) and paste the faces at that scale")
    ap.add_argument("--save_faces", action="store_true", help="also write <stem>_<k>_crop.png and <stem>_<k>_restore.png")
    ap.add_argument("--inset", type=int, default=DEFAULT_INSET, help="px of the crop border that keep the photo")
    ap.add_argument("--feather", type=int, default=DEFAULT_FEATHER, help="px over which the blend rises to the restored face")
    ap.add_argument("--antialias", action="store_true", help="shrink large faces into the crop, and restored crops into small faces, through a "
                                                             "tent filter one destination pixel wide instead of four bilinear taps")
    ap.add_argument("--color_fix", choices=["none", "stats", "wavelet"], default="none",
                    help="before the paste the restored crop takes its colours back from the crop: per-channel mean and deviation (stats) "
                         "or everything below the finest --color_levels wavelet levels (wavelet)")
    ap.add_argument("--color_levels", type=int, default=5, help="levels of --color_fix wavelet, 1..6")
    ap.add_argument("--format", choices=["png", "jpg"], default="png", help="file format of the output photos (the --save_faces files stay PNG)")
    ap.add_argument("--quality", type=int, default=None, help="--format jpg: JPEG quality 1..100 (default 90)")
    ap.add_argument("--subsampling", choices=["420", "444"], default=None, help="--format jpg: chroma subsampling (default 420)")
    ap.add_argument("--encode", choices=["host", "device"], default=None,
                    help="--format jpg: code the file on the device (default) or with Pillow on the host; equal bytes")
    ap.add_argument("--decode", choices=["host", "device"], default=None,
                    help="decode baseline JPEG inputs on the device or everything with Pillow on the host (the default); equal bytes")
    ap.add_argument("--png_encode", choices=["host", "device"], default=None,
                    help="code the PNG files with Pillow on the host (the default) or on the device; equal pixels")
    ap.add_argument("--bg_weights", type=str, default=None,
                    help="SRVGGNetCompact or RRDBNet (x4plus / x2plus) checkpoint (not shipped): upscale the photo under the faces with it instead of LANCZOS; needs --upscale 2 or 4")
    ap.add_argument("--bg_band_rows", type=int, default=None, help="--bg_weights: process every photo in bands of this many rows (the same bytes)")
    ap.add_argument("--parse_weights", type=str, default=None,
                    help="ParseNet checkpoint (not shipped): paste through the face-parsing mask of the restored crop instead of the whole square")
    ap.add_argument("--parse_sigma", type=float, default=None, help="--parse_weights: sigma of the mask's two Gaussian blurs (default 11 size / 512; the blur's radius is round(50 size / 512) "
                         "but at most 64, so above --size 655 the taps are cut below 3 sigma)")
    ap.add_argument("--parse_border", type=int, default=None, help="--parse_weights: px at each side of the mask set to 0 (default round(10 size / 512))")
    args = ap.parse_args(argv)
    parse_state = None
    if args.parse_weights is not None:
        from .parse import check_parse_arguments
        parse_state, parse_taps, parse_border = check_parse_arguments(ap, args.parse_weights, args.size, args.parse_sigma, args.parse_border)
    elif args.parse_sigma is not None or args.parse_border is not None:
        ap.error("--parse_sigma and --parse_border belong to --parse_weights")
    bg_state = None
    if args.bg_weights is not None:
        from .upscale import check_background_arguments
        bg_state = check_background_arguments(ap, args.bg_weights, args.upscale, args.bg_band_rows)
    elif args.bg_band_rows is not None:
        ap.error("--bg_band_rows belongs to --bg_weights")
    if (args.landmarks is None) == (args.detect_weights is None):
        ap.error("exactly one of --landmarks and --detect_weights must be given")
    detect_params = None
    try:                       # the flags are checked before any model is loaded
        if args.detect_weights is not None:
            detect_params = check_detect_arguments(args.detect_threshold, args.detect_nms, args.detect_side, args.detect_max_faces,
                                                   args.detect_min_face)
            if not os.path.isfile(args.detect_weights):
                raise ValueError(f"--detect_weights: no such file: {args.detect_weights}")
        color_fix, color_levels = check_color_fix(args.color_fix, args.color_levels)
        if args.format != "jpg" and (args.quality is not None or args.subsampling is not None or args.encode is not None):
            raise ValueError("--quality, --subsampling and --encode belong to --format jpg")
        if args.format == "jpg":
            from .jpeg import DEFAULT_QUALITY, DEFAULT_RESTART, check_params
            args.quality, args.subsampling, _ = check_params(DEFAULT_QUALITY if args.quality is None else args.quality,
                                                              args.subsampling or "420", DEFAULT_RESTART)
            args.encode = args.encode or "device"
        if args.png_encode == "device" and args.format == "jpg" and not args.save_faces:
            raise ValueError("--png_encode device with --format jpg needs --save_faces: no other file is a PNG")
    except ValueError as e:
        ap.error(str(e))
    if args.batch < 1 or args.inset < 0 or args.feather < 0:
        ap.error("--batch must be at least 1, --inset and --feather at least 0")
    args.latent, args.n_mlp = 512, 8
    try:                       # the inputs are checked before any model is loaded
        names = list_photos(args.photos)
        landmarks = {} if args.landmarks is None else load_landmarks(args.landmarks, names, args.size, args.upscale, args.antialias)
    except (ValueError, OSError) as e:
        ap.error(str(e))
    from . import hip_ops
    hip_ops.BF16_CONV = {"f32": False, "bf16": True, "bf16x3": "x3"}[args.conv_dtype]

    world, rank = int(os.environ.get("WORLD_SIZE", "1")), int(os.environ.get("RANK", "0"))
    local = int(os.environ.get("LOCAL_RANK", "0"))
    torch.cuda.set_device(local)
    device = torch.device("cuda", local)

    g_ema = Restoration_net(args.size, args.latent, args.n_mlp, channel_multiplier=args.channel_multiplier)
    if args.ckpt is not None:
        print("load models:", args.ckpt)
        try:
            g_ema.load_state_dict(torch.load(args.ckpt, map_location="cpu")["g_ema"])
        except RuntimeError as e:  # as the other CLIs: print and carry on with the initial weights
            print(str(e))
    g_ema = g_ema.to(device).eval()
    psp = E4e_embedding(args.psp_checkpoint_path, out_size=args.size, size=1024, device=device, use_generator=True)
    diffusion = load_ddpm(args.ddpm_ckpt, device=device, timesteps=args.timesteps)
    pipe = RestorationPipeline(g_ema, psp, diffusion, mixing=args.mixing, with_sample=not args.no_sample)
    restorer = PhotoRestorer(pipe, args.batch, upscale=args.upscale, size=args.size, inset=args.inset, feather=args.feather,
                             antialias=args.antialias, color_fix=color_fix, color_levels=color_levels)
    if bg_state is not None:
        from .upscale import make_upscaler
        restorer.background = make_upscaler(bg_state, device, band_rows=args.bg_band_rows)
    if parse_state is not None:
        from .parse import FaceParser
        restorer.parser, restorer.parse_taps, restorer.parse_border = FaceParser(parse_state, device), parse_taps, parse_border
    detector = None
    if args.detect_weights is not None:
        try:
            detector = load_detector(args.detect_weights, device)
        except ValueError as e:
            ap.error(str(e))
    restore_photos(args, restorer, names, landmarks, device, rank, world, detector, detect_params)


if __name__ == "__main__":
    main()
