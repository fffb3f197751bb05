"""The inference CLI with its output scored against ground truth on the device.

    python -m vspbfr_amd.restoration_metrics <the flags of vspbfr_amd.restoration_test> \\
        [--ingest host|device [--decode host|device]] [--encode host|device] --metrics [--ssim_window gauss11|uniform7] [--lpips_weights LIN[,VGG]] [--id_weights PATH]
        [--niqe_params NPZ] [--fid_weights W [--fid_stats S]] [--lmd_weights W [--lmd_box X0,Y0,SIDE]]

`vspbfr_amd/restoration_test.py` stays the line-by-line counterpart of the reference's script and is not edited: its file name
puts it under this repository's rule that a feature leaves every existing `*_test.py` / `test_*.py` file as it is.  This module
is that CLI again -- same flags, same defaults, same loop, same output names (`get_store_data` is shared, the rest restated) --
with the scoring in the loop: `PngWriter.submit` returns the uint8 device tensor whose bytes go to disk, the `restore` and `gt`
tensors of a batch go to `metrics.Evaluator.add` (quantised once, used twice; no host synchronisation per batch, so PNG encoding
still overlaps the next batch), and after `writer.drain()` the dataset's `metrics_<rank>.json` is written beside its PNGs and one
summary line printed.  `--metrics` is off by default: without it the output directory is byte for byte that of
`vspbfr_amd.restoration_test` (tests/test_metrics_cli_gpu.py compares the two).  `--metrics` with a dataset whose
`--hq_data_list` entry is `None` is refused before anything is loaded -- unless `--niqe_params NPZ` (a pristine model:
`vspbfr_amd.niqe_fit`) is given: then every report gains the no-reference `niqe` column of the restored image, and a dataset without
ground truth gets a report with that column alone.  `--fid_weights W` adds the report's `fid` entry (against the ground truth,
or against `--fid_stats S`, which also lets a dataset without ground truth be scored) and writes `fid_features_<rank>.npy` beside the
report.  `--lmd_weights W` (a 2D-FAN state dict) adds the `lmd` and `nme` columns of every dataset, which must all have
ground truth; `--lmd_box` names the square of every image the landmark network sees.  Multi-GPU as restoration_test; `metrics.merge_reports`
joins the per-rank files."""
import argparse
import os

import torch

from .e4e import E4e_embedding
from .imageio import PngWriter, RestoreTestSet, output_name
from .pipeline import RestorationPipeline, load_ddpm, shard_range
from .restoration_test import get_store_data
from .restorenet import Restoration_net


def _host_batches(args, data, lo, hi, device):
    """--ingest host: decode, LANCZOS resize and crop on the main thread (PIL), as vspbfr_amd.restoration_test does"""
    for start in range(lo, hi, args.batch):
        idx = list(range(start, min(start + args.batch, hi)))
        items = [data[i] for i in idx]
        gts = None
        if data.hq is not None:
            gts = torch.stack([it[1] for it in items])
            items = [it[0] for it in items]
        yield idx, torch.stack(items).to(device, non_blocking=True), gts


def _batches(args, data, lo, hi, device):
    """(idx, low on the device, gts or None) per batch; --debug stops after 11 batches"""
    if getattr(args, "ingest", "host") == "device":
        from .imageio import DeviceRestoreLoader
        it = DeviceRestoreLoader(data, args.batch, device, lo, hi, decode=getattr(args, "decode", None) or "host")
    else:
        it = _host_batches(args, data, lo, hi, device)
    for k, b in enumerate(it):
        if args.debug and k > 10:
            break
        yield b


def tester_restore_ddpm(args, pipe, lq_root, hq_root, eval_dict, data_name, device, rank=0, world=1):
    data = RestoreTestSet(lq_root, None if hq_root == "None" else hq_root, (args.size, args.size))
    lo, hi = shard_range(len(data), rank, world)
    os.makedirs(eval_dict, exist_ok=True)
    writer = PngWriter(encode=getattr(args, "encode", "host"))
    evaluator = None
    if args.metrics:
        from .metrics import Evaluator
        niqe_params = getattr(args, "niqe_model", None)
        # a dataset without ground truth is scored by NIQE alone (main() has refused it already when no model was given)
        fid = getattr(args, "fid", None)
        kw = {} if fid is None else {"fid": fid}
        if getattr(args, "lmd", None) is not None:
            kw.update(lmd=args.lmd, lmd_box=args.lmd_box_value)
        evaluator = Evaluator(args.ssim_window, *args.scorers, niqe=niqe_params, **kw) if data.hq is not None else Evaluator(
            args.ssim_window, niqe=niqe_params, **kw)
    print("testing!!! len:%d (rank %d handles %d..%d)" % (len(data), rank, lo, hi))
    with torch.no_grad():
        for idx, low, gts in _batches(args, data, lo, hi, device):
            out = pipe(low)
            u8 = {}
            for kind, t in (("restore", out["restored"]), ("low", low), ("sample", out["style_sample"]), ("gt", gts)):
                if t is not None:
                    u8[kind] = writer.submit(t.to(device) if kind == "gt" else t, [output_name(eval_dict, i, rank, data_name, kind) for i in idx])
            if evaluator is not None:   # the bytes that go to disk, scored on the device: no host synchronisation here
                if data.hq is not None:
                    evaluator.add(u8["restore"], u8["gt"], [(os.path.relpath(data.lq[i], lq_root), os.path.relpath(data.hq[i], hq_root)) for i in idx], idx)
                else:
                    evaluator.add(u8["restore"], None, [(os.path.relpath(data.lq[i], lq_root), None) for i in idx], idx)
    writer.drain()
    if evaluator is not None:
        from .metrics import summary_line, write_report_with_features
        report = evaluator.report(data_name)
        write_report_with_features(evaluator, report, os.path.join(eval_dict, "metrics_%d.json" % rank))      # + fid_features_<rank>.npy with FID
        print(summary_line(report))
    return eval_dict


def main(argv=None):
    ap = argparse.ArgumentParser(description="Visual Style prompt restoration test with scoring against ground truth (MI355X path)")
    ap.add_argument("--batch", type=int, default=1, help="batch sizes for each gpu")
    ap.add_argument("--size", type=int, default=512, help="image sizes for the models")
    ap.add_argument("--mixing", type=float, default=0.5, help="probability of latent code mixing")
    ap.add_argument("--channel_multiplier", type=int, default=2)
    ap.add_argument("--debug", type=bool, default=False, help="for debugging")
    ap.add_argument("--ckpt", type=str, default=None)
    ap.add_argument("--ddpm_ckpt", type=str, default="pre-train/code_diffuser.pt")
    ap.add_argument("--psp_checkpoint_path", type=str, default="pre-train/style_encoder_decoder.pt")
    ap.add_argument("--eval_dir", type=str, default="./eval_dir")
    ap.add_argument("--lq_data_list", type=str, default="")
    ap.add_argument("--hq_data_list", type=str, default="")
    ap.add_argument("--data_name_list", type=str, default="")
    ap.add_argument("--timesteps", type=int, default=4, help="extension: DDPM steps (the reference hard-codes 4, :35-38)")
    ap.add_argument("--no_sample", action="store_true", help="extension: skip the 1024^2 tail and the *_sample.png output")
    ap.add_argument("--conv_dtype", choices=["f32", "bf16", "bf16x3"], default="f32",
                    help="extension: bf16 = the bf16-kernel configuration (vsp_conv2d_bf16; not the parity path); "
                         "bf16x3 = split-precision operands on the bf16 pipe (fp32-grade)")
    ap.add_argument("--metrics", action="store_true",
                    help="extension: score *_restore.png against *_gt.png on the device (PSNR, SSIM; LPIPS / ID with the weights "
                         "below) and write metrics_<rank>.json beside the PNGs; needs a ground-truth root for every dataset")
    ap.add_argument("--ingest", choices=["host", "device"], default="host",
                    help="extension: host = PIL decode + LANCZOS resize + crop on the main thread (as restoration_test); device = decode on "
                         "a thread pool, resize and crop on the GPU (imageio.DeviceRestoreLoader), the same bytes")
    ap.add_argument("--decode", choices=["host", "device"], default=None,
                    help="extension, with --ingest device: host (the default) = PIL decodes on the thread pool; device = baseline JPEG files "
                         "are decoded on the GPU (vspbfr_amd.jpeg) and resized where the decoder wrote them, PNG files keep PIL; the same bytes")
    ap.add_argument("--encode", choices=["host", "device"], default="host",
                    help="extension: host = PIL encodes the PNGs on the writer's threads (as restoration_test); device = row filters and deflate "
                         "on the GPU (vspbfr_amd.png), the threads frame and write; other file bytes, the same pixels")
    ap.add_argument("--ssim_window", choices=["gauss11", "uniform7"], default="gauss11",
                    help="extension: SSIM window (gauss11: Wang et al.; uniform7: scikit-image's default, the reference's dssim)")
    ap.add_argument("--lpips_weights", type=str, default=None, help="extension: LIN[,VGG] weight files; adds the lpips column")
    ap.add_argument("--id_weights", type=str, default=None, help="extension: resnet101(256) state dict; adds the id column")
    ap.add_argument("--niqe_params", type=str, default=None,
                    help="extension: .npz pristine model (mu_pris_param, cov_pris_param; python -m vspbfr_amd.niqe_fit); adds the no-reference "
                         "niqe column and lets a dataset without ground truth be scored by it alone")
    ap.add_argument("--fid_weights", type=str, default=None,
                    help="extension: FID Inception state dict (pt_inception layout); adds the report's fid entry and writes "
                         "fid_features_<rank>.npy beside metrics_<rank>.json")
    ap.add_argument("--fid_stats", type=str, default=None,
                    help="extension: .npz or torch file with mu / sigma: FID against these statistics instead of the ground truth; lets a "
                         "dataset without ground truth be scored")
    from .fan import add_lmd_arguments, check_lmd_arguments
    add_lmd_arguments(ap)
    args = ap.parse_args(argv)
    args.lmd_box_value = check_lmd_arguments(ap, args, args.metrics, all(
        d["hq"] not in ("None", "") for d in get_store_data(args.lq_data_list, args.hq_data_list, args.data_name_list)))
    if not args.metrics and (args.fid_weights or args.fid_stats):
        ap.error("--fid_weights / --fid_stats only have a meaning with --metrics")
    if args.fid_stats and not args.fid_weights:
        ap.error("--fid_stats only has a meaning with --fid_weights")
    args.fid_ref = None
    if args.fid_stats:
        from .fid import load_stats
        try:
            args.fid_ref = load_stats(args.fid_stats)
        except (ValueError, OSError) as e:
            ap.error(str(e))
    if args.decode is not None and args.ingest != "device":
        ap.error("--decode only has a meaning with --ingest device")
    if not args.metrics and (args.lpips_weights or args.id_weights):
        ap.error("--lpips_weights / --id_weights only have a meaning with --metrics")
    if not args.metrics and args.niqe_params:
        ap.error("--niqe_params only has a meaning with --metrics")
    args.niqe_model = None
    if args.niqe_params:
        from .niqe import load_params
        try:
            args.niqe_model = load_params(args.niqe_params)
        except (ValueError, OSError) as e:
            ap.error(str(e))
    if args.metrics:
        missing = [d["name"] for d in get_store_data(args.lq_data_list, args.hq_data_list, args.data_name_list) if d["hq"] in ("None", "")]
        if missing and args.fid_weights and args.fid_ref is None:
            ap.error("--fid_weights without --fid_stats measures against ground truth; none given for: " + ", ".join(missing))
        if missing and args.niqe_model is None and args.fid_ref is None:
            ap.error("--metrics needs a ground-truth root (--hq_data_list) for every dataset; none given for: " + ", ".join(missing))
    args.latent, args.n_mlp = 512, 8
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
        except RuntimeError as e:  # the reference prints and carries on with the initial weights (:246-250)
            print(str(e))
    g_ema = g_ema.to(device).eval()
    name_ = os.path.basename(str(args.ckpt)).strip().split(".")[0]
    eval_root = os.path.join(args.eval_dir, name_)
    psp = E4e_embedding(args.psp_checkpoint_path, out_size=args.size, size=1024, device=device, use_generator=True)
    store = get_store_data(args.lq_data_list, args.hq_data_list, args.data_name_list)
    if args.metrics:
        from .metrics import load_scorers
        args.scorers = load_scorers(args.lpips_weights, args.id_weights, device)
        if args.fid_weights:
            from . import fid as fid_mod
            args.fid = (fid_mod.FidInception(fid_mod.load(args.fid_weights), device), args.fid_ref, args.fid_stats)
        if args.lmd_weights:
            from .fan import FanLandmarks
            args.lmd = FanLandmarks(args.lmd_weights, device)
    for k, d in enumerate(store):
        diffusion = load_ddpm(args.ddpm_ckpt, device=device, timesteps=args.timesteps)
        pipe = RestorationPipeline(g_ema, psp, diffusion, mixing=args.mixing, with_sample=not args.no_sample)
        eval_dict = os.path.join(eval_root, str(len(store) - 1), d["name"])  # the reference's `str(i)` is the last index (:174)
        tester_restore_ddpm(args, pipe, d["lq"], d["hq"], eval_dict, d["name"], device, rank, world)


if __name__ == "__main__":
    main()
