"""Score two existing folders of PNGs with the device metrics of vspbfr_amd.metrics (same kernel, same report as
`python -m vspbfr_amd.restoration_metrics`): what someone comparing against another method's outputs needs.

    python -m vspbfr_amd.score --restored eval_dir/.../demo --gt eval_dir/.../demo [--pattern _restore.png/_gt.png]
        [--ssim_window gauss11|uniform7] [--lpips_weights LIN[,VGG]] [--id_weights PATH] [--niqe_params NPZ]
        [--fid_weights W [--fid_stats S]] [--lmd_weights W [--lmd_box X0,Y0,SIDE]] [--batch 8] [--out metrics.json]

`--niqe_params` (a pristine model, `vspbfr_amd.niqe_fit` or a published one) adds the no-reference `niqe` column and makes --gt
optional: without --gt every file of --restored that carries the restored suffix (all files when none does) is scored alone.

`--fid_weights` (an FID Inception state dict, `vspbfr_amd.fid`) adds the report's top-level `fid` entry: against the ground truth's
features, or against `--fid_stats` (mu / sigma of a reference set), which makes --gt optional too.  With --out the features go to
`<out stem>_fid_features.npy` (and `..._gt.npy`) beside the report, so that `metrics.merge_reports` can recompute the distance.

`--lmd_weights` (a 2D-FAN state dict, `vspbfr_amd.fan`) adds the `lmd` and `nme` columns: the mean distance between the 68 landmarks
found on the restored image and on its ground truth, in image pixels and over the ground truth's outer-eye-corner distance; `--lmd_box`
names the square of every image the landmark network sees (default: the whole image).  It needs --gt.

Pairing: a file `<stem><restored suffix>` of --restored goes with `<stem><gt suffix>` of --gt (the CLI's own naming,
`{index}_{rank}_{name}_restore.png` / `..._gt.png`); when no file of --restored carries the suffix, the two folders are
paired by sorted order and must hold the same number of images."""
import argparse
import json
import os

from .imageio import list_images


def pair_files(restored_dir, gt_dir, pattern="_restore.png/_gt.png"):
    """[(restored path, gt path)] -- pure host code."""
    if pattern.count("/") != 1 or not all(pattern.split("/")):
        raise ValueError(f"--pattern takes RESTORED_SUFFIX/GT_SUFFIX (got {pattern!r})")
    rs, gs = pattern.split("/")
    restored = [p for p in list_images(restored_dir) if p.endswith(rs)]
    if restored:
        pairs = []
        for p in restored:
            q = os.path.join(gt_dir, os.path.relpath(p, restored_dir)[:-len(rs)] + gs)
            if not os.path.exists(q):
                raise FileNotFoundError(f"no ground truth {q} for {p}")
            pairs.append((p, q))
        return pairs
    a, b = list_images(restored_dir), list_images(gt_dir)
    if os.path.abspath(restored_dir) == os.path.abspath(gt_dir):
        raise ValueError(f"no file in {restored_dir} ends with {rs!r} and --restored and --gt are the same folder")
    if len(a) != len(b) or not a:
        raise ValueError(f"cannot pair by sorted order: {len(a)} images in {restored_dir}, {len(b)} in {gt_dir}")
    return list(zip(a, b))


def _load_u8(path):
    from .imageio import load_rgb_u8
    return load_rgb_u8(path)


def restored_files(restored_dir, pattern="_restore.png/_gt.png"):
    """[(restored path, None)] for a run without ground truth -- pure host code"""
    if pattern.count("/") != 1 or not all(pattern.split("/")):
        raise ValueError(f"--pattern takes RESTORED_SUFFIX/GT_SUFFIX (got {pattern!r})")
    files = list_images(restored_dir)
    tagged = [p for p in files if p.endswith(pattern.split("/")[0])]
    if not (tagged or files):
        raise ValueError(f"no images in {restored_dir}")
    return [(p, None) for p in (tagged or files)]


def score_pairs(pairs, window="gauss11", lpips=None, idloss=None, batch=8, dataset=None, device="cuda", niqe=None, fid=None, evaluator=None,
                lmd=None, lmd_box=None):
    """The report of a list of (restored, gt) files; images of one size are batched, an odd one goes alone.  gt = None in every
    pair (with `niqe` params or `fid` statistics): the no-reference report.  `fid`: metrics.Evaluator's argument; `evaluator`: a list
    that receives the Evaluator (its FID features go to disk beside the report); `lmd` / `lmd_box`: metrics.Evaluator's arguments."""
    import torch

    from .metrics import Evaluator
    kw = {} if lmd is None else {"lmd": lmd, "lmd_box": lmd_box}
    ev = Evaluator(window, lpips, idloss, niqe, **kw) if fid is None else Evaluator(window, lpips, idloss, niqe, fid=fid, **kw)
    if evaluator is not None:
        evaluator.append(ev)
    pend, shape = [], None

    def flush():
        if pend:
            r = torch.stack([p[1] for p in pend]).to(device, non_blocking=True)
            g = None if pend[0][2] is None else torch.stack([p[2] for p in pend]).to(device, non_blocking=True)
            ev.add(r, g, [p[3] for p in pend], [p[0] for p in pend])
            pend.clear()

    for i, (rp, gp) in enumerate(pairs):
        r, g = _load_u8(rp), None if gp is None else _load_u8(gp)
        if g is not None and r.shape != g.shape:
            raise ValueError(f"{rp} is {tuple(r.shape[:2])}, {gp} is {tuple(g.shape[:2])}: a pair must have one size")
        if shape != r.shape or len(pend) >= batch:
            flush()
            shape = r.shape
        pend.append((i, r, g, (os.path.basename(rp), None if gp is None else os.path.basename(gp))))
    flush()
    return ev.report(dataset)


def main(argv=None):
    ap = argparse.ArgumentParser(description="PSNR / SSIM / LPIPS / ID of a folder of restored PNGs against ground truth (MI355X)")
    ap.add_argument("--restored", required=True)
    ap.add_argument("--gt", default=None, help="ground-truth folder; optional with --niqe_params or --fid_stats")
    ap.add_argument("--pattern", default="_restore.png/_gt.png", help="RESTORED_SUFFIX/GT_SUFFIX")
    ap.add_argument("--ssim_window", choices=["gauss11", "uniform7"], default="gauss11")
    ap.add_argument("--lpips_weights", default=None, help="LIN[,VGG] weight files; adds the lpips column")
    ap.add_argument("--id_weights", default=None, help="resnet101(256) state dict; adds the id column")
    ap.add_argument("--niqe_params", default=None, help=".npz with mu_pris_param / cov_pris_param; adds the niqe column")
    ap.add_argument("--fid_weights", default=None, help="FID Inception state dict (pt_inception layout); adds the report's fid entry")
    ap.add_argument("--fid_stats", default=None, help=".npz or torch file with mu / sigma: FID against these statistics instead of --gt")
    from .fan import add_lmd_arguments, check_lmd_arguments
    add_lmd_arguments(ap)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--dataset", default=None, help="name written into the report")
    ap.add_argument("--out", default=None, help="write the JSON report here (default: print it)")
    args = ap.parse_args(argv)
    if args.batch < 1:
        ap.error("--batch must be at least 1")
    if args.fid_stats and not args.fid_weights:
        ap.error("--fid_stats only has a meaning with --fid_weights")
    if args.gt is None and args.fid_weights and not args.fid_stats:
        ap.error("--fid_weights without --fid_stats measures against ground truth: it needs --gt")
    if args.gt is None and not args.niqe_params and not args.fid_stats:
        ap.error("--gt is required unless --niqe_params asks for the no-reference score")
    if args.gt is None and (args.lpips_weights or args.id_weights):
        ap.error("--lpips_weights / --id_weights compare against ground truth: they need --gt")
    lmd_box = check_lmd_arguments(ap, args, True, args.gt is not None)
    niqe_params = fid_stats = None
    try:
        if args.fid_stats:
            from .fid import load_stats
            fid_stats = load_stats(args.fid_stats)
        if args.niqe_params:
            from .niqe import load_params
            niqe_params = load_params(args.niqe_params)
        pairs = pair_files(args.restored, args.gt, args.pattern) if args.gt is not None else restored_files(args.restored, args.pattern)
    except (ValueError, FileNotFoundError) as e:
        ap.error(str(e))
    from .metrics import load_scorers, summary_line, write_report
    lp, idl = load_scorers(args.lpips_weights, args.id_weights)
    fid, held = None, []
    if args.fid_weights:
        from . import fid as fid_mod
        fid = (fid_mod.FidInception(fid_mod.load(args.fid_weights), "cuda"), fid_stats, args.fid_stats)
    kw = {}
    if args.lmd_weights:
        from .fan import FanLandmarks
        try:
            kw = {"lmd": FanLandmarks(args.lmd_weights, "cuda"), "lmd_box": lmd_box}
        except ValueError as e:
            ap.error(str(e))
    report = score_pairs(pairs, args.ssim_window, lp, idl, args.batch, args.dataset, niqe=niqe_params, fid=fid, evaluator=held, **kw)
    if args.out and fid is not None:
        from .metrics import write_report_with_features
        write_report_with_features(held[0], report, args.out)
    elif args.out:
        write_report(report, args.out)
    else:
        print(json.dumps(report, indent=1, allow_nan=False))
    print(summary_line(report))
    return report


if __name__ == "__main__":
    main()
