"""Full-reference image quality of restored faces against ground truth, measured on the device: PSNR, SSIM and -- with
user-supplied weights -- LPIPS and identity similarity; and, for runs without ground truth, the no-reference NIQE score of the
restored image alone against a user-supplied pristine model (vspbfr_amd/niqe.py).

The reference has the pixel metrics as host code for one image at a time (my_lpips.psnr / my_lpips.dssim,
my_lpips/__init__.py:57-61; networks_basic.DSSIM / L2, networks_basic.py:143-180) and never calls them.  Here they come from
one kernel launch per batch (`hip_ops.pair_stats_u8`: exact sum of squared differences + mean SSIM over the valid window
positions) on the SAME uint8 tensors the PNG writer sends to disk, so a reported number is the number anyone gets from the
files.  Nothing below synchronises with the host until `Evaluator.report()`.

Windows: "gauss11" (11 x 11 Gaussian, sigma 1.5, population covariance: Wang et al. 2004, the form restoration papers report)
and "uniform7" (7 x 7 box, sample covariance: scikit-image's defaults, what the reference's `dssim` computes)."""
import json
import math
import os

import torch

WINDOWS = ("gauss11", "uniform7")
COLUMNS = ("psnr", "ssim", "lpips", "id", "niqe", "lmd", "nme")
PEAK = 255.0


def psnr_from_sse(sse, count):
    """PSNR of an 8-bit image pair from its exact sum of squared differences over `count` samples, in float64 on the host
    (the reference's psnr(p0, p1, 255.): 10 log10(peak^2 / mse)); None when the images are identical."""
    sse, count = int(sse), int(count)
    if sse == 0:
        return None
    return 10.0 * math.log10(PEAK * PEAK * count / sse)


def _as_u8_pair(a, b):
    from . import hip_ops as H
    if not (isinstance(a, torch.Tensor) and isinstance(b, torch.Tensor)):
        raise RuntimeError("metrics: operands must be tensors")
    if a.dtype != b.dtype or a.shape != b.shape:
        raise RuntimeError(f"metrics: operands differ in dtype or shape ({a.dtype} {tuple(a.shape)} vs {b.dtype} {tuple(b.shape)})")
    if a.dtype == torch.uint8:
        if a.dim() != 4 or a.shape[3] != 3:
            raise RuntimeError(f"metrics: uint8 operands must be (B, H, W, 3) (got {tuple(a.shape)})")
        return a, b
    if a.dtype == torch.float32:
        if a.dim() != 4 or a.shape[1] != 3:
            raise RuntimeError(f"metrics: float operands must be (B, 3, H, W) in [-1, 1] (got {tuple(a.shape)})")
        return H.quantize_u8_nhwc(a.contiguous(), -1.0, 1.0), H.quantize_u8_nhwc(b.contiguous(), -1.0, 1.0)
    raise RuntimeError(f"metrics: operands must be float32 (B, 3, H, W) or uint8 (B, H, W, 3) (got {a.dtype})")


def psnr_ssim(a, b, window="gauss11"):
    """Two (B, 3, H, W) float32 tensors in [-1, 1] (quantised to 8 bits the way the PNG writer does) or two (B, H, W, 3) uint8
    tensors -> (psnr float64 (B,), ssim float64 (B,)) on the device; psnr is +inf for identical images.  No synchronisation."""
    from . import hip_ops as H
    a, b = _as_u8_pair(a, b)
    sse, ssim = H.pair_stats_u8(a, b, window)
    count = float(a.shape[1] * a.shape[2] * a.shape[3])
    psnr = 10.0 * torch.log10((PEAK * PEAK * count) / sse.to(torch.float64))
    return psnr, ssim


def dequantize(u8):
    """(B, H, W, 3) uint8 -> (B, 3, H, W) float32 in [-1, 1]: the image a reader of the PNG file gets (u8 / 127.5 - 1)."""
    return (u8.permute(0, 3, 1, 2).to(torch.float32) / 127.5 - 1.0).contiguous()


def _mean(values):
    values = [v for v in values if v is not None]
    return math.fsum(values) / len(values) if values else None


def summarize(rows, dataset=None, window="gauss11"):
    """The report of a list of per-image rows: mean of every column present (mean PSNR = mean of the per-image PSNR over the
    pairs that have one; identical pairs are counted in `psnr_infinite`)."""
    rows = sorted(rows, key=lambda r: r["index"])
    cols = [c for c in COLUMNS if any(c in r for r in rows)]
    return {
        "dataset": dataset, "count": len(rows), "window": window,
        "psnr_infinite": sum(1 for r in rows if "sse" in r and r.get("psnr") is None),
        "mean": {c: _mean([r.get(c) for r in rows]) for c in cols},
        "images": rows,
    }


class Evaluator:
    """Scores batches of restored images against their ground truth.

        ev = Evaluator(window="gauss11", lpips=PerceptualLoss(...) or None, idloss=IDLoss(...) or None)
        ev.add(restored_u8, gt_u8, names)      # per batch, (B, H, W, 3) uint8 on the device; no host synchronisation
        report = ev.report(dataset="celeba")   # one device-to-host copy of all columns: the only synchronisation

    `names`: one `(lq, hq)` pair of file names per image (or None).  `lpips` / `idloss` add the columns `lpips`
    (= PerceptualLoss(restored, gt) per image) and `id` (= cosine of the IDLoss.get_id embeddings per image); both see the
    de-quantised uint8 images, so every column describes the files on disk.

    `niqe` = (mu, cov) of a pristine model (`niqe.load_params`) adds the column `niqe`: the no-reference score of the restored image
    alone (one more launch per batch; the 36 x 36 finish runs on the host inside `report()`; an image without two usable blocks gets
    None).  With `niqe` and neither `lpips` nor `idloss`, `add(restored, None, names)` scores a batch that has no ground truth: its
    rows hold `niqe` only.

    `fid` = (FidInception, (mu, sigma) or None[, the statistics' file name]) adds the top-level `fid` entry of the report (vspbfr_amd/fid.py):
    `add` appends the batch's device features of the restored images -- and of the ground truth when the statistics are None --
    without a host synchronisation; `report()` makes one more copy, computes the Frechet distance on the host and keeps the features
    in `fid_features` (and `fid_gt_features`), in row order.  The rows do not change: FID is a property of the set.  With statistics,
    `add(restored, None, names)` is legal like it is for NIQE.

    `lmd` = a fan.FanLandmarks adds the columns `lmd` and `nme`: `add` runs restored and ground truth through the landmark
    network in one batch and appends the per-image mean landmark distance in image pixels and that distance over the ground truth's
    outer-eye-corner distance, both computed on the device; `lmd_box` = (x0, y0, s) is the square of every image the network sees
    (default: the whole image).  An image of which a heatmap held a non-finite value gets None in both.  Like `lpips`, `lmd` needs the
    ground truth."""

    def __init__(self, window="gauss11", lpips=None, idloss=None, niqe=None, niqe_crop_border=0, fid=None, lmd=None, lmd_box=None):
        if window not in WINDOWS:
            raise ValueError(f"window must be one of {WINDOWS} (got {window!r})")
        self.window, self.lpips, self.idloss, self.niqe, self.niqe_crop_border = window, lpips, idloss, niqe, niqe_crop_border
        if fid is not None and (not isinstance(fid, (tuple, list)) or len(fid) not in (2, 3)):
            raise ValueError("fid takes (FidInception, (mu, sigma) or None[, file name])")
        self.fid = None if fid is None else (fid[0], fid[1], fid[2] if len(fid) == 3 else None)
        self.fid_dev, self.fid_gt_dev = [], []   # per batch (B, 2048) float32 on the device
        self.fid_features = self.fid_gt_features = None
        self.meta = []       # (index, lq, hq, samples per image; None without ground truth)
        if lmd is None and lmd_box is not None:
            raise ValueError("lmd_box only has a meaning with lmd")
        self.lmd, self.lmd_box = lmd, lmd_box
        self.dev = {"sse": [], "ssim": [], "lpips": [], "id": [], "lmd": [], "nme": []}
        self.niqe_feats = []  # per batch (B, nblk, 36) float64 on the device

    def __len__(self):
        return len(self.meta)

    def add(self, restored, gt, names=None, indices=None):
        from . import hip_ops as H
        if gt is None:
            if self.fid is not None and self.fid[1] is None:
                raise RuntimeError("Evaluator.add without ground truth: FID without reference statistics is measured against the ground truth")
            if (self.niqe is None and self.fid is None) or self.lpips is not None or self.idloss is not None or self.lmd is not None:
                raise RuntimeError("Evaluator.add without ground truth needs an Evaluator that scores NIQE only (niqe=params, no lpips / idloss / lmd)")
            if self.dev["sse"]:
                raise RuntimeError("Evaluator.add: this evaluator already holds batches with ground truth")
        if not isinstance(restored, torch.Tensor) or restored.dtype != torch.uint8 or (gt is not None and gt.dtype != torch.uint8):
            raise RuntimeError("Evaluator.add takes the (B, H, W, 3) uint8 tensors that go to disk (hip_ops.quantize_u8_nhwc)")
        if gt is None:
            restored, _ = _as_u8_pair(restored, restored)
        else:
            if self.meta and not self.dev["sse"]:
                raise RuntimeError("Evaluator.add: this evaluator already holds batches without ground truth")
            restored, gt = _as_u8_pair(restored, gt)
        B = restored.shape[0]
        names = [(None, None)] * B if names is None else [tuple(n) for n in names]
        indices = list(range(len(self.meta), len(self.meta) + B)) if indices is None else [int(i) for i in indices]
        if len(names) != B or len(indices) != B or any(len(n) != 2 for n in names):
            raise RuntimeError(f"Evaluator.add: {B} images need {B} (lq, hq) name pairs and indices")
        if self.niqe is not None:
            self.niqe_feats.append(H.niqe_features_u8(restored, self.niqe_crop_border)[0])
        if self.fid is not None:
            self.fid_dev.append(self.fid[0].features(restored))
            if self.fid[1] is None:
                self.fid_gt_dev.append(self.fid[0].features(gt))
        if gt is None:
            self.meta.extend((i, n[0], n[1], None) for i, n in zip(indices, names))
            return
        sse, ssim = H.pair_stats_u8(restored, gt, self.window)
        self.dev["sse"].append(sse)
        self.dev["ssim"].append(ssim)
        if self.lpips is not None or self.idloss is not None:
            with torch.no_grad():
                r, g = dequantize(restored), dequantize(gt)
                if self.lpips is not None:
                    self.dev["lpips"].append(self.lpips(r, g).reshape(B).to(torch.float64))
                if self.idloss is not None:
                    z = self.idloss.get_id(torch.cat([r, g], 0))
                    self.dev["id"].append((z[:B] * z[B:]).sum(1).to(torch.float64))
        if self.lmd is not None:
            from .fan import lmd_nme
            # one batch of 2 B images: an image's landmarks do not depend on its place in it
            lm, _, bad = self.lmd.landmarks(torch.cat([restored, gt], 0), self.lmd_box)
            d, n = lmd_nme(lm[:B], lm[B:])
            bad = bad[:B] | bad[B:]
            self.dev["lmd"].append(torch.where(bad, torch.full_like(d, float("nan")), d))
            self.dev["nme"].append(torch.where(bad, torch.full_like(n, float("nan")), n))
        count = restored.shape[1] * restored.shape[2] * restored.shape[3]
        self.meta.extend((i, n[0], n[1], count) for i, n in zip(indices, names))

    def report(self, dataset=None):
        cols = [k for k, v in self.dev.items() if v]
        # one copy, one synchronisation: every column as float64 (an sse is an integer below 2^53, so it survives exactly)
        table = torch.stack([torch.cat(self.dev[k]).to(torch.float64) for k in cols]).cpu().tolist() if self.meta and cols else []
        host = dict(zip(cols, table)) if cols else {}
        scores = None
        if self.niqe is not None and self.meta:
            from .niqe import score_from_features
            # one more copy: the block features of every image, flattened (batches of different sizes have different block counts)
            flat = torch.cat([f.reshape(-1) for f in self.niqe_feats]).cpu().numpy()
            scores, at = [], 0
            for f in self.niqe_feats:
                per = f.shape[1] * f.shape[2]
                for _ in range(f.shape[0]):
                    scores.append(score_from_features(flat[at:at + per].reshape(f.shape[1], f.shape[2]), self.niqe))
                    at += per
        rows = []
        for k, (index, lq, hq, count) in enumerate(self.meta):
            row = {"index": index, "lq": lq, "hq": hq}
            if count is not None:
                sse = int(host["sse"][k])
                row.update({"sse": sse, "psnr": psnr_from_sse(sse, count), "ssim": host["ssim"][k]})
            for col in ("lpips", "id"):
                if col in host:
                    row[col] = host[col][k]
            if scores is not None:
                row["niqe"] = scores[k]
            for col in ("lmd", "nme"):     # a non-finite heatmap (or a ground truth whose eye corners coincide) has no figure
                if col in host:
                    row[col] = host[col][k] if math.isfinite(host[col][k]) else None
            rows.append(row)
        report = summarize(rows, dataset, self.window)
        if self.fid is not None:
            n = len(self.meta)
            # one more copy: the restored features and, against ground truth, the ground truth's behind them
            both = torch.cat(self.fid_dev + self.fid_gt_dev).cpu().numpy() if n else None
            order = sorted(range(n), key=lambda k: self.meta[k][0])          # the rows' order
            self.fid_features = both[:n][order] if n else None
            self.fid_gt_features = both[n:][order] if n and self.fid[1] is None else None
            report["fid"] = fid_entry(self.fid_features, self.fid_gt_features, self.fid[1], self.fid[2])
        return report


def fid_entry(features, gt_features, ref_stats, ref_name):
    """the report's `fid` entry from (n, 2048) features: against the ground truth's features, else against (mu, sigma); the value is
    None below two images (a covariance needs two)"""
    from .fid import frechet_distance, stats
    n = 0 if features is None else int(features.shape[0])
    against = "stats" if gt_features is None else "gt"
    value = None
    if n >= 2:
        mu, sigma = stats(features)
        rmu, rsigma = stats(gt_features) if gt_features is not None else ref_stats
        value = frechet_distance(mu, sigma, rmu, rsigma)
    return {"value": value, "count": n, "against": against, "ref": ref_name if against == "stats" else None}


def fid_feature_dtype(dims=2048):
    return [("index", "<i8"), ("features", "<f4", (dims,))]


def fid_feature_path(report_path, gt=False):
    """the feature file beside a report: metrics_<rank>.json -> fid_features_<rank>.npy (fid_features_<rank>_gt.npy for the ground truth)"""
    d, base = os.path.split(report_path)
    stem = os.path.splitext(base)[0]
    stem = "fid_features_" + stem[len("metrics_"):] if stem.startswith("metrics_") else stem + "_fid_features"
    return os.path.join(d, stem + ("_gt" if gt else "") + ".npy")


def write_fid_features(path, indices, features):
    """one record per image: its row's `index` and its float32 features (2048 of them from the FID Inception)"""
    import numpy as np
    features = np.zeros((0, 2048), dtype=np.float32) if features is None else np.asarray(features, dtype=np.float32)
    if features.ndim != 2 or features.shape[0] != len(indices):
        raise ValueError(f"write_fid_features: {len(indices)} indices for features {features.shape}")
    rec = np.zeros(len(indices), dtype=fid_feature_dtype(features.shape[1]))
    rec["index"] = np.asarray(indices, dtype=np.int64)
    rec["features"] = features
    with open(path, "wb") as f:
        np.save(f, rec)


def read_fid_features(path):
    import numpy as np
    rec = np.load(path, allow_pickle=False)
    if rec.ndim != 1 or rec.dtype.names != ("index", "features") or rec.dtype != np.dtype(fid_feature_dtype(rec.dtype["features"].shape[0])):
        raise ValueError(f"{path}: not a feature file (records of an int64 index and float32 features)")
    return rec["index"], rec["features"]


def write_report_with_features(ev, report, path):
    """write_report, and the evaluator's FID features beside it when the report has a `fid` entry"""
    write_report(report, path)
    if "fid" in report:
        idx = [r["index"] for r in report["images"]]
        write_fid_features(fid_feature_path(path), idx, ev.fid_features)
        if report["fid"]["against"] == "gt":
            write_fid_features(fid_feature_path(path, gt=True), idx, ev.fid_gt_features)


def write_report(report, path):
    with open(path, "w") as f:
        json.dump(report, f, indent=1, allow_nan=False)
        f.write("\n")


def merge_reports(paths):
    """Join the per-rank files of one dataset (pure host code): rows by index, means recomputed over all of them.  When every file has
    a `fid` entry and its feature file beside it, `fid` is recomputed from the concatenated features in index order; a mixture of files
    with and without `fid`, or a missing feature file, is refused.  Files without `fid` merge as they always did."""
    reports = []
    for p in paths:
        with open(p) as f:
            reports.append(json.load(f))
    if not reports:
        raise ValueError("merge_reports: no files")
    for key in ("dataset", "window"):
        if len({r[key] for r in reports}) != 1:
            raise ValueError(f"merge_reports: the files disagree on {key!r}: {sorted(str(r[key]) for r in reports)}")
    rows = [row for r in reports for row in r["images"]]
    if len({row["index"] for row in rows}) != len(rows):
        raise ValueError("merge_reports: an image index appears more than once")
    merged = summarize(rows, reports[0]["dataset"], reports[0]["window"])
    with_fid = [r for r in reports if "fid" in r]
    if with_fid:
        import numpy as np
        if len(with_fid) != len(reports):
            raise ValueError("merge_reports: some files have a fid entry and some have none")
        heads = {(r["fid"]["against"], r["fid"]["ref"]) for r in reports}
        if len(heads) != 1:
            raise ValueError(f"merge_reports: the files disagree on what fid is measured against: {sorted(map(str, heads))}")
        against, ref = next(iter(heads))

        def gather(gt):
            idx, feats = [], []
            for p, r in zip(paths, reports):
                fp = fid_feature_path(p, gt)
                if not os.path.exists(fp):
                    raise ValueError(f"merge_reports: {p} has a fid entry but {fp} is missing")
                i, f = read_fid_features(fp)
                if sorted(i.tolist()) != sorted(row["index"] for row in r["images"]):
                    raise ValueError(f"merge_reports: {fp} does not hold the images of {p}")
                idx.append(i), feats.append(f)
            idx, feats = np.concatenate(idx), np.concatenate(feats)
            return feats[np.argsort(idx, kind="stable")]

        ref_stats = None
        if against == "stats":
            from .fid import load_stats
            ref_stats = load_stats(ref, dims=None)
        merged["fid"] = fid_entry(gather(False), gather(True) if against == "gt" else None, ref_stats, ref)
    return merged


def summary_line(report):
    m = report["mean"]
    parts = [f"{c} {m[c]:.6g}" if m.get(c) is not None else f"{c} n/a" for c in COLUMNS if c in m]
    if "fid" in report:
        v = report["fid"]["value"]
        parts.append("fid n/a" if v is None else f"fid {v:.6g}")
    return "metrics %s (%s, %d images, %d identical): %s" % (report["dataset"], report["window"], report["count"],
                                                            report["psnr_infinite"], ", ".join(parts))


def load_scorers(lpips_weights=None, id_weights=None, device="cuda"):
    """The optional learned metrics from user-supplied weight files: `lpips_weights` = "LIN[,VGG]" (the reference's
    my_lpips/weights/v0.1/vgg.pth and a torchvision vgg16 state dict), `id_weights` = a resnet101(num_classes=256) state dict."""
    lp = idl = None
    if lpips_weights:
        from .lpips import PerceptualLoss
        parts = str(lpips_weights).split(",")
        if len(parts) > 2 or not all(parts):
            raise ValueError("--lpips_weights takes LIN or LIN,VGG")
        lp = PerceptualLoss(lin_weights=parts[0], vgg_weights=parts[1] if len(parts) == 2 else None).to(device)
    if id_weights:
        from .id_loss import IDLoss
        idl = IDLoss(str(id_weights), device=device)
    return lp, idl
