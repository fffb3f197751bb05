"""No-reference quality for runs without ground truth: NIQE (Mittal, Soundararajan, Bovik 2013) on the device.

The 36 features per 96 x 96 block -- luma, two scales, local normalisation, the asymmetric generalised Gaussian fits of the
normalised block and of its four neighbour products -- come from ONE kernel launch per batch (`hip_ops.niqe_features_u8`,
csrc/niqe.hip) on the uint8 tensor the PNG writer sends to disk, without host synchronisation.  What is left is a 36 x 36
problem per image: mean and covariance over the blocks, the distance to a pristine model; that runs in NumPy float64 on the host,
from `metrics.Evaluator.report()` only.

No pristine model is shipped (as with the LPIPS and ID weights).  `load_params` reads the usual `.npz` (`mu_pris_param`,
`cov_pris_param`); `python -m vspbfr_amd.niqe_fit` builds one from a folder of high-quality images with the same kernel."""
import numpy as np

FEATURES = 36
SHARPNESS_SHARE = 0.75   # the fit keeps the blocks whose mean sigma_loc exceeds this share of the image's sharpest block


def features(u8, crop_border=0):
    """(B, H, W, 3) uint8 on the device -> (features float64 (B, nblk, 36), sharpness float32 (B, nblk)) on the device; no
    synchronisation.  A block with a one-sided map (a flat block: exact zeros) has NaN in its row."""
    from . import hip_ops as H
    return H.niqe_features_u8(u8, crop_border)


def _check_params(mu, cov, where):
    mu, cov = np.asarray(mu, dtype=np.float64).reshape(-1), np.asarray(cov, dtype=np.float64)
    if mu.shape != (FEATURES,) or cov.shape != (FEATURES, FEATURES):
        raise ValueError(f"{where}: a NIQE model is a mean of {FEATURES} and a {FEATURES} x {FEATURES} covariance "
                         f"(got {mu.shape} and {cov.shape})")
    if not (np.isfinite(mu).all() and np.isfinite(cov).all()):
        raise ValueError(f"{where}: the NIQE model holds non-finite values")
    return mu, cov


def load_params(path):
    """(mu (36,), cov (36, 36)) float64 from an .npz with `mu_pris_param` / `cov_pris_param` (also `mu_prisparam` / `cov_prisparam`)."""
    with np.load(path) as z:
        for mk, ck in (("mu_pris_param", "cov_pris_param"), ("mu_prisparam", "cov_prisparam")):
            if mk in z.files and ck in z.files:
                return _check_params(z[mk], z[ck], str(path))
        raise ValueError(f"{path}: no mu_pris_param / cov_pris_param (or mu_prisparam / cov_prisparam) in {sorted(z.files)}")


def save_params(path, mu, cov):
    mu, cov = _check_params(mu, cov, "save_params")
    np.savez(path, mu_pris_param=mu.reshape(1, FEATURES), cov_pris_param=cov)


def _finite_rows(feats):
    feats = np.asarray(feats, dtype=np.float64).reshape(-1, FEATURES)
    return feats[~np.isnan(feats).any(axis=1)]


def score_from_features(feats, params):
    """The NIQE score of one image from its (nblk, 36) block features: sqrt(d pinv((cov_pris + cov) / 2) d^T), d = mu_pris - mu, mean
    and `np.cov` over the rows without NaN.  Host NumPy float64.  None when fewer than two rows are left (no covariance)."""
    mu_p, cov_p = params
    rows = _finite_rows(feats)
    if rows.shape[0] < 2:
        return None
    mu = rows.mean(axis=0)
    cov = np.cov(rows, rowvar=False)
    d = (np.asarray(mu_p, dtype=np.float64).reshape(-1) - mu).reshape(1, FEATURES)
    q = float((d @ np.linalg.pinv((np.asarray(cov_p, dtype=np.float64) + cov) / 2.0) @ d.T)[0, 0])
    return float(np.sqrt(q))


def select_sharp(feats, sharpness, share=SHARPNESS_SHARE):
    """The rows of one image's (nblk, 36) features whose block sharpness exceeds `share` x the image's maximum."""
    feats = np.asarray(feats, dtype=np.float64).reshape(-1, FEATURES)
    sharpness = np.asarray(sharpness, dtype=np.float64).reshape(-1)
    if sharpness.shape[0] != feats.shape[0]:
        raise ValueError(f"select_sharp: {feats.shape[0]} blocks but {sharpness.shape[0]} sharpness values")
    return feats[sharpness > share * sharpness.max()]


def fit_params(feature_iter, share=SHARPNESS_SHARE):
    """A pristine model from an iterable of per-image (features (nblk, 36), sharpness (nblk,)): the sharp blocks of every image
    (`select_sharp`), rows with NaN dropped, their mean and `np.cov`.  -> (mu (36,), cov (36, 36))."""
    kept = [_finite_rows(select_sharp(f, s, share)) for f, s in feature_iter]
    rows = np.concatenate(kept, axis=0) if kept else np.zeros((0, FEATURES))
    if rows.shape[0] <= FEATURES:
        raise ValueError(f"fit_params: {rows.shape[0]} usable blocks cannot fix a {FEATURES} x {FEATURES} covariance; give more images")
    return _check_params(rows.mean(axis=0), np.cov(rows, rowvar=False), "fit_params")
