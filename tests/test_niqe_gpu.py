"""GPU: the NIQE feature kernel (vspbfr_amd/csrc/niqe.hip) against the float64 oracle tests/niqe_ref.py.

Bound of the smooth quantities (left_std, right_std, rnorm of every map): 4 x e_ref, e_ref = the worst relative error of a plain
float32 restatement (torch CPU) of the white-noise case, measured here.  That case has no brightness to cancel, so its error is
what the format costs; the factor 4 covers the other summation order and scale 2's float32 input.  The same bound holds on the
bright-flat case, where the plain form loses three digits: the kernel accumulates around the block's own integer mean."""
import numpy as np
import pytest
import torch
from scipy.special import gamma as G

import niqe_ref as R

pytestmark = pytest.mark.gpu

# name -> (kind, H, W, seed, byte offset of the operand)
CASES = {
    "white_96x192": ("white", 96, 192, 11, 0),
    "white_192x96": ("white", 192, 96, 12, 0),
    "smooth_192x192": ("smooth", 192, 192, 13, 0),
    "white_192x192": ("white", 192, 192, 14, 0),
    "bright_200x301_off1": ("bright", 200, 301, 15, 1),
    "smooth_200x301_off3": ("smooth", 200, 301, 16, 3),
    "bright_192x192": ("bright", 192, 192, 17, 0),
    "white_512": ("white", 512, 512, 18, 0),
}
_cache = {}


def oracle(name):
    if name not in _cache:
        kind, h, w, seed, _ = CASES[name]
        img = R.case_image(kind, h, w, seed)
        _cache[name] = (img, R.analyse(img))
    return _cache[name]


def bound():
    if "e_ref" not in _cache:
        img, ref = oracle("white_192x192")
        _cache["e_ref"] = float(np.max(np.abs(R.plain_fp32(img) - ref["smooth"]) / np.abs(ref["smooth"])))
    return _cache["e_ref"], 4.0 * _cache["e_ref"]


def on_device(img, off=0):
    """(1, H, W, 3) uint8 on the device whose first byte sits `off` bytes behind an aligned address"""
    n = img.size
    buf = torch.empty(n + 8, dtype=torch.uint8, device="cuda")
    view = buf[off:off + n].view(1, *img.shape)
    view.copy_(torch.from_numpy(img)[None])
    assert view.data_ptr() % 4 == off % 4
    return view


def run(u8):
    from vspbfr_amd import hip_ops as H
    f, s, m = H.niqe_features_u8(u8, 0, with_moments=True)
    return f.cpu().numpy(), s.cpu().numpy(), m.cpu().numpy()


def smooth_of_moments(mom):
    """(nblk, 2, 5, 6) -> (nblk, 2, 5, 3)"""
    return np.stack([R.smooth_from_raw(mom[:, s], float((96 >> s) ** 2)) for s in range(2)], axis=1)


@pytest.mark.parametrize("name", list(CASES))
def test_features_against_the_oracle(name):
    img, ref = oracle(name)
    assert ref["tiny"] == 0                                        # the oracle itself is well-conditioned on this input
    e_ref, bnd = bound()
    feats, sharp, mom = run(on_device(img, CASES[name][4]))
    feats, sharp, mom = feats[0], sharp[0], mom[0]
    assert feats.shape == ref["features"].shape and np.isfinite(feats).all()
    # 1. the smooth quantities
    sm = smooth_of_moments(mom)
    err = np.abs(sm - ref["smooth"]) / np.abs(ref["smooth"])
    print(f"{name}: e_ref {e_ref:.3e} e_hip {err.max():.3e} ratio {err.max() / e_ref:.3f} (bound 4)")
    assert err.max() <= bnd
    assert np.abs(sharp - ref["sharpness"]).max() <= 1e-5 * ref["sharpness"].max()
    # 2. alpha: the oracle's grid point, or its neighbour where the oracle's own lookup flips within the bound
    cols = [0] + [2 + 4 * m for m in range(4)]
    flips = 0
    for b in range(feats.shape[0]):
        for s in range(2):
            for m in range(5):
                k = int(round((feats[b, 18 * s + cols[m]] - 0.2) / 0.001))
                assert abs(feats[b, 18 * s + cols[m]] - R.GAM[k]) < 1e-12
                k0 = ref["alpha_idx"][b, s, m]
                if k != k0:
                    rn = ref["smooth"][b, s, m, 2]
                    assert abs(k - k0) == 1 and k in (R.lookup(rn * (1 - bnd)), R.lookup(rn * (1 + bnd))), (name, b, s, m, k, k0)
                    flips += 1
                # 3. the remaining features, recomputed in float64 from the kernel's own deviations and alpha
                a = R.GAM[k]
                sc = np.sqrt(G(1 / a) / G(3 / a))
                bl, br = sm[b, s, m, 0] * sc, sm[b, s, m, 1] * sc
                want = [a, (bl + br) / 2] if m == 0 else [a, (br - bl) * G(2 / a) / G(1 / a), bl, br]
                got = feats[b, 18 * s + cols[m]:18 * s + cols[m] + len(want)]
                assert np.allclose(got, want, rtol=1e-12, atol=0), (name, b, s, m, got, want)
    print(f"{name}: {flips} alpha flips of {feats.shape[0] * 10}")


def fit_set():
    """six 384^2 images with a softer right half (the fit's selection has work to do) and their oracle analyses, computed once"""
    if "fit_set" not in _cache:
        imgs = []
        for i in range(6):
            img = R.case_image(("white", "smooth")[i % 2], 384, 384, 50 + i)
            img[:, 192:] = (img[:, 192:].astype(np.int32) // (2 + i) + 60).astype(np.uint8)
            imgs.append(img)
        _cache["fit_set"] = (imgs, [R.analyse(img) for img in imgs])
    return _cache["fit_set"]


def kernel_alpha(feats, ref, bnd, what):
    """the kernel's grid indices (nblk, 2, 5), each the oracle's or its neighbour where the oracle's own lookup flips within the bound"""
    cols = [0] + [2 + 4 * m for m in range(4)]
    k = np.rint((feats.reshape(-1, 2, 18)[:, :, cols] - 0.2) / 0.001).astype(np.int64)
    for idx in zip(*np.nonzero(k != ref["alpha_idx"])):
        rn = ref["smooth"][idx][2]
        assert abs(k[idx] - ref["alpha_idx"][idx]) == 1 and k[idx] in (R.lookup(rn * (1 - bnd)), R.lookup(rn * (1 + bnd))), (what, idx)
    return k


def feature_budget(smooth, alpha_idx, bnd):
    """(reference features, per-element error budget): the features with the shape parameters held at alpha_idx, and the largest change
    when both deviations of a map move by the bound, together or against each other (every feature is linear in them)"""
    base = R.features_with_alpha(smooth, alpha_idx)
    e = np.zeros_like(base)
    for sl, sr in ((1, 1), (1, -1), (-1, 1), (-1, -1)):
        sm = smooth.copy()
        sm[..., 0] *= 1 + sl * bnd
        sm[..., 1] *= 1 + sr * bnd
        e = np.maximum(e, np.abs(R.features_with_alpha(sm, alpha_idx) - base))
    return base, e


def test_score_against_the_oracle():
    """The final score of images that are not in the model, against a full-rank model (96 oracle rows of six other images).  The shape
    parameters are settled first (the oracle's, or a neighbour only where the oracle's own lookup flips within the bound) and held;
    the rest of the bound is propagated through the oracle by finite differences: each deviation of each map moved by +-bound, the
    larger change of the score, summed."""
    _, bnd = bound()
    from vspbfr_amd import niqe
    mu_p, cov_p = R.fit(fit_set()[1], share=0.0)
    assert np.linalg.matrix_rank(cov_p) == 36
    scores = []
    for name in ("white_192x192", "smooth_200x301_off3", "bright_192x192"):
        img, ref = oracle(name)
        feats, _, _ = run(on_device(img))
        k = kernel_alpha(feats[0], ref, bnd, name)
        want = R.score(R.features_with_alpha(ref["smooth"], k), mu_p, cov_p)
        if (k == ref["alpha_idx"]).all():
            assert want == R.score(ref["features"], mu_p, cov_p)
        allowed = 0.0
        for idx in np.ndindex(ref["smooth"].shape[:3] + (2,)):
            worst = 0.0
            for sign in (1.0, -1.0):
                sm = ref["smooth"].copy()
                sm[idx] *= 1.0 + sign * bnd
                worst = max(worst, abs(R.score(R.features_with_alpha(sm, k), mu_p, cov_p) - want))
            allowed += worst
        got = niqe.score_from_features(feats[0], (mu_p, cov_p))
        print(f"{name}: score {got:.9f} oracle {want:.9f} rel err {abs(got - want) / want:.3e} allowed {allowed / want:.3e}")
        assert abs(got - want) <= allowed and allowed < 1e-3 * want
        scores.append(want)
    assert len({round(v, 6) for v in scores}) == 3                 # the score depends on the image


def test_flat_blocks_give_exact_zeros():
    """Left half constant: the blocks inside it are exact zeros (no sample on either side, NaN rows that the score drops), every
    other block is finite, and the score is finite."""
    from vspbfr_amd import niqe
    img = R.case_image("half", 192, 384, 21)
    feats, sharp, mom = run(on_device(img))
    feats, mom = feats[0], mom[0]
    flat = [0, 4]                                                  # block column 0: the Gaussian's reach stays inside the constant half
    assert np.isnan(feats[flat]).any(axis=1).all() and (mom[flat] == 0).all() and (sharp[0][flat] == 0).all()
    rest = [2, 3, 6, 7]                                            # white noise; block column 1 sees noise in its last three columns only
    assert np.isfinite(feats[rest]).all() and np.isfinite(mom).all()
    n = np.array([96.0 ** 2, 48.0 ** 2])[None, :, None]
    assert (mom[..., 0] + mom[..., 2] <= n).all() and (mom[rest][:, :, 0, 0] + mom[rest][:, :, 0, 2] > 0).all()
    mu_p, cov_p = R.fit([oracle("white_512")[1], oracle("smooth_192x192")[1], oracle("bright_192x192")[1]], share=0.0)
    s = niqe.score_from_features(feats, (mu_p, cov_p))
    assert s is not None and np.isfinite(s)
    f3, _, _ = run(torch.cat([on_device(R.case_image("white", 192, 384, 22)), on_device(img)]))
    assert f3[1].tobytes() == feats.tobytes()


def test_bits_do_not_depend_on_batch_position_launch_or_stream():
    from vspbfr_amd import hip_ops as H
    imgs = np.stack([R.case_image(("white", "smooth", "bright")[i % 3], 192, 192, 30 + i) for i in range(8)])
    dev = torch.from_numpy(imgs).cuda()
    f8, s8, m8 = H.niqe_features_u8(dev, 0, with_moments=True)
    again = H.niqe_features_u8(dev, 0, with_moments=True)
    for a, b in zip((f8, s8, m8), again):
        assert torch.equal(a.view(torch.uint8), b.view(torch.uint8))
    f3, s3, m3 = H.niqe_features_u8(dev[[5, 0, 2]].contiguous(), 0, with_moments=True)
    for k, i in enumerate((5, 0, 2)):
        assert torch.equal(f3[k].view(torch.uint8), f8[i].view(torch.uint8)) and torch.equal(m3[k], m8[i]) and torch.equal(s3[k], s8[i])
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        f1, s1 = H.niqe_features_u8(dev[6:7], 0)
    side.synchronize()
    assert torch.equal(f1[0].view(torch.uint8), f8[6].view(torch.uint8)) and torch.equal(s1[0], s8[6])
    # the batch against the oracle as well: image 7 of 8
    ref = R.analyse(imgs[7])
    _, bnd = bound()
    sm = smooth_of_moments(m8[7].cpu().numpy())
    assert (np.abs(sm - ref["smooth"]) / np.abs(ref["smooth"])).max() <= bnd


def test_crop_border_and_refusals():
    from vspbfr_amd import hip_ops as H
    img = R.case_image("smooth", 208, 304, 40)
    ref = R.analyse(img, crop_border=5)                            # 198 x 294 -> 192 x 288
    _, bnd = bound()
    f, s, m = H.niqe_features_u8(torch.from_numpy(img)[None].cuda(), 5, with_moments=True)
    sm = smooth_of_moments(m[0].cpu().numpy())
    assert (np.abs(sm - ref["smooth"]) / np.abs(ref["smooth"])).max() <= bnd
    with pytest.raises(RuntimeError, match="fewer than two"):
        H.niqe_features_u8(torch.zeros(1, 191, 191, 3, dtype=torch.uint8, device="cuda"))
    with pytest.raises(RuntimeError, match="fewer than two"):
        H.niqe_features_u8(torch.zeros(1, 192, 192, 3, dtype=torch.uint8, device="cuda"), 49)
    with pytest.raises(RuntimeError, match="uint8 RGB"):
        H.niqe_features_u8(torch.zeros(1, 192, 192, 1, dtype=torch.uint8, device="cuda"))


def test_fit_tool_equals_the_oracles_fit(tmp_path):
    """`python -m vspbfr_amd.niqe_fit` on a folder against the oracle's fit on the same files: the same blocks are selected; every
    selected row lies within the bound of the smooth quantities propagated to the features; the saved model is the mean and `np.cov` of
    the tool's own rows; and it differs from the oracle's model by no more than those row budgets allow (mean: their mean; covariance:
    sum over rows of |d_i| e_j + e_i |d_j| + e_i e_j with d the centred rows and e the budgets plus their mean, over N - 1)."""
    from PIL import Image
    from vspbfr_amd import niqe, niqe_fit
    _, bnd = bound()
    imgs, refs = fit_set()
    src = tmp_path / "hq"
    src.mkdir()
    for i, img in enumerate(imgs):
        Image.fromarray(img).save(src / f"im{i}.png")
    out = tmp_path / "model.npz"
    niqe_fit.main(["--images", str(src), "--out", str(out), "--batch", "3"])
    mu, cov = niqe.load_params(out)
    rows, want, budget, same_alpha = [], [], [], True
    for (f, sh), ref in zip(niqe_fit.image_features(sorted(str(p) for p in src.iterdir()), 0, 3), refs):
        keep = R.sharp_mask(ref["sharpness"])
        assert np.array_equal(R.sharp_mask(sh.astype(np.float64)), keep) and 0 < keep.sum() < len(keep)      # the same blocks
        k = kernel_alpha(f, ref, bnd, "fit")
        same_alpha = same_alpha and bool((k == ref["alpha_idx"]).all())
        base, e = feature_budget(ref["smooth"], k, bnd)
        assert (np.abs(f - base) <= e).all()
        rows.append(f[keep])
        want.append(base[keep])
        budget.append(e[keep])
    rows, want, budget = np.concatenate(rows), np.concatenate(want), np.concatenate(budget)
    n = rows.shape[0]
    assert 36 < n < 96
    assert np.allclose(mu, rows.mean(0), rtol=1e-12, atol=0) and np.allclose(cov, np.cov(rows, rowvar=False), rtol=1e-10, atol=1e-18)
    mu_o, cov_o = want.mean(0), np.cov(want, rowvar=False)
    if same_alpha:                                                 # then the reference above IS the oracle's own fit
        mo, co = R.fit(refs)
        assert np.array_equal(mu_o, mo) and np.array_equal(cov_o, co)
    d, e2 = np.abs(want - mu_o), budget + budget.mean(0)
    cov_budget = (d.T @ e2 + e2.T @ d + e2.T @ e2) / (n - 1)
    with np.errstate(invalid="ignore", divide="ignore"):
        print(f"fit: {n} rows, mean err / budget {np.nanmax(np.abs(mu - mu_o) / budget.mean(0)):.3f}, "
              f"cov err / budget {np.nanmax(np.abs(cov - cov_o) / cov_budget):.3f}")
    assert (np.abs(mu - mu_o) <= budget.mean(0)).all()
    assert (np.abs(cov - cov_o) <= cov_budget).all()
