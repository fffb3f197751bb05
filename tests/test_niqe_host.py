"""CPU: the host side of the no-reference score -- model files, the 36 x 36 finish, the fit's block selection, the report with the
`niqe` column, the argument rules of the two CLIs and the refusals of the C entry (no launch happens on any of these paths)."""
import json

import numpy as np
import pytest

import niqe_ref as R


def _model(seed=0):
    rng = np.random.default_rng(seed)
    a = rng.normal(size=(36, 36))
    return rng.normal(size=36), a @ a.T / 36 + np.eye(36)


def test_load_params_names_shapes_and_refusals(tmp_path):
    from vspbfr_amd import niqe
    mu, cov = _model()
    niqe.save_params(tmp_path / "a.npz", mu, cov)
    got = niqe.load_params(tmp_path / "a.npz")
    assert np.array_equal(got[0], mu) and np.array_equal(got[1], cov) and got[0].shape == (36,)
    np.savez(tmp_path / "b.npz", mu_prisparam=mu[None], cov_prisparam=cov)          # the other spelling, (1, 36)
    assert np.array_equal(niqe.load_params(tmp_path / "b.npz")[0], mu)
    np.savez(tmp_path / "c.npz", mu_pris_param=mu[:35], cov_pris_param=cov)
    np.savez(tmp_path / "d.npz", mu_pris_param=mu, cov_pris_param=cov[:, :35])
    np.savez(tmp_path / "e.npz", mean=mu, cov=cov)
    bad = cov.copy()
    bad[0, 0] = np.nan
    np.savez(tmp_path / "f.npz", mu_pris_param=mu, cov_pris_param=bad)
    for name, word in (("c", "36"), ("d", "36"), ("e", "mu_pris_param"), ("f", "non-finite")):
        with pytest.raises(ValueError, match=word):
            niqe.load_params(tmp_path / f"{name}.npz")


def test_score_from_features_equals_the_oracle_and_drops_nan_rows():
    from vspbfr_amd import niqe
    rng = np.random.default_rng(3)
    feats = rng.normal(size=(9, 36))
    params = _model(4)
    assert abs(niqe.score_from_features(feats, params) - R.score(feats, *params)) < 1e-12
    holes = feats.copy()
    holes[2, 7] = np.nan
    holes[5] = np.nan
    assert niqe.score_from_features(holes, params) == niqe.score_from_features(feats[[0, 1, 3, 4, 6, 7, 8]], params)
    assert abs(niqe.score_from_features(holes, params) - R.score(holes, *params)) < 1e-12
    holes[1:] = np.nan
    assert niqe.score_from_features(holes, params) is None                        # one row: no covariance


def test_fit_params_keeps_the_sharp_blocks():
    from vspbfr_amd import niqe
    rng = np.random.default_rng(5)
    per_image, kept = [], []
    for _ in range(16):
        f, s = rng.normal(size=(16, 36)), rng.uniform(1, 10, 16)
        f[3, 0] = np.nan
        per_image.append((f, s))
        keep = s > 0.75 * s.max()
        keep[3] = False
        kept.append(f[keep])
    with pytest.raises(ValueError, match="usable blocks"):
        niqe.fit_params(per_image[:1])
    rows = np.concatenate(kept)
    assert 36 < len(rows) < 16 * 15
    mu, cov = niqe.fit_params(per_image)
    assert np.allclose(mu, rows.mean(0), rtol=0, atol=1e-14) and np.allclose(cov, np.cov(rows, rowvar=False), rtol=0, atol=1e-14)
    with pytest.raises(ValueError, match="sharpness"):
        niqe.select_sharp(np.zeros((4, 36)), np.ones(3))
    assert niqe.select_sharp(np.arange(4 * 36.0).reshape(4, 36), [1.0, 4.0, 3.0, 3.5]).shape == (2, 36)


def _rows_gt():
    return [{"index": 1, "lq": "b", "hq": "b", "sse": 0, "psnr": None, "ssim": 1.0}, {"index": 0, "lq": "a", "hq": "a", "sse": 7, "psnr": 40.0, "ssim": 0.5}]


def test_reports_with_and_without_the_column(tmp_path):
    from vspbfr_amd import metrics as M
    gt = M.summarize(_rows_gt(), "d", "gauss11")
    assert list(gt) == ["dataset", "count", "window", "psnr_infinite", "mean", "images"] and gt["psnr_infinite"] == 1
    assert gt["mean"] == {"psnr": 40.0, "ssim": 0.75} and M.summary_line(gt) == "metrics d (gauss11, 2 images, 1 identical): psnr 40, ssim 0.75"
    # the bytes of a report without NIQE are what they were: key order, no new key
    assert json.dumps(gt, indent=1) == json.dumps({"dataset": "d", "count": 2, "window": "gauss11", "psnr_infinite": 1,
                                                   "mean": {"psnr": 40.0, "ssim": 0.75}, "images": list(reversed(_rows_gt()))}, indent=1)
    both = M.summarize([dict(r, niqe=3.0 + r["index"]) for r in _rows_gt()], "d")
    assert both["mean"] == {"psnr": 40.0, "ssim": 0.75, "niqe": 3.5} and both["psnr_infinite"] == 1
    assert M.summary_line(both).endswith("psnr 40, ssim 0.75, niqe 3.5")
    alone = M.summarize([{"index": 0, "lq": "a", "hq": None, "niqe": 5.0}, {"index": 1, "lq": "b", "hq": None, "niqe": None}], "w")
    assert alone["mean"] == {"niqe": 5.0} and alone["psnr_infinite"] == 0           # rows without an sse are not identical pairs
    assert M.summary_line(alone) == "metrics w (gauss11, 2 images, 0 identical): niqe 5"
    for k, rows in enumerate(([alone["images"][0]], [alone["images"][1]])):
        M.write_report(M.summarize(rows, "w"), tmp_path / f"m{k}.json")
    assert M.merge_reports([tmp_path / "m0.json", tmp_path / "m1.json"]) == alone


def test_evaluator_argument_rules():
    import torch
    from vspbfr_amd import metrics as M
    x = torch.zeros(1, 192, 192, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="NIQE only"):
        M.Evaluator().add(x, None)
    with pytest.raises(RuntimeError, match="NIQE only"):
        M.Evaluator(niqe=_model(), lpips=object()).add(x, None)
    for gt in (None, x):                                           # one rule with and without ground truth: the bytes that go to disk
        with pytest.raises(RuntimeError, match="uint8"):
            M.Evaluator(niqe=_model()).add(x.permute(0, 3, 1, 2).float(), gt)
    ev = M.Evaluator(niqe=_model())
    assert ev.niqe is not None and ev.report("none") == M.summarize([], "none")


def test_cli_argument_rules(tmp_path, capsys):
    from vspbfr_amd import restoration_metrics, score
    mu, cov = _model()
    from vspbfr_amd import niqe
    niqe.save_params(tmp_path / "p.npz", mu, cov)
    base = ["--lq_data_list", str(tmp_path), "--hq_data_list", "None", "--data_name_list", "wild"]

    def refused(entry, argv):
        with pytest.raises(SystemExit) as e:
            entry(argv)
        assert e.value.code == 2
        return capsys.readouterr().err

    assert "--niqe_params only has a meaning with --metrics" in refused(restoration_metrics.main, base + ["--niqe_params", str(tmp_path / "p.npz")])
    assert "--metrics needs a ground-truth root (--hq_data_list) for every dataset; none given for: wild" in refused(
        restoration_metrics.main, base + ["--metrics"])
    assert "missing.npz" in refused(restoration_metrics.main, base + ["--metrics", "--niqe_params", str(tmp_path / "missing.npz")])
    assert "--gt is required unless --niqe_params" in refused(score.main, ["--restored", str(tmp_path)])
    assert "need --gt" in refused(score.main, ["--restored", str(tmp_path), "--niqe_params", str(tmp_path / "p.npz"), "--id_weights", "w.pt"])
    assert "no images" in refused(score.main, ["--restored", str(tmp_path), "--niqe_params", str(tmp_path / "p.npz")])
    (tmp_path / "r").mkdir()
    for n in ("0_restore.png", "0_low.png", "1_restore.png"):
        (tmp_path / "r" / n).write_bytes(b"")
    assert [p[0].split("/")[-1] for p in score.restored_files(str(tmp_path / "r"))] == ["0_restore.png", "1_restore.png"]
    assert len(score.restored_files(str(tmp_path / "r"), "_x.png/_y.png")) == 3


def test_entry_refuses_bad_arguments_without_a_gpu():
    import ctypes as C

    from vspbfr_amd import _lib
    from vspbfr_amd import hip_ops as H
    f = (C.c_double * 72)(*([-1.0] * 72))
    s = (C.c_float * 2)(-1.0, -1.0)
    d = C.c_void_p(256)                                            # non-null dummy: never dereferenced on these paths
    call = _lib.lib.vsp_niqe_features_u8
    fp, sp = C.cast(f, C.c_void_p), C.cast(s, C.c_void_p)
    assert call(fp, None, sp, d, 1, 192, 192, -1, d, None, None) == -1 and "crop_border" in _lib.last_error()
    assert call(fp, None, sp, d, 1, 96, 191, 0, d, None, None) == -1 and "fewer than two" in _lib.last_error()
    assert call(fp, None, sp, d, 1, 192, 192, 48, d, None, None) == -1 and "fewer than two" in _lib.last_error()
    for args in ((None, None, sp, d), (fp, None, None, d), (fp, None, sp, None)):
        assert call(*args, 1, 96, 192, 0, d, None, None) == -1 and "null" in _lib.last_error()
    assert call(fp, None, sp, d, 1, 96, 192, 0, None, None, None) == -1 and "null" in _lib.last_error()
    assert list(f) == [-1.0] * 72 and list(s) == [-1.0, -1.0]      # nothing written
    assert _lib.lib.vsp_niqe_work_bytes(8, 512, 512, 0) == 0
    assert H.niqe_blocks(200, 301) == (2, 3) and H.niqe_blocks(200, 301, 5) == (1, 3) and H.niqe_blocks(90, 500) == (0, 5)
    t = H.niqe_gamma_table().numpy()
    assert t.shape == (4, 9801) and np.array_equal(t[0], R.GAM) and np.abs(t[1] / R.R_GAM - 1).max() < 1e-13 and (np.diff(t[1]) > 0).all()
    import torch
    with pytest.raises(RuntimeError, match="CUDA"):
        H.niqe_features_u8(torch.zeros(1, 192, 192, 3, dtype=torch.uint8))
