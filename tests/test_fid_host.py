"""CPU checks of the host side of FID (vspbfr_amd/fid.py, the `fid` entry of vspbfr_amd/metrics.py, the CLI rules) and of the refusals of
the three vsp_fid_* entries, which happen before any launch."""
import json
import os

import numpy as np
import pytest
import torch

import fid_ref as R


def _spd(rng, d, scale=1.0):
    a = rng.standard_normal((d, d))
    return scale * (a @ a.T / d + 0.1 * np.eye(d))


# ---------------------------------------------------------------------------------------------------------------- frechet_distance
def test_identical_statistics_give_zero():
    from vspbfr_amd import fid
    rng = np.random.default_rng(0)
    s = _spd(rng, 24)
    mu = rng.standard_normal(24)
    assert abs(fid.frechet_distance(mu, s, mu, s)) <= 1e-8 * 2 * np.trace(s)


def test_diagonal_covariances_have_a_closed_form():
    from vspbfr_amd import fid
    rng = np.random.default_rng(1)
    a, b = rng.uniform(0.1, 4.0, 32), rng.uniform(0.1, 4.0, 32)
    m1, m2 = rng.standard_normal(32), rng.standard_normal(32)
    want = ((np.sqrt(a) - np.sqrt(b)) ** 2).sum() + ((m1 - m2) ** 2).sum()
    assert abs(fid.frechet_distance(m1, np.diag(a), m2, np.diag(b)) - want) <= 1e-9 * (a.sum() + b.sum())


def test_commuting_covariances_and_the_independent_restatement():
    from vspbfr_amd import fid
    rng = np.random.default_rng(2)
    q, _ = np.linalg.qr(rng.standard_normal((20, 20)))
    a, b = rng.uniform(0.1, 3.0, 20), rng.uniform(0.1, 3.0, 20)
    s1, s2 = (q * a) @ q.T, (q * b) @ q.T                       # one eigenbasis: they commute
    m = rng.standard_normal(20)
    want = ((np.sqrt(a) - np.sqrt(b)) ** 2).sum()
    assert abs(fid.frechet_distance(m, s1, m, s2) - want) <= 1e-9 * (a.sum() + b.sum())
    s1, s2 = _spd(rng, 20), _spd(rng, 20, 2.0)                  # general pair, against the symmetric-form restatement
    m2 = rng.standard_normal(20)
    got, ref = fid.frechet_distance(m, s1, m2, s2), R.frechet_ref(m, s1, m2, s2)
    assert abs(got - ref) <= 1e-8 * (np.trace(s1) + np.trace(s2))
    assert abs(fid.frechet_distance(m2, s2, m, s1) - got) <= 1e-8 * (np.trace(s1) + np.trace(s2))


def test_rank_deficient_pair_takes_the_eps_branch(monkeypatch):
    """two covariances of three samples in 16 dimensions.  scipy's root of the singular product may or may not come out finite, so the
    branch is also driven directly: a first root with a non-finite entry must lead to the root of the eps-shifted product."""
    from scipy import linalg

    from vspbfr_amd import fid
    rng = np.random.default_rng(3)
    f1, f2 = rng.standard_normal((3, 16)), rng.standard_normal((3, 16))
    (m1, s1), (m2, s2) = fid.stats(f1), fid.stats(f2)
    assert np.linalg.matrix_rank(s1) == 2
    got = fid.frechet_distance(m1, s1, m2, s2)
    assert np.isfinite(got) and abs(got - R.frechet_ref(m1, s1, m2, s2)) <= 1e-3 * (np.trace(s1) + np.trace(s2))
    real, calls = linalg.sqrtm, []

    def sqrtm(a, *args, **kw):
        calls.append(a.copy())
        return np.full(a.shape, np.inf) if len(calls) == 1 else real(a, *args, **kw)

    monkeypatch.setattr(linalg, "sqrtm", sqrtm)
    d1, d2 = np.diag(rng.uniform(1.0, 2.0, 6)), np.diag(rng.uniform(1.0, 2.0, 6))
    got = fid.frechet_distance(np.zeros(6), d1, np.zeros(6), d2, eps=1e-6)
    assert len(calls) == 2 and np.allclose(calls[1], (d1 + 1e-6 * np.eye(6)) @ (d2 + 1e-6 * np.eye(6)), rtol=0, atol=1e-15)
    want = ((np.sqrt(np.diag(d1)) - np.sqrt(np.diag(d2))) ** 2).sum()
    assert abs(got - want) <= 1e-4


def test_large_imaginary_part_is_refused_and_a_small_one_dropped(monkeypatch):
    from scipy import linalg

    from vspbfr_amd import fid
    s = np.eye(4)
    monkeypatch.setattr(linalg, "sqrtm", lambda a, *k, **kw: np.eye(4) * (1 + 0.5j))
    with pytest.raises(ValueError, match="imaginary component"):
        fid.frechet_distance(np.zeros(4), s, np.zeros(4), s)
    monkeypatch.setattr(linalg, "sqrtm", lambda a, *k, **kw: np.eye(4) * (1 + 1e-5j))
    assert abs(fid.frechet_distance(np.zeros(4), s, np.zeros(4), s)) <= 1e-12
    with pytest.raises(ValueError, match="dimensions"):
        fid.frechet_distance(np.zeros(4), s, np.zeros(3), np.eye(3))
    with pytest.raises(ValueError, match="expected"):
        fid.frechet_distance(np.zeros(4), np.eye(3), np.zeros(4), s)


def test_stats_is_mean_and_unbiased_covariance():
    from vspbfr_amd import fid
    rng = np.random.default_rng(4)
    f = rng.standard_normal((7, 12)).astype(np.float32)
    mu, sigma = fid.stats(torch.from_numpy(f))
    rmu, rsigma = R.stats_ref(f)
    assert mu.dtype == np.float64 and np.abs(mu - rmu).max() <= 1e-14 and np.abs(sigma - rsigma).max() <= 1e-14
    assert np.abs(sigma - np.cov(f.astype(np.float64), rowvar=False)).max() <= 1e-15
    with pytest.raises(ValueError, match="at least 2"):
        fid.stats(f[:1])
    g = f.copy()
    g[2, 3] = np.nan
    with pytest.raises(ValueError, match="not finite"):
        fid.stats(g)


def test_statistics_files_of_both_formats_and_their_refusals(tmp_path):
    from vspbfr_amd import fid
    rng = np.random.default_rng(5)
    mu, sigma = rng.standard_normal(2048), _spd(rng, 8)
    big = np.zeros((2048, 2048))
    big[:8, :8] = sigma
    for name in ("s.npz", "s.pth"):
        p = str(tmp_path / name)
        fid.save_stats(p, mu, big)
        m, s = fid.load_stats(p)
        assert m.dtype == np.float64 and np.array_equal(m, mu) and np.array_equal(s, big)
    # the layout of the widely used torch file: a dict with the two names, float32 tensors or arrays
    torch.save({"mu": mu.astype(np.float32), "sigma": torch.from_numpy(big).float()}, str(tmp_path / "t.pth"))
    m, s = fid.load_stats(str(tmp_path / "t.pth"))
    assert np.array_equal(m, mu.astype(np.float32).astype(np.float64)) and s.shape == (2048, 2048)
    np.savez(str(tmp_path / "small.npz"), mu=mu[:8], sigma=sigma)
    assert fid.load_stats(str(tmp_path / "small.npz"), dims=None)[1].shape == (8, 8)
    with pytest.raises(ValueError, match="dimension 8, expected 2048"):
        fid.load_stats(str(tmp_path / "small.npz"))
    np.savez(str(tmp_path / "bad.npz"), mu=mu[:8], sigma=sigma[:7])
    with pytest.raises(ValueError, match="expected"):
        fid.load_stats(str(tmp_path / "bad.npz"), dims=None)
    np.savez(str(tmp_path / "names.npz"), m=mu, s=big)
    with pytest.raises(ValueError, match="mu and sigma"):
        fid.load_stats(str(tmp_path / "names.npz"))
    torch.save([1, 2], str(tmp_path / "list.pth"))
    with pytest.raises(ValueError, match="a dict with mu and sigma"):
        fid.load_stats(str(tmp_path / "list.pth"))


# ------------------------------------------------------------------------------------------------------------- reports and merging
def _rows(idx):
    return [{"index": i, "lq": f"a{i}.png", "hq": f"b{i}.png", "sse": 100 + i, "psnr": 30.0 + i, "ssim": 0.5 + 0.01 * i} for i in idx]


def _rank(tmp_path, rank, idx, feats, gt_feats=None, ref_stats=None, ref=None, with_fid=True):
    from vspbfr_amd import metrics as M
    rep = M.summarize(_rows(idx), "set", "gauss11")
    path = str(tmp_path / f"metrics_{rank}.json")
    if with_fid:
        rep["fid"] = M.fid_entry(feats, gt_feats, ref_stats, ref)
        M.write_fid_features(M.fid_feature_path(path), idx, feats)
        if gt_feats is not None:
            M.write_fid_features(M.fid_feature_path(path, gt=True), idx, gt_feats)
    M.write_report(rep, path)
    return path, rep


def test_reports_without_fid_are_what_they_were(tmp_path):
    """a report without `fid` has the keys it always had, merges as it did, and its summary line has no fid part"""
    from vspbfr_amd import metrics as M
    p0, r0 = _rank(tmp_path, 0, [0, 2], None, with_fid=False)
    p1, r1 = _rank(tmp_path, 1, [1, 3], None, with_fid=False)
    assert list(r0) == ["dataset", "count", "window", "psnr_infinite", "mean", "images"]
    merged = M.merge_reports([p0, p1])
    want = M.summarize(_rows([0, 1, 2, 3]), "set", "gauss11")
    assert json.dumps(merged, indent=1) == json.dumps(want, indent=1)
    assert "fid" not in M.summary_line(merged)
    assert not [f for f in os.listdir(tmp_path) if f.startswith("fid_features")]


def test_merge_recomputes_fid_from_the_feature_files(tmp_path):
    from vspbfr_amd import fid
    from vspbfr_amd import metrics as M
    rng = np.random.default_rng(6)
    feats = rng.standard_normal((6, 32)).astype(np.float32)
    gts = rng.standard_normal((6, 32)).astype(np.float32)
    # against ground truth: ranks hold interleaved indices, rank 1's rows out of order on disk
    p0, r0 = _rank(tmp_path, 0, [0, 2, 4], feats[[0, 2, 4]], gts[[0, 2, 4]])
    p1, r1 = _rank(tmp_path, 1, [5, 1, 3], feats[[5, 1, 3]], gts[[5, 1, 3]])
    assert r0["fid"]["against"] == "gt" and r0["fid"]["ref"] is None and r0["fid"]["count"] == 3
    merged = M.merge_reports([p0, p1])
    want = fid.frechet_distance(*fid.stats(feats), *fid.stats(gts))
    assert merged["fid"] == {"value": merged["fid"]["value"], "count": 6, "against": "gt", "ref": None}
    assert abs(merged["fid"]["value"] - want) <= 1e-12 * max(1.0, abs(want))
    assert [r["index"] for r in merged["images"]] == list(range(6))
    assert ("fid %.6g" % merged["fid"]["value"]) in M.summary_line(merged) and M.summary_line(merged).endswith("fid %.6g" % merged["fid"]["value"])
    idx, f = M.read_fid_features(M.fid_feature_path(p1))
    assert idx.tolist() == [5, 1, 3] and f.dtype == np.float32 and np.array_equal(f, feats[[5, 1, 3]])
    assert os.path.basename(M.fid_feature_path(p1)) == "fid_features_1.npy" and os.path.basename(M.fid_feature_path(p1, True)) == "fid_features_1_gt.npy"
    # against statistics
    sub = tmp_path / "stats"
    sub.mkdir()
    ref = str(sub / "ref.npz")
    fid.save_stats(ref, *fid.stats(gts))
    rs = fid.load_stats(ref, dims=None)
    q0, _ = _rank(sub, 0, [0, 1, 2], feats[:3], None, rs, ref)
    q1, s1 = _rank(sub, 1, [3, 4, 5], feats[3:], None, rs, ref)
    assert s1["fid"]["against"] == "stats" and s1["fid"]["ref"] == ref
    merged = M.merge_reports([q0, q1])
    assert merged["fid"]["against"] == "stats" and abs(merged["fid"]["value"] - want) <= 1e-9 * max(1.0, abs(want))
    # one image: no covariance, the value is null
    assert M.fid_entry(feats[:1], None, rs, ref) == {"value": None, "count": 1, "against": "stats", "ref": ref}


def test_merge_refuses_a_mixture_and_a_missing_feature_file(tmp_path):
    from vspbfr_amd import metrics as M
    rng = np.random.default_rng(7)
    feats = rng.standard_normal((4, 32)).astype(np.float32)
    p0, _ = _rank(tmp_path, 0, [0, 1], feats[:2], feats[2:])
    p1, _ = _rank(tmp_path, 1, [2, 3], None, with_fid=False)
    with pytest.raises(ValueError, match="some files have a fid entry and some have none"):
        M.merge_reports([p0, p1])
    p1, _ = _rank(tmp_path, 1, [2, 3], feats[2:], feats[:2])
    M.merge_reports([p0, p1])
    os.remove(M.fid_feature_path(p1, gt=True))
    with pytest.raises(ValueError, match="fid_features_1_gt.npy is missing"):
        M.merge_reports([p0, p1])
    M.write_fid_features(M.fid_feature_path(p1, gt=True), [2, 7], feats[:2])
    with pytest.raises(ValueError, match="does not hold the images"):
        M.merge_reports([p0, p1])


def test_evaluator_argument_rules():
    from vspbfr_amd.metrics import Evaluator
    with pytest.raises(ValueError, match="fid takes"):
        Evaluator(fid="net")
    ev = Evaluator(fid=(object(), None))
    with pytest.raises(RuntimeError, match="measured against the ground truth"):
        ev.add(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), None)
    with pytest.raises(RuntimeError, match="scores NIQE only"):
        Evaluator().add(torch.zeros((1, 8, 8, 3), dtype=torch.uint8), None)


# ----------------------------------------------------------------------------------------------------------------------- CLI rules
@pytest.mark.parametrize("argv,msg", [
    (["--restored", "d", "--fid_stats", "s.npz"], "--fid_stats only has a meaning with --fid_weights"),
    (["--restored", "d", "--fid_weights", "w.pth"], "it needs --gt"),
    (["--restored", "d"], "--gt is required"),
    (["--restored", "d", "--fid_weights", "w.pth", "--fid_stats", "/nonexistent/s.npz"], "s.npz"),
])
def test_score_argument_rules(argv, msg, capsys):
    from vspbfr_amd import score
    with pytest.raises(SystemExit) as e:
        score.main(argv)
    assert e.value.code == 2 and msg in capsys.readouterr().err


@pytest.mark.parametrize("argv,msg", [
    (["--fid_weights", "w.pth"], "only have a meaning with --metrics"),
    (["--metrics", "--fid_stats", "s.npz"], "--fid_stats only has a meaning with --fid_weights"),
    (["--metrics", "--fid_weights", "w.pth", "--lq_data_list", "a", "--hq_data_list", "None", "--data_name_list", "n"], "measures against ground truth"),
])
def test_restoration_metrics_argument_rules(argv, msg, capsys):
    from vspbfr_amd import restoration_metrics
    with pytest.raises(SystemExit) as e:
        restoration_metrics.main(argv)
    assert e.value.code == 2 and msg in capsys.readouterr().err


@pytest.mark.parametrize("argv", [["--images", "d", "--weights", "w"], ["--images", "d", "--weights", "w", "--stats", "s", "--ref_images", "r"],
                                  ["--images", "d", "--weights", "w", "--stats", "s", "--batch", "0"], ["--weights", "w", "--stats", "s"]])
def test_fid_cli_argument_rules(argv):
    from vspbfr_amd import fid
    with pytest.raises(SystemExit) as e:
        fid.parse_args(argv)
    assert e.value.code == 2
    assert fid.parse_args(["--images", "d", "--weights", "w", "--stats", "s"]).batch == 16


# ----------------------------------------------------------------------------------------------------- refusals without a GPU
A, B_, C_, D_ = 4096, 1 << 20, 1 << 21, 1 << 22                  # non-null, 16-byte aligned, far apart: never dereferenced


def _conv(**kw):
    from vspbfr_amd import _lib
    a = dict(out=A, x=B_, w=C_, bias=D_, B=1, H=8, W=8, Cin=32, x_pitch=32, Cout=48, KH=3, KW=3, ph=1, pw=1, stride=1, c_off=0, c_pitch=48)
    a.update(kw)
    rc = _lib.lib.vsp_fid_conv_f32(a["out"], a["x"], a["w"], a["bias"], a["B"], a["H"], a["W"], a["Cin"], a["x_pitch"], a["Cout"], a["KH"],
                                   a["KW"], a["ph"], a["pw"], a["stride"], a["c_off"], a["c_pitch"], None)
    return rc, _lib.last_error()


@pytest.mark.parametrize("kw,code,msg", [
    (dict(out=None), -1, "null pointer"), (dict(x=None), -1, "null pointer"), (dict(w=None), -1, "null pointer"), (dict(bias=None), -1, "null pointer"),
    (dict(Cin=24, x_pitch=24), -1, "multiples of 16"), (dict(Cout=40), -1, "multiples of 16"), (dict(Cin=0, x_pitch=0), -1, "multiples of 16"),
    (dict(KH=7, KW=7, ph=3, pw=3), -1, "filter 7 x 7"), (dict(KH=3, KW=5), -1, "filter 3 x 5"), (dict(KH=2, KW=2), -1, "filter 2 x 2"),
    (dict(stride=3), -1, "stride 3"), (dict(stride=0), -1, "stride 0"),
    (dict(ph=3), -1, "padding 3 x 1"), (dict(KH=1, KW=7, ph=1, pw=3), -1, "padding 1 x 3"), (dict(pw=-1), -1, "padding"),
    (dict(H=2, W=2, ph=0, pw=0), -1, "the output is empty"), (dict(H=0), -1, "map 0 x 8"),
    (dict(c_off=16, c_pitch=48), -1, "output pitch 48 < offset 16 + 48"), (dict(c_pitch=32), -1, "output pitch"),
    (dict(x_pitch=16), -1, "input pitch 16"), (dict(c_off=2, c_pitch=64), -1, "multiple of 4"),
    (dict(out=A + 4), -1, "16-byte aligned"), (dict(x=B_ + 8), -1, "16-byte aligned"), (dict(w=C_ + 4), -1, "16-byte aligned"),
    (dict(x=A + 1024), -1, "overlaps"), (dict(out=B_ + 4096), -1, "overlaps"),
    (dict(B=4096, H=512, W=512), -3, "2 GiB"), (dict(B=1024, H=1024, W=1024, Cin=16, x_pitch=16, Cout=16, c_pitch=16), -3, "2 GiB"),
])
def test_conv_refusals(kw, code, msg):
    rc, err = _conv(**kw)
    assert rc == code and msg in err, (rc, err)


def test_conv_accepts_nothing_to_do():
    """B = 0 returns VSP_OK before any pointer is looked at"""
    assert _conv(B=0)[0] == 0
    from vspbfr_amd import _lib
    assert _lib.lib.vsp_fid_conv_f32(None, None, None, None, 0, 8, 8, 32, 32, 48, 3, 3, 1, 1, 1, 0, 48, None) == 0


def _pool(**kw):
    from vspbfr_amd import _lib
    a = dict(out=A, x=B_, B=1, H=8, W=8, C=32, x_pitch=32, mode=1, c_off=0, c_pitch=32)
    a.update(kw)
    rc = _lib.lib.vsp_fid_pool_f32(a["out"], a["x"], a["B"], a["H"], a["W"], a["C"], a["x_pitch"], a["mode"], a["c_off"], a["c_pitch"], None)
    return rc, _lib.last_error()


@pytest.mark.parametrize("kw,code,msg", [
    (dict(out=None), -1, "null pointer"), (dict(x=None), -1, "null pointer"), (dict(mode=4), -1, "mode 4"), (dict(mode=-1), -1, "mode -1"),
    (dict(C=24), -1, "multiples of 16"), (dict(mode=0, H=2), -1, "the output is empty"), (dict(c_pitch=16), -1, "output pitch"),
    (dict(c_off=16), -1, "output pitch 32 < offset 16 + 32"), (dict(x_pitch=16), -1, "input pitch"), (dict(out=A + 8), -1, "16-byte aligned"),
    (dict(x=A + 64), -1, "overlaps"), (dict(B=1 << 14, H=256, W=256), -3, "2 GiB"),
])
def test_pool_refusals(kw, code, msg):
    rc, err = _pool(**kw)
    assert rc == code and msg in err, (rc, err)
    assert _pool(B=0)[0] == 0


def test_stem_refusals():
    import ctypes as C

    from vspbfr_amd import _lib
    items = (_lib.DetSrc * 2)()
    for i in range(2):
        items[i].off, items[i].h, items[i].w, items[i].slot = i * 300, 10, 10, i
    ip = C.cast(items, C.c_void_p)

    def stem(y=A, src=B_, src_bytes=600, it=ip, it_dev=C_, n=2, B=2, TH=299, TW=299, w=D_, b=D_ + 4096):
        return _lib.lib.vsp_fid_stem_u8(y, src, src_bytes, it, it_dev, n, B, TH, TW, w, b, None), _lib.last_error()

    for kw, code, msg in ((dict(y=None), -1, "null pointer"), (dict(src=None), -1, "null pointer"), (dict(it=None), -1, "null pointer"),
                          (dict(it_dev=None), -1, "null pointer"), (dict(w=None), -1, "null pointer"), (dict(b=None), -1, "null pointer"),
                          (dict(n=3), -1, "3 items for a batch of 2"), (dict(TH=2), -1, "target 2 x 299"), (dict(y=A + 4), -1, "16-byte aligned"),
                          (dict(src_bytes=599), -1, "item 1: bytes outside src"), (dict(B=2, n=2, src_bytes=1 << 31), -3, "2 GiB"),
                          (dict(B=40000, TH=299, TW=299), -3, "2 GiB"), (dict(src=A + 64, y=A), -1, "overlaps")):
        rc, err = stem(**kw)
        assert rc == code and msg in err, (kw, rc, err)
    items[1].slot = 2
    rc, err = stem()
    assert rc == -1 and "slot 2 outside 0..1" in err
    items[1].slot, items[1].h = 1, 0
    rc, err = stem()
    assert rc == -1 and "image 0 x 10" in err
    assert stem(n=0)[0] == 0


def test_wrappers_refuse_before_the_library():
    from vspbfr_amd import hip_ops as H
    t = torch.zeros(64)
    with pytest.raises(RuntimeError, match="CUDA tensor"):
        H.fid_pool_f32((t, 0, 16), (t, 0, 16), 1, 2, 2, 16, H.FID_POOL_AVG_S1)
    assert H.fid_conv_out(299, 299, 3, 3, 0, 0, 2) == (149, 149) and H.fid_conv_out(17, 17, 1, 7, 0, 3, 1) == (17, 17)
    assert H.fid_pool_out(147, 147, H.FID_POOL_MAX_S2) == (73, 73) and H.fid_pool_out(8, 8, H.FID_POOL_GLOBAL_AVG) == (1, 1)
    assert H.FID_FILTERS == ((1, 1), (3, 3), (5, 5), (1, 7), (7, 1), (1, 3), (3, 1))
