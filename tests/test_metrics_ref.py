"""CPU: the float64 oracle of the pixel metrics (tests/metrics_ref.py) on cases with closed forms, and the host side of
vspbfr_amd.metrics / vspbfr_amd.score / the --metrics flags of vspbfr_amd.restoration_metrics (reports, merging, file pairing, refusals)."""
import json
import math

import numpy as np
import pytest

import metrics_ref as R

WINDOWS = ("uniform7", "gauss11")


def test_gauss_taps():
    t = R.gauss_taps()
    assert t.shape == (11,) and abs(t.sum() - 1.0) < 1e-15 and np.array_equal(t, t[::-1])
    assert abs(t[5] / t[4] - math.exp(1.0 / 4.5)) < 1e-14          # exp(-d^2 / (2 * 1.5^2))


@pytest.mark.parametrize("window", WINDOWS)
def test_identical_images(window):
    a, b = R.pair("identical", 40, 52)
    assert R.sse(a, b) == 0 and R.psnr(a, b) is None
    assert abs(R.ssim(a, b, window) - 1.0) < 1e-12


@pytest.mark.parametrize("window", WINDOWS)
@pytest.mark.parametrize("p,q", [(0, 255), (10, 200), (230, 231), (128, 128)])
def test_constant_images_closed_form(window, p, q):
    """Variances and covariance vanish: S = (2 p q + C1) / (p^2 + q^2 + C1) at every position, for both windows."""
    a, b = np.full((19, 23, 3), p, np.uint8), np.full((19, 23, 3), q, np.uint8)
    want = (2.0 * p * q + R.C1) / (p * p + q * q + R.C1)
    assert abs(R.ssim(a, b, window) - want) < 1e-9              # the filters' own rounding on the constant 255^2 plane
    assert R.sse(a, b) == (p - q) ** 2 * a.size
    if p != q:
        assert abs(R.psnr(a, b) - 20.0 * math.log10(255.0 / abs(p - q))) < 1e-12


@pytest.mark.parametrize("window", WINDOWS)
def test_negative_image(window):
    """y = 255 - x: vy = vx, vxy = -vx, uy = 255 - ux, so S = (2 ux (255 - ux) + C1)(C2 - 2 vx) / ((ux^2 + (255 - ux)^2 + C1)(2 vx + C2))
    from the statistics of x alone."""
    a, b = R.pair("negative", 33, 47, c=1)
    x = a[..., 0].astype(np.float64)
    w, k = R.WIN[window], (49.0 / 48.0 if window == "uniform7" else 1.0)
    taps = np.full(7, 1.0 / 7.0) if window == "uniform7" else R.gauss_taps()
    win = np.lib.stride_tricks.sliding_window_view(x, (w, w))
    w2 = np.outer(taps, taps)
    ux = (win * w2).sum((-1, -2))
    vx = k * ((win * win * w2).sum((-1, -2)) - ux * ux)
    s = ((2 * ux * (255 - ux) + R.C1) * (R.C2 - 2 * vx)) / ((ux * ux + (255 - ux) ** 2 + R.C1) * (2 * vx + R.C2))
    assert s.shape == (33 - w + 1, 47 - w + 1)
    assert abs(R.ssim(a, b, window) - s.mean()) < 1e-10
    assert R.ssim(a, b, window) < 0.0


@pytest.mark.parametrize("window", WINDOWS)
def test_border_mode_does_not_matter(window):
    """Only positions whose window lies inside the image count, so the filter's treatment of the border is irrelevant."""
    a, b = R.pair("smooth", 31, 45)
    vals = [R.ssim(a, b, window, mode) for mode in ("reflect", "constant", "nearest", "wrap")]
    assert max(vals) - min(vals) < 1e-12
    assert R.ssim_map(a[..., 0], b[..., 0], window).shape == (31 - R.WIN[window] + 1, 45 - R.WIN[window] + 1)


@pytest.mark.parametrize("window", WINDOWS)
def test_channel_mean_and_direct_window_sum(window):
    a, b = R.pair("noise", 24, 29)
    per = [R.ssim(a[..., c], b[..., c], window) for c in range(3)]
    assert abs(R.ssim(a, b, window) - np.mean(per)) < 1e-15
    # one position computed directly from its window
    w, k = R.WIN[window], (49.0 / 48.0 if window == "uniform7" else 1.0)
    taps = np.full(7, 1.0 / 7.0) if window == "uniform7" else R.gauss_taps()
    w2 = np.outer(taps, taps)
    x, y = a[3:3 + w, 5:5 + w, 1].astype(np.float64), b[3:3 + w, 5:5 + w, 1].astype(np.float64)
    ux, uy = (w2 * x).sum(), (w2 * y).sum()
    vx, vy, vxy = k * ((w2 * x * x).sum() - ux * ux), k * ((w2 * y * y).sum() - uy * uy), k * ((w2 * x * y).sum() - ux * uy)
    s = ((2 * ux * uy + R.C1) * (2 * vxy + R.C2)) / ((ux * ux + uy * uy + R.C1) * (vx + vy + R.C2))
    assert abs(R.ssim_map(a[..., 1], b[..., 1], window)[3, 5] - s) < 1e-11


def test_single_window_image():
    a, b = R.pair("noise", 7, 7)
    assert R.ssim_map(a[..., 0], b[..., 0], "uniform7").shape == (1, 1)
    with pytest.raises(ValueError):
        R.ssim_map(a[..., 0], b[..., 0], "gauss11")


def test_naive_fp32_form_loses_digits_on_the_bright_flat_pair():
    """The reason the kernel keeps the box sums in integers and centres the Gaussian moments: uncentred fp32 moments cancel."""
    a, b = R.pair("bright_flat", 128, 128)
    assert 225 < a.mean() < 235
    for window in WINDOWS:
        assert abs(R.ssim_fp32_naive(a, b, window) - R.ssim(a, b, window)) > 2e-6
    a, b = R.pair("noise", 128, 128)
    assert abs(R.ssim_fp32_naive(a, b, "gauss11") - R.ssim(a, b, "gauss11")) < 2e-6


# ------------------------------------------------------------------------------------------------ host side of the package
def _rows():
    return [{"index": 2, "lq": "c.png", "hq": "c.png", "sse": 0, "psnr": None, "ssim": 1.0},
            {"index": 0, "lq": "a.png", "hq": "a.png", "sse": 100, "psnr": 30.0, "ssim": 0.5, "lpips": 0.25},
            {"index": 1, "lq": "b.png", "hq": "b.png", "sse": 400, "psnr": 20.0, "ssim": 0.75, "lpips": 0.75}]


def test_psnr_from_sse():
    from vspbfr_amd import metrics as M
    assert M.psnr_from_sse(0, 100) is None
    assert M.psnr_from_sse(100, 100) == pytest.approx(20.0 * math.log10(255.0), abs=1e-12)
    a, b = R.pair("smooth", 20, 20)
    assert M.psnr_from_sse(R.sse(a, b), a.size) == pytest.approx(R.psnr(a, b), abs=1e-12)


def test_report_and_null_psnr(tmp_path):
    from vspbfr_amd import metrics as M
    rep = M.summarize(_rows(), "demo", "uniform7")
    assert [r["index"] for r in rep["images"]] == [0, 1, 2]
    assert rep["count"] == 3 and rep["psnr_infinite"] == 1 and rep["dataset"] == "demo" and rep["window"] == "uniform7"
    assert rep["mean"]["psnr"] == 25.0 and rep["mean"]["ssim"] == 0.75 and rep["mean"]["lpips"] == 0.5 and "id" not in rep["mean"]
    M.write_report(rep, tmp_path / "m.json")
    text = (tmp_path / "m.json").read_text()
    assert '"psnr": null' in text and "Infinity" not in text and "NaN" not in text
    assert json.loads(text) == rep
    only = M.summarize([_rows()[0]], "demo")
    assert only["mean"]["psnr"] is None and only["psnr_infinite"] == 1
    assert "psnr n/a" in M.summary_line(only) and "ssim 0.75" in M.summary_line(rep)


def test_merge_reports(tmp_path):
    from vspbfr_amd import metrics as M
    rows = _rows()
    M.write_report(M.summarize(rows[:1], "demo", "gauss11"), tmp_path / "metrics_1.json")
    M.write_report(M.summarize(rows[1:], "demo", "gauss11"), tmp_path / "metrics_0.json")
    merged = M.merge_reports([tmp_path / "metrics_0.json", tmp_path / "metrics_1.json"])
    assert merged == M.summarize(rows, "demo", "gauss11")
    M.write_report(M.summarize(rows[1:], "demo", "uniform7"), tmp_path / "other.json")
    with pytest.raises(ValueError, match="window"):
        M.merge_reports([tmp_path / "metrics_1.json", tmp_path / "other.json"])
    with pytest.raises(ValueError, match="more than once"):
        M.merge_reports([tmp_path / "metrics_0.json", tmp_path / "metrics_0.json"])
    with pytest.raises(ValueError):
        M.merge_reports([])


def test_evaluator_and_psnr_ssim_refuse_bad_operands():
    import torch
    from vspbfr_amd import hip_ops as H
    from vspbfr_amd import metrics as M
    with pytest.raises(ValueError, match="window"):
        M.Evaluator(window="box3")
    u = torch.zeros(1, 16, 16, 3, dtype=torch.uint8)
    with pytest.raises(RuntimeError, match="CUDA"):
        H.pair_stats_u8(u, u, "gauss11")
    with pytest.raises(RuntimeError, match="uint8"):
        M.Evaluator().add(torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 16, 16))
    with pytest.raises(RuntimeError, match="differ"):
        M.psnr_ssim(u, torch.zeros(1, 16, 17, 3, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match=r"\(B, H, W, 3\)"):
        M.psnr_ssim(torch.zeros(1, 3, 16, 16, dtype=torch.uint8), torch.zeros(1, 3, 16, 16, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="float32"):
        M.psnr_ssim(u.double(), u.double())


def test_kernel_entry_refuses_without_a_gpu():
    """Argument checks of vsp_pair_stats_u8 come before any device work."""
    from vspbfr_amd import _lib
    f, wb = _lib.lib.vsp_pair_stats_u8, _lib.lib.vsp_pair_stats_work_bytes
    assert f(256, 256, 256, 256, 1, 6, 16, 3, _lib.WIN_UNIFORM7, 256, None) == -1 and "smaller than" in _lib.last_error()
    assert f(256, 256, 256, 256, 1, 16, 10, 3, _lib.WIN_GAUSS11, 256, None) == -1 and "smaller than" in _lib.last_error()
    assert f(256, 256, 256, 256, 1, 16, 16, 2, _lib.WIN_GAUSS11, 256, None) == -1 and "C must be 1 or 3" in _lib.last_error()
    assert f(256, 256, 256, 256, 1, 16, 16, 3, 9, 256, None) == -1 and "window" in _lib.last_error()
    assert f(None, 256, 256, 256, 1, 16, 16, 3, _lib.WIN_GAUSS11, 256, None) == -1 and "null pointer" in _lib.last_error()
    assert f(256, 256, 256, 256, 1, 16, 16, 3, _lib.WIN_GAUSS11, None, None) == -1 and "null pointer" in _lib.last_error()
    assert wb(1, 6, 16, 3, 7) == 0 and wb(1, 16, 16, 2, 7) == 0
    assert wb(5, 512, 512, 3, 11) == 5 * 16 * 16 * 16                 # ceil(502 / 32)^2 tiles, 16 bytes each
    assert wb(2, 7, 7, 1, 7) == 2 * 16


def test_score_file_pairing(tmp_path):
    from vspbfr_amd.score import pair_files
    d = tmp_path / "out"
    d.mkdir()
    for i in range(3):
        for kind in ("restore", "low", "gt"):
            (d / f"{i:06d}_0_demo_{kind}.png").write_bytes(b"")
    pairs = pair_files(str(d), str(d))
    assert [(p.split("/")[-1], q.split("/")[-1]) for p, q in pairs] == [
        (f"{i:06d}_0_demo_restore.png", f"{i:06d}_0_demo_gt.png") for i in range(3)]
    (d / "000001_0_demo_gt.png").unlink()
    with pytest.raises(FileNotFoundError):
        pair_files(str(d), str(d))
    # other methods' folders: no suffix -> sorted order
    ra, ga = tmp_path / "theirs", tmp_path / "truth"
    ra.mkdir()
    ga.mkdir()
    for n in ("b.png", "a.png"):
        (ra / n).write_bytes(b"")
    for n in ("y.png", "x.png"):
        (ga / n).write_bytes(b"")
    assert [(p.split("/")[-1], q.split("/")[-1]) for p, q in pair_files(str(ra), str(ga))] == [("a.png", "x.png"), ("b.png", "y.png")]
    (ga / "z.png").write_bytes(b"")
    with pytest.raises(ValueError, match="sorted order"):
        pair_files(str(ra), str(ga))
    with pytest.raises(ValueError, match="same folder"):
        pair_files(str(ra), str(ra))
    with pytest.raises(ValueError, match="pattern"):
        pair_files(str(ra), str(ga), "_restore.png")
    # a custom suffix pair
    (ra / "a.png").rename(ra / "a_out.png")
    (ga / "a.png").write_bytes(b"")
    assert pair_files(str(ra), str(ga), "_out.png/.png") == [(str(ra / "a_out.png"), str(ga / "a.png"))]


def test_cli_refusals(capsys, tmp_path):
    """--metrics without a ground-truth root is refused before anything is loaded; the weight flags need --metrics."""
    from vspbfr_amd import restoration_metrics as cli
    from vspbfr_amd import score
    base = ["--lq_data_list", "lqA,lqB", "--data_name_list", "a,b"]
    with pytest.raises(SystemExit) as e:
        cli.main(base + ["--hq_data_list", "hqA,None", "--metrics"])
    assert e.value.code == 2
    err = capsys.readouterr().err
    assert "ground-truth root" in err and ": b" in err
    with pytest.raises(SystemExit):
        cli.main(base + ["--metrics"])                                   # no --hq_data_list at all
    assert "ground-truth root" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(base + ["--hq_data_list", "hqA,hqB", "--id_weights", "w.pt"])
    assert "--metrics" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        cli.main(base + ["--hq_data_list", "hqA,hqB", "--metrics", "--ssim_window", "box3"])
    assert "box3" in capsys.readouterr().err
    with pytest.raises(SystemExit):
        score.main(["--restored", str(tmp_path / "a"), "--gt", str(tmp_path / "b")])
    assert "cannot pair" in capsys.readouterr().err
