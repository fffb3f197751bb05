"""GPU, end to end: `python -m vspbfr_amd.restoration_metrics --metrics` (the inference CLI with scoring) scores the bytes it writes.
The rows of metrics_0.json are compared with what the float64 oracle (tests/metrics_ref.py) computes from the *_restore.png / *_gt.png
files read back from disk; `python -m vspbfr_amd.score` on that directory gives the same numbers bit for bit; the same call without
--metrics, and `vspbfr_amd.restoration_test` itself, write the same PNG bytes and no report; the learned columns of an Evaluator equal
direct calls of the existing modules."""
import json
import os
import random
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

import metrics_ref as R

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cli_run(tmp_path_factory):
    """Three synthetic checkpoints (as tests/test_cli_gpu.py builds them), 3 LQ + 3 HQ files of mixed sizes, one run of
    `restoration_test`, and of `restoration_metrics` without and with --metrics, from the same seeds."""
    from PIL import Image
    from scipy import ndimage
    from vspbfr_amd import restoration_metrics, restoration_test as cli
    from vspbfr_amd.diffusion import Code_diffuser
    from vspbfr_amd.e4e import Encoder4Editing, Generator
    from vspbfr_amd.restorenet import Restoration_net
    tmp = tmp_path_factory.mktemp("metrics_cli")
    torch.manual_seed(0)
    ck = tmp / "ckpt"
    ck.mkdir()
    torch.save({"g_ema": Restoration_net(512, 512, 8).state_dict()}, ck / "restoration_net.pt")
    torch.save({"att_mapper": Code_diffuser(timesteps=4).state_dict()}, ck / "code_diffuser.pt")
    enc = Encoder4Editing(50, "ir_se", Namespace(input_channel=3, stylegan_size=1024))
    dec = Generator(1024, 512, 8)
    sd = {"encoder." + k: v for k, v in enc.state_dict().items()}
    sd.update({"decoder." + k: v for k, v in dec.state_dict().items()})
    torch.save({"state_dict": sd, "latent_avg": torch.zeros(18, 512),
                "opts": {"encoder_type": "Encoder4Editing", "stylegan_size": 1024, "start_from_latent_avg": True}},
               ck / "style_encoder_decoder.pt")
    lq, hq = tmp / "lq", tmp / "hq"
    lq.mkdir()
    hq.mkdir()
    rng = np.random.default_rng(1)
    for i, (w, h) in enumerate([(512, 512), (640, 600), (300, 400)]):
        sharp = ndimage.gaussian_filter(rng.integers(0, 256, (h, w, 3)).astype(np.float64), (3, 3, 0)) * 4 - 384
        sharp = np.clip(sharp, 0, 255)
        Image.fromarray(sharp.astype(np.uint8)).save(hq / f"face_{i}.png")
        Image.fromarray(np.clip(ndimage.gaussian_filter(sharp, (4, 4, 0)) + rng.normal(0, 5, sharp.shape), 0, 255).astype(np.uint8)).save(
            lq / f"face_{i}.png")
    runs = {}
    for tag, entry, extra in (("reference_cli", cli.main, []), ("plain", restoration_metrics.main, []),
                              ("metrics", restoration_metrics.main, ["--metrics"])):
        torch.manual_seed(123)
        random.seed(123)
        out = tmp / f"eval_{tag}"
        entry(["--batch", "2", "--ckpt", str(ck / "restoration_net.pt"), "--ddpm_ckpt", str(ck / "code_diffuser.pt"),
                  "--psp_checkpoint_path", str(ck / "style_encoder_decoder.pt"), "--eval_dir", str(out), "--timesteps", "4", "--no_sample",
                  "--lq_data_list", str(lq), "--hq_data_list", str(hq), "--data_name_list", "demo"] + extra)
        runs[tag] = out / "restoration_net" / "0" / "demo"
    return runs


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def test_without_the_flag_nothing_changes(cli_run):
    ref, plain, scored = cli_run["reference_cli"], cli_run["plain"], cli_run["metrics"]
    pngs = sorted(f"{i:06d}_0_demo_{k}.png" for i in range(3) for k in ("restore", "low", "gt"))
    assert sorted(os.listdir(ref)) == pngs and sorted(os.listdir(plain)) == pngs
    assert sorted(os.listdir(scored)) == sorted(pngs + ["metrics_0.json"])
    for n in pngs:
        assert (ref / n).read_bytes() == (plain / n).read_bytes() == (scored / n).read_bytes(), n


def test_report_rows_equal_the_oracle_on_the_files(cli_run):
    d = cli_run["metrics"]
    rep = json.loads((d / "metrics_0.json").read_text())
    assert rep["dataset"] == "demo" and rep["count"] == 3 and rep["window"] == "gauss11" and rep["psnr_infinite"] == 0
    assert [r["index"] for r in rep["images"]] == [0, 1, 2]
    assert [(r["lq"], r["hq"]) for r in rep["images"]] == [(f"face_{i}.png", f"face_{i}.png") for i in range(3)]
    for i, row in enumerate(rep["images"]):
        a, b = _png(d / f"{i:06d}_0_demo_restore.png"), _png(d / f"{i:06d}_0_demo_gt.png")
        ref = R.ssim(a, b, "gauss11")
        e_ref = abs(R.ssim_fp32_naive(a, b, "gauss11") - ref)
        print(f"image {i}: sse {row['sse']} psnr {row['psnr']:.6f} ssim {row['ssim']:.9f} e_ref {e_ref:.2e} e_hip {abs(row['ssim'] - ref):.2e}")
        assert row["sse"] == R.sse(a, b)
        assert abs(row["psnr"] - R.psnr(a, b)) < 1e-9
        assert abs(row["ssim"] - ref) <= max(e_ref, 1e-6)
    assert rep["mean"]["psnr"] == pytest.approx(np.mean([r["psnr"] for r in rep["images"]]), abs=1e-12)
    assert rep["mean"]["ssim"] == pytest.approx(np.mean([r["ssim"] for r in rep["images"]]), abs=1e-15)
    assert set(rep["mean"]) == {"psnr", "ssim"}


def test_score_module_reproduces_the_rows(cli_run, tmp_path):
    d = cli_run["metrics"]
    rep = json.loads((d / "metrics_0.json").read_text())
    out = tmp_path / "score.json"
    done = subprocess.run([sys.executable, "-m", "vspbfr_amd.score", "--restored", str(d), "--gt", str(d), "--dataset", "demo", "--batch", "3",
                           "--out", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stderr[-2000:]
    assert "metrics demo (gauss11, 3 images" in done.stdout
    got = json.loads(out.read_text())
    assert got["mean"] == rep["mean"] and got["count"] == 3
    for r, g in zip(rep["images"], got["images"]):
        assert (g["sse"], g["psnr"], g["ssim"]) == (r["sse"], r["psnr"], r["ssim"])            # floats compared exactly: same bits
        assert g["lq"] == f"{r['index']:06d}_0_demo_restore.png" and g["hq"] == f"{r['index']:06d}_0_demo_gt.png"
    # the other window, scored from the same files against the oracle
    from vspbfr_amd.score import pair_files, score_pairs
    uni = score_pairs(pair_files(str(d), str(d)), "uniform7", batch=2)
    for i, row in enumerate(uni["images"]):
        a, b = _png(d / f"{i:06d}_0_demo_restore.png"), _png(d / f"{i:06d}_0_demo_gt.png")
        assert row["sse"] == R.sse(a, b) and abs(row["ssim"] - R.ssim(a, b, "uniform7")) <= 1e-6


def test_learned_columns_equal_direct_calls(cli_run):
    """The Evaluator's `lpips` and `id` columns are PerceptualLoss() / IDLoss(None).get_id (initial weights) on the de-quantised batch,
    called as the Evaluator calls them (same batches, so the same kernels: equality up to 1e-6).  At its initial weights the identity
    network maps every image to nearly one vector (cosines 0.99994 +- 2e-5), so this comparison cannot tell a right pairing from a wrong
    one: test_id_column_pairs_restored_with_its_own_gt does that."""
    from vspbfr_amd import metrics as M
    from vspbfr_amd.id_loss import IDLoss
    from vspbfr_amd.lpips import PerceptualLoss
    d = cli_run["metrics"]
    torch.manual_seed(5)
    lp, idl = PerceptualLoss().cuda(), IDLoss(None)
    r8 = torch.from_numpy(np.stack([_png(d / f"{i:06d}_0_demo_restore.png") for i in range(3)])).cuda()
    g8 = torch.from_numpy(np.stack([_png(d / f"{i:06d}_0_demo_gt.png") for i in range(3)])).cuda()
    r, g = M.dequantize(r8), M.dequantize(g8)
    assert torch.equal(r, (r8.permute(0, 3, 1, 2).float() / 127.5 - 1.0).contiguous())
    ev = M.Evaluator("gauss11", lp, idl)
    ev.add(r8[:2], g8[:2], [("a", "a"), ("b", "b")])
    ev.add(r8[2:], g8[2:], [("c", "c")])
    rep = ev.report("demo")
    with torch.no_grad():
        want_lp = torch.cat([lp(r[:2], g[:2]).reshape(2), lp(r[2:], g[2:]).reshape(1)]).double().cpu().numpy()
        wrong_lp = torch.cat([lp(r[:2], g[1:]).reshape(2), lp(r[2:], g[:1]).reshape(1)]).double().cpu().numpy()   # restored i, gt i + 1
        z01, z2 = idl.get_id(torch.cat([r[:2], g[:2]])), idl.get_id(torch.cat([r[2:], g[2:]]))
        want_id = (torch.cat([z01[:2], z2[:1]]) * torch.cat([z01[2:], z2[1:]])).sum(1).double().cpu().numpy()
    assert set(rep["mean"]) == {"psnr", "ssim", "lpips", "id"} and [x["index"] for x in rep["images"]] == [0, 1, 2]
    for i, row in enumerate(rep["images"]):
        print(f"image {i}: lpips {row['lpips']:.7f} (direct {want_lp[i]:.7f}, mismatched {wrong_lp[i]:.7f}) "
              f"id {row['id']:+.7f} (direct {want_id[i]:+.7f})")
        assert abs(row["lpips"] - want_lp[i]) <= 1e-6 * max(1.0, abs(want_lp[i]))
        assert abs(row["lpips"] - wrong_lp[i]) > 1e-6 * max(1.0, abs(want_lp[i]))         # a wrong pairing would not have passed
        assert abs(row["id"] - want_id[i]) <= 1e-6 and -1.0 - 1e-6 <= row["id"] <= 1.0 + 1e-6
        assert row["sse"] == R.sse(r8[i].cpu().numpy(), g8[i].cpu().numpy())
    assert rep["mean"]["id"] == pytest.approx(float(np.mean([x["id"] for x in rep["images"]])), abs=1e-15)


def test_id_column_pairs_restored_with_its_own_gt():
    """The pairing logic of the `id` column with an embedding whose cosines are known in closed form: get_id = normalised (2 x 2 average
    pool + 1) of the de-quantised image.  Restored image i is white in quadrant i and black elsewhere; its ground truth is white in
    quadrant i and 128 in quadrant i + 1.  Then cos(restored i, gt i) = 12 / (2 sqrt(3) sqrt(12 + 3 v^2)), v = 128 / 127.5 = 0.89373,
    cos(restored i, gt i + 1) = 0 and cos(restored i, restored i) = 1: a wrong pairing, a shifted batch half or a self-cosine
    cannot pass."""
    import torch.nn.functional as F
    from vspbfr_amd import metrics as M

    class QuadrantId:
        def get_id(self, x):
            return F.normalize(F.adaptive_avg_pool2d(x, 2).flatten(1) + 1.0)

    quad = [(slice(0, 32), slice(0, 32)), (slice(0, 32), slice(32, 64)), (slice(32, 64), slice(0, 32)), (slice(32, 64), slice(32, 64))]
    r8 = torch.zeros(3, 64, 64, 3, dtype=torch.uint8)
    g8 = torch.zeros(3, 64, 64, 3, dtype=torch.uint8)
    for i in range(3):
        r8[i][quad[i]] = 255
        g8[i][quad[i]] = 255
        g8[i][quad[i + 1]] = 128
    r8, g8 = r8.cuda(), g8.cuda()
    ev = M.Evaluator("uniform7", None, QuadrantId())
    ev.add(r8[:2], g8[:2])
    ev.add(r8[2:], g8[2:])
    rep = ev.report()
    v = 128.0 / 127.5
    want = 12.0 / (2.0 * 3.0 ** 0.5 * (12.0 + 3.0 * v * v) ** 0.5)
    assert abs(want - 0.89373) < 1e-5
    for i, row in enumerate(rep["images"]):
        assert abs(row["id"] - want) <= 1e-6, (i, row["id"], want)               # fp32 pooling and normalisation: a few 6e-8
        assert row["sse"] == 32 * 32 * 3 * 128 * 128 and "lpips" not in row
