"""GPU, end to end: `python -m vspbfr_amd.restoration_metrics --metrics --niqe_params` on a dataset WITHOUT ground truth writes
the PNGs it writes without the flag and a report with the `niqe` column alone; on a dataset with ground truth every column; and
`python -m vspbfr_amd.score --niqe_params` without --gt reproduces the rows bit for bit from the files."""
import json
import os
import random
import subprocess
import sys
from argparse import Namespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def cli_run(tmp_path_factory):
    from PIL import Image
    from scipy import ndimage
    from vspbfr_amd import niqe, restoration_metrics
    from vspbfr_amd.diffusion import Code_diffuser
    from vspbfr_amd.e4e import Encoder4Editing, Generator
    from vspbfr_amd.restorenet import Restoration_net
    tmp = tmp_path_factory.mktemp("niqe_cli")
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
    for i in range(4):
        sharp = np.clip(ndimage.gaussian_filter(rng.integers(0, 256, (512, 512, 3)).astype(np.float64), (3, 3, 0)) * 4 - 384, 0, 255)
        Image.fromarray(sharp.astype(np.uint8)).save(hq / f"face_{i}.png")
        Image.fromarray(np.clip(ndimage.gaussian_filter(sharp, (4, 4, 0)) + rng.normal(0, 5, sharp.shape), 0, 255).astype(np.uint8)).save(
            lq / f"face_{i}.png")
    a = rng.normal(size=(36, 36))
    niqe.save_params(tmp / "model.npz", rng.normal(size=36), a @ a.T / 36 + np.eye(36))
    runs = {"model": tmp / "model.npz"}
    for tag, hq_arg, extra in (("plain", "None", []), ("wild", "None", ["--metrics", "--niqe_params", str(tmp / "model.npz")]),
                               ("paired", str(hq), ["--metrics", "--niqe_params", str(tmp / "model.npz")])):
        torch.manual_seed(123)
        random.seed(123)
        out = tmp / f"eval_{tag}"
        restoration_metrics.main(["--batch", "2", "--ckpt", str(ck / "restoration_net.pt"), "--ddpm_ckpt", str(ck / "code_diffuser.pt"),
                                  "--psp_checkpoint_path", str(ck / "style_encoder_decoder.pt"), "--eval_dir", str(out), "--timesteps", "4",
                                  "--no_sample", "--lq_data_list", str(lq), "--hq_data_list", hq_arg, "--data_name_list", "demo"] + extra)
        runs[tag] = out / "restoration_net" / "0" / "demo"
    return runs


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def test_a_dataset_without_ground_truth_gets_a_niqe_report_and_the_same_pngs(cli_run):
    from vspbfr_amd import hip_ops as H
    from vspbfr_amd import niqe
    plain, wild = cli_run["plain"], cli_run["wild"]
    pngs = sorted(f"{i:06d}_0_demo_{k}.png" for i in range(4) for k in ("restore", "low"))
    assert sorted(os.listdir(plain)) == pngs and sorted(os.listdir(wild)) == sorted(pngs + ["metrics_0.json"])
    for n in pngs:
        assert (plain / n).read_bytes() == (wild / n).read_bytes(), n
    rep = json.loads((wild / "metrics_0.json").read_text())
    assert rep["count"] == 4 and rep["psnr_infinite"] == 0 and set(rep["mean"]) == {"niqe"}
    params = niqe.load_params(cli_run["model"])
    for i, row in enumerate(rep["images"]):
        assert set(row) == {"index", "lq", "hq", "niqe"} and row["hq"] is None and row["lq"] == f"face_{i}.png"
        u8 = torch.from_numpy(_png(wild / f"{i:06d}_0_demo_restore.png").copy())[None].cuda()
        assert row["niqe"] == niqe.score_from_features(H.niqe_features_u8(u8)[0][0].cpu().numpy(), params)   # the file's own score, same bits
        assert np.isfinite(row["niqe"]) and row["niqe"] > 0
    assert rep["mean"]["niqe"] == pytest.approx(np.mean([r["niqe"] for r in rep["images"]]), abs=1e-12)


def test_a_dataset_with_ground_truth_gets_every_column(cli_run):
    rep = json.loads((cli_run["paired"] / "metrics_0.json").read_text())
    wild = json.loads((cli_run["wild"] / "metrics_0.json").read_text())
    assert set(rep["mean"]) == {"psnr", "ssim", "niqe"} and rep["count"] == 4
    for row, w in zip(rep["images"], wild["images"]):
        assert list(row) == ["index", "lq", "hq", "sse", "psnr", "ssim", "niqe"]
        assert row["niqe"] == w["niqe"]                             # the same restored bytes, the same score


def test_score_module_without_gt_reproduces_the_rows(cli_run, tmp_path):
    d = cli_run["wild"]
    rep = json.loads((d / "metrics_0.json").read_text())
    out = tmp_path / "score.json"
    done = subprocess.run([sys.executable, "-m", "vspbfr_amd.score", "--restored", str(d), "--niqe_params", str(cli_run["model"]), "--dataset",
                           "demo", "--batch", "3", "--out", str(out)], cwd=ROOT, capture_output=True, text=True, timeout=600)
    assert done.returncode == 0, done.stderr[-2000:]
    got = json.loads(out.read_text())
    assert got["mean"] == rep["mean"] and got["count"] == 4
    for r, g in zip(rep["images"], got["images"]):
        assert g["niqe"] == r["niqe"] and g["lq"] == f"{r['index']:06d}_0_demo_restore.png" and g["hq"] is None
