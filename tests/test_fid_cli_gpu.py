"""GPU, end to end: `--fid_weights` / `--fid_stats` of `python -m vspbfr_amd.restoration_metrics --metrics` and `python -m vspbfr_amd.score`
(DESIGN 25).  The report's `fid.value` is the Frechet distance of the statistics of the feature files written beside it; two ranks merge
to what one pass over the same files gives; a dataset without ground truth is scored against statistics; without the flags the output
directory is the parent's, byte for byte.  Every Frechet distance here takes the root of a 2048 x 2048 product on the host, a few seconds
each, so the runs are few and shared."""
import json
import os
import random
from argparse import Namespace

import numpy as np
import pytest
import torch

import fid_ref as R

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def cli_run(tmp_path_factory):
    from PIL import Image
    from scipy import ndimage
    from vspbfr_amd import fid, restoration_metrics
    from vspbfr_amd.diffusion import Code_diffuser
    from vspbfr_amd.e4e import Encoder4Editing, Generator
    from vspbfr_amd.restorenet import Restoration_net
    tmp = tmp_path_factory.mktemp("fid_cli")
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
    torch.save(R.shared_state(), ck / "fid_inception.pth")
    lq, hq = tmp / "lq", tmp / "hq"
    lq.mkdir()
    hq.mkdir()
    rng = np.random.default_rng(1)
    for i in range(4):
        sharp = np.clip(ndimage.gaussian_filter(rng.integers(0, 256, (512, 512, 3)).astype(np.float64), (3, 3, 0)) * 4 - 384, 0, 255)
        Image.fromarray(sharp.astype(np.uint8)).save(hq / f"face_{i}.png")
        Image.fromarray(np.clip(ndimage.gaussian_filter(sharp, (4, 4, 0)) + rng.normal(0, 5, sharp.shape), 0, 255).astype(np.uint8)).save(
            lq / f"face_{i}.png")
    # reference statistics: those of 8 random feature rows (any valid pair serves)
    f = rng.standard_normal((8, 2048))
    stats_file = tmp / "ref_stats.npz"
    fid.save_stats(str(stats_file), f.mean(0), np.cov(f, rowvar=False))
    runs = {"stats": stats_file, "weights": ck / "fid_inception.pth", "hq": hq}
    w = ["--fid_weights", str(ck / "fid_inception.pth")]
    for tag, hq_arg, extra, world in (("plain", "None", [], 1), ("wild", "None", ["--metrics"] + w + ["--fid_stats", str(stats_file)], 1),
                                      ("ranks", str(hq), ["--metrics"] + w, 2)):
        out = tmp / f"eval_{tag}"
        for rank in range(world):
            torch.manual_seed(123)
            random.seed(123)
            old = {k: os.environ.get(k) for k in ("WORLD_SIZE", "RANK")}
            os.environ.update({"WORLD_SIZE": str(world), "RANK": str(rank)})
            try:
                restoration_metrics.main(["--batch", "2", "--ckpt", str(ck / "restoration_net.pt"), "--ddpm_ckpt", str(ck / "code_diffuser.pt"),
                                          "--psp_checkpoint_path", str(ck / "style_encoder_decoder.pt"), "--eval_dir", str(out), "--timesteps",
                                          "4", "--no_sample", "--lq_data_list", str(lq), "--hq_data_list", hq_arg, "--data_name_list",
                                          "demo"] + extra)
            finally:
                for k, v in old.items():
                    os.environ.pop(k, None) if v is None else os.environ.__setitem__(k, v)
        runs[tag] = out / "restoration_net" / "0" / "demo"
    return runs


def _value_of_files(report_path, ref_stats=None):
    from vspbfr_amd import fid
    from vspbfr_amd import metrics as M
    _, f = M.read_fid_features(M.fid_feature_path(str(report_path)))
    other = fid.stats(M.read_fid_features(M.fid_feature_path(str(report_path), gt=True))[1]) if ref_stats is None else ref_stats
    return fid.frechet_distance(*fid.stats(f), *other)


def test_without_ground_truth_fid_against_statistics_and_the_same_pngs(cli_run, capsys):
    from vspbfr_amd import fid
    from vspbfr_amd import metrics as M
    plain, wild = cli_run["plain"], cli_run["wild"]
    pngs = sorted(f"{i:06d}_0_demo_{k}.png" for i in range(4) for k in ("restore", "low"))
    assert sorted(os.listdir(plain)) == pngs                        # without the flags: what the parent writes, nothing more
    assert sorted(os.listdir(wild)) == sorted(pngs + ["metrics_0.json", "fid_features_0.npy"])
    for n in pngs:
        assert (plain / n).read_bytes() == (wild / n).read_bytes(), n
    rep = json.loads((wild / "metrics_0.json").read_text())
    assert rep["count"] == 4 and rep["mean"] == {} and all(set(r) == {"index", "lq", "hq"} for r in rep["images"])
    assert rep["fid"]["count"] == 4 and rep["fid"]["against"] == "stats" and rep["fid"]["ref"] == str(cli_run["stats"])
    want = _value_of_files(wild / "metrics_0.json", fid.load_stats(str(cli_run["stats"])))
    assert abs(rep["fid"]["value"] - want) <= 1e-12 * max(1.0, abs(want))
    assert M.summary_line(rep).endswith("fid %.6g" % rep["fid"]["value"])
    idx, f = M.read_fid_features(M.fid_feature_path(str(wild / "metrics_0.json")))
    assert idx.tolist() == [0, 1, 2, 3] and f.shape == (4, 2048) and np.isfinite(f).all() and f.std() > 0
    # the features are those of the files on disk
    from PIL import Image
    net = fid.FidInception(fid.load(str(cli_run["weights"])), "cuda")
    again = net.features([np.asarray(Image.open(wild / f"{i:06d}_0_demo_restore.png").convert("RGB")) for i in range(4)]).cpu().numpy()
    assert np.array_equal(again, f)


def test_two_ranks_merge_to_one_pass_of_score_over_their_files(cli_run, tmp_path, capsys):
    from vspbfr_amd import metrics as M
    from vspbfr_amd import score
    d = cli_run["ranks"]
    files = sorted(os.listdir(d))
    assert [f for f in files if not f.endswith(".png")] == ["fid_features_0.npy", "fid_features_0_gt.npy", "fid_features_1.npy",
                                                            "fid_features_1_gt.npy", "metrics_0.json", "metrics_1.json"]
    r0 = json.loads((d / "metrics_0.json").read_text())
    assert r0["fid"]["against"] == "gt" and r0["fid"]["ref"] is None and r0["fid"]["count"] == 2 and set(r0["mean"]) == {"psnr", "ssim"}
    want0 = _value_of_files(d / "metrics_0.json")
    assert abs(r0["fid"]["value"] - want0) <= 1e-12 * max(1.0, abs(want0))
    merged = M.merge_reports([str(d / "metrics_0.json"), str(d / "metrics_1.json")])
    assert merged["count"] == 4 and merged["fid"]["count"] == 4 and merged["fid"]["against"] == "gt"
    # one pass of score over the same files, with the other columns ...
    out = tmp_path / "score.json"
    rep = score.main(["--restored", str(d), "--gt", str(d), "--fid_weights", str(cli_run["weights"]), "--out", str(out), "--batch", "3"])
    assert rep["fid"]["count"] == 4 and set(rep["mean"]) == {"psnr", "ssim"}
    assert abs(rep["fid"]["value"] - merged["fid"]["value"]) <= 1e-9 * max(1.0, abs(merged["fid"]["value"]))
    assert sorted(os.listdir(tmp_path)) == ["score.json", "score_fid_features.npy", "score_fid_features_gt.npy"]
    assert "fid %.6g" % rep["fid"]["value"] in capsys.readouterr().out
    # ... and against statistics without ground truth and without any other column
    rep = score.main(["--restored", str(d), "--fid_weights", str(cli_run["weights"]), "--fid_stats", str(cli_run["stats"]), "--out",
                      str(tmp_path / "wild.json")])
    assert rep["mean"] == {} and rep["fid"]["against"] == "stats" and rep["fid"]["count"] == 4
    want = _value_of_files(tmp_path / "wild.json", __import__("vspbfr_amd.fid", fromlist=["load_stats"]).load_stats(str(cli_run["stats"])))
    assert abs(rep["fid"]["value"] - want) <= 1e-12 * max(1.0, abs(want))
