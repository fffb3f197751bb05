"""GPU, end to end: the CLIs with a 2D-FAN file (random weights, 2 modules of depth 2 at full widths: tests/fan_ref.py; the restorer's
checkpoints as in tests/test_metrics_cli_gpu.py).  `score --lmd_weights` and `restoration_metrics --metrics --lmd_weights` add the
`lmd` and `nme` columns, equal to the figures NumPy gives from `FanLandmarks.landmarks` on the files; `python -m vspbfr_amd.fan`
writes those landmarks; a run of each CLI without the flag writes the files and the report of the code paths of before, byte for byte."""
import json
import random
from argparse import Namespace

import numpy as np
import pytest
import torch

import fan_ref as R

pytestmark = pytest.mark.gpu
SEED = 123
BOX = "16,8,480"


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


@pytest.fixture(scope="module")
def fan_file(tmp_path_factory):
    path = tmp_path_factory.mktemp("fan_weights") / "2dfan.pth"
    torch.save({"state_dict": {"module." + k: v for k, v in R.state_of(R.make_model(0, 2, 2), tracked=True).items()}}, path)
    return str(path)


@pytest.fixture(scope="module")
def folders(tmp_path_factory):
    """four pairs of 96 x 96 files under the CLI's own names, and one pair of another size"""
    from PIL import Image
    tmp = tmp_path_factory.mktemp("fan_pairs")
    for i in range(5):
        hw = (96, 96) if i < 4 else (72, 120)
        Image.fromarray(R.test_photo(*hw, 10 + i)).save(tmp / f"{i:06d}_0_demo_restore.png")
        Image.fromarray(R.test_photo(*hw, 10 + i) if i == 2 else R.test_photo(*hw, 20 + i)).save(tmp / f"{i:06d}_0_demo_gt.png")
    return tmp


def _expected(net, d, names, box):
    """lmd and nme per pair from the landmarks of the files, in NumPy"""
    out = []
    for r, g in names:
        lm = [net.landmarks(torch.from_numpy(_png(d / n)).unsqueeze(0).cuda(), box)[0].cpu().numpy() for n in (r, g)]
        a, b = R.lmd_nme_ref(*lm)
        out.append((float(a[0]), float(b[0])))
    return out


def test_score_with_and_without_the_flag(folders, fan_file, tmp_path):
    from vspbfr_amd import metrics as M, score
    from vspbfr_amd.fan import FanLandmarks
    base = ["--restored", str(folders), "--gt", str(folders), "--dataset", "demo", "--batch", "3"]
    score.main(base + ["--out", str(tmp_path / "plain.json")])
    score.main(base + ["--out", str(tmp_path / "lmd.json"), "--lmd_weights", fan_file, "--lmd_box", "8,4,80"])
    # without the flag: the report of the code path of before (score_pairs and write_report without a word of lmd), byte for byte
    M.write_report(score.score_pairs(score.pair_files(str(folders), str(folders)), batch=3, dataset="demo"), str(tmp_path / "before.json"))
    assert (tmp_path / "plain.json").read_bytes() == (tmp_path / "before.json").read_bytes()
    assert b"lmd" not in (tmp_path / "plain.json").read_bytes() and b"nme" not in (tmp_path / "plain.json").read_bytes()
    plain, rep = json.loads((tmp_path / "plain.json").read_text()), json.loads((tmp_path / "lmd.json").read_text())
    assert [{k: v for k, v in r.items() if k not in ("lmd", "nme")} for r in rep["images"]] == plain["images"]
    assert {k: v for k, v in rep["mean"].items() if k not in ("lmd", "nme")} == plain["mean"]
    net = FanLandmarks(fan_file, "cuda")
    assert net.describe()["num_modules"] == 2 and net.describe()["depth"] == 2 and net.side == 256
    want = _expected(net, folders, [(r["lq"], r["hq"]) for r in rep["images"]], (8.0, 4.0, 80.0))
    for row, (d, e) in zip(rep["images"], want):
        print(f"FAN score {row['lq']}: lmd {row['lmd']!r} (NumPy {d!r}) nme {row['nme']!r} (NumPy {e!r})")
        assert abs(row["lmd"] - d) <= 1e-12 * max(d, 1e-300)
        assert (row["nme"] is None and not np.isfinite(e)) or abs(row["nme"] - e) <= 1e-12 * e
    assert rep["images"][2]["lmd"] == 0.0 and sum(r["lmd"] > 0 for r in rep["images"]) == 4
    assert rep["mean"]["lmd"] == pytest.approx(np.mean([d for d, _ in want]), rel=1e-12)


def test_landmark_cli_writes_the_68_points(folders, fan_file, tmp_path):
    from vspbfr_amd import fan
    from vspbfr_amd.detect import as_json_floats
    out = tmp_path / "sub" / "landmarks68.json"
    fan.main(["--faces", str(folders), "--weights", fan_file, "--out", str(out), "--box", "8,4,80"])
    got = json.loads(out.read_text())
    assert sorted(got) == sorted(f"{i:06d}_0_demo_{k}.png" for i in range(5) for k in ("restore", "gt"))
    net = fan.FanLandmarks(fan_file, "cuda")
    for name, pts in got.items():
        lm = net.landmarks(torch.from_numpy(_png(folders / name)).unsqueeze(0).cuda(), (8.0, 4.0, 80.0))[0][0].cpu().numpy()
        assert np.array_equal(np.asarray(pts, dtype=np.float64), as_json_floats(lm)) and len(pts) == 68
    assert got["000002_0_demo_restore.png"] == got["000002_0_demo_gt.png"]


@pytest.fixture(scope="module")
def cli_run(tmp_path_factory, fan_file):
    """the restorer's three synthetic checkpoints, 2 LQ + 2 HQ files, and one run of `restoration_metrics --metrics` without and one
    with --lmd_weights, from the same seeds"""
    from PIL import Image
    from vspbfr_amd import restoration_metrics
    from vspbfr_amd.diffusion import Code_diffuser
    from vspbfr_amd.e4e import Encoder4Editing, Generator
    from vspbfr_amd.restorenet import Restoration_net
    tmp = tmp_path_factory.mktemp("fan_cli")
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
    for i in range(2):
        Image.fromarray(R.test_photo(512, 512, 40 + i)).save(hq / f"face_{i}.png")
        Image.fromarray(R.test_photo(512, 512, 50 + i)).save(lq / f"face_{i}.png")
    runs = {}
    for tag, extra in (("plain", []), ("lmd", ["--lmd_weights", fan_file, "--lmd_box", BOX])):
        torch.manual_seed(SEED)
        random.seed(SEED)
        out = tmp / f"eval_{tag}"
        restoration_metrics.main(["--batch", "2", "--ckpt", str(ck / "restoration_net.pt"), "--ddpm_ckpt", str(ck / "code_diffuser.pt"),
                                  "--psp_checkpoint_path", str(ck / "style_encoder_decoder.pt"), "--eval_dir", str(out), "--timesteps", "4",
                                  "--no_sample", "--lq_data_list", str(lq), "--hq_data_list", str(hq), "--data_name_list", "demo", "--metrics"] + extra)
        runs[tag] = out / "restoration_net" / "0" / "demo"
    return runs


def test_restoration_metrics_with_and_without_the_flag(cli_run, fan_file):
    import os

    from vspbfr_amd import metrics as M
    from vspbfr_amd.fan import FanLandmarks
    plain, scored = cli_run["plain"], cli_run["lmd"]
    assert sorted(os.listdir(plain)) == sorted(os.listdir(scored))
    for n in sorted(os.listdir(plain)):
        if n.endswith(".png"):
            assert (plain / n).read_bytes() == (scored / n).read_bytes(), n
    rep = json.loads((scored / "metrics_0.json").read_text())
    assert b"lmd" not in (plain / "metrics_0.json").read_bytes()
    # the flagged report without its two columns, written again, is the unflagged file byte for byte
    bare = dict(rep, images=[{k: v for k, v in r.items() if k not in ("lmd", "nme")} for r in rep["images"]],
                mean={k: v for k, v in rep["mean"].items() if k not in ("lmd", "nme")})
    assert (json.dumps(bare, indent=1, allow_nan=False) + "\n").encode() == (plain / "metrics_0.json").read_bytes()
    assert list(rep["mean"]) == ["psnr", "ssim", "lmd", "nme"] and "lmd" in M.summary_line(rep)
    net = FanLandmarks(fan_file, "cuda")
    names = [(f"{r['index']:06d}_0_demo_restore.png", f"{r['index']:06d}_0_demo_gt.png") for r in rep["images"]]
    for row, (d, e) in zip(rep["images"], _expected(net, scored, names, tuple(float(v) for v in BOX.split(",")))):
        print(f"FAN restoration_metrics image {row['index']}: lmd {row['lmd']!r} (NumPy {d!r}) nme {row['nme']!r} (NumPy {e!r})")
        assert d > 0 and abs(row["lmd"] - d) <= 1e-12 * d
        assert (row["nme"] is None and not np.isfinite(e)) or abs(row["nme"] - e) <= 1e-12 * e
