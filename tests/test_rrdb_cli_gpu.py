"""GPU, end to end: both CLIs reach the RRDBNet upscaler through the keys of a random one-block checkpoint, on two small photos
(set up as in tests/test_sr_cli_gpu.py).  `python -m vspbfr_amd.restore_photos --landmarks --upscale 2 --bg_weights` with a x2 network:
the photo without a face is the network's own output and report.json says RRDBNet; `python -m vspbfr_amd.upscale` with a x4 network at
its own scale in bands as PNG (the bytes of RrdbUpscaler.upscale) and at --scale 2."""
import json
import os
import random
from argparse import Namespace

import numpy as np
import pytest
import torch

import photo_ref as P0
import rrdb_ref as R

pytestmark = pytest.mark.gpu
SEED = 123
MODEL = ["--timesteps", "4", "--no_sample", "--batch", "1"]


def _img(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def _files(root):
    return sorted(os.path.relpath(os.path.join(dp, f), root) for dp, _, fs in os.walk(root) for f in fs)


@pytest.fixture(scope="module")
def cli_run(tmp_path_factory):
    from PIL import Image
    from vspbfr_amd import restore_photos, upscale
    from vspbfr_amd.diffusion import Code_diffuser
    from vspbfr_amd.e4e import Encoder4Editing, Generator
    from vspbfr_amd.restorenet import Restoration_net
    tmp = tmp_path_factory.mktemp("rrdb_cli")
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
    states = {"x2": R.make_state(1, 2, seed=11), "x4": R.make_state(1, 4, seed=12)}
    torch.save({"params_ema": states["x2"]}, ck / "rrdb_x2.pth")
    torch.save({"params": {"module." + k: v for k, v in states["x4"].items()}}, ck / "rrdb_x4.pth")
    weights = ["--ckpt", str(ck / "restoration_net.pt"), "--ddpm_ckpt", str(ck / "code_diffuser.pt"), "--psp_checkpoint_path",
               str(ck / "style_encoder_decoder.pt")]
    photos = tmp / "photos"
    (photos / "sub").mkdir(parents=True)
    imgs = {"a.png": P0.test_photo(200, 260, seed=31), "sub/b.png": P0.test_photo(61, 47, seed=32)}
    for name, a in imgs.items():
        Image.fromarray(a).save(photos / name)
    marks = {"a.png": [P0.landmarks_for(4.0, 12.0, (100.0, 130.0)).tolist()]}
    (tmp / "landmarks.json").write_text(json.dumps(marks))
    torch.manual_seed(SEED)
    random.seed(SEED)
    restore_photos.main(MODEL + weights + ["--photos", str(photos), "--out", str(tmp / "bg_x2"), "--landmarks", str(tmp / "landmarks.json"),
                                           "--upscale", "2", "--bg_weights", str(ck / "rrdb_x2.pth")])
    upscale.main(["--photos", str(photos), "--weights", str(ck / "rrdb_x4.pth"), "--out", str(tmp / "own_x4"), "--band_rows", "40"])
    upscale.main(["--photos", str(photos), "--weights", str(ck / "rrdb_x4.pth"), "--out", str(tmp / "own_x2"), "--scale", "2"])
    return {"imgs": imgs, "states": states, "tmp": tmp}


def test_restore_photos_runs_the_rrdb_background(cli_run):
    from vspbfr_amd import rrdb
    out = cli_run["tmp"] / "bg_x2"
    assert _files(out) == ["a.png", "report.json", "sub/b.png"]
    rep = json.loads((out / "report.json").read_text())
    assert rep["background"] == {"model": "RRDBNet", "num_block": 1, "scale": 2, "banded": False, "nonfinite": []}
    assert [p["faces"] for p in rep["photos"]] == [1, 0]
    net = rrdb.RrdbUpscaler(cli_run["states"]["x2"], "cuda")
    src = cli_run["imgs"]["sub/b.png"]
    alone, _ = net.upscale(photos=[src])
    assert np.array_equal(_img(out / "sub/b.png"), alone.view(2 * src.shape[0], 2 * src.shape[1], 3).cpu().numpy())
    a = cli_run["imgs"]["a.png"]
    assert _img(out / "a.png").shape == (2 * a.shape[0], 2 * a.shape[1], 3)


def test_the_upscale_cli_runs_the_rrdb_network(cli_run):
    from vspbfr_amd import rrdb
    tmp = cli_run["tmp"]
    assert _files(tmp / "own_x4") == ["a.png", "sub/b.png"] and _files(tmp / "own_x2") == ["a.png", "sub/b.png"]
    net = rrdb.RrdbUpscaler(cli_run["states"]["x4"], "cuda")
    for name, src in cli_run["imgs"].items():
        h, w = src.shape[:2]
        out, _ = net.upscale(photos=[src])
        assert np.array_equal(_img(tmp / "own_x4" / name), out.view(4 * h, 4 * w, 3).cpu().numpy())
        small, _ = net.upscale_to(2, photos=[src])
        assert np.array_equal(_img(tmp / "own_x2" / name), small.view(2 * h, 2 * w, 3).cpu().numpy())
