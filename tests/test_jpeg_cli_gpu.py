"""GPU, end to end: `python -m vspbfr_amd.restore_photos` on three small photos with random-weight checkpoints, at `--format png` and at
`--format jpg --encode device` with the same seeds: every .jpg equals Pillow's encoding of the corresponding .png's pixels at the same
parameters; `--encode host` writes equal bytes; the same at --upscale 2 and 4:4:4; report.json names the .jpg files and lists the
format; without the new flags the files equal those of the png run, report.json included; bad flags are refused before any model loads."""
import json
import os
import random
from argparse import Namespace

import numpy as np
import pytest
import torch

import jpeg_ref as J
import photo_ref as R

pytestmark = pytest.mark.gpu
SEED = 123
MODEL = ["--timesteps", "4", "--no_sample", "--batch", "2"]


def _files(root):
    return sorted(os.path.relpath(os.path.join(dp, f), root) for dp, _, fs in os.walk(root) for f in fs)


@pytest.fixture(scope="module")
def cli_run(tmp_path_factory):
    from PIL import Image
    from vspbfr_amd import restore_photos
    from vspbfr_amd.diffusion import Code_diffuser
    from vspbfr_amd.e4e import Encoder4Editing, Generator
    from vspbfr_amd.restorenet import Restoration_net
    tmp = tmp_path_factory.mktemp("jpeg_cli")
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
    weights = ["--ckpt", str(ck / "restoration_net.pt"), "--ddpm_ckpt", str(ck / "code_diffuser.pt"), "--psp_checkpoint_path",
               str(ck / "style_encoder_decoder.pt")]
    imgs = {"a_edge.png": R.test_photo(300, 260, seed=61), "b_pair.png": R.test_photo(420, 333, seed=62),
            "sub/c_plain.png": R.test_photo(123, 77, seed=63)}
    marks = {"a_edge.png": [R.landmarks_for(2.0, 12.0, (40.0, 50.0)).tolist()],
             "b_pair.png": [R.landmarks_for(2.4, -8.0, (150.0, 160.0)).tolist(), R.landmarks_for(3.0, 5.0, (300.0, 170.0)).tolist()]}
    root = tmp / "photos"
    (root / "sub").mkdir(parents=True)
    for name, a in imgs.items():
        Image.fromarray(a).save(root / name)
    (tmp / "landmarks.json").write_text(json.dumps(marks))
    runs = {"stems": [os.path.splitext(n)[0] for n in imgs], "base": weights + ["--photos", str(root), "--landmarks", str(tmp / "landmarks.json")],
            "tmp": tmp}
    for tag, extra in (("plain", []), ("png", ["--format", "png"]), ("device", ["--format", "jpg", "--encode", "device"]),
                       ("host", ["--format", "jpg", "--encode", "host"]),
                       ("png2", ["--upscale", "2"]),
                       ("device2", ["--upscale", "2", "--format", "jpg", "--quality", "75", "--subsampling", "444"])):
        torch.manual_seed(SEED)
        random.seed(SEED)
        out = tmp / tag
        restore_photos.main(MODEL + runs["base"] + ["--out", str(out), "--save_faces"] + extra)
        runs[tag] = out
    return runs


def _pixels(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


@pytest.mark.parametrize("jpg,png,quality,sub", [("device", "png", 90, "420"), ("host", "png", 90, "420"), ("device2", "png2", 75, "444")])
def test_jpg_equals_pillow_on_the_png_pixels(cli_run, jpg, png, quality, sub):
    for stem in cli_run["stems"]:
        data = open(cli_run[jpg] / (stem + ".jpg"), "rb").read()
        assert data == J.pillow_file(_pixels(cli_run[png] / (stem + ".png")), quality, sub, J.DEFAULT_RESTART), stem
        assert not os.path.exists(cli_run[jpg] / (stem + ".png"))


def test_device_and_host_routes_write_the_same_files(cli_run):
    assert _files(cli_run["device"]) == _files(cli_run["host"])
    for f in _files(cli_run["device"]):
        assert open(cli_run["device"] / f, "rb").read() == open(cli_run["host"] / f, "rb").read(), f


def test_faces_stay_png_and_the_report_names_the_jpgs(cli_run):
    names = _files(cli_run["device"])
    assert sum(n.endswith(".jpg") for n in names) == 3
    assert [n for n in names if n.endswith("_crop.png")] == [n for n in _files(cli_run["png"]) if n.endswith("_crop.png")]
    for n in names:
        if n.endswith(".png"):
            assert open(cli_run["device"] / n, "rb").read() == open(cli_run["png"] / n, "rb").read(), n
    rep = json.load(open(cli_run["device"] / "report.json"))
    assert (rep["format"], rep["quality"], rep["subsampling"]) == ("jpg", 90, "420")
    assert sorted(p["output"] for p in rep["photos"]) == sorted(s + ".jpg" for s in cli_run["stems"])
    rep2 = json.load(open(cli_run["device2"] / "report.json"))
    assert (rep2["format"], rep2["quality"], rep2["subsampling"], rep2["upscale"]) == ("jpg", 75, "444", 2)
    plain = json.load(open(cli_run["plain"] / "report.json"))
    assert "format" not in plain and "quality" not in plain and "subsampling" not in plain


def test_the_default_is_untouched(cli_run):
    assert _files(cli_run["plain"]) == _files(cli_run["png"])
    for f in _files(cli_run["plain"]):
        assert open(cli_run["plain"] / f, "rb").read() == open(cli_run["png"] / f, "rb").read(), f


@pytest.mark.parametrize("extra", [["--format", "jpg", "--quality", "0"], ["--format", "jpg", "--quality", "101"], ["--quality", "80"],
                                   ["--format", "png", "--encode", "device"], ["--format", "jpg", "--subsampling", "422"]])
def test_bad_flags_are_refused_before_any_model_loads(cli_run, extra):
    from vspbfr_amd import restore_photos
    with pytest.raises(SystemExit):
        restore_photos.main(MODEL + ["--ckpt", "/nonexistent.pt"] + cli_run["base"][6:] + ["--out", str(cli_run["tmp"] / "refused")] + extra)
    assert not os.path.exists(cli_run["tmp"] / "refused")
