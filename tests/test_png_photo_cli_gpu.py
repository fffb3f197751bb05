"""GPU, end to end: `python -m vspbfr_amd.restore_photos` on three small photos with random-weight checkpoints, plain and with
`--png_encode device` at the same seeds: the same file names; every photo and every --save_faces file decodes to the pixels of the plain
run's file; every photo file equals the ragged restatement of its pixels and every face file the uniform restatement, so the device wrote
them, not PIL; the same at --upscale 2; report.json lists `png_encode`; without the flag the directory equals the plain run byte for byte;
the refused flag combinations exit before any model loads."""
import json
import os
import random
from argparse import Namespace

import numpy as np
import pytest
import torch

import photo_ref as P
import png_ragged_ref as RR
import png_ref as R

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
    tmp = tmp_path_factory.mktemp("png_photo_cli")
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
    imgs = {"a_edge.png": P.test_photo(300, 260, seed=61), "b_pair.png": P.test_photo(420, 333, seed=62),
            "sub/c_plain.png": P.test_photo(123, 77, seed=63)}
    marks = {"a_edge.png": [P.landmarks_for(2.0, 12.0, (40.0, 50.0)).tolist()],
             "b_pair.png": [P.landmarks_for(2.4, -8.0, (150.0, 160.0)).tolist(), P.landmarks_for(3.0, 5.0, (300.0, 170.0)).tolist()]}
    root = tmp / "photos"
    (root / "sub").mkdir(parents=True)
    for name, a in imgs.items():
        Image.fromarray(a).save(root / name)
    (tmp / "landmarks.json").write_text(json.dumps(marks))
    runs = {"stems": [os.path.splitext(n)[0] for n in imgs], "base": weights + ["--photos", str(root), "--landmarks", str(tmp / "landmarks.json")],
            "tmp": tmp}
    for tag, extra in (("plain", []), ("device", ["--png_encode", "device"]), ("host", ["--png_encode", "host"]),
                       ("plain2", ["--upscale", "2"]), ("device2", ["--upscale", "2", "--png_encode", "device"]),
                       ("jpg", ["--format", "jpg", "--png_encode", "device"])):
        torch.manual_seed(SEED)
        random.seed(SEED)
        out = tmp / tag
        restore_photos.main(MODEL + runs["base"] + ["--out", str(out), "--save_faces"] + extra)
        runs[tag] = out
    return runs


def _pixels(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


@pytest.mark.parametrize("dev,plain", [("device", "plain"), ("device2", "plain2")])
def test_same_names_and_pixels_and_the_device_wrote_them(cli_run, dev, plain):
    names = _files(cli_run[plain])
    assert _files(cli_run[dev]) == names and sum(n.endswith(".png") for n in names) == 3 + 2 * 3
    photos = [s + ".png" for s in cli_run["stems"]]
    for n in names:
        if not n.endswith(".png"):
            continue
        want = _pixels(cli_run[plain] / n)
        assert np.array_equal(_pixels(cli_run[dev] / n), want), n
        data = open(cli_run[dev] / n, "rb").read()
        # a photo went through the ragged entry, a 512^2 face file through the uniform one
        assert data == (RR.encode_png(want) if n in photos else R.encode_png(want)), n


def test_the_report_lists_png_encode(cli_run):
    assert json.load(open(cli_run["device"] / "report.json"))["png_encode"] == "device"
    rep2 = json.load(open(cli_run["device2"] / "report.json"))
    assert (rep2["png_encode"], rep2["upscale"]) == ("device", 2)
    assert json.load(open(cli_run["host"] / "report.json"))["png_encode"] == "host"
    plain, dev = json.load(open(cli_run["plain"] / "report.json")), json.load(open(cli_run["device"] / "report.json"))
    assert "png_encode" not in plain
    dev.pop("png_encode")
    assert dev == plain


def test_without_the_flag_nothing_changes(cli_run):
    """--png_encode host is the plain run but for the report's one key"""
    assert _files(cli_run["plain"]) == _files(cli_run["host"])
    for f in _files(cli_run["plain"]):
        if f != "report.json":
            assert open(cli_run["plain"] / f, "rb").read() == open(cli_run["host"] / f, "rb").read(), f


def test_with_jpg_photos_the_face_files_take_the_device_encoder(cli_run):
    names = _files(cli_run["jpg"])
    assert sum(n.endswith(".jpg") for n in names) == 3 and sum(n.endswith(".png") for n in names) == 6
    for n in names:
        if n.endswith(".png"):
            want = _pixels(cli_run["plain"] / n)
            assert open(cli_run["jpg"] / n, "rb").read() == R.encode_png(want), n
    rep = json.load(open(cli_run["jpg"] / "report.json"))
    assert (rep["format"], rep["png_encode"]) == ("jpg", "device")


@pytest.mark.parametrize("extra", [["--format", "jpg", "--png_encode", "device"], ["--format", "png", "--encode", "device"],
                                   ["--png_encode", "gpu"]])
def test_refused_flag_combinations_exit_before_any_model_loads(cli_run, extra):
    from vspbfr_amd import restore_photos
    with pytest.raises(SystemExit):
        restore_photos.main(MODEL + ["--ckpt", "/nonexistent.pt"] + cli_run["base"][6:] + ["--out", str(cli_run["tmp"] / "refused")] + extra)
    assert not os.path.exists(cli_run["tmp"] / "refused")
