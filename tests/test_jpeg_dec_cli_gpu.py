"""GPU, end to end: `python -m vspbfr_amd.restore_photos --decode device` against `--decode host` on five small photos with one face
each and random-weight checkpoints -- a baseline 4:2:0 JPEG without restart markers, a 4:4:4 one with optimised Huffman tables, a 4:2:0
one with a restart interval of 3, a progressive one and a PNG: equal output files byte for byte at --upscale 1 and 2, --format png and jpg;
report.json says which route decoded each photo; without the flag the files and the report are what they were."""
import json
import os
import random
from argparse import Namespace

import pytest
import torch

import photo_ref as R

pytestmark = pytest.mark.gpu
SEED = 123
MODEL = ["--timesteps", "4", "--no_sample", "--batch", "2"]
PHOTOS = [("a_base.jpg", (200, 260), 71, dict(quality=90, subsampling=2)),
          ("b_444.jpg", (180, 150), 72, dict(quality=85, subsampling=0, optimize=True)),
          ("c_rst.jpg", (150, 190), 73, dict(quality=75, subsampling=2, restart_marker_blocks=3)),
          ("d_prog.jpg", (160, 160), 74, dict(quality=90, progressive=True)),
          ("sub/e_plain.png", (140, 170), 75, {})]
WANT = {"a_base.jpg": "device", "b_444.jpg": "device", "c_rst.jpg": "device", "d_prog.jpg": "host", "sub/e_plain.png": "host"}


def _files(root):
    return sorted(os.path.relpath(os.path.join(dp, f), root) for dp, _, fs in os.walk(root) for f in fs)


@pytest.fixture(scope="module")
def cli_run(tmp_path_factory):
    from PIL import Image
    from vspbfr_amd import restore_photos
    from vspbfr_amd.diffusion import Code_diffuser
    from vspbfr_amd.e4e import Encoder4Editing, Generator
    from vspbfr_amd.restorenet import Restoration_net
    tmp = tmp_path_factory.mktemp("jpeg_dec_cli")
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
    root = tmp / "photos"
    (root / "sub").mkdir(parents=True)
    marks = {}
    for name, (w, h), seed, kw in PHOTOS:
        Image.fromarray(R.test_photo(w, h, seed=seed)).save(root / name, **kw)
        marks[name] = [R.landmarks_for(3.0, 6.0, (w * 0.45, h * 0.5)).tolist()]
    (tmp / "landmarks.json").write_text(json.dumps(marks))
    runs = {"base": weights + ["--photos", str(root), "--landmarks", str(tmp / "landmarks.json")]}
    for tag, extra in (("plain", []), ("host", ["--decode", "host"]), ("device", ["--decode", "device"]),
                       ("host2", ["--decode", "host", "--upscale", "2", "--format", "jpg"]),
                       ("device2", ["--decode", "device", "--upscale", "2", "--format", "jpg"]),
                       ("host1j", ["--decode", "host", "--format", "jpg"]), ("device1j", ["--decode", "device", "--format", "jpg"]),
                       ("host2p", ["--decode", "host", "--upscale", "2"]), ("device2p", ["--decode", "device", "--upscale", "2"])):
        torch.manual_seed(SEED)
        random.seed(SEED)
        out = tmp / tag
        restore_photos.main(MODEL + runs["base"] + ["--out", str(out), "--save_faces"] + extra)
        runs[tag] = out
    return runs


@pytest.mark.parametrize("host,device,ext", [("host", "device", ".png"), ("host2", "device2", ".jpg"), ("host1j", "device1j", ".jpg"),
                                              ("host2p", "device2p", ".png")])
def test_device_decode_writes_the_files_of_the_host_decode(cli_run, host, device, ext):
    names = [n for n in _files(cli_run[host]) if n != "report.json"]
    assert names == [n for n in _files(cli_run[device]) if n != "report.json"]
    assert sum(n.endswith(ext) and "_crop" not in n and "_restore" not in n for n in names) == 5
    for n in names:
        assert open(cli_run[host] / n, "rb").read() == open(cli_run[device] / n, "rb").read(), n


def test_report_names_the_route(cli_run):
    for tag in ("device", "device2", "device1j", "device2p"):
        rep = json.load(open(cli_run[tag] / "report.json"))
        assert {p["photo"]: p["decode"] for p in rep["photos"]} == WANT
        assert all(p["faces"] == 1 for p in rep["photos"])
    rep = json.load(open(cli_run["host"] / "report.json"))
    assert {p["decode"] for p in rep["photos"]} == {"host"}


def test_without_the_flag_nothing_changes(cli_run):
    assert _files(cli_run["plain"]) == _files(cli_run["host"])
    for n in _files(cli_run["plain"]):
        if n != "report.json":
            assert open(cli_run["plain"] / n, "rb").read() == open(cli_run["host"] / n, "rb").read(), n
    plain, host = json.load(open(cli_run["plain"] / "report.json")), json.load(open(cli_run["host"] / "report.json"))
    assert all("decode" not in p for p in plain["photos"])
    for p in host["photos"]:
        del p["decode"]
    assert plain == host
