"""GPU, end to end: both CLIs of the background upscaler on two small photos with random-weight checkpoints (set up as in
tests/test_photo_cli_gpu.py).  `python -m vspbfr_amd.restore_photos --landmarks --upscale 2` with and without --bg_weights: the same file
set, the right sizes, other pixels outside the faces, the `background` block in report.json; a x4 network at --upscale 4 in bands together
with --detect_weights, --decode device and --png_encode device; `python -m vspbfr_amd.upscale` at the network's scale as PNG (the bytes of
SrUpscaler.upscale) and at --scale 2 from the x4 network as JPEG."""
import json
import os
import random
from argparse import Namespace

import numpy as np
import pytest
import torch

import detect_cases as K
import photo_ref as P0
import sr_ref as R

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
    tmp = tmp_path_factory.mktemp("sr_cli")
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
    torch.save({"module." + k: v for k, v in K.model().state_dict().items()}, ck / "retinaface.pt")
    states = {"x2": R.make_state(4, 2, seed=11), "x4": R.make_state(3, 4, seed=12)}
    torch.save({"params_ema": states["x2"]}, ck / "sr_x2.pth")
    torch.save({"params": {"module." + k: v for k, v in states["x4"].items()}}, ck / "sr_x4.pth")
    weights = ["--ckpt", str(ck / "restoration_net.pt"), "--ddpm_ckpt", str(ck / "code_diffuser.pt"), "--psp_checkpoint_path",
               str(ck / "style_encoder_decoder.pt")]
    photos = tmp / "photos"
    (photos / "sub").mkdir(parents=True)
    imgs = {"a.png": P0.test_photo(200, 260, seed=31), "sub/b.png": P0.test_photo(300, 240, seed=32)}
    for name, a in imgs.items():
        Image.fromarray(a).save(photos / name)
    marks = {"a.png": [P0.landmarks_for(4.0, 12.0, (100.0, 130.0)).tolist()]}
    (tmp / "landmarks.json").write_text(json.dumps(marks))
    runs = {"imgs": imgs, "marks": marks, "states": states, "tmp": tmp}
    base = MODEL + weights + ["--photos", str(photos)]
    for tag, extra in (("lanczos", ["--landmarks", str(tmp / "landmarks.json"), "--upscale", "2"]),
                       ("bg_x2", ["--landmarks", str(tmp / "landmarks.json"), "--upscale", "2", "--bg_weights", str(ck / "sr_x2.pth")]),
                       ("bg_x4", ["--detect_weights", str(ck / "retinaface.pt"), "--detect_threshold", "0.5", "--detect_max_faces", "2", "--upscale", "4",
                                  "--bg_weights", str(ck / "sr_x4.pth"), "--bg_band_rows", "16", "--decode", "device", "--png_encode", "device"])):
        torch.manual_seed(SEED)
        random.seed(SEED)
        restore_photos.main(base + ["--out", str(tmp / tag)] + extra)
        runs[tag] = tmp / tag
    upscale.main(["--photos", str(photos), "--weights", str(ck / "sr_x4.pth"), "--out", str(tmp / "own_x4")])
    upscale.main(["--photos", str(photos), "--weights", str(ck / "sr_x4.pth"), "--out", str(tmp / "own_x2"), "--scale", "2", "--format", "jpg",
                  "--band_rows", "40"])
    return runs


def test_background_run_has_the_same_files_and_other_pixels_outside_the_faces(cli_run):
    from vspbfr_amd import photo as P
    a, b = cli_run["lanczos"], cli_run["bg_x2"]
    assert _files(a) == _files(b) == ["a.png", "report.json", "sub/b.png"]
    for name, src in cli_run["imgs"].items():
        h, w = src.shape[:2]
        la, bg = _img(a / name), _img(b / name)
        assert la.shape == bg.shape == (2 * h, 2 * w, 3)
        outside = np.ones((2 * h, 2 * w), dtype=bool)
        for pts in cli_run["marks"].get(name, []):
            A = P.similarity_from_landmarks(np.asarray(pts), size=512)
            x0, y0, x1, y1 = P.face_bbox(P.paste_matrix(A, 2), 512, 2 * h, 2 * w)
            outside[y0:y1, x0:x1] = False
        assert outside.any() and (la[outside] != bg[outside]).any(), name
    ra, rb = (json.loads((d / "report.json").read_text()) for d in (a, b))
    assert "background" not in ra and rb["background"] == {"model": "SRVGGNetCompact", "num_conv": 4, "scale": 2, "banded": False, "nonfinite": []}
    assert [(p["photo"], p["faces"], p["size"]) for p in ra["photos"]] == [(p["photo"], p["faces"], p["size"]) for p in rb["photos"]]
    assert [p["faces"] for p in rb["photos"]] == [1, 0]


def test_the_photo_without_a_face_is_the_upscalers_output(cli_run):
    from vspbfr_amd import upscale as U
    net = U.SrUpscaler(cli_run["states"]["x2"], "cuda")
    src = cli_run["imgs"]["sub/b.png"]
    out, _ = net.upscale(photos=[src])
    assert np.array_equal(_img(cli_run["bg_x2"] / "sub/b.png"), out.view(2 * src.shape[0], 2 * src.shape[1], 3).cpu().numpy())


def test_x4_in_bands_with_detection_device_decode_and_device_png(cli_run):
    out = cli_run["bg_x4"]
    rep = json.loads((out / "report.json").read_text())
    assert rep["background"] == {"model": "SRVGGNetCompact", "num_conv": 3, "scale": 4, "banded": True, "nonfinite": []}
    assert rep["upscale"] == 4 and rep["png_encode"] == "device" and "detect" in rep
    for name, src in cli_run["imgs"].items():
        assert _img(out / name).shape == (4 * src.shape[0], 4 * src.shape[1], 3)
    print("faces found:", [(p["photo"], p["faces"]) for p in rep["photos"]])


def test_the_upscale_cli(cli_run):
    from vspbfr_amd import upscale as U
    tmp = cli_run["tmp"]
    assert _files(tmp / "own_x4") == ["a.png", "sub/b.png"] and _files(tmp / "own_x2") == ["a.jpg", "sub/b.jpg"]
    net = U.SrUpscaler(cli_run["states"]["x4"], "cuda")
    for name, src in cli_run["imgs"].items():
        h, w = src.shape[:2]
        out, _ = net.upscale(photos=[src])
        assert np.array_equal(_img(tmp / "own_x4" / name), out.view(4 * h, 4 * w, 3).cpu().numpy())
        small, _ = net.upscale_to(2, photos=[src])
        jpg = _img(tmp / "own_x2" / (os.path.splitext(name)[0] + ".jpg"))
        assert jpg.shape == (2 * h, 2 * w, 3)
        assert np.abs(jpg.astype(int) - small.view(2 * h, 2 * w, 3).cpu().numpy()).mean() < 12        # a JPEG of that picture, quality 90
