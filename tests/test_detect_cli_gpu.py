"""GPU, end to end: `python -m vspbfr_amd.restore_photos --detect_weights` on two photos with random-weight checkpoints (set up as in
tests/test_photo_cli_gpu.py) and the random-weight detector of tests/detect_cases.py.  The faces it finds are used, listed in report.json
and written to <out>/landmarks.json; a second run that reads that file with the same seeds writes the same photo files byte for byte;
a run with --decode device, where the detector reads the decoder's buffer, writes the same files again; `python -m vspbfr_amd.detect`
writes the same landmarks; a run with neither --landmarks nor --detect_weights is a parser error."""
import json
import random
from argparse import Namespace

import numpy as np
import pytest
import torch

import detect_cases as K
import detect_ref as R

pytestmark = pytest.mark.gpu
SEED = 123
MODEL = ["--timesteps", "4", "--no_sample", "--batch", "1"]
DETECT = ["--detect_threshold", "0.5", "--detect_max_faces", "2"]


@pytest.fixture(scope="module")
def cli_run(tmp_path_factory):
    from PIL import Image
    from vspbfr_amd import detect, restore_photos
    from vspbfr_amd.diffusion import Code_diffuser
    from vspbfr_amd.e4e import Encoder4Editing, Generator
    from vspbfr_amd.restorenet import Restoration_net
    tmp = tmp_path_factory.mktemp("detect_cli")
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
    weights = ["--ckpt", str(ck / "restoration_net.pt"), "--ddpm_ckpt", str(ck / "code_diffuser.pt"), "--psp_checkpoint_path",
               str(ck / "style_encoder_decoder.pt")]
    photos = tmp / "photos"
    (photos / "sub").mkdir(parents=True)
    imgs = {"a.png": R.test_photo(200, 260, seed=31), "sub/b.png": R.test_photo(300, 240, seed=32)}
    for name, a in imgs.items():
        Image.fromarray(a).save(photos / name)
    runs = {"imgs": imgs, "photos": photos, "weights": weights, "tmp": tmp}
    found = ["--detect_weights", str(ck / "retinaface.pt")] + DETECT
    for tag, where in (("detect", found), ("landmarks", None), ("decode_device", found + ["--decode", "device"])):
        torch.manual_seed(SEED)
        random.seed(SEED)
        out = tmp / tag
        restore_photos.main(MODEL + weights + ["--photos", str(photos), "--out", str(out)]
                            + (where or ["--landmarks", str(tmp / "detect" / "landmarks.json")]))
        runs[tag] = out
    detect.main(["--photos", str(photos), "--weights", str(ck / "retinaface.pt"), "--out", str(tmp / "alone.json"), "--threshold", "0.5",
                 "--max_faces", "2"])
    return runs


def test_detected_faces_are_used_and_reported(cli_run):
    out = cli_run["detect"]
    rep = json.loads((out / "report.json").read_text())
    assert rep["detect"] == {"threshold": 0.5, "nms": 0.4, "side": 1024, "max_faces": 2, "min_face": 0.0}
    marks = json.loads((out / "landmarks.json").read_text())
    used = 0
    for p in rep["photos"]:
        n = p["faces"]
        assert n == len(p["score"]) == len(p["box"]) == len(marks.get(p["photo"], [])) and n + len(p.get("dropped", [])) <= 2
        assert all(0.5 < s <= 1.0 for s in p["score"]) and p["score"] == sorted(p["score"], reverse=True)
        for face, box in zip(marks.get(p["photo"], []), p["box"]):
            assert np.asarray(face).shape == (5, 2) and box[0] < box[2] and box[1] < box[3]
        for d in p.get("dropped", []):
            assert d["reason"] and "score" in d and "box" in d
        used += n
    print(f"faces used: {used}; photos {[(p['photo'], p['faces'], len(p.get('dropped', []))) for p in rep['photos']]}")
    assert used >= 1
    changed = [name for name, a in cli_run["imgs"].items() if (out / name).read_bytes() and not np.array_equal(_png(out / name), a)]
    assert changed


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def test_a_run_from_the_written_landmarks_gives_the_same_files(cli_run):
    a, b = cli_run["detect"], cli_run["landmarks"]
    for name in cli_run["imgs"]:
        assert (a / name).read_bytes() == (b / name).read_bytes(), name
    ra, rb = (json.loads((d / "report.json").read_text()) for d in (a, b))
    assert [(p["photo"], p["faces"]) for p in ra["photos"]] == [(p["photo"], p["faces"]) for p in rb["photos"]]
    assert "detect" not in rb and not (b / "landmarks.json").exists()


def test_with_decode_device_the_detector_reads_the_decoders_buffer(cli_run):
    """the group's packed device buffer goes to detect(device_photos=...): the same faces, the same files"""
    a, b = cli_run["detect"], cli_run["decode_device"]
    assert (a / "landmarks.json").read_bytes() == (b / "landmarks.json").read_bytes()
    for name in cli_run["imgs"]:
        assert (a / name).read_bytes() == (b / name).read_bytes(), name
    rep = json.loads((b / "report.json").read_text())
    assert all("decode" in p and "score" in p for p in rep["photos"]) and rep["detect"]["max_faces"] == 2


def test_the_detector_cli_writes_the_same_landmarks(cli_run):
    alone = json.loads((cli_run["tmp"] / "alone.json").read_text())
    rep = json.loads((cli_run["detect"] / "report.json").read_text())
    used = json.loads((cli_run["detect"] / "landmarks.json").read_text())
    for p in rep["photos"]:
        dropped = {d["face"] for d in p.get("dropped", [])}
        kept = [f for j, f in enumerate(alone.get(p["photo"], [])) if j not in dropped]
        assert kept == used.get(p["photo"], []), p["photo"]


def test_neither_source_of_faces_is_a_parser_error(cli_run, capsys):
    from vspbfr_amd import restore_photos
    with pytest.raises(SystemExit) as e:
        restore_photos.main(MODEL + cli_run["weights"] + ["--photos", str(cli_run["photos"]), "--out", str(cli_run["tmp"] / "none")])
    assert e.value.code == 2 and "exactly one of --landmarks and --detect_weights" in capsys.readouterr().err
