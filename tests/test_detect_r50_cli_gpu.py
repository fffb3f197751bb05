"""GPU, end to end: both CLIs with a ResNet-50 RetinaFace file (random weights, tests/detect_r50_cases.py; the restorer's checkpoints as
in tests/test_detect_cli_gpu.py).  `restore_photos --detect_weights` finds faces with it, lists `backbone` in report.json and writes
landmarks.json; a second run from that file writes the same photo files byte for byte; `python -m vspbfr_amd.detect` writes the same
landmarks.  A MobileNet file through the factory writes exactly the files a run through RetinaFaceDetector itself writes."""
import json
import random
from argparse import Namespace

import numpy as np
import pytest
import torch

import detect_cases as K0
import detect_r50_cases as K
import detect_ref as R

pytestmark = pytest.mark.gpu
SEED = 123
MODEL = ["--timesteps", "4", "--no_sample", "--batch", "1"]
DETECT = ["--detect_threshold", "0.5", "--detect_max_faces", "2", "--detect_side", "256"]


@pytest.fixture(scope="module")
def cli_run(tmp_path_factory):
    from PIL import Image
    from vspbfr_amd import detect, restore_photos
    from vspbfr_amd.diffusion import Code_diffuser
    from vspbfr_amd.e4e import Encoder4Editing, Generator
    from vspbfr_amd.restorenet import Restoration_net
    tmp = tmp_path_factory.mktemp("detect_r50_cli")
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
    torch.save({"module." + k: v for k, v in K.state().items()}, ck / "retinaface_r50.pth")
    torch.save(K0.model().state_dict(), ck / "retinaface_mnet.pth")
    weights = ["--ckpt", str(ck / "restoration_net.pt"), "--ddpm_ckpt", str(ck / "code_diffuser.pt"), "--psp_checkpoint_path",
               str(ck / "style_encoder_decoder.pt")]
    photos = tmp / "photos"
    (photos / "sub").mkdir(parents=True)
    imgs = {"a.png": R.test_photo(200, 260, seed=31), "sub/b.png": R.test_photo(300, 240, seed=32)}
    for name, a in imgs.items():
        Image.fromarray(a).save(photos / name)
    runs = {"imgs": imgs, "photos": photos, "tmp": tmp, "ck": ck}

    def restore(tag, where):
        torch.manual_seed(SEED)
        random.seed(SEED)
        restore_photos.main(MODEL + weights + ["--photos", str(photos), "--out", str(tmp / tag)] + where)
        runs[tag] = tmp / tag

    restore("r50", ["--detect_weights", str(ck / "retinaface_r50.pth")] + DETECT)
    restore("r50_landmarks", ["--landmarks", str(tmp / "r50" / "landmarks.json")])
    restore("mnet", ["--detect_weights", str(ck / "retinaface_mnet.pth")] + DETECT)
    factory = restore_photos.load_detector
    restore_photos.load_detector = lambda w, device: detect.RetinaFaceDetector(w, device)      # the route of before, without the factory
    try:
        restore("mnet_direct", ["--detect_weights", str(ck / "retinaface_mnet.pth")] + DETECT)
    finally:
        restore_photos.load_detector = factory
    for tag, name in (("r50", "retinaface_r50.pth"), ("mnet", "retinaface_mnet.pth")):
        detect.main(["--photos", str(photos), "--weights", str(ck / name), "--out", str(tmp / f"alone_{tag}.json"), "--threshold", "0.5",
                     "--max_faces", "2", "--side", "256"])
    return runs


def test_the_r50_file_finds_the_faces_and_names_its_backbone(cli_run):
    out = cli_run["r50"]
    rep = json.loads((out / "report.json").read_text())
    assert rep["detect"] == {"threshold": 0.5, "nms": 0.4, "side": 256, "max_faces": 2, "min_face": 0.0, "backbone": "resnet50"}
    marks = json.loads((out / "landmarks.json").read_text())
    used = 0
    for p in rep["photos"]:
        n = p["faces"]
        assert n == len(p["score"]) == len(p["box"]) == len(marks.get(p["photo"], [])) and n + len(p.get("dropped", [])) <= 2
        assert all(0.5 < s <= 1.0 for s in p["score"]) and p["score"] == sorted(p["score"], reverse=True)
        for face, box in zip(marks.get(p["photo"], []), p["box"]):
            assert np.asarray(face).shape == (5, 2) and box[0] < box[2] and box[1] < box[3]
        used += n
    print(f"faces used: {used}; photos {[(p['photo'], p['faces'], len(p.get('dropped', []))) for p in rep['photos']]}")
    assert used >= 1


def test_a_run_from_the_written_landmarks_gives_the_same_files(cli_run):
    a, b = cli_run["r50"], cli_run["r50_landmarks"]
    for name in cli_run["imgs"]:
        assert (a / name).read_bytes() == (b / name).read_bytes(), name
    ra, rb = (json.loads((d / "report.json").read_text()) for d in (a, b))
    assert [(p["photo"], p["faces"]) for p in ra["photos"]] == [(p["photo"], p["faces"]) for p in rb["photos"]]
    assert "detect" not in rb and not (b / "landmarks.json").exists()


def test_the_detector_cli_writes_the_same_landmarks(cli_run):
    alone = json.loads((cli_run["tmp"] / "alone_r50.json").read_text())
    rep = json.loads((cli_run["r50"] / "report.json").read_text())
    used = json.loads((cli_run["r50"] / "landmarks.json").read_text())
    for p in rep["photos"]:
        dropped = {d["face"] for d in p.get("dropped", [])}
        kept = [f for j, f in enumerate(alone.get(p["photo"], [])) if j not in dropped]
        assert kept == used.get(p["photo"], []), p["photo"]


def test_a_mobilenet_file_writes_the_files_it_wrote_before(cli_run):
    from vspbfr_amd import detect
    a, b = cli_run["mnet"], cli_run["mnet_direct"]
    for name in list(cli_run["imgs"]) + ["report.json", "landmarks.json"]:
        assert (a / name).read_bytes() == (b / name).read_bytes(), name
    assert "backbone" not in json.loads((a / "report.json").read_text())["detect"]
    det = detect.RetinaFaceDetector(str(cli_run["ck"] / "retinaface_mnet.pth"), "cuda")
    names = sorted(cli_run["imgs"])
    res = det.detect(photos=[cli_run["imgs"][n] for n in names], threshold=0.5, max_faces=2, side=256)
    want = detect.landmarks_json({n: list(d["landmarks"]) for n, d in zip(names, res) if len(d["landmarks"])})
    assert (cli_run["tmp"] / "alone_mnet.json").read_text() == want
