"""GPU, end to end: `python -m vspbfr_amd.restore_photos` on three photos -- a 512 x 512 one whose landmarks are the template, a 700 x 900
one with two overlapping faces, one without an entry in the landmarks file -- with random-weight checkpoints, at upscale 1 and 2.  The
written photos equal tests/photo_ref.py's paste of the written `*_restore.png` crops byte for byte, the `*_crop.png` files equal its
crop, and the template-aligned face's restoration equals what `vspbfr_amd.restoration_metrics` writes for the same image and seeds."""
import json
import os
import random
from argparse import Namespace

import numpy as np
import pytest
import torch

import photo_ref as R

pytestmark = pytest.mark.gpu
SEED = 123
MODEL = ["--timesteps", "4", "--no_sample", "--batch", "1"]


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


@pytest.fixture(scope="module")
def cli_run(tmp_path_factory):
    from PIL import Image
    from vspbfr_amd import restoration_metrics, restore_photos
    from vspbfr_amd.diffusion import Code_diffuser
    from vspbfr_amd.e4e import Encoder4Editing, Generator
    from vspbfr_amd.restorenet import Restoration_net
    tmp = tmp_path_factory.mktemp("photo_cli")
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
    photos = tmp / "photos"
    (photos / "sub").mkdir(parents=True)
    imgs = {"a_aligned.png": R.test_photo(512, 512, seed=21), "b_group.png": R.test_photo(700, 900, seed=22),
            "sub/c_plain.png": R.test_photo(123, 77, seed=23)}
    for name, a in imgs.items():
        Image.fromarray(a).save(photos / name)
    marks = {"a_aligned.png": [R.FFHQ512_TEMPLATE.tolist()],
             "b_group.png": [R.landmarks_for(1.6, 12.0, (300.0, 420.0)).tolist(), R.landmarks_for(1.3, -8.0, (470.0, 520.0)).tolist()]}
    (tmp / "landmarks.json").write_text(json.dumps(marks))
    # the aligned photo alone through the aligned-face CLI, twice with the same seeds
    lq = tmp / "lq"
    lq.mkdir()
    Image.fromarray(imgs["a_aligned.png"]).save(lq / "a_aligned.png")
    runs = {"imgs": imgs, "marks": {k: [np.asarray(p) for p in v] for k, v in marks.items()}}
    for tag in ("metrics_1", "metrics_2"):
        torch.manual_seed(SEED)
        random.seed(SEED)
        out = tmp / tag
        restoration_metrics.main(MODEL + weights + ["--eval_dir", str(out), "--lq_data_list", str(lq), "--hq_data_list", "None",
                                                    "--data_name_list", "demo"])
        runs[tag] = _png(out / "restoration_net" / "0" / "demo" / "000000_0_demo_restore.png")
    for tag, extra in (("x1", []), ("x2", ["--upscale", "2"])):
        torch.manual_seed(SEED)
        random.seed(SEED)
        out = tmp / tag
        restore_photos.main(MODEL + weights + ["--photos", str(photos), "--landmarks", str(tmp / "landmarks.json"), "--out", str(out),
                                               "--save_faces"] + extra)
        runs[tag] = out
    return runs


def _faces(runs, out, name, upscale):
    stem = os.path.splitext(name)[0]
    return [(_png(out / f"{stem}_{k}_restore.png"), R.paste_matrix(R.similarity(pts), upscale)) for k, pts in enumerate(runs["marks"].get(name, []))]


def _outside(runs, name, shape, upscale):
    """mask of the pixels outside every face's bounding box"""
    m = np.ones(shape[:2], dtype=bool)
    for pts in runs["marks"].get(name, []):
        x0, y0, x1, y1 = R.bbox(R.paste_matrix(R.similarity(pts), upscale), 512, shape[0], shape[1])
        m[y0:y1, x0:x1] = False
    return m


def test_files_and_report(cli_run):
    for tag in ("x1", "x2"):
        out = cli_run[tag]
        have = sorted(os.path.relpath(os.path.join(dp, f), out) for dp, _, fs in os.walk(out) for f in fs)
        want = ["a_aligned.png", "a_aligned_0_crop.png", "a_aligned_0_restore.png", "b_group.png", "b_group_0_crop.png", "b_group_0_restore.png",
                "b_group_1_crop.png", "b_group_1_restore.png", "report.json", "sub/c_plain.png"]
        assert have == want
        rep = json.loads((out / "report.json").read_text())
        assert [(p["photo"], p["faces"]) for p in rep["photos"]] == [("a_aligned.png", 1), ("b_group.png", 2), ("sub/c_plain.png", 0)]
        assert rep["upscale"] == (1 if tag == "x1" else 2) and rep["crop_size"] == 512


def test_output_photos_are_the_reference_paste_of_the_saved_restorations(cli_run):
    out = cli_run["x1"]
    for name, photo in cli_run["imgs"].items():
        got = _png(out / name)
        ref = R.paste(photo, _faces(cli_run, out, name, 1), 512)
        print(f"{name}: differing bytes {int((got != ref).sum())}, changed pixels {int((ref != photo).any(axis=2).sum())}")
        assert np.array_equal(got, ref), name
        m = _outside(cli_run, name, photo.shape, 1)
        assert np.array_equal(got[m], photo[m]), name                            # outside every bounding box: the input
    assert np.array_equal(_png(out / "sub/c_plain.png"), cli_run["imgs"]["sub/c_plain.png"])      # written through
    assert not np.array_equal(_png(out / "b_group.png"), cli_run["imgs"]["b_group.png"])


def test_saved_crops_are_the_reference_crop(cli_run):
    for tag in ("x1", "x2"):
        out = cli_run[tag]
        for name, marks in cli_run["marks"].items():
            for k, pts in enumerate(marks):
                got = _png(out / f"{os.path.splitext(name)[0]}_{k}_crop.png")
                assert np.array_equal(got, R.crop(cli_run["imgs"][name], R.invert(R.similarity(pts)), 512)), (tag, name, k)
        assert np.array_equal(_png(out / "a_aligned_0_crop.png"), cli_run["imgs"]["a_aligned.png"])   # template landmarks: the photo itself


def test_upscale_two_doubles_the_photos_over_a_lanczos_background(cli_run):
    from PIL import Image
    out = cli_run["x2"]
    for name, photo in cli_run["imgs"].items():
        h, w = photo.shape[:2]
        got = _png(out / name)
        assert got.shape == (2 * h, 2 * w, 3)
        bg = np.asarray(Image.fromarray(photo).resize((2 * w, 2 * h), Image.Resampling.LANCZOS))
        m = _outside(cli_run, name, got.shape, 2)
        assert np.array_equal(got[m], bg[m]), name
        ref = R.paste(bg, _faces(cli_run, out, name, 2), 512)
        print(f"{name} x2: differing bytes {int((got != ref).sum())}")
        assert np.array_equal(got, ref), name
    assert np.array_equal(_png(out / "a_aligned_0_restore.png"), _png(cli_run["x1"] / "a_aligned_0_restore.png"))


def test_template_aligned_face_restores_as_the_aligned_face_cli_does(cli_run):
    """restoration_metrics at --batch 1 is bit-reproducible run to run with the same seeds (asserted first); the whole-photo CLI hands the
    pipeline the same tensor under the same seeds, so its restored crop is that file's pixels"""
    a, b = cli_run["metrics_1"], cli_run["metrics_2"]
    print(f"restoration_metrics run to run: max |diff| {int(np.abs(a.astype(int) - b.astype(int)).max())}")
    assert np.array_equal(a, b)
    got = _png(cli_run["x1"] / "a_aligned_0_restore.png")
    print(f"restore_photos vs restoration_metrics: max |diff| {int(np.abs(got.astype(int) - a.astype(int)).max())}")
    assert np.array_equal(got, a)
