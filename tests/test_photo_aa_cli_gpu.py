"""GPU, end to end: `python -m vspbfr_amd.restore_photos --antialias` on three photos -- one with an 820 px face (shrunk 1.6 times into the
crop), one with a 150 px face (its restored crop shrunk 3.4 times on the way back) beside a face at scale, one without an entry -- with
random-weight checkpoints, at upscale 1 and 2: every written file equals tests/photo_aa_ref.py, and report.json lists the minifications.
Without the flag the case of tests/test_photo_cli_gpu.py gives the bytes of tests/photo_ref.py, as before, and the report has no new key."""
import json
import os
import random
from argparse import Namespace

import numpy as np
import pytest
import torch

import photo_aa_ref as AA
import photo_ref as R

pytestmark = pytest.mark.gpu
SEED = 123
MODEL = ["--timesteps", "4", "--no_sample", "--batch", "2"]


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


@pytest.fixture(scope="module")
def cli_run(tmp_path_factory):
    from PIL import Image
    from vspbfr_amd import restore_photos
    from vspbfr_amd.diffusion import Code_diffuser
    from vspbfr_amd.e4e import Encoder4Editing, Generator
    from vspbfr_amd.restorenet import Restoration_net
    tmp = tmp_path_factory.mktemp("photo_aa_cli")
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
    runs = {}
    # the anti-aliased case
    imgs = {"a_large.png": R.test_photo(900, 1000, seed=51), "b_small.png": R.test_photo(300, 260, seed=52),
            "sub/c_plain.png": R.test_photo(123, 77, seed=53)}
    marks = {"a_large.png": [R.landmarks_for(1 / 1.6, 12.0, (450.0, 520.0)).tolist()],
             "b_small.png": [R.landmarks_for(3.4, -8.0, (100.0, 120.0)).tolist(), R.landmarks_for(1.0, 5.0, (190.0, 130.0)).tolist()]}
    # the case of tests/test_photo_cli_gpu.py, for the run without the flag
    old_imgs = {"a_aligned.png": R.test_photo(512, 512, seed=21), "b_group.png": R.test_photo(700, 900, seed=22),
                "sub/c_plain.png": R.test_photo(123, 77, seed=23)}
    old_marks = {"a_aligned.png": [R.FFHQ512_TEMPLATE.tolist()],
                 "b_group.png": [R.landmarks_for(1.6, 12.0, (300.0, 420.0)).tolist(), R.landmarks_for(1.3, -8.0, (470.0, 520.0)).tolist()]}
    for case, (im, mk) in (("aa", (imgs, marks)), ("old", (old_imgs, old_marks))):
        root = tmp / f"photos_{case}"
        (root / "sub").mkdir(parents=True)
        for name, a in im.items():
            Image.fromarray(a).save(root / name)
        (tmp / f"landmarks_{case}.json").write_text(json.dumps(mk))
        runs[case] = {"imgs": im, "marks": {k: [np.asarray(p) for p in v] for k, v in mk.items()}}
    for tag, case, extra in (("x1", "aa", ["--antialias"]), ("x2", "aa", ["--antialias", "--upscale", "2"]), ("plain", "old", [])):
        torch.manual_seed(SEED)
        random.seed(SEED)
        out = tmp / tag
        restore_photos.main(MODEL + weights + ["--photos", str(tmp / f"photos_{case}"), "--landmarks", str(tmp / f"landmarks_{case}.json"),
                                               "--out", str(out), "--save_faces"] + extra)
        runs[tag] = out
    runs["tmp"], runs["weights"] = tmp, weights
    return runs


def _faces(marks, out, name, upscale):
    stem = os.path.splitext(name)[0]
    return [(_png(out / f"{stem}_{k}_restore.png"), R.paste_matrix(R.similarity(pts), upscale)) for k, pts in enumerate(marks.get(name, []))]


def test_report_lists_the_minifications(cli_run):
    for tag, s in (("x1", 1), ("x2", 2)):
        rep = json.loads((cli_run[tag] / "report.json").read_text())
        assert [(p["photo"], p["faces"]) for p in rep["photos"]] == [("a_large.png", 1), ("b_small.png", 2), ("sub/c_plain.png", 0)]
        a, b, c = rep["photos"]
        assert a["crop_minify"] == pytest.approx([1.6], abs=1e-5) and a["paste_minify"] == pytest.approx([1 / 1.6 / s], abs=1e-5)
        assert b["crop_minify"] == pytest.approx([1 / 3.4, 1.0], abs=1e-5) and b["paste_minify"] == pytest.approx([3.4 / s, 1.0 / s], abs=1e-5)
        assert c["crop_minify"] == [] and c["paste_minify"] == []


def test_saved_crops_are_the_anti_aliased_reference_crop(cli_run):
    imgs, marks = cli_run["aa"]["imgs"], cli_run["aa"]["marks"]
    ref = {(name, k): AA.crop(imgs[name], R.similarity(pts), 512) for name, per in marks.items() for k, pts in enumerate(per)}
    plain = R.crop(imgs["a_large.png"], R.invert(R.similarity(marks["a_large.png"][0])), 512)
    assert not np.array_equal(ref[("a_large.png", 0)], plain)                    # the filter does change the large face's crop
    for tag in ("x1", "x2"):
        for (name, k), want in ref.items():
            got = _png(cli_run[tag] / f"{os.path.splitext(name)[0]}_{k}_crop.png")
            print(f"{tag} {name} face {k}: differing bytes {int((got != want).sum())}")
            assert np.array_equal(got, want), (tag, name, k)


def test_output_photos_are_the_anti_aliased_reference_paste(cli_run):
    from PIL import Image
    imgs, marks = cli_run["aa"]["imgs"], cli_run["aa"]["marks"]
    for tag, s in (("x1", 1), ("x2", 2)):
        out = cli_run[tag]
        for name, photo in imgs.items():
            h, w = photo.shape[:2]
            bg = photo if s == 1 else np.asarray(Image.fromarray(photo).resize((2 * w, 2 * h), Image.Resampling.LANCZOS))
            got = _png(out / name)
            faces = _faces(marks, out, name, s)
            ref = AA.paste(bg, faces, 512)
            print(f"{tag} {name}: differing bytes {int((got != ref).sum())}, changed pixels {int((ref != bg).any(axis=2).sum())}")
            assert np.array_equal(got, ref), (tag, name)
    assert np.array_equal(_png(cli_run["x1"] / "sub/c_plain.png"), imgs["sub/c_plain.png"])


def test_without_the_flag_the_bytes_are_the_bilinear_ones(cli_run):
    imgs, marks, out = cli_run["old"]["imgs"], cli_run["old"]["marks"], cli_run["plain"]
    rep = json.loads((out / "report.json").read_text())
    assert all(sorted(p) == ["faces", "output", "photo", "size"] for p in rep["photos"])
    assert sorted(rep) == ["crop_size", "feather", "inset", "photos", "upscale"]
    for name, photo in imgs.items():
        for k, pts in enumerate(marks.get(name, [])):
            assert np.array_equal(_png(out / f"{os.path.splitext(name)[0]}_{k}_crop.png"), R.crop(photo, R.invert(R.similarity(pts)), 512)), (name, k)
        assert np.array_equal(_png(out / name), R.paste(photo, _faces(marks, out, name, 1), 512)), name
    assert np.array_equal(_png(out / "a_aligned_0_crop.png"), imgs["a_aligned.png"])


def test_a_minification_above_sixteen_is_refused_before_any_model_is_loaded(cli_run, capsys):
    from PIL import Image
    from vspbfr_amd import restore_photos
    tmp = cli_run["tmp"]
    root = tmp / "photos_big"
    root.mkdir()
    Image.fromarray(R.test_photo(64, 64, seed=1)).save(root / "tiny.png")
    (tmp / "landmarks_big.json").write_text(json.dumps({"tiny.png": [R.landmarks_for(17.0, 0.0, (30.0, 30.0)).tolist()]}))
    args = ["--photos", str(root), "--landmarks", str(tmp / "landmarks_big.json"), "--out", str(tmp / "big"), "--ckpt", "/nonexistent.pt",
            "--ddpm_ckpt", "/nonexistent.pt", "--psp_checkpoint_path", "/nonexistent.pt", "--antialias"]
    with pytest.raises(SystemExit):
        restore_photos.main(args)
    assert "tiny.png" in capsys.readouterr().err and not (tmp / "big").exists()
