"""GPU, end to end: `python -m vspbfr_amd.restore_photos --save_faces --color_fix wavelet` and `stats` on three small photos -- one whose
face hangs off two edges, one with two faces, one without an entry -- with random-weight checkpoints: every _fixed.png equals
tests/color_fix_ref.py applied to that run's _crop.png and _restore.png, every output photo equals tests/photo_ref.py's paste of the fixed
crops, _crop.png and _restore.png equal those of a run without the flag, and `--color_fix none` writes the same files, byte for byte, as
no flag at all (report.json included)."""
import json
import os
import random
from argparse import Namespace

import numpy as np
import pytest
import torch

import color_fix_ref as CF
import photo_ref as R

pytestmark = pytest.mark.gpu
SEED = 123
MODEL = ["--timesteps", "4", "--no_sample", "--batch", "2"]


def _png(path):
    from PIL import Image
    return np.asarray(Image.open(path).convert("RGB"))


def _files(root):
    return sorted(os.path.relpath(os.path.join(dp, f), root) for dp, _, fs in os.walk(root) for f in fs)


@pytest.fixture(scope="module")
def cli_run(tmp_path_factory):
    from PIL import Image
    from vspbfr_amd import restore_photos
    from vspbfr_amd.diffusion import Code_diffuser
    from vspbfr_amd.e4e import Encoder4Editing, Generator
    from vspbfr_amd.restorenet import Restoration_net
    tmp = tmp_path_factory.mktemp("color_fix_cli")
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
    marks = {"a_edge.png": [R.landmarks_for(2.0, 12.0, (40.0, 50.0)).tolist()],              # over the left and the top edge
             "b_pair.png": [R.landmarks_for(2.4, -8.0, (150.0, 160.0)).tolist(), R.landmarks_for(3.0, 5.0, (300.0, 170.0)).tolist()]}
    root = tmp / "photos"
    (root / "sub").mkdir(parents=True)
    for name, a in imgs.items():
        Image.fromarray(a).save(root / name)
    (tmp / "landmarks.json").write_text(json.dumps(marks))
    runs = {"imgs": imgs, "marks": {k: [np.asarray(p) for p in v] for k, v in marks.items()}, "tmp": tmp}
    for tag, extra in (("plain", []), ("none", ["--color_fix", "none"]), ("wavelet", ["--color_fix", "wavelet"]),
                       ("stats", ["--color_fix", "stats", "--color_levels", "3"])):
        torch.manual_seed(SEED)
        random.seed(SEED)
        out = tmp / tag
        restore_photos.main(MODEL + weights + ["--photos", str(root), "--landmarks", str(tmp / "landmarks.json"), "--out", str(out),
                                               "--save_faces"] + extra)
        runs[tag] = out
    return runs


def _each_face(runs):
    for name, per in runs["marks"].items():
        h, w = runs["imgs"][name].shape[:2]
        for k, pts in enumerate(per):
            yield name, os.path.splitext(name)[0], k, pts, CF.validity_from_landmarks(pts, 512, w, h)


@pytest.mark.parametrize("mode", ["wavelet", "stats"])
def test_fixed_crops_equal_the_restatement(cli_run, mode):
    out = cli_run[mode]
    partly = 0
    for name, stem, k, pts, valid in _each_face(cli_run):
        crop, restored, fixed = (_png(out / f"{stem}_{k}_{what}.png") for what in ("crop", "restore", "fixed"))
        want = CF.fix(crop, restored, mode, valid)
        print(f"{mode} {name} face {k}: valid {int(valid.sum())} of {valid.size}, differing bytes {int((fixed != want).sum())}, "
              f"moved by the fix {float((want != restored).mean()):.3f}")
        assert np.array_equal(fixed, want), (name, k)
        assert not np.array_equal(fixed, restored)
        partly += 0 < valid.sum() < valid.size
    assert partly == 1                                                        # the face over the edge


@pytest.mark.parametrize("mode", ["wavelet", "stats"])
def test_output_photos_are_the_paste_of_the_fixed_crops(cli_run, mode):
    out = cli_run[mode]
    for name, photo in cli_run["imgs"].items():
        stem = os.path.splitext(name)[0]
        faces = [(_png(out / f"{stem}_{k}_fixed.png"), R.paste_matrix(R.similarity(pts), 1)) for k, pts in enumerate(cli_run["marks"].get(name, []))]
        got, ref = _png(out / name), R.paste(photo, faces, 512)
        print(f"{mode} {name}: differing bytes {int((got != ref).sum())}, changed pixels {int((ref != photo).any(axis=2).sum())}")
        assert np.array_equal(got, ref), name
        if faces:
            assert not np.array_equal(got, _png(cli_run["plain"] / name))    # the fix does reach the photo


@pytest.mark.parametrize("mode", ["wavelet", "stats"])
def test_crop_and_restore_files_are_those_of_a_run_without_the_flag(cli_run, mode):
    plain, out = cli_run["plain"], cli_run[mode]
    assert [f for f in _files(out) if not f.endswith("_fixed.png")] == _files(plain)
    assert len([f for f in _files(out) if f.endswith("_fixed.png")]) == 3
    for f in _files(plain):
        if f.endswith(("_crop.png", "_restore.png")):
            assert (out / f).read_bytes() == (plain / f).read_bytes(), f
    rep, old = json.loads((out / "report.json").read_text()), json.loads((plain / "report.json").read_text())
    assert rep.pop("color_fix") == mode and rep.pop("color_levels") == (5 if mode == "wavelet" else 3) and rep == old


def test_color_fix_none_writes_what_no_flag_writes(cli_run):
    plain, none = cli_run["plain"], cli_run["none"]
    assert _files(none) == _files(plain) and "report.json" in _files(plain) and not any("fixed" in f for f in _files(plain))
    for f in _files(plain):
        assert (none / f).read_bytes() == (plain / f).read_bytes(), f
    assert sorted(json.loads((plain / "report.json").read_text())) == ["crop_size", "feather", "inset", "photos", "upscale"]


def test_bad_flags_are_refused_before_any_model_is_loaded(cli_run, capsys):
    from vspbfr_amd import restore_photos
    tmp = cli_run["tmp"]
    base = ["--photos", str(tmp / "photos"), "--landmarks", str(tmp / "landmarks.json"), "--out", str(tmp / "bad"), "--ckpt", "/nonexistent.pt",
            "--ddpm_ckpt", "/nonexistent.pt", "--psp_checkpoint_path", "/nonexistent.pt"]
    for extra, text in ((["--color_fix", "wavelet", "--color_levels", "7"], "levels"), (["--color_fix", "adain"], "invalid choice")):
        with pytest.raises(SystemExit):
            restore_photos.main(base + extra)
        assert text in capsys.readouterr().err and not (tmp / "bad").exists()
