"""The inputs of tests/test_parse_cli_gpu.py, built from fixed seeds: random-weight checkpoints of every model the CLIs load, three small
photos and one landmark file -- and the two runs of `python -m vspbfr_amd.restore_photos` WITHOUT --parse_weights whose output directories
are pinned byte for byte in tests/golden/parse_cli_parent.json, recorded from the commit before the face parser existed."""
import hashlib
import json
import os
import random
from argparse import Namespace

import torch

import detect_cases as K
import photo_ref as P0
import sr_ref

SEED = 123
MODEL = ["--timesteps", "4", "--no_sample", "--batch", "1"]
GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "parse_cli_parent.json")


def build_inputs(tmp):
    """-> dict(imgs, marks, ck, photos, base): checkpoints under tmp/ckpt, photos under tmp/photos, tmp/landmarks.json; `base` holds the
    arguments every run shares"""
    from PIL import Image
    from vspbfr_amd.diffusion import Code_diffuser
    from vspbfr_amd.e4e import Encoder4Editing, Generator
    from vspbfr_amd.restorenet import Restoration_net
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
    torch.save({"params_ema": sr_ref.make_state(2, 2, seed=11)}, ck / "sr_x2.pth")
    weights = ["--ckpt", str(ck / "restoration_net.pt"), "--ddpm_ckpt", str(ck / "code_diffuser.pt"), "--psp_checkpoint_path",
               str(ck / "style_encoder_decoder.pt")]
    photos = tmp / "photos"
    (photos / "sub").mkdir(parents=True)
    imgs = {"a.png": P0.test_photo(200, 260, seed=31), "sub/b.png": P0.test_photo(300, 240, seed=32), "c.png": P0.test_photo(64, 48, seed=33)}
    for name, a in imgs.items():
        Image.fromarray(a).save(photos / name)
    marks = {"a.png": [P0.landmarks_for(4.0, 12.0, (100.0, 130.0)).tolist()], "sub/b.png": [P0.landmarks_for(3.0, -8.0, (150.0, 120.0)).tolist()]}
    (tmp / "landmarks.json").write_text(json.dumps(marks))
    return {"imgs": imgs, "marks": marks, "ck": ck, "photos": photos, "base": MODEL + weights + ["--photos", str(photos)]}


def unflagged_runs(tmp, case):
    """{tag: arguments} of the two pinned runs without --parse_weights: the plain one, and one with every other option of the paste path
    (upscale 2 over a background network, the anti-aliased entries, a colour fix, the device's PNG encoder)"""
    lm = ["--landmarks", str(tmp / "landmarks.json"), "--save_faces"]
    return {"plain": lm, "combo": lm + ["--upscale", "2", "--color_fix", "wavelet", "--antialias", "--bg_weights", str(case["ck"] / "sr_x2.pth"),
                                        "--png_encode", "device"]}


def run_cli(main, case, out, extra):
    torch.manual_seed(SEED)
    random.seed(SEED)
    main(case["base"] + ["--out", str(out)] + extra)
    return out


def hash_dir(root):
    """{relative path: sha256 of the file's bytes}"""
    out = {}
    for dp, _, fs in os.walk(root):
        for f in fs:
            p = os.path.join(dp, f)
            with open(p, "rb") as fh:
                out[os.path.relpath(p, root).replace(os.sep, "/")] = hashlib.sha256(fh.read()).hexdigest()
    return dict(sorted(out.items()))
