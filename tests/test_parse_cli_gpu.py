"""GPU, end to end: both CLIs of the face-parsing paste mask on small photos with random-weight checkpoints (set up as in
tests/test_sr_cli_gpu.py; tests/parse_cli_case.py builds them).  Without --parse_weights the output directory equals, byte for byte,
what the commit before the parser wrote (tests/golden/parse_cli_parent.json).  `python -m vspbfr_amd.restore_photos --landmarks
--save_faces` with and without --parse_weights: the mask
and class files, the `parse` block and `mask_mean` in report.json, the photo equal to the restatement's masked paste of the written
crops through the written class map; --parse_weights together with --detect_weights, --color_fix wavelet, --antialias, --bg_weights and
--png_encode device; `python -m vspbfr_amd.parse` on the restored crops of the first run, which must give the files of that run."""
import json
import os

import numpy as np
import pytest
import torch

import parse_cli_case as C
import parse_ref as R
import photo_ref as P0

pytestmark = pytest.mark.gpu


def _img(path, mode="RGB"):
    from PIL import Image
    return np.asarray(Image.open(path).convert(mode))


def _files(root):
    return sorted(os.path.relpath(os.path.join(dp, f), root) for dp, _, fs in os.walk(root) for f in fs)


@pytest.fixture(scope="module")
def cli_run(tmp_path_factory):
    from PIL import Image
    from vspbfr_amd import parse, restore_photos
    tmp = tmp_path_factory.mktemp("parse_cli")
    case = C.build_inputs(tmp)
    ck = case["ck"]
    state = R.make_state(seed=21)
    torch.save({"module." + k: v for k, v in state.items()}, ck / "parsenet.pth")
    runs = {"imgs": case["imgs"], "marks": case["marks"], "state": state, "tmp": tmp}
    unflagged = C.unflagged_runs(tmp, case)
    lm = unflagged["plain"]
    for tag, extra in (("plain", lm), ("combo", unflagged["combo"]), ("parse", lm + ["--parse_weights", str(ck / "parsenet.pth")]),
                       ("all", ["--detect_weights", str(ck / "retinaface.pt"), "--detect_threshold", "0.5", "--detect_max_faces", "2", "--upscale", "2",
                                "--parse_weights", str(ck / "parsenet.pth"), "--parse_sigma", "7.5", "--parse_border", "4", "--color_fix", "wavelet",
                                "--antialias", "--bg_weights", str(ck / "sr_x2.pth"), "--png_encode", "device", "--save_faces"])):
        runs[tag] = C.run_cli(restore_photos.main, case, tmp / tag, extra)
    faces = tmp / "faces"
    faces.mkdir()
    for name in ("a_0_restore.png", "sub/b_0_restore.png"):
        Image.fromarray(_img(tmp / "parse" / name)).save(faces / name.replace("/", "_"))
    parse.main(["--faces", str(faces), "--weights", str(ck / "parsenet.pth"), "--out", str(tmp / "own")])
    return runs


@pytest.mark.parametrize("tag", ["plain", "combo"])
def test_without_the_flag_the_output_directory_is_the_parent_commits_byte_for_byte(cli_run, tag):
    """tests/golden/parse_cli_parent.json holds the sha256 of every file the commit before the face parser wrote for these seeded inputs:
    the plain run, and one with --upscale 2, --bg_weights, --antialias, --color_fix wavelet and --png_encode device (photos, crops,
    restored and fixed crops, report.json).  Every layer of the unflagged path -- the Python around the entries as well as the kernels --
    must still write exactly those bytes."""
    golden = json.loads(open(C.GOLDEN).read())
    assert C.hash_dir(cli_run["tmp"] / "photos") == golden["inputs"]                 # the seeded inputs are the recorded ones
    got = C.hash_dir(cli_run[tag])
    assert sorted(got) == sorted(golden[tag]), sorted(set(got) ^ set(golden[tag]))
    assert got == golden[tag], [f for f in got if got[f] != golden[tag][f]]


def test_the_run_without_the_flag_has_no_trace_of_the_parser(cli_run):
    a, b = cli_run["plain"], cli_run["parse"]
    want = ["a.png", "a_0_crop.png", "a_0_restore.png", "c.png", "report.json", "sub/b.png", "sub/b_0_crop.png", "sub/b_0_restore.png"]
    assert _files(a) == want
    assert _files(b) == sorted(want + ["a_0_mask.png", "a_0_parse.png", "sub/b_0_mask.png", "sub/b_0_parse.png"])
    ra, rb = (json.loads((d / "report.json").read_text()) for d in (a, b))
    assert "parse" not in ra and all("mask_mean" not in p for p in ra["photos"])
    assert rb["parse"] == {"model": "ParseNet", "sigma": 11.0, "radius": 50, "border": 10, "nonfinite": []}
    assert [(p["photo"], p["faces"], len(p.get("mask_mean", []))) for p in rb["photos"]] == [("a.png", 1, 1), ("c.png", 0, 0), ("sub/b.png", 1, 1)]
    assert all(0 < p["mask_mean"][0] < 1 for p in rb["photos"] if p["faces"])
    # the same seeds: the crops and the network's output do not depend on the flag, the photo does
    for name in ("a_0_crop.png", "a_0_restore.png", "sub/b_0_restore.png", "c.png"):
        assert np.array_equal(_img(a / name), _img(b / name)), name
    assert not np.array_equal(_img(a / "a.png"), _img(b / "a.png"))


def test_the_photo_is_the_masked_paste_of_the_written_files(cli_run):
    from vspbfr_amd import parse as P
    out = cli_run["parse"]
    rep = {p["photo"]: p for p in json.loads((out / "report.json").read_text())["photos"]}
    for name, stem in (("a.png", "a"), ("sub/b.png", "sub/b")):
        cls = _img(out / f"{stem}_0_parse.png", "L")
        assert cls.shape == (512, 512) and cls.max() <= 18 and len(np.unique(cls)) >= 3
        mask = R.paste_weights(R.KEEP[cls][None], P.default_taps(512), P.default_border(512))[0]
        assert np.array_equal(_img(out / f"{stem}_0_mask.png", "L"), ((mask.astype(np.int64) * 255 + 128) >> 8).astype(np.uint8))
        assert abs(rep[name]["mask_mean"][0] - mask.mean() / 256) < 1e-5
        Pm = P0.paste_matrix(P0.similarity(np.asarray(cli_run["marks"][name][0]), 512), 1)
        ref = R.paste_masked(cli_run["imgs"][name], [(_img(out / f"{stem}_0_restore.png"), Pm, mask)], 512)
        assert np.array_equal(_img(out / name), ref), name
    assert np.array_equal(_img(out / "c.png"), cli_run["imgs"]["c.png"])


def test_everything_together_still_runs(cli_run):
    out = cli_run["all"]
    rep = json.loads((out / "report.json").read_text())
    assert rep["parse"] == {"model": "ParseNet", "sigma": 7.5, "radius": 50, "border": 4, "nonfinite": []}
    assert rep["upscale"] == 2 and rep["png_encode"] == "device" and "detect" in rep and "background" in rep and rep["color_fix"] == "wavelet"
    for name, src in cli_run["imgs"].items():
        assert _img(out / name).shape == (2 * src.shape[0], 2 * src.shape[1], 3)
    for p in rep["photos"]:
        assert len(p.get("mask_mean", [])) == p["faces"] or p["faces"] == 0
    print("faces found:", [(p["photo"], p["faces"], p.get("mask_mean")) for p in rep["photos"]])


def test_the_parse_cli_gives_the_files_of_the_restore_run(cli_run):
    tmp = cli_run["tmp"]
    assert _files(tmp / "own") == ["a_0_restore_mask.png", "a_0_restore_parse.png", "sub_b_0_restore_mask.png", "sub_b_0_restore_parse.png"]
    for own, theirs in (("a_0_restore", "a_0"), ("sub_b_0_restore", "sub/b_0")):
        for kind in ("mask", "parse"):
            assert np.array_equal(_img(tmp / "own" / f"{own}_{kind}.png", "L"), _img(cli_run["parse"] / f"{theirs}_{kind}.png", "L")), (own, kind)
