"""CPU checks of the face detector: the checkpoint's key layout and the loader's rules, the BatchNorm fold, prior counts, the
NumPy restatement of the post-processing on hand-made boxes, the JSON writer, the parsers, the entries' refusals, and the margins of the
case the GPU detection test runs."""
import ctypes as C
import json

import numpy as np
import pytest
import torch

import detect_cases as K
import detect_ref as R


def test_key_layout_and_loader_rules():
    from vspbfr_amd import detect as D
    sd = K.model().state_dict()
    assert len(sd) == 300 and set(sd) == set(D.expected_state())
    assert {k: tuple(v.shape) for k, v in sd.items()} == {k: tuple(s) for k, s in D.expected_state().items()}
    clean = D.check_state_dict({"module." + k: v for k, v in sd.items()})
    assert len(clean) == 300 - 47 and not any(k.startswith("module.") or k.endswith("num_batches_tracked") for k in clean)
    assert "ssh2.conv7x7_3.0.weight" in clean and "ssh2.conv7X7_2.0.weight" in clean
    bad = dict(sd)
    del bad["fpn.merge2.1.running_var"]
    bad["body.stage9.0.weight"] = torch.zeros(1)
    with pytest.raises(ValueError) as e:
        D.check_state_dict(bad)
    assert "missing keys fpn.merge2.1.running_var" in str(e.value) and "unexpected keys body.stage9.0.weight" in str(e.value)
    bad = dict(sd)
    bad["BboxHead.1.conv1x1.bias"] = torch.zeros(4)
    with pytest.raises(ValueError, match="BboxHead.1.conv1x1.bias has shape"):
        D.check_state_dict(bad)


def test_bn_fold_equals_the_unfused_tree_in_float64():
    from vspbfr_amd import detect as D
    net = K.model()
    folded = D.fold_state(D.check_state_dict(net.state_dict()))
    assert all(v.dtype == torch.float64 for v in folded.values())
    x = R.canvas(K.detection_case()["canvas_photos"], K.HC, K.WC)
    got = R.folded_forward(folded, x)
    for g, want, name in zip(got, K.detection_case()["o64"], ("conf", "loc", "lm")):
        err = float(np.abs(g.numpy() - want).max())
        print(f"fold {name}: max|d| = {err:.3e} of {float(np.abs(want).max()):.3e}")
        assert err <= 1e-12 * max(1.0, float(np.abs(want).max()))


@pytest.mark.parametrize("hw,want", [((96, 128), 504), ((97, 131), 608), ((1024, 1024), 43008), ((1, 1), 6)])
def test_prior_counts(hw, want):
    from vspbfr_amd import _lib, detect as D
    Hc, Wc = hw
    assert want == 2 * sum(-(-Hc // s) * -(-Wc // s) for s in (8, 16, 32))
    assert D.num_priors(Hc, Wc) == want == _lib.lib.vsp_det_priors(Hc, Wc) == len(R.priors(Hc, Wc)[0])
    cx, cy, m = R.priors(Hc, Wc)
    assert (cx[0], cy[0], m[0], m[1]) == (4.0, 4.0, 16.0, 32.0) and (cx[-1], m[-1]) == ((-(-Wc // 32) - 0.5) * 32, 512.0)


def _boxes(rows):
    """[(x1, y1, x2, y2, score)] -> score, box, pts of the restatement"""
    a = np.asarray(rows, dtype=np.float64)
    return a[:, 4].copy(), a[:, :4].copy(), np.zeros((len(a), 10))


def test_nms_restatement_on_hand_made_boxes():
    # a tie on the score goes to the lower prior index: 1 and 2 overlap fully, 1 is kept
    s, b, p = _boxes([(50, 50, 60, 60, 0.6), (0, 0, 10, 10, 0.9), (0, 0, 10, 10, 0.9), (100, 0, 110, 10, 0.2)])
    r = R.select_nms(s, b, p, 0.5, 0.4)
    assert list(r["order"]) == [1, 2, 0] and list(r["keep"]) == [1, 0] and r["status"] == 0 and r["candidates"] == 3
    # IoU exactly at the threshold is kept: 10 x 10 boxes shifted by 5 have IoU 50 / 150 = 1/3; so is a score exactly at the threshold dropped
    s, b, p = _boxes([(0, 0, 10, 10, 0.9), (5, 0, 15, 10, 0.8), (0, 0, 10, 10, 0.5)])
    assert R.iou_matrix(b)[0, 1] == 1.0 / 3.0
    assert list(R.select_nms(s, b, p, 0.5, 1.0 / 3.0)["keep"]) == [0, 1]
    assert list(R.select_nms(s, b, p, 0.5, np.nextafter(1.0 / 3.0, 0.0))["keep"]) == [0]
    # the caps set their status bits; a non-finite candidate is dropped and counted
    s, b, p = _boxes([(20 * k, 0, 20 * k + 10, 10, 0.9 - 0.01 * k) for k in range(8)])
    r = R.select_nms(s, b, p, 0.5, 0.4, max_candidates=6, max_faces=3)
    assert list(r["keep"]) == [0, 1, 2] and r["status"] == R.CAND_CAPPED | R.FACES_CAPPED and r["candidates"] == 8
    r = R.select_nms(s, b, p, 0.5, 0.4, max_candidates=8, max_faces=8)
    assert list(r["keep"]) == list(range(8)) and r["status"] == 0
    b[2, 1] = np.inf
    p[5, 3] = np.nan
    r = R.select_nms(s, b, p, 0.5, 0.4)
    assert list(r["keep"]) == [0, 1, 3, 4, 6, 7] and r["status"] == R.NONFINITE and r["nonfinite"] == 2 and r["candidates"] == 6


def test_decode_restatement_follows_the_formulas():
    conf, loc, lm = (np.zeros((504, n)) for n in (2, 4, 10))
    conf[7] = (0.0, np.log(3.0))
    loc[7] = (1.0, -2.0, np.log(2.0) / 0.2, 0.0)
    lm[7, 4:6] = (0.5, 0.25)
    score, box, pts = R.decode(conf, loc, lm, 96, 128)
    assert abs(score[7] - 0.75) < 1e-15 and abs(score[0] - 0.5) < 1e-15
    # prior 7: level 0, cell 3 (row 0, column 3), anchor 1 of size 32 -> centre (28, 4)
    assert np.allclose(box[7], (28 + 3.2 - 32, 4 - 6.4 - 16, 28 + 3.2 + 32, 4 - 6.4 + 16), atol=1e-12)
    assert np.allclose(pts[7, 4:6], (28 + 1.6, 4 + 0.8), atol=1e-12) and np.allclose(pts[7, 0:2], (28, 4))


def test_json_round_trip_is_exact():
    from vspbfr_amd import detect as D
    rng = np.random.default_rng(0)
    vals = np.concatenate([rng.uniform(-50, 4000, 500), [0.0, -0.5, 0.1, 1e-7, 16777216.0, 1234.5677]]).astype(np.float32)
    for v in vals:
        assert np.float32(json.loads(D.format_f32(v))) == v
    faces = {"a/b.png": [vals[:10].reshape(5, 2), vals[10:20].reshape(5, 2)], "c.jpg": [vals[-10:].reshape(5, 2)]}
    back = json.loads(D.landmarks_json(faces))
    assert list(back) == ["a/b.png", "c.jpg"] and len(back["a/b.png"]) == 2
    for name, fs in faces.items():
        for f, g in zip(fs, back[name]):
            assert np.array_equal(np.asarray(g, dtype=np.float32), f)
            assert np.array_equal(np.asarray(g, dtype=np.float64), D.as_json_floats(f))


def test_parser_errors(tmp_path, capsys):
    from vspbfr_amd import detect as D, restore_photos
    (tmp_path / "photos").mkdir()
    base = ["--photos", str(tmp_path / "photos"), "--out", str(tmp_path / "out")]
    for extra, msg in (([], "exactly one of --landmarks and --detect_weights"),
                       (["--landmarks", "x.json", "--detect_weights", "w.pt"], "exactly one of --landmarks and --detect_weights"),
                       (["--detect_weights", "w.pt", "--detect_threshold", "1.5"], "threshold 1.5 outside"),
                       (["--detect_weights", "w.pt", "--detect_max_faces", "0"], "max_faces 0"),
                       (["--detect_weights", str(tmp_path / "none.pt")], "no such file")):
        with pytest.raises(SystemExit) as e:
            restore_photos.main(base + extra)
        assert e.value.code == 2 and msg in capsys.readouterr().err, extra
    for extra, msg in ((["--nms", "-0.1"], "nms -0.1 outside"), (["--side", "8"], "side 8 outside"), ([], "no such file")):
        with pytest.raises(SystemExit) as e:
            D.main(["--photos", str(tmp_path / "photos"), "--weights", str(tmp_path / "none.pt"), "--out", str(tmp_path / "l.json")] + extra)
        assert e.value.code == 2 and msg in capsys.readouterr().err, extra


def test_entries_refuse_what_they_do_not_serve():
    """validation precedes every launch: no GPU needed"""
    from vspbfr_amd import _lib
    L, p = _lib.lib, C.c_void_p(256)
    for call, msg in ((lambda: L.vsp_det_sep_f32(p, p, p, p, p, p, 1, 8, 24, 5, 5, 1, 0.1, None), "multiple of 16"),
                      (lambda: L.vsp_det_sep_f32(p, p, p, p, p, p, 1, 8, 16, 5, 5, 3, 0.1, None), "stride 3"),
                      (lambda: L.vsp_det_sep_f32(p, p, p, p, p, p, 1, 512, 16, 5, 5, 1, 0.1, None), "Cin 512"),
                      (lambda: L.vsp_det_conv3x3_f32(p, p, p, p, 1, 64, 48, 5, 5, 48, 0, 0, 0.0, None), "Cout 48"),
                      (lambda: L.vsp_det_conv3x3_f32(p, p, p, p, 1, 64, 32, 5, 5, 48, 32, 0, 0.0, None), "channels 32..63 of 48"),
                      (lambda: L.vsp_det_lateral_f32(p, p, p, p, p, 1, 64, 5, 5, 6, 5, 1, 0.1, None), "coarser map"),
                      (lambda: L.vsp_det_heads_f32(p, p, p, p, p, p, 1, 5, 5, 40, 0, None), "priors 0..49 of 40"),
                      (lambda: L.vsp_det_entry_u8(p, p, 100, p, p, 2, p, p, 1, 64, 64, 1, 0.1, None), "2 items for a batch of 1"),
                      (lambda: L.vsp_det_decode_nms_f32(p, p, p, 0, p, p, p, 1, 96, 128, 1.0, 0.4, 1024, 8, None), "threshold"),
                      (lambda: L.vsp_det_decode_nms_f32(p, p, p, 0, p, p, p, 1, 96, 128, 0.5, 0.4, 4096, 8, None), "max_candidates 4096"),
                      (lambda: L.vsp_det_decode_nms_f32(p, p, p, 0, p, p, p, 1, 96, 128, 0.5, 0.4, 64, 8, None), "work of 0 bytes"),
                      (lambda: L.vsp_det_sep_f32(None, p, p, p, p, p, 1, 8, 16, 5, 5, 1, 0.1, None), "null pointer")):
        rc = call()
        assert rc == -1 and msg in _lib.last_error(), (rc, msg, _lib.last_error())
    assert L.vsp_det_sep_f32(p, p, p, p, p, p, 40, 256, 256, 4096, 4096, 1, 0.1, None) == -3 and "2 GiB" in _lib.last_error()
    it = (_lib.DetSrc * 1)()
    it[0].off, it[0].h, it[0].w, it[0].slot = 0, 65, 10, 0
    assert L.vsp_det_entry_u8(p, p, 10000, C.cast(it, C.c_void_p), p, 1, p, p, 1, 64, 64, 1, 0.1, None) == -1 and "does not fit" in _lib.last_error()
    it[0].h, it[0].off = 10, 9800
    assert L.vsp_det_entry_u8(p, p, 10000, C.cast(it, C.c_void_p), p, 1, p, p, 1, 64, 64, 1, 0.1, None) == -1 and "outside src" in _lib.last_error()
    assert L.vsp_det_work_bytes(2, 96, 128, 64) == 2 * (504 * 4 + 64 * 64 * 4) and L.vsp_det_work_bytes(1, 96, 128, 0) == 0
    assert C.sizeof(_lib.DetFace) == 64 and C.sizeof(_lib.DetSrc) == 24


def test_margins_of_the_gpu_detection_case():
    """For the seed of the GPU detection test the float32 and float64 restatements keep the same ordered set, and the smallest
    score-to-threshold and IoU-to-nms margins are at least 20 times the largest fp32-vs-float64 deviation of that quantity."""
    case = K.detection_case()
    for k, d in enumerate(case["det"]):
        r64, r32 = d["r64"], d["r32"]
        assert list(r64["order"]) == list(r32["order"]) and list(r64["keep"]) == list(r32["keep"]) and len(r64["keep"]) >= 3
        ms, mi = R.margins(d["d64"][0], d["d64"][1], K.THRESHOLD, K.NMS, r64["order"])
        ds = float(np.abs(d["d32"][0].astype(np.float64) - d["d64"][0]).max())
        di = float(np.nanmax(np.abs(R.iou_matrix(d["d32"][1][r64["order"]]).astype(np.float64) - R.iou_matrix(d["d64"][1][r64["order"]]))))
        print(f"image {k}: {r64['candidates']} candidates, {len(r64['keep'])} kept; score margin {ms:.2e} / deviation {ds:.2e}, IoU margin {mi:.2e} / deviation {di:.2e}")
        assert ms >= 20 * ds and mi >= 20 * di


def test_synthetic_heads_are_decided_alike_at_both_precisions():
    """the inputs of the GPU post-processing test: float32 and float64 restatements agree on every ordered set it compares"""
    conf, loc, lm = K.synthetic_heads()
    for caps in ((1024, 256), (64, 4)):
        for k in range(3):
            r = [R.select_nms(*R.decode(conf[k], loc[k], lm[k], K.HC, K.WC, dt), K.THRESHOLD, K.NMS, *caps) for dt in (np.float64, np.float32)]
            assert list(r[0]["keep"]) == list(r[1]["keep"]) and r[0]["status"] == r[1]["status"] and list(r[0]["order"]) == list(r[1]["order"])
            if k == 0:
                assert r[0]["candidates"] == 54 and 3 <= len(r[0]["keep"]) < 54
            if k == 1 and caps == (64, 4):
                assert r[0]["status"] == R.CAND_CAPPED | R.FACES_CAPPED and r[0]["candidates"] > 64
            if k == 2:
                assert r[0]["candidates"] == 0 and len(r[0]["keep"]) == 0
