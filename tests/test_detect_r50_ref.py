"""CPU checks of the ResNet-50 face detector: the checkpoint's key layout against the restated torch.nn tree, every rule and
refusal of the loader, the dispatch by key both ways, the BatchNorm fold against the unfused tree in float64, the weight image's index
map and round trip, the entries' refusals (no GPU needed: validation precedes every launch), the 2 GiB guard's chunking, the parsers'
help and report.json's `detect` entry, and the margins of the GPU detection case."""
import ctypes as C

import numpy as np
import pytest
import torch

import detect_cases as K0
import detect_r50_cases as K
import detect_r50_ref as R5
import detect_ref as R


def test_key_layout_and_count_are_those_of_the_restated_tree():
    from vspbfr_amd import detect_r50 as D5
    sd = K.state()
    want = D5.expected_state()
    assert list(want) == list(sd) and len(sd) == 456                      # the tree's own count, in the tree's own order
    assert all(tuple(sd[k].shape) == tuple(want[k]) for k in sd)
    assert len(D5.conv_units()) == 73 and len(D5.expected_state(with_tracked=False)) == 456 - 73
    assert want["body.layer4.0.downsample.0.weight"] == (2048, 1024, 1, 1) and want["body.layer2.0.conv2.weight"] == (128, 128, 3, 3)
    assert want["ssh3.conv7x7_3.0.weight"] == (64, 64, 3, 3) and want["LandmarkHead.2.conv1x1.weight"] == (20, 256, 1, 1)
    assert not any(k.startswith("body.fc") for k in want)
    strides = {c: s for c, _, _, s in D5.conv_units()}
    assert strides["body.layer3.0.conv2"] == 2 and strides["body.layer3.0.conv1"] == 1 and strides["body.layer3.0.downsample.0"] == 2 \
        and strides["body.layer1.0.conv2"] == 1 and strides["body.layer3.1.conv2"] == 1


def test_loader_rules_and_refusals_by_name():
    from vspbfr_amd import detect_r50 as D5
    sd = K.state()
    plain = D5.check_state_dict(sd)
    assert len(plain) == 456 - 73 and all(v.dtype == torch.float64 for v in plain.values())
    for wrapped in ({"module." + k: v for k, v in sd.items()}, {"state_dict": sd}, {k: v for k, v in sd.items() if not k.endswith("num_batches_tracked")}):
        got = D5.check_state_dict(wrapped)
        assert list(got) == list(plain) and all(torch.equal(got[k], plain[k]) for k in plain)

    def refused(edit, match):
        bad = dict(sd)
        edit(bad)
        with pytest.raises(ValueError, match=match):
            D5.check_state_dict(bad)

    refused(lambda d: d.pop("body.layer3.5.bn2.running_var"), "RetinaFace resnet50 checkpoint: missing keys body.layer3.5.bn2.running_var")
    refused(lambda d: d.pop("fpn.merge1.0.weight"), "missing keys fpn.merge1.0.weight")
    refused(lambda d: d.update({"body.fc.weight": torch.zeros(1000, 2048)}), "unexpected keys body.fc.weight")
    refused(lambda d: d.update({"body.layer1.3.conv1.weight": torch.zeros(64, 256, 1, 1)}), "unexpected keys body.layer1.3.conv1.weight")
    refused(lambda d: d.update({"ssh1.conv3X3.0.weight": torch.zeros(32, 64, 3, 3)}), r"ssh1.conv3X3.0.weight has shape \(32, 64, 3, 3\), expected \(128, 256, 3, 3\)")
    refused(lambda d: d.update({"BboxHead.1.conv1x1.bias": torch.zeros(4)}), "BboxHead.1.conv1x1.bias has shape")
    refused(lambda d: d.update({"body.layer2.0.conv2.weight": torch.zeros(128, 128, 1, 1)}), "body.layer2.0.conv2.weight has shape")


def test_dispatch_by_key_both_ways(tmp_path):
    from vspbfr_amd import detect as D, detect_r50 as D5
    r50, mob = K.state(), K0.model().state_dict()
    torch.save({"module." + k: v for k, v in r50.items()}, tmp_path / "r50.pth")
    torch.save(mob, tmp_path / "mob.pth")
    for w in (r50, {"state_dict": r50}, str(tmp_path / "r50.pth")):
        det = D.load_detector(w, "cpu")
        assert type(det) is D5.RetinaFaceR50Detector and det.backbone == "resnet50" and isinstance(det, D.RetinaFaceDetector)
    assert D5.RetinaFaceR50Detector.canvas is D.RetinaFaceDetector.canvas and D5.RetinaFaceR50Detector.detect is D.RetinaFaceDetector.detect \
        and D5.RetinaFaceR50Detector.postprocess is D.RetinaFaceDetector.postprocess
    for w in (mob, {"module." + k: v for k, v in mob.items()}, str(tmp_path / "mob.pth")):
        det = D.load_detector(w, "cpu")
        assert type(det) is D.RetinaFaceDetector and not hasattr(det, "backbone")
        ref = D.RetinaFaceDetector(mob, "cpu")
        assert list(det.p) == list(ref.p) and all(torch.equal(det.p[k], ref.p[k]) for k in ref.p)
    with pytest.raises(ValueError, match="RetinaFace mobilenet0.25 checkpoint: missing keys"):
        D.load_detector({"weight": torch.zeros(3)}, "cpu")
    broken = dict(r50)
    broken.pop("ClassHead.0.conv1x1.bias")
    with pytest.raises(ValueError, match="RetinaFace resnet50 checkpoint: missing keys ClassHead.0.conv1x1.bias"):
        D.load_detector(broken, "cpu")
    # the device tensors: f16 images for the 72 convolutions, fp32 for the stem, the heads and every bias
    p = D.load_detector(r50, "cpu").p
    assert sum(v.dtype == torch.float16 for v in p.values()) == 72 and p["body.conv1.w"].dtype == torch.float32 and tuple(p["body.conv1.w"].shape) == (147, 64)
    assert p["body.layer4.0.conv2.w"].shape == (9, 16, 32, 64, 8) and p["heads.2.w"].shape == (256, 32) and p["heads.2.w"].dtype == torch.float32
    assert all(v.dtype == torch.float32 for k, v in p.items() if k.endswith(".b"))


def test_weight_image_index_map_and_round_trip():
    from vspbfr_amd import detect_r50 as D5
    g = torch.Generator().manual_seed(1)
    for co, ci, k in ((64, 64, 1), (128, 96, 3), (48, 160, 3)):
        w = torch.randn(co, ci, k, k, generator=g, dtype=torch.float64)
        img = D5.pack_conv_weight(w)
        assert tuple(img.shape) == (k * k, ci // 32, co // 16, 64, 8)
        assert torch.equal(D5.unpack_conv_weight(img), w)
        flat = img.reshape(-1)
        for o, i, t in ((0, 0, 0), (co - 1, ci - 1, k * k - 1), (17, 41, k * k // 2), (co - 16, 8, 0), (15, 31, k * k - 1), (33, 63, 0)):
            assert float(flat[R5.pack_index(o, i, t, ci, co)]) == float(w[o, i, t // k, t % k]), (co, ci, k, o, i, t)
    for bad in ((40, 64, 1, 1), (64, 48, 1, 1), (64, 64, 3, 1)):
        with pytest.raises(ValueError, match="pack_conv_weight"):
            D5.pack_conv_weight(torch.zeros(bad))
    w = torch.randn(64, 3, 7, 7, generator=g, dtype=torch.float64)
    s = D5.pack_stem(w)
    assert tuple(s.shape) == (147, 64) and float(s[(7 * 2 + 5) * 3 + 1, 9]) == float(w[9, 1, 2, 5])


def test_fold_against_the_unfused_tree_in_float64():
    """fold_state's tensors, unpacked and run without any rounding, give the unfused tree's outputs to 1e-12 relative"""
    from vspbfr_amd import detect as D, detect_r50 as D5
    folded = D5.fold_state(D5.check_state_dict(K.state()))
    assert all(v.dtype == torch.float64 for v in folded.values())
    fw = {}
    for conv, _, shape, _ in D5.conv_units():
        w = folded[conv + ".w"]
        fw[conv] = (w.reshape(7, 7, 3, 64).permute(3, 2, 0, 1) if shape[1] == 3 else D5.unpack_conv_weight(w), folded[conv + ".b"])
        assert tuple(fw[conv][0].shape) == tuple(shape)
    for k in range(3):
        fw[f"heads.{k}"] = (folded[f"heads.{k}.w"].t().reshape(32, 256, 1, 1), folded[f"heads.{k}.b"])
    photos = K.detection_case()["canvas_photos"]
    with torch.no_grad():
        want = K.model()(R.canvas(photos, K.HC, K.WC))
        got = R5.forward(fw, photos, K.HC, K.WC, torch.float64, rounded=False)
        own = R5.forward(K.folded(), photos, K.HC, K.WC, torch.float64, rounded=False)
    for a, b, c, name in zip(got, want, own, ("conf", "loc", "lm")):
        rel = float((a - b).abs().max() / b.abs().max())
        print(f"fold {name}: max|d| / max|ref| = {rel:.2e}, the restatement's own fold {float((c - b).abs().max() / b.abs().max()):.2e}")
        assert rel <= 1e-12 and float((c - b).abs().max() / b.abs().max()) <= 1e-12
    # the heads lie side by side as detect.fold_state lays them
    assert torch.equal(folded["heads.1.w"][:, 4:12], D.pack_pointwise(K.state()["BboxHead.1.conv1x1.weight"].double()))


def test_entries_refuse_what_they_do_not_serve():
    """validation precedes every launch: no GPU needed"""
    from vspbfr_amd import _lib
    L, p, q, o = _lib.lib, C.c_void_p(1 << 20), C.c_void_p(1 << 24), C.c_void_p(1 << 28)
    tab = (_lib.DetSrc * 2)()

    def items(h=5, w=7, off=0, slot=0):
        tab[0].off, tab[0].h, tab[0].w, tab[0].slot = off, h, w, slot
        return tab

    def stem(y=p, src=q, src_bytes=3 * 35, it=None, dev=o, n=1, w=q, b=q, B=2, Hc=32, Wc=32):
        return L.vsp_det50_stem_u8(y, src, src_bytes, C.cast(it if it is not None else items(), C.c_void_p), dev, n, w, b, B, Hc, Wc, None)

    def pool(y=p, x=q, B=2, H=5, W=7, ch=64):
        return L.vsp_det50_pool_f16(y, x, B, H, W, ch, None)

    def conv(y=p, yp=256, yo=0, x=q, xp=64, xo=0, B=2, H=5, W=7, cin=64, cout=256, k=1, s=1, flags=1, w=o, b=o, r=None, rp=0, ro=0, u=None, up=0, uo=0):
        return L.vsp_det50_conv_f16(y, yp, yo, x, xp, xo, B, H, W, cin, cout, k, s, flags, w, b, r, rp, ro, u, up, uo, None)

    def heads(conf=p, loc=p, lm=p, x=q, xp=256, w=o, b=o, B=2, H=2, W=3, P=12, p0=0):
        return L.vsp_det50_heads_f32(conf, loc, lm, x, xp, w, b, B, H, W, P, p0, None)

    far = C.c_void_p(1 << 30)
    for call, msg in ((lambda: stem(y=None), "null pointer"), (lambda: stem(dev=None), "null pointer"), (lambda: stem(b=None), "null pointer"),
                      (lambda: stem(Hc=0), "canvas 0 x 32"), (lambda: stem(n=3), "3 items for a batch of 2"), (lambda: stem(n=-1), "-1 items"),
                      (lambda: stem(it=items(h=33)), "photo 33 x 7 does not fit"), (lambda: stem(it=items(w=0)), "photo 5 x 0"),
                      (lambda: stem(src_bytes=3 * 35 - 1), "bytes outside src"), (lambda: stem(it=items(off=1)), "bytes outside src"),
                      (lambda: stem(it=items(off=-1)), "bytes outside src"), (lambda: stem(it=items(slot=2)), "slot 2 outside 0..1"),
                      (lambda: stem(it=items(slot=-1)), "slot -1"), (lambda: stem(y=C.c_void_p((1 << 20) + 4)), "aligned"),
                      (lambda: stem(w=C.c_void_p((1 << 24) + 8)), "aligned"),
                      (lambda: pool(y=None), "null pointer"), (lambda: pool(ch=60), "60 channels"), (lambda: pool(ch=4096), "4096 channels"),
                      (lambda: pool(H=0), "map 0 x 7"), (lambda: pool(x=C.c_void_p((1 << 24) + 8)), "aligned"),
                      (lambda: pool(y=C.c_void_p((1 << 24) + 64)), "overlaps the input"),
                      (lambda: conv(y=None), "null pointer"), (lambda: conv(w=None), "null pointer"), (lambda: conv(b=None), "null pointer"),
                      (lambda: conv(cin=32), "32 -> 256 channels"), (lambda: conv(cin=96, xp=96), "96 -> 256"), (lambda: conv(cin=4096, xp=4096), "4096 -> 256"),
                      (lambda: conv(cout=32), "64 -> 32"), (lambda: conv(cout=192 + 32), "64 -> 224"), (lambda: conv(cout=4096, yp=4096), "64 -> 4096"),
                      (lambda: conv(k=5), "filter 5 x 5"), (lambda: conv(k=2), "filter 2 x 2"), (lambda: conv(s=3), "stride 3"), (lambda: conv(s=0), "stride 0"),
                      (lambda: conv(flags=2), "unknown flags"), (lambda: conv(H=0), "map 0 x 7"), (lambda: conv(B=-1), "batch -1"),
                      (lambda: conv(xp=56), "input channels 0..63 of a pitch of 56"), (lambda: conv(xo=8), "input channels 8..71 of a pitch of 64"),
                      (lambda: conv(xp=132, xo=4), "input channels"), (lambda: conv(xp=68), "input channels"), (lambda: conv(xo=-8, xp=128), "input channels"),
                      (lambda: conv(yp=192), "output channels 0..255 of a pitch of 192"), (lambda: conv(yp=320, yo=128), "output channels 128..383"),
                      (lambda: conv(yp=258), "output channels"), (lambda: conv(yp=320, yo=2), "output channels"), (lambda: conv(yo=-4, yp=512), "output channels"),
                      (lambda: conv(r=far, rp=128), "residual channels 0..255 of a pitch of 128"), (lambda: conv(r=far, rp=512, ro=258), "residual channels"),
                      (lambda: conv(H=4, W=6, u=far, up=64), "coarser-level channels 0..255 of a pitch of 64"),
                      (lambda: conv(u=far, up=256), "needs an even output map, not 5 x 7"), (lambda: conv(H=6, W=7, u=far, up=256), "even output map"),
                      (lambda: conv(H=9, W=12, s=2, u=far, up=256), "not 5 x 6"),
                      (lambda: conv(x=C.c_void_p((1 << 24) + 8)), "aligned"), (lambda: conv(y=C.c_void_p((1 << 20) + 4)), "aligned"),
                      (lambda: conv(r=C.c_void_p((1 << 30) + 4), rp=256), "aligned"), (lambda: conv(H=4, W=6, u=C.c_void_p((1 << 30) + 2), up=256), "aligned"),
                      (lambda: conv(b=C.c_void_p((1 << 28) + 4)), "aligned"),
                      (lambda: conv(y=q), "output overlaps the input"), (lambda: conv(y=C.c_void_p((1 << 24) + 2 * 70 * 64 - 8)), "output overlaps the input"),
                      (lambda: conv(r=p, rp=512), "residual overlaps the output"), (lambda: conv(yp=512, r=p, rp=512, ro=256), "residual overlaps the output"),
                      (lambda: conv(r=C.c_void_p((1 << 20) + 512), rp=256), "residual overlaps the output"),
                      (lambda: conv(H=4, W=6, u=p, up=256), "coarser level overlaps the output"),
                      (lambda: heads(conf=None), "null pointer"), (lambda: heads(x=None), "null pointer"), (lambda: heads(P=11), "priors 0..11 of 11"),
                      (lambda: heads(p0=1), "priors 1..12 of 12"), (lambda: heads(p0=-2), "priors"), (lambda: heads(xp=128), "input pitch 128"),
                      (lambda: heads(xp=260), "input pitch 260"), (lambda: heads(x=C.c_void_p((1 << 24) + 8)), "aligned"), (lambda: heads(H=0), "map 0 x 3")):
        rc = call()
        assert rc == -1 and msg in _lib.last_error(), (rc, msg, _lib.last_error())
    # what is served passes validation up to the launch itself (B = 0 / n = 0 return before any pointer is looked at)
    assert conv(B=0, y=None) == 0 and pool(B=0, y=None) == 0 and heads(B=0, x=None) == 0 and stem(n=0, y=None) == 0
    two = 1 << 31
    assert stem(src_bytes=two) == -3 and "2 GiB" in _lib.last_error()
    assert stem(B=64, Hc=1024, Wc=1024, it=items(), src_bytes=3 * 35) == -3 and stem(B=63, Hc=1024, Wc=1024, y=None) == -1
    assert pool(B=64, H=512, W=512, ch=64) == -3 and "2 GiB" in _lib.last_error()
    assert conv(B=64, H=256, W=256, cin=256, xp=256, cout=64, yp=64) == -3 and "2 GiB" in _lib.last_error()
    assert conv(B=64, H=256, W=256, cin=64, xp=64, cout=256, yp=256) == -3 and conv(B=16, H=256, W=256, r=far, rp=1024) == -3
    assert conv(B=16, H=256, W=256, cin=64, cout=64, yp=64, u=far, up=4096) == -3
    assert heads(B=2048, H=64, W=64, P=2 * 64 * 64) == -3 and "2 GiB" in _lib.last_error()


def test_a_batch_past_the_guard_runs_in_chunks_and_one_image_past_it_is_refused():
    from vspbfr_amd import detect_r50 as D5
    assert D5.image_bytes(64, 96) == 32 * 48 * 64 * 2 and D5.image_bytes(1024, 1024) == 1 << 25
    det = D5.RetinaFaceR50Detector(K.state(), "cpu")
    calls = []
    det._network = lambda sources, B, Hc, Wc: (calls.append((B, [items for _, items in sources])),
                                               tuple(torch.full((B, 4, n), float(len(calls))) for n in (2, 4, 10)))[1]
    src = [("buf0", [(0, 5, 7, 2), (105, 5, 7, 0)]), ("buf1", [(0, 9, 9, 1), (9, 9, 9, 4), (18, 9, 9, 3)])]
    det.GUARD_BYTES = 2 * D5.image_bytes(64, 96) + 1
    out = det.network(src, 5, 64, 96)
    assert [c[0] for c in calls] == [2, 2, 1]
    assert calls[0][1] == [[(105, 5, 7, 0)], [(0, 9, 9, 1)]] and calls[1][1] == [[(0, 5, 7, 0)], [(18, 9, 9, 1)]] and calls[2][1] == [[], [(9, 9, 9, 0)]]
    assert [tuple(t.shape) for t in out] == [(5, 4, 2), (5, 4, 4), (5, 4, 10)] and out[0][:, 0, 0].tolist() == [1.0, 1.0, 2.0, 2.0, 3.0]
    det.GUARD_BYTES = D5.image_bytes(64, 96)
    with pytest.raises(ValueError, match="one image of a 64 x 96 canvas"):
        det.network(src, 5, 64, 96)
    del det.GUARD_BYTES
    assert det.GUARD_BYTES == 1 << 31
    with pytest.raises(ValueError, match="multiples of 32"):
        det.network(src, 5, 64, 100)
    with pytest.raises(ValueError, match="fill slots"):
        det.network(src[:1], 5, 64, 96)


def test_parsers_and_the_report_entry(tmp_path, capsys):
    import argparse
    from vspbfr_amd import detect as D, restore_photos
    params = D.check_detect_arguments(0.5, 0.4, 1024, 2, 0.0)
    r50, mob = D.load_detector(K.state(), "cpu"), D.load_detector(K0.model().state_dict(), "cpu")
    assert restore_photos.detect_report(mob, params) is params                       # the MobileNet route's entry is the one it was
    assert restore_photos.detect_report(r50, params) == dict(params, backbone="resnet50") and "backbone" not in params
    ap = argparse.ArgumentParser()
    ap.add_argument("--weights", help="x")
    for main, flag in ((D.main, "--weights"), (restore_photos.main, "--detect_weights")):
        with pytest.raises(SystemExit):
            main(["--help"])
        text = " ".join(capsys.readouterr().out.split())
        assert flag in text and "mobilenet0.25 or resnet50" in text
    (tmp_path / "photos").mkdir()
    with pytest.raises(SystemExit) as e:
        D.main(["--photos", str(tmp_path / "photos"), "--weights", str(tmp_path / "none.pth"), "--out", str(tmp_path / "o.json")])
    assert e.value.code == 2 and "no such file" in capsys.readouterr().err
    assert "detect_r50" in D.__doc__ and "DESIGN 27" in restore_photos.__doc__


def test_margins_of_the_gpu_detection_case():
    """For the seed of the GPU detection test, in float64: every candidate's score is further from the threshold, every compared pair's
    IoU further from the NMS threshold, and every two candidates' scores further from each other, than twice the largest deviation of
    the float32 restatement with the kernels' rounding points from float64 in that quantity; both keep the same ordered set; NMS
    suppresses in both images; no face is left out of the comparison."""
    case = K.detection_case()
    for k, d in enumerate(case["det"]):
        r64, r32 = d["r64"], d["r32"]
        o = r64["order"]
        assert list(o) == list(r32["order"]) and list(r64["keep"]) == list(r32["keep"]) and r64["status"] == r32["status"] == 0
        assert 3 <= len(r64["keep"]) < r64["candidates"] <= 1024
        ms, mi = R.margins(d["d64"][0], d["d64"][1], K.THRESHOLD, K.NMS, o)
        gap = float(np.diff(np.sort(d["d64"][0][o])).min())
        ds = float(np.abs(d["d32"][0].astype(np.float64) - d["d64"][0]).max())
        di = float(np.nanmax(np.abs(R.iou_matrix(d["d32"][1][o]).astype(np.float64) - R.iou_matrix(d["d64"][1][o]))))
        print(f"image {k}: {r64['candidates']} candidates, {len(r64['keep'])} kept; score margin {ms:.2e} and gap {gap:.2e} / deviation {ds:.2e}, "
              f"IoU margin {mi:.2e} / deviation {di:.2e}")
        assert ms > 2 * ds and mi > 2 * di and gap > 2 * ds
    # image 0 of the batch is the image alone, in the restatement too
    for a, b in zip(case["alone64"], case["o64"]):
        assert np.array_equal(a[0], b[0])
