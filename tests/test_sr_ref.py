"""CPU checks of the background upscaler: the checkpoint's key layout and every refusal of the loader, the weight image round
trip, the band planner, the restatement's shuffle and skip against torch's own, the restatement in bands against itself, the entries'
refusals (no GPU needed: validation precedes every launch) and the errors of both parsers."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import sr_ref as R


def test_key_layout_and_inference_of_num_conv_and_scale():
    from vspbfr_amd import upscale as U
    want = U.expected_state(32, 4)
    assert len(want) == 101 and want["body.66.weight"] == (48, 64, 3, 3) and want["body.65.weight"] == (64,)
    assert want["body.0.weight"] == (64, 3, 3, 3) and "body.67.weight" not in want
    for nc, s in ((32, 4), (16, 2), (1, 2)):
        sd = R.make_state(nc, s, seed=3)
        assert {k: tuple(v.shape) for k, v in sd.items()} == U.expected_state(nc, s)
        for wrapped in (sd, {"params_ema": sd}, {"params": {"module." + k: v for k, v in sd.items()}}):
            st = U.check_state_dict(wrapped)
            assert (st.num_conv, st.scale) == (nc, s) and len(st.tensors) == 3 * nc + 5
            assert all(t.dtype == torch.float32 for t in st.tensors.values())
    assert U.check_state_dict(st) is st


def test_loader_refusals_name_the_key():
    from vspbfr_amd import upscale as U
    sd = R.make_state(2, 2, seed=4)

    def refused(edit, match):
        bad = dict(sd)
        edit(bad)
        with pytest.raises(ValueError, match=match):
            U.check_state_dict(bad)

    refused(lambda d: d.pop("body.3.weight"), r"missing keys body\.3\.weight")
    refused(lambda d: d.pop("body.2.bias"), r"missing keys body\.2\.bias")
    refused(lambda d: d.update({"body.9.scale": torch.zeros(1)}), r"unexpected keys body\.9\.scale")
    refused(lambda d: d.update({"body.3.weight": torch.zeros(1)}), r"body\.3\.weight has shape \(1,\)")
    refused(lambda d: d.update({"body.2.weight": torch.zeros(64, 64, 1, 1)}), r"body\.2\.weight has shape")
    refused(lambda d: d.update({"body.0.weight": torch.zeros(48, 3, 3, 3)}), r"body\.0\.weight has 48 features")
    refused(lambda d: d.update({"body.6.weight": torch.zeros(27, 64, 3, 3)}), r"body\.6\.weight has shape \(27, 64, 3, 3\); Cout must be 12")
    refused(lambda d: d.update({"body.7.weight": torch.zeros(64)}), r"body\.7\.weight gives num_conv")
    with pytest.raises(ValueError, match="num_conv 0"):       # head and tail alone
        U.check_state_dict({"body.0.weight": sd["body.0.weight"], "body.0.bias": sd["body.0.bias"], "body.1.weight": sd["body.1.weight"],
                            "body.2.weight": sd["body.6.weight"], "body.2.bias": sd["body.6.bias"]})
    with pytest.raises(ValueError, match="no body.N.weight"):
        U.check_state_dict({"conv_first.weight": torch.zeros(1)})
    with pytest.raises(ValueError, match="expected a state dict"):
        U.check_state_dict([1, 2])


def test_weight_image_layout_and_round_trip():
    """the documented element map, entry by entry, and unpack(pack(w)) = f16(w) for the body (NB = 4) and both tails (NB = 1 and 3)"""
    from vspbfr_amd import upscale as U
    g = torch.Generator().manual_seed(5)
    for cout, nb in ((64, 4), (12, 1), (48, 3)):
        w = torch.randn(cout, 64, 3, 3, generator=g)
        img = U.pack_body_weight(w)
        assert img.dtype == torch.float16 and tuple(img.shape) == (18, nb, 64, 8) and img.is_contiguous()
        ref = torch.zeros(18, nb, 64, 8, dtype=torch.float16)
        wh = w.to(torch.float16)
        for s in range(18):
            for b in range(nb):
                for lane in range(64):
                    co = 16 * b + (lane & 15)
                    if co < cout:
                        c0 = 32 * (s & 1) + 8 * (lane >> 4)
                        ref[s, b, lane] = wh[co, c0:c0 + 8, (s >> 1) // 3, (s >> 1) % 3]
        assert torch.equal(img, ref)
        assert torch.equal(U.unpack_body_weight(img, cout), wh)
    hw = torch.randn(64, 3, 3, 3, generator=g)
    ph = U.pack_head_weight(hw)
    assert tuple(ph.shape) == (27, 64) and ph[(3 * 1 + 2) * 3 + 1, 17] == hw[17, 1, 1, 2]
    with pytest.raises(ValueError, match="pack_body_weight"):
        U.pack_body_weight(torch.zeros(64, 32, 3, 3))


@pytest.mark.parametrize("h,rows,halo", [(64, 8, 34), (64, 40, 34), (1, 5, 3), (17, 1, 2), (33, 33, 4), (33, 32, 0), (100, 7, 3)])
def test_plan_bands_covers_every_row_once(h, rows, halo):
    from vspbfr_amd.upscale import plan_bands
    bands = plan_bands(h, rows, halo)
    written = np.zeros(h, dtype=int)
    for r0, r1, a0, a1 in bands:
        written[r0:r1] += 1
        assert 0 < r1 - r0 <= rows and a0 == max(0, r0 - halo) and a1 == min(h, r1 + halo) and 0 <= a0 <= r0 < r1 <= a1 <= h
    assert (written == 1).all() and len(bands) == -(-h // rows)
    for bad in ((0, 1, 1), (4, 0, 1), (4, 1, -1)):
        with pytest.raises(ValueError):
            plan_bands(*bad)


def test_shuffle_and_skip_are_torchs():
    g = torch.Generator().manual_seed(6)
    for s in (2, 4):
        t = torch.randn(1, 3 * s * s, 5, 7, generator=g, dtype=torch.float64)
        assert torch.equal(R.shuffle(t, s), F.pixel_shuffle(t, s))
        x = torch.randn(1, 3, 5, 7, generator=g, dtype=torch.float64)
        assert torch.equal(R.nearest(x, s), F.interpolate(x, scale_factor=s, mode="nearest"))


@pytest.mark.parametrize("rows", [3, 8, 40])
def test_restatement_in_bands_equals_itself(rows):
    """a halo of num_conv + 2 rows is the receptive radius: exact equality, float64 and float32"""
    from vspbfr_amd.upscale import plan_bands
    sd = R.make_state(4, 2, seed=7)
    x = R.test_photo(29, 11, seed=8)
    for dtype in (torch.float64, torch.float32):
        whole = R.net(sd, x, dtype)
        assert torch.equal(R.net_banded(sd, x, dtype, rows, plan_bands(29, rows, 6)), whole)
    short = R.net_banded(sd, x, torch.float64, rows, plan_bands(29, rows, 2))
    assert rows >= 29 or not torch.equal(short, R.net(sd, x, torch.float64))      # a halo below the radius is visible


def test_conditioning_of_the_test_weights():
    """the residual is alive behind 16 layers, some outputs clamp, and float32 differs from float64 by at most one byte"""
    sd = R.make_state(16, 2, seed=1)
    x = R.test_photo(37, 53, seed=2)
    v64, v32 = R.net(sd, x, torch.float64), R.net(sd, x, torch.float32)
    skip = torch.from_numpy(np.repeat(np.repeat(x, 2, 0), 2, 1)).double() / 255
    assert (v64 - skip).abs().mean() > 0.02 and 0 < ((v64 < 0) | (v64 > 1)).double().mean() < 0.25
    q64, q32 = R.quantise(v64), R.quantise(v32)
    assert np.abs(q64.astype(int) - q32).max() <= 1 and (q64 != q32).mean() < 0.05
    assert any((sd[f"body.{2 * k + 1}.weight"] < 0).any() for k in range(17))


def _table(shapes, scale=2):
    from vspbfr_amd import upscale as U
    src = np.concatenate([[0], np.cumsum([3 * h * w for h, w in shapes])]).tolist()
    out = np.concatenate([[0], np.cumsum([3 * h * w * scale * scale for h, w in shapes])]).tolist()
    tab, px = U.item_table([(k, 0, h, 0, h) for k, (h, w) in enumerate(shapes)], shapes, src, out, scale)
    return tab, px, src[-1], out[-1]


def test_item_table():
    from vspbfr_amd import _lib
    tab, px, sb, ob = _table([(9, 33), (1, 1), (8, 32)], 4)
    assert C.sizeof(_lib.SrItem) == 48 and px == 9 * 33 + 1 + 256 and (sb, ob) == (3 * px, 48 * px)
    assert [(t.tile0, t.act_off, t.src_off, t.out_off, t.keep0, t.keepn, t.slot) for t in tab] == [
        (0, 0, 0, 0, 0, 9, 0), (4, 297, 891, 48 * 297, 0, 1, 1), (5, 298, 894, 48 * 298, 0, 8, 2)]


def test_entries_refuse_what_they_do_not_serve():
    """validation precedes every launch: no GPU needed"""
    from vspbfr_amd import _lib
    L, p = _lib.lib, C.c_void_p(4096)
    tab, px, sb, ob = _table([(5, 7), (3, 4)])
    it = C.cast(tab, C.c_void_p)
    act = px * 128

    def head(y=p, act_bytes=act, src=p, src_bytes=sb, items=it, dev=p, n=2, w=p, b=p, a=p):
        return L.vsp_sr_head_u8(y, act_bytes, src, src_bytes, items, dev, n, w, b, a, None)

    def body(y=p, x=C.c_void_p(8192), act_bytes=act, items=it, dev=p, n=2, w=p, b=p, a=p):
        return L.vsp_sr_body_f16(y, x, act_bytes, items, dev, n, w, b, a, None)

    def tail(out=p, out_bytes=ob, f32=None, info=p, n_info=2, x=p, act_bytes=act, src=p, src_bytes=sb, items=it, dev=p, n=2, w=p, b=p, scale=2):
        return L.vsp_sr_tail_u8(out, out_bytes, f32, info, n_info, x, act_bytes, src, src_bytes, items, dev, n, w, b, scale, None)

    for call, msg in ((lambda: head(y=None), "null pointer"), (lambda: head(a=None), "null pointer"), (lambda: head(items=None), "null pointer"),
                      (lambda: body(x=None), "null pointer"), (lambda: body(w=None), "null pointer"), (lambda: body(x=p), "in place"),
                      (lambda: tail(out=None), "null pointer"), (lambda: tail(info=None), "null pointer"), (lambda: tail(src=None), "null pointer"),
                      (lambda: tail(scale=3), "scale 3"), (lambda: tail(scale=1), "scale 1"), (lambda: tail(scale=8), "scale 8"),
                      (lambda: head(act_bytes=act - 128), "activation outside"), (lambda: body(act_bytes=act - 2), "activation outside"),
                      (lambda: head(src_bytes=sb - 1), "outside src"), (lambda: tail(src_bytes=sb - 1), "outside src"),
                      (lambda: tail(out_bytes=ob - 1), "outside out"), (lambda: tail(n_info=1), "slot 1"),
                      (lambda: tail(scale=4), "outside out"), (lambda: head(n=-1), "items"), (lambda: head(y=C.c_void_p(4100)), "aligned")):
        rc = call()
        assert rc == -1 and msg in _lib.last_error(), (rc, msg, _lib.last_error())
    for field, value, msg in (("h", 0, "photo 0 x 7"), ("w", -1, "photo 5 x -1"), ("tile0", 1, "tile0"), ("keepn", 0, "rows"), ("keep0", 5, "rows"),
                              ("src_off", -1, "outside src"), ("act_off", -1, "activation outside"), ("out_off", -4, "outside out")):
        tab2, *_ = _table([(5, 7), (3, 4)])
        setattr(tab2[0], field, value)
        rc = tail(items=C.cast(tab2, C.c_void_p))
        assert rc == -1 and msg in _lib.last_error(), (field, rc, _lib.last_error())
    two = 1 << 31
    assert head(act_bytes=two) == -3 and "2 GiB" in _lib.last_error()
    assert head(src_bytes=two) == -3 and body(act_bytes=two) == -3 and tail(out_bytes=two) == -3 and tail(act_bytes=two) == -3
    assert tail(out_bytes=two // 4, f32=p) == -3 and "2 GiB" in _lib.last_error()
    assert head(n=0) == 0 and body(n=0) == 0 and tail(n=0) == 0


def test_upscaler_argument_checks_need_no_kernel():
    """what upscale() refuses before it launches (the constructor only moves tensors: the CPU stands in for the device)"""
    from vspbfr_amd import upscale as U
    net = U.SrUpscaler(R.make_state(1, 2, seed=9), "cpu")
    assert (net.num_conv, net.scale, net.halo) == (1, 2, 3) and tuple(net.tail[0].shape) == (18, 1, 64, 8) and net.tail[1].numel() == 16
    x = R.test_photo(4, 4)
    for kw, msg in ((dict(), "photos or device_photos"), (dict(photos=[x], device_photos=(None, [], [])), "photos or device_photos"),
                    (dict(photos=[x.astype(np.float32)]), "must be uint8"), (dict(photos=[]), "at least one photo"),
                    (dict(photos=[x], out_offsets=[0, 1]), "one output offset"), (dict(photos=[x], out=torch.zeros(3, dtype=torch.uint8)), "out must be"),
                    (dict(photos=[x], band_rows=0), "band_rows 0"),
                    (dict(device_photos=(torch.zeros(10, dtype=torch.uint8), [0], [(2, 2)])), "outside the buffer")):
        with pytest.raises(ValueError, match=msg):
            net.upscale(**kw)
    for scale in (1, 4, 3):
        with pytest.raises(ValueError, match="cannot fill an upscale"):
            net.upscale_to(scale, photos=[x])
    units, banded = net._units([(64, 96), (5, 7)], 40)
    assert banded == [True, True] and [u[:3] for u in units] == [(0, 0, 40), (0, 40, 64), (1, 0, 5)]
    net.act_limit = 20 * 96 * 128                             # the 2 GiB guard, scaled down: the first photo no longer fits in one piece
    units, banded = net._units([(64, 96), (5, 7)], None)
    assert banded == [True, False] and all((a1 - a0) * 96 * 128 <= net.act_limit for k, _, _, a0, a1 in units if k == 0)
    assert sorted(r for k, r0, r1, _, _ in units if k == 0 for r in range(r0, r1)) == list(range(64))
    assert [len(g) for g in net._groups(units, [(64, 96), (5, 7)])] == [1] * (len(units) - 2) + [2]
    with pytest.raises(ValueError, match="does not fit"):
        net._units([(64, 96 * 8)], None)


def test_face_plan_and_restorer_refuse_scales_the_network_cannot_fill():
    from vspbfr_amd import upscale as U
    from vspbfr_amd.photo import PhotoRestorer
    net2 = U.SrUpscaler(R.make_state(1, 2, seed=9), "cpu")
    with pytest.raises(ValueError, match="cannot fill an upscale of 4"):
        PhotoRestorer(None, 1, upscale=4, background=net2)
    with pytest.raises(ValueError, match="cannot fill an upscale of 1"):
        PhotoRestorer(None, 1, upscale=1, background=net2)
    assert PhotoRestorer(None, 1, upscale=2, background=net2).background is net2 and PhotoRestorer(None, 1, upscale=2).background is None


def test_parser_errors(tmp_path, capsys):
    """--bg_weights with --upscale 1, a x2 network at upscale 4, a refused checkpoint, a missing file: parser errors of both CLIs, raised
    before any model is built"""
    from vspbfr_amd import restore_photos, upscale
    x2, bad = tmp_path / "x2.pth", tmp_path / "bad.pth"
    torch.save({"params_ema": R.make_state(1, 2, seed=9)}, x2)
    sd = R.make_state(1, 2, seed=9)
    sd.pop("body.3.weight")
    torch.save({"params": sd}, bad)
    (tmp_path / "photos").mkdir()
    base = ["--photos", str(tmp_path / "photos"), "--out", str(tmp_path / "out"), "--landmarks", str(tmp_path / "none.json")]

    def refused(main, argv, msg):
        with pytest.raises(SystemExit) as e:
            main(argv)
        err = capsys.readouterr().err
        assert e.value.code == 2 and msg in err, err

    refused(restore_photos.main, base + ["--bg_weights", str(x2)], "needs an upscale of 2 or 4, not 1")
    refused(restore_photos.main, base + ["--bg_weights", str(x2), "--upscale", "4"], "x2 network: it cannot fill an upscale of 4")
    refused(restore_photos.main, base + ["--bg_weights", str(bad), "--upscale", "2"], "missing keys body.3.weight")
    refused(restore_photos.main, base + ["--bg_weights", str(tmp_path / "nope.pth"), "--upscale", "2"], "no such file")
    refused(restore_photos.main, base + ["--bg_band_rows", "8", "--upscale", "2"], "--bg_band_rows belongs to --bg_weights")
    refused(restore_photos.main, base + ["--bg_weights", str(x2), "--upscale", "2", "--bg_band_rows", "0"], "at least 1")
    own = ["--photos", str(tmp_path / "photos"), "--out", str(tmp_path / "out")]
    refused(upscale.main, own + ["--weights", str(x2), "--scale", "4"], "x2 network: it cannot fill an upscale of 4")
    refused(upscale.main, own + ["--weights", str(bad)], "missing keys body.3.weight")
    refused(upscale.main, own + ["--weights", str(x2), "--scale", "1"], "invalid choice")
