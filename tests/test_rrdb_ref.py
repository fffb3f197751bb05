"""CPU checks of the RRDBNet background upscaler: the checkpoint's key layout and every refusal of the loader, the weight image
maps, the restatement's unshuffle and reflection against torch's own, the restatement against an independent torch.nn tree under the
public key names, the trunk's band halo and the 4x maps' band halo on both sides (derived: exact; one row less: visible), the share of
unclamped outputs of every GPU case, the entries' refusals (no GPU needed: validation precedes every launch), the CLI dispatch by key and
describe()."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn as nn
import torch.nn.functional as F

import rrdb_ref as R
import sr_ref

# the whole-net cases of tests/test_rrdb_gpu.py: (num_block, scale, h, w)
GPU_CASES = [(1, 4, 5, 7), (2, 4, 9, 33), (2, 2, 11, 13), (3, 4, 17, 20), (23, 4, 9, 11)]


def test_key_layout_and_inference_of_num_block_and_scale():
    from vspbfr_amd import rrdb
    for nb in (1, 6, 23):
        for s in (4, 2):
            want = rrdb.expected_state(nb, s)
            assert len(want) == 30 * nb + 12 and len(rrdb.conv_names(nb)) == 15 * nb + 6
            assert want["conv_first.weight"] == (64, 3 if s == 4 else 12, 3, 3) and want["conv_last.weight"] == (3, 64, 3, 3)
            assert want[f"body.{nb - 1}.rdb3.conv5.weight"] == (64, 192, 3, 3) and want["body.0.rdb1.conv1.weight"] == (32, 64, 3, 3)
            assert want["body.0.rdb2.conv4.weight"] == (32, 160, 3, 3) and want["body.0.rdb2.conv4.bias"] == (32,)
            assert f"body.{nb}.rdb1.conv1.weight" not in want
            assert set(k.split(".")[0] for k in want) == {"conv_first", "body", "conv_body", "conv_up1", "conv_up2", "conv_hr", "conv_last"}
    assert len(rrdb.expected_state(23, 4)) == 702
    sd = R.make_state(2, 2, seed=3)
    for wrapped in (sd, {"params_ema": sd}, {"params": sd}, {"params": {"module." + k: v for k, v in sd.items()}}):
        st = rrdb.check_state_dict(wrapped)
        assert (st.num_block, st.scale) == (2, 2) and len(st.tensors) == 72 and all(t.dtype == torch.float32 for t in st.tensors.values())
    assert rrdb.check_state_dict(st) is st
    assert rrdb.check_state_dict(R.make_state(1, 4)).scale == 4


def test_loader_refusals_name_the_key():
    from vspbfr_amd import rrdb
    sd = R.make_state(2, 4, seed=4)

    def refused(edit, match):
        bad = dict(sd)
        edit(bad)
        with pytest.raises(ValueError, match=match):
            rrdb.check_state_dict(bad)

    refused(lambda d: d.pop("body.1.rdb2.conv3.bias"), "missing keys body.1.rdb2.conv3.bias")
    refused(lambda d: d.pop("conv_hr.weight"), "missing keys conv_hr.weight")
    refused(lambda d: d.update({"conv_extra.weight": torch.zeros(1)}), "unexpected keys conv_extra.weight")
    refused(lambda d: d.update({"body.0.rdb4.conv1.weight": torch.zeros(1)}), "unexpected keys body.0.rdb4.conv1.weight")
    refused(lambda d: d.update({"body.0.rdb1.conv2.weight": torch.zeros(32, 64, 3, 3)}), "body.0.rdb1.conv2.weight has shape")
    refused(lambda d: d.update({"conv_last.bias": torch.zeros(4)}), "conv_last.bias has shape")
    refused(lambda d: d.update({"conv_first.weight": torch.zeros(32, 3, 3, 3)}), "conv_first.weight has 32 features")
    refused(lambda d: d.update({"conv_first.weight": torch.zeros(64, 4, 3, 3)}), "Cin must be 3")
    refused(lambda d: d.update({"body.0.rdb1.conv1.weight": torch.zeros(16, 64, 3, 3)}), "growth of 16")
    refused(lambda d: d.pop("conv_first.weight"), "no conv_first.weight key")
    refused(lambda d: [d.pop(k) for k in list(d) if k.startswith("body.")], "num_block >= 1")
    refused(lambda d: [d.pop(k) for k in list(d) if k.startswith("body.0.")], "missing keys body.0.rdb1.conv1.bias")
    with pytest.raises(ValueError, match="expected a state dict"):
        rrdb.check_state_dict([1, 2])
    assert rrdb.check_state_dict(R.make_state(1, 2)).tensors["conv_first.weight"].shape[1] == 12


def test_weight_images_entry_by_entry_and_round_trip():
    from vspbfr_amd import rrdb
    g = torch.Generator().manual_seed(5)
    for cout, cin in ((32, 64), (32, 96), (32, 160), (64, 192), (64, 64), (3, 64)):
        w = torch.randn(cout, cin, 3, 3, generator=g)
        img = rrdb.pack_conv_weight(w)
        nb = -(-cout // 16)
        assert img.shape == (cin // 32, 9, nb, 64, 8) and img.dtype == torch.float16
        w16 = w.to(torch.float16)
        for kc, t, b, l, j in ((0, 0, 0, 0, 0), (cin // 32 - 1, 8, nb - 1, 63, 7), (1, 5, 0, 37, 3), (0, 7, nb - 1, 18, 6), (1, 2, 0, 2, 1)):
            co, ci = 16 * b + (l & 15), 32 * kc + 8 * (l >> 4) + j
            want = w16[co, ci, t // 3, t % 3] if co < cout else 0
            assert img[kc, t, b, l, j] == want, (cout, cin, kc, t, b, l, j)
        flat = torch.zeros(nb * 16, cin, 3, 3, dtype=torch.float16)
        flat[:cout] = w16
        idx = torch.arange(img.numel())
        j, l, b, t, kc = idx % 8, idx // 8 % 64, idx // 512 % nb, idx // (512 * nb) % 9, idx // (512 * nb * 9)
        assert torch.equal(img.reshape(-1), flat[16 * b + (l & 15), 32 * kc + 8 * (l >> 4) + j, t // 3, t % 3])
        assert torch.equal(rrdb.unpack_conv_weight(img, cout), w16)
    for cin in (3, 12):
        w = torch.randn(64, cin, 3, 3, generator=g)
        p = rrdb.pack_head_weight(w)
        assert p.shape == (9 * cin, 64) and p[(3 * 1 + 2) * cin + cin - 1, 17] == w[17, cin - 1, 1, 2]
        assert torch.equal(rrdb.unpack_head_weight(p), w)
    for bad in (torch.zeros(32, 48, 3, 3), torch.zeros(32, 64, 1, 1)):
        with pytest.raises(ValueError, match="pack_conv_weight"):
            rrdb.pack_conv_weight(bad)
    with pytest.raises(ValueError, match="pack_head_weight"):
        rrdb.pack_head_weight(torch.zeros(64, 4, 3, 3))


def test_unshuffle_and_reflection_against_torch():
    g = torch.Generator().manual_seed(6)
    for h, w in ((2, 2), (5, 7), (6, 9), (4, 6), (33, 64)):
        x = torch.randn(h, w, 3, generator=g, dtype=torch.float64)
        nchw = x.permute(2, 0, 1)[None]
        want = F.pixel_unshuffle(F.pad(nchw, (0, w % 2, 0, h % 2), mode="reflect"), 2)[0].permute(1, 2, 0)
        assert torch.equal(R.unshuffle_by_index(x), want), (h, w)
    x = torch.randn(1, 4, 3, 5, generator=g)
    assert torch.equal(R.nearest2(x), F.interpolate(x, scale_factor=2, mode="nearest"))


class _RDB(nn.Module):
    def __init__(self):
        super().__init__()
        for k in range(1, 5):
            setattr(self, f"conv{k}", nn.Conv2d(64 + 32 * (k - 1), 32, 3, 1, 1))
        self.conv5 = nn.Conv2d(192, 64, 3, 1, 1)

    def forward(self, x):
        x1 = F.leaky_relu(self.conv1(x), 0.2)
        x2 = F.leaky_relu(self.conv2(torch.cat((x, x1), 1)), 0.2)
        x3 = F.leaky_relu(self.conv3(torch.cat((x, x1, x2), 1)), 0.2)
        x4 = F.leaky_relu(self.conv4(torch.cat((x, x1, x2, x3), 1)), 0.2)
        return self.conv5(torch.cat((x, x1, x2, x3, x4), 1)) * 0.2 + x


class _RRDB(nn.Module):
    def __init__(self):
        super().__init__()
        self.rdb1, self.rdb2, self.rdb3 = _RDB(), _RDB(), _RDB()

    def forward(self, x):
        return self.rdb3(self.rdb2(self.rdb1(x))) * 0.2 + x


class _Tree(nn.Module):
    """the public definition as a torch.nn tree: its state dict has the public key names"""

    def __init__(self, nb, scale):
        super().__init__()
        self.scale = scale
        self.conv_first = nn.Conv2d(3 if scale == 4 else 12, 64, 3, 1, 1)
        self.body = nn.Sequential(*[_RRDB() for _ in range(nb)])
        for n in ("conv_body", "conv_up1", "conv_up2", "conv_hr"):
            setattr(self, n, nn.Conv2d(64, 64, 3, 1, 1))
        self.conv_last = nn.Conv2d(64, 3, 3, 1, 1)

    def forward(self, x):
        feat = self.conv_first(F.pixel_unshuffle(x, 2) if self.scale == 2 else x)
        feat = feat + self.conv_body(self.body(feat))
        feat = F.leaky_relu(self.conv_up1(F.interpolate(feat, scale_factor=2, mode="nearest")), 0.2)
        feat = F.leaky_relu(self.conv_up2(F.interpolate(feat, scale_factor=2, mode="nearest")), 0.2)
        return self.conv_last(F.leaky_relu(self.conv_hr(feat), 0.2))


@pytest.mark.parametrize("nb,scale,h,w", [(1, 4, 5, 7), (2, 2, 7, 9), (2, 2, 6, 8)])
def test_restatement_against_an_independent_tree(nb, scale, h, w):
    sd, photo = R.make_state(nb, scale, seed=7), R.make_photo(h, w, seed=8)
    tree = _Tree(nb, scale).double()
    tree.load_state_dict({k: v.double() for k, v in sd.items()}, strict=True)
    x = torch.from_numpy(photo).double().permute(2, 0, 1)[None] / 255
    if scale == 2:
        x = F.pad(x, (0, w % 2, 0, h % 2), mode="reflect")
    with torch.no_grad():
        want = tree(x)[0].permute(1, 2, 0)[:scale * h, :scale * w]
    got = R.Net(sd, torch.float64, f16=False).forward(photo)
    assert got.shape == (scale * h, scale * w, 3)
    assert float((got - want).abs().max()) <= 1e-12 * max(1.0, float(want.abs().max()))


@pytest.mark.parametrize("scale,h,w", [(4, 50, 6), (2, 100, 6)])
def test_trunk_band_halo_on_both_sides(scale, h, w):
    """nb = 1: the derived halo (19 network rows: 19 photo rows at x4, 38 at x2) gives the unbanded values exactly; one network row less
    is visible"""
    from vspbfr_amd import rrdb
    sd, photo = R.make_state(1, scale, seed=9), R.make_photo(h, w, seed=10)
    halo = rrdb.net_halo(1, scale)
    sp = 1 if scale == 4 else 2
    assert halo == 19 * sp and rrdb.net_halo(23, 4) == 349 and rrdb.net_halo(23, 2) == 698
    net = R.Net(sd, torch.float64)
    whole = net.forward(photo)
    band = 4 * sp
    assert torch.equal(net.forward_banded(photo, band, halo), whole)
    assert not torch.equal(net.forward_banded(photo, band, halo - sp), whole)


def test_tail_band_halo_on_both_sides():
    from vspbfr_amd import rrdb
    sd, photo = R.make_state(1, 4, seed=11), R.make_photo(9, 5, seed=12)
    net = R.Net(sd, torch.float64)
    whole = net.forward(photo)
    assert rrdb.TAIL_HALO == 2
    assert torch.equal(net.forward(photo, tail_band=(3, rrdb.TAIL_HALO)), whole)
    assert not torch.equal(net.forward(photo, tail_band=(3, rrdb.TAIL_HALO - 1)), whole)


def test_planner_units_and_tail_bands():
    from vspbfr_amd import rrdb
    net = rrdb.RrdbUpscaler(R.make_state(1, 2, seed=13), "cpu")
    units, banded = net._units([(101, 40), (6, 7)], 7)            # 7 rounds up to 8: band starts on even rows
    assert banded == [True, True] and all(u[1] % 2 == 0 and u[3] % 2 == 0 for u in units)
    assert sorted(r for k, r0, r1, _, _ in units if k == 0 for r in range(r0, r1)) == list(range(101))
    assert units[1] == (0, 8, 16, 0, 54)
    assert net._units([(101, 40)], None) == ([(0, 0, 101, 0, 101)], [False])
    net.act_limit = 60 * 20 * 512                               # 60 network rows of 20 pixels
    units, banded = net._units([(400, 40)], None)
    assert banded == [True] and all(((-(-a1 // 2)) - a0 // 2) <= 60 for _, _, _, a0, a1 in units) and len(units) > 1
    with pytest.raises(ValueError, match="does not fit"):
        net._units([(400, 400)], None)
    with pytest.raises(ValueError, match="does not fit"):
        net._units([(400, 40)], 200)
    net.tail_limit = 1024 * 20 * 9                              # nine rows of the 2x map with the halo: bands of five
    bands = net.tail_bands(3, 21, 40, 20)
    assert bands[0] == (3, 8, 1, 10) and bands[-1] == (18, 21, 16, 23) and [b[0] for b in bands] == [3, 8, 13, 18]
    assert net.tail_bands(0, 40, 40, 20)[-1] == (35, 40, 33, 40)
    net.tail_limit = 1024 * 20 * 4
    with pytest.raises(ValueError, match="does not fit"):
        net.tail_bands(0, 40, 40, 20)
    with pytest.raises(ValueError, match="reflects an odd side"):
        net.upscale(photos=[np.zeros((1, 4, 3), np.uint8)])


@pytest.mark.parametrize("nb,scale,h,w", GPU_CASES)
def test_gpu_cases_are_mostly_unclamped(nb, scale, h, w):
    """a condition of the GPU tests, not a tolerance: at least half of the float64 outputs lie strictly inside (0, 1)"""
    _, _, ref, e_ref, bound = R.case(nb, scale, h, w)
    share = R.inside_share(ref)
    print(f"nb {nb} x{scale} {h}x{w}: inside {share:.3f} e_ref {e_ref:.3g} byte bound {bound:.3f}")
    assert share >= 0.5 and ref.shape == (scale * h, scale * w, 3)


def test_entries_refuse_what_they_do_not_serve():
    """validation precedes every launch: no GPU needed"""
    from vspbfr_amd import _lib
    L, p, q = _lib.lib, C.c_void_p(1 << 20), C.c_void_p(1 << 24)
    f = C.c_float

    def head(y=p, pitch=64, src=q, src_bytes=3 * 35, off=0, h=5, w=7, scale=4, row0=0, rows=5, wt=p, b=p):
        return L.vsp_rrdb_head_u8(y, pitch, src, src_bytes, off, h, w, scale, row0, rows, wt, b, None)

    def conv(y=p, yp=192, yo=64, x=p, xp=192, H=5, W=7, cin=64, cout=32, flags=1, w=q, b=q, r1=None, r1p=0, s1=0.0, r2=None, r2p=0, s2=0.0):
        return L.vsp_rrdb_conv_f16(y, yp, yo, x, xp, H, W, cin, cout, flags, w, b, r1, r1p, f(s1), r2, r2p, f(s2), None)

    def tail(out=q, out_bytes=3 * 20 * 28, off=0, pitch=3 * 28, ow=28, f32=None, info=q, x=p, xp=64, H=20, W=28, k0=0, kn=20, w=q, b=q):
        return L.vsp_rrdb_tail_u8(out, out_bytes, off, pitch, ow, f32, info, x, xp, H, W, k0, kn, w, b, None)

    other = C.c_void_p(1 << 22)
    for call, msg in ((lambda: head(y=None), "null pointer"), (lambda: head(src=None), "null pointer"), (lambda: head(b=None), "null pointer"),
                      (lambda: head(scale=3), "scale 3"), (lambda: head(h=0), "photo 0 x 7"), (lambda: head(w=-1), "photo 5 x -1"),
                      (lambda: head(scale=2, h=1, rows=1), "needs at least 2"), (lambda: head(scale=2, w=1, rows=3), "needs at least 2"),
                      (lambda: head(pitch=32), "pitch 32"), (lambda: head(pitch=66), "pitch 66"), (lambda: head(y=C.c_void_p(4100)), "aligned"),
                      (lambda: head(src_bytes=3 * 35 - 1), "outside src"), (lambda: head(off=1), "outside src"), (lambda: head(off=-1), "outside src"),
                      (lambda: head(rows=6), "rows 0..5 of 5"), (lambda: head(row0=-1), "rows"), (lambda: head(rows=0), "rows"),
                      (lambda: head(scale=2, rows=4), "rows 0..3 of 3"),
                      (lambda: conv(y=None), "null pointer"), (lambda: conv(w=None), "null pointer"), (lambda: conv(b=None), "null pointer"),
                      (lambda: conv(cin=32), "32 -> 32 channels"), (lambda: conv(cin=224, xp=224), "224 -> 32"), (lambda: conv(cin=80), "80 -> 32"),
                      (lambda: conv(cout=16), "64 -> 16"), (lambda: conv(cout=48), "64 -> 48"), (lambda: conv(H=0), "map 0 x 7"),
                      (lambda: conv(flags=4), "unknown flags"), (lambda: conv(r2=other, r2p=64), "second residual without a first"),
                      (lambda: conv(xp=60), "input pitch 60"), (lambda: conv(xp=68), "input pitch 68"), (lambda: conv(cin=96, xp=64, y=other), "input pitch 64"),
                      (lambda: conv(yp=80, y=other), "output pitch 80"), (lambda: conv(yo=66), "offset 66"), (lambda: conv(yp=194, y=other), "output pitch 194"),
                      (lambda: conv(y=other, r1=q, r1p=16), "residual pitch 16"), (lambda: conv(y=other, r1=q, r1p=34), "residual pitch 34"),
                      (lambda: conv(x=C.c_void_p((1 << 20) + 8), y=other), "aligned"), (lambda: conv(y=C.c_void_p((1 << 22) + 4)), "aligned"),
                      (lambda: conv(y=other, r1=C.c_void_p((1 << 24) + 4), r1p=64), "aligned"),
                      (lambda: conv(yo=32), "overlaps the channels"), (lambda: conv(cin=96, yo=64), "overlaps the channels"),
                      (lambda: conv(yo=64, flags=3), "overlaps the channels"), (lambda: conv(yp=256, yo=64), "overlaps the channels"),
                      (lambda: conv(y=C.c_void_p((1 << 20) + 128)), "overlaps the input"),
                      (lambda: conv(y=other, yo=0, r1=other, r1p=192, s1=1.0), "residual 1 aliases"),
                      (lambda: conv(y=other, yo=0, r1=q, r1p=64, r2=C.c_void_p((1 << 22) + 64), r2p=192), "residual 2 aliases"),
                      (lambda: tail(out=None), "null pointer"), (lambda: tail(info=None), "null pointer"), (lambda: tail(x=None), "null pointer"),
                      (lambda: tail(W=0), "map 20 x 0"), (lambda: tail(xp=32), "input pitch 32"), (lambda: tail(x=C.c_void_p(4104)), "aligned"),
                      (lambda: tail(kn=21), "rows 0..20 of 20"), (lambda: tail(k0=-1), "rows"), (lambda: tail(kn=0), "rows"), (lambda: tail(k0=20, kn=1), "rows"),
                      (lambda: tail(ow=29), "29 columns of 28"), (lambda: tail(ow=0), "0 columns"), (lambda: tail(out_bytes=3 * 20 * 28 - 1), "outside out"),
                      (lambda: tail(off=1), "outside out"), (lambda: tail(off=-3), "outside out"), (lambda: tail(pitch=83), "outside out")):
        rc = call()
        assert rc == -1 and msg in _lib.last_error(), (rc, msg, _lib.last_error())
    two = 1 << 31
    assert head(src_bytes=two) == -3 and "2 GiB" in _lib.last_error()
    assert head(h=4096, w=4096, rows=4096, src_bytes=3 << 24) == -3 and head(h=4096, w=4096, rows=4095, src_bytes=3 << 24, y=None) == -1
    assert conv(y=C.c_void_p(1 << 40), H=4096, W=4096, xp=64, yp=64, yo=0) == -3 and "2 GiB" in _lib.last_error()
    assert conv(y=C.c_void_p(1 << 40), H=2048, W=4096, xp=128, yp=64, yo=0) == -3 and "2 GiB" in _lib.last_error()
    assert conv(y=C.c_void_p(1 << 40), H=2048, W=2048, xp=64, yp=64, yo=0, flags=3) == -3
    assert tail(out_bytes=two) == -3 and tail(out_bytes=two // 4, f32=p) == -3 and tail(H=4096, W=4096) == -3


def test_describe_and_interface():
    from vspbfr_amd import rrdb, upscale
    from vspbfr_amd.photo import PhotoRestorer
    net = rrdb.RrdbUpscaler(R.make_state(2, 2, seed=14), "cpu", band_rows=12)
    assert isinstance(net, upscale.SrUpscaler) and (net.scale, net.num_block, net.band_rows, net.halo) == (2, 2, 12, 68)
    assert net.describe() == {"model": "RRDBNet", "num_block": 2, "scale": 2, "banded": False, "nonfinite": []}
    assert net.describe(True, ["a.png"]) == {"model": "RRDBNet", "num_block": 2, "scale": 2, "banded": True, "nonfinite": ["a.png"]}
    assert len(net.convs) == 15 * 2 + 4 and net.convs["body.1.rdb3.conv5"][0].shape == (6, 9, 4, 64, 8) and net.head[0].shape == (108, 64)
    assert net.tail[0].shape == (2, 9, 1, 64, 8) and net.tail[1].shape == (16,) and float(net.tail[1][3:].abs().max()) == 0
    with pytest.raises(ValueError, match="cannot fill an upscale of 4"):
        net.upscale_to(4, photos=[np.zeros((4, 4, 3), np.uint8)])
    with pytest.raises(ValueError, match="cannot fill an upscale of 4"):
        PhotoRestorer(None, 1, upscale=4, background=net)
    assert PhotoRestorer(None, 1, upscale=2, background=net).background is net


def test_cli_dispatch_by_key(tmp_path, capsys):
    """an RRDBNet file reaches rrdb; a compact file and a junk file behave as before; a x2 RRDBNet at --upscale 4 is a parser error"""
    import argparse
    from vspbfr_amd import restore_photos, rrdb, upscale
    x2, x4, compact, junk, broken = (tmp_path / n for n in ("x2.pth", "x4.pth", "compact.pth", "junk.pth", "broken.pth"))
    torch.save({"params_ema": R.make_state(1, 2, seed=15)}, x2)
    torch.save({"params": {"module." + k: v for k, v in R.make_state(1, 4, seed=16).items()}}, x4)
    torch.save({"params": sr_ref.make_state(2, 4, seed=17)}, compact)
    torch.save({"weight": torch.zeros(3)}, junk)
    bad = R.make_state(1, 4, seed=18)
    bad.pop("conv_up2.bias")
    torch.save(bad, broken)
    ap = argparse.ArgumentParser()
    st = upscale.check_background_arguments(ap, str(x2), 2)
    assert isinstance(st, rrdb.RrdbState) and (st.num_block, st.scale) == (1, 2)
    st = upscale.check_background_arguments(ap, str(x4), None, 16)
    assert isinstance(st, rrdb.RrdbState) and st.scale == 4
    assert isinstance(upscale.make_upscaler(st, "cpu", 16), rrdb.RrdbUpscaler)
    assert upscale.check_background_arguments(ap, str(x4), 2).scale == 4
    st = upscale.check_background_arguments(ap, str(compact), 4)
    assert isinstance(st, upscale.SrState) and st.num_conv == 2
    assert type(upscale.make_upscaler(st, "cpu")) is upscale.SrUpscaler
    assert upscale.is_rrdb_state({"params": {"module.conv_first.weight": 0}}) and not upscale.is_rrdb_state({"body.0.weight": 0}) \
        and not upscale.is_rrdb_state([1])
    # upscale.check_state_dict itself stays as it was
    with pytest.raises(ValueError, match="no body.N.weight key"):
        upscale.check_state_dict({"conv_first.weight": torch.zeros(64, 3, 3, 3)})
    (tmp_path / "photos").mkdir()
    base = ["--photos", str(tmp_path / "photos"), "--out", str(tmp_path / "out"), "--landmarks", str(tmp_path / "none.json")]

    def refused(main, argv, msg):
        with pytest.raises(SystemExit) as e:
            main(argv)
        err = capsys.readouterr().err
        assert e.value.code == 2 and msg in err, err

    refused(restore_photos.main, base + ["--bg_weights", str(x2), "--upscale", "4"], "x2 network: it cannot fill an upscale of 4")
    refused(restore_photos.main, base + ["--bg_weights", str(x2)], "needs an upscale of 2 or 4, not 1")
    refused(restore_photos.main, base + ["--bg_weights", str(junk), "--upscale", "2"], "no body.N.weight key")
    refused(restore_photos.main, base + ["--bg_weights", str(broken), "--upscale", "2"], "missing keys conv_up2.bias")
    own = ["--photos", str(tmp_path / "photos"), "--out", str(tmp_path / "out")]
    refused(upscale.main, own + ["--weights", str(x2), "--scale", "4"], "x2 network: it cannot fill an upscale of 4")
    refused(upscale.main, own + ["--weights", str(broken)], "RRDBNet checkpoint")
    refused(upscale.main, own + ["--weights", str(junk)], "SRVGGNetCompact checkpoint: no body.N.weight key")
