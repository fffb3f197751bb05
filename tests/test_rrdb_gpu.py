"""GPU checks of the RRDBNet background upscaler (csrc/rrdb.hip through vspbfr_amd/rrdb.py) against tests/rrdb_ref.py in float64.

Bounds (derived, never fitted): with e_ref = max |restatement float32 - restatement float64| of the same case,
    f16 kernel output:  |y - ref64| <= 1/2 f16 ulp at ref64 + 4 e_ref + 2e-6 max |ref64|, e_ref and ref64 before the final rounding to f16;
    fp32 net output:    |v - ref64| <= 4 e_ref + 2e-6 max |ref64|;
    u8 net output:      |u8 - 255 clamp(ref64)| <= 0.5 + 255 (4 e_ref + 2e-6 max |ref64|), every byte.
Every case prints e_ref / e_hip / ratio under -s.  The tile is 8 rows x 32 columns: the maps sit one below, on and one above it, besides
1 x 1, 1 x 9, 5 x 7 and 33 x 65 (more than one tile each way)."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import rrdb_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
MAPS = [(1, 1), (1, 9), (5, 7), (8, 32), (9, 33), (7, 31), (33, 65)]
NETS = [(1, 4, 5, 7), (2, 4, 9, 33), (2, 2, 11, 13), (3, 4, 17, 20), (23, 4, 9, 11)]
GUARD = 4096                                                  # sentinel elements behind every output buffer
NAN = float("nan")


def _report(name, e_ref, e_hip):
    print(f"{name}: e_ref {e_ref:.3g} e_hip {e_hip:.3g} ratio {e_hip / max(e_ref, 1e-30):.3g}")


def _check_f16(name, got, pre64, pre32):
    """got: the kernel's f16 values as float64, in the layout of pre64"""
    e_ref = float((pre32.double() - pre64).abs().max())
    bound = R.f16_half_ulp(pre64) + 4 * e_ref + 2e-6 * float(pre64.abs().max())
    err = (got - pre64).abs()
    _report(name, e_ref, float(err.max()))
    assert torch.isfinite(got).all() and bool((err <= bound).all()), (name, float((err - bound).max()))


def _acts(h, w, c, g, scale=0.5):
    """(h, w, c) float64 of f16 values, some of them tiny or zero"""
    a = torch.randn(h, w, c, generator=g) * scale
    a[:, :, ::7] *= 1e-6
    return a.to(torch.float16).double()


def _weights(cout, cin, g):
    from vspbfr_amd import rrdb
    w = torch.randn(cout, cin, 3, 3, generator=g) * (1.6 / (9 * cin)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.05
    return w.to(torch.float16), b, rrdb.pack_conv_weight(w).to(DEV), b.to(DEV)


def _ref_conv(x, w16, b, dtype, act, up, res):
    """x (H, W, Cin) float64 of f16 values -> (OH, OW, Cout) in dtype, before the rounding to f16"""
    xi = x.to(dtype).permute(2, 0, 1)[None]
    if up:
        xi = R.nearest2(xi)
    v = F.conv2d(xi, w16.to(dtype), b.to(dtype), padding=1)[0].permute(1, 2, 0)
    if act:
        v = R.lrelu(v)
    for r, s in res:
        v = s * v + r.to(dtype)
    return v


# name: (Cin, Cout, act, up, residual scales, slice)
CONVS = {"64to32": (64, 32, True, False, (), True), "96to32": (96, 32, True, False, (), True), "128to32": (128, 32, True, False, (), True),
         "160to32": (160, 32, True, False, (), True), "192to32": (192, 32, True, False, (), True),
         "192to64_res": (192, 64, False, False, (0.2,), False), "192to64_res2": (192, 64, False, False, (0.2, 0.2), False),
         "64to64": (64, 64, False, False, (), False), "64to64_res1": (64, 64, False, False, (1.0,), False), "64to64_up": (64, 64, True, True, (), False)}


@pytest.mark.parametrize("name", list(CONVS))
def test_conv_alone(name):
    """slice: the output is the 32-channel slice at offset Cin of the tensor it reads (pitch Cin + 64: a neighbouring slice behind it);
    otherwise a tensor of its own at channel offset 4 of a pitch of Cout + 8.  NaN fills every channel of the input at and above Cin and
    every channel of a residual at and above Cout: none of them may be read, and all but the slice written must keep their bits."""
    from vspbfr_amd import hip_ops as H
    cin, cout, act, up, scales, slc = CONVS[name]
    g = torch.Generator().manual_seed(sum(map(ord, name)))
    w16, b, img, bd = _weights(cout, cin, g)
    for h, w in MAPS:
        oh, ow = (2 * h, 2 * w) if up else (h, w)
        x = _acts(h, w, cin, g)
        xp = cin + 64 if slc else cin + 8
        xt = torch.full((h * w * xp + GUARD,), NAN, dtype=torch.float16)
        xt[:h * w * xp].view(h, w, xp)[:, :, :cin] = x.to(torch.float16)
        xt[h * w * xp:] = 7.0
        xd = xt.to(DEV)
        res, res_arg = [], []
        for s in scales:
            r = _acts(oh, ow, cout, g)
            rt = torch.full((oh * ow * (cout + 4),), NAN, dtype=torch.float16)
            rt.view(oh, ow, cout + 4)[:, :, :cout] = r.to(torch.float16)
            res.append((r, s))
            res_arg.append((rt.to(DEV), cout + 4, s))
        res_arg += [None] * (2 - len(res_arg))
        if slc:
            yd, yp, yo = xd, xp, cin
        else:
            yp, yo = cout + 8, 4
            yd = torch.full((oh * ow * yp + GUARD,), 7.0, dtype=torch.float16, device=DEV)
        H.rrdb_conv_f16(yd, yp, yo, xd, xp, h, w, img, bd, act=act, up=up, res1=res_arg[0], res2=res_arg[1])
        torch.cuda.synchronize()
        pre64, pre32 = (_ref_conv(x, w16, b, dt, act, up, res) for dt in (torch.float64, torch.float32))
        yt = yd.cpu()
        full = yt[:oh * ow * yp].view(oh, ow, yp)
        _check_f16(f"conv {name} {h}x{w}", full[:, :, yo:yo + cout].double(), pre64, pre32)
        assert (yt[oh * ow * yp:] == 7.0).all(), "written behind the output"
        if slc:
            assert torch.equal(full[:, :, :cin], x.to(torch.float16)) and torch.isnan(full[:, :, cin + cout:]).all()
        else:
            assert (full[:, :, :yo] == 7.0).all() and (full[:, :, yo + cout:] == 7.0).all()
            assert torch.equal(xd.cpu().view(torch.int16), xt.view(torch.int16))


@pytest.mark.parametrize("scale", [4, 2])
def test_head_alone(scale):
    from vspbfr_amd import hip_ops as H
    from vspbfr_amd import rrdb
    sd = R.make_state(1, scale, seed=21)
    n64, n32 = R.Net(sd, torch.float64), R.Net(sd, torch.float32)
    wp, bd = rrdb.pack_head_weight(sd["conv_first.weight"]).to(DEV), sd["conv_first.bias"].to(DEV)
    for (h, w), off, window in (((2, 2), 1, None), ((5, 7), 3, None), ((6, 9), 1, (1, 2)), ((33, 64), 3, None), ((33, 64), 1, (7, 9))):
        photo = R.make_photo(h, w, seed=h * w)
        flat = np.concatenate([np.full(off, 255, np.uint8), photo.reshape(-1), np.full(5, 255, np.uint8)])
        nh, nw = rrdb.net_rows(h, scale), rrdb.net_rows(w, scale)
        row0, rows = window if window and window[0] + window[1] <= nh else (0, nh)
        y = torch.full((rows * nw * 72 + GUARD,), 7.0, dtype=torch.float16, device=DEV)
        assert H.rrdb_head_u8(y, 72, torch.from_numpy(flat).to(DEV), off, h, w, scale, wp, bd, row0=row0, rows=rows) == (rows, nw)
        torch.cuda.synchronize()
        pre64, pre32 = (n.conv("conv_first", n.net_input(photo))[0].permute(1, 2, 0)[row0:row0 + rows] for n in (n64, n32))
        yt = y.cpu()
        full = yt[:rows * nw * 72].view(rows, nw, 72)
        _check_f16(f"head x{scale} {h}x{w} rows {row0}+{rows}", full[:, :, :64].double(), pre64, pre32)
        assert (full[:, :, 64:] == 7.0).all() and (yt[rows * nw * 72:] == 7.0).all()


def test_tail_alone():
    """bytes and the fp32 copy, a kept-row window, the crop of columns and rows on odd sizes, and a planted f16 infinity"""
    from vspbfr_amd import hip_ops as H
    from vspbfr_amd import rrdb
    g = torch.Generator().manual_seed(31)
    w = torch.randn(3, 64, 3, 3, generator=g) * (0.05 / (9 * 64)) ** 0.5
    b = torch.randn(3, generator=g) * 0.05 + 0.5
    w16, img = w.to(torch.float16), rrdb.pack_conv_weight(w).to(DEV)
    b16 = torch.zeros(16)
    b16[:3] = b
    bd = b16.to(DEV)
    for (h, wd), (k0, kn), ow, plant in (((1, 1), (0, 1), 1, None), ((5, 7), (0, 5), 7, None), ((9, 33), (2, 5), 31, None), ((12, 36), (0, 10), 34, None),
                                         ((33, 65), (8, 25), 65, (20, 40, 5)), ((7, 31), (0, 7), 31, (0, 0, 63))):
        x = _acts(h, wd, 64, g, scale=1.0)
        xt = x.to(torch.float16)
        if plant:
            xt[plant] = float("inf")
        pitch, off = 3 * ow + 2, 5
        n = off + kn * pitch + GUARD
        out = torch.full((n,), 99, dtype=torch.uint8, device=DEV)
        f32 = torch.full((n,), 7.0, dtype=torch.float32, device=DEV)
        info = torch.zeros(1, dtype=torch.int32, device=DEV)
        H.rrdb_tail_u8(out, off, pitch, ow, info, xt.reshape(-1).to(DEV), 64, h, wd, k0, kn, img, bd, out_f32=f32)
        torch.cuda.synchronize()
        v64, v32 = (F.conv2d(x.to(dt).permute(2, 0, 1)[None], w16.to(dt), b.to(dt), padding=1)[0].permute(1, 2, 0)[k0:k0 + kn, :ow]
                    for dt in (torch.float64, torch.float32))
        e_ref = float((v32.double() - v64).abs().max())
        bound = 4 * e_ref + 2e-6 * float(v64.abs().max())
        assert v64.numel() < 100 or R.inside_share(v64) >= 0.5
        ot, ft = out.cpu(), f32.cpu()
        rows_u8 = torch.stack([ot[off + r * pitch: off + r * pitch + 3 * ow] for r in range(kn)]).view(kn, ow, 3)
        rows_f = torch.stack([ft[off + r * pitch: off + r * pitch + 3 * ow] for r in range(kn)]).view(kn, ow, 3)
        ok = torch.ones(kn, ow, dtype=torch.bool)
        if plant:
            py, px, _ = plant
            for yy in range(max(py - 1, 0), min(py + 2, h)):
                for xx in range(max(px - 1, 0), min(px + 2, wd)):
                    if k0 <= yy < k0 + kn and xx < ow:
                        ok[yy - k0, xx] = False
            assert not ok.all() and (rows_u8[~ok] == 0).all() and not torch.isfinite(rows_f[~ok]).any()
        assert int(info.item()) == (H.RRDB_NONFINITE if plant else 0)
        e_f = float((rows_f.double() - v64)[ok].abs().max())
        e_b = float((rows_u8.double() - 255 * v64.clamp(0, 1))[ok].abs().max())
        _report(f"tail {h}x{wd} rows {k0}+{kn} cols {ow}", e_ref, e_f)
        assert e_f <= bound and e_b <= 0.5 + 255 * bound, (e_f, e_b, bound)
        # nothing but the kept rows' bytes is written
        mask = torch.ones(n, dtype=torch.bool)
        for r in range(kn):
            mask[off + r * pitch: off + r * pitch + 3 * ow] = False
        assert (ot[mask] == 99).all() and (ft[mask] == 7.0).all()


@pytest.fixture(scope="module")
def nets():
    from vspbfr_amd import rrdb
    cache = {}

    def get(nb, scale, h, w):
        if (nb, scale, h, w) not in cache:
            sd = R.case(nb, scale, h, w)[0]
            cache[(nb, scale, h, w)] = rrdb.RrdbUpscaler(sd, DEV)
        return cache[(nb, scale, h, w)]
    return get


@pytest.mark.parametrize("nb,scale,h,w", NETS)
def test_whole_net(nets, nb, scale, h, w):
    sd, photo, ref, e_ref, byte_bound = R.case(nb, scale, h, w)
    assert R.inside_share(ref) >= 0.5
    net = nets(nb, scale, h, w)
    n = 3 * scale * h * scale * w
    f32 = torch.zeros(n, dtype=torch.float32, device=DEV)
    out, info = net.upscale(photos=[photo], out_f32=f32)
    again, _ = net.upscale(photos=[photo])
    assert torch.equal(out, again), "two launches differ"
    assert info["shapes"] == [(scale * h, scale * w)] and info["launches"] == 15 * nb + 4 + 3 and info["flags"].tolist() == [0]
    v = f32.cpu().view(scale * h, scale * w, 3).double()
    e_f = float((v - ref).abs().max())
    e_b = float((out.cpu().view(scale * h, scale * w, 3).double() - 255 * ref.clamp(0, 1)).abs().max())
    _report(f"net nb {nb} x{scale} {h}x{w} (byte error {e_b:.3f} of {byte_bound:.3f})", e_ref, e_f)
    assert e_f <= (byte_bound - 0.5) / 255 and e_b <= byte_bound


def test_bands_equal_the_unbanded_bytes(nets):
    """band_rows; the trunk guard and the guard of the 4x maps scaled down, each on its own"""
    from vspbfr_amd import rrdb
    for nb, scale, h, w, rows in ((1, 4, 45, 9, 5), (1, 2, 90, 13, 6)):
        net = rrdb.RrdbUpscaler(R.make_state(nb, scale, seed=41), DEV)
        photo = R.make_photo(h, w, seed=42)
        whole, iw = net.upscale(photos=[photo])
        assert iw["banded"] == [False] and iw["launches"] == 15 * nb + 4 + 3
        cut, ic = net.upscale(photos=[photo], band_rows=rows)
        assert ic["banded"] == [True] and ic["launches"] > 2 * (15 * nb + 7) and torch.equal(cut, whole)
        nw = (w + 1) // 2 if scale == 2 else w
        limits = net.act_limit, net.tail_limit
        try:
            net.tail_limit = 1024 * nw * 7                      # bands of three rows of the 2x map
            tb, it = net.upscale(photos=[photo])
            assert it["banded"] == [False] and it["launches"] > 15 * nb + 4 + 3 * 8 and torch.equal(tb, whole)
            net.tail_limit = limits[1]
            net.act_limit = 512 * nw * (2 * (15 * nb + 4) + 1 + 3)     # trunk bands of three network rows
            ab, ia = net.upscale(photos=[photo])
            assert ia["banded"] == [True] and torch.equal(ab, whole)
        finally:
            net.act_limit, net.tail_limit = limits


def test_device_photos_equal_the_numpy_source(nets):
    net = nets(2, 2, 11, 13)
    photos = [R.make_photo(11, 13, seed=51), R.make_photo(6, 9, seed=52)]
    a, ia = net.upscale(photos=photos)
    assert ia["shapes"] == [(22, 26), (12, 18)]
    flat = np.concatenate([np.zeros(5, np.uint8), photos[0].reshape(-1), np.zeros(3, np.uint8), photos[1].reshape(-1)])
    offs = [5, 5 + photos[0].size + 3]
    dst = torch.full((a.numel() + 63,), 99, dtype=torch.uint8, device=DEV)
    b, _ = net.upscale(device_photos=(torch.from_numpy(flat).to(DEV), offs, [(11, 13), (6, 9)]), out=dst, out_offsets=[63, 63 + ia["offsets"][1]])
    assert b is dst and torch.equal(b[63:], a) and (b[:63] == 99).all()


def test_x4_net_at_upscale_2_is_the_ragged_resize_of_its_own_output(nets):
    from vspbfr_amd.resample import ResamplePlan
    net = nets(1, 4, 5, 7)
    photos = [R.make_photo(24, 36, seed=61), R.make_photo(17, 40, seed=62)]
    out, info = net.upscale_to(2, photos=photos)
    assert info["shapes"] == [(48, 72), (34, 80)]
    big, ib = net.upscale(photos=photos)
    assert torch.equal(big, info["net_out"])
    plan = ResamplePlan(ib["shapes"], [(w, h) for h, w in info["shapes"]], [(0, 0)] * 2, None, device_sources=(big, ib["offsets"]),
                        out_sizes=info["shapes"])
    assert torch.equal(plan.run_into(torch.empty(plan.out_bytes, dtype=torch.uint8, device=DEV)), out)
    assert out.float().std() > 5


def test_background_then_paste_keeps_the_networks_bytes_outside_the_boxes(nets):
    import photo_ref as P0
    from vspbfr_amd import photo as P
    net = nets(2, 2, 11, 13)
    photos = [P0.test_photo(90, 80, seed=3), P0.test_photo(50, 64, seed=4)]
    faces = [(0, P0.landmarks_for(2.0, 10.0, (45.0, 40.0), 64)), (1, P0.landmarks_for(2.5, -20.0, (20.0, 30.0), 64))]
    plan = P.FacePlan(photos, faces, size=64, upscale=2)
    bg = plan.background(DEV, upscaler=net)
    alone, info = net.upscale(photos=photos)
    assert torch.equal(bg, alone) and info["offsets"] == plan.out_off and info["shapes"] == plan.out_shape
    assert not torch.equal(bg, plan.background(DEV))          # the LANCZOS background is another picture
    restored = torch.from_numpy(np.stack([P0.test_photo(64, 64, seed=101 + i) for i in range(2)])).to(DEV)
    out = P.paste_faces(plan, restored, DEV, out=bg.clone())
    changed = 0
    for k, (o, b) in enumerate(zip(plan.split(out), plan.split(alone))):
        outside = torch.ones(o.shape[:2], dtype=torch.bool, device=DEV)
        for i, (x0, y0, x1, y1) in enumerate(plan.boxes):
            if plan.face_photo[i] == k:
                outside[y0:y1, x0:x1] = False
        assert outside.any() and torch.equal(o[outside], b[outside])
        changed += int((o != b).any())
    assert changed == 2
    with pytest.raises(ValueError, match="cannot fill an upscale of 4"):
        P.FacePlan(photos, faces, size=64, upscale=4).background(DEV, upscaler=net)
