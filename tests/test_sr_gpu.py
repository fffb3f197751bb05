"""GPU checks of the background upscaler (csrc/sr.hip through vspbfr_amd/upscale.py) against tests/sr_ref.py in float64.

Bounds (derived, never fitted): with e_ref = max |restatement float32 - restatement float64| of the same case,
    f16 kernel output:  |y - ref64| <= 1/2 f16 ulp at ref64 (2^-24 in the subnormal range) + 4 e_ref + 2e-6 max |ref64|, e_ref and ref64
                        taken before the final rounding to f16;
    fp32 net output:    |v - ref64| <= 4 e_ref + 2e-6 max |ref64|;
    u8 net output:      |u8 - 255 clamp(ref64)| <= 0.5 + 255 (4 e_ref + 2e-6 max |ref64|), every byte.
Every case prints e_ref / e_hip / ratio under -s.  The tile is 8 rows x 32 columns: the sizes sit one below, on and one above it in
each direction, besides 1 x 1, 5 x 7, 33 x 65 and a ragged group of three in one launch."""

import numpy as np
import pytest
import torch

import sr_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
SIZES = [(1, 1), (5, 7), (7, 31), (8, 32), (9, 33), (7, 33), (9, 31), (33, 65)]
GROUP = [(9, 33), (1, 1), (5, 40)]
CASES = [[s] for s in SIZES] + [GROUP]
IDS = ["x".join(map(str, s)) for s in SIZES] + ["ragged"]
GUARD = 4096                                                  # sentinel elements behind every output buffer


def _photos(shapes, seed=20):
    return [R.test_photo(h, w, seed=seed + k) for k, (h, w) in enumerate(shapes)]


def _acts(shapes, seed=40):
    """per item a (1, 64, h, w) float64 tensor of f16 values, some of them subnormal or zero"""
    g = torch.Generator().manual_seed(seed)
    out = []
    for h, w in shapes:
        a = torch.randn(1, 64, h, w, generator=g) * 0.5
        a[:, ::7] *= 1e-6
        out.append(a.to(torch.float16).to(torch.float64))
    return out


def _table(shapes, scale):
    from vspbfr_amd import upscale as U
    src = np.concatenate([[0], np.cumsum([3 * h * w for h, w in shapes])]).tolist()
    out = np.concatenate([[0], np.cumsum([3 * h * w * scale * scale for h, w in shapes])]).tolist()
    tab, px = U.item_table([(k, 0, h, 0, h) for k, (h, w) in enumerate(shapes)], shapes, src, out, scale)
    return tab, torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(DEV), px, out


def _nhwc(acts):
    return torch.cat([a[0].permute(1, 2, 0).reshape(-1) for a in acts]).to(torch.float16)


def _report(name, e_ref, e_hip):
    print(f"{name}: e_ref {e_ref:.3g} e_hip {e_hip:.3g} ratio {e_hip / max(e_ref, 1e-30):.3g}")


def _check_f16(name, got, pre64, pre32):
    """got: the kernel's f16 values as float64, in the layout of pre64"""
    pre64, pre32 = pre64.numpy(), pre32.double().numpy()
    e_ref, half = np.abs(pre32 - pre64).max(), 0.5 * R.f16_ulp(pre64)
    err = np.abs(got - pre64)
    _report(name, e_ref, np.maximum(err - half, 0).max())
    assert np.isfinite(got).all() and (err <= half + 4 * e_ref + 2e-6 * np.abs(pre64).max()).all(), name


def _layer(seed, cout=64, var=1.6):
    g = torch.Generator().manual_seed(seed)
    return (torch.randn(cout, 64, 3, 3, generator=g) * (var / 576) ** 0.5, torch.randn(cout, generator=g) * 0.05,
            torch.rand(64, generator=g) * 0.75 - 0.25)


@pytest.mark.parametrize("shapes", CASES, ids=IDS)
def test_head_alone(shapes):
    from vspbfr_amd import hip_ops as H, upscale as U
    sd = R.make_state(1, 2, seed=50)
    w, b, a = sd["body.0.weight"], sd["body.0.bias"], sd["body.1.weight"]
    photos = _photos(shapes)
    tab, tab_dev, px, _ = _table(shapes, 2)
    src = torch.from_numpy(np.concatenate([p.reshape(-1) for p in photos])).to(DEV)
    y = torch.full((px * 64 + GUARD,), 7.0, dtype=torch.float16, device=DEV)
    H.sr_head_u8(y[:px * 64], src, tab, tab_dev, len(shapes), U.pack_head_weight(w).to(DEV), b.to(DEV), a.to(DEV))
    y = y.cpu().double()
    assert (y[px * 64:] == 7.0).all()
    pre64 = torch.cat([R.head_pre(p, w, b, a, torch.float64)[0].permute(1, 2, 0).reshape(-1) for p in photos])
    pre32 = torch.cat([R.head_pre(p, w, b, a, torch.float32)[0].permute(1, 2, 0).reshape(-1) for p in photos])
    _check_f16(f"head {shapes}", y[:px * 64].numpy(), pre64, pre32)


@pytest.mark.parametrize("shapes", CASES, ids=IDS)
def test_body_alone(shapes):
    from vspbfr_amd import hip_ops as H, upscale as U
    w, b, a = _layer(51)
    acts = _acts(shapes)
    tab, tab_dev, px, _ = _table(shapes, 2)
    x = _nhwc(acts).to(DEV)
    y = torch.full((px * 64 + GUARD,), 7.0, dtype=torch.float16, device=DEV)
    H.sr_body_f16(y[:px * 64], x, tab, tab_dev, len(shapes), U.pack_body_weight(w).to(DEV), b.to(DEV), a.to(DEV))
    y = y.cpu().double()
    assert (y[px * 64:] == 7.0).all()
    pre64 = torch.cat([R.body_pre(t, w, b, a, torch.float64)[0].permute(1, 2, 0).reshape(-1) for t in acts])
    pre32 = torch.cat([R.body_pre(t, w, b, a, torch.float32)[0].permute(1, 2, 0).reshape(-1) for t in acts])
    _check_f16(f"body {shapes}", y[:px * 64].numpy(), pre64, pre32)


@pytest.mark.parametrize("scale", [2, 4])
@pytest.mark.parametrize("shapes", CASES, ids=IDS)
def test_tail_alone(shapes, scale):
    from vspbfr_amd import hip_ops as H, upscale as U
    w, b, _ = _layer(52 + scale, cout=3 * scale * scale, var=0.4)
    acts, photos = _acts(shapes), _photos(shapes)
    tab, tab_dev, px, offs = _table(shapes, scale)
    src = torch.from_numpy(np.concatenate([p.reshape(-1) for p in photos])).to(DEV)
    nbytes = offs[-1]
    out = torch.full((nbytes + GUARD,), 99, dtype=torch.uint8, device=DEV)
    f32 = torch.full((nbytes,), float("nan"), dtype=torch.float32, device=DEV)
    info = torch.zeros(len(shapes), dtype=torch.int32, device=DEV)
    img = U.pack_body_weight(w)
    bias = torch.zeros(16 * img.shape[1])
    bias[:b.numel()] = b
    H.sr_tail_u8(out[:nbytes], info, _nhwc(acts).to(DEV), src, tab, tab_dev, len(shapes), img.to(DEV), bias.to(DEV), scale, out_f32=f32)
    out, f32 = out.cpu().numpy(), f32.cpu().double().numpy()
    assert (out[nbytes:] == 99).all() and not info.cpu().any()
    v64 = torch.cat([R.tail_pre(t, p, w, b, scale, torch.float64).reshape(-1) for t, p in zip(acts, photos)])
    v32 = torch.cat([R.tail_pre(t, p, w, b, scale, torch.float32).reshape(-1) for t, p in zip(acts, photos)])
    _check_net(f"tail x{scale} {shapes}", out[:nbytes], f32, v64, v32)


def _check_net(name, u8, f32, v64, v32):
    v64n = v64.numpy()
    e_ref = np.abs(v32.double().numpy() - v64n).max()
    tol = 4 * e_ref + 2e-6 * np.abs(v64n).max()
    err = np.abs(f32 - v64n)
    _report(name + " fp32", e_ref, err.max())
    assert np.isfinite(f32).all() and (err <= tol).all(), name
    err8 = np.abs(u8.astype(np.float64) - 255 * np.clip(v64n, 0, 1))
    print(f"{name} u8: worst {err8.max():.4f} of {0.5 + 255 * tol:.4f}; bytes off the float64 rounding {np.mean(u8 != R.quantise(v64).reshape(-1)):.4f}")
    assert (err8 <= 0.5 + 255 * tol).all(), name


NETS = [(2, 2, (5, 7)), (16, 2, (37, 53)), (32, 4, (33, 65)), (32, 4, (64, 96))]


@pytest.fixture(scope="module")
def nets():
    """the upscalers of the whole-net cases, built once"""
    from vspbfr_amd import upscale as U
    out = {}
    for nc, s, _ in NETS:
        if (nc, s) not in out:
            sd = R.make_state(nc, s, seed=60 + nc)
            out[(nc, s)] = (sd, U.SrUpscaler(sd, DEV))
    return out


@pytest.fixture(scope="module")
def photo64():
    """the 64 x 96 photo through the 32-convolution x4 net, unbanded: the bytes the band, group and source tests compare with"""
    return R.test_photo(64, 96, seed=70)


@pytest.mark.parametrize("nc,s,hw", NETS, ids=[f"{nc}conv_x{s}_{h}x{w}" for nc, s, (h, w) in NETS])
def test_whole_net(nets, nc, s, hw):
    sd, net = nets[(nc, s)]
    x = R.test_photo(*hw, seed=70)
    f32 = torch.full((3 * s * s * hw[0] * hw[1],), float("nan"), dtype=torch.float32, device=DEV)
    out, info = net.upscale(photos=[x], out_f32=f32)
    assert info["launches"] == nc + 2 and info["shapes"] == [(s * hw[0], s * hw[1])] and not info["flags"].cpu().any()
    _check_net(f"net {nc} conv x{s} {hw}", out.cpu().numpy(), f32.cpu().double().numpy(), R.net(sd, x, torch.float64).reshape(-1),
               R.net(sd, x, torch.float32).reshape(-1))


def test_a_group_equals_each_photo_alone(nets):
    _, net = nets[(32, 4)]
    photos = _photos([(9, 33), (40, 17), (1, 5), (33, 65)], seed=80)
    out, info = net.upscale(photos=photos)
    assert info["launches"] == 34
    for p, o, (h, w) in zip(photos, info["offsets"], info["shapes"]):
        alone, _ = net.upscale(photos=[p])
        assert torch.equal(out[o:o + 3 * h * w], alone)


@pytest.mark.parametrize("rows", [8, 40])
def test_bands_equal_the_unbanded_bytes(nets, photo64, rows):
    _, net = nets[(32, 4)]
    whole, _ = net.upscale(photos=[photo64])
    banded, info = net.upscale(photos=[photo64], band_rows=rows)
    assert info["banded"] == [True] and info["launches"] == 34 and torch.equal(banded, whole)


def test_the_activation_guard_bands_and_splits_on_its_own(nets):
    """the 2 GiB guard scaled down: the photo is cut without being asked, and its bands no longer fit one launch group"""
    _, net = nets[(16, 2)]
    photos = [R.test_photo(64, 96, seed=70), R.test_photo(9, 33, seed=71)]
    whole, _ = net.upscale(photos=photos)
    limit = net.act_limit
    try:
        net.act_limit = (2 * 18 + 6) * 96 * 128             # 42 rows of the 64: bands of 6 rows with their halo of 18
        cut, info = net.upscale(photos=photos)
    finally:
        net.act_limit = limit
    assert info["banded"] == [True, False] and info["launches"] > 18 and torch.equal(cut, whole)


def test_device_photos_equal_the_numpy_source(nets):
    _, net = nets[(16, 2)]
    photos = _photos([(20, 31), (9, 40)], seed=90)
    a, ia = net.upscale(photos=photos)
    pad = 5                                                   # the photos need not start at byte 0 or lie back to back
    flat = np.concatenate([np.zeros(pad, np.uint8), photos[0].reshape(-1), np.zeros(3, np.uint8), photos[1].reshape(-1)])
    offs = [pad, pad + photos[0].size + 3]
    dst = torch.full((a.numel() + 64,), 99, dtype=torch.uint8, device=DEV)
    b, ib = net.upscale(device_photos=(torch.from_numpy(flat).to(DEV), offs, [(20, 31), (9, 40)]), out=dst, out_offsets=[64, 64 + ia["offsets"][1]])
    assert b is dst and torch.equal(b[64:], a) and (b[:64] == 99).all()


def test_x4_net_at_upscale_2_is_the_ragged_resize_of_its_own_output(nets):
    from vspbfr_amd.resample import ResamplePlan
    _, net = nets[(32, 4)]
    photos = _photos([(24, 36), (17, 40)], seed=95)
    out, info = net.upscale_to(2, photos=photos)
    assert info["shapes"] == [(48, 72), (34, 80)]
    big, ib = net.upscale(photos=photos)
    assert torch.equal(big, info["net_out"])
    plan = ResamplePlan(ib["shapes"], [(w, h) for h, w in info["shapes"]], [(0, 0)] * 2, None, device_sources=(big, ib["offsets"]),
                        out_sizes=info["shapes"])
    assert torch.equal(plan.run_into(torch.empty(plan.out_bytes, dtype=torch.uint8, device=DEV)), out)
    assert out.float().std() > 10


def test_background_then_paste_keeps_the_upscalers_bytes_outside_the_boxes(nets):
    import photo_ref as P0
    from vspbfr_amd import photo as P
    _, net = nets[(16, 2)]
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
    with pytest.raises(ValueError, match="cannot fill an upscale of 1"):
        P.FacePlan(photos, faces, size=64, upscale=1).background(DEV, upscaler=net)


def test_a_planted_f16_overflow_sets_the_flag_and_writes_finite_bytes():
    """one body weight scaled so that an activation exceeds 65 504: the f16 store gives inf, the tail sees a non-finite value, writes 0
    for it and flags the photo; the photo beside it in the group stays clean"""
    from vspbfr_amd import hip_ops as H, upscale as U
    sd = R.make_state(2, 2, seed=97)
    sd["body.2.weight"][5, 3, 1, 1] = 6.5e4
    net = U.SrUpscaler(sd, DEV)
    hot, calm = R.test_photo(9, 33, seed=98), np.zeros((5, 7, 3), np.uint8)
    assert R.net(sd, hot, torch.float32, upto=1).isinf().sum() >= 4 and R.net(sd, calm, torch.float32).isfinite().all()
    f32 = torch.zeros(3 * 4 * (9 * 33 + 35), dtype=torch.float32, device=DEV)
    out, info = net.upscale(photos=[hot, calm], out_f32=f32)
    flags = info["flags"].cpu().tolist()
    bad = ~torch.isfinite(f32)
    assert flags == [H.SR_NONFINITE, 0] and bad.any() and (out[bad] == 0).all() and not bad[info["offsets"][1]:].any()
    assert torch.equal(out[info["offsets"][1]:], net.upscale(photos=[calm])[0])
    print(f"non-finite outputs: {int(bad.sum())} of {bad.numel()}, flags {flags}")
