"""GPU checks of the FID kernels (csrc/fid.hip through vspbfr_amd/hip_ops.py and vspbfr_amd/fid.py) against tests/fid_ref.py.

Every bound is 4 e_ref + 2e-6 max |ref64| with e_ref = max |restatement float32 - restatement float64| of the same case, computed here.
The network has no discrete decision (ReLU and max are continuous), so no element is left out anywhere.  Every comparison prints its
e_ref / e_hip / ratio under -s.  The convolution's tile is 64 flat pixels x 64 channels with a K chunk of 16: the cases sit below, on and
above each of them, and every buffer carries sentinels behind the output and in the neighbouring channel slices."""
import numpy as np
import pytest
import torch
import torch.nn.functional as F

import fid_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 1024                                                  # sentinel floats behind every output buffer
SENTINEL = -777.25

# (kh, kw, ph, pw): the seven filters with the paddings the network uses
FILTERS = [(1, 1, 0, 0), (3, 3, 1, 1), (5, 5, 2, 2), (1, 7, 0, 3), (7, 1, 3, 0), (1, 3, 0, 1), (3, 1, 1, 0)]
CHANNELS = [(16, 16), (32, 48), (80, 192), (48, 64), (160, 192), (448, 384)]
MAPS = [(1, 1), (1, 9), (3, 5), (9, 7), (17, 17), (8, 8)]
# every filter on every map, the channel pairs rotating so that every filter meets every pair; c_off alternates
CONV_CASES = [(f, CHANNELS[(i + j) % 6], m, 1, 48 * ((i + j) % 2)) for i, f in enumerate(FILTERS) for j, m in enumerate(MAPS)]
# stride 2 for 3x3 without padding; a padding that is not the filter's own
CONV_CASES += [((3, 3, 0, 0), ch, m, 2, off) for ch, m, off in (((32, 48), (7, 7), 0), ((80, 192), (8, 8), 48), ((48, 64), (35, 35), 48))]
CONV_CASES += [((3, 3, 0, 1), (32, 48), (9, 7), 1, 0), ((5, 5, 1, 2), (16, 16), (3, 5), 2, 48), ((1, 1, 0, 0), (48, 64), (9, 7), 2, 0)]


def _report(name, e_ref, e_hip):
    print(f"{name}: e_ref {e_ref:.3g} e_hip {e_hip:.3g} ratio {e_hip / max(e_ref, 1e-30):.3g}")


def _check(name, got, ref64, ref32):
    e_ref = float((ref32.double() - ref64).abs().max())
    e_hip = float((got.double().cpu() - ref64).abs().max())
    _report(name, e_ref, e_hip)
    assert torch.isfinite(got).all()
    assert e_hip <= R.bound(e_ref, ref64), (name, e_hip, e_ref)


def _slice_out(B, oh, ow, cout, c_off):
    """an output buffer full of sentinels: (buffer, pitch)"""
    pitch = max(112, c_off + cout + 16)
    return torch.full((B * oh * ow * pitch + GUARD,), SENTINEL, dtype=torch.float32, device=DEV), pitch


def _untouched(buf, B, oh, ow, cout, c_off, pitch):
    """every element outside the slice still holds the sentinel"""
    body = buf[:B * oh * ow * pitch].view(-1, pitch)
    assert (body[:, :c_off] == SENTINEL).all() and (body[:, c_off + cout:] == SENTINEL).all() and (buf[B * oh * ow * pitch:] == SENTINEL).all()
    return body[:, c_off:c_off + cout].reshape(B, oh, ow, cout)


def _padded_in(x_nchw, pad=16):
    """(B, C, H, W) float32 -> NHWC device buffer with `pad` NaN channels behind the C real ones: (buffer, pitch)"""
    B, C, H, W = x_nchw.shape
    buf = torch.full((B, H, W, C + pad), float("nan"), dtype=torch.float32)
    buf[..., :C] = x_nchw.permute(0, 2, 3, 1)
    return buf.reshape(-1).to(DEV), C + pad


@pytest.mark.parametrize("case", CONV_CASES, ids=lambda c: "k%dx%d_p%d%d_c%d_%d_m%dx%d_s%d_o%d" % (c[0] + c[1] + c[2] + (c[3], c[4])))
def test_conv_alone(case):
    from vspbfr_amd import fid as Fd
    from vspbfr_amd import hip_ops as H
    (kh, kw, ph, pw), (cin, cout), (h, w), stride, c_off = case
    B = 3
    g = torch.Generator().manual_seed(1000 + 7 * kh + 3 * kw + cin + h * w + stride)
    x = torch.randn((B, cin, h, w), generator=g)
    wt = torch.randn((cout, cin, kh, kw), generator=g) * (2.0 / (cin * kh * kw)) ** 0.5
    bias = 0.1 * torch.randn(cout, generator=g)
    ref64 = F.relu(F.conv2d(x.double(), wt.double(), bias.double(), stride=stride, padding=(ph, pw))).permute(0, 2, 3, 1)
    ref32 = F.relu(F.conv2d(x, wt, bias, stride=stride, padding=(ph, pw))).permute(0, 2, 3, 1)
    oh, ow = ref64.shape[1:3]
    assert (oh, ow) == H.fid_conv_out(h, w, kh, kw, ph, pw, stride)
    xin, x_pitch = _padded_in(x)
    wd, bd = Fd.pack_weight(wt).to(DEV), bias.to(DEV)
    out, pitch = _slice_out(B, oh, ow, cout, c_off)
    H.fid_conv_f32((out, c_off, pitch), (xin, 0, x_pitch), wd, bd, B, h, w, stride, (ph, pw))
    got = _untouched(out, B, oh, ow, cout, c_off, pitch)
    _check("conv", got, ref64, ref32)
    # three images in one launch equal each alone, bit for bit
    for i in range(B):
        one, _ = _slice_out(1, oh, ow, cout, c_off)
        H.fid_conv_f32((one, c_off, pitch), (xin[i * h * w * x_pitch:(i + 1) * h * w * x_pitch], 0, x_pitch), wd, bd, 1, h, w, stride, (ph, pw))
        assert torch.equal(_untouched(one, 1, oh, ow, cout, c_off, pitch)[0], got[i])


def test_conv_reads_a_slice_of_its_input():
    """the input pointer may be a channel offset into a wider tensor (the second of two 1x1 results that share a buffer)"""
    from vspbfr_amd import fid as Fd
    from vspbfr_amd import hip_ops as H
    g = torch.Generator().manual_seed(5)
    B, h, w = 2, 9, 7
    x = torch.randn((B, 112, h, w), generator=g)
    wt = torch.randn((96, 64, 3, 3), generator=g) * (2.0 / 576) ** 0.5
    bias = 0.1 * torch.randn(96, generator=g)
    ref64 = F.relu(F.conv2d(x[:, 48:].double(), wt.double(), bias.double(), padding=1)).permute(0, 2, 3, 1)
    ref32 = F.relu(F.conv2d(x[:, 48:], wt, bias, padding=1)).permute(0, 2, 3, 1)
    xin = x.permute(0, 2, 3, 1).contiguous().reshape(-1).to(DEV)
    out, pitch = _slice_out(B, h, w, 96, 0)
    H.fid_conv_f32((out, 0, pitch), (xin, 48, 112), Fd.pack_weight(wt).to(DEV), bias.to(DEV), B, h, w, 1, (1, 1))
    _check("conv input slice", _untouched(out, B, h, w, 96, 0, pitch), ref64, ref32)


def _pool_ref(x, mode):
    from vspbfr_amd import hip_ops as H
    if mode == H.FID_POOL_MAX_S2:
        return F.max_pool2d(x, 3, 2)
    if mode == H.FID_POOL_AVG_S1:
        return F.avg_pool2d(x, 3, 1, 1, count_include_pad=False)
    return F.max_pool2d(x, 3, 1, 1)


@pytest.mark.parametrize("mode", [0, 1, 2])
@pytest.mark.parametrize("hw", [(3, 3), (7, 8), (35, 35)])
def test_pool_into_a_slice(mode, hw):
    from vspbfr_amd import hip_ops as H
    h, w = hw
    B, C, c_off = 3, 32, 48
    g = torch.Generator().manual_seed(31 * mode + h)
    x = torch.randn((B, C, h, w), generator=g)
    ref64, ref32 = _pool_ref(x.double(), mode).permute(0, 2, 3, 1), _pool_ref(x, mode).permute(0, 2, 3, 1)
    oh, ow = ref64.shape[1:3]
    assert (oh, ow) == H.fid_pool_out(h, w, mode)
    xin, x_pitch = _padded_in(x)
    out, pitch = _slice_out(B, oh, ow, C, c_off)
    H.fid_pool_f32((out, c_off, pitch), (xin, 0, x_pitch), B, h, w, C, mode)
    got = _untouched(out, B, oh, ow, C, c_off, pitch)
    if mode == H.FID_POOL_AVG_S1:
        _check("avg pool", got, ref64, ref32)
    else:
        assert torch.equal(got.cpu(), ref32)                  # a max rounds nothing
    for i in range(B):
        one, _ = _slice_out(1, oh, ow, C, c_off)
        H.fid_pool_f32((one, c_off, pitch), (xin[i * h * w * x_pitch:(i + 1) * h * w * x_pitch], 0, x_pitch), 1, h, w, C, mode)
        assert torch.equal(_untouched(one, 1, oh, ow, C, c_off, pitch)[0], got[i])


def test_avg_pool_divides_by_the_in_bounds_taps():
    """a map of ones stays ones: the corners divide by 4, the edges by 6, the interior by 9; a 1 x 1 map divides by 1"""
    from vspbfr_amd import hip_ops as H
    for h, w in ((1, 1), (1, 4), (5, 6)):
        x = torch.ones(h * w * 16, dtype=torch.float32, device=DEV)
        out = torch.zeros(h * w * 16, dtype=torch.float32, device=DEV)
        H.fid_pool_f32((out, 0, 16), (x, 0, 16), 1, h, w, 16, H.FID_POOL_AVG_S1)
        assert (out == 1.0).all()
    # and with a ramp the sums are those of the valid taps only
    x = torch.arange(9, dtype=torch.float32).view(1, 1, 3, 3).expand(1, 16, 3, 3)
    out = torch.zeros(9 * 16, dtype=torch.float32, device=DEV)
    H.fid_pool_f32((out, 0, 16), (x.permute(0, 2, 3, 1).contiguous().reshape(-1).to(DEV), 0, 16), 1, 3, 3, 16, H.FID_POOL_AVG_S1)
    want = torch.tensor([[8 / 4, 15 / 6, 12 / 4], [21 / 6, 36 / 9, 27 / 6], [20 / 4, 33 / 6, 24 / 4]], dtype=torch.float64)
    assert (out.view(3, 3, 16)[..., 5].double().cpu() - want).abs().max() <= 1e-6


@pytest.mark.parametrize("hw,C", [((1, 1), 64), ((2, 2), 64), ((8, 8), 2048)])
def test_global_average(hw, C):
    from vspbfr_amd import hip_ops as H
    h, w = hw
    B = 3
    g = torch.Generator().manual_seed(h + C)
    x = torch.randn((B, C, h, w), generator=g)
    ref64, ref32 = x.double().mean(dim=(2, 3)), x.mean(dim=(2, 3))
    xin, x_pitch = _padded_in(x)
    out = torch.full((B * C + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    H.fid_pool_f32((out, 0, C), (xin, 0, x_pitch), B, h, w, C, H.FID_POOL_GLOBAL_AVG)
    assert (out[B * C:] == SENTINEL).all()
    got = out[:B * C].view(B, C)
    _check("global average", got, ref64, ref32)
    one = torch.empty(C, dtype=torch.float32, device=DEV)
    H.fid_pool_f32((one, 0, C), (xin[h * w * x_pitch:2 * h * w * x_pitch], 0, x_pitch), 1, h, w, C, H.FID_POOL_GLOBAL_AVG)
    assert torch.equal(one, got[1])


@pytest.fixture(scope="module")
def net():
    from vspbfr_amd import fid as Fd
    return Fd.FidInception(Fd.check_state_dict(R.shared_state()), DEV)


def test_stem_ragged_at_odd_byte_offsets(net):
    """u8 images of 75 x 75, 64 x 97 and 512 x 512 in one call, at byte offsets 1 and 3 (mod 4), through the resize"""
    from vspbfr_amd import _lib
    from vspbfr_amd import hip_ops as H
    g = torch.Generator().manual_seed(77)
    imgs = [torch.randint(0, 256, s + (3,), generator=g, dtype=torch.uint8) for s in ((75, 75), (64, 97), (512, 512))]
    parts, offs, at = [], [], 1
    parts.append(torch.zeros(1, dtype=torch.uint8))
    for k, im in enumerate(imgs):
        offs.append(at)
        parts.append(im.reshape(-1))
        at += im.numel()
        fill = (3 - at) % 4 if k == 0 else 2
        parts.append(torch.zeros(fill, dtype=torch.uint8))
        at += fill
    assert offs[0] % 4 == 1 and offs[1] % 4 == 3
    src = torch.cat(parts).to(DEV)
    items = (_lib.DetSrc * 3)()
    for i, im in enumerate(imgs):
        items[i].off, items[i].h, items[i].w, items[i].slot = offs[i], im.shape[0], im.shape[1], i
    items_dev = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(DEV)
    w, b = net.weights["Conv2d_1a_3x3"]
    y = torch.full((3 * 149 * 149 * 32 + GUARD,), SENTINEL, dtype=torch.float32, device=DEV)
    H.fid_stem_u8(y[:3 * 149 * 149 * 32], src, items, items_dev, 3, 3, 299, 299, w, b)
    assert (y[3 * 149 * 149 * 32:] == SENTINEL).all()
    got = y[:3 * 149 * 149 * 32].view(3, 149, 149, 32)
    sd = R.shared_state()
    t64, t32 = R.build(sd, torch.float64), R.build(sd, torch.float32, folded=True)
    with torch.no_grad():
        for i, im in enumerate(imgs):
            refs = []
            for tree, dt in ((t64, torch.float64), (t32, torch.float32)):
                x = R.resize_bilinear(im[None].permute(0, 3, 1, 2).to(dt), 299) / 127.5 - 1
                refs.append(tree.Conv2d_1a_3x3(x).permute(0, 2, 3, 1)[0])
            _check(f"stem {tuple(im.shape[:2])}", got[i], refs[0], refs[1])


@pytest.mark.parametrize("name", ["n75", "n107", "full"])
def test_whole_network(net, name):
    imgs = R.case_images(name)
    ref64, ref32 = R.case_reference(name)
    got = net.features(imgs.to(DEV), resize=R.CASES[name]["resize"])
    assert got.shape == (imgs.shape[0], 2048) and got.dtype == torch.float32
    _check("network " + name, got, ref64, ref32)


def test_chunks_of_one_equal_one_call_and_a_second_stream(net):
    imgs = R.case_images("n75").to(DEV)
    whole = net.features(imgs, resize=False)
    assert torch.equal(net.features(imgs, resize=False, chunk=1), whole)
    assert torch.equal(net.features(imgs[1:2], resize=False), whole[1:2])
    s = torch.cuda.Stream()
    s.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(s):
        other = net.features(imgs, resize=False)
    s.synchronize()
    assert torch.equal(other, whole)
    # a list of images and a packed buffer serve like the tensor
    lst = net.features([im.cpu().numpy() for im in imgs], resize=False)
    n = 75 * 75 * 3
    packed = net.features(device_photos=(imgs.reshape(-1), [0, n, 2 * n], [(75, 75)] * 3), resize=False)
    assert torch.equal(lst, whole) and torch.equal(packed, whole)


def test_statistics_of_the_device_features(net):
    """stats of the device's features against the float64 features' statistics, the feature bound propagated linearly: with |df| <= b,
    |d mu| <= b and |d cov_ij| <= 2 b / (N - 1) sum_n (|d_ni| + |d_nj|) + 4 b^2 N / (N - 1), d the centred float64 features"""
    from vspbfr_amd import fid as Fd
    ref64, ref32 = R.case_reference("n75")
    got = net.features(R.case_images("n75").to(DEV), resize=False)
    b = R.bound(float((ref32.double() - ref64).abs().max()), ref64)
    mu, sigma = Fd.stats(got)
    mu64, sigma64 = R.stats_ref(ref64.numpy())
    N = ref64.shape[0]
    d = np.abs(ref64.numpy() - mu64).sum(0)
    lim = 2 * b / (N - 1) * (d[:, None] + d[None, :]) + 4 * b * b * N / (N - 1) + 1e-15
    _report("stats mu", b, float(np.abs(mu - mu64).max()))
    _report("stats sigma", float(lim.max()), float(np.abs(sigma - sigma64).max()))
    assert np.abs(mu - mu64).max() <= b
    assert (np.abs(sigma - sigma64) <= lim).all()
