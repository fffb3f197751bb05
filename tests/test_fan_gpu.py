"""GPU: the landmark network's kernels (csrc/fan.hip) against the float64 restatement of tests/fan_ref.py.

    max|HIP - float64| <= 4 e_ref + 2e-6 max|float64| (+ 1/2 f16 ulp, taken element by element at each value, where the output is f16),
    e_ref = max|float32 CPU restatement - float64| on the same rounded operands, both before the final rounding to f16

-- the project's bound; nothing in it comes from the kernels.  Every comparison prints e_ref, the HIP error and their ratio (`pytest -s`).
There is no argmax margin rule on network outputs: heatmaps are compared within the bound, and the decode kernel is compared exactly
with the NumPy decode of the same heatmap bits, the device's own included.  The bits of an image at another batch size or position,
the pool and the decode are compared exactly.  B = 2 throughout; 13 x 17 and 5 x 7 maps put tile tails and the boundary between the two
images inside a 128-pixel tile."""
import numpy as np
import pytest
import torch

import fan_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
NM, DP, SIDE = 2, 2, 64


def close(got, r64, r32, what, f16=False):
    got, r64, r32 = (np.asarray(t.detach().cpu() if isinstance(t, torch.Tensor) else t, dtype=np.float64) for t in (got, r64, r32))
    assert got.shape == r64.shape, (what, got.shape, r64.shape)
    eref, top = float(np.abs(r32 - r64).max()), float(np.abs(r64).max())
    tol = 4.0 * eref + 2e-6 * top
    d = np.abs(got - r64) - (R.f16_half_ulp(r64) if f16 else 0.0)        # what is left beyond each value's own rounding
    err = float(d.max())
    print(f"FAN {what}: e_ref={eref:.3e} e_hip={float(np.abs(got - r64).max()):.3e} beyond rounding={err:.3e} "
          f"ratio={err / eref if eref else float('nan'):.2f} tol={tol:.3e}")
    assert np.isfinite(got).all() and err <= tol, f"{what}: {err:.3e} beyond the rounding, tol={tol:.3e} (e_ref {eref:.3e})"


def rand16(gen, *shape, scale=1.0):
    """f16 values as float32: the same operands everywhere"""
    return torch.randn(*shape, generator=gen, dtype=torch.float64).mul_(scale).float().half().float()


def rand32(gen, *shape, scale=1.0):
    return torch.randn(*shape, generator=gen, dtype=torch.float64).mul_(scale).float()


def nhwc(x, pitch=None, off=0, fill=0.0, dtype=torch.float16):
    """(B, C, H, W) -> the flat device buffer (B, H, W, pitch) with x in channels off .. off + C - 1"""
    B, C_, H, W = x.shape
    t = torch.full((B, H, W, pitch or C_), fill, dtype=dtype)
    t[..., off:off + C_] = x.permute(0, 2, 3, 1).to(dtype)
    return t.reshape(-1).to(DEV)


def nchw(buf, B, H, W, pitch, off=0, C_=None):
    v = buf.cpu().float().reshape(B, H, W, pitch)[..., off:off + (C_ or pitch - off)]
    return v.permute(0, 3, 1, 2).contiguous()


def operands(k, cin, cout, hw, seed, affine=True, bias=False, b_positive=False, B=2):
    g = torch.Generator().manual_seed(seed)
    o = {"x": rand16(g, B, cin, *hw), "w": rand16(g, cout, cin, k, k, scale=(k * k * cin) ** -0.5), "b": rand32(g, cout, scale=0.1) if bias else None,
         "aff": None, "g": g}
    if affine:
        a, s = 0.75 + 0.5 * torch.rand(cin, generator=g, dtype=torch.float64).float(), rand32(g, cin, scale=0.3)
        o["aff"] = (a, s.abs() + 0.5 if b_positive else s)
    return o


def run(o, hw, cout, relu=False, res1=None, res2=None, up=None, out_f32=False, raw=False, B=2, cin_pad=None):
    """one launch on dense buffers -> (y, raw or None) as (B, C, H, W) float32"""
    from vspbfr_amd import fan, hip_ops as H
    x, w = o["x"], o["w"]
    cin = cin_pad or x.shape[1]
    n = B * hw[0] * hw[1]
    y = torch.full((n * cout,), float("nan"), device=DEV, dtype=torch.float32 if out_f32 else torch.float16)
    rw = torch.full((n * cout,), float("nan"), device=DEV, dtype=torch.float16) if raw else None
    win = lambda t: None if t is None else (nhwc(t), t.shape[1], 0)
    H.fan_conv_f16((y, cout, 0), (nhwc(x, cin), cin, 0), B, hw[0], hw[1], fan.pack_conv_weight(fan.pad_cin(w, cin)).half().to(DEV), cout,
                   b=None if o["b"] is None else o["b"].to(DEV), affine=None if o["aff"] is None else tuple(t.to(DEV) for t in o["aff"]),
                   relu=relu, raw=None if rw is None else (rw, cout, 0), res1=win(res1), res2=win(res2), up=win(up), out_f32=out_f32)
    return nchw(y, B, *hw, cout), None if rw is None else nchw(rw, B, *hw, cout)


def refs(o, relu=False, **tail):
    """(v, y) in float64 and float32, before the roundings"""
    out = []
    for dt in (torch.float64, torch.float32):
        v = R.conv_ref(o["x"], o["w"], dt, o["b"], o["aff"], relu)
        out.append((v, R.tail_ref(v, dt, **tail)))
    return out


# ----------------------------------------------------------------------------------------------------------------------------- stem
@pytest.mark.parametrize("hw,boxes", [((37, 53), [[-6.5, 4.25, 40.0], [10.0, 3.0, 31.5]]), ((64, 64), [[0.0, 0.0, 64.0]] * 2)],
                         ids=["37x53 box partly outside", "64x64 whole image"])
def test_stem_samples_the_box(hw, boxes):
    from vspbfr_amd import fan, hip_ops as H
    g = torch.Generator().manual_seed(21)
    photos = np.stack([R.test_photo(*hw, 1), R.test_photo(*hw, 2)])
    w, b = rand32(g, 64, 3, 7, 7, scale=147 ** -0.5), rand32(g, 64, scale=0.1)
    box = np.asarray(boxes, np.float32)
    y = torch.full((2 * 16 * 16 * 64,), float("nan"), device=DEV, dtype=torch.float16)
    H.fan_stem_u8(y, torch.from_numpy(photos).to(DEV), torch.from_numpy(box).to(DEV), fan.pack_stem(w).to(DEV), b.to(DEV), 32)
    close(nchw(y, 2, 16, 16, 64), R.stem_ref(photos, box, 32, w, b, torch.float64), R.stem_ref(photos, box, 32, w, b, torch.float32),
          f"stem {hw} side 32", f16=True)


# ---------------------------------------------------------------------------------------------------------------------- convolution
CONV_CASES = [  # name, k, cin, cout, (H, W), kwargs of operands, relu
    ("3x3 256->128 affine", 3, 256, 128, (13, 17), {}, False),
    ("3x3 128->64 affine", 3, 128, 64, (13, 17), {}, False),
    ("3x3 64->64 affine", 3, 64, 64, (13, 17), {}, False),
    ("3x3 64->32 affine", 3, 64, 32, (5, 7), {}, False),
    ("3x3 32->32 affine", 3, 32, 32, (13, 17), {}, False),
    ("3x3 128->64 no affine", 3, 128, 64, (5, 7), {"affine": False}, False),
    ("3x3 64->64 affine, every b_c > 0", 3, 64, 64, (5, 7), {"b_positive": True}, False),
    ("1x1 64->128 affine no bias", 1, 64, 128, (13, 17), {}, False),
    ("1x1 128->256 affine no bias", 1, 128, 256, (5, 7), {}, False),
    ("1x1 256->256 bias relu", 1, 256, 256, (13, 17), {"affine": False, "bias": True}, True),
    ("3x3 256->128 affine 2x2 map", 3, 256, 128, (2, 2), {}, False),
    ("3x3 64->32 affine 4x4 map", 3, 64, 32, (4, 4), {}, False),
    ("1x1 256->256 bias 4x4 map", 1, 256, 256, (4, 4), {"affine": False, "bias": True}, False),
]


@pytest.mark.parametrize("name,k,cin,cout,hw,kw,relu", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_convolution(name, k, cin, cout, hw, kw, relu):
    o = operands(k, cin, cout, hw, cin + cout + k + hw[0], **kw)
    if kw.get("b_positive"):
        assert bool((o["aff"][1] > 0).all())       # relu(b_c) > 0 in every channel: padding in front of the affine would show
    y, _ = run(o, hw, cout, relu=relu)
    (v64, _), (v32, _) = refs(o, relu)
    close(y, v64, v32, f"conv {name} {hw}", f16=True)


def test_heatmap_head_fp32_and_f16():
    """1x1 256 -> 68 with bias: the fp32 output and the f16 raw copy of one launch, and the f16 output of another; no padded channel
    is stored (the buffers have a pitch of 68)"""
    o = operands(1, 256, 68, (13, 17), 5, affine=False, bias=True)
    (v64, _), (v32, _) = refs(o)
    y, raw = run(o, (13, 17), 68, out_f32=True, raw=True)
    close(y, v64, v32, "conv 1x1 256->68 fp32")
    close(raw, v64, v32, "conv 1x1 256->68 raw f16", f16=True)
    assert torch.equal(raw, y.half().float())                      # the same fp32 sum, rounded once
    y16, _ = run(o, (13, 17), 68)
    assert torch.equal(y16, raw)


def test_two_residuals_behind_the_68_channel_input():
    """1x1 68 -> 256: the input is a 96-channel window whose last 28 are zero; previous + bl(ll) + al(t) is ((v + res1) + res2)"""
    o = operands(1, 68, 256, (13, 17), 6, affine=False, bias=True)
    r1, r2 = rand16(o["g"], 2, 256, 13, 17, scale=4.0), rand16(o["g"], 2, 256, 13, 17)
    y, _ = run(o, (13, 17), 256, res1=r1, res2=r2, cin_pad=96)
    (_, y64), (_, y32) = refs(o, res1=r1, res2=r2)
    close(y, y64, y32, "conv 1x1 68->256 two residuals", f16=True)


def test_dual_store_and_the_coarser_level():
    """raw = f16(acc) and y = f16(acc + residual [+ coarser level]) from one fp32 sum; 8 x 10 with a 4 x 5 level"""
    o = operands(3, 256, 128, (13, 17), 7)
    res = rand16(o["g"], 2, 128, 13, 17, scale=3.0)
    y, raw = run(o, (13, 17), 128, res1=res, raw=True)
    (v64, y64), (v32, y32) = refs(o, res1=res)
    close(raw, v64, v32, "dual store: raw", f16=True)
    close(y, y64, y32, "dual store: output", f16=True)
    o = operands(3, 64, 64, (8, 10), 8)
    res, up = rand16(o["g"], 2, 64, 8, 10), rand16(o["g"], 2, 64, 4, 5, scale=2.0)
    y, raw = run(o, (8, 10), 64, res1=res, up=up, raw=True)
    (v64, y64), (v32, y32) = refs(o, res1=res, up=up)
    close(raw, v64, v32, "coarser level: raw", f16=True)
    close(y, y64, y32, "coarser level 8x10 + 4x5", f16=True)
    with pytest.raises(RuntimeError, match="even map"):
        odd = operands(3, 64, 64, (5, 7), 9)
        run(odd, (5, 7), 64, up=rand16(odd["g"], 2, 64, 2, 3))


def test_convolution_writes_only_its_channel_window_and_reads_one():
    """3x3 256 -> 64 into channels 128 .. 191 of a 256-pitch tensor prefilled with a sentinel, from channels 64 .. 319 of a NaN-filled
    320-pitch one"""
    from vspbfr_amd import fan, hip_ops as H
    o = operands(3, 256, 64, (13, 17), 77)
    wi, aff = fan.pack_conv_weight(o["w"]).half().to(DEV), tuple(t.to(DEV) for t in o["aff"])
    y = torch.full((2 * 13 * 17 * 256,), 7.0, device=DEV, dtype=torch.float16)
    H.fan_conv_f16((y, 256, 128), (nhwc(o["x"], 320, 64, fill=float("nan")), 320, 64), 2, 13, 17, wi, 64, affine=aff)
    full = nchw(y, 2, 13, 17, 256)
    assert bool((full[:, :128] == 7.0).all()) and bool((full[:, 192:] == 7.0).all())
    (v64, _), (v32, _) = refs(o)
    close(full[:, 128:192], v64, v32, "conv 3x3 256->64 window", f16=True)
    dense, _ = run(o, (13, 17), 64)
    assert torch.equal(dense, full[:, 128:192])


def test_residual_in_place_and_batch_independence():
    """the output may be the residual's own window (same bits as apart), and image 1 alone has the bits it has behind image 0"""
    from vspbfr_amd import fan, hip_ops as H
    o = operands(3, 256, 128, (13, 17), 99)
    res = rand16(o["g"], 2, 256, 13, 17)
    wi, aff = fan.pack_conv_weight(o["w"]).half().to(DEV), tuple(t.to(DEV) for t in o["aff"])
    xb, rb = nhwc(o["x"]), nhwc(res)
    apart = torch.zeros(2 * 13 * 17 * 256, device=DEV, dtype=torch.float16)
    H.fan_conv_f16((apart, 256, 128), (xb, 256, 0), 2, 13, 17, wi, 128, affine=aff, res1=(rb, 256, 128))
    inplace = rb.clone()
    H.fan_conv_f16((inplace, 256, 128), (xb, 256, 0), 2, 13, 17, wi, 128, affine=aff, res1=(inplace, 256, 128))
    a, b = nchw(apart, 2, 13, 17, 256), nchw(inplace, 2, 13, 17, 256)
    assert torch.equal(a[:, 128:], b[:, 128:]) and torch.equal(b[:, :128], res[:, :128])
    (_, y64), (_, y32) = refs(o, res1=res[:, 128:])
    close(b[:, 128:], y64, y32, "conv in place", f16=True)
    with pytest.raises(RuntimeError, match="without being its window"):
        H.fan_conv_f16((inplace, 256, 128), (xb, 256, 0), 2, 13, 17, wi, 128, affine=aff, res1=(inplace, 256, 0))
    one = torch.zeros(13 * 17 * 256, device=DEV, dtype=torch.float16)
    H.fan_conv_f16((one, 256, 128), (nhwc(o["x"][1:]), 256, 0), 1, 13, 17, wi, 128, affine=aff, res1=(nhwc(res[1:]), 256, 128))
    assert torch.equal(one, apart[13 * 17 * 256:])
    # and on a 2 x 2 map, where one 16-pixel block of a wave holds both images
    s = operands(3, 256, 128, (2, 2), 100)
    both, _ = run(s, (2, 2), 128)
    s["x"] = s["x"][1:]
    alone, _ = run(s, (2, 2), 128, B=1)
    assert torch.equal(alone[0], both[1])


DEPTH_CASES = [("3x3 32->32 affine", 3, 32, 32, {}, False), ("3x3 32->64 affine residual raw", 3, 32, 64, {}, True),
               ("1x1 64->64 bias", 1, 64, 64, {"affine": False, "bias": True}, False),
               # more than one step of 32 channels per tap: the advance of the pixel, weight and coefficient fetches inside a tap
               ("3x3 64->64 affine", 3, 64, 64, {}, False), ("3x3 128->64 affine residual raw", 3, 128, 64, {}, True),
               ("3x3 96->32 no affine", 3, 96, 32, {"affine": False}, False), ("1x1 128->64 affine", 1, 128, 64, {}, False)]


@pytest.mark.parametrize("name,k,cin,cout,kw,dual", DEPTH_CASES, ids=[c[0] for c in DEPTH_CASES])
def test_both_pipeline_depths(name, k, cin, cout, kw, dual):
    """A launch of more than 512 workgroups fetches one step ahead, a smaller one runs the ring of three stages: two images of 182 x 182 are
    518 tiles of 128 pixels, image 1 alone 259.  Both are within the bound, and image 1 has the same bits on either route."""
    hw = (182, 182)
    o = operands(k, cin, cout, hw, 300 + cin + cout, **kw)
    res = rand16(o["g"], 2, cout, *hw) if dual else None
    y, raw = run(o, hw, cout, res1=res, raw=dual)
    (v64, y64), (v32, y32) = refs(o, res1=res)
    close(y, y64, y32, f"conv {name} {hw}, one step ahead", f16=True)
    if dual:
        close(raw, v64, v32, f"conv {name} {hw}, one step ahead: raw", f16=True)
    o["x"] = o["x"][1:]
    y1, raw1 = run(o, hw, cout, res1=None if res is None else res[1:], raw=dual, B=1)
    assert torch.equal(y1[0], y[1]) and (not dual or torch.equal(raw1[0], raw[1]))


# ----------------------------------------------------------------------------------------------------------------------------- pool
def test_pool_is_bit_exact():
    from vspbfr_amd import hip_ops as H
    g = torch.Generator().manual_seed(31)
    x = (rand16(g, 2, 128, 8, 10) * torch.exp2(torch.randint(-12, 12, (2, 128, 8, 10), generator=g).float())).half().float()
    y = torch.full((2 * 4 * 5 * 128,), float("nan"), device=DEV, dtype=torch.float16)
    H.fan_pool_f16((y, 128, 0), (nhwc(x), 128, 0), 2, 8, 10, 128)
    assert torch.equal(nchw(y, 2, 4, 5, 128), R.pool_ref(x))
    # between windows: channels 64 .. 127 of a 192-pitch input into channels 8 .. 71 of a 96-pitch output
    y = torch.full((2 * 4 * 5 * 96,), 7.0, device=DEV, dtype=torch.float16)
    H.fan_pool_f16((y, 96, 8), (nhwc(x[:, :64], 192, 64, fill=float("nan")), 192, 64), 2, 8, 10, 64)
    full = nchw(y, 2, 4, 5, 96)
    assert torch.equal(full[:, 8:72], R.pool_ref(x[:, :64])) and bool((full[:, :8] == 7.0).all()) and bool((full[:, 72:] == 7.0).all())
    with pytest.raises(RuntimeError, match="odd map"):
        H.fan_pool_f16((y, 96, 8), (nhwc(x[:, :64, :7]), 64, 0), 2, 7, 10, 64)


# --------------------------------------------------------------------------------------------------------------------------- decode
def _decode(heat, box):
    """heat (B, K, n, n) float32 -> the kernel's (lm, peak, per-image flag) as NumPy"""
    from vspbfr_amd import hip_ops as H
    B, K, n, _ = heat.shape
    lm, peak, flag = H.fan_decode(nhwc(torch.as_tensor(heat), dtype=torch.float32), K, torch.as_tensor(box).to(DEV), B, n, K)
    torch.cuda.synchronize()
    return lm.cpu().numpy(), peak.cpu().numpy(), flag.ne(0).any(dim=1).cpu().numpy()


def test_decode_on_crafted_maps():
    n = 8
    heat = np.zeros((2, 68, n, n), np.float32)
    box = np.array([[10.0, 20.0, 64.0], [-3.5, 0.25, 100.0]], np.float32)
    heat[0, 0, 3, 5] = heat[0, 0, 6, 2] = 2.0               # a tie: the lowest flat index
    heat[0, 1, 0, 4], heat[0, 1, 0, 5], heat[0, 1, 0, 3] = 3.0, 1.0, 0.5          # a border peak
    heat[0, 2, 4, 4], heat[0, 2, 4, 3], heat[0, 2, 4, 5], heat[0, 2, 3, 4], heat[0, 2, 5, 4] = 5.0, 1.0, 1.0, 2.0, 1.0   # a zero difference
    heat[0, 3, 7, 7] = 1.0
    heat[0, 4] = -1.0
    rng = np.random.default_rng(4)
    heat[0, 5:] = rng.integers(0, 4, (63, n, n)).astype(np.float32)               # many ties, every lane's part of the scan
    heat[1] = rng.normal(0, 1, (68, n, n)).astype(np.float32)
    heat[1, 7, 2, 2], heat[1, 9] = np.nan, np.inf                                 # flagged in image 1 alone, never the peak
    heat[1, 11, 5, 5] = -np.inf
    got, want = _decode(heat, box), R.decode_ref(heat, box)
    assert want[2].tolist() == [False, True] and want[0][0, 0].tolist() == [54.0, 48.0] and want[0][0, 1].tolist() == [48.0, 24.0]
    for a, b, name in zip(got, want, ("landmarks", "peaks", "flags")):
        assert np.array_equal(a, b), name
    # a 64 x 64 map with one wave: 64 cells per lane
    big = rng.normal(0, 1, (2, 68, 64, 64)).astype(np.float32)
    big[:, :, 0, 0] = big.max(axis=(2, 3)) + 1          # the first cell, on two borders
    big[:, 1::2, 0, 0] = -9
    for a, b in zip(_decode(big, box), R.decode_ref(big, box)):
        assert np.array_equal(a, b)


# -------------------------------------------------------------------------------------------------------------------- whole network
@pytest.fixture(scope="module")
def case():
    """the 2-module, depth-2 network at full widths on two 80 x 80 photos, side 64: 16 x 16 heatmaps, levels 16 / 8 / 4; the float64
    and float32 restatements are computed once"""
    from vspbfr_amd.fan import FanLandmarks
    sd = R.state_of(R.make_model(0, NM, DP))
    photos = np.stack([R.test_photo(80, 80, 1), R.test_photo(80, 80, 2)])
    boxes = np.array([[0, 0, 80], [5.5, -3, 70]], np.float32)
    red = R.reduce(sd, NM, DP)
    return {"net": FanLandmarks(sd, DEV, side=SIDE), "photos": photos, "boxes": boxes, "u8": torch.from_numpy(photos).to(DEV),
            "h64": R.forward(red, photos, boxes, SIDE, NM, DP, torch.float64), "h32": R.forward(red, photos, boxes, SIDE, NM, DP, torch.float32)}


def test_whole_network(case):
    from vspbfr_amd import fan
    net, u8, box = case["net"], case["u8"], torch.from_numpy(case["boxes"])
    heat = net.heatmaps(u8, box)
    assert tuple(heat.shape) == (2, 68, 16, 16) and heat.dtype == torch.float32
    close(heat, case["h64"], case["h32"], "network heatmaps")
    # image 0 alone has the bits it has inside the batch of 2 -- and so has a batch that the guard splits into single images
    assert torch.equal(net.heatmaps(u8[:1], box[:1])[0], heat[0])
    net.GUARD_BYTES = fan.image_bytes(SIDE) + 1
    try:
        split = net.heatmaps(u8, box)
    finally:
        del net.GUARD_BYTES
    assert torch.equal(split, heat)
    # landmarks(): the kernel's decode of the device's own heatmaps equals the NumPy decode of those bits
    lm, peak, bad = net.landmarks(u8, box)
    want = R.decode_ref(heat.cpu().numpy(), case["boxes"])
    assert np.array_equal(lm.cpu().numpy(), want[0]) and np.array_equal(peak.cpu().numpy(), want[1]) and bad.cpu().tolist() == [False, False]
    assert lm.dtype == torch.float32 and tuple(lm.shape) == (2, 68, 2)


def test_evaluator_columns(case):
    from vspbfr_amd import metrics as M
    net, x = case["net"], case["u8"]
    y = torch.from_numpy(np.stack([R.test_photo(80, 80, 5), R.test_photo(80, 80, 6)])).to(DEV)
    box = (2.0, 1.0, 76.0)
    ev = M.Evaluator(lmd=net, lmd_box=box)
    ev.add(x, x, [("a", "a"), ("b", "b")])
    ev.add(x, y, [("c", "c"), ("d", "d")])
    rep = ev.report("d")
    rows = rep["images"]
    assert rows[0]["lmd"] == 0.0 and rows[1]["lmd"] == 0.0
    lx, ly = (net.landmarks(t, box)[0].cpu().numpy() for t in (x, y))
    d, e = R.lmd_nme_ref(lx, ly)
    for k in range(2):
        print(f"FAN evaluator image {k}: lmd {rows[2 + k]['lmd']!r} (NumPy {d[k]!r}) nme {rows[2 + k]['nme']!r} (NumPy {e[k]!r})")
        assert d[k] > 0 and abs(rows[2 + k]["lmd"] - d[k]) <= 1e-12 * d[k]
        if np.isfinite(e[k]):
            assert abs(rows[2 + k]["nme"] - e[k]) <= 1e-12 * e[k]
        else:
            assert rows[2 + k]["nme"] is None
    want = [v for v in d if v is not None]
    assert rep["mean"]["lmd"] == pytest.approx(float(np.sum(want)) / 4, rel=1e-12) and "lmd" in M.summary_line(rep)
    plain = M.Evaluator()
    plain.add(x, x, [("a", "a"), ("b", "b")])
    plain.add(x, y, [("c", "c"), ("d", "d")])
    bare = plain.report("d")
    assert "lmd" not in bare["mean"] and all("lmd" not in r and "nme" not in r for r in bare["images"])
    assert [{k: v for k, v in r.items() if k not in ("lmd", "nme")} for r in rows] == bare["images"]
    assert {k: v for k, v in rep["mean"].items() if k not in ("lmd", "nme")} == bare["mean"]
    with pytest.raises(RuntimeError, match="NIQE only"):
        M.Evaluator(lmd=net).add(x, None)


def test_landmarks_and_add_do_not_make_the_host_wait(case):
    """torch's sync debug mode raises at every call of torch's that makes the host wait for the device -- a blocking copy from or to host
    memory, an item(), a stream or device synchronisation.  With one box for every image (the default, and a triple) landmarks() and
    Evaluator.add make none; the report's one copy does."""
    from vspbfr_amd import metrics as M
    net, x = case["net"], case["u8"]
    y = torch.from_numpy(np.stack([R.test_photo(80, 80, 5), R.test_photo(80, 80, 6)])).to(DEV)
    ev = M.Evaluator(lmd=net, lmd_box=(2.0, 1.0, 76.0))
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        a = net.landmarks(x)
        b = net.landmarks(x, (2.0, 1.0, 76.0))
        ev.add(x, y)
        with pytest.raises(RuntimeError, match="synchroniz"):          # the mode is live: a copy to the host is refused
            a[0].cpu()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert tuple(a[0].shape) == tuple(b[0].shape) == (2, 68, 2) and len(ev.report("d")["images"]) == 2
    # the filled boxes are the copied ones
    assert torch.equal(net.boxes(x, (2.0, 1.0, 76.0)), net.boxes(x, torch.tensor([[2.0, 1.0, 76.0]] * 2)))
