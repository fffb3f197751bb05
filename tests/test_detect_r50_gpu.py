"""GPU: the ResNet-50 detector's kernels (csrc/detect_r50.hip) against the float64 restatement of tests/detect_r50_ref.py.

    max|HIP - float64| <= 4 e_ref + 2e-6 max|float64| (+ 1/2 f16 ulp of max|float64| where the output is f16),
    e_ref = max|float32 CPU restatement - float64| on the same rounded operands, both before the final rounding to f16

-- the project's bound; nothing in it comes from the kernels.  For an f16 output it is also asserted element by element with the half
ulp taken at each value, which leaves the arithmetic's own error visible.  Every comparison prints e_ref, the HIP error and their ratio
(`pytest -s`).
Orders and sets (kept priors, status words) and the bits of an image at another batch size or position are compared exactly.  B = 2
throughout; 13 x 17 and 5 x 7 maps put tile tails, stride-2 tails and the boundary between the two images inside a 128-pixel tile."""
import numpy as np
import pytest
import torch

import detect_r50_cases as K
import detect_r50_ref as R5
import detect_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def close(got, r64, r32, what, f16=False, scale=1.0):
    got, r64, r32 = (np.asarray(t.detach().cpu() if isinstance(t, torch.Tensor) else t, dtype=np.float64) for t in (got, r64, r32))
    assert got.shape == r64.shape, (what, got.shape, r64.shape)
    eref, err, top = float(np.abs(r32 - r64).max()), float(np.abs(got - r64).max()), float(np.abs(r64).max())
    tol = (4.0 * eref + 2e-6 * top + (R5.f16_half_ulp(top) if f16 else 0.0)) * scale
    print(f"DET50 {what}: e_ref={eref:.3e} e_hip={err:.3e} ratio={err / eref if eref else float('nan'):.2f} tol={tol:.3e}")
    assert np.isfinite(got).all() and err <= tol, f"{what}: max|d|={err:.3e} tol={tol:.3e} (e_ref {eref:.3e})"
    if f16:
        # the same bound element by element, with the half ulp taken at each value instead of at the largest: what is left of an
        # element's error beyond its own rounding is the arithmetic's
        half = 2.0 ** (np.floor(np.log2(np.maximum(np.abs(r64), 2.0 ** -14))) - 11)
        beyond = float((np.abs(got - r64) - half).max())
        print(f"DET50 {what}: beyond each value's own half ulp: {beyond:.3e} (allowed {(4.0 * eref + 2e-6 * top) * scale:.3e})")
        assert beyond <= (4.0 * eref + 2e-6 * top) * scale, f"{what}: {beyond:.3e} beyond the rounding"


def rand16(gen, *shape, scale=1.0):
    """f16 values as float32: the same operands everywhere"""
    return torch.randn(*shape, generator=gen, dtype=torch.float64).mul_(scale).float().half().float()


def rand32(gen, *shape, scale=1.0):
    return torch.randn(*shape, generator=gen, dtype=torch.float64).mul_(scale).float()


def nhwc(x, pitch=None, off=0, fill=0.0):
    """(B, C, H, W) of f16 values -> the flat f16 device buffer (B, H, W, pitch) with x in channels off .. off + C - 1"""
    B, C_, H, W = x.shape
    t = torch.full((B, H, W, pitch or C_), fill, dtype=torch.float16)
    t[..., off:off + C_] = x.permute(0, 2, 3, 1).half()
    return t.reshape(-1).to(DEV)


def nchw(buf, B, H, W, pitch, off=0, C_=None):
    v = buf.cpu().float().reshape(B, H, W, pitch)[..., off:off + (C_ or pitch - off)]
    return v.permute(0, 3, 1, 2).contiguous()


@pytest.fixture(scope="module")
def detector():
    from vspbfr_amd.detect_r50 import RetinaFaceR50Detector
    return RetinaFaceR50Detector(K.state(), DEV)


def _stem_inputs():
    g = torch.Generator().manual_seed(21)
    photos = [R.test_photo(37, 53, 1), R.test_photo(64, 96, 2)]
    return photos, rand32(g, 64, 3, 7, 7, scale=147 ** -0.5 / 64), rand32(g, 64, scale=0.1)


def test_stem_reads_the_photos_where_they_lie_and_the_pool_skips_taps_outside():
    from vspbfr_amd import _lib, detect_r50 as D5, hip_ops as H
    photos, w, b = _stem_inputs()
    flat = np.concatenate([p.reshape(-1) for p in photos])
    tab = (_lib.DetSrc * 2)()
    tab[0].off, tab[0].h, tab[0].w, tab[0].slot = 0, 37, 53, 1            # the slots are swapped: item order is not canvas order
    tab[1].off, tab[1].h, tab[1].w, tab[1].slot = 37 * 53 * 3, 64, 96, 0
    tab_dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(DEV)
    y = torch.full((2 * 32 * 48 * 64,), float("nan"), device=DEV, dtype=torch.float16)
    H.det50_stem_u8(y, torch.from_numpy(flat).to(DEV), tab, tab_dev, 2, D5.pack_stem(w).to(DEV), b.to(DEV), 2, 64, 96)
    order = [photos[1], photos[0]]
    got = nchw(y, 2, 32, 48, 64)
    close(got, R5.stem_ref(order, 64, 96, w, b, torch.float64), R5.stem_ref(order, 64, 96, w, b, torch.float32), "stem 64x96 + 37x53 in 64x96", f16=True)
    # the pool is exact: on the kernel's own stem output, and on an odd map whose last window hangs over both borders
    p = H.det50_pool_f16(torch.full((2 * 16 * 24 * 64,), float("nan"), device=DEV, dtype=torch.float16), y, 2, 32, 48, 64)
    assert torch.equal(nchw(p, 2, 16, 24, 64), torch.nn.functional.max_pool2d(got, 3, 2, 1))
    x = (rand16(torch.Generator().manual_seed(22), 2, 64, 13, 17) - 3.0).half().float()     # mostly negative: a zero-padded pool would show
    p = H.det50_pool_f16(torch.empty(2 * 7 * 9 * 64, device=DEV, dtype=torch.float16), nhwc(x), 2, 13, 17, 64)
    assert torch.equal(nchw(p, 2, 7, 9, 64), torch.nn.functional.max_pool2d(x, 3, 2, 1))


CONV_CASES = [  # name, k, stride, cin, cout, (H, W), relu, residual, upsample-add
    ("1x1 64->256 residual relu", 1, 1, 64, 256, (13, 17), True, True, False),
    ("1x1/2 256->512", 1, 2, 256, 512, (13, 17), False, False, False),
    ("1x1 2048->512", 1, 1, 2048, 512, (5, 7), False, False, False),
    ("1x1 1024->256 relu upsample-add", 1, 1, 1024, 256, (8, 10), True, False, True),
    ("3x3 64->64", 3, 1, 64, 64, (13, 17), False, False, False),
    ("3x3/2 128->128", 3, 2, 128, 128, (13, 17), False, False, False),
    ("3x3 512->512", 3, 1, 512, 512, (5, 7), False, False, False),       # the layer a split of K would serve: there is one route
]


def _conv_operands(k, cin, cout, hw, seed):
    g = torch.Generator().manual_seed(seed)
    return rand16(g, 2, cin, *hw), rand16(g, cout, cin, k, k, scale=(k * k * cin) ** -0.5), rand32(g, cout, scale=0.1), g


@pytest.mark.parametrize("name,k,stride,cin,cout,hw,relu,residual,upadd", CONV_CASES, ids=[c[0] for c in CONV_CASES])
def test_convolution(name, k, stride, cin, cout, hw, relu, residual, upadd):
    from vspbfr_amd import detect_r50 as D5, hip_ops as H
    x, w, b, g = _conv_operands(k, cin, cout, hw, cin + cout + k)
    oh, ow = (hw[0] - 1) // stride + 1, (hw[1] - 1) // stride + 1
    res = rand16(g, 2, cout, oh, ow) if residual else None
    up = rand16(g, 2, cout, oh // 2, ow // 2) if upadd else None
    y = torch.full((2 * oh * ow * cout,), float("nan"), device=DEV, dtype=torch.float16)
    H.det50_conv_f16(y, cout, 0, nhwc(x), cin, 0, 2, hw[0], hw[1], D5.pack_conv_weight(w).half().to(DEV), b.to(DEV), stride, relu,
                     res=None if res is None else (nhwc(res), cout, 0), up=None if up is None else (nhwc(up), cout, 0))
    kw = dict(stride=stride, relu=relu, res=res, up=up)
    close(nchw(y, 2, oh, ow, cout), R5.conv_ref(x, w, b, torch.float64, **kw), R5.conv_ref(x, w, b, torch.float32, **kw), f"conv {name} {hw}", f16=True)


def test_convolution_writes_only_its_channel_window_and_reads_one():
    """3x3 256 -> 128 at channel offset 64 of a 256-pitch tensor prefilled with a sentinel; the input is channels 64.. of a 320-pitch one"""
    from vspbfr_amd import detect_r50 as D5, hip_ops as H
    x, w, b, _ = _conv_operands(3, 256, 128, (13, 17), 77)
    y = torch.full((2 * 13 * 17 * 256,), 7.0, device=DEV, dtype=torch.float16)
    H.det50_conv_f16(y, 256, 64, nhwc(x, 320, 64, fill=float("nan")), 320, 64, 2, 13, 17, D5.pack_conv_weight(w).half().to(DEV), b.to(DEV), 1, True)
    full = nchw(y, 2, 13, 17, 256)
    assert bool((full[:, :64] == 7.0).all()) and bool((full[:, 192:] == 7.0).all())
    close(full[:, 64:192], R5.conv_ref(x, w, b, torch.float64, relu=True), R5.conv_ref(x, w, b, torch.float32, relu=True), "conv 3x3 256->128 window", f16=True)
    dense = torch.empty(2 * 13 * 17 * 128, device=DEV, dtype=torch.float16)
    H.det50_conv_f16(dense, 128, 0, nhwc(x), 256, 0, 2, 13, 17, D5.pack_conv_weight(w).half().to(DEV), b.to(DEV), 1, True)
    assert torch.equal(nchw(dense, 2, 13, 17, 128), full[:, 64:192])


def test_residual_in_place_and_batch_independence():
    """the output may be the residual's own window (same bits as apart), and image 1 alone has the bits it has behind image 0"""
    from vspbfr_amd import detect_r50 as D5, hip_ops as H
    x, w, b, g = _conv_operands(1, 64, 256, (13, 17), 99)
    res = rand16(g, 2, 256, 13, 17)
    wi, bd = D5.pack_conv_weight(w).half().to(DEV), b.to(DEV)
    apart = torch.empty(2 * 13 * 17 * 256, device=DEV, dtype=torch.float16)
    H.det50_conv_f16(apart, 256, 0, nhwc(x), 64, 0, 2, 13, 17, wi, bd, 1, True, res=(nhwc(res), 256, 0))
    inplace = nhwc(res)
    H.det50_conv_f16(inplace, 256, 0, nhwc(x), 64, 0, 2, 13, 17, wi, bd, 1, True, res=(inplace, 256, 0))
    assert torch.equal(apart, inplace)
    close(nchw(inplace, 2, 13, 17, 256), R5.conv_ref(x, w, b, torch.float64, relu=True, res=res), R5.conv_ref(x, w, b, torch.float32, relu=True, res=res),
          "conv in place", f16=True)
    one = torch.empty(13 * 17 * 256, device=DEV, dtype=torch.float16)
    H.det50_conv_f16(one, 256, 0, nhwc(x[1:]), 64, 0, 1, 13, 17, wi, bd, 1, True, res=(nhwc(res[1:]), 256, 0))
    assert torch.equal(one, apart[13 * 17 * 256:])


def test_heads_write_the_prior_layout():
    from vspbfr_amd import detect as D, hip_ops as H
    g = torch.Generator().manual_seed(5)
    levels, P = [(8, 12), (4, 6), (2, 3)], 2 * (8 * 12 + 4 * 6 + 2 * 3)
    conf, loc, lm = (torch.full((2, P, n), float("nan"), device=DEV) for n in (2, 4, 10))
    want64, want32, p0 = [], [], 0
    for h, w_ in levels:
        x, w, b = rand16(g, 2, 256, h, w_), rand32(g, 32, 256, 1, 1, scale=1 / 16), rand32(g, 32, scale=0.3)
        H.det50_heads(nhwc(x), 256, 2, h, w_, D.pack_pointwise(w).to(DEV), b.to(DEV), conf, loc, lm, p0)
        p0 += 2 * h * w_
        want64.append(R5.heads_ref(x, w, b, torch.float64))
        want32.append(R5.heads_ref(x, w, b, torch.float32))
    for i, (got, name) in enumerate(((conf, "conf"), (loc, "loc"), (lm, "lm"))):
        close(got, torch.cat([t[i] for t in want64], dim=1), torch.cat([t[i] for t in want32], dim=1), f"heads {name}")


def test_whole_network(detector):
    from vspbfr_amd import detect_r50 as D5
    case = K.detection_case()
    sources, B, Hc, Wc, _ = detector.canvas(photos=case["canvas_photos"], side=K.SIDE)
    assert (B, Hc, Wc) == (2, K.HC, K.WC)
    out = detector.network(sources, B, Hc, Wc)
    for got, r64, r32, name in zip(out, case["o64"], case["o32"], ("conf", "loc", "lm")):
        close(got, r64, r32, f"network {name}")
    # image 0 alone has the bits it has inside the batch of 2 -- and so has a batch that the 2 GiB guard splits into single images
    s1, B1, _, _, _ = detector.canvas(photos=case["canvas_photos"][:1], side=K.SIDE)
    # the canvas of one photo alone is its own size rounded to 32: the same 64 x 96 here
    alone = detector.network(s1, B1, Hc, Wc)
    for a, b in zip(alone, out):
        assert torch.equal(a[0], b[0])
    detector.GUARD_BYTES = D5.image_bytes(Hc, Wc) + 1
    try:
        split = detector.network(sources, B, Hc, Wc)
    finally:
        del detector.GUARD_BYTES
    for a, b in zip(split, out):
        assert torch.equal(a, b)


def test_detect_end_to_end(detector):
    case = K.detection_case()
    res = detector.detect(photos=case["photos"], side=K.SIDE, threshold=K.THRESHOLD, nms=K.NMS)
    for k, (d, (h, w, hr, wr)) in enumerate(zip(res, case["geo"])):
        ref = case["det"][k]
        keep = ref["r64"]["keep"]
        assert d["canvas"] == (K.HC, K.WC) and d["resized"] == (hr, wr)
        assert list(d["prior"].astype(np.int64)) == list(keep) and d["status"] == ref["r64"]["status"] == 0
        assert (d["candidates"], d["nonfinite"]) == (ref["r64"]["candidates"], 0)
        close(d["score"], ref["d64"][0][keep], ref["d32"][0][keep], f"detect score photo {k}")
        sc = max(w / wr, h / hr)                                 # the bound on canvas coordinates, scaled into the photo with them
        for name, col in (("landmarks", 2), ("box", 1)):
            c64, c32 = ref["d64"][col][keep], ref["d32"][col][keep]
            eref = float(np.abs(c32.astype(np.float64) - c64).max())
            tol = (4.0 * eref + 2e-6 * float(np.abs(c64).max())) * sc
            want = R.to_photo(c64.reshape(len(keep), -1, 2), h, w, hr, wr)
            err = float(np.abs(d[name].astype(np.float64).reshape(want.shape) - want).max())
            print(f"DET50 detect {name} photo {k}: e_ref={eref:.3e} e_hip={err:.3e} ratio={err / (eref * sc):.2f} tol={tol:.3e} scale={sc:.4f}")
            assert err <= tol
