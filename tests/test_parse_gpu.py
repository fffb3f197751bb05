"""GPU checks of the face-parsing paste masks (csrc/parse.hip and the masked paste of csrc/face_warp.hip through vspbfr_amd/parse.py and
vspbfr_amd/photo.py) against tests/parse_ref.py.

Bounds (derived, never fitted): with e_ref = max |restatement float32 - restatement float64| of the same case,
    f16 kernel output:  |y - ref64| <= 1/2 f16 ulp at ref64 (2^-24 in the subnormal range) + 4 e_ref + 2e-6 max |ref64|, e_ref and ref64
                        taken before the final rounding to f16;
    fp32 logits:        |v - ref64| <= 4 e_ref + 2e-6 max |ref64|;
    classes:            equal to the float64 argmax at every pixel whose float64 top-two gap exceeds twice the logit bound; the share of
                        pixels left out is capped (0.5 % tail alone, 10 % whole network) and tests/test_parse_ref.py asserts the caps on
                        the same inputs without a GPU;
    blur, masked paste: bytes equal.
Every case prints e_ref / e_hip / ratio under -s.  The convolution's tile is 8 rows x 32 columns at stride 1 and 8 x 16 at stride 2: the
maps sit on, one above and one below it, besides 2 x 2 (the smallest a reflection takes) and odd sizes."""
import numpy as np
import pytest
import torch

import parse_ref as R
import photo_ref as P0

pytestmark = pytest.mark.gpu
DEV = "cuda"
GUARD = 4096                                                  # sentinel elements behind every output buffer

CHANNELS = [(64, 64), (64, 128), (128, 256), (256, 256), (256, 128), (128, 64)]
# (h, w, stride, up)
GEOMETRIES = [(2, 2, 1, False), (3, 5, 1, False), (8, 32, 1, False), (9, 33, 1, False), (7, 31, 1, False),
              (2, 2, 2, False), (3, 5, 2, False), (16, 34, 2, False), (2, 2, 1, True), (5, 17, 1, True)]


def _report(name, e_ref, e_hip):
    print(f"{name}: e_ref {e_ref:.3g} e_hip {e_hip:.3g} ratio {e_hip / max(e_ref, 1e-30):.3g}")


def _nhwc(t):
    return t.permute(0, 2, 3, 1).contiguous().reshape(-1)


def _check_f16(name, got, pre64, pre32):
    """got: the kernel's f16 values as float64, in the layout of pre64"""
    pre64, pre32 = pre64.numpy(), pre32.double().numpy()
    e_ref, half = np.abs(pre32 - pre64).max(), 0.5 * R.f16_ulp(pre64)
    err = np.abs(got - pre64)
    _report(name, e_ref, np.maximum(err - half, 0).max())
    assert np.isfinite(got).all() and (err <= half + 4 * e_ref + 2e-6 * np.abs(pre64).max()).all(), name


def _conv_inputs(cin, cout, h, w, stride, up, nres, faces, seed):
    from vspbfr_amd import hip_ops as H
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(faces, cin, h, w, generator=g) * 0.5)
    x[:, ::7] *= 1e-6                                         # some subnormal inputs
    x = x.to(torch.float16).to(torch.float64)
    wt = torch.randn(cout, cin, 3, 3, generator=g) * (1.0 / (9 * cin)) ** 0.5
    b = torch.randn(cout, generator=g) * 0.05
    oh, ow = H.parse_conv_out(h, w, stride, up)
    res = [(torch.randn(faces, cout, oh, ow, generator=g) * 0.5).to(torch.float16).to(torch.float64) for _ in range(nres)]
    return x, wt, b, res, oh, ow


def _run_conv(x, wt, b, res, oh, ow, stride, up, act, alias):
    """-> the kernel's output as float64 (NHWC, flat); sentinels behind the output are asserted"""
    from vspbfr_amd import hip_ops as H, parse as P
    faces, cin, h, w = x.shape
    cout = wt.shape[0]
    n = faces * oh * ow * cout
    y = torch.full((n + GUARD,), 7.0, dtype=torch.float16, device=DEV)
    rs = [_nhwc(r).to(torch.float16).to(DEV) for r in res]
    if alias:                                                 # the first residual IS the output tensor
        y[:n] = rs[0]
        rs[0] = y[:n]
    H.parse_conv_f16(y[:n], _nhwc(x).to(torch.float16).to(DEV), faces, h, w, P.pack_conv_weight(wt).to(DEV), b.to(DEV), stride=stride,
                     act=act, up=up, res1=rs[0] if rs else None, res2=rs[1] if len(rs) > 1 else None)
    y = y.cpu().double()
    assert (y[n:] == 7.0).all()
    return y[:n].numpy()


@pytest.mark.parametrize("gi", range(len(GEOMETRIES)), ids=[f"{h}x{w}_s{s}{'_up' if u else ''}" for h, w, s, u in GEOMETRIES])
@pytest.mark.parametrize("ci", range(len(CHANNELS)), ids=[f"{a}to{b}" for a, b in CHANNELS])
def test_conv_alone(ci, gi):
    """every channel pair at every geometry; activation, residual count and aliasing cycle with the case index so that each combination
    occurs for every geometry and every channel pair somewhere: act = k even; residuals k % 3; the first residual aliases the output for
    odd k"""
    (cin, cout), (h, w, stride, up) = CHANNELS[ci], GEOMETRIES[gi]
    k = ci + gi
    act, nres = k % 2 == 0, k % 3
    alias = nres >= 1 and k % 2 == 1
    x, wt, b, res, oh, ow = _conv_inputs(cin, cout, h, w, stride, up, nres, 2, 300 + 16 * ci + gi)
    got = _run_conv(x, wt, b, res, oh, ow, stride, up, act, alias)
    pre64 = _nhwc(R.conv_pre(x, wt, b, torch.float64, stride, up, act, res))
    pre32 = _nhwc(R.conv_pre(x, wt, b, torch.float32, stride, up, act, res))
    _check_f16(f"conv {cin}->{cout} {h}x{w} s{stride} up{int(up)} act{int(act)} res{nres} alias{int(alias)}", got, pre64, pre32)


@pytest.mark.parametrize("act,nres,alias", [(False, 0, False), (True, 0, False), (False, 1, False), (True, 1, True), (False, 2, False), (True, 2, True)])
def test_conv_epilogue_options_at_one_shape(act, nres, alias):
    """with and without activation, one and two residuals, a residual aliasing the output: all at 128 -> 256, 9 x 33"""
    x, wt, b, res, oh, ow = _conv_inputs(128, 256, 9, 33, 1, False, nres, 2, 900)
    got = _run_conv(x, wt, b, res, oh, ow, 1, False, act, alias)
    pre64 = _nhwc(R.conv_pre(x, wt, b, torch.float64, 1, False, act, res))
    pre32 = _nhwc(R.conv_pre(x, wt, b, torch.float32, 1, False, act, res))
    _check_f16(f"conv epilogue act{int(act)} res{nres} alias{int(alias)}", got, pre64, pre32)


@pytest.mark.parametrize("h,w,stride,up", [(9, 33, 1, False), (16, 34, 2, False), (5, 17, 1, True)])
def test_three_faces_in_one_launch_equal_each_face_alone(h, w, stride, up):
    x, wt, b, res, oh, ow = _conv_inputs(128, 256, h, w, stride, up, 1, 3, 950)
    together = _run_conv(x, wt, b, res, oh, ow, stride, up, True, False).reshape(3, -1)
    for f in range(3):
        alone = _run_conv(x[f:f + 1], wt, b, [res[0][f:f + 1]], oh, ow, stride, up, True, False)
        assert np.array_equal(together[f].view(np.uint64), alone.view(np.uint64)), f     # bit for bit


# --------------------------------------------------------------------------------------------------------------------- head and tail
@pytest.mark.parametrize("faces", [1, 3])
@pytest.mark.parametrize("h,w", [(2, 2), (9, 33), (32, 32)])
def test_head_alone(h, w, faces):
    from vspbfr_amd import hip_ops as H, parse as P
    g = torch.Generator().manual_seed(40 + h)
    wt, b = torch.randn(64, 3, 3, 3, generator=g) * (1.0 / 27) ** 0.5, torch.randn(64, generator=g) * 0.05
    crops = np.random.default_rng(h * w + faces).integers(0, 256, (faces, h, w, 3), dtype=np.uint8)
    n = faces * h * w * 64
    y = torch.full((n + GUARD,), 7.0, dtype=torch.float16, device=DEV)
    H.parse_head_u8(y[:n], torch.from_numpy(crops).to(DEV), P.pack_head_weight(wt).to(DEV), b.to(DEV))
    y = y.cpu().double()
    assert (y[n:] == 7.0).all()
    _check_f16(f"head {faces} x {h}x{w}", y[:n].numpy(), _nhwc(R.head_pre(crops, wt, b, torch.float64)), _nhwc(R.head_pre(crops, wt, b, torch.float32)))


def _run_tail(x, wt, b, keep=None):
    from vspbfr_amd import hip_ops as H, parse as P
    faces, _, h, w = x.shape
    bias = torch.zeros(32)
    bias[:19] = b
    kw = {} if keep is None else {"keep": keep}
    cls, kmap, info, lg = H.parse_mask_u8(_nhwc(x).to(torch.float16).to(DEV), faces, h, w, P.pack_conv_weight(wt, nb=2).to(DEV), bias.to(DEV),
                                          logits=True, **kw)
    return cls.cpu().numpy(), kmap.cpu().numpy(), info.cpu().numpy(), lg.cpu().double().numpy()


@pytest.mark.parametrize("faces", [1, 3])
@pytest.mark.parametrize("h,w", [(2, 2), (9, 33), (32, 32)])
def test_tail_alone(h, w, faces):
    x, wt, b = R.tail_case(h, w, faces, seed=60 + h)
    cls, kmap, info, lg = _run_tail(x, wt, b)
    l64, l32 = R.mask_logits(x, wt, b, torch.float64).numpy(), R.mask_logits(x, wt, b, torch.float32).double().numpy()
    tol, e_ref = R.logit_bound(l64, l32)
    err = np.abs(lg - l64)
    _report(f"tail {faces} x {h}x{w}", e_ref, err.max())
    assert np.isfinite(lg).all() and (err <= tol).all() and not info.any()
    assert np.array_equal(cls, R.argmax_classes(lg)[0]) and np.array_equal(kmap, R.KEEP[cls])      # the device's argmax of its own logits


def test_tail_class_map_and_the_planted_tie():
    """on the inputs of tests/test_parse_ref.py::test_condition_of_the_tail_class_test: the class is the float64 argmax wherever the
    float64 top-two gap (the tied class aside) exceeds twice the logit bound, at most 0.5 % of the pixels are left out, and the two
    classes with identical weights and bias resolve to the lower index on the device"""
    x, wt, b = R.tail_case()
    cls, kmap, info, lg = _run_tail(x, wt, b)
    l64, l32 = R.mask_logits(x, wt, b, torch.float64).numpy(), R.mask_logits(x, wt, b, torch.float32).double().numpy()
    tol, e_ref = R.logit_bound(l64, l32)
    out = R.left_out(l64, tol, drop=R.TIE[1])
    c64 = R.argmax_classes(l64)[0]
    print(f"tail classes: e_ref {e_ref:.3g} e_hip {np.abs(lg - l64).max():.3g} left out {out.mean():.4%}, differing among the held {int((cls != c64)[~out].sum())}, "
          f"pixels won by the tied pair {int((c64 == R.TIE[0]).sum())}")
    assert out.mean() <= R.TAIL_LEFT_OUT_CAP and (cls[~out] == c64[~out]).all()
    assert np.array_equal(lg[..., R.TIE[0]], lg[..., R.TIE[1]]) and (cls != R.TIE[1]).all() and (c64 == R.TIE[0]).sum() > 20
    # another keep table
    keep = [1 if c in (3, 5) else 0 for c in range(19)]
    cls2, kmap2, _, _ = _run_tail(x, wt, b, keep=keep)
    assert np.array_equal(cls2, cls) and np.array_equal(kmap2, np.isin(cls, (3, 5)).astype(np.uint8))


# -------------------------------------------------------------------------------------------------------------------- whole network
@pytest.fixture(scope="module")
def parsers():
    from vspbfr_amd import parse as P
    return {size: P.FaceParser(R.net_case(size, faces)[0], DEV) for size, faces in R.NET_CASES}


@pytest.mark.parametrize("size,faces", R.NET_CASES)
def test_whole_network(parsers, size, faces):
    net = parsers[size]
    _, crops, l64, l32 = R.net_case(size, faces)
    dev = torch.from_numpy(crops).to(DEV)
    before = net.launches
    lg = net.logits(dev).cpu().double().numpy()
    assert net.launches - before == 1 + 3 * 8 + 2 * 10 + 1                   # head, three per scaled block, two per body block, tail
    tol, e_ref = R.logit_bound(l64, l32)
    err = np.abs(lg - l64)
    _report(f"net S {size} F {faces} logits", e_ref, err.max())
    out = R.left_out(l64, tol)
    c64 = R.argmax_classes(l64)[0]
    cls = net.classes(dev).cpu().numpy()
    print(f"net S {size} F {faces}: left out {out.mean():.4%}, classes differing among the held {int((cls != c64)[~out].sum())}, overall {np.mean(cls != c64):.4%}")
    assert np.isfinite(lg).all() and (err <= tol).all()
    assert out.mean() <= R.NET_LEFT_OUT_CAP and (cls[~out] == c64[~out]).all()
    assert np.array_equal(cls, R.argmax_classes(lg)[0])
    # chunks of one face give the same bits as the whole call
    net.max_chunk, keep = 1, net.max_chunk
    try:
        assert torch.equal(net.classes(dev), torch.from_numpy(cls).to(DEV))
    finally:
        net.max_chunk = keep


# ---------------------------------------------------------------------------------------------------------------------------- blur
def _keep_maps(size):
    rng = np.random.default_rng(size)
    blob = np.zeros((size, size), np.uint8)
    blob[size // 4:3 * size // 4, size // 5:4 * size // 5] = 1
    corner = np.zeros((size, size), np.uint8)
    corner[0, 0] = 1
    far = np.zeros((size, size), np.uint8)
    far[size - 1, size - 1] = 1
    return np.stack([np.ones((size, size), np.uint8), np.zeros((size, size), np.uint8), corner, far, blob,
                     (rng.random((size, size)) < 0.5).astype(np.uint8)])


@pytest.mark.parametrize("size", [32, 64])
@pytest.mark.parametrize("which", ["default", "r1", "widest", "identity"])
def test_blur_and_border_bytes(size, which):
    from vspbfr_amd import hip_ops as H, parse as P
    taps = {"default": P.default_taps(size), "r1": np.array([32768, 16384]), "widest": P.taps_for(size / 3.0, min(size - 1, 64)),
            "identity": np.array([65536])}[which]
    if which == "widest" and size == 32:
        assert taps.size == 32                                # R = S - 1
    keep = _keep_maps(size)
    for border in (0, P.default_border(size), size // 2):
        n = keep.size
        out = torch.from_numpy(np.full(n + GUARD, 999, np.uint16)).to(DEV)
        got = H.parse_blur_u16(torch.from_numpy(keep).to(DEV), taps, border, out=out[:n].view(keep.shape))
        ref = R.paste_weights(keep, taps, border)
        full = out.cpu().numpy()
        assert (full[n:] == 999).all()
        got = got.cpu().numpy()
        print(f"blur S {size} {which} R {taps.size - 1} border {border}: differing {int((got != ref).sum())}, max weight {int(ref.max())}")
        assert np.array_equal(got, ref)
        if border == 0:
            assert (ref[0] == 256).all() and (ref[1] == 0).all()


# -------------------------------------------------------------------------------------------------------------------- masked paste
S = 64
SIZES = [(67, 131), (130, 65), (1, 40), (50, 50), (90, 80)]        # (w, h): rows off dword alignment, one pixel wide, one without a face
FACES = [(0, 0.37, 17.0, (33.0, 65.0)),        # larger than its photo: over all four edges at once
         (0, 2.9, -163.0, (30.0, 60.0)),       # small (minified 2.9 times into the photo), overlapped by face 0
         (0, 1.0, 17.0, (0.0, 60.0)),          # over the left edge
         (0, 1.3, 5.0, (33.0, 129.0)),         # over the bottom edge
         (1, 1.0, 17.0, (128.0, 63.0)),        # over the bottom right corner
         (1, 0.8, -10.0, (50.0, 30.0)),
         (1, 0.8, 10.0, (70.0, 34.0)),         # overlaps the face before it
         (4, 1.1, 17.0, (45.0, 40.0)),
         (2, 2.9, 0.0, (0.0, 20.0))]           # on the one-pixel-wide photo


def _masks(n, seed=5):
    rng = np.random.default_rng(seed)
    m = rng.integers(0, 257, (n, S, S)).astype(np.uint16)
    m[:, :8] = 0
    m[:, -8:] = 256
    m[1::2] = R.paste_weights((rng.random((len(m[1::2]), S, S)) < 0.6).astype(np.uint8), np.array([32768, 12288, 4096]), 2)     # smooth ones
    return m


def _paste(photos, faces, restored, masks, upscale, antialias, base=None):
    from vspbfr_amd import photo as P
    plan = P.FacePlan(photos, faces, size=S, upscale=upscale, antialias=antialias)
    base = photos if base is None else base
    out = torch.from_numpy(np.concatenate([b.reshape(-1) for b in base])).to(DEV)
    mask = None if masks is None else torch.from_numpy(np.ascontiguousarray(masks, dtype=np.uint16)).to(DEV)
    out = P.paste_faces(plan, torch.from_numpy(restored).to(DEV), DEV, out=out, mask=mask)
    return [o.cpu().numpy() for o in plan.split(out)]


def _ref_paste(base, faces, restored, masks, upscale, antialias):
    out = []
    for k, b in enumerate(base):
        mine = [(restored[i], P0.paste_matrix(P0.similarity(pts, S), upscale), masks[i]) for i, (kk, pts) in enumerate(faces) if kk == k]
        out.append(R.paste_masked(b, mine, S, antialias=antialias))
    return out


@pytest.mark.parametrize("antialias", [False, True], ids=["plain", "aa"])
@pytest.mark.parametrize("upscale", [1, 2])
def test_masked_paste_bytes(upscale, antialias):
    photos = [P0.test_photo(w, h, seed=11 + k) for k, (w, h) in enumerate(SIZES)]
    faces = [(k, P0.landmarks_for(sc, ang, c, S)) for k, sc, ang, c in FACES]
    restored = np.stack([P0.test_photo(S, S, seed=101 + i) for i in range(len(faces))])
    masks = _masks(len(faces))
    base = photos if upscale == 1 else [np.ascontiguousarray(np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)) for p in photos]
    got = _paste(photos, faces, restored, masks, upscale, antialias, base)
    ref = _ref_paste(base, faces, restored, masks, upscale, antialias)
    for k in range(len(photos)):
        print(f"masked paste x{upscale} aa{int(antialias)} photo {k} {got[k].shape}: differing bytes {int((got[k] != ref[k]).sum())}, "
              f"changed {int((ref[k] != base[k]).any(axis=2).sum())} px")
        assert np.array_equal(got[k], ref[k]), k
    assert np.array_equal(got[3], base[3]) and not np.array_equal(got[0], base[0])
    # a mask of all 256 gives the bytes of the existing entries, an all-zero mask leaves the photos untouched
    full = _paste(photos, faces, restored, np.full_like(masks, 256), upscale, antialias, base)
    plain = _paste(photos, faces, restored, None, upscale, antialias, base)
    zero = _paste(photos, faces, restored, np.zeros_like(masks), upscale, antialias, base)
    for k in range(len(photos)):
        assert np.array_equal(full[k], plain[k]) and np.array_equal(zero[k], base[k]), k
    # the overlapping pair in the other order
    order = list(range(len(faces)))
    order[5], order[6] = 6, 5
    faces2, restored2, masks2 = [faces[i] for i in order], restored[order], masks[order]
    got2 = _paste(photos, faces2, restored2, masks2, upscale, antialias, base)
    ref2 = _ref_paste(base, faces2, restored2, masks2, upscale, antialias)
    assert np.array_equal(got2[1], ref2[1]) and not np.array_equal(got2[1], got[1])


# ----------------------------------------------------------------------------------------------------------------------- end to end
class _Pipe:
    """a stand-in for the restoration pipeline: a fixed pointwise map of the crops"""

    def __call__(self, low):
        return {"restored": (low.flip(1) * 0.9).clamp(-1, 1)}


def _restorer_case(upscale):
    photos = [P0.test_photo(90, 80, seed=3), P0.test_photo(50, 64, seed=4), P0.test_photo(40, 40, seed=5)]
    marks = [[P0.landmarks_for(2.0, 10.0, (45.0, 40.0), S), P0.landmarks_for(1.5, -15.0, (60.0, 50.0), S)], [P0.landmarks_for(2.5, -20.0, (20.0, 30.0), S)], None]
    return photos, marks


@pytest.mark.parametrize("color_fix", [None, "wavelet"])
@pytest.mark.parametrize("antialias", [False, True], ids=["plain", "aa"])
def test_photo_restorer_with_a_parser(parsers, antialias, color_fix):
    from vspbfr_amd import parse as P, photo as PH
    net = parsers[64]
    photos, marks = _restorer_case(1)
    rest = PH.PhotoRestorer(_Pipe(), 2, upscale=1, size=S, antialias=antialias, color_fix=color_fix, parser=net)
    outs, crops, restored, plan, *fixed = rest(photos, marks, DEV)
    info = rest.parse_info
    cls, mask = info["classes"].cpu().numpy(), info["mask"].cpu().numpy()
    assert cls.shape == (3, S, S) and not info["flags"].cpu().any()
    assert torch.equal(info["classes"], net.classes(restored))                 # from the network's restored crops, also with a colour fix
    ref_mask = R.paste_weights(R.KEEP[cls], P.default_taps(S), P.default_border(S))
    assert np.array_equal(mask, ref_mask) and 0 < ref_mask.mean() < 256
    pasted = (fixed[0] if fixed else restored).cpu().numpy()
    faces = [(k, pts) for k, per in enumerate(marks) for pts in (per or [])]
    ref = _ref_paste(photos, faces, pasted, ref_mask, 1, antialias)
    bg = plan.split(plan.background(DEV))
    for k in range(3):
        got = outs[k].cpu().numpy()
        assert np.array_equal(got, ref[k]), k
        outside = np.ones(got.shape[:2], bool)
        for i, (x0, y0, x1, y1) in enumerate(plan.boxes):
            if plan.face_photo[i] == k:
                outside[y0:y1, x0:x1] = False
        assert np.array_equal(got[outside], bg[k].cpu().numpy()[outside])
    assert np.array_equal(outs[2].cpu().numpy(), photos[2])
    # without a parser: the old path, other bytes
    plain = PH.PhotoRestorer(_Pipe(), 2, upscale=1, size=S, antialias=antialias, color_fix=color_fix)(photos, marks, DEV)[0]
    assert not np.array_equal(plain[0].cpu().numpy(), outs[0].cpu().numpy())
    print(f"restorer aa{int(antialias)} fix {color_fix}: mask mean {ref_mask.mean() / 256:.3f}, classes {np.unique(cls).tolist()}")


def test_photo_restorer_with_a_parser_keeps_the_upscalers_bytes_where_the_weight_is_zero(parsers):
    import sr_ref
    from vspbfr_amd import photo as PH, upscale as U
    net = parsers[64]
    sr = U.SrUpscaler(sr_ref.make_state(2, 2, seed=60), DEV)
    photos, marks = _restorer_case(2)
    rest = PH.PhotoRestorer(_Pipe(), 4, upscale=2, size=S, background=sr, parser=net)
    outs, crops, restored, plan = rest(photos, marks, DEV)
    bg, _ = sr.upscale(photos=photos)
    bgs = [b.cpu().numpy() for b in plan.split(bg)]
    faces = [(k, pts) for k, per in enumerate(marks) for pts in (per or [])]
    ref = _ref_paste(bgs, faces, restored.cpu().numpy(), rest.parse_info["mask"].cpu().numpy(), 2, False)
    kept = 0
    for k in range(3):
        got = outs[k].cpu().numpy()
        assert np.array_equal(got, ref[k]), k
        for i, (x0, y0, x1, y1) in enumerate(plan.boxes):
            if plan.face_photo[i] == k:
                same = (got[y0:y1, x0:x1] == bgs[k][y0:y1, x0:x1]).all(axis=2)
                kept += int(same.sum())
                assert same.any() and not same.all()            # inside the box: the upscaler's bytes where w = 0, the face elsewhere
    print(f"upscaler bytes kept inside the paste boxes: {kept} px")


def test_a_planted_f16_overflow_sets_the_flag_gives_class_zero_and_keeps_the_photo():
    """one head weight of 1e5 (fp32) drives channel 5 of the first activation past 65 504 wherever the crop is not mid-grey: the f16
    store gives inf, the logits are not finite, the pixel is class 0, the face is flagged, its mask is 0 and the photo keeps its pixels;
    the mid-grey crop beside it in the call stays finite"""
    from vspbfr_amd import hip_ops as H, parse as P, photo as PH
    sd = R.make_state(seed=77)
    sd["encoder.0.conv2d.weight"][5, 0, 1, 1] = 1e5
    net = P.FaceParser(sd, DEV)
    hot, calm = R.test_crops(1, S, seed=78)[0], np.full((S, S, 3), 128, np.uint8)
    with torch.no_grad():
        l32 = R.logits(R.fold(sd), np.stack([hot, calm]), torch.float32)
    assert not torch.isfinite(l32[0]).all(dim=-1).any() and torch.isfinite(l32[1]).all()       # every pixel of the hot face, none of the calm one
    crops = torch.from_numpy(np.stack([hot, calm])).to(DEV)
    lg = net.logits(crops)
    mask, flags, cls = net.mask(crops, classes=True)
    bad = ~torch.isfinite(lg).all(dim=-1)
    assert flags.cpu().tolist() == [H.PARSE_NONFINITE, 0] and bad[0].any() and not bad[1].any() and (cls[bad] == 0).all()
    print(f"non-finite pixels: {int(bad.sum())} of {bad.numel()}, flags {flags.cpu().tolist()}, mask sum of the hot face {int(mask[0].cpu().numpy().sum())}")
    assert bad[0].all() and int(mask[0].cpu().numpy().sum()) == 0
    photo = P0.test_photo(90, 80, seed=3)
    plan = PH.FacePlan([photo], [(0, P0.landmarks_for(2.0, 10.0, (45.0, 40.0), S))], size=S)
    out = PH.paste_faces(plan, crops[:1], DEV, mask=mask[:1])
    assert np.array_equal(plan.split(out)[0].cpu().numpy(), photo)
