"""CPU checks of the face-parsing paste masks: vspbfr_amd/parse.py against tests/parse_ref.py, the restatement against torch
and against itself, the entries' refusals, both parsers -- and the conditions of the GPU class tests, recomputed here on the very inputs
tests/test_parse_gpu.py uses, so that they are verified where there is no GPU."""
import ctypes as C

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import parse_ref as R
import photo_ref as P0


# ------------------------------------------------------------------------------------------------------------------------- loader
def test_key_set_and_count():
    from vspbfr_amd import parse as P
    want = P.expected_state()
    sd = R.ParseNet().state_dict()
    assert len(want) == 238 and set(want) == set(sd)
    assert all(tuple(sd[k].shape) == tuple(s) for k, s in want.items())
    assert len(P.blocks()) == 18 and sum(1 for _, _, _, s in P.blocks() if s != "none") == 8
    st = P.check_state_dict({"module." + k: v for k, v in R.make_state(1).items()})
    assert len(st.tensors) == 238 - 36 and P.check_state_dict(st) is st
    sd2 = {k: v for k, v in R.make_state(1).items() if not k.endswith("num_batches_tracked")}
    assert set(P.check_state_dict(sd2).tensors) == set(st.tensors)


def test_loader_refusals_name_the_key():
    from vspbfr_amd import parse as P
    sd = R.make_state(2)
    for drop in ("encoder.0.conv2d.bias", "body.4.conv2.norm.norm.running_var", "decoder.3.shortcut_func.conv2d.weight", "out_img_conv.conv2d.bias"):
        bad = dict(sd)
        bad.pop(drop)
        with pytest.raises(ValueError, match="missing keys " + drop.replace(".", r"\.")):
            P.check_state_dict(bad)
    for extra in ("body.0.shortcut_func.conv2d.weight", "encoder.0.norm.norm.weight", "out_mask_conv.conv2d.extra"):
        with pytest.raises(ValueError, match="unexpected keys " + extra.replace(".", r"\.")):
            P.check_state_dict(dict(sd, **{extra: torch.zeros(1)}))
    for key, shape in (("out_mask_conv.conv2d.weight", (18, 64, 3, 3)), ("out_img_conv.conv2d.weight", (3, 64, 1, 1)),
                       ("encoder.1.conv1.norm.norm.weight", (64,)), ("decoder.2.conv1.conv2d.weight", (128, 128, 3, 3))):
        with pytest.raises(ValueError, match=key.replace(".", r"\.") + " has shape"):
            P.check_state_dict(dict(sd, **{key: torch.zeros(shape)}))
    with pytest.raises(ValueError, match="expected a state dict"):
        P.check_state_dict([1])
    for size in (16, 40, 31, 0, 512.5, True):
        with pytest.raises(ValueError, match="multiple of 16"):
            P.check_size(size)
    assert P.check_size(32) == 32 and P.check_size(512) == 512


# --------------------------------------------------------------------------------------------------------------------------- fold
def test_fold_equals_the_unfused_tree_in_float64():
    """The folded network WITHOUT any f16 rounding against the nn tree in eval mode, both float64.  Bound: a logit is a chain of 39
    convolutions deep; one convolution of K = 9 Cin <= 2304 terms carries a relative error of at most (K + 3) eps on the sum of its
    absolute products in either form, and the two forms differ by the three roundings of the fold per weight.  With every intermediate
    tensor bounded by A = max |activation| the difference is below 39 (2304 + 8) eps A_sum, A_sum the largest sum of |w| |x| of a pixel;
    the test takes the crude 39 * 2312 * eps * 64 (A_sum < 64 holds for these weights by a wide margin: asserted)."""
    from vspbfr_amd import parse as P
    sd = R.make_state(3)
    crops = R.test_crops(1, 32, seed=4)
    mine, theirs = P.fold_state(sd), R.fold(sd)
    assert set(mine) == set(theirs) and len(mine) == 2 + 8 + 36
    for k in mine:
        assert torch.equal(mine[k][0], theirs[k][0]) and torch.equal(mine[k][1], theirs[k][1]), k
    net = R.unfused(sd)
    x = R.crops_f(crops, torch.float64)
    with torch.no_grad():
        ref = net(x)
        worst = 0.0

        def conv(t, name, stride=1, up=False, act=False):
            nonlocal worst
            w, b = mine[name]
            g = R.gather_input(t, up)
            worst = max(worst, float(F.conv2d(g.abs(), w.abs(), b.abs(), stride=stride).max()))
            y = F.conv2d(g, w, b, stride=stride)
            return F.leaky_relu(y, 0.2) if act else y

        t = conv(x, "head")
        feat = None
        for p, _, _, scale in P.blocks():
            if p == "body.0":
                feat = t
            sc = t if scale == "none" else conv(t, p + ".shortcut", stride=2 if scale == "down" else 1, up=scale == "up")
            u = conv(t, p + ".conv1", up=scale == "up", act=True)
            t = sc + conv(u, p + ".conv2", stride=2 if scale == "down" else 1)
            if p == "body.9":
                t = t + feat
        got = conv(t, "mask")
    assert worst < 64, worst
    bound = 39 * 2312 * np.finfo(np.float64).eps * 64
    err = float((got - ref).abs().max())
    print(f"fold: max |folded - unfused| {err:.3g} of {bound:.3g}, largest sum of absolute products {worst:.3g}")
    assert err <= bound


def test_folded_restatement_without_rounding_is_the_tree():
    """the restatement's own index gathers (up, reflection) and block order give the tree's logits when nothing is rounded to f16.  Weights
    and biases still pass through fp32 (the kernels' biases are fp32): a relative 2^-24 per operand, so at most 2^-24 of the largest sum
    of absolute products (below 64, asserted in the test above) per convolution, 39 convolutions deep, on top of the float64 bound."""
    sd = R.make_state(5)
    crops = R.test_crops(1, 32, seed=6)
    folded = R.fold(sd)
    keep = R.f16
    try:
        R.f16 = lambda t: t
        with torch.no_grad():
            got = R.logits(folded, crops, torch.float64)
    finally:
        R.f16 = keep
    with torch.no_grad():
        ref = R.unfused(sd)(R.crops_f(crops, torch.float64)).permute(0, 2, 3, 1)
    assert float((got - ref).abs().max()) <= 39 * 64 * (2.0 ** -24 + 2312 * np.finfo(np.float64).eps)


# ------------------------------------------------------------------------------------------------------------------- weight image
@pytest.mark.parametrize("cout,cin,nb", [(64, 64, 4), (128, 64, 4), (256, 128, 4), (64, 256, 4), (19, 64, 2)])
def test_weight_image_entry_by_entry_and_round_trip(cout, cin, nb):
    from vspbfr_amd import parse as P
    g = torch.Generator().manual_seed(cout + cin)
    w = torch.randn(cout, cin, 3, 3, generator=g)
    img = P.pack_conv_weight(w, nb=nb)
    cb_n, kc_n = -(-cout // (16 * nb)), cin // 64
    assert tuple(img.shape) == (cb_n, kc_n, 18, nb, 64, 8) and img.dtype == torch.float16 and img.is_contiguous()
    w16 = w.to(torch.float16)
    idx = np.indices(tuple(img.shape)).reshape(6, -1)
    cb, kc, s, n, l, j = idx
    co, ci = 16 * nb * cb + 16 * n + (l & 15), 64 * kc + 32 * (s & 1) + 8 * (l >> 4) + j
    ky, kx = (s >> 1) // 3, (s >> 1) % 3
    inside = co < cout
    want = torch.zeros(idx.shape[1], dtype=torch.float16)
    want[torch.from_numpy(inside)] = w16[co[inside], ci[inside], ky[inside], kx[inside]]
    assert torch.equal(img.reshape(-1), want)
    assert torch.equal(P.unpack_conv_weight(img, cout), w16)
    # every weight appears exactly once
    assert int(inside.sum()) == w.numel()


def test_weight_packing_refusals_and_head_layout():
    from vspbfr_amd import parse as P
    for shape in ((64, 32, 3, 3), (64, 96, 3, 3), (64, 64, 1, 1), (0, 64, 3, 3)):
        with pytest.raises(ValueError, match="pack_conv_weight"):
            P.pack_conv_weight(torch.zeros(shape))
    with pytest.raises(ValueError, match="pack_conv_weight"):
        P.pack_conv_weight(torch.zeros(64, 64, 3, 3), nb=3)
    w = torch.randn(64, 3, 3, 3)
    h = P.pack_head_weight(w)
    for ky, kx, c, co in ((0, 0, 0, 0), (2, 1, 2, 63), (1, 2, 1, 17)):
        assert h[(3 * ky + kx) * 3 + c, co] == w[co, c, ky, kx]
    with pytest.raises(ValueError, match="pack_head_weight"):
        P.pack_head_weight(torch.zeros(64, 3, 3, 1))


# --------------------------------------------------------------------------------------------------------------------- index maps
@pytest.mark.parametrize("h", [2, 3, 5])
@pytest.mark.parametrize("up", [False, True])
def test_up_and_reflection_index_maps_are_torchs(h, up):
    w = h + 1
    x = torch.arange(2 * 3 * h * w, dtype=torch.float64).reshape(2, 3, h, w)
    ref = F.interpolate(x, scale_factor=2, mode="nearest") if up else x
    ref = F.pad(ref, (1, 1, 1, 1), mode="reflect")
    assert torch.equal(R.gather_input(x, up), ref)
    n = 2 * h if up else h
    assert R.reflect_index(n)[0] == 1 and R.reflect_index(n)[-1] == n - 2 and (R.up_index(h) == np.arange(2 * h) // 2).all()


def test_conv_out_sizes():
    from vspbfr_amd import hip_ops as H
    assert H.parse_conv_out(3, 5, 2) == (2, 3) and H.parse_conv_out(2, 2, 2) == (1, 1) and H.parse_conv_out(16, 34, 2) == (8, 17)
    assert H.parse_conv_out(5, 17, 1, up=True) == (10, 34) and H.parse_conv_out(9, 33) == (9, 33)
    x = torch.zeros(1, 64, 3, 5, dtype=torch.float64)
    y = R.conv_pre(x, torch.zeros(64, 64, 3, 3), torch.zeros(64), torch.float64, stride=2)
    assert tuple(y.shape[2:]) == (2, 3)


# --------------------------------------------------------------------------------------------------------------------------- taps
@pytest.mark.parametrize("size", [32, 48, 64, 128, 256, 512, 1024])
def test_default_taps(size):
    from vspbfr_amd import parse as P
    g = P.default_taps(size).astype(np.int64)
    r = min(int(round(50 * size / 512)), size - 1, 64)
    assert g.size == r + 1 and g[0] + 2 * g[1:].sum() == 65536 and (g >= 0).all() and (np.diff(g) <= 0).all()
    sigma = 11 * size / 512
    ideal = np.exp(-np.arange(r + 1) ** 2 / (2 * sigma ** 2))
    ideal = 65536 * ideal / (ideal[0] + 2 * ideal[1:].sum())
    assert np.abs(g[1:] - ideal[1:]).max() <= 0.5 and abs(g[0] - ideal[0]) <= 0.5 + r     # the remainder of 2 r roundings sits on the centre
    assert P.default_border(size) == int(round(10 * size / 512))
    assert P.default_border(512) == 10 and P.default_taps(512).size == 51 and P.default_border(32) == 1


def test_bad_tap_tables_are_refused():
    from vspbfr_amd import parse as P
    for bad in ([65535], [32768, 16385], [65538, -1], [], [0] * 66, [[65536]]):
        with pytest.raises(ValueError, match="taps"):
            P.check_taps(bad)
    assert P.check_taps([65536]).tolist() == [65536] and P.check_taps([32768, 16384]).size == 2
    for sigma, radius in ((0, 3), (-1, 3), (2.0, 65), (2.0, -1)):
        with pytest.raises(ValueError, match="taps_for"):
            P.taps_for(sigma, radius)


# --------------------------------------------------------------------------------------------------------------------------- blur
def test_blur_of_a_constant_map_is_constant():
    from vspbfr_amd import parse as P
    for size in (32, 64):
        taps = P.default_taps(size)
        assert (R.paste_weights(np.ones((1, size, size)), taps, 0) == 256).all() and (R.paste_weights(np.zeros((1, size, size)), taps, 0) == 0).all()
        w = R.paste_weights(np.ones((1, size, size)), taps, 3)
        assert (w[:, 3:-3, 3:-3] == 256).all() and w[:, :3].max() == 0 and w[:, -3:].max() == 0 and w[:, :, :3].max() == 0 and w[:, :, -3:].max() == 0


def test_blur_of_an_impulse_is_the_outer_product_of_the_twice_convolved_taps():
    """An impulse far from the edges: the exact answer is 16384 (g*g)[dy] (g*g)[dx] / 2^64 with g*g the taps convolved with themselves
    (sum 2^32).  Each of the four passes rounds once (error <= 1/2) and a later pass of unit gain carries earlier errors through without
    growth, so |m - exact| <= 4 * 1/2 = 2 before the final (m + 32) >> 6, which adds 1/2 in units of the weight: |w - exact / 64| <= 2 / 64 + 1/2."""
    from vspbfr_amd import parse as P
    size, c = 64, 32
    taps = P.default_taps(size).astype(np.int64)
    r = taps.size - 1
    keep = np.zeros((1, size, size), np.uint8)
    keep[0, c, c] = 1
    full = np.concatenate([taps[:0:-1], taps])
    gg = np.convolve(full, full).astype(np.float64)                  # 4 r + 1 entries, centre at 2 r
    exact = np.zeros((size, size))
    for dy in range(-2 * r, 2 * r + 1):
        for dx in range(-2 * r, 2 * r + 1):
            exact[c + dy, c + dx] = 16384.0 * gg[2 * r + dy] * gg[2 * r + dx] / 2.0 ** 64
    assert 2 * r < c                                                  # no reflection takes part
    w = R.paste_weights(keep, taps, 0)[0].astype(np.float64)
    assert np.abs(w - exact / 64).max() <= 2 / 64 + 0.5
    # larger impulse for a visible answer: an 8 x 8 block, by linearity within the same per-pass rounding
    keep[0, c - 4:c + 4, c - 4:c + 4] = 1
    big = np.zeros((size, size))
    for y in range(c - 4, c + 4):
        for x in range(c - 4, c + 4):
            big += np.roll(np.roll(exact, y - c, axis=0), x - c, axis=1)
    w = R.paste_weights(keep, taps, 0)[0].astype(np.float64)
    assert w.max() >= 3 and np.abs(w - big / 64).max() <= 2 / 64 + 0.5


def test_blur_reflects_101_at_both_ends():
    taps = np.array([32768, 8192, 8192], dtype=np.int64)             # R = 2
    m = np.zeros((1, 1, 8), np.int64)
    m[0, 0, 0], m[0, 0, 7] = 1 << 14, 1 << 13
    one = R.blur_pass(m, taps, 2)[0, 0]
    # position 0 sees m[2] m[1] m[0] m[1] m[2]; position 1 sees m[1] m[0] m[1] m[2] m[3]: index -1 is 1, never 0 twice
    assert one[0] == (32768 * 16384 + 32768) >> 16 and one[1] == (8192 * 16384 + 32768) >> 16 and one[2] == one[1] and one[3] == 0
    assert one[7] == (32768 * 8192 + 32768) >> 16 and one[6] == (8192 * 8192 + 32768) >> 16 and one[5] == one[6] and one[4] == 0
    assert (R.reflect101(np.array([-2, -1, 0, 7, 8, 9]), 8) == [2, 1, 0, 7, 6, 5]).all()
    # R = S - 1, the widest table an entry takes
    assert (R.reflect101(np.arange(-7, 15), 8) == [7, 6, 5, 4, 3, 2, 1, 0, 1, 2, 3, 4, 5, 6, 7, 6, 5, 4, 3, 2, 1, 0]).all()


# ------------------------------------------------------------------------------------------------------------------------- argmax
def test_argmax_ties_keep_table_and_non_finite_logits():
    lg = np.zeros((4, 19))
    lg[0, 5] = lg[0, 9] = 1.0                                        # an exact tie: the lower index
    lg[1, 18] = 2.0
    lg[2, 4], lg[2, 11] = 3.0, np.inf                                # non-finite: class 0
    lg[3, 2], lg[3, 0] = 1.0, np.nan
    cls, bad = R.argmax_classes(lg)
    assert cls.tolist() == [5, 18, 0, 0] and bad.tolist() == [False, False, True, True]
    assert R.KEEP.tolist() == [0, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 1, 0, 0, 0] and R.KEEP[cls].tolist() == [1, 0, 0, 0]
    from vspbfr_amd import hip_ops as H, parse as P
    assert tuple(R.KEEP) == P.KEEP == H.PARSE_KEEP
    # two classes with identical weights and bias tie exactly in the restatement, in both precisions
    x, w, b = R.tail_case()
    for dt in (torch.float64, torch.float32):
        l = R.mask_logits(x, w, b, dt).numpy()
        assert (l[..., R.TIE[0]] == l[..., R.TIE[1]]).all()
        cls, _ = R.argmax_classes(l)
        assert (cls != R.TIE[1]).all() and (cls == R.TIE[0]).mean() > 0.05


# ------------------------------------------------------------------------------------------------------------------- masked paste
def _two_faces(S=64):
    photo = P0.test_photo(120, 100, seed=3)
    pts = [P0.landmarks_for(1.4, 12.0, (52.0, 50.0), S), P0.landmarks_for(1.1, -25.0, (70.0, 60.0), S)]
    Ps = [P0.paste_matrix(P0.similarity(p, S), 1) for p in pts]
    crops = [P0.test_photo(S, S, seed=50 + i) for i in range(2)]
    return photo, crops, Ps


@pytest.mark.parametrize("antialias", [False, True])
def test_masked_paste_with_a_full_mask_is_the_unmasked_paste(antialias):
    import photo_aa_ref as A
    S = 64
    photo, crops, Ps = _two_faces(S)
    full = np.full((S, S), 256, np.uint16)
    for order in ((0, 1), (1, 0)):
        plain = (A.paste if antialias else P0.paste)(photo, [(crops[i], Ps[i]) for i in order], S)
        masked = R.paste_masked(photo, [(crops[i], Ps[i], full) for i in order], S, antialias=antialias)
        assert np.array_equal(plain, masked) and not np.array_equal(plain, photo)
    a = R.paste_masked(photo, [(crops[i], Ps[i], full) for i in (0, 1)], S)
    b = R.paste_masked(photo, [(crops[i], Ps[i], full) for i in (1, 0)], S)
    assert not np.array_equal(a, b)                                  # the faces overlap: the order shows
    zero = np.zeros((S, S), np.uint16)
    assert np.array_equal(R.paste_masked(photo, [(crops[0], Ps[0], zero)], S), photo)
    half = np.full((S, S), 128, np.uint16)
    h = R.paste_masked(photo, [(crops[0], Ps[0], half)], S)
    assert not np.array_equal(h, photo) and not np.array_equal(h, P0.paste(photo, [(crops[0], Ps[0])], S))


# ---------------------------------------------------------------------------------------------------------------------- refusals
def test_entries_refuse_what_they_do_not_serve():
    """validation precedes every launch: no GPU needed.  One mutation each."""
    from vspbfr_amd import _lib
    L, p, q, r = _lib.lib, C.c_void_p(1 << 20), C.c_void_p(1 << 24), C.c_void_p(1 << 28)
    keep = (C.c_uint8 * 19)(*R.KEEP.tolist())
    taps = (C.c_int32 * 3)(32768, 8192, 8192)

    def head(y=p, crops=q, F=1, H=8, W=8, w=p, b=p):
        return L.vsp_parse_head_u8(y, crops, F, H, W, w, b, None)

    def conv(y=p, x=q, F=1, H=8, W=8, cin=64, cout=64, stride=1, flags=0, w=r, b=r, r1=None, r2=None):
        return L.vsp_parse_conv_f16(y, x, F, H, W, cin, cout, stride, flags, w, b, r1, r2, None)

    def mask(cls=p, kp=p, lg=None, info=p, x=q, F=1, H=8, W=8, w=r, b=r, table=keep):
        return L.vsp_parse_mask_u8(cls, kp, lg, info, x, F, H, W, w, b, table, None)

    def blur(out=p, kp=q, work=r, wb=4 * 64, F=1, S=8, t=taps, R_=2, border=1):
        return L.vsp_parse_blur_u16(out, kp, work, wb, F, S, t, R_, border, None)

    odd = C.c_void_p((1 << 20) + 8)
    bad_keep = (C.c_uint8 * 19)(*([2] + [0] * 18))
    short = (C.c_int32 * 3)(32768, 8192, 8191)
    neg = (C.c_int32 * 3)(65536, -1, 1)
    cases = [(lambda: head(y=None), "null pointer"), (lambda: head(w=None), "null pointer"), (lambda: head(H=1), "map 1 x 8"),
             (lambda: head(y=odd), "aligned"), (lambda: head(F=-1), "faces"),
             (lambda: conv(x=None), "null pointer"), (lambda: conv(b=None), "null pointer"), (lambda: conv(cin=32), "32 -> 64 channels"),
             (lambda: conv(cout=96), "64 -> 96 channels"), (lambda: conv(cin=0), "channels"), (lambda: conv(H=1), "map 1 x 8"),
             (lambda: conv(W=1), "map 8 x 1"), (lambda: conv(stride=3), "stride 3"), (lambda: conv(stride=0), "stride 0"),
             (lambda: conv(stride=2, flags=2), "up together with stride 2"), (lambda: conv(flags=4), "unknown flags"),
             (lambda: conv(y=odd), "aligned"), (lambda: conv(r1=odd), "aligned"), (lambda: conv(r2=p), "second residual without a first"),
             (lambda: conv(x=C.c_void_p((1 << 20) + 4096)), "overlaps the input"), (lambda: conv(x=p), "overlaps the input"),
             (lambda: conv(r1=C.c_void_p((1 << 20) + 16)), "residual overlaps the output"),
             (lambda: conv(r1=q, r2=C.c_void_p((1 << 20) - 16)), "residual overlaps the output"),
             (lambda: mask(cls=None), "null pointer"), (lambda: mask(table=None), "null pointer"), (lambda: mask(info=None), "null pointer"),
             (lambda: mask(W=1), "map 8 x 1"), (lambda: mask(x=odd), "aligned"), (lambda: mask(table=bad_keep), "keep table entry 0 is 2"),
             (lambda: blur(out=None), "null pointer"), (lambda: blur(t=None), "null pointer"), (lambda: blur(t=short), "sum to 65534"),
             (lambda: blur(t=neg), "tap 1 is -1"), (lambda: blur(R_=65), "radius 65"), (lambda: blur(R_=-1), "radius -1"),
             (lambda: blur(S=2, R_=2), "radius 2"), (lambda: blur(border=5), "border 5"), (lambda: blur(border=-1), "border -1"),
             (lambda: blur(wb=4 * 64 - 1), "work of 255 bytes"), (lambda: blur(work=C.c_void_p((1 << 20) + 64)), "overlap"), (lambda: blur(S=1), "size 1")]
    for call, msg in cases:
        rc = call()
        assert rc == -1 and msg in _lib.last_error(), (rc, msg, _lib.last_error())
    # 2 GiB guards: VSP_ENOTSUP
    assert head(F=64, H=512, W=512) == -3 and "2 GiB" in _lib.last_error()
    assert conv(F=32, H=512, W=512, cout=128) == -3 and "2 GiB" in _lib.last_error()
    assert conv(F=64, H=256, W=256, cin=128, flags=2) == -3 and mask(F=64, H=512, W=512) == -3
    assert blur(F=4096, S=512, R_=2, wb=1 << 40) == -3
    assert head(F=0) == 0 and conv(F=0) == 0 and mask(F=0) == 0 and blur(F=0) == 0


def test_masked_paste_entries_refuse_a_bad_mask():
    """through the existing check_paste with one more buffer: the plain entry's refusals come first, then the mask's"""
    from vspbfr_amd import _lib, photo as P
    S = 64
    photo, crops, Ps = _two_faces(S)
    pts = [P0.landmarks_for(1.4, 12.0, (52.0, 50.0), S)]
    for aa in (False, True):
        plan = P.FacePlan([photo], [(0, pts[0])], size=S, upscale=1, antialias=aa)
        ramp = P.default_ramp()
        p = C.c_void_p(1 << 20)
        items = plan.paste_aa_items if aa else plan.paste_items
        fwd = (plan.paste_fwd.ctypes.data_as(C.c_void_p) if plan.paste_fwd.size else None, p if plan.paste_fwd.size else None,
               plan.paste_fwd.size) if aa else ()
        entry = _lib.lib.vsp_face_paste_mask_aa_u8 if aa else _lib.lib.vsp_face_paste_mask_u8

        def call(mask=p, elems=S * S, ramp_len=int(ramp.size), crop_bytes=3 * S * S):
            return entry(p, plan.out_bytes, p, crop_bytes, plan.paste_tables.ctypes.data_as(C.c_void_p), p, plan.paste_tables.size, *fwd,
                         C.cast(items, C.c_void_p), p, plan.n, S, C.cast(plan.tiles, C.c_void_p), p, plan.ntiles,
                         plan.tile_faces.ctypes.data_as(C.c_void_p), p, plan.tile_faces.size, ramp.ctypes.data_as(C.c_void_p), p, ramp_len,
                         mask, elems, None)

        for kw, msg in ((dict(mask=None), "null pointer (mask)"), (dict(elems=S * S - 1), "need more"), (dict(mask=C.c_void_p((1 << 20) + 1)), "misaligned mask"),
                        (dict(ramp_len=0), "ramp of 1.."), (dict(crop_bytes=3 * S * S - 1), "crop outside")):
            rc = call(**kw)
            assert rc == -1 and msg in _lib.last_error(), (aa, kw, rc, _lib.last_error())
        assert call(elems=1 << 30) == -3 and "2 GiB" in _lib.last_error()


def test_parser_object_needs_no_kernel_to_be_built_and_checks_its_arguments():
    from vspbfr_amd import parse as P
    from vspbfr_amd.photo import PhotoRestorer
    net = P.FaceParser(R.make_state(8), "cpu")
    assert len(net.layers) == 44 and tuple(net.tail[0].shape) == (1, 1, 18, 2, 64, 8) and net.tail[1].numel() == 32 and net.tail[1][19:].abs().max() == 0
    assert tuple(net.layers["encoder.2.conv1"][0].shape) == (4, 2, 18, 4, 64, 8) and net.layers["decoder.3.conv2"][1].dtype == torch.float32
    assert net.chunk_of(512) == 16 and net.chunk_of(32) == 16
    net.act_limit = 3 * 64 * 64 * 256                                # the 2 GiB guard, scaled down: three faces of 64 per pass
    assert net.chunk_of(64) == 3
    with pytest.raises(ValueError, match="needs an activation"):
        net.chunk_of(128)
    for bad in (torch.zeros(1, 32, 32, 3), torch.zeros(1, 32, 48, 3, dtype=torch.uint8), torch.zeros(1, 40, 40, 3, dtype=torch.uint8),
                torch.zeros(32, 32, 3, dtype=torch.uint8), torch.zeros(1, 16, 16, 3, dtype=torch.uint8)):
        with pytest.raises(ValueError):
            net.classes(bad)
    d = net.describe(512)
    assert d == {"model": "ParseNet", "sigma": 11.0, "radius": 50, "border": 10, "nonfinite": []}
    with pytest.raises(ValueError, match="multiple of 16"):
        PhotoRestorer(None, 1, size=40, parser=net)
    assert PhotoRestorer(None, 1, size=64, parser=net).parser is net and PhotoRestorer(None, 1, size=40).parser is None
    grey = P.mask_png(torch.tensor([0, 1, 128, 255, 256], dtype=torch.int32))
    assert grey.tolist() == [0, 1, 128, 254, 255]


def test_parser_errors(tmp_path, capsys):
    """both CLIs refuse before any model is built"""
    from PIL import Image
    from vspbfr_amd import parse, restore_photos
    good, bad = tmp_path / "parse.pth", tmp_path / "bad.pth"
    torch.save(R.make_state(9), good)
    sd = R.make_state(9)
    sd.pop("body.3.conv1.conv2d.weight")
    torch.save(sd, bad)
    (tmp_path / "photos").mkdir()
    (tmp_path / "faces").mkdir()
    Image.fromarray(R.test_crops(1, 32)[0]).save(tmp_path / "faces" / "a.png")
    base = ["--photos", str(tmp_path / "photos"), "--out", str(tmp_path / "out"), "--landmarks", str(tmp_path / "none.json")]

    def refused(main, argv, msg):
        with pytest.raises(SystemExit) as e:
            main(argv)
        err = capsys.readouterr().err
        assert e.value.code == 2 and msg in err, err

    refused(restore_photos.main, base + ["--parse_weights", str(bad)], "missing keys body.3.conv1.conv2d.weight")
    refused(restore_photos.main, base + ["--parse_weights", str(tmp_path / "nope.pth")], "no such file")
    refused(restore_photos.main, base + ["--parse_weights", str(good), "--size", "40"], "multiple of 16")
    refused(restore_photos.main, base + ["--parse_weights", str(good), "--parse_sigma", "0"], "must be positive")
    refused(restore_photos.main, base + ["--parse_weights", str(good), "--parse_border", "300"], "outside 0..256")
    refused(restore_photos.main, base + ["--parse_sigma", "3"], "belong to --parse_weights")
    refused(restore_photos.main, base + ["--parse_border", "3"], "belong to --parse_weights")
    own = ["--faces", str(tmp_path / "faces"), "--out", str(tmp_path / "out")]
    refused(parse.main, own + ["--weights", str(bad)], "missing keys body.3.conv1.conv2d.weight")
    refused(parse.main, own + ["--weights", str(tmp_path / "nope.pth")], "no such file")
    refused(parse.main, own + ["--weights", str(good), "--sigma", "-1"], "must be positive")
    refused(parse.main, own + ["--weights", str(good), "--border", "17"], "outside 0..16")
    Image.fromarray(R.test_crops(1, 48)[0][:, :40]).save(tmp_path / "faces" / "b.png")
    refused(parse.main, own + ["--weights", str(good)], "square and of one size")


# --------------------------------------------------------------------------------- the conditions of the GPU class tests, on the CPU
def test_condition_of_the_tail_class_test():
    """tests/test_parse_gpu.py compares the device's classes with the float64 argmax wherever the float64 top-two gap exceeds twice the
    logit bound: at most 0.5 % of the pixels may be left out (the tied class aside), and the float32 restatement itself must agree there"""
    x, w, b = R.tail_case()
    l64, l32 = R.mask_logits(x, w, b, torch.float64).numpy(), R.mask_logits(x, w, b, torch.float32).double().numpy()
    tol, e_ref = R.logit_bound(l64, l32)
    out = R.left_out(l64, tol, drop=R.TIE[1])
    c64, c32 = R.argmax_classes(l64)[0], R.argmax_classes(l32)[0]
    print(f"tail: e_ref {e_ref:.3g} bound {tol:.3g} smallest gap {R.top_two_gap(np.delete(l64, R.TIE[1], axis=-1)).min():.3g} left out {out.mean():.4%}")
    assert out.mean() <= R.TAIL_LEFT_OUT_CAP and (c64[~out] == c32[~out]).all()


@pytest.mark.parametrize("size,faces", R.NET_CASES)
def test_condition_of_the_whole_network_class_test(size, faces):
    """the same for the whole network at the GPU test's sizes, seeds and inputs: at most 10 % left out, logits of order one (no f16
    overflow territory), and the float32 restatement agrees with float64 on every pixel that is held"""
    _, crops, l64, l32 = R.net_case(size, faces)
    tol, e_ref = R.logit_bound(l64, l32)
    out = R.left_out(l64, tol)
    c64, c32 = R.argmax_classes(l64)[0], R.argmax_classes(l32)[0]
    print(f"net S {size} F {faces}: max |logit| {np.abs(l64).max():.3g} sigma {l64.std():.3g} e_ref {e_ref:.3g} bound {tol:.3g} left out {out.mean():.4%} "
          f"classes seen {len(np.unique(c64))}")
    assert crops.shape == (faces, size, size, 3) and np.isfinite(l64).all() and np.abs(l64).max() < 8
    assert out.mean() <= R.NET_LEFT_OUT_CAP and (c64[~out] == c32[~out]).all()
    assert len(np.unique(c64)) >= 3                                  # a class map worth comparing
