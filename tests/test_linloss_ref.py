"""CPU checks of tests/linloss_ref.py: the restatements against torch in float64, the teeth of tests/test_linloss_gpu.py -- for each
family a deliberately wrong variant, evaluated in float32 (or exactly, for the selections) on the inputs the GPU module uses, must be
REJECTED by stream_ref.bound / by the exact comparison -- and the test_order_* restatements: the kernels' summation orders evaluated in
float32 on the GPU module's inputs, which must lie within the bound.  The one recorded ratio e_hip / e_ref beyond 4 is the LPIPS
gradient at a pixel of tiny norm (test_order_lpips_backward reproduces its 5.27 and 7.25 to the digit); the orders of the tiled GEMM
and of the gemv are evaluated on their deepest-K cases all the same (recorded ratios 2.76 and 0.57).  Where a wrong variant coincides
with the definition on a case (a K that is a multiple of 16 has no tail to drop), the test names the cases it bites on."""
import pytest
import torch
import torch.nn.functional as F

import linloss_ref as R
from stream_ref import bound

F64, F32 = torch.float64, torch.float32


@pytest.fixture(autouse=True)
def _grad_on():
    """(other test modules switch autograd off for the process at import)"""
    with torch.enable_grad():
        yield


def _rejected(wrong32, ref64, ref32, what):
    with pytest.raises(AssertionError):
        bound(wrong32, ref64, ref32, what)


def _same64(a, b, what, tol=1e-12):
    assert a.shape == b.shape, what
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), (what, float((a - b).abs().max()))


# ------------------------------------------------------------------------------------------------------------------ small GEMM
def _torch_gemm(kw):
    a, b = kw["a"].double(), kw["b"].double()
    v = torch.matmul(a, b.transpose(-1, -2)) * kw["alpha"]
    N, zs = b.shape[-2], kw.get("bias_zs", 0)
    bias = kw["bias"].double() * kw["bias_scale"]
    if a.dim() == 3:
        v = v + torch.stack([bias[z * zs:z * zs + N] for z in range(a.shape[0])]).unsqueeze(1)
    else:
        v = F.linear(a, b * kw["alpha"], bias[:N])
    return F.leaky_relu(v, 0.2) * R.SQRT2 if kw["act"] == 1 else torch.sigmoid(v)


@pytest.mark.parametrize("name", list(R.GEMM_CASES))
def test_gemm_is_linear(name):
    kw = R.gemm_case(name)
    _same64(R.gemm_nt(**kw, dtype=F64), _torch_gemm(kw), name)


@pytest.mark.parametrize("variant", ["drop_k16", "drop_k4", "drop_wave", "bias_unscaled", "bias_zs0"])
def test_gemm_teeth(variant):
    """a vector loop without its K % 16 (K % 4) tail on every case that has one; a wave's k-steps lost wherever K >= 32; an unscaled
    bias everywhere; bias_zs ignored on the batched cases"""
    bites = 0
    for name, (Z, M, N, K, _kind, _kw) in R.GEMM_CASES.items():
        if {"drop_k16": K % 16 == 0, "drop_k4": K % 4 == 0, "drop_wave": K < 32, "bias_unscaled": False, "bias_zs0": Z < 2}[variant]:
            continue
        kw = R.gemm_case(name)
        _rejected(R.gemm_nt(**kw, dtype=F32, variant=variant), R.gemm_nt(**kw, dtype=F64), R.gemm_nt(**kw, dtype=F32), f"{name} {variant}")
        bites += 1
    assert bites >= {"drop_k16": 5, "drop_k4": 2, "drop_wave": 10, "bias_unscaled": len(R.GEMM_CASES), "bias_zs0": 3}[variant]


def test_gemm_case_forms():
    """the storage of each case is what its comment says: which entry form it reaches follows from pitches and offsets alone"""
    vec = {n: R.gemm_is_vec(R.gemm_case(n)) for n in R.GEMM_CASES}
    assert not vec["offset1_12x21x64"] and not vec["batched_strided_3x18x37x22"]
    assert all(v for n, v in vec.items() if n not in ("offset1_12x21x64", "batched_strided_3x18x37x22", "k0_bias_7x19x0"))
    kw = R.gemm_case("vec_masked_36x40x513")
    assert kw["a"].stride() == (516, 1) and kw["b"].stride() == (516, 1) and kw["a"].shape == (36, 513) and kw["b"].shape == (40, 513)
    assert R.gemm_case("offset1_12x21x64")["a"].storage_offset() == 1
    assert R.gemm_case("batched_strided_3x18x37x22")["a"].stride() == (22 * 18, 1, 18)
    for name, (Z, M, N, K, _k, _kw) in R.WIDE_CASES.items():
        assert M >= 1024
    for name, (Z, M, N, K, _k, _kw) in R.GEMV_OFF_CASES.items():
        assert Z == 0 and M <= 16 and K >= 512 and K % 256 == 0         # the entry's condition for the few-row form


def test_order_restatements_are_sums():
    """the two order functions add every product exactly once: in float64-sized error of the plain sum"""
    g = torch.Generator().manual_seed(3)
    for K, vec in ((20, True), (76, True), (513, True), (22, False), (64, False)):
        a, b = torch.randn(5, K, generator=g), torch.randn(7, K, generator=g)
        assert float((R.gemm_tiled_order(a, b, vec).double() - a.double() @ b.double().t()).abs().max()) < 1e-4
    a, b = torch.randn(9, 512, generator=g), torch.randn(6, 512, generator=g)
    assert float((R.gemv_order(a, b).double() - a.double() @ b.double().t()).abs().max()) < 1e-4
    v = torch.randn(3, 64, generator=g)
    assert float((R.wave_tree(v).double() - v.double().sum(-1)).abs().max()) < 1e-5


def _order_case(name, order):
    kw = R.gemm_case(name)
    raw = order(kw["a"], kw["b"])
    v = raw * torch.tensor(kw["alpha"], dtype=F32) + kw["bias"][:raw.shape[1]] * torch.tensor(kw["bias_scale"], dtype=F32)
    got = R.epilogue(v, kw["act"], torch.tensor(0.2, dtype=F32), torch.tensor(R.SQRT2, dtype=F32))
    assert got.dtype == F32
    return bound(got, R.gemm_nt(**kw, dtype=F64), R.gemm_nt(**kw, dtype=F32), f"order {name}")


@pytest.mark.parametrize("name", list(R.GEMV_OFF_CASES))
def test_order_tiled_gemm_deep_k(name):
    """gemm_nt_kernel<true,1> on few rows against K = 1024 / 4096: four serial chains of K / 4 products each, against torch's blocked
    sum -- the order alone, in float32 on the CPU, is within the bound"""
    _order_case(name, lambda a, b: R.gemm_tiled_order(a, b, True))


def test_order_gemv():
    """gemv_rows_kernel / style_mods_kernel: a lane chain of K / 64 fmaf, then the DPP tree"""
    _order_case("gemv_9x35x512", R.gemv_order)
    for K in R.STYLE_K:
        lat, layers = R.style_case(K, 9)
        for layer, (cin, _co, _d, _b, row) in zip(layers, R.STYLE_LAYERS):
            w, bias, _wsq, alpha, bs, _ws = layer
            got = R.gemv_order(lat[:, row].contiguous(), w) * torch.tensor(alpha, dtype=F32)
            if bias is not None:
                got = got + bias * torch.tensor(bs, dtype=F32)
            bound(got, R.style_mod(lat, layer, row, F64), R.style_mod(lat, layer, row, F32), f"order style mod K={K} cin={cin}")


# ------------------------------------------------------------------------------------------------------------------ style plan
@pytest.mark.parametrize("K", R.STYLE_K)
def test_style_restatement_and_teeth(K):
    lat, layers = R.style_case(K, 9)
    for layer, (cin, cout, demod, has_bias, row) in zip(layers, R.STYLE_LAYERS):
        w, bias, wsq, alpha, bs, ws = layer
        m64 = R.style_mod(lat, layer, row, F64)
        _same64(m64, F.linear(lat[:, row].double(), w.double() * alpha, None if bias is None else bias.double() * bs), f"mod {cin}")
        m32 = R.style_mod(lat, layer, row, F32)
        if has_bias:
            _rejected(R.style_mod(lat, layer, row, F32, "bias_unscaled"), m64, m32, f"style bias unscaled cin={cin}")
        other = (row + 1) % R.STYLE_ROWS                                      # the row of another layer's style
        _rejected(R.style_mod(lat, layer, other, F32), m64, m32, f"style wrong row cin={cin}")
        if demod:
            d64 = R.demod_coefs(m64, wsq, ws, 1e-8, F64)
            _same64(d64, torch.rsqrt(ws * ws * (m64 ** 2) @ wsq.double().t() + 1e-8), f"demod {cin}")
            _rejected(R.demod_coefs(m32, wsq, 1.0, 1e-8, F32), d64, R.demod_coefs(m32, wsq, ws, 1e-8, F32), f"style wscale cin={cin}")


# ------------------------------------------------------------------------------------------------------------------ max-pool
def _torch_pool(x, dy, k, s, p):
    x64 = x.double().requires_grad_(True)
    y = F.max_pool2d(x64, k, s, p)
    (gx,) = torch.autograd.grad(y, x64, dy.double())
    return y.detach(), gx


def _same_with_nan(a, b):
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, 12345.0), torch.nan_to_num(b, 12345.0))


@pytest.mark.parametrize("k,s,p", R.POOL_GEOMETRIES + [(2, 2, 0), (3, 2, 1)])
@pytest.mark.parametrize("hw", R.POOL_MAPS + [(9, 8), (8, 8)])
def test_maxpool_is_max_pool2d(k, s, p, hw):
    x, dy = R.pool_case((2, 3, *hw), k, s, p)
    y, gx = _torch_pool(x, dy, k, s, p)
    for dt in (F64, F32):                                                     # (selections and exact sums: the same in both)
        assert torch.equal(R.maxpool_argmax(x, k, s, p, dt)[0].double(), y)
        assert torch.equal(R.maxpool_bwd(dy, x, k, s, p, dt).double(), gx)


@pytest.mark.parametrize("geometry", [(2, 2, 0), (3, 2, 1)])
@pytest.mark.parametrize("kind", R.POOL_PLANTS)
def test_maxpool_planted_values_follow_aten(kind, geometry):
    """NaN, +-inf: the restatement's output (NaN positions included) and its full gradient are CPU torch's, in float64 and float32"""
    x, dy, (k, s, p) = R.pool_planted(kind, geometry)
    for dt in (F64, F32):
        xt = x.to(dt).requires_grad_(True)
        y = F.max_pool2d(xt, k, s, p)
        (gx,) = torch.autograd.grad(y, xt, dy.to(dt))
        assert _same_with_nan(R.maxpool_argmax(x, k, s, p, dt)[0], y.detach()), kind
        assert torch.equal(R.maxpool_bwd(dy, x, k, s, p, dt), gx), kind
    if kind == "two_nan_diag" and geometry == (2, 2, 0):
        gx = R.maxpool_bwd(dy, x, k, s, p)
        assert float(gx[0, 0, 3, 4]) == float(dy[0, 0, 1, 2]) != 0 and float(gx[0, 0, 2, 5]) == 0      # element (1, 0) of the window, not (0, 1)


def test_maxpool_teeth():
    """last-maximum ties: on every quantised map with k >= 2; the first-NaN rule: on every plant with two or more NaNs; the window range
    off by one: at k < s"""
    for k, s, p in R.POOL_GEOMETRIES + [(2, 2, 0), (3, 2, 1)]:
        for hw in R.POOL_MAPS:
            x, dy = R.pool_case((2, 5, *hw), k, s, p)
            ref = R.maxpool_bwd(dy, x, k, s, p)
            if k >= 2:
                assert not torch.equal(R.maxpool_bwd(dy, x, k, s, p, variant="last_tie"), ref), (k, s, p, hw)
                assert torch.equal(R.maxpool_argmax(x, k, s, p, variant="last_tie")[0], R.maxpool_argmax(x, k, s, p)[0])
            if k < s:
                assert not torch.equal(R.maxpool_argmax(x, k, s, p, variant="range_off")[0], R.maxpool_argmax(x, k, s, p)[0])
                assert not torch.equal(R.maxpool_bwd(dy, x, k, s, p, variant="range_off"), ref)
    for geometry in ((2, 2, 0), (3, 2, 1)):
        for kind in R.POOL_PLANTS:
            x, dy, (k, s, p) = R.pool_planted(kind, geometry)
            differs = not torch.equal(R.maxpool_bwd(dy, x, k, s, p, variant="first_nan"), R.maxpool_bwd(dy, x, k, s, p))
            assert differs == (kind in ("two_nan_diag", "two_nan_row", "three_nan")), (kind, geometry)
            assert _same_with_nan(R.maxpool_argmax(x, k, s, p, variant="first_nan")[0], R.maxpool_argmax(x, k, s, p)[0])


def test_maxpool_second_pass_sizes():
    """the large shapes exceed one pass of the capped grid (256 threads x kMaxStreamBlocks) in the unit each kernel strides over"""
    B, Cc, H, W = R.POOL_BIG_2X2
    assert H % 2 == 0 and W % 4 == 0 and B * Cc * (H // 2) * (W // 4) > R.STREAM_ELEMS
    B, Cc, H, W = R.POOL_BIG_GENERIC
    assert H % 2 == 1 and B * Cc * (H // 2) * (W // 2) > R.STREAM_ELEMS and B * Cc * H * W > R.STREAM_ELEMS


# ------------------------------------------------------------------------------------------------------------------ LPIPS layer
def _torch_lpips(a, b, w_):
    """the formula of tests/test_hip_ops.py::test_lpips_layer_forward_backward"""
    na = a / (torch.sqrt((a ** 2).sum(1, keepdim=True)) + 1e-10)
    nb = b / (torch.sqrt((b ** 2).sum(1, keepdim=True)) + 1e-10)
    return ((na - nb) ** 2 * w_.view(1, -1, 1)).sum(1).mean(1)


def _lpips_small_cases():
    return [(C, hw) for C in R.LPIPS_REG_C for hw in R.lpips_small_hw(C)] + R.LPIPS_GENERIC


@pytest.mark.parametrize("C,HW", _lpips_small_cases())
def test_lpips_is_the_formula_and_has_teeth(C, HW):
    f0, f1, w, gout = R.lpips_case(C, HW)
    b = f1.double().requires_grad_(True)
    r = _torch_lpips(f0.double(), b, w.double())
    _same64(R.lpips_layer(f0, f1, w, F64), r.detach(), f"lpips {C} {HW}")
    (gb,) = torch.autograd.grad(r, b, gout.double())
    g64, g32 = R.lpips_layer_bwd(gout, f0, f1, w, F64), R.lpips_layer_bwd(gout, f0, f1, w, F32)
    finite = torch.isfinite(gb)                            # autograd: sqrt'(0) * 0 = NaN at an all-zero pixel of f1; the definition drops the term
    assert bool(finite.permute(0, 2, 1)[f1.abs().sum(1) > 0].all())
    gb0 = torch.where(finite, gb, g64)
    assert float(((g64 - gb0).abs() / gb0.abs().clamp_min(1.0)).max()) <= 1e-12
    assert bool(torch.isfinite(g64).all()) and bool(torch.isfinite(g32).all())
    # teeth, per group of pixels (the groups differ in scale by 1e5 and 1e10)
    groups = dict(R.lpips_pixel_groups(f1))
    assert set(groups) == {"ordinary", "tiny", "zero-f1"} or HW == 1
    no_k2 = R.lpips_layer_bwd(gout, f0, f1, w, F32, "no_k2")
    eps_in = R.lpips_layer_bwd(gout, f0, f1, w, F32, "eps_in_sqrt")
    if "ordinary" in groups:
        m = groups["ordinary"]
        _rejected(R.lpips_grouped(no_k2, m), R.lpips_grouped(g64, m), R.lpips_grouped(g32, m), f"lpips bwd no k2 {C} {HW}")
    m = groups["tiny"]
    _rejected(R.lpips_grouped(eps_in, m), R.lpips_grouped(g64, m), R.lpips_grouped(g32, m), f"lpips bwd eps in sqrt {C} {HW}")
    _rejected(R.lpips_layer(f0, f1, w, F32, "eps_in_sqrt"), R.lpips_layer(f0, f1, w, F64), R.lpips_layer(f0, f1, w, F32), f"lpips eps in sqrt {C} {HW}")


@pytest.mark.parametrize("C,HW", _lpips_small_cases())
def test_order_lpips_backward(C, HW):
    """The one LPIPS figure beyond 4 e_ref on the GPU is the gradient at the planted pixel of tiny norm (5.3 at C = 64, HW = 64; 7.3 at
    C = 192, HW = 257): there g r and f1 k2 are ~1e5 each and cancel to the tangential part, so the last bits of |f1|^2 and of the dot
    product show -- and the kernels add those as fmaf chains over the channels in turn, torch in blocks.  The chains alone, in float32
    on the CPU, are within the bound in every group of pixels."""
    f0, f1, w, gout = R.lpips_case(C, HW)
    got = R.lpips_bwd_order(gout, f0, f1, w)
    g64, g32 = R.lpips_layer_bwd(gout, f0, f1, w, F64), R.lpips_layer_bwd(gout, f0, f1, w, F32)
    for name, m in R.lpips_pixel_groups(f1):
        bound(R.lpips_grouped(got, m), R.lpips_grouped(g64, m), R.lpips_grouped(g32, m), f"order lpips bwd C={C} HW={HW} [{name}]")


def test_lpips_sizes_follow_the_launch_code():
    assert [R.lpips_wave_pixels(C) for C in (64, 128, 256)] == [64, 32, 16] and [R.lpips_block_pixels(C) for C in (64, 128, 256, 3)] == [256, 128, 64, 256]
    assert R.lpips_second_pass_hw(256, "fwd") == 2048 * 64 + 70 and R.lpips_second_pass_hw(256, "bwd") == 4096 * 64 + 70
    assert R.lpips_second_pass_hw(3, "fwd") == 1024 * 256 + 70 and R.lpips_second_pass_hw(3, "bwd") == 4096 * 256 + 70
    for C, direction in R.LPIPS_SECOND_PASS:
        HW = R.lpips_second_pass_hw(C, direction)
        idx, first = R.lpips_subset(HW, C, direction)
        assert first < HW and set(range(first, HW)) <= set(idx.tolist()) and set(range(256)) <= set(idx.tolist()) and len(idx) > 4000
        assert all(q % HW in set(idx.tolist()) for px in R.LPIPS_BIG_ZEROS.values() for q in px)
    # a subset evaluated with hw passed explicitly is the full evaluation at those pixels
    f0, f1, w, gout = R.lpips_case(64, 300)
    idx = torch.tensor([0, 5, 100, 150, 299])
    sub, full = R.lpips_layer_bwd(gout, f0[:, :, idx], f1[:, :, idx], w, F64, hw=300), R.lpips_layer_bwd(gout, f0, f1, w, F64)[:, :, idx]
    assert float(((sub - full).abs() / full.abs().clamp_min(1e-3)).max()) <= 1e-12       # (torch's channel sum depends on the layout in the last bits)


# ------------------------------------------------------------------------------------------------------------------ resize adjoint
@pytest.mark.parametrize("ihw,ohw", R.RESIZE_ADJ_SIZES + [R.RESIZE_ADJ_BIG[:2]])
def test_resize_adjoint_is_interpolate(ihw, ohw):
    """with float64 taps the scatter is autograd of F.interpolate to 1e-12; the float32 taps (the kernels' own) move a weight by less
    than 1e-5; forward and adjoint restatements are adjoint to each other with either taps"""
    x, g = R.resize_case(ihw, ohw)
    x64 = x.double().requires_grad_(True)
    y = F.interpolate(x64, ohw, mode="bilinear", align_corners=False)
    (gx,) = torch.autograd.grad(y, x64, g.double())
    _same64(R.resize_bilinear(x, ohw, F64, tap_dtype=F64), y.detach(), f"resize {ihw}->{ohw}")
    _same64(R.resize_bilinear_bwd(g, ihw, F64, tap_dtype=F64), gx, f"resize adjoint {ihw}->{ohw}")
    a64 = R.resize_bilinear_bwd(g, ihw, F64)
    assert float((a64 - gx).abs().max()) <= 1e-5 * float(g.abs().sum((2, 3)).max())
    lhs, rhs = float((R.resize_bilinear(x, ohw, F64) * g.double()).sum()), float((x.double() * a64).sum())
    assert abs(lhs - rhs) <= 1e-12 * float(x.abs().sum()) * float(g.abs().max())


def test_resize_taps_are_the_fused_float32_ones():
    """a size at which the contracted (one rounding) and the two-rounding float32 coordinate differ: the restatement takes the fused one"""
    differ = 0
    for I, Osz in ((20, 45), (31, 17), (40, 300), (50, 300)):
        s = torch.tensor(I, dtype=F32) / torch.tensor(Osz, dtype=F32)
        o = torch.arange(Osz, dtype=F32)
        two = ((o + 0.5) * s - 0.5).clamp_min(0)
        i0, _i1, l1 = R.resize_taps(I, Osz)
        fused = i0.float() + l1
        exact = ((o.double() + 0.5) * s.double() - 0.5).clamp_min(0)
        assert bool(((fused.double() - exact).abs() <= (two.double() - exact).abs()).all())
        differ += int((fused != two).sum())
    assert differ > 0


@pytest.mark.parametrize("ihw,ohw", R.RESIZE_ADJ_SIZES)
def test_resize_adjoint_teeth(ihw, ohw):
    """align-corners taps are rejected wherever the two conventions differ.  They are the same operator on an axis of one input pixel
    and on an axis of equal sizes -- (1, 1) -> (3, 2) and (1, 6) -> (4, 6) consist of such axes only, the other four cases bite (with
    one OUTPUT pixel align-corners reads input 0, the definition the centre)."""
    _x, g = R.resize_case(ihw, ohw)
    wrong = R.resize_bilinear_bwd(g, ihw, F32, variant="align_corners")
    if all(i == 1 or i == o for i, o in zip(ihw, ohw)):
        assert (ihw, ohw) in (((1, 1), (3, 2)), ((1, 6), (4, 6)))
        bound(wrong, R.resize_bilinear_bwd(g, ihw, F64), R.resize_bilinear_bwd(g, ihw, F32), f"resize adjoint align_corners {ihw}->{ohw} (same operator)")
    else:
        _rejected(wrong, R.resize_bilinear_bwd(g, ihw, F64), R.resize_bilinear_bwd(g, ihw, F32), f"resize adjoint align_corners {ihw}->{ohw}")
