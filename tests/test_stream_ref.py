"""CPU checks of tests/stream_ref.py: the restatements against torch in float64, and the teeth of the GPU file -- for each family a
deliberately wrong variant, evaluated in float32 on the inputs tests/test_stream_kernels_gpu.py uses, must be REJECTED by
stream_ref.bound.  Where a wrong variant coincides with the definition on a case (an identity resize has the same source coordinates
under both align_corners conventions; plane_mean's padded divisor is the right one at hw = 64), that case is named beside the test and
the variant must be rejected on every other one."""
import pytest
import torch
import torch.nn.functional as F

import stream_ref as R
from oracle import ops as O

F64, F32 = torch.float64, torch.float32


@pytest.fixture(autouse=True)
def _grad_on():
    """(other test modules switch autograd off for the process at import)"""
    with torch.enable_grad():
        yield


def _rejected(wrong32, ref64, ref32, what):
    with pytest.raises(AssertionError):
        R.bound(wrong32, ref64, ref32, what)


def _same64(a, b, what, tol=1e-12):
    assert a.shape == b.shape, what
    assert float((a - b).abs().max()) <= tol * max(1.0, float(b.abs().max())), (what, float((a - b).abs().max()))


# ------------------------------------------------------------------------------------------------------------------ restatements
@pytest.mark.parametrize("mat", R.SAMPLER_MATS + ["magnify"])
@pytest.mark.parametrize("shape,out_hw", R.SAMPLER_MAPS + [((1, 2, 8, 8), (64, 64))])
def test_affine_sample_is_grid_sample(shape, out_hw, mat):
    x, th, g = R.sampler_case(shape, out_hw, mat)
    x64 = x.double().requires_grad_(True)
    want = F.grid_sample(x64, F.affine_grid(th.double(), (*shape[:2], *out_hw), align_corners=False), "bilinear", "zeros", align_corners=False)
    _same64(R.affine_sample(x, th, out_hw, F64), want.detach(), f"affine_sample {mat}", 1e-9)
    (gx,) = torch.autograd.grad(want, x64, g.double())
    _same64(R.affine_sample_adjoint(g, th, shape[2:], F64), gx, f"affine_sample adjoint {mat}", 1e-9)
    if mat in ("shift3", "shift1e6"):
        assert float(want.detach().abs().max()) == 0.0 and float(R.affine_sample(x, th, out_hw, F32).abs().max()) == 0.0


@pytest.mark.parametrize("hw", R.SKIP_MAPS)
def test_skip_is_upfirdn2d(hw):
    kw = R.pointwise_case(8, 3, *hw, with_skip=True)
    _same64(R.skip(kw["up_src"], kw["up_k"], F64), O.upfirdn2d(kw["up_src"].double(), kw["up_k"].double(), up=2, pad=(2, 1)), f"skip {hw}")


@pytest.mark.parametrize("ihw,ohw", R.UPSAMPLE_SIZES + [((256, 256), (256, 256))])
def test_upsample_add_is_interpolate(ihw, ohw):
    x, y = R.upsample_case(ihw, ohw)
    _same64(R.upsample_add(x, y, F64), F.interpolate(x.double(), ohw, mode="bilinear", align_corners=True) + y.double(), f"upsample_add {ihw}->{ohw}")
    if ihw == ohw:
        assert torch.equal(R.upsample_add(x, y, F32), x + y)


@pytest.mark.parametrize("ihw,ohw", R.RESIZE_SIZES + [((5, 7), (9, 16))])
def test_resize_bilinear_is_interpolate(ihw, ohw):
    x, _ = R.upsample_case(ihw, ohw)
    _same64(R.resize_bilinear(x, ohw, F64), F.interpolate(x.double(), ohw, mode="bilinear", align_corners=False), f"resize {ihw}->{ohw}")


def test_small_restatements():
    g = torch.Generator().manual_seed(5)
    x = torch.randn(2, 3, 6, 10, generator=g)
    _same64(R.avgpool2x2(x, F64), F.avg_pool2d(x.double(), 2), "avgpool")
    _same64(R.plane_mean(x, F64), x.double().mean((2, 3)), "plane_mean")
    M, t = torch.randn(2, 3, 3, generator=g), torch.randn(2, 3, generator=g)
    want = torch.stack([(M[b].double() @ x[b].double().reshape(3, -1)).view(3, 6, 10) + t[b].double().view(3, 1, 1) for b in range(2)])
    _same64(R.color_affine(x, M, t, F64), want, "color_affine")
    from oracle import models
    q = torch.randn(2, 3, 9, 11, generator=g) * 0.8
    assert torch.equal(R.quantize_u8_nhwc(q), models.save_image_quantize(q).permute(0, 2, 3, 1))
    heads = torch.randn(4, 2, 5, generator=g)
    avg = torch.randn(4, 5, generator=g)
    want = torch.stack([heads[0] + avg[0]] + [heads[i] + heads[0] + avg[i] for i in range(1, 4)], 1)
    _same64(R.e4e_codes(heads, avg, F64), want.double(), "e4e_codes", 1e-6)
    a, b = torch.randn(2, 5, 8, generator=g), torch.randn(2, 3, generator=g)
    out = R.rows_concat(2, 4, [(a, 6, True, True), (b, 3, False, False)])
    assert out.shape == (2, 4, 9) and torch.equal(out[1, 0, :6], a[1, 3, :6]) and torch.equal(out[0, 2, 6:], b[0])
    # the two activation stages are the oracle's FusedLeakyReLU
    v, b1 = torch.randn(2, 5, 3, 3, generator=g), torch.randn(5, generator=g)
    _same64(R.fused_leaky_relu(v, b1, F64), O.fused_leaky_relu(v.double(), b1.double()), "fused_leaky_relu")


def test_bound_refuses_what_is_not_a_result():
    ref = torch.ones(3, dtype=F64)
    with pytest.raises(AssertionError):
        R.bound(torch.ones(4), ref, ref.float(), "shape")
    with pytest.raises(AssertionError):
        R.bound(torch.tensor([1.0, float("nan"), 1.0]), ref, ref.float(), "nan")
    e_ref, e_hip, _ = R.bound(ref.float(), ref, ref.float(), "exact")
    assert e_ref == 0.0 and e_hip == 0.0


# ------------------------------------------------------------------------------------------------------------------ teeth
@pytest.mark.parametrize("variant", ["parity", "noflip", "col_off"])
@pytest.mark.parametrize("hw", R.SKIP_MAPS)
def test_teeth_pointwise_skip(hw, variant):
    """every skip case of the GPU file, with and without res: a wrong tap parity, an unflipped kernel, a source column off by one"""
    for cin in R.SKIP_CIN:
        for cout in R.SKIP_COUT:
            for ops in ((), ("res",)):
                kw = R.pointwise_case(cin, cout, *hw, operands=ops, with_skip=True)
                _rejected(R.pointwise(**kw, dtype=F32, variant=variant), R.pointwise(**kw, dtype=F64), R.pointwise(**kw, dtype=F32),
                          f"skip {variant} {cin}->{cout} {hw} {ops}")


@pytest.mark.parametrize("variant", ["drop_last", "style0"])
@pytest.mark.parametrize("cout", R.FEW_OUT_COUT)
def test_teeth_pointwise_few_out_channels(cout, variant):
    """style0 needs a style scale: the operand sets without one are skipped for it, nothing else is"""
    for cin in R.FEW_OUT_CIN:
        for hw in R.FEW_OUT_MAPS:
            for name, ops in R.OPERAND_SETS.items():
                if variant == "style0" and "in_scale" not in ops:
                    continue
                kw = R.pointwise_case(cin, cout, *hw, operands=ops)
                _rejected(R.pointwise(**kw, dtype=F32, variant=variant), R.pointwise(**kw, dtype=F64), R.pointwise(**kw, dtype=F32),
                          f"few-out {variant} {cin}->{cout} {hw} {name}")


@pytest.mark.parametrize("variant", ["drop_last", "style0"])
@pytest.mark.parametrize("cin", R.FEW_IN_CIN)
def test_teeth_pointwise_few_in_channels(cin, variant):
    for cout in R.FEW_IN_COUT:
        for name, acts in R.ACT_SETS.items():
            kw = R.pointwise_case(cin, cout, 5, 9, operands=("in_scale", "ch_bias") + acts)
            _rejected(R.pointwise(**kw, dtype=F32, variant=variant), R.pointwise(**kw, dtype=F64), R.pointwise(**kw, dtype=F32),
                      f"few-in {variant} {cin}->{cout} {name}")


# the matrices on which the wrong sampler differs from the definition at all: align_corners=True coincides with False for the identity
# and the zero matrix at equal sizes and wherever everything is outside; a tap lands on column IW only under the half-pixel shift
# (+x for image 0) and the rotation
SAMPLER_BITES = {"align_corners": [(0, "identity"), (0, "half_shift"), (0, "rot45"), (1, "half_shift"), (1, "rot45")],
                 "clamp_iw": [(0, "half_shift"), (1, "half_shift"), (0, "rot45"), (1, "rot45")]}


@pytest.mark.parametrize("variant", list(SAMPLER_BITES))
def test_teeth_sampler(variant):
    for m, mat in SAMPLER_BITES[variant]:
        shape, out_hw = R.SAMPLER_MAPS[m]
        x, th, _ = R.sampler_case(shape, out_hw, mat)
        _rejected(R.affine_sample(x, th, out_hw, F32, variant), R.affine_sample(x, th, out_hw, F64), R.affine_sample(x, th, out_hw, F32),
                  f"sampler {variant} {mat} map {m}")


def test_teeth_upsample_add():
    """align_corners=False coordinates: the same as True whenever an axis keeps its size or has one input pixel -- (1,1)->(4,5),
    (1,6)->(3,6), (5,1)->(5,4) and (3,4)->(3,4) cannot tell the two apart, (3,4)->(1,1) and (5,7)->(9,16) must"""
    bites = 0
    for ihw, ohw in R.UPSAMPLE_SIZES:
        x, y = R.upsample_case(ihw, ohw)
        wrong, r64, r32 = R.upsample_add(x, y, F32, "align_false"), R.upsample_add(x, y, F64), R.upsample_add(x, y, F32)
        if (ihw, ohw) in (((3, 4), (1, 1)), ((5, 7), (9, 16))):
            _rejected(wrong, r64, r32, f"upsample_add align_false {ihw}->{ohw}")
            bites += 1
        else:
            R.bound(wrong, r64, r32, f"upsample_add align_false {ihw}->{ohw} (coincides)")
    assert bites == 2


@pytest.mark.parametrize("offset", [0.0, 1e3])
@pytest.mark.parametrize("planes", [1, 5])
def test_teeth_plane_mean(planes, offset):
    for hw in R.PLANE_HW:
        if hw == 64:       # 64 ceil(64 / 64) = 64: the padded divisor is the right one
            continue
        x = R.plane_mean_case(hw, planes, offset)
        _rejected(R.plane_mean(x, F32, "wave_padded"), R.plane_mean(x, F64), R.plane_mean(x, F32), f"plane_mean padded hw={hw} x{planes} +{offset}")


# ------------------------------------------------------------------------------------------------------------------ orders of summation
# Three families print e_hip / e_ref above 4 on the GPU and pass through the additive 2e-6 max |ref| term.  Each time the cause is the
# ORDER of a float32 sum, not a defect: the same order evaluated in float32 here, on the same inputs, stays within the same bound.
@pytest.mark.parametrize("cin,cout", [c for c in R.LDS_LIMIT_CASES if c[1] <= 4])
def test_order_pointwise_serial_channel_chain(cin, cout):
    """4096 / 16384 input channels: a thread adds them in one chain, torch's einsum in blocks"""
    kw = R.pointwise_case(cin, cout, 4, 4, operands=("in_scale", "ch_bias"), B=1)
    R.bound(R.pointwise_serial(**kw), R.pointwise(**kw, dtype=F64), R.pointwise(**kw, dtype=F32), f"serial chain {cin}->{cout}")


@pytest.mark.parametrize("planes", [1, 5])
def test_order_plane_mean_wave(planes):
    """lane-strided partial sums + butterfly: torch's sum of 65 numbers happens to be exact to 5e-10, one rounding of the result is 6e-8"""
    for hw in R.PLANE_HW:
        for offset in (0.0, 1e3):
            x = R.plane_mean_case(hw, planes, offset)
            R.bound(R.plane_mean_wave(x), R.plane_mean(x, F64), R.plane_mean(x, F32), f"wave order hw={hw} x{planes} +{offset:g}")


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_order_adjoint_shuffled_scatter(seed):
    """the magnifying adjoint: each of the central 3 x 3 input pixels collects ~1800 additions, in whatever order the atomics land"""
    shape, out_hw = (1, 2, 8, 8), (64, 64)
    x, th, g = R.sampler_case(shape, out_hw, "magnify")
    r64 = R.affine_sample_adjoint(g, th, shape[2:], F64)
    _same64(R.affine_sample_adjoint_scatter(g, th, shape[2:], F64, seed), r64, "scatter adjoint", 1e-9)
    R.bound(R.affine_sample_adjoint_scatter(g, th, shape[2:], F32, seed), r64, R.affine_sample_adjoint(g, th, shape[2:], F32), f"shuffled scatter {seed}")
