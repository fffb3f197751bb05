"""GPU checks of the HBM-stream kernels -- csrc/pointwise.hip, csrc/augment.hip and the helpers in the second half of csrc/rowops.hip --
against the float64 restatements of tests/stream_ref.py, at the shapes that reach every compiled form and loop body.

Bound (stream_ref.bound, the rule of tests/test_tacc_kernels.py): max |HIP - float64| <= 4 e_ref + 2e-6 max |float64| with e_ref the
error of the same restatement run in float32 on the CPU; integer and copy operations are exact.  Every comparison prints its
e_ref / e_hip / ratio line under -s; one full run is kept in profiles/stream_kernels_gputest.log.  tests/test_stream_ref.py shows on
the CPU that wrong variants of each family miss this bound on these very inputs.

Outputs that the hip_ops wrappers allocate cannot carry a sentinel; wherever a test calls a C entry with a buffer of its own (the ragged
bf16 planes, the LDS limits, the refusals) GUARD elements behind the output are checked to be untouched.

Worst ratio e_hip / e_ref per family in the recorded run (the bound is 4 e_ref + the additive term):
    pointwise few outputs 3.13 (24 -> 1 on 5x9), its skip 1.95, bf16 x 2.71; few inputs 1.57, bf16 y 0.18 beyond the half unit;
    affine_sample forward 1.10, color_affine 1.00, film 1.50, axpby_idx / add3 / scale_add / upsample_add / e4e_codes 1.00,
    avgpool2x2 1.17, resize_bilinear 0.99, demod_coefs 1.60.
Three families print more than 4 and pass through the 2e-6 max |ref| term; each time it is the ORDER of a float32 sum, and
tests/test_stream_ref.py (test_order_*) evaluates that order in float32 on the CPU, on these inputs, and finds it within the bound:
    pointwise at the LDS limit 5.31 (4096 -> 4: e_hip 2.4e-6 on |y| <= 2): a thread adds its 4096 channels in one fmaf chain, torch's
        einsum in blocks (the CPU chain: 5.02);
    plane_mean 131 (hw = 65, one plane: e_hip 6.0e-8 = one rounding of a mean of 0.5, torch's own sum of those 65 numbers happens to
        be exact to 5e-10; the lane-strided sum + butterfly gives the identical 6.006e-08 on the CPU), every other case <= 3.6;
    affine_sample adjoint 2.5 ... 6.1 from run to run, 2.54 in the recorded one (the magnifying case: ~1800 atomic additions per
        central input pixel in the order they land; shuffled float32 scatters on the CPU read 2.2 ... 3.4), every other adjoint
        case <= 1.5."""
import math

import pytest
import torch

import stream_ref as R
from oracle import models as OM

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
GUARD = 1024                       # sentinel elements behind every output buffer a test allocates itself
SENTINEL = 7.0
BIG = (2, 5, 256, 256)             # 655 360 elements > 524 288 = one pass of the capped grid: the stride loop runs a second time
assert 2 * 5 * 256 * 256 > R.STREAM_ELEMS


@pytest.fixture(autouse=True)
def _grad_on():
    """(other test modules switch autograd off for the process at import)"""
    with torch.enable_grad():
        yield


def dev(t):
    return None if t is None else t.to(DEV)


@pytest.fixture(scope="module")
def H():
    from vspbfr_amd import hip_ops
    return hip_ops


def _g(seed):
    return torch.Generator().manual_seed(seed)


def _launch_kw(kw, x=None):
    """the keyword arguments of stream_ref.pointwise as device operands of hip_ops.pointwise"""
    d = {("up_kernel" if k == "up_k" else k): dev(v) for k, v in kw.items() if k not in ("x", "w")}
    return (dev(kw["x"]) if x is None else x, dev(kw["w"])), d


def _guarded(numel, dtype):
    buf = torch.full((numel + GUARD,), SENTINEL, dtype=dtype, device=DEV)
    return buf, buf[:numel]


def _guard_intact(buf, numel, what):
    torch.cuda.synchronize()
    assert bool((buf[numel:] == SENTINEL).all()), f"{what}: wrote behind its output"


def _pointwise_entry(H, kw, x=None, y_dtype=F32, bf16_entry=False):
    """vsp_pointwise_f32 / _bf16 on an output of the test's own with a sentinel strip: (return code, output, buffer)"""
    from vspbfr_amd._lib import lib
    (xd, wd), d = _launch_kw(kw, x)
    B, Cin, Hh, Ww = xd.shape
    Cout = wd.shape[0]
    n = B * Cout * Hh * Ww
    buf, y = _guarded(n, y_dtype)
    fn = lib.vsp_pointwise_bf16 if bf16_entry else lib.vsp_pointwise_f32
    p = H._ptr
    rc = fn(p(y), p(xd), p(wd), p(d.get("in_scale")), p(d.get("ch_bias")), p(d.get("bias1")), 1 if "bias1" in d else 0, p(d.get("bias2")),
            1 if "bias2" in d else 0, p(d.get("res")), p(d.get("up_src")), p(d.get("up_kernel")), Ww, B, Cin, Cout, Hh * Ww, H._stream())
    return rc, y.view(B, Cout, Hh, Ww), buf


# ================================================================================================== pointwise, few outputs
@pytest.mark.parametrize("cin", R.FEW_OUT_CIN)    # 1, 7: slow channel loop, one partial group; 8 / 24: fast loop with one / three groups
#                                                   (on the maps with HW % 4 == 0); 12: slow loop, one whole group + a partial one
@pytest.mark.parametrize("cout", R.FEW_OUT_COUT)  # pw_few_out_kernel<1>, <2>, <3>, <4>
def test_pointwise_few_outputs(H, cout, cin):
    """B = 2 so that the per-image style scale matters.  Maps: 4x4 (one quad row per thread), 5x9 (HW % 4 == 1: planes off 16-byte
    alignment, load1 / store1 tail), 34x36 (HW = 1224: a second block, partly empty).  Operand sets: none, in_scale, ch_bias + res, all."""
    for hw in R.FEW_OUT_MAPS:
        for name, ops in R.OPERAND_SETS.items():
            kw = R.pointwise_case(cin, cout, *hw, operands=ops)
            args, d = _launch_kw(kw)
            R.bound(H.pointwise(*args, **d), R.pointwise(**kw, dtype=F64), R.pointwise(**kw, dtype=F32), f"few-out {cin}->{cout} {hw} {name}")


@pytest.mark.parametrize("hw", R.SKIP_MAPS)       # 2x2: half map 1x1, every outside tap; 4x4, 8x12: in-row quad body (W % 4 == 0);
#                                                   6x6, 6x10, 10x14: per-pixel body (W % 4 == 2)
def test_pointwise_few_outputs_skip(H, hw):
    """the FIR-upsampled skip inside the kernel, with a 4x4 kernel that is neither symmetric nor separable: Cin 8 (fast channel loop where
    HW % 4 == 0) and 12 (slow loop in front of the quad body), Cout 1, 3, 4, each once with res as well (r += a on a loaded residual)"""
    for cin in R.SKIP_CIN:
        for cout in R.SKIP_COUT:
            for ops in (("in_scale", "ch_bias"), ("in_scale", "ch_bias", "res")):
                kw = R.pointwise_case(cin, cout, *hw, operands=ops, with_skip=True)
                args, d = _launch_kw(kw)
                R.bound(H.pointwise(*args, **d), R.pointwise(**kw, dtype=F64), R.pointwise(**kw, dtype=F32),
                        f"skip {cin}->{cout} {hw} {'res' if 'res' in ops else 'nores'}")


@pytest.mark.parametrize("hw,with_skip", [((5, 9), False),     # ragged planes: 2-byte aligned, 8-byte load4 at halfword alignment, load1 tail
                                          ((34, 36), False),    # two blocks
                                          ((8, 12), True)])     # quad skip body behind bf16 loads
def test_pointwise_few_outputs_bf16_wide_side(H, hw, with_skip):
    """x in bf16 (pw_few_out_kernel<CO, bf16_t>): float64 on the bf16-rounded x, and bit-identical to the fp32 launch on the same values"""
    for cin in (7, 8, 24):
        for cout in (1, 3, 4):
            kw = R.pointwise_case(cin, cout, *hw, operands=("in_scale", "ch_bias", "res"), with_skip=with_skip)
            kw["x"] = kw["x"].to(BF).float()                    # the values the kernel sees
            (x32, wd), d = _launch_kw(kw)
            xb = x32.to(BF)
            got = H.pointwise(xb, wd, **d)
            assert got.dtype == F32 and torch.equal(got, H.pointwise(x32, wd, **d))
            R.bound(got, R.pointwise(**kw, dtype=F64), R.pointwise(**kw, dtype=F32), f"few-out bf16 x {cin}->{cout} {hw}")
            rc, y, buf = _pointwise_entry(H, kw, x=xb, bf16_entry=True)
            assert rc == 0
            _guard_intact(buf, y.numel(), f"few-out bf16 x {cin}->{cout} {hw}")
            assert torch.equal(y, got)


# ================================================================================================== pointwise, few inputs
@pytest.mark.parametrize("cout", R.FEW_IN_COUT)   # 5; 64 (the input layer); 257: the LDS fill loop strides past its 256 threads
@pytest.mark.parametrize("cin", R.FEW_IN_CIN)     # pw_few_in_kernel<1>, <2>, <3>, <4>
def test_pointwise_few_inputs(H, cin, cout):
    """maps 5x9 (ragged, tail) and 33x35 (HW = 1155: two blocks, ragged); no / first / second / both FusedLeakyReLU stages, each with and
    without in_scale + ch_bias"""
    for hw in R.FEW_IN_MAPS:
        for name, acts in R.ACT_SETS.items():
            for lin in ((), ("in_scale", "ch_bias")):
                kw = R.pointwise_case(cin, cout, *hw, operands=lin + acts)
                args, d = _launch_kw(kw)
                R.bound(H.pointwise(*args, **d), R.pointwise(**kw, dtype=F64), R.pointwise(**kw, dtype=F32),
                        f"few-in {cin}->{cout} {hw} {name}{' scale+bias' if lin else ''}")


@pytest.mark.parametrize("cin", R.FEW_IN_CIN)     # pw_few_in_kernel<1..4, bf16_t>
def test_pointwise_few_inputs_bf16_output(H, cin):
    """bf16 features out on 33x35 (planes of 1155 halfwords: 8-byte store4 at halfword alignment, store1 tail), reached through the
    bf16-activation configuration: the fp32 launch rounded once, within half a bf16 unit + the fp32 bound of float64, nothing behind y"""
    for cout in R.FEW_IN_COUT:
        kw = R.pointwise_case(cin, cout, 33, 35, operands=("in_scale", "ch_bias", "bias1", "bias2"))
        args, d = _launch_kw(kw)
        ref = H.pointwise(*args, **d)
        H.ACT_BF16, H.BF16_CONV = True, True
        try:
            got = H.pointwise(*args, **d)
        finally:
            H.ACT_BF16, H.BF16_CONV = False, False
        assert ref.dtype == F32 and got.dtype == BF and torch.equal(got, ref.to(BF))
        r64 = R.pointwise(**kw, dtype=F64)
        R.bound(got.float(), r64, R.pointwise(**kw, dtype=F32), f"few-in bf16 y {cin}->{cout}", slack=R.bf16_half_ulp(r64))
        rc, y, buf = _pointwise_entry(H, kw, y_dtype=BF, bf16_entry=True)
        assert rc == 0
        _guard_intact(buf, y.numel(), f"few-in bf16 y {cin}->{cout}")
        assert torch.equal(y, got)


# ================================================================================================== pointwise, LDS limit
@pytest.mark.parametrize("cin,cout", R.LDS_LIMIT_CASES)   # few outputs: Cout * Cin floats, 4096 x 4 and 16384 x 1 = 64 KB exactly;
#                                                           few inputs: Cout * (Cin + 3) floats, 2340 x 7 = 65 520 bytes, 4096 x 4 = 64 KB
def test_pointwise_lds_limit(H, cin, cout):
    """the widest launch the entry admits is correct, one channel more is VSP_EINVAL with the limit in the message and no launch"""
    from vspbfr_amd._lib import last_error
    kw = R.pointwise_case(cin, cout, 4, 4, operands=("in_scale", "ch_bias"), B=1)
    rc, y, buf = _pointwise_entry(H, kw)
    assert rc == 0, last_error()
    _guard_intact(buf, y.numel(), f"lds limit {cin}->{cout}")
    R.bound(y, R.pointwise(**kw, dtype=F64), R.pointwise(**kw, dtype=F32), f"lds limit {cin}->{cout}")
    wide = cout <= 4
    over = R.pointwise_case(cin + 1 if wide else cin, cout if wide else cout + 1, 4, 4, operands=("in_scale", "ch_bias"), B=1)
    for bf16_entry in (False, True):
        x = dev(over["x"]).to(BF) if (bf16_entry and wide) else None
        rc, y, buf = _pointwise_entry(H, over, x=x, y_dtype=BF if (bf16_entry and not wide) else F32, bf16_entry=bf16_entry)
        assert rc == -1                                                       # VSP_EINVAL
        msg = last_error()
        assert "65536" in msg and "LDS" in msg and (f"Cin <= {cin}" in msg if wide else f"Cout <= {cout}" in msg), msg
        torch.cuda.synchronize()
        assert bool((buf == SENTINEL).all())                                  # refused before any launch
    with pytest.raises(RuntimeError, match="LDS"):
        H.pointwise(dev(over["x"]), dev(over["w"]))


# ================================================================================================== affine_sample, adjoint
@pytest.mark.parametrize("mat", R.SAMPLER_MATS)   # identity; half-pixel shift (taps half on column -1 / IW and row -1 / IH); 45 degree
#                                                   rotation x 1.3; shift 3.0 (all outside); shift 1e6 (the clamp before the int
#                                                   conversion); zero matrix (every pixel samples the centre)
@pytest.mark.parametrize("m", [0, 1])             # 2x3x9x7 -> 11x13 and 1x2x16x16 -> 16x16
def test_affine_sample_forward_and_adjoint(m, mat):
    from vspbfr_amd import non_leaking as NL
    shape, out_hw = R.SAMPLER_MAPS[m]
    x, th, g = R.sampler_case(shape, out_hw, mat)
    xd = dev(x).requires_grad_(True)
    y = NL.affine_sample(xd, dev(th), out_hw)
    (gx,) = torch.autograd.grad(y, xd, dev(g))
    if mat in ("shift3", "shift1e6"):
        assert bool(torch.isfinite(y).all()) and float(y.detach().abs().max()) == 0.0 and float(gx.abs().max()) == 0.0
    R.bound(y, R.affine_sample(x, th, out_hw, F64), R.affine_sample(x, th, out_hw, F32), f"affine_sample {mat} map {m}")
    R.bound(gx, R.affine_sample_adjoint(g, th, shape[2:], F64), R.affine_sample_adjoint(g, th, shape[2:], F32), f"affine_sample adjoint {mat} map {m}")
    assert torch.equal(NL.affine_sample(dev(x), dev(th), out_hw), y.detach())              # the no-grad route is the same launch


@pytest.mark.parametrize("shape,out_hw,mat", [((1, 2, 8, 8), (64, 64), "magnify"),        # every output lands on the central 3x3 input pixels: hundreds of atomic adds each
                                              ((2, 3, 9, 7), (11, 13), "rot45"),
                                              ((2, 3, 140, 150), (300, 300), "rot45")])     # 540 000 outputs > 524 288: second grid pass
def test_affine_sample_adjoint_identities(shape, out_hw, mat):
    """forward and adjoint against float64; <A x, g> = <x, A^T g> in float64 from the two device results, within what the two bounds
    allow (|<A x - ref, g>| <= tol_fwd sum |g|, likewise the adjoint's: Hoelder); second order: the backward of the adjoint IS the forward"""
    from vspbfr_amd import non_leaking as NL
    x, th, g = R.sampler_case(shape, out_hw, mat)
    xd, gd, thd = dev(x).requires_grad_(True), dev(g).requires_grad_(True), dev(th)
    y = NL.affine_sample(xd, thd, out_hw)
    (gx,) = torch.autograd.grad(y, xd, gd, create_graph=True)
    tols = []
    for what, got, r64, r32 in (("forward", y, R.affine_sample(x, th, out_hw, F64), R.affine_sample(x, th, out_hw, F32)),
                                ("adjoint", gx, R.affine_sample_adjoint(g, th, shape[2:], F64), R.affine_sample_adjoint(g, th, shape[2:], F32))):
        e_ref, _, _ = R.bound(got, r64, r32, f"affine_sample {what} {mat} {shape}->{out_hw}")
        tols.append(4 * e_ref + 2e-6 * float(r64.abs().max()))
    lhs = float((y.detach().cpu().double() * g.double()).sum())
    rhs = float((x.double() * gx.detach().cpu().double()).sum())
    tol = tols[0] * float(g.double().abs().sum()) + tols[1] * float(x.double().abs().sum())
    print(f"STREAM affine_sample dot identity {mat} {shape}: <Ax,g>={lhs:.9e} <x,Atg>={rhs:.9e} |d|={abs(lhs - rhs):.3e} tol={tol:.3e}")
    assert abs(lhs - rhs) <= tol
    v = torch.randn(*shape, generator=_g(77)).to(DEV)
    (gg,) = torch.autograd.grad(gx, gd, v)
    assert torch.equal(gg, NL.affine_sample(v, thd, out_hw))


# ================================================================================================== color_affine
@pytest.mark.parametrize("shape", [(2, 3, 5, 7), (2, 3, 300, 300),
                                   (3, 3, 420, 420)])  # one thread per pixel of an image: 3 x 176 400 = 529 200 threads, second grid pass
def test_color_affine(shape):
    from vspbfr_amd import non_leaking as NL
    g = _g(shape[0] * 1000 + shape[2])
    B = shape[0]
    x = torch.randn(*shape, generator=g)
    mat = torch.zeros(B, 4, 4)
    mat[:, :3, :] = torch.randn(B, 3, 4, generator=g)                 # a non-symmetric M and an offset per image
    mat[:, 3, 3] = 1
    M, t = mat[:, :3, :3].contiguous(), mat[:, :3, 3].contiguous()
    assert not torch.equal(M, M.transpose(1, 2)) and not torch.equal(M[0], M[1])
    R.bound(NL.apply_color(dev(x), mat), R.color_affine(x, M, t, F64), R.color_affine(x, M, t, F32), f"color_affine {shape}")
    R.bound(NL._color_raw(dev(x), dev(M), None), R.color_affine(x, M, None, F64), R.color_affine(x, M, None, F32), f"color_affine no t {shape}")
    cot = torch.randn(*shape, generator=g)
    xd = dev(x).requires_grad_(True)
    (gx,) = torch.autograd.grad(NL.apply_color(xd, mat), xd, dev(cot))
    x64 = x.double().requires_grad_(True)
    (g64,) = torch.autograd.grad(R.color_affine(x64, M, t, F64), x64, cot.double())
    Mt = M.transpose(1, 2)
    R.bound(gx, g64, R.color_affine(cot, Mt, None, F32), f"color_affine gradient {shape}")
    if shape[2] == 5:
        with pytest.raises(RuntimeError, match="3-channel"):
            NL.apply_color(dev(x[:, :2].contiguous()), mat)


# ================================================================================================== row helpers
@pytest.mark.parametrize("shape", [(1, 1, 1, 1), (1, 5, 5, 41), BIG])   # 1 element; 1025 = four blocks + 1; second grid pass
def test_elementwise_helpers(H, shape):
    """film, axpby_idx, add3 (with and without c), scale_add (with and without y)"""
    g = _g(sum(shape))
    h, a, b = (torch.randn(*shape, generator=g) for _ in range(3))
    R.bound(H.film(dev(h), dev(a), dev(b)), R.film(h, a, b, F64), R.film(h, a, b, F32), f"film {shape}")
    c1, c2 = torch.rand(7, generator=g) + 0.1, torch.randn(7, generator=g)
    R.bound(H.axpby_idx(dev(h), dev(a), dev(c1), dev(c2), 5), R.axpby_idx(h, a, c1, c2, 5, F64), R.axpby_idx(h, a, c1, c2, 5, F32), f"axpby_idx {shape}")
    R.bound(H.add3(dev(h), dev(a), dev(b)), R.add3(h, a, b, F64), R.add3(h, a, b, F32), f"add3 {shape}")
    R.bound(H.add3(dev(h), dev(a)), R.add3(h, a, None, F64), R.add3(h, a, None, F32), f"add3 no c {shape}")
    gate = torch.rand(*shape[:2], generator=g) + 0.25
    R.bound(H.scale_add(dev(h), dev(gate), dev(a)), R.scale_add(h, gate, a, F64), R.scale_add(h, gate, a, F32), f"scale_add {shape}")
    R.bound(H.scale_add(dev(h), dev(gate)), R.scale_add(h, gate, None, F64), R.scale_add(h, gate, None, F32), f"scale_add no y {shape}")


@pytest.mark.parametrize("shape", [(1, 1, 2, 2), (2, 3, 6, 10), (2, 5, 512, 512)])   # -> 1x1; 3x5; 655 360 outputs: second grid pass
def test_avgpool2x2(H, shape):
    x = torch.randn(*shape, generator=_g(shape[2]))
    R.bound(H.avgpool2x2(dev(x)), R.avgpool2x2(x, F64), R.avgpool2x2(x, F32), f"avgpool2x2 {shape}")


def test_avgpool2x2_refusals(H):
    from vspbfr_amd._lib import last_error, lib
    for shape in ((1, 1, 3, 4), (1, 1, 4, 3)):
        with pytest.raises(RuntimeError, match="even"):
            H.avgpool2x2(torch.zeros(*shape, device=DEV))
    base = torch.zeros(4 * 6 + 1, device=DEV)
    x = base[1:]                                                       # one element off 8-byte alignment
    assert x.data_ptr() % 8 == 4
    buf, out = _guarded(2 * 3, F32)
    assert lib.vsp_avgpool2x2_f32(H._ptr(out), H._ptr(x), 1, 2, 3, H._stream()) == -1 and "8-byte" in last_error()
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())


@pytest.mark.parametrize("ihw,ohw", R.UPSAMPLE_SIZES)   # IH = IW = 1 (both ratios 0); IH = 1 / IW = 1 with the other axis kept; OH = OW = 1
#                                                         (ratio forced to 0); the identity size; 5x7 -> 9x16 (ratios 1/2 and 2/5)
def test_upsample_add(H, ihw, ohw):
    x, y = R.upsample_case(ihw, ohw)
    got = H.upsample_add(dev(x), dev(y))
    R.bound(got, R.upsample_add(x, y, F64), R.upsample_add(x, y, F32), f"upsample_add {ihw}->{ohw}")
    if ihw == ohw:
        assert torch.equal(got, dev(x) + dev(y))


def test_upsample_add_and_resize_second_grid_pass(H):
    x, y = R.upsample_case((128, 128), BIG[2:], planes=BIG[:2])
    R.bound(H.upsample_add(dev(x), dev(y)), R.upsample_add(x, y, F64), R.upsample_add(x, y, F32), "upsample_add 128x128->256x256 x10")
    x, _ = R.upsample_case((100, 90), BIG[2:], planes=BIG[:2])
    R.bound(H.resize_bilinear(dev(x), BIG[2:]), R.resize_bilinear(x, BIG[2:], F64), R.resize_bilinear(x, BIG[2:], F32), "resize_bilinear 100x90->256x256 x10")


@pytest.mark.parametrize("ihw,ohw", R.RESIZE_SIZES)     # one input pixel; one output pixel; 2x9 -> 7x3 (up in one axis, down in the other)
def test_resize_bilinear(H, ihw, ohw):
    x, _ = R.upsample_case(ihw, ohw)
    R.bound(H.resize_bilinear(dev(x), ohw), R.resize_bilinear(x, ohw, F64), R.resize_bilinear(x, ohw, F32), f"resize_bilinear {ihw}->{ohw}")


@pytest.mark.parametrize("planes", [1, 5])              # one wave of a workgroup's four; a second workgroup with one wave
@pytest.mark.parametrize("hw", R.PLANE_HW)              # 1; one below, on and one above the wave width; 64 x 64 + 1
def test_plane_mean(H, hw, planes):
    for offset in (0.0, 1e3):
        x = R.plane_mean_case(hw, planes, offset)
        R.bound(H.plane_mean(dev(x)), R.plane_mean(x, F64), R.plane_mean(x, F32), f"plane_mean hw={hw} x{planes} +{offset:g}")
    if hw == 1 and planes == 1:
        x = torch.randn(*BIG, generator=_g(3)) + 0.5
        R.bound(H.plane_mean(dev(x)), R.plane_mean(x, F64), R.plane_mean(x, F32), f"plane_mean {BIG}")


def test_subsample(H):
    g = _g(11)
    for hw in ((7, 5), (1, 1)):
        x = torch.randn(2, 3, *hw, generator=g)
        for s in (1, 2, 3):
            assert torch.equal(H.subsample(dev(x), s).cpu(), R.subsample(x, s)), (hw, s)
    x = torch.randn(*BIG, generator=g)
    assert torch.equal(H.subsample(dev(x), 1).cpu(), x)                           # 655 360 outputs: second grid pass
    x = torch.randn(2, 5, 511, 513, generator=g)
    assert torch.equal(H.subsample(dev(x), 2).cpu(), R.subsample(x, 2))           # 2 x 5 x 256 x 257 outputs through the stride


def test_quantize_u8_nhwc(H):
    g = _g(13)
    for shape in ((2, 3, 300, 300), (1, 1, 1, 1)):                                # 540 000 bytes: second grid pass; one byte
        x = torch.randn(*shape, generator=g) * 0.8
        want = OM.save_image_quantize(x).permute(0, 2, 3, 1).contiguous()
        assert torch.equal(R.quantize_u8_nhwc(x), want)
        got = H.quantize_u8_nhwc(dev(x)).cpu()
        assert got.dtype == torch.uint8 and got.shape == want.shape
        assert torch.equal(got, want), f"{shape}: {int((got != want).sum())} bytes differ"
    x = torch.randn(2, 3, 37, 53, generator=g) * 2 + 1
    assert torch.equal(H.quantize_u8_nhwc(dev(x), 0.0, 2.5).cpu(), R.quantize_u8_nhwc(x, 0.0, 2.5))
    lo, hi = 0.3, 0.3 + 1e-6                                                       # hi - lo below 1e-5: the range is 1e-5
    x = 0.3 + torch.rand(2, 3, 9, 11, generator=g) * 2e-6 - 5e-7
    want = R.quantize_u8_nhwc(x, lo, hi)
    assert int(want.max()) < 64 and int(want.max()) > 0                           # (a range of hi - lo would have reached 255)
    assert torch.equal(H.quantize_u8_nhwc(dev(x), lo, hi).cpu(), want)


@pytest.mark.parametrize("T,B,D", [(1, 3, 5), (18, 2, 512), (4, 1, 1), (18, 60, 512)])   # one token: no w0 to add; the model's shape; one
#                                                                                          column; 552 960 elements: second grid pass
def test_e4e_codes(H, T, B, D):
    g = _g(T * 100 + B)
    heads, avg = torch.randn(T, B, D, generator=g), torch.randn(T, D, generator=g)
    R.bound(H.e4e_codes(dev(heads), dev(avg)), R.e4e_codes(heads, avg, F64), R.e4e_codes(heads, avg, F32), f"e4e_codes {(T, B, D)} avg")
    R.bound(H.e4e_codes(dev(heads)), R.e4e_codes(heads, None, F64), R.e4e_codes(heads, None, F32), f"e4e_codes {(T, B, D)}")


@pytest.mark.parametrize("B,T", [(2, 4), (3, 1), (64, 18)])      # (64, 18) with the three-segment case: 64 x 18 x 518 elements, second pass
def test_rows_concat(H, B, T):
    g = _g(B * 10 + T)
    wide = torch.randn(B, T + 2, 512 + 3, generator=g)           # longer and wider than what is read: through its strides
    tok5, tok1 = torch.randn(B, T, 5, generator=g), torch.randn(B, T, 1, generator=g)
    row512, row1 = torch.randn(B, 512, generator=g), torch.randn(B, 1, generator=g)
    cases = {"one segment": [(tok5, 5, True, False)],
             "one column": [(tok1, 1, True, False)],
             "one broadcast column": [(row1, 1, False, False)],
             "strided + broadcast": [(wide, 512, True, False), (row512, 512, False, False)],
             "flipped strided + column": [(wide, 5, True, True), (tok1, 1, True, False)],
             "three": [(wide, 512, True, True), (row1, 1, False, False), (tok5, 5, True, False)]}
    for name, segs in cases.items():
        got = H.rows_concat(B, T, [(dev(t), w, p, f) for t, w, p, f in segs])
        assert torch.equal(got.cpu(), R.rows_concat(B, T, segs)), f"rows_concat {name} B={B} T={T}"


@pytest.mark.parametrize("B,cout", [(1, 1), (3, 5), (2, 130), (16, 512)])   # one row; 15 rows (off the 4 per workgroup); 260; 8192 rows
@pytest.mark.parametrize("cin", [1, 63, 65, 512])                            # off the wave width on both sides, and 8 loop trips
def test_demod_coefs(H, cin, B, cout):
    g = _g(cin * 1000 + cout)
    style, wsq = torch.randn(B, cin, generator=g), torch.rand(cout, cin, generator=g) * 9
    ws = 1 / math.sqrt(cin * 9)
    R.bound(H.demod_coefs(dev(style), dev(wsq), ws), R.demod_coefs(style, wsq, ws, 1e-8, F64), R.demod_coefs(style, wsq, ws, 1e-8, F32),
            f"demod_coefs {B}x{cin}->{cout}")
