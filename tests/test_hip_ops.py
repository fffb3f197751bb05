"""Parity of the gfx950 kernels (through the C ABI, via vspbfr_amd.hip_ops / vspbfr_amd.op) against the CPU oracle and
the reference's golden vectors.  Needs a real MI355X: `pytest -m gpu`."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from oracle import cases, ops as O

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"


def dev(t):
    return t.to(DEV).contiguous()


def close(a, b, rtol=1e-5, atol=1e-5, what=""):
    a = a.detach().cpu().numpy() if isinstance(a, torch.Tensor) else a
    b = b.detach().cpu().numpy() if isinstance(b, torch.Tensor) else b
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.isfinite(a).all(), f"{what}: non-finite output"
    err = np.abs(a - b).max() if a.size else 0.0
    tol = atol + rtol * (np.abs(b).max() if b.size else 0.0)
    assert err <= tol, f"{what}: max|d|={err:.3e} tol={tol:.3e}"


@pytest.fixture(scope="module")
def H():
    from vspbfr_amd import hip_ops
    return hip_ops


# ------------------------------------------------------------------------------------------------ fused_bias_act
@pytest.mark.parametrize("name", list(cases.LRELU_CASES))
def test_fused_leaky_relu_golden(golden, name):
    from vspbfr_amd.op import fused_leaky_relu
    x, b = cases.lrelu_inputs(name)
    y = fused_leaky_relu(dev(x), dev(b) if b is not None else None)
    close(y, golden("ops")[name], 1e-6, 1e-6, name)  # bit-level ops: one add, one select, one multiply


@pytest.mark.parametrize("act,grad", [(1, 0), (1, 1), (1, 2), (3, 0), (3, 1), (3, 2)])
@pytest.mark.parametrize("shape", [(3, 7, 5, 6), (2, 8, 16, 16), (4, 12)])
def test_fused_bias_act_modes(H, act, grad, shape):
    g = torch.Generator().manual_seed(act * 10 + grad)
    x = torch.randn(shape, generator=g)
    b = torch.randn(shape[1], generator=g)
    ref = torch.randn(shape, generator=g)
    y = H.fused_bias_act(dev(x), dev(b), dev(ref), act, grad, 0.2, math.sqrt(2))
    close(y, O.fused_bias_act(x, b, ref, act, grad, 0.2, math.sqrt(2)), 1e-6, 1e-6)
    # no bias / no ref = empty tensors, as in the reference's python wrapper
    e = torch.empty(0, device=DEV)
    y = H.fused_bias_act(dev(x), e, e, act, 0, 0.1, 2.0)
    close(y, O.fused_bias_act(x, None, None, act, 0, 0.1, 2.0), 1e-6, 1e-6)


def test_fused_bias_act_large_and_empty(H):
    x = torch.randn(2, 64, 128, 128)
    b = torch.randn(64)
    close(H.fused_bias_act(dev(x), dev(b), torch.empty(0, device=DEV), 3, 0, 0.2, math.sqrt(2)), O.fused_leaky_relu(x, b), 1e-6, 1e-6)
    z = H.fused_bias_act(torch.empty(0, 4, device=DEV), torch.empty(0, device=DEV), torch.empty(0, device=DEV), 3, 0, 0.2, 1.0)
    assert z.numel() == 0


def test_op_error_behaviour(H):
    from vspbfr_amd.op import fused_leaky_relu, upfirdn2d
    with pytest.raises(RuntimeError):
        fused_leaky_relu(torch.randn(2, 3), torch.randn(3))  # CPU tensor -> RuntimeError (reference: TORCH_CHECK is_cuda)
    with pytest.raises(RuntimeError):
        H.fused_bias_act(torch.randn(4, 6, device=DEV).t(), torch.empty(0, device=DEV), torch.empty(0, device=DEV), 3, 0, 0.2, 1.0)
    with pytest.raises(RuntimeError):
        upfirdn2d(torch.randn(1, 1, 4, 4), torch.ones(2, 2))


# ------------------------------------------------------------------------------------------------ upfirdn2d
@pytest.mark.parametrize("name", list(cases.FIR_CASES))
def test_upfirdn2d_golden(golden, name):
    from vspbfr_amd.op import upfirdn2d
    x, k, up, down, pad = cases.fir_inputs(name)
    y = upfirdn2d(dev(x), dev(k), up=up, down=down, pad=pad)
    close(y, golden("ops")[name], 1e-6, 2e-6, name)


@pytest.mark.parametrize("shape,pad", [((2, 16, 257, 257), (1, 1)), ((2, 16, 256, 256), (2, 2)), ((1, 3, 65, 31), (1, 1)),
                                       ((1, 2, 33, 200), (2, 2))])
def test_upfirdn2d_blur_big(shape, pad):
    from vspbfr_amd.op import upfirdn2d
    x = torch.randn(shape)
    k = O.make_kernel([1, 3, 3, 1]) * 4
    close(upfirdn2d(dev(x), dev(k), pad=pad), O.upfirdn2d(x, k, pad=pad), 1e-6, 2e-6)


def test_blur_fused_epilogue(H):
    B, C_, Hh, Ww = 2, 6, 33, 37
    x = torch.randn(B, C_, Hh, Ww)
    k = O.make_kernel([1, 3, 3, 1]) * 4
    ps, nz, nw = torch.rand(B, C_) + 0.5, torch.randn(B, 1, Hh - 1, Ww - 1), torch.tensor([0.3])
    bias, r1, r2 = torch.randn(C_), torch.randn(B, C_, Hh - 1, Ww - 1), torch.randn(B, C_, Hh - 1, Ww - 1)
    ref = O.upfirdn2d(x, k, pad=(1, 1)) * ps.view(B, C_, 1, 1) + nz * nw
    ref = O.fused_leaky_relu(ref, bias) + r1 + r2
    y = H.blur_fused(dev(x), dev(k), (1, 1), plane_scale=dev(ps), noise=dev(nz), noise_w=dev(nw), act_bias=dev(bias), act=True,
                     res1=dev(r1), res2=dev(r2))
    close(y, ref, 1e-5, 1e-5)


# ------------------------------------------------------------------------------------------------ conv2d
CONV_SHAPES = [
    # B, Cin, Cout, H, W, k, stride, pad, dil
    (2, 8, 16, 12, 12, 3, 1, 1, 1),
    (1, 3, 16, 20, 33, 3, 1, 1, 1),      # Cin not a multiple of 4, ragged width
    (2, 16, 64, 32, 32, 3, 1, 1, 1),
    (1, 64, 64, 40, 48, 3, 1, 1, 1),
    (1, 32, 32, 64, 64, 3, 1, 2, 2),
    (1, 16, 16, 40, 40, 3, 1, 4, 4),
    (1, 16, 16, 40, 40, 3, 1, 8, 8),
    (2, 16, 32, 33, 33, 3, 2, 0, 1),     # stride 2, pad 0 (StyledConv_down after blur)
    (2, 16, 32, 32, 32, 3, 2, 1, 1),     # stride 2, pad 1 (IR-SE, style heads)
    (2, 24, 3, 16, 16, 1, 1, 0, 1),      # 1x1 to 3 channels (ToRGB)
    (1, 12, 20, 7, 9, 1, 1, 0, 1),
    (3, 512, 128, 4, 4, 3, 1, 1, 1),     # tiny maps, deep K
    (2, 128, 128, 8, 8, 3, 1, 1, 1),
    (2, 64, 64, 2, 2, 3, 2, 1, 1),       # 2x2 -> 1x1 (last conv of a GradualStyleBlock)
    (1, 40, 72, 16, 16, 3, 1, 1, 1),     # channel counts that are not multiples of the tile
]


@pytest.mark.parametrize("shape", CONV_SHAPES)
def test_conv2d_vs_torch(H, shape):
    B, Cin, Cout, Hh, Ww, k, s, p, d = shape
    g = torch.Generator().manual_seed(sum(shape))
    x = torch.randn(B, Cin, Hh, Ww, generator=g)
    w = torch.randn(Cout, Cin, k, k, generator=g) / math.sqrt(Cin * k * k)
    b = torch.randn(Cout, generator=g)
    ref = F.conv2d(x, w, b, stride=s, padding=p, dilation=d)
    y = H.conv2d(dev(x), dev(w), dev(b), s, p, d)
    close(y, ref, 2e-5, 2e-5, str(shape))


def test_conv2d_all_tile_configs(H):
    from vspbfr_amd._lib import lib
    B, Cin, Cout, Hh, Ww = 2, 24, 80, 37, 45
    x = torch.randn(B, Cin, Hh, Ww)
    w = torch.randn(Cout, Cin, 3, 3) / math.sqrt(Cin * 9)
    ref = F.conv2d(x, w, None, padding=1)
    n = lib.vsp_conv2d_num_configs()
    assert n >= 8
    ran = 0
    for c in range(1, n + 1):
        try:
            y = H.conv2d(dev(x), dev(w), None, 1, 1, 1, tile_hint=c)
        except RuntimeError as ex:  # a forced configuration may legitimately not fit (LDS) -- the library says so
            assert "does not fit" in str(ex), str(ex)
            continue
        close(y, ref, 2e-5, 2e-5, f"cfg {c} {lib.vsp_conv2d_config_name(c - 1)}")
        ran += 1
    assert ran >= 24
    # K-split configurations on the kind of layer they exist for: deep K, tiny map, ragged channel count
    x2 = torch.randn(3, 200, 5, 5)
    w2 = torch.randn(40, 200, 3, 3) / math.sqrt(200 * 9)
    ref2 = F.conv2d(x2, w2, None, padding=1)
    for c in range(1, n + 1):
        if b"k1p" in lib.vsp_conv2d_config_name(c - 1):  # not a K-split configuration
            continue
        try:
            y2 = H.conv2d(dev(x2), dev(w2), None, 1, 1, 1, tile_hint=c)
        except RuntimeError as ex:
            assert "does not fit" in str(ex), str(ex)
            continue
        close(y2, ref2, 2e-5, 2e-5, f"ksplit cfg {c}")


def test_conv2d_prologue_epilogue(H):
    B, Cin, Cout, Hh, Ww = 2, 16, 32, 18, 21
    x = torch.randn(B, Cin, Hh, Ww)
    w = torch.randn(Cout, Cin, 3, 3) / math.sqrt(Cin * 9)
    s_in, shift = torch.rand(B, Cin) + 0.5, torch.randn(Cin) * 0.1
    demod, cs, cb = torch.rand(B, Cout) + 0.5, torch.rand(Cout) + 0.5, torch.randn(Cout)
    b1, b2, nz, nw = torch.randn(Cout), torch.randn(Cout), torch.randn(B, 1, Hh, Ww), torch.tensor([0.4])
    r1, r2 = torch.randn(B, Cout, Hh, Ww), torch.randn(B, Cout, Hh, Ww)
    xin = x * s_in.view(B, Cin, 1, 1) + shift.view(1, Cin, 1, 1)
    ref = torch.stack([F.conv2d(xin[i:i + 1], w, padding=1)[0] for i in range(B)])
    ref = ref * demod.view(B, Cout, 1, 1) * cs.view(1, Cout, 1, 1) + cb.view(1, Cout, 1, 1)
    ref = O.fused_leaky_relu(ref, b1) + nz * nw
    ref = O.fused_leaky_relu(ref, b2) + r1 + r2
    pc = H.PackedConv(H.pack_weight(dev(w)), 1, Cout, Cin, 3, 3, 1, (1,), (1,))
    y = H.conv2d_packed(dev(x), pc, in_scale=dev(s_in), in_shift=dev(shift), out_scale=dev(demod), ch_scale=dev(cs),
                        ch_bias=dev(cb), act1=True, bias1=dev(b1), noise=dev(nz), noise_w=dev(nw), act2=1, bias2=dev(b2),
                        res1=dev(r1), res2=dev(r2))
    close(y, ref, 3e-5, 3e-5)
    # PReLU flavour + per-channel (batch-independent) input scale, as the IR-SE units use it
    a = torch.rand(Cout) * 0.3
    sc = torch.rand(Cin) + 0.5
    ref2 = F.prelu(F.conv2d(x * sc.view(1, Cin, 1, 1) + shift.view(1, Cin, 1, 1), w, padding=1), a)
    y2 = H.conv2d_packed(dev(x), pc, in_scale=dev(sc), in_scale_per_sample=False, in_shift=dev(shift), act2=2, prelu=dev(a))
    close(y2, ref2, 3e-5, 3e-5)
    # nn.LeakyReLU(0.01) flavour (GradualStyleBlock)
    ref3 = F.leaky_relu(F.conv2d(x, w, cb, padding=1), 0.01)
    y3 = H.conv2d_packed(dev(x), pc, ch_bias=dev(cb), act2=1, slope2=0.01, gain2=1.0)
    close(y3, ref3, 3e-5, 3e-5)


def test_conv2d_dilation_groups_into_slices(H):
    """The four dilated branches of a SMART layer in ONE launch, each writing its channel slice (no torch.cat)."""
    B, Cin, Cg, Hh, Ww = 2, 16, 8, 24, 24
    x = torch.randn(B, Cin, Hh, Ww)
    ws = [torch.randn(Cg, Cin, 3, 3) / math.sqrt(Cin * 9) for _ in range(4)]
    ref = torch.cat([F.conv2d(x, w_, padding=d, dilation=d) for w_, d in zip(ws, (1, 2, 4, 8))], dim=1)
    wp = torch.stack([H.pack_weight(dev(w_))[0] for w_ in ws]).contiguous()
    pc = H.PackedConv(wp, 4, Cg, Cin, 3, 3, 1, (1, 2, 4, 8), (1, 2, 4, 8))
    close(H.conv2d_packed(dev(x), pc), ref, 2e-5, 2e-5)


@pytest.mark.parametrize("B,Cin,Cg,Hh,Ww", [(2, 16, 8, 24, 24), (1, 24, 16, 37, 21), (2, 64, 32, 32, 32), (1, 40, 20, 16, 48)])
def test_conv2d_dilation_groups_fused_kernels(H, B, Cin, Cg, Hh, Ww):
    """Every 'd' configuration (four dilated branches from one staged patch) incl. style scale, demod and the epilogue."""
    from vspbfr_amd._lib import lib
    x = torch.randn(B, Cin, Hh, Ww)
    ws = [torch.randn(Cg, Cin, 3, 3) / math.sqrt(Cin * 9) for _ in range(4)]
    s_in, demod, bias = torch.rand(B, Cin) + 0.5, torch.rand(B, 4 * Cg) + 0.5, torch.randn(4 * Cg)
    xs = x * s_in.view(B, Cin, 1, 1)
    ref = torch.cat([F.conv2d(xs, w_, padding=d, dilation=d) for w_, d in zip(ws, (1, 2, 4, 8))], dim=1)
    ref = F.leaky_relu(ref * demod.view(B, -1, 1, 1) + bias.view(1, -1, 1, 1), 0.2) * math.sqrt(2)
    wp = torch.stack([H.pack_weight(dev(w_))[0] for w_ in ws]).contiguous()
    pc = H.PackedConv(wp, 4, Cg, Cin, 3, 3, 1, (1, 2, 4, 8), (1, 2, 4, 8))
    ran = 0
    for c in range(1, lib.vsp_conv2d_num_configs() + 1):
        if not lib.vsp_conv2d_config_name(c - 1).endswith(b"d"):
            continue
        try:
            y = H.conv2d_packed(dev(x), pc, in_scale=dev(s_in), out_scale=dev(demod), act2=1, bias2=dev(bias), tile_hint=c)
        except RuntimeError as ex:
            assert "does not fit" in str(ex), str(ex)
            continue
        close(y, ref, 3e-5, 3e-5, f"cfg {lib.vsp_conv2d_config_name(c - 1)}")
        ran += 1
    assert ran >= 2


@pytest.mark.parametrize("B,Cin,Cout,Hh,Ww", [(2, 8, 12, 8, 8), (1, 16, 16, 5, 9), (1, 64, 32, 32, 32)])
def test_conv_transpose_s2_phases(H, B, Cin, Cout, Hh, Ww):
    x = torch.randn(B, Cin, Hh, Ww)
    w = torch.randn(Cout, Cin, 3, 3) / math.sqrt(Cin * 9)  # stored (Cout, Cin, k, k) like ModulatedConv2d.weight[0]
    ref = F.conv_transpose2d(x, w.transpose(0, 1), stride=2, padding=0)
    y = H.conv_transpose2d_s2(dev(x), H.pack_transposed_s2(dev(w)))
    close(y, ref, 2e-5, 2e-5)


@pytest.mark.parametrize("B,Cin,Cout,Hh,Ww", [(2, 8, 12, 8, 8), (1, 16, 16, 5, 9), (1, 64, 32, 32, 32), (2, 40, 72, 17, 33), (3, 512, 512, 4, 4)])
def test_conv_transpose_s2_fused(H, B, Cin, Cout, Hh, Ww):
    """One-launch transposed conv (all four sub-pixel phases) incl. style scaling and demodulation, every 't' configuration."""
    from vspbfr_amd._lib import lib
    x = torch.randn(B, Cin, Hh, Ww)
    w = torch.randn(Cout, Cin, 3, 3) / math.sqrt(Cin * 9)
    s_in, demod = torch.rand(B, Cin) + 0.5, torch.rand(B, Cout) + 0.5
    ref = F.conv_transpose2d(x * s_in.view(B, Cin, 1, 1), w.transpose(0, 1), stride=2, padding=0) * demod.view(B, Cout, 1, 1)
    pc = H.PackedConv(H.pack_weight(dev(w)), 1, Cout, Cin, 3, 3, 1, (1,), (1,))
    y = H.conv_transpose2d_s2_fused(dev(x), pc, in_scale=dev(s_in), out_scale=dev(demod))
    close(y, ref, 2e-5, 2e-5)
    ran = 0
    for c in range(1, lib.vsp_conv2d_num_configs() + 1):
        if not lib.vsp_conv2d_config_name(c - 1).endswith(b"t"):
            continue
        try:
            yc = H.conv_transpose2d_s2_fused(dev(x), pc, in_scale=dev(s_in), out_scale=dev(demod), tile_hint=c)
        except RuntimeError as ex:
            assert "does not fit" in str(ex), str(ex)
            continue
        close(yc, ref, 2e-5, 2e-5, f"cfg {c}")
        ran += 1
    assert ran >= 4


def test_conv2d_gradfix_mirror():
    from vspbfr_amd.op import conv2d_gradfix
    x = torch.randn(1, 12, 10, 10)
    w = torch.randn(8, 6, 3, 3) * 0.2
    close(conv2d_gradfix.conv2d(dev(x), dev(w), padding=1, groups=2), F.conv2d(x, w, padding=1, groups=2), 2e-5, 2e-5)
    wt = torch.randn(12, 5, 3, 3) * 0.2
    close(conv2d_gradfix.conv_transpose2d(dev(x), dev(wt), stride=2, padding=0), F.conv_transpose2d(x, wt, stride=2), 2e-5, 2e-5)


# ------------------------------------------------------------------------------------------------ modulated conv layers vs golden
def _modulated(H, x, weight, mod, demodulate, mode, blur, dilation=1):
    """modulate-input / demodulate-output form of the reference's grouped conv (same algebra as its fused=False
    branch, models/RestoreNet.py:343-370), on the HIP kernels."""
    _, Cout, Cin, k, _ = weight.shape
    scale = 1 / math.sqrt(Cin * k * k)
    w = weight[0] * scale
    demod = H.demod_coefs(mod, (weight[0] ** 2).sum((2, 3)).contiguous(), scale) if demodulate else None
    if mode == "up":
        y = H.conv_transpose2d_s2(x, H.pack_transposed_s2(w.contiguous()), in_scale=mod, out_scale=demod)
        return H.blur_fused(y, blur, (1, 1))
    if mode == "down":
        xb = H.blur_fused(x, blur, (2, 2))
        pc = H.PackedConv(H.pack_weight(w.contiguous()), 1, Cout, Cin, k, k, 2, (1,), (0,))
        return H.conv2d_packed(xb, pc, in_scale=mod, out_scale=demod)
    pad = ((k - 1) * dilation) // 2
    pc = H.PackedConv(H.pack_weight(w.contiguous()), 1, Cout, Cin, k, k, 1, (dilation,), (pad,))
    return H.conv2d_packed(x, pc, in_scale=mod, out_scale=demod)


@pytest.mark.parametrize("name", list(cases.MODCONV_CASES))
def test_modulated_conv_golden(H, golden, name):
    kind, cin, cout, k, sdim, xs, extra = cases.MODCONV_CASES[name]
    shapes = [("weight", (1, cout, cin, k, k))] + ([("blur.kernel", (4, 4))] if kind != "same" else [])
    shapes += [("modulation.weight", (cin, sdim)), ("modulation.bias", (cin,))]
    sd = {n: dev(t) for n, t in cases.module_weights(name, shapes).items()}
    x, style = dev(cases.tensor(name, "x", xs)), dev(cases.tensor(name, "style", (xs[0], sdim)))
    mod = H.linear(style, sd["modulation.weight"], sd["modulation.bias"], alpha=1 / math.sqrt(sdim))
    y = _modulated(H, x, sd["weight"], mod, extra.get("demodulate", True), kind, sd.get("blur.kernel"))
    close(y, golden("layers")[name], 3e-5, 3e-5, name)


@pytest.mark.parametrize("name", list(cases.DILCONV_CASES))
def test_dilated_modulated_conv_golden(H, golden, name):
    cin, cout, xs, d = cases.DILCONV_CASES[name]
    sd = cases.module_weights(name, [("weight", (1, cout, cin, 3, 3))])
    x, style = dev(cases.tensor(name, "x", xs)), dev(cases.tensor(name, "style", (xs[0], cin)) * 0.5 + 1.0)
    y = _modulated(H, x, dev(sd["weight"]), style, True, "same", None, dilation=d)
    close(y, golden("layers")[name], 3e-5, 3e-5, name)


# ------------------------------------------------------------------------------------------------ gemm + row helpers
@pytest.mark.parametrize("M,N,K", [(8, 512, 2048), (144, 512, 512), (36, 512, 513), (3, 17, 5), (8, 1024, 8192), (1, 16, 16)])
def test_linear(H, M, N, K):
    x, w, b = torch.randn(M, K), torch.randn(N, K) / math.sqrt(K), torch.randn(N)
    close(H.linear(dev(x), dev(w), dev(b)), F.linear(x, w, b), 3e-5, 3e-5)
    close(H.linear(dev(x), dev(w), dev(b), alpha=0.5, bias_scale=0.01, act=1), O.fused_leaky_relu(F.linear(x, w * 0.5), b * 0.01), 3e-5, 3e-5)
    close(H.linear(dev(x), dev(w), dev(b), act=2), torch.sigmoid(F.linear(x, w, b)), 3e-5, 3e-5)


@pytest.mark.parametrize("M,N,K", [(8, 512, 2048), (16, 130, 1024), (5, 511, 768), (1, 64, 512), (13, 32, 4096)])
def test_linear_few_rows(H, M, N, K):
    """The few-row form of the small GEMM (one wave per output column, M <= 16, K a multiple of 256: the style modulations of
    every modulated conv at batch 8 / 16) against float64, contiguous rows and rows that are a strided slice latent[:, i]."""
    g_ = torch.Generator().manual_seed(M * 1000 + N)
    x, w, b = torch.randn(M, K, generator=g_), torch.randn(N, K, generator=g_) / math.sqrt(K), torch.randn(N, generator=g_)
    ref = F.linear(x.double(), w.double() * 0.7, b.double() * 0.3)
    close(H.linear(dev(x), dev(w), dev(b), alpha=0.7, bias_scale=0.3), ref.float(), 2e-5, 2e-5, "plain")
    close(H.linear(dev(x), dev(w), dev(b), alpha=0.7, bias_scale=0.3, act=1), (F.leaky_relu(ref, 0.2) * math.sqrt(2)).float(), 2e-5, 2e-5, "lrelu")
    lat = torch.randn(M, 18, K, generator=g_)
    close(H.linear(dev(lat)[:, 7], dev(w), None, alpha=0.7), F.linear(lat[:, 7].double(), w.double() * 0.7).float(), 2e-5, 2e-5, "strided rows")


def test_gemm_strided_batched(H):
    B, T, D = 3, 18, 64
    Kt, Q, V = torch.randn(B, T, D), torch.randn(B, T, D), torch.randn(B, T, D)
    # K Q^T (NT), score V (NN via strides), k^T q (TN via strides)
    s = H.gemm_nt(dev(Kt), dev(Q), alpha=0.25)
    close(s, torch.matmul(Kt, Q.transpose(1, 2)) * 0.25, 3e-5, 3e-5)
    sc = torch.softmax(torch.randn(B, T, T), -1)
    h = H.gemm_nt(dev(sc), dev(V), dims=(B, T, D, T), a_strides=(T * T, T, 1), b_strides=(T * D, 1, D))
    close(h, torch.matmul(sc, V), 3e-5, 3e-5)
    a = H.gemm_nt(dev(Kt), dev(Q), dims=(B, D, D, T), a_strides=(T * D, 1, D), b_strides=(T * D, 1, D))
    close(a, torch.matmul(Kt.transpose(1, 2), Q), 3e-5, 3e-5)


def test_row_helpers(H):
    x = torch.randn(3, 18, 96)
    close(H.pixelnorm_dim1(dev(x)), O.pixel_norm(x), 1e-5, 1e-5)
    z = torch.randn(5, 512)
    close(H.pixelnorm_dim1(dev(z)), O.pixel_norm(z), 1e-5, 1e-5)
    a = torch.randn(3, 18, 96)
    g, b = torch.rand(96) + 0.5, torch.randn(96)
    close(H.layernorm(dev(x)), F.layer_norm(x, (96,)), 2e-5, 2e-5)
    close(H.layernorm(dev(x), add=dev(a)), F.layer_norm(x + a, (96,)), 2e-5, 2e-5)
    close(H.layernorm(dev(x), gamma=dev(g), beta=dev(b), post_lrelu=True), F.leaky_relu(F.layer_norm(x, (96,), g, b), 0.2) * math.sqrt(2), 2e-5, 2e-5)
    close(H.softmax_lastdim(dev(x)), torch.softmax(x, -1), 1e-5, 1e-6)
    close(H.softmax_dim1(dev(x)), torch.softmax(x, 1), 1e-5, 1e-6)
    close(H.film(dev(x), dev(a), dev(a * 2)), x * (1 + a) + a * 2, 1e-6, 1e-6)
    c1, c2 = torch.rand(7), torch.rand(7)
    close(H.axpby_idx(dev(x), dev(a), dev(c1), dev(c2), 3), c1[3] * x + c2[3] * a, 1e-6, 1e-6)
    img = torch.randn(2, 5, 12, 16)
    close(H.avgpool2x2(dev(img)), F.avg_pool2d(img, 2), 1e-6, 1e-6)
    close(H.avgpool2x2(dev(img)), F.interpolate(img, (6, 8), mode="bilinear"), 1e-6, 1e-6)
    big = torch.randn(2, 5, 24, 32)
    close(H.upsample_add(dev(img), dev(big)), F.interpolate(img, (24, 32), mode="bilinear", align_corners=True) + big, 1e-5, 1e-5)
    close(H.plane_mean(dev(img)), img.mean((2, 3)), 1e-6, 1e-6)
    gate = torch.rand(2, 5)
    close(H.scale_add(dev(img), dev(gate), dev(img * 3)), img * gate.view(2, 5, 1, 1) + img * 3, 1e-6, 1e-6)
    close(H.subsample(dev(img), 2), img[:, :, ::2, ::2], 0, 0)
    close(H.add3(dev(img), dev(img), dev(img)), img * 3, 1e-6, 1e-6)
    st, wsq = torch.randn(4, 32), torch.rand(24, 32)
    close(H.demod_coefs(dev(st), dev(wsq), 0.1), torch.rsqrt(0.01 * (st ** 2) @ wsq.t() + 1e-8), 2e-5, 1e-6)


def _row_close(got, ref64, ref32, what):
    """max|HIP - float64| <= 4 * e_ref + 2e-6 * max|float64| with e_ref = max|torch fp32 on the CPU - float64| (the rule of
    tests/test_tacc_kernels.py: nothing in the bound comes from the kernel)."""
    got = got.detach().cpu().double()
    assert got.shape == ref64.shape and torch.isfinite(got).all(), what
    e_ref = float((ref32.double() - ref64).abs().max())
    err = float((got - ref64).abs().max())
    tol = 4 * e_ref + 2e-6 * float(ref64.abs().max())
    print(f"ROW {what}: e_ref={e_ref:.3e} e_hip={err:.3e} ratio={err / e_ref if e_ref else float('nan'):.2f} tol={tol:.3e}")
    assert err <= tol, f"{what}: max|d|={err:.3e} tol={tol:.3e} (e_ref {e_ref:.3e})"


@pytest.mark.parametrize("rows", [1, 4, 5, 1025])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 512, 513, 1000])
def test_row_helpers_shapes_and_ranges(H, n, rows):
    """layernorm / softmax_lastdim over rows of length n, softmax_dim1 / pixelnorm_dim1 over a dim 1 of length n with `rows` columns
    behind it, against float64: row lengths around the wave width and off it, row counts around the 4 rows per workgroup, softmax
    inputs with a common offset of +100 and with a spread beyond expf's fp32 range (a lost max gives inf / nan), layernorm rows with
    mean 1e3 and unit variance (a one-pass variance loses everything).  The TACC kernels inline the same reductions.
    Not every printed ratio is under 4: pixelnorm_dim1 over 512 and more rows is at 4 ... 5.6 e_ref (errors of 1 ... 3.5e-6 on values of
    |max| ~5) and passes through the additive 2e-6 * max|ref| term -- its thread sums the squares serially with fmaf, torch pairwise."""
    g = torch.Generator().manual_seed(n * 10000 + rows)

    def draw(*shape):
        return torch.randn(*shape, generator=g, dtype=torch.float64)

    for tag, x in (("n01", draw(rows, n)), ("offset", draw(rows, n) + 100.0), ("spread", draw(rows, n) * 60.0)):
        x = x.float()
        if tag == "spread" and n >= 63:
            assert float(x.max() - x.min()) > 100
        _row_close(H.softmax_lastdim(dev(x)), torch.softmax(x.double(), -1), torch.softmax(x, -1), f"softmax_lastdim {tag} {rows}x{n}")
        x3 = x.t().contiguous().view(1, n, rows)
        _row_close(H.softmax_dim1(dev(x3)), torch.softmax(x3.double(), 1), torch.softmax(x3, 1), f"softmax_dim1 {tag} 1x{n}x{rows}")
    x = draw(2, n, rows).float() * 3
    _row_close(H.softmax_dim1(dev(x)), torch.softmax(x.double(), 1), torch.softmax(x, 1), f"softmax_dim1 2x{n}x{rows}")
    _row_close(H.pixelnorm_dim1(dev(x)), O.pixel_norm(x.double()), O.pixel_norm(x), f"pixelnorm_dim1 2x{n}x{rows}")
    for tag, x in (("n01", draw(rows, n)), ("mean1e3", draw(rows, n) + 1e3)):
        x = x.float()
        a = draw(rows, n).float()
        gm, bt = (torch.rand(n, generator=g, dtype=torch.float64) + 0.5).float(), draw(n).float()
        _row_close(H.layernorm(dev(x)), F.layer_norm(x.double(), (n,)), F.layer_norm(x, (n,)), f"layernorm {tag} {rows}x{n}")
        _row_close(H.layernorm(dev(x), add=dev(a)), F.layer_norm(x.double() + a.double(), (n,)), F.layer_norm(x + a, (n,)),
                   f"layernorm add {tag} {rows}x{n}")
        _row_close(H.layernorm(dev(x), gamma=dev(gm), beta=dev(bt), post_lrelu=True),
                   F.leaky_relu(F.layer_norm(x.double(), (n,), gm.double(), bt.double()), 0.2) * math.sqrt(2),
                   F.leaky_relu(F.layer_norm(x, (n,), gm, bt), 0.2) * math.sqrt(2), f"layernorm affine {tag} {rows}x{n}")


def test_linear_many_rows_is_row_independent(H):
    """The small-GEMM kernel's wide form (M >= 1024: four row blocks per workgroup share the B fragments): against float64, and
    BIT-identical to the same rows computed in slices that take the one-block form (an image's result must not depend on the batch)."""
    g_ = torch.Generator().manual_seed(43)
    M, K, N = 1300, 512, 96
    x, w, b = torch.randn(M, K, generator=g_), torch.randn(N, K, generator=g_) * 0.05, torch.randn(N, generator=g_)
    ref = torch.sigmoid(x.double() @ w.double().t() + b.double()).float()
    y = H.linear(dev(x), dev(w), dev(b), act=2)
    close(y, ref, 1e-5, 1e-6, "wide form")
    parts = torch.cat([H.linear(dev(x[i:i + 900]), dev(w), dev(b), act=2) for i in range(0, M, 900)], 0)
    assert torch.equal(y, parts)


def test_conv2d_true_groups_and_batched_head_gemm(H):
    """Grouped convolution with per-group input slices (the batched map2style heads) + the batched per-head linear."""
    for G in (3, 5):
        _grouped_case(H, G)


def _grouped_case(H, G):
    B, C_, Hh = 2, 16, 8
    x = torch.randn(B, G * C_, Hh, Hh)
    ws = [torch.randn(C_, C_, 3, 3) / math.sqrt(C_ * 9) for _ in range(G)]
    bias = torch.randn(G * C_)
    ref = F.leaky_relu(F.conv2d(x, torch.cat(ws, 0), bias, stride=2, padding=1, groups=G), 0.01)
    wp = torch.stack([H.pack_weight(dev(w_))[0] for w_ in ws]).contiguous()
    pc = H.PackedConv(wp, G, C_, C_, 3, 3, 2, (1,), (1,), x_group_stride=C_)
    y = H.conv2d_packed(dev(x), pc, ch_bias=dev(bias), act2=1, slope2=0.01, gain2=1.0)
    close(y, ref, 2e-5, 2e-5)
    feat = torch.randn(B, G * C_)
    lw, lb = torch.randn(G, 24, C_), torch.randn(G, 24)
    out = H.gemm_nt(dev(feat), dev(lw), dims=(G, B, 24, C_), a_strides=(C_, G * C_, 1), b_strides=(24 * C_, C_, 1), alpha=0.5,
                    bias=dev(lb), bias_scale=2.0, bias_zs=24)
    ref2 = torch.stack([F.linear(feat[:, g * C_:(g + 1) * C_], lw[g] * 0.5, lb[g] * 2.0) for g in range(G)])
    close(out, ref2, 2e-5, 2e-5)


@pytest.mark.parametrize("B,Cin,Cout,Hh,Ww", [(2, 32, 3, 64, 64), (1, 7, 3, 5, 9), (2, 3, 64, 33, 31), (1, 512, 3, 16, 16), (2, 4, 20, 8, 8)])
def test_pointwise_stream_kernels(H, B, Cin, Cout, Hh, Ww):
    """ToRGB (few outputs: style scale, bias, skip residual) and the 3 -> 64 input layer (few inputs: two FusedLeakyReLUs)."""
    x = torch.randn(B, Cin, Hh, Ww)
    w = torch.randn(Cout, Cin) / math.sqrt(Cin)
    s_in = torch.rand(B, Cin) + 0.5
    lin = torch.einsum("bchw,oc->bohw", x * s_in.view(B, Cin, 1, 1), w)
    if Cout <= 4:
        cb, res = torch.randn(Cout), torch.randn(B, Cout, Hh, Ww)
        close(H.pointwise(dev(x), dev(w), in_scale=dev(s_in), ch_bias=dev(cb), res=dev(res)), lin + cb.view(1, -1, 1, 1) + res,
              2e-5, 2e-5)
        close(H.pointwise(dev(x), dev(w)), torch.einsum("bchw,oc->bohw", x, w), 2e-5, 2e-5)
        if Hh % 2 == 0 and Ww % 2 == 0:  # the FIR-upsampled skip evaluated inside the kernel
            from vspbfr_amd.op import upfirdn2d
            k1 = torch.tensor([1., 3., 3., 1.])
            k = k1[:, None] * k1[None, :]
            k = k / k.sum() * 4
            skip = torch.randn(B, Cout, Hh // 2, Ww // 2)
            up = upfirdn2d(dev(skip), dev(k), up=2, down=1, pad=(2, 1)).cpu()
            close(H.pointwise(dev(x), dev(w), in_scale=dev(s_in), ch_bias=dev(cb), up_src=dev(skip), up_kernel=dev(k)),
                  lin + cb.view(1, -1, 1, 1) + up, 2e-5, 2e-5)
    else:
        b1, b2 = torch.randn(Cout), torch.randn(Cout)
        ref = F.leaky_relu(lin + b1.view(1, -1, 1, 1), 0.2) * math.sqrt(2)
        ref = F.leaky_relu(ref + b2.view(1, -1, 1, 1), 0.2) * math.sqrt(2)
        close(H.pointwise(dev(x), dev(w), in_scale=dev(s_in), bias1=dev(b1), bias2=dev(b2)), ref, 2e-5, 2e-5)
    with pytest.raises(RuntimeError):
        H.pointwise(dev(torch.randn(1, 8, 4, 4)), dev(torch.randn(8, 8)))


@pytest.mark.parametrize("shape,with_bias", [((2, 8, 9, 7), True), ((3, 16), True), ((2, 4, 6, 6), False)])
@torch.enable_grad()
def test_fused_leaky_relu_autograd_any_order(H, shape, with_bias):
    """first and second derivatives of the op against torch autograd over the oracle's formula."""
    from oracle import ops as O
    from vspbfr_amd.op import fused_leaky_relu
    x = torch.randn(*shape, dtype=torch.float32)
    b = torch.randn(shape[1]) if with_bias else None
    g = torch.randn(*shape)
    xr, br = x.clone().requires_grad_(True), (b.clone().requires_grad_(True) if with_bias else None)
    xd, bd = dev(x).requires_grad_(True), (dev(b).requires_grad_(True) if with_bias else None)
    yr, yd = O.fused_leaky_relu(xr, br), fused_leaky_relu(xd, bd)
    close(yd.detach(), yr.detach(), 1e-6, 1e-6)
    ins_r, ins_d = ([xr, br] if with_bias else [xr]), ([xd, bd] if with_bias else [xd])
    gr = torch.autograd.grad(yr, ins_r, g)
    gd = torch.autograd.grad(yd, ins_d, dev(g))
    for a, r in zip(gd, gr):
        close(a.detach(), r.detach(), 1e-5, 1e-5)
    # second order: d/dg of <grad_x, v> (the mask is piecewise constant: only the g path carries curvature-free terms)
    v = torch.randn(*shape)
    g2r = torch.randn(*shape).requires_grad_(True)
    g2d = dev(g2r.detach()).requires_grad_(True)
    hr = torch.autograd.grad(O.fused_leaky_relu(xr, br), xr, g2r, create_graph=True)[0]
    hd = torch.autograd.grad(fused_leaky_relu(xd, bd), xd, g2d, create_graph=True)[0]
    close(torch.autograd.grad(hd, g2d, dev(v))[0], torch.autograd.grad(hr, g2r, v)[0], 1e-5, 1e-5)


@pytest.mark.parametrize("up,down,pad,k", [(1, 1, (1, 1), 4), (2, 1, (2, 1), 4), (1, 2, (2, 2), 4), (1, 1, (2, 2), 4), (2, 1, (1, 0), 2),
                                             (1, 1, (-1, 2), 3)])
@torch.enable_grad()
def test_upfirdn2d_autograd_any_order(H, up, down, pad, k):
    from oracle import ops as O
    from vspbfr_amd.op import upfirdn2d
    x = torch.randn(2, 3, 11, 9)
    kern = torch.rand(k, k) + 0.1
    xr, xd = x.clone().requires_grad_(True), dev(x).requires_grad_(True)
    yr, yd = O.upfirdn2d(xr, kern, up=up, down=down, pad=pad), upfirdn2d(xd, dev(kern), up=up, down=down, pad=pad)
    close(yd.detach(), yr.detach(), 1e-5, 1e-5)
    g = torch.randn_like(yr).requires_grad_(True)
    gdv = dev(g.detach()).requires_grad_(True)
    gr = torch.autograd.grad(yr, xr, g, create_graph=True)[0]
    gd = torch.autograd.grad(yd, xd, gdv, create_graph=True)[0]
    assert gd.shape == xd.shape
    close(gd.detach(), gr.detach(), 1e-5, 1e-5)
    v = torch.randn_like(x)
    close(torch.autograd.grad(gd, gdv, dev(v))[0], torch.autograd.grad(gr, g, v)[0], 1e-5, 1e-5)   # double backward


@pytest.mark.parametrize("B,Cin,Cout,Hh,Ww", [(2, 8, 64, 16, 16), (1, 20, 36, 13, 29), (2, 64, 64, 32, 32), (1, 256, 128, 16, 24),
                                               (1, 3, 4, 7, 5), (1, 24, 40, 20, 36), (2, 16, 32, 40, 24), (1, 12, 96, 34, 52)])
def test_conv2d_winograd(H, B, Cin, Cout, Hh, Ww):
    """F(2x2,3x3) kernel against F.conv2d, with the whole prologue / epilogue chain of a StyledConv."""
    x = torch.randn(B, Cin, Hh, Ww)
    w = torch.randn(Cout, Cin, 3, 3) / math.sqrt(Cin * 9)
    pc = H.PackedConv(H.pack_weight(dev(w)), 1, Cout, Cin, 3, 3, 1, (1,), (1,))
    close(H.conv2d_packed(dev(x), pc, winograd=True), F.conv2d(x, w, padding=1), 3e-5, 3e-5)
    s_in, demod, bias = torch.rand(B, Cin) + 0.5, torch.rand(B, Cout) + 0.5, torch.randn(Cout)
    nz, nw = torch.randn(B, 1, Hh, Ww), torch.tensor([0.7])
    r1, r2 = torch.randn(B, Cout, Hh, Ww), torch.randn(B, Cout, Hh, Ww)
    ref = F.conv2d(x * s_in.view(B, Cin, 1, 1), w, padding=1) * demod.view(B, Cout, 1, 1) + nz * nw
    ref = F.leaky_relu(ref + bias.view(1, -1, 1, 1), 0.2) * math.sqrt(2) + r1 + r2
    y = H.conv2d_packed(dev(x), pc, in_scale=dev(s_in), out_scale=dev(demod), noise=dev(nz), noise_w=dev(nw), act2=1,
                        bias2=dev(bias), res1=dev(r1), res2=dev(r2), winograd=True)
    close(y, ref, 5e-5, 5e-5)
    # folded BatchNorm input (scale + shift, zero padding AFTER the affine map) and PReLU, as in the IR-SE50 body
    a, sh, pr = torch.rand(Cin) + 0.5, torch.randn(Cin), torch.rand(Cout) * 0.3
    ref2 = F.prelu(F.conv2d(x * a.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1), w, padding=1), pr)
    y2 = H.conv2d_packed(dev(x), pc, in_scale=dev(a), in_scale_per_sample=False, in_shift=dev(sh), act2=2, prelu=dev(pr),
                         winograd=True)
    close(y2, ref2, 5e-5, 5e-5)
    with pytest.raises(RuntimeError):
        H.conv2d_packed(dev(x), H.PackedConv(H.pack_weight(dev(w)), 1, Cout, Cin, 3, 3, 2, (1,), (1,)), winograd=True)


@pytest.mark.parametrize("B,Cin,Cout,Hh,Ww", [(2, 64, 64, 32, 32), (1, 20, 40, 36, 48), (2, 8, 72, 16, 64), (1, 256, 128, 24, 40),
                                               (3, 12, 200, 8, 16)])
def test_conv2d_winograd4(H, B, Cin, Cout, Hh, Ww):
    """F(4x4,3x3) pair (vsp_conv2d_winograd4_f32: input transform + barrier-free GEMM) against float64 F.conv2d: plain, and with the whole
    prologue / epilogue chain of a StyledConv; partial pixel tiles (H, W not multiples of 16 / 32), partial channel tiles and chunks."""
    g_ = torch.Generator().manual_seed(Cin * 7 + Cout)
    x = torch.randn(B, Cin, Hh, Ww, generator=g_)
    w = torch.randn(Cout, Cin, 3, 3, generator=g_) / math.sqrt(Cin * 9)
    pc = H.PackedConv(H.pack_weight(dev(w)), 1, Cout, Cin, 3, 3, 1, (1,), (1,))
    assert H.winograd4_eligible(pc, Hh, Ww, Hh, Ww)
    close(H.conv2d_packed(dev(x), pc, winograd=4), F.conv2d(x.double(), w.double(), padding=1).float(), 5e-5, 5e-5)
    s_in, demod, bias = torch.rand(B, Cin, generator=g_) + 0.5, torch.rand(B, Cout, generator=g_) + 0.5, torch.randn(Cout, generator=g_)
    nz, nw = torch.randn(B, 1, Hh, Ww, generator=g_), torch.tensor([0.7])
    r1, r2 = torch.randn(B, Cout, Hh, Ww, generator=g_), torch.randn(B, Cout, Hh, Ww, generator=g_)
    ref = F.conv2d((x * s_in.view(B, Cin, 1, 1)).double(), w.double(), padding=1) * demod.view(B, Cout, 1, 1).double() + (nz * nw).double()
    ref = (F.leaky_relu(ref + bias.view(1, -1, 1, 1).double(), 0.2) * math.sqrt(2) + r1.double() + r2.double()).float()
    kw = dict(in_scale=dev(s_in), out_scale=dev(demod), noise=dev(nz), noise_w=dev(nw), act2=1, bias2=dev(bias), res1=dev(r1), res2=dev(r2))
    y = H.conv2d_packed(dev(x), pc, winograd=4, **kw)
    close(y, ref, 6e-5, 6e-5)
    # written into a channel window of a wider tensor
    out = torch.full((B, Cout + 5, Hh, Ww), 7.0, device=DEV)
    H.conv2d_packed(dev(x), pc, out=out, y_coff=3, winograd=4)
    close(out[:, 3:3 + Cout], F.conv2d(x, w, padding=1), 6e-5, 6e-5)
    assert bool((out[:, :3] == 7.0).all()) and bool((out[:, 3 + Cout:] == 7.0).all())
    # what the deep-layer form does not serve goes to F(2x2,3x3): an affine input shift, maps that are not whole 4 x 4 tiles
    a, sh = torch.rand(Cin) + 0.5, torch.randn(Cin)
    y2 = H.conv2d_packed(dev(x), pc, in_scale=dev(a), in_scale_per_sample=False, in_shift=dev(sh), winograd=4)
    close(y2, F.conv2d(x * a.view(1, -1, 1, 1) + sh.view(1, -1, 1, 1), w, padding=1), 5e-5, 5e-5)
    x3 = torch.randn(1, Cin, 18, 22)
    assert not H.winograd4_eligible(pc, 18, 22, 18, 22)
    close(H.conv2d_packed(dev(x3), pc, winograd=4), F.conv2d(x3, w, padding=1), 5e-5, 5e-5)


def test_conv2d_winograd4_refusals(H):
    """The C entry refuses what it cannot serve (VSP_ENOTSUP / VSP_EINVAL through RuntimeError), it does not compute something else."""
    from vspbfr_amd import _lib
    x = dev(torch.randn(1, 8, 16, 32))
    w = dev(torch.randn(64, 8, 3, 3))
    pc = H.PackedConv(H.pack_weight(w), 1, 64, 8, 3, 3, 1, (1,), (1,))
    u4 = pc.form("wino4")
    assert u4.numel() == _lib.lib.vsp_winograd4_weight_floats(8, 64)
    p = _lib.ConvParams()
    out = torch.empty(1, 64, 16, 32, device=DEV)
    p.x, p.w, p.y = x.data_ptr(), u4.data_ptr(), out.data_ptr()
    p.B, p.Cin, p.H, p.W, p.G, p.cout_g, p.OH, p.OW, p.KH, p.KW = 1, 8, 16, 32, 1, 64, 16, 32, 3, 3
    p.stride_y = p.stride_x = 1
    for g in range(4):
        p.dil[g], p.pad_y[g], p.pad_x[g] = 1, 1, 1
    p.y_ch, p.y_h, p.y_w, p.osy, p.osx, p.x_ch = 64, 16, 32, 1, 1, 8
    import ctypes as C
    nfl = _lib.lib.vsp_conv2d_winograd4_work_floats(C.byref(p))
    work = torch.empty(nfl, device=DEV)
    assert _lib.lib.vsp_conv2d_winograd4_f32(C.byref(p), work.data_ptr(), nfl, None) == 0
    torch.cuda.synchronize()
    close(out, F.conv2d(x.cpu(), w.cpu(), padding=1), 5e-5, 5e-5)
    assert _lib.lib.vsp_conv2d_winograd4_f32(C.byref(p), work.data_ptr(), nfl - 1, None) != 0          # work buffer too small
    p.dil[0] = p.pad_y[0] = p.pad_x[0] = 2
    assert _lib.lib.vsp_conv2d_winograd4_f32(C.byref(p), work.data_ptr(), nfl, None) != 0              # dilation
    p.dil[0] = p.pad_y[0] = p.pad_x[0] = 1
    p.stride_y = p.stride_x = 2
    assert _lib.lib.vsp_conv2d_winograd4_f32(C.byref(p), work.data_ptr(), nfl, None) != 0              # stride
    p.stride_y = p.stride_x = 1
    p.y = out.data_ptr() + 4
    assert _lib.lib.vsp_conv2d_winograd4_f32(C.byref(p), work.data_ptr(), nfl, None) == -3             # VSP_ENOTSUP: output not 16-byte aligned


@pytest.mark.parametrize("cin,cout", [(64, 64), (6, 3), (30, 72), (130, 40)])
def test_winograd4_weight_kernel(H, cin, cout):
    """vsp_winograd4_weight_f32 against U = G g G^T in float64 (points 0, +-3/4, +-3/2, inf) in the fragment order include/vspbfr_hip.h
    states for vsp_conv2d_winograd4_f32, zero padding included."""
    g_ = torch.Generator().manual_seed(17)
    wp = torch.randn(1, 9, cin, cout, generator=g_)
    Gm = torch.tensor(((64 / 81, 0, 0), (-128 / 243, -32 / 81, -8 / 27), (-128 / 243, 32 / 81, -8 / 27), (32 / 243, 16 / 81, 8 / 27),
                       (32 / 243, -16 / 81, 8 / 27), (0, 0, 1)), dtype=torch.float64)
    U = torch.einsum("ay,bx,yxio->abio", Gm, Gm, wp[0].double().view(3, 3, cin, cout)).reshape(36, cin, cout)
    nch, nct = (cin + 3) // 4, (cout + 63) // 64
    Up = U.new_zeros(36, nch * 4, nct * 64)
    Up[:, :cin, :cout] = U
    # [tile][chunk][wave 12][q 3][lane = kq 4 x lr 16][mb 4]  <-  U[pos = 3 wave + q][ci = 4 chunk + kq][co = 64 tile + 16 mb + lr]
    ref = Up.view(12, 3, nch, 4, nct, 4, 16).permute(4, 2, 0, 1, 3, 6, 5).float().contiguous().view(-1)
    got = H.winograd4_weight(dev(wp)).cpu()
    assert got.numel() == ref.numel() == H.lib.vsp_winograd4_weight_floats(cin, cout)
    close(got, ref, 1e-7, 1.2e-7, "winograd4 weight")


@pytest.mark.parametrize("B,Cin,Cg,Hh,Ww", [(2, 16, 8, 24, 24), (1, 24, 16, 37, 21), (2, 64, 32, 32, 32), (1, 40, 64, 16, 48), (1, 32, 128, 19, 19)])
def test_conv2d_winograd_dilation_groups(H, B, Cin, Cg, Hh, Ww):
    """The four dilated SMART branches through the polyphase Winograd kernel (one launch, all three channel-block variants)."""
    x = torch.randn(B, Cin, Hh, Ww)
    ws = [torch.randn(Cg, Cin, 3, 3) / math.sqrt(Cin * 9) for _ in range(4)]
    s_in, demod, bias = torch.rand(B, Cin) + 0.5, torch.rand(B, 4 * Cg) + 0.5, torch.randn(4 * Cg)
    xs = x * s_in.view(B, Cin, 1, 1)
    ref = torch.cat([F.conv2d(xs, w_, padding=d, dilation=d) for w_, d in zip(ws, (1, 2, 4, 8))], dim=1)
    ref = F.leaky_relu(ref * demod.view(B, -1, 1, 1) + bias.view(1, -1, 1, 1), 0.2) * math.sqrt(2)
    wp = torch.stack([H.pack_weight(dev(w_))[0] for w_ in ws]).contiguous()
    pc = H.PackedConv(wp, 4, Cg, Cin, 3, 3, 1, (1, 2, 4, 8), (1, 2, 4, 8))
    y = H.conv2d_packed(dev(x), pc, in_scale=dev(s_in), out_scale=dev(demod), act2=1, bias2=dev(bias), winograd=True)
    close(y, ref, 5e-5, 5e-5)
    # a single dilated conv (G = 1, d = 2)
    pc1 = H.PackedConv(H.pack_weight(dev(ws[1])), 1, Cg, Cin, 3, 3, 1, (2,), (2,))
    close(H.conv2d_packed(dev(x), pc1, winograd=True), F.conv2d(x, ws[1], padding=2, dilation=2), 5e-5, 5e-5)


def _bf(t):
    """round to bf16 (RNE) and back: what vsp_conv2d_bf16 feeds the matrix pipe"""
    return t.to(torch.bfloat16).float()


@pytest.mark.parametrize("variant", [0, 1, 2, 3, 4, 6, 7])
@pytest.mark.parametrize("B,Cin,Cout,Hh,Ww", [(2, 16, 64, 32, 32), (1, 40, 36, 13, 29), (2, 64, 64, 64, 64), (1, 256, 128, 16, 24),
                                               (1, 32, 160, 8, 8), (1, 64, 32, 70, 45)])
def test_conv2d_bf16(H, B, Cin, Cout, Hh, Ww, variant):
    """bf16-MFMA kernel: exact (to fp32 summation order) against F.conv2d on the bf16-rounded operands it documents, every
    tile variant, with the prologue / epilogue chain of a StyledConv; and within bf16 rounding of the fp32 result."""
    x = torch.randn(B, Cin, Hh, Ww)
    w = torch.randn(Cout, Cin, 3, 3) / math.sqrt(Cin * 9)
    pc = H.PackedConv(H.pack_weight(dev(w)), 1, Cout, Cin, 3, 3, 1, (1,), (1,))
    y = H.conv2d_packed(dev(x), pc, bf16=True, tile_hint=variant)
    close(y, F.conv2d(_bf(x), _bf(w), padding=1), 2e-5, 2e-5, "plain")
    close(y, F.conv2d(x, w, padding=1), 2e-2, 2e-2, "vs fp32")
    s_in, demod, bias = torch.rand(B, Cin) + 0.5, torch.rand(B, Cout) + 0.5, torch.randn(Cout)
    nz, nw = torch.randn(B, 1, Hh, Ww), torch.tensor([0.7])
    r1, r2 = torch.randn(B, Cout, Hh, Ww), torch.randn(B, Cout, Hh, Ww)
    ref = F.conv2d(_bf(x * s_in.view(B, Cin, 1, 1)), _bf(w), padding=1) * demod.view(B, Cout, 1, 1) + nz * nw
    ref = F.leaky_relu(ref + bias.view(1, -1, 1, 1), 0.2) * math.sqrt(2) + r1 + r2
    y = H.conv2d_packed(dev(x), pc, in_scale=dev(s_in), out_scale=dev(demod), noise=dev(nz), noise_w=dev(nw), act2=1,
                        bias2=dev(bias), res1=dev(r1), res2=dev(r2), bf16=True, tile_hint=variant)
    close(y, ref, 5e-5, 5e-5, "styled")
    a, sh, pr = torch.rand(Cin) + 0.5, torch.randn(Cin), torch.rand(Cout) * 0.3
    xa = (x.double() * a.view(1, -1, 1, 1).double() + sh.view(1, -1, 1, 1).double()).float()  # = the kernel's fmaf (one rounding)
    ref2 = F.prelu(F.conv2d(_bf(xa), _bf(w), padding=1), pr)
    y2 = H.conv2d_packed(dev(x), pc, in_scale=dev(a), in_scale_per_sample=False, in_shift=dev(sh), act2=2, prelu=dev(pr),
                         bf16=True, tile_hint=variant)
    close(y2, ref2, 5e-5, 5e-5, "bn+prelu")


@pytest.mark.parametrize("B,Cin,Cg,Hh,Ww", [(2, 16, 8, 24, 24), (1, 32, 16, 37, 21), (2, 64, 32, 64, 64), (1, 48, 64, 16, 48), (1, 32, 128, 19, 19)])
def test_conv2d_bf16_dilation_groups(H, B, Cin, Cg, Hh, Ww):
    """The four dilated SMART branches in one launch of the bf16 kernel (polyphase sub-images), into a channel slice."""
    x = torch.randn(B, Cin, Hh, Ww)
    ws = [torch.randn(Cg, Cin, 3, 3) / math.sqrt(Cin * 9) for _ in range(4)]
    s_in, demod, bias = torch.rand(B, Cin) + 0.5, torch.rand(B, 4 * Cg) + 0.5, torch.randn(4 * Cg)
    xs = _bf(x * s_in.view(B, Cin, 1, 1))
    ref = torch.cat([F.conv2d(xs, _bf(w_), padding=d, dilation=d) for w_, d in zip(ws, (1, 2, 4, 8))], dim=1)
    ref = F.leaky_relu(ref * demod.view(B, -1, 1, 1) + bias.view(1, -1, 1, 1), 0.2) * math.sqrt(2)
    wp = torch.stack([H.pack_weight(dev(w_))[0] for w_ in ws]).contiguous()
    pc = H.PackedConv(wp, 4, Cg, Cin, 3, 3, 1, (1, 2, 4, 8), (1, 2, 4, 8))
    out = torch.full((B, 4 * Cg + 3, Hh, Ww), 7.0, device=DEV)
    H.conv2d_packed(dev(x), pc, out=out, y_coff=2, in_scale=dev(s_in), out_scale=dev(demod), act2=1, bias2=dev(bias), bf16=True)
    close(out[:, 2:2 + 4 * Cg], ref, 5e-5, 5e-5)
    assert (out[:, :2] == 7.0).all() and (out[:, -1] == 7.0).all()
    with pytest.raises(RuntimeError):
        H.conv2d_packed(dev(x), H.PackedConv(H.pack_weight(dev(ws[0])), 1, Cg, Cin, 3, 3, 2, (2,), (2,)), bf16=True)  # stride 2 AND dilation


@pytest.mark.parametrize("B,Cin,Cout,Hh,Ww,pad,variant", [(2, 16, 64, 33, 33, 0, 4), (1, 64, 128, 65, 65, 0, 6), (2, 64, 128, 64, 64, 1, 0),
                                                       (1, 48, 40, 37, 29, 1, 4), (1, 256, 256, 16, 16, 1, 6), (1, 32, 64, 129, 129, 0, 0)])
def test_conv2d_bf16_stride2(H, B, Cin, Cout, Hh, Ww, pad, variant):
    """stride-2 mode (parity planes): StyledConv_down after its blur (padding 0) and the IR-SE / style-head down-convs (1)."""
    x = torch.randn(B, Cin, Hh, Ww)
    w = torch.randn(Cout, Cin, 3, 3) / math.sqrt(Cin * 9)
    s_in, demod, bias = torch.rand(B, Cin) + 0.5, torch.rand(B, Cout) + 0.5, torch.randn(Cout)
    pc = H.PackedConv(H.pack_weight(dev(w)), 1, Cout, Cin, 3, 3, 2, (1,), (pad,))
    ref = F.conv2d(_bf(x * s_in.view(B, Cin, 1, 1)), _bf(w), stride=2, padding=pad)
    nz, nw = torch.randn(B, 1, ref.shape[2], ref.shape[3]), torch.tensor([0.3])
    ref = F.leaky_relu(ref * demod.view(B, Cout, 1, 1) + nz * nw + bias.view(1, -1, 1, 1), 0.2) * math.sqrt(2)
    y = H.conv2d_packed(dev(x), pc, in_scale=dev(s_in), out_scale=dev(demod), noise=dev(nz), noise_w=dev(nw), act2=1,
                        bias2=dev(bias), bf16=True, tile_hint=variant)
    close(y, ref, 5e-5, 5e-5)


def test_conv2d_bf16_stride2_true_groups(H):
    """the batched e4e style heads: G groups, each with its own input slice, stride 2, padding 1, LeakyReLU(0.01)"""
    B, G, Cin, Cg, S = 2, 3, 32, 48, 16
    x = torch.randn(B, G * Cin, S, S)
    ws = [torch.randn(Cg, Cin, 3, 3) / math.sqrt(Cin * 9) for _ in range(G)]
    bias = torch.randn(G * Cg)
    ref = torch.cat([F.conv2d(_bf(x[:, g * Cin:(g + 1) * Cin]), _bf(ws[g]), stride=2, padding=1) for g in range(G)], 1)
    ref = F.leaky_relu(ref + bias.view(1, -1, 1, 1), 0.01)
    wp = torch.stack([H.pack_weight(dev(w_))[0] for w_ in ws]).contiguous()
    pc = H.PackedConv(wp, G, Cg, Cin, 3, 3, 2, (1,), (1,), x_group_stride=Cin)
    y = H.conv2d_packed(dev(x), pc, ch_bias=dev(bias), act2=1, slope2=0.01, gain2=1.0, bf16=True)
    close(y, ref, 5e-5, 5e-5)


@pytest.mark.parametrize("B,Cin,Cout,Hh,Ww,variant", [(2, 16, 64, 32, 32, 4), (1, 64, 32, 64, 64, 5), (1, 40, 72, 13, 21, 0), (2, 128, 64, 16, 16, 0),
                                                   (1, 32, 32, 70, 33, 0), (1, 48, 40, 37, 66, 8)])
def test_conv2d_bf16_transposed(H, B, Cin, Cout, Hh, Ww, variant):
    """stride-2 transposed conv in one pass on the bf16 pipe, against F.conv_transpose2d on the bf16-rounded operands"""
    x = torch.randn(B, Cin, Hh, Ww)
    w = torch.randn(Cout, Cin, 3, 3) / math.sqrt(Cin * 9)
    s_in, demod = torch.rand(B, Cin) + 0.5, torch.rand(B, Cout) + 0.5
    pc = H.PackedConv(H.pack_weight(dev(w)), 1, Cout, Cin, 3, 3, 1, (1,), (1,))
    ref = F.conv_transpose2d(_bf(x * s_in.view(B, Cin, 1, 1)), _bf(w).transpose(0, 1), stride=2) * demod.view(B, Cout, 1, 1)
    y = H.conv_transpose2d_s2_fused(dev(x), pc, in_scale=dev(s_in), out_scale=dev(demod), bf16=True, tile_hint=variant)
    close(y, ref, 5e-5, 5e-5)


def test_conv2d_bf16_empty_batch_and_errors(H):
    """edge cases of the bf16 entry: an empty batch is a no-op, ineligible layers raise RuntimeError (no silent fp32 fallback
    when bf16=True is asked for explicitly)"""
    w = torch.randn(32, 16, 3, 3)
    pc = H.PackedConv(H.pack_weight(dev(w)), 1, 32, 16, 3, 3, 1, (1,), (1,))
    y = H.conv2d_packed(torch.empty(0, 16, 8, 8, device=DEV), pc, bf16=True)
    assert y.shape == (0, 32, 8, 8)
    pc1 = H.PackedConv(H.pack_weight(dev(torch.randn(32, 16, 1, 1))), 1, 32, 16, 1, 1, 1, (1,), (0,))
    with pytest.raises(RuntimeError):
        H.conv2d_packed(torch.randn(1, 16, 8, 8, device=DEV), pc1, bf16=True)
    pc12 = H.PackedConv(H.pack_weight(dev(torch.randn(32, 12, 3, 3))), 1, 32, 12, 3, 3, 1, (1,), (1,))
    with pytest.raises(RuntimeError):
        H.conv2d_packed(torch.randn(1, 12, 8, 8, device=DEV), pc12, bf16=True)


@pytest.mark.parametrize("variant", [0, 1, 4, 7])
@pytest.mark.parametrize("B,Cin,Cout,Hh,Ww", [(2, 16, 64, 32, 32), (1, 40, 36, 13, 29), (1, 256, 128, 16, 24), (1, 64, 32, 70, 45)])
def test_conv2d_bf16x3(H, B, Cin, Cout, Hh, Ww, variant):
    """split-precision form: hi + lo bf16 operands, three MFMAs per product -- fp32-grade against F.conv2d in float64"""
    x = torch.randn(B, Cin, Hh, Ww)
    w = torch.randn(Cout, Cin, 3, 3) / math.sqrt(Cin * 9)
    s_in, demod, bias = torch.rand(B, Cin) + 0.5, torch.rand(B, Cout) + 0.5, torch.randn(Cout)
    pc = H.PackedConv(H.pack_weight(dev(w)), 1, Cout, Cin, 3, 3, 1, (1,), (1,))
    ref = F.conv2d((x * s_in.view(B, Cin, 1, 1)).double(), w.double(), padding=1) * demod.view(B, Cout, 1, 1).double()
    ref = (F.leaky_relu(ref + bias.view(1, -1, 1, 1).double(), 0.2) * math.sqrt(2)).float()
    y = H.conv2d_packed(dev(x), pc, in_scale=dev(s_in), out_scale=dev(demod), act2=1, bias2=dev(bias), bf16="x3", tile_hint=variant)
    close(y, ref, 6e-5, 6e-5)      # 2^-16 per product; plain bf16 operands sit at 2e-2 on the same data
    # stride 2 (parity planes) and the four dilation groups
    pc2 = H.PackedConv(H.pack_weight(dev(w)), 1, Cout, Cin, 3, 3, 2, (1,), (1,))
    close(H.conv2d_packed(dev(x), pc2, bf16="x3"), F.conv2d(x.double(), w.double(), stride=2, padding=1).float(), 6e-5, 6e-5)
    if Cout % 4 == 0:
        ws = [torch.randn(Cout // 4, Cin, 3, 3) / math.sqrt(Cin * 9) for _ in range(4)]
        wp = torch.stack([H.pack_weight(dev(w_))[0] for w_ in ws]).contiguous()
        pc4 = H.PackedConv(wp, 4, Cout // 4, Cin, 3, 3, 1, (1, 2, 4, 8), (1, 2, 4, 8))
        ref4 = torch.cat([F.conv2d(x.double(), w_.double(), padding=d, dilation=d) for w_, d in zip(ws, (1, 2, 4, 8))], 1).float()
        close(H.conv2d_packed(dev(x), pc4, bf16="x3"), ref4, 6e-5, 6e-5)


@pytest.mark.parametrize("B,Cin,Cout,Hh,Ww", [(2, 16, 64, 32, 32), (1, 40, 72, 13, 21), (1, 128, 64, 33, 64)])
def test_conv2d_bf16x3_transposed(H, B, Cin, Cout, Hh, Ww):
    """split-precision transposed mode against F.conv_transpose2d in float64"""
    x = torch.randn(B, Cin, Hh, Ww)
    w = torch.randn(Cout, Cin, 3, 3) / math.sqrt(Cin * 9)
    s_in, demod = torch.rand(B, Cin) + 0.5, torch.rand(B, Cout) + 0.5
    pc = H.PackedConv(H.pack_weight(dev(w)), 1, Cout, Cin, 3, 3, 1, (1,), (1,))
    ref = (F.conv_transpose2d((x * s_in.view(B, Cin, 1, 1)).double(), w.double().transpose(0, 1), stride=2)
           * demod.view(B, Cout, 1, 1).double()).float()
    y = H.conv_transpose2d_s2_fused(dev(x), pc, in_scale=dev(s_in), out_scale=dev(demod), bf16="x3")
    close(y, ref, 6e-5, 6e-5)


# ------------------------------------------------------------------------------------------------ keyed random tensors
def test_keyed_fill_matches_restatement_and_is_shard_invariant(H):
    """vsp_keyed_fill_f32 against oracle/device_rng.py (Philox4x32-10 words are integer arithmetic: any mismatch there shows
    as an O(1) difference; Box-Muller differs by libm rounding only), several tensors in one launch incl. a ragged one, and
    the sharding property: images [lo, hi) drawn alone equal rows lo..hi-1 of the full batch, bit for bit."""
    from oracle import device_rng as R
    shapes = [(5, 1, 32, 32), (5, 18, 512), (5, 512), (5, 1, 4, 4), (5, 7)]   # (5, 7): per-image size not a multiple of 4, last
    ids = [H.SEG_GEN + 3, H.SEG_XT, H.SEG_Z, H.SEG_ENC, 999]
    seed, i0 = 0x1234_5678_9ABC_DEF0, (1 << 33) + 11                          # 64-bit seed and image index both reach the counter
    full = H.keyed_fill(shapes, ids, seed, i0)
    for t, s, i in zip(full, shapes, ids):
        assert t.shape == s and t.is_contiguous()
        close(t, R.keyed_fill(s, i, seed, i0), 2e-6, 2e-6, f"segment {i}")
    part = H.keyed_fill([(2,) + s[1:] for s in shapes], ids, seed, i0 + 2)
    for t, p in zip(full, part):
        assert torch.equal(t[2:4], p)
    alone = H.keyed_fill([shapes[0]], [ids[0]], seed, i0)[0]                  # independent of what else is drawn with it
    assert torch.equal(alone, full[0])
    u = H.keyed_fill([(3, 3, 64, 64)], [H.SEG_LQ], 7, 0, dist="uniform")[0]
    close(u, R.keyed_fill((3, 3, 64, 64), H.SEG_LQ, 7, 0, dist="uniform"), 0, 1e-7)
    assert float(u.min()) > -1.0 and float(u.max()) < 1.0
    big = H.keyed_fill([(8, 1, 512, 512)], [H.SEG_DEC], 1, 0)[0]             # moments of 2M draws
    assert abs(float(big.mean())) < 3e-3 and abs(float(big.std()) - 1.0) < 3e-3
    assert abs(float((big ** 4).mean()) - 3.0) < 0.05
    assert H.keyed_fill([], [], 1, 0) == []
    with pytest.raises(RuntimeError):
        H.keyed_fill([(2, 4), (3, 4)], [1, 2], 1, 0)                          # mixed batch sizes
    with pytest.raises(RuntimeError):
        H.keyed_fill([(2, 4)] * 65, list(range(65)), 1, 0)                    # more segments than one launch takes
    with pytest.raises(RuntimeError):
        H.keyed_fill([(2, 7), (2, 8)], [1, 2], 1, 0)                          # a vector segment behind an odd-sized one


# ------------------------------------------------------------------------------------------------ bf16 activations in HBM
def _b16(t):
    return t.to(torch.bfloat16)


def test_convert_roundtrip_and_unaligned(H):
    """vsp_convert_*: RNE to bf16 (== torch's), exact back; tensors that start at an odd element (2-byte aligned bf16 / 4-byte
    aligned fp32 storage offsets) go through the same 8- / 16-byte accesses."""
    x = torch.randn(4099, device=DEV) * 3
    for off in (0, 1, 2, 3):
        xs = x[off:]
        b = H.to_bf16(xs)
        assert b.dtype == torch.bfloat16 and torch.equal(b, xs.to(torch.bfloat16))
        base = torch.zeros(4200, device=DEV, dtype=torch.bfloat16)
        base[off:off + b.numel()] = b
        bs = base[off:off + b.numel()]                       # bf16 view at element offset `off`
        assert torch.equal(H.to_f32(bs), b.float())
    assert H.to_bf16(None) is None and H.to_f32(x) is x and H.to_bf16(H.to_bf16(x)).dtype == torch.bfloat16
    e = torch.empty(0, device=DEV)
    assert H.to_bf16(e).numel() == 0


@pytest.mark.parametrize("C_,Hh,Ww,k,pad", [(3, 65, 65, 4, (1, 1)), (2, 64, 64, 4, (2, 2)), (5, 33, 129, 4, (1, 1)), (2, 40, 70, 3, (1, 1))])
def test_blur_bf16_io_matches_fp32_kernel(H, C_, Hh, Ww, k, pad, blur_2d):
    """vsp_upfirdn2d_bf16 = the fp32 blur on the same (bf16-representable) operands, rounded once at the store: bit-identical
    to rounding the fp32 kernel's output.  Odd widths make every plane start on a 2-byte boundary."""
    B = 2
    x = _b16(torch.randn(B, C_, Hh, Ww, device=DEV))
    kern = dev(cases.fir_kernel("blur4" if k == 4 else "rand3x3", "bf16io"))
    oh, ow = Hh + 2 * pad[0] - k + 1, Ww + 2 * pad[0] - k + 1
    nz = torch.randn(B, 1, oh, ow, device=DEV)
    nw, ab = torch.full((1,), 0.3, device=DEV), torch.randn(C_, device=DEV)
    r1, r2 = _b16(torch.randn(B, C_, oh, ow, device=DEV)), _b16(torch.randn(B, C_, oh, ow, device=DEV))
    got = H.blur_fused(x, kern, pad, noise=nz, noise_w=nw, act_bias=ab, act=True, res1=r1, res2=r2)
    ref = H.blur_fused(x.float(), kern, pad, noise=nz, noise_w=nw, act_bias=ab, act=True, res1=r1.float(), res2=r2.float())
    assert got.dtype == torch.bfloat16 and ref.dtype == torch.float32
    assert torch.equal(got, _b16(ref))
    assert torch.equal(H.blur_fused(x, kern, pad), _b16(H.blur_fused(x.float(), kern, pad)))      # plain blur
    got2 = H.blur_fused(x, kern, pad, res1=r1.float())                                          # fp32 residual: converted
    assert torch.equal(got2, _b16(H.blur_fused(x.float(), kern, pad, res1=r1.float())))
    small = _b16(torch.randn(1, 2, 9, 9, device=DEV))                                            # narrower than 16: fp32 kernel
    assert H.blur_fused(small, kern, pad).dtype == torch.float32


@pytest.fixture
def blur_2d(H):
    """the blur kernels in their general 2-D form (the separable row / column form sums in another order)"""
    prev = H.SEPARABLE_BLUR
    H.SEPARABLE_BLUR = False
    yield
    H.SEPARABLE_BLUR = prev


def test_blur_bf16_separable_form_vs_fp64(H):
    """Round 6: outer-product taps (every blur of the path) run as a row pass + a column pass in the bf16 strip kernel (VSP_FIR_SEPARABLE),
    and rows that are not whole 8-column strips (the down-sampling blurs: 2^n + 1 outputs) take whole strips + a tail launch.  Against a
    float64 upfirdn2d of the same bf16 operands: every output within ONE bf16 unit of the rounded reference, at most 2 % off at all; the
    2-D form on the same operands likewise (it is the same sum in another order)."""
    kern = cases.fir_kernel("blur4", "bf16io")
    assert H.taps_separable(dev(kern))
    assert not H.taps_separable(dev(cases.fir_kernel("rand3x3", "bf16io")))
    for it, (B, C_, Hh, Ww, pad) in enumerate([(2, 5, 33, 129, (1, 1)), (1, 3, 67, 515, (1, 1)), (2, 4, 66, 66, (2, 2)), (1, 2, 35, 35, (1, 1)),
                                               (2, 3, 128, 128, (2, 2)), (1, 6, 40, 24, (2, 2)), (2, 2, 16, 16, (2, 2))]):
        g_ = torch.Generator(device=DEV).manual_seed(300 + it)
        x = _b16(torch.randn(B, C_, Hh, Ww, device=DEV, generator=g_))
        oh, ow = Hh + 2 * pad[0] - 3, Ww + 2 * pad[0] - 3
        nz = torch.randn(B, 1, oh, ow, device=DEV, generator=g_)
        nw, ab = torch.full((1,), 0.3, device=DEV), torch.randn(C_, device=DEV, generator=g_)
        r1 = _b16(torch.randn(B, C_, oh, ow, device=DEV, generator=g_))
        for kw in (dict(noise=nz, noise_w=nw, act_bias=ab, act=True, res1=r1), {}):
            got = H.blur_fused(x, dev(kern), pad, **kw)
            assert got.dtype == torch.bfloat16 and got.shape == (B, C_, oh, ow)
            ref = torch.nn.functional.conv2d(torch.nn.functional.pad(x.double().cpu(), (pad[0], pad[1], pad[0], pad[1])).view(B * C_, 1, Hh + 2 * pad[0], -1),
                                             kern.double().flip(0, 1).view(1, 1, 4, 4)).view(B, C_, oh, ow)
            if kw:
                ref = ref + 0.3 * nz.double().cpu()
                ref = torch.nn.functional.leaky_relu(ref + ab.double().cpu().view(1, -1, 1, 1), 0.2) * math.sqrt(2.0) + r1.double().cpu()
            want = ref.float().to(torch.bfloat16)
            d = (got.cpu().float() - want.float()).abs()
            ulp = torch.maximum(want.float().abs(), torch.tensor(1e-30)) * 2.0 ** -7        # one bf16 unit: 2^-8 relative spacing, < 2^-7 |v|
            assert bool((d <= ulp + 1e-6).all()), (it, sorted(kw), float((d / ulp).max()))
            assert float((d > 0).float().mean()) < 0.02, (it, sorted(kw), float((d > 0).float().mean()))


def test_blur_bf16_strip_kernel_bit_identical_many_draws(H, blur_2d):
    """The column-strip bf16 blur (round 5: planes 1 .. N-1 of every 4x4 blur whose rows are whole 16-byte segments) against the fp32
    tile kernel rounded once, over many draws: a fused-multiply-add contraction that differed between the two kernels showed as ONE
    bf16 unit on one output in 20 000 -- invisible to a single draw."""
    kern = dev(cases.fir_kernel("blur4", "bf16io"))
    for it, (B, C_, Hh, Ww, pad) in enumerate([(2, 5, 33, 129, (1, 1))] * 12 + [(1, 3, 67, 515, (1, 1)), (2, 4, 66, 66, (2, 2)), (1, 2, 35, 35, (1, 1))]):
        g_ = torch.Generator(device=DEV).manual_seed(100 + it)
        x = _b16(torch.randn(B, C_, Hh, Ww, device=DEV, generator=g_))
        oh, ow = Hh + 2 * pad[0] - 3, Ww + 2 * pad[0] - 3
        nz = torch.randn(B, 1, oh, ow, device=DEV, generator=g_)
        nw, ab = torch.full((1,), 0.3, device=DEV), torch.randn(C_, device=DEV, generator=g_)
        r1, r2 = _b16(torch.randn(B, C_, oh, ow, device=DEV, generator=g_)), _b16(torch.randn(B, C_, oh, ow, device=DEV, generator=g_))
        for kw in (dict(noise=nz, noise_w=nw, act_bias=ab, act=True, res1=r1, res2=r2), dict(act_bias=ab, act=True, res1=r1), dict(res2=r2), {}):
            got = H.blur_fused(x, kern, pad, **kw)
            kw32 = {a: (v.float() if torch.is_tensor(v) and v.dtype == torch.bfloat16 else v) for a, v in kw.items()}
            assert torch.equal(got, _b16(H.blur_fused(x.float(), kern, pad, **kw32))), (it, sorted(kw))


def test_pointwise_bf16_wide_side(H):
    B, Cin, S = 2, 64, 64
    x = _b16(torch.randn(B, Cin, S, S, device=DEV))
    w, sc, cb = torch.randn(3, Cin, device=DEV) / 8, torch.rand(B, Cin, device=DEV) + 0.5, torch.randn(3, device=DEV)
    skip, kern = torch.randn(B, 3, S // 2, S // 2, device=DEV), dev(cases.fir_kernel("blur4", "x"))
    got = H.pointwise(x, w, in_scale=sc, ch_bias=cb, up_src=skip, up_kernel=kern)
    ref = H.pointwise(x.float(), w, in_scale=sc, ch_bias=cb, up_src=skip, up_kernel=kern)
    assert got.dtype == torch.float32 and torch.equal(got, ref)       # same fp32 arithmetic on the same values
    img = torch.rand(B, 3, S, S, device=DEV) * 2 - 1
    w2, b1, b2 = torch.randn(64, 3, device=DEV), torch.randn(64, device=DEV), torch.randn(64, device=DEV)
    ref2 = H.pointwise(img, w2, bias1=b1, bias2=b2)
    H.ACT_BF16, H.BF16_CONV = True, True
    try:
        got2 = H.pointwise(img, w2, bias1=b1, bias2=b2)
    finally:
        H.ACT_BF16, H.BF16_CONV = False, False
    assert got2.dtype == torch.bfloat16 and torch.equal(got2, _b16(ref2))


@pytest.fixture
def shared_weights(H):
    """vsp_conv2d_bf16 with ONE weight set and the style scale applied to the staged pixels (round 6 moved modulated layers with bf16
    activations to per-image weights, which round differently: test_conv2d_bf16_per_image_weights)"""
    prev = H.BF16_MODW
    H.BF16_MODW = False
    yield
    H.BF16_MODW = prev


@pytest.mark.parametrize("B,Cin,Cout,Hh,Ww,G,mode", [
    (2, 64, 64, 64, 64, 1, "s1"),        # plain stride 1
    (3, 24, 40, 34, 48, 1, "s1"),        # Cin = 16 + 8 (the second octet of the last chunk is empty), ragged output channels and map
    (2, 128, 32, 64, 64, 4, "s1"),       # four dilation groups over one shared input
    (2, 512, 512, 16, 16, 1, "s1"),      # deep layer, many chunks
    (2, 64, 128, 64, 64, 1, "s2"),       # stride 2 (parity planes), padding 0 after the blur in the path: tested with padding 1 and 0
    (2, 32, 48, 30, 44, 1, "s2"),
    (2, 128, 64, 32, 32, 1, "tc"),       # one-pass transposed
    (1, 64, 32, 40, 64, 1, "tc"),
])
def test_conv2d_bf16_per_image_weights(H, B, Cin, Cout, Hh, Ww, G, mode):
    """Round 6: a modulated layer with bf16 activations runs vsp_conv2d_bf16 on PER-IMAGE weights bf16(W * style[b]) (vsp_modulate_weight_bf16,
    w_bstride; the reference's own fused form, models/RestoreNet.py:381-416) and its staging is a copy.  Against float64 F.conv2d /
    F.conv_transpose2d on exactly those operands (bf16 pixels, bf16-rounded modulated weights; products exact, fp32 accumulation): within one
    bf16 unit of the rounded reference everywhere.  Also: the weight image itself against a host restatement, bit for bit."""
    g_ = torch.Generator(device=DEV).manual_seed(Cin * 3 + Hh)
    x = _b16(torch.randn(B, Cin, Hh, Ww, device=DEV, generator=g_))
    ws = [torch.randn(Cout, Cin, 3, 3, device=DEV, generator=g_) / math.sqrt(Cin * 9) for _ in range(G)]
    s_in = torch.rand(B, Cin, device=DEV, generator=g_) + 0.5
    demod, bias = torch.rand(B, G * Cout, device=DEV, generator=g_) + 0.5, torch.randn(G * Cout, device=DEV, generator=g_)
    dils = (1, 2, 4, 8)[:G] if G > 1 else (1,)
    wp = torch.stack([H.pack_weight(w_)[0] for w_ in ws]).contiguous() if G > 1 else H.pack_weight(ws[0])
    # the weight image: [b][group][chunk][tap][octet][co_pad][8]
    pc0 = H.PackedConv(wp, G, Cout, Cin, 3, 3, 1, dils, dils)
    img, nbytes = H.bf16_modulated_weight(pc0, s_in)
    nch, co_pad = (Cin + 15) // 16, (Cout + 31) // 32 * 32
    assert nbytes == G * nch * 9 * 2 * co_pad * 16 and img.shape == (B, nbytes // 2)
    wz = torch.zeros(B, G, 9, nch * 16, co_pad, device=DEV)
    wz[:, :, :, :Cin, :Cout] = wp[None] * s_in[:, None, None, :, None]
    want = wz.view(B, G, 9, nch, 2, 8, co_pad).permute(0, 1, 3, 2, 4, 6, 5).to(torch.bfloat16).contiguous().view(B, -1)
    assert torch.equal(img, want)

    def wmod(b, g):   # bf16(W * s) as float64, (Cout, Cin, 3, 3)
        return (ws[g] * s_in[b].view(1, -1, 1, 1)).to(torch.bfloat16).double().cpu()

    def close(got, ref, what):
        assert got.dtype == torch.bfloat16 and got.shape == ref.shape, (what, got.shape, ref.shape)
        want_ = ref.float().to(torch.bfloat16).float()
        err = (got.cpu().float() - want_).abs()
        lim = ref.abs().float() * 2.0 ** -7 + 3e-5 * float(ref.abs().max())
        assert bool((err <= lim).all()), (what, float((err / lim).max()))

    xd = x.double().cpu()
    if mode == "s1":
        pc = pc0
        kw = dict(in_scale=s_in, out_scale=demod, act2=1, bias2=bias)
        prof = H.ConvProfiler()
        H.PROFILER = prof
        try:
            got = H.conv2d_packed(x, pc, bf16=True, tile_hint=0, **kw) if G == 1 else None
        finally:
            H.PROFILER = None
        if G > 1:
            H.BF16_DG = False     # (keep the launch on vsp_conv2d_bf16: the dilation-group kernel has its own test)
            try:
                got = H.conv2d_packed(x, pc, bf16=True, **kw)
            finally:
                H.BF16_DG = True
        ref = torch.stack([torch.cat([F.conv2d(xd[b:b + 1], wmod(b, g), padding=dils[g], dilation=dils[g]) for g in range(G)], 1)[0] for b in range(B)])
        ref = F.leaky_relu(ref * demod.double().cpu()[:, :, None, None] + bias.double().cpu()[None, :, None, None], 0.2) * math.sqrt(2.0)
        close(got, ref, "stride 1")
    elif mode == "s2":
        for pad in (1, 0):
            pc = H.PackedConv(wp, 1, Cout, Cin, 3, 3, 2, (1,), (pad,))
            got = H.conv2d_packed(x, pc, bf16=True, in_scale=s_in, out_scale=demod)
            ref = torch.stack([F.conv2d(xd[b:b + 1], wmod(b, 0), stride=2, padding=pad)[0] for b in range(B)]) * demod.double().cpu()[:, :, None, None]
            close(got, ref, f"stride 2 pad {pad}")
    else:
        pc = H.PackedConv(wp, 1, Cout, Cin, 3, 3, 1, (1,), (1,))
        got = H.conv_transpose2d_s2_fused(x, pc, in_scale=s_in, out_scale=demod, bf16=True)
        ref = torch.stack([F.conv_transpose2d(xd[b:b + 1], wmod(b, 0).transpose(0, 1), stride=2)[0] for b in range(B)]) * demod.double().cpu()[:, :, None, None]
        close(got, ref, "transposed")
    # the launch really took the per-image form: with it switched off the result differs somewhere (another rounding), and stays close
    H.BF16_MODW = False
    try:
        if mode == "s1" and G == 1:
            alt = H.conv2d_packed(x, pc, bf16=True, in_scale=s_in, out_scale=demod, act2=1, bias2=bias)
            assert not torch.equal(alt, got)
            assert float((alt.float() - got.float()).abs().max()) < 0.05 * float(got.float().abs().max())
    finally:
        H.BF16_MODW = True


def test_conv2d_bf16_per_image_weights_refusals(H):
    """w_bstride is served by vsp_conv2d_bf16 with bf16 activations only; every other entry refuses it (VSP_EINVAL), it does not ignore it."""
    import ctypes as C
    from vspbfr_amd import _lib
    x = torch.randn(1, 16, 16, 16, device=DEV)
    w = torch.randn(16, 16, 3, 3, device=DEV)
    pc = H.PackedConv(H.pack_weight(w), 1, 16, 16, 3, 3, 1, (1,), (1,))
    y = torch.empty(1, 16, 16, 16, device=DEV)
    p = _lib.ConvParams()
    p.x, p.w, p.y = x.data_ptr(), pc.w.data_ptr(), y.data_ptr()
    p.B, p.Cin, p.H, p.W, p.G, p.cout_g, p.OH, p.OW, p.KH, p.KW = 1, 16, 16, 16, 1, 16, 16, 16, 3, 3
    p.stride_y = p.stride_x = 1
    p.dil[0] = p.pad_y[0] = p.pad_x[0] = 1
    p.y_ch, p.y_h, p.y_w, p.osy, p.osx = 16, 16, 16, 1, 1
    p.slope1 = p.slope2 = 0.2
    p.gain1 = p.gain2 = 1.0
    p.w_bstride = 4096
    assert _lib.lib.vsp_conv2d_f32(C.byref(p), None) == -1          # VSP_EINVAL
    assert _lib.lib.vsp_conv2d_bf16(C.byref(p), None) == -1         # fp32 activations
    assert b"w_bstride" in _lib.lib.vsp_last_error() or b"per-image" in _lib.lib.vsp_last_error()
    p.w_bstride = 0
    assert _lib.lib.vsp_conv2d_f32(C.byref(p), None) == 0


@pytest.mark.parametrize("B,Cin,Cout,Hh,Ww", [(2, 32, 64, 64, 64), (1, 64, 32, 33, 70), (2, 128, 128, 32, 32)])
def test_conv2d_bf16_io(H, B, Cin, Cout, Hh, Ww, shared_weights):
    """io_bf16: the bf16 conv kernel with bf16 x / y / residuals equals the same kernel with fp32 I/O on the same
    (bf16-representable) operands, rounded once at the store -- stride 1 with the whole epilogue, the four dilation groups,
    stride 2 and the one-pass transposed form (whose (2H+1)^2 planes are only 2-byte aligned)."""
    x = _b16(torch.randn(B, Cin, Hh, Ww, device=DEV))
    w = torch.randn(Cout, Cin, 3, 3, device=DEV) / math.sqrt(Cin * 9)
    s_in, demod, bias = torch.rand(B, Cin, device=DEV) + 0.5, torch.rand(B, Cout, device=DEV) + 0.5, torch.randn(Cout, device=DEV)
    nz, nw = torch.randn(B, 1, Hh, Ww, device=DEV), torch.full((1,), 0.2, device=DEV)
    r1, r2 = _b16(torch.randn(B, Cout, Hh, Ww, device=DEV)), _b16(torch.randn(B, Cout, Hh, Ww, device=DEV))
    pc = H.PackedConv(H.pack_weight(w), 1, Cout, Cin, 3, 3, 1, (1,), (1,))
    kw = dict(in_scale=s_in, out_scale=demod, act2=1, bias2=bias, noise=nz, noise_w=nw)
    got = H.conv2d_packed(x, pc, bf16=True, res1=r1, res2=r2, **kw)
    ref = H.conv2d_packed(x.float(), pc, bf16=True, res1=r1.float(), res2=r2.float(), **kw)
    assert got.dtype == torch.bfloat16 and ref.dtype == torch.float32 and torch.equal(got, _b16(ref))
    pc2 = H.PackedConv(H.pack_weight(w), 1, Cout, Cin, 3, 3, 2, (1,), (1,))
    assert torch.equal(H.conv2d_packed(x, pc2, bf16=True), _b16(H.conv2d_packed(x.float(), pc2, bf16=True)))
    yt = H.conv_transpose2d_s2_fused(x, pc, in_scale=s_in, out_scale=demod, bf16=True)
    assert yt.dtype == torch.bfloat16 and yt.shape[-1] == 2 * Ww + 1
    assert torch.equal(yt, _b16(H.conv_transpose2d_s2_fused(x.float(), pc, in_scale=s_in, out_scale=demod, bf16=True)))
    if Cout % 4 == 0 and Cout // 4 >= 8:
        wp = torch.stack([H.pack_weight(torch.randn(Cout // 4, Cin, 3, 3, device=DEV) / math.sqrt(Cin * 9))[0] for _ in range(4)]).contiguous()
        pc4 = H.PackedConv(wp, 4, Cout // 4, Cin, 3, 3, 1, (1, 2, 4, 8), (1, 2, 4, 8))
        H.BF16_DG = False   # (this test is about vsp_conv2d_bf16's own I/O forms; with bf16 input the launch would go to vsp_conv2d_bf16dg,
        try:                #  which rounds the style scale into the weight: test_conv2d_bf16dg)
            assert torch.equal(H.conv2d_packed(x, pc4, bf16=True, in_scale=s_in), _b16(H.conv2d_packed(x.float(), pc4, bf16=True, in_scale=s_in)))
        finally:
            H.BF16_DG = True
    # a bf16 tensor handed to a layer that runs on an fp32 kernel is converted, the result is fp32
    assert H.conv2d_packed(x, pc, bf16=False, winograd=False).dtype == torch.float32
    o32 = torch.empty(B, Cout, Hh, Ww, device=DEV)                    # an fp32 `out` keeps the launch on fp32 I/O
    assert H.conv2d_packed(x, pc, bf16=True, out=o32, **kw) is o32 and torch.equal(o32, H.conv2d_packed(x.float(), pc, bf16=True, **kw))


@pytest.mark.parametrize("B,Cin,Cout,Hh,Ww,hint", [(2, 32, 64, 64, 64, 0), (1, 64, 32, 40, 128, 0), (2, 16, 32, 16, 64, 1), (1, 24, 64, 9, 64, 2),
                                                   (1, 128, 128, 64, 64, 2), (1, 64, 64, 70, 192, 1),
                                                   (5, 64, 64, 256, 256, 0), (6, 32, 32, 256, 256, 1)])   # more tiles than resident workgroups: the persistent walk, two workgroups per CU
def test_conv2d_bf16rv(H, B, Cin, Cout, Hh, Ww, hint):
    """vsp_conv2d_bf16rv (row-vector K: two channels x four pixels per lane fragment) against vsp_conv2d_bf16 with fp32 output on the
    same bf16-representable operands: same products, another summation order and ONE rounding at the store -- whole epilogue
    (style scale, demodulation, noise, bias, activation, two residuals), both tile variants, ragged row counts, 1 and 3 chunks,
    the affine (folded BatchNorm) prologue whose shift must not leak into the zero padding."""
    x = _b16(torch.randn(B, Cin, Hh, Ww, device=DEV))
    w = torch.randn(Cout, Cin, 3, 3, device=DEV) / math.sqrt(Cin * 9)
    s_in, demod, bias = torch.rand(B, Cin, device=DEV) + 0.5, torch.rand(B, Cout, device=DEV) + 0.5, torch.randn(Cout, device=DEV)
    nz, nw = torch.randn(B, 1, Hh, Ww, device=DEV), torch.full((1,), 0.2, device=DEV)
    r1, r2 = _b16(torch.randn(B, Cout, Hh, Ww, device=DEV)), _b16(torch.randn(B, Cout, Hh, Ww, device=DEV))
    pc = H.PackedConv(H.pack_weight(w), 1, Cout, Cin, 3, 3, 1, (1,), (1,))

    def close(got, ref):
        assert got.dtype == torch.bfloat16 and got.shape == ref.shape
        err = (got.float() - ref).abs()
        assert bool((err <= ref.abs() * 2.0 ** -8 + 2e-5 * ref.abs().max()).all()), float(err.max())

    kw = dict(in_scale=s_in, out_scale=demod, act2=1, bias2=bias, noise=nz, noise_w=nw)
    close(H.conv2d_packed(x, pc, bf16="rv", tile_hint=hint, res1=r1, res2=r2, **kw), H.conv2d_packed(x.float(), pc, bf16=True, res1=r1.float(), res2=r2.float(), **kw))
    close(H.conv2d_packed(x, pc, bf16="rv", tile_hint=hint), H.conv2d_packed(x.float(), pc, bf16=True))
    close(H.conv2d_packed(x, pc, bf16="rv", tile_hint=hint, act1=True, bias1=bias, res1=r1), H.conv2d_packed(x.float(), pc, bf16=True, act1=True, bias1=bias, res1=r1.float()))
    bn_s, bn_h = torch.rand(Cin, device=DEV) + 0.5, torch.randn(Cin, device=DEV)
    kw2 = dict(in_scale=bn_s, in_scale_per_sample=False, in_shift=bn_h, act2=2, prelu=torch.rand(Cout, device=DEV) * 0.5)
    close(H.conv2d_packed(x, pc, bf16="rv", tile_hint=hint, **kw2), H.conv2d_packed(x.float(), pc, bf16=True, **kw2))


@pytest.mark.parametrize("B,Cin,Cg,Hh,Ww,dils", [(2, 32, 16, 40, 64, (1, 2, 4, 8)), (1, 64, 32, 64, 128, (1, 2, 4, 8)), (1, 16, 8, 19, 64, (2, 8)),
                                                   (3, 64, 16, 128, 256, (8, 4, 2, 1))])
def test_conv2d_bf16rv_dilation_groups(H, B, Cin, Cg, Hh, Ww, dils):
    """The dilation groups of a SMART branch launch on vsp_conv2d_bf16rv (columns de-interleaved into d residue sub-rows in LDS, rows
    polyphase) against vsp_conv2d_bf16 with fp32 output on the same bf16-representable operands: 16 / 32 / 8 channels per group (the
    zero-padded half of a 32-row weight slab is never stored), ragged row counts, more tiles than resident workgroups."""
    G = len(dils)
    x = _b16(torch.randn(B, Cin, Hh, Ww, device=DEV))
    wp = torch.stack([H.pack_weight(torch.randn(Cg, Cin, 3, 3, device=DEV) / math.sqrt(Cin * 9))[0] for _ in range(G)]).contiguous()
    pc = H.PackedConv(wp, G, Cg, Cin, 3, 3, 1, dils, dils)
    s_in, demod, bias = torch.rand(B, Cin, device=DEV) + 0.5, torch.rand(B, G * Cg, device=DEV) + 0.5, torch.randn(G * Cg, device=DEV)
    r1 = _b16(torch.randn(B, G * Cg, Hh, Ww, device=DEV))
    for kw in (dict(in_scale=s_in), dict(in_scale=s_in, out_scale=demod, act2=1, bias2=bias, res1=r1), dict()):
        got = H.conv2d_packed(x, pc, bf16="rv", **kw)
        kwf = {k: (v.float() if k == "res1" else v) for k, v in kw.items()}
        ref = H.conv2d_packed(x.float(), pc, bf16=True, **kwf)
        assert got.dtype == torch.bfloat16 and got.shape == ref.shape
        err = (got.float() - ref).abs()
        assert bool((err <= ref.abs() * 2.0 ** -8 + 2e-5 * ref.abs().max()).all()), (float(err.max()), kw.keys())


@pytest.mark.parametrize("B,Cin,Cout,Hh,Ww,hint", [(5, 64, 64, 256, 256, 0), (6, 32, 32, 256, 256, 1)])
def test_conv2d_bf16rv_repeat(H, B, Cin, Cout, Hh, Ww, hint):
    """The fence around the packed-fp32 miscompare of round 4 (conv_bf16_rv.hip refuses to build with SLP vectorisation): more
    tiles than resident workgroups, two workgroups per CU, 50 launches of the same operands -- every launch BIT-identical to the first
    (the failure was sporadic: 0.01-0.05 % of the outputs, never the same ones) and the first one within one bf16 rounding of float64
    F.conv2d on the bf16-rounded operands, DIRECTLY (not through vsp_conv2d_bf16)."""
    g_ = torch.Generator().manual_seed(B * 1000 + Cin)
    x = torch.randn(B, Cin, Hh, Ww, generator=g_).to(torch.bfloat16)
    w = torch.randn(Cout, Cin, 3, 3, generator=g_) / math.sqrt(Cin * 9)
    s_in, demod, bias = torch.rand(B, Cin, generator=g_) + 0.5, torch.rand(B, Cout, generator=g_) + 0.5, torch.randn(Cout, generator=g_)
    nz, nw = torch.randn(B, 1, Hh, Ww, generator=g_), torch.full((1,), 0.2)
    pc = H.PackedConv(H.pack_weight(dev(w)), 1, Cout, Cin, 3, 3, 1, (1,), (1,))
    xd = dev(x)
    kw = dict(in_scale=dev(s_in), out_scale=dev(demod), act2=1, bias2=dev(bias), noise=dev(nz), noise_w=dev(nw))
    first = H.conv2d_packed(xd, pc, bf16="rv", tile_hint=hint, **kw)
    first_bare = H.conv2d_packed(xd, pc, bf16="rv", tile_hint=hint)
    for _ in range(50):
        assert torch.equal(H.conv2d_packed(xd, pc, bf16="rv", tile_hint=hint, **kw), first)
    for _ in range(10):
        assert torch.equal(H.conv2d_packed(xd, pc, bf16="rv", tile_hint=hint), first_bare)
    sel = [0, B - 1]
    wb = w.to(torch.bfloat16).double()
    xs = (x[sel].float() * s_in[sel].view(2, Cin, 1, 1)).to(torch.bfloat16).double()      # the kernel commits bf16(x * s)
    ref = F.conv2d(xs, wb, padding=1) * demod[sel].double().view(2, Cout, 1, 1) + nz[sel].double() * 0.2
    ref = F.leaky_relu(ref + bias.double().view(1, -1, 1, 1), 0.2) * math.sqrt(2)
    ref_bare = F.conv2d(x[sel].double(), wb, padding=1)
    for got, r in ((first[sel], ref), (first_bare[sel], ref_bare)):
        err = (got.double().cpu() - r).abs()
        assert bool((err <= r.abs() * 2.0 ** -8 + 2e-5 * r.abs().max()).all()), float(err.max())


@pytest.mark.parametrize("B,Cin,Cg,Hh,Ww,dils", [(2, 64, 16, 64, 64, (1, 2, 4, 8)), (1, 32, 16, 37, 24, (1, 2, 4, 8)), (3, 64, 8, 40, 64, (2, 8)),
                                                   (1, 16, 16, 9, 8, (4,)), (2, 48, 12, 19, 40, (8, 1, 2)), (2, 64, 16, 256, 256, (1, 2, 4, 8))])
def test_conv2d_bf16dg(H, B, Cin, Cg, Hh, Ww, dils):
    """vsp_conv2d_bf16dg (the dilation groups of a SMART branch launch on v_mfma_f32_16x16x32_bf16: patch channel-last and polyphase in LDS,
    weights as register-resident A fragments) DIRECTLY against float64 F.conv2d(dilation = d) on the operands the kernel multiplies: bf16
    activations and bf16(w * style scale) -- the scale is rounded into the WEIGHT here -- exact products, fp32 accumulation, one bf16 rounding
    at the store.  Ragged maps, partial channel blocks, fewer groups, the whole epilogue chain with both residuals, repeat launches
    bit-identical, and the automatic choice for a bf16 input."""
    g_ = torch.Generator().manual_seed(Hh * 7 + Ww)
    G = len(dils)
    x = torch.randn(B, Cin, Hh, Ww, generator=g_).to(torch.bfloat16)
    ws = [torch.randn(Cg, Cin, 3, 3, generator=g_) / math.sqrt(Cin * 9) for _ in dils]
    s_in, demod, bias = torch.rand(B, Cin, generator=g_) + 0.5, torch.rand(B, G * Cg, generator=g_) + 0.5, torch.randn(G * Cg, generator=g_)
    nz, nw = torch.randn(B, 1, Hh, Ww, generator=g_), torch.full((1,), 0.3)
    r1 = torch.randn(B, G * Cg, Hh, Ww, generator=g_).to(torch.bfloat16)
    r2 = torch.randn(B, G * Cg, Hh, Ww, generator=g_).to(torch.bfloat16)
    wp = torch.stack([H.pack_weight(dev(w_))[0] for w_ in ws]).contiguous()
    pc = H.PackedConv(wp, G, Cg, Cin, 3, 3, 1, dils, dils)
    sel = [0, B - 1] if Hh * Ww >= 65536 else list(range(B))

    def ref(scale, full):
        outs = []
        for b in sel:
            sb = scale[b].view(1, Cin, 1, 1) if scale is not None else torch.ones(1, Cin, 1, 1)
            y = torch.cat([F.conv2d(x[b:b + 1].double(), (w_ * sb).to(torch.bfloat16).double(), padding=d, dilation=d) for w_, d in zip(ws, dils)], 1)
            if full:
                y = y * demod[b].double().view(1, -1, 1, 1) + nz[b:b + 1].double() * 0.3
                y = F.leaky_relu(y + bias.double().view(1, -1, 1, 1), 0.2) * math.sqrt(2) + r1[b:b + 1].double() + r2[b:b + 1].double()
            outs.append(y)
        return torch.cat(outs)

    def close(got, want):
        assert got.dtype == torch.bfloat16
        err = (got[sel].double().cpu() - want).abs()
        assert bool((err <= want.abs() * 2.0 ** -8 + 2e-5 * want.abs().max()).all()), float(err.max())

    xd = dev(x)
    bare = H.conv2d_packed(xd, pc, bf16="dg")
    close(bare, ref(None, False))
    kw = dict(in_scale=dev(s_in), out_scale=dev(demod), noise=dev(nz), noise_w=dev(nw), act2=1, bias2=dev(bias), res1=dev(r1), res2=dev(r2))
    full = H.conv2d_packed(xd, pc, bf16="dg", **kw)
    close(full, ref(s_in, True))
    for _ in range(5):
        assert torch.equal(H.conv2d_packed(xd, pc, bf16="dg", **kw), full)
    if G > 1:   # a bf16 input to a dilation-group launch takes this kernel by itself
        assert torch.equal(H.conv2d_packed(xd, pc, bf16=True, **kw), full)
    with pytest.raises(RuntimeError):   # an affine input shift is not served
        H.conv2d_packed(xd, pc, bf16="dg", in_scale=dev(torch.rand(Cin)), in_scale_per_sample=False, in_shift=dev(torch.randn(Cin)))
    with pytest.raises(RuntimeError):   # nor is y one element (2 bytes) off a 4-byte boundary
        H.conv2d_packed(xd, pc, bf16="dg", out=torch.empty(bare.numel() + 1, device=DEV, dtype=torch.bfloat16)[1:].view(bare.shape))


def test_conv2d_bf16rv_refusals(H):
    """Launches the row-vector kernel does not serve: VSP_ENOTSUP at the C entry (the automatic path then uses vsp_conv2d_bf16),
    an error when it is forced."""
    w = torch.randn(32, 32, 3, 3, device=DEV) / 17
    pc = H.PackedConv(H.pack_weight(w), 1, 32, 32, 3, 3, 1, (1,), (1,))
    x = _b16(torch.randn(1, 32, 32, 48, device=DEV))            # W % 64 != 0
    with pytest.raises(RuntimeError, match="row-vector"):
        H.conv2d_packed(x, pc, bf16="rv")
    H.BF16_CONV, H.ACT_BF16 = True, True
    try:
        y = H.conv2d_packed(x, pc)                               # automatic: the general bf16 kernel
        x2 = _b16(torch.randn(1, 32, 128, 128, device=DEV))
        y2 = H.conv2d_packed(x2, pc)                             # automatic: eligible and profitable -> the row-vector kernel
    finally:
        H.BF16_CONV, H.ACT_BF16 = False, False
    assert y.dtype == torch.bfloat16 and y2.dtype == torch.bfloat16
    ref2 = H.conv2d_packed(x2.float(), pc, bf16=True)
    assert float((y2.float() - ref2).abs().max()) <= float(ref2.abs().max()) * 2.0 ** -7


# ------------------------------------------------------------------------------------------------ convolution backward
def _grads(fn, *tensors):
    with torch.enable_grad():   # (this module switches autograd off globally)
        ts = [t.clone().requires_grad_(True) for t in tensors]
        y = fn(*ts)
        g = torch.randn(y.shape, generator=torch.Generator().manual_seed(5)).to(y.device, y.dtype)
        y.backward(g)
    return [y.detach()] + [t.grad for t in ts]


@pytest.mark.parametrize("case", [
    dict(cin=24, cout=40, hw=(19, 23), k=3, stride=1, pad=1, dil=1, groups=1, bias=True),
    dict(cin=16, cout=24, hw=(21, 18), k=3, stride=1, pad=2, dil=2, groups=1, bias=False),
    dict(cin=18, cout=12, hw=(12, 12), k=3, stride=1, pad=1, dil=1, groups=3, bias=False),      # the groups=batch form
    dict(cin=32, cout=3, hw=(16, 16), k=1, stride=1, pad=0, dil=1, groups=1, bias=True),        # ToRGB
    dict(cin=16, cout=32, hw=(17, 17), k=3, stride=2, pad=0, dil=1, groups=1, bias=False),      # StyledConv_down after its blur
    dict(cin=16, cout=16, hw=(18, 20), k=3, stride=2, pad=0, dil=1, groups=2, bias=False),
    dict(cin=80, cout=72, hw=(70, 66), k=3, stride=1, pad=1, dil=1, groups=1, bias=False),      # several tiles, ragged channel tiles
    dict(cin=16, cout=24, hw=(28, 28), k=3, stride=2, pad=1, dil=1, groups=1, bias=False),      # ResNet bottleneck (identity loss), even size
    dict(cin=16, cout=16, hw=(15, 17), k=3, stride=2, pad=1, dil=1, groups=1, bias=True),       # ... odd sizes
])
def test_conv2d_gradfix_autograd(case):
    """conv2d_gradfix.conv2d with autograd against torch autograd of F.conv2d in float64: forward, data gradient (forward
    kernels on the adjoint geometry), weight gradient (vsp_conv2d_wgrad_f32), bias gradient."""
    from vspbfr_amd.op import conv2d_gradfix
    c = case
    B = 2
    g_ = torch.Generator().manual_seed(11)
    x = torch.randn(B, c["cin"], *c["hw"], generator=g_)
    w = torch.randn(c["cout"], c["cin"] // c["groups"], c["k"], c["k"], generator=g_) / math.sqrt(c["cin"] // c["groups"] * c["k"] ** 2)
    b = torch.randn(c["cout"], generator=g_) if c["bias"] else None
    kw = dict(stride=c["stride"], padding=c["pad"], dilation=c["dil"], groups=c["groups"])
    ts = [x, w] + ([b] if b is not None else [])
    ref = _grads(lambda x_, w_, *b_: F.conv2d(x_, w_, b_[0] if b_ else None, **kw), *[t.double() for t in ts])
    got = _grads(lambda x_, w_, *b_: conv2d_gradfix.conv2d(x_, w_, b_[0] if b_ else None, **kw), *[dev(t) for t in ts])
    for name, a, r in zip(("y", "dx", "dw", "db"), got, ref):
        close(a, r.float(), 3e-5, 3e-5, name)
    with conv2d_gradfix.no_weight_gradients(), torch.enable_grad():
        xs, ws = dev(x).requires_grad_(True), dev(w).requires_grad_(True)
        conv2d_gradfix.conv2d(xs, ws, None, **kw).sum().backward()
        assert ws.grad is None and xs.grad is not None
    with torch.no_grad():
        assert not conv2d_gradfix.conv2d(dev(x), dev(w), None, **kw).requires_grad


@pytest.mark.parametrize("groups", [1, 2])
def test_conv_transpose2d_gradfix_autograd(groups):
    from vspbfr_amd.op import conv2d_gradfix
    B, cin, cout, Hh, Ww = 2, 16 * groups, 12, 9, 11
    g_ = torch.Generator().manual_seed(3)
    x = torch.randn(B, cin, Hh, Ww, generator=g_)
    w = torch.randn(cin, cout, 3, 3, generator=g_) / math.sqrt(cin // groups * 9)
    ref = _grads(lambda x_, w_: F.conv_transpose2d(x_, w_, stride=2, groups=groups), x.double(), w.double())
    got = _grads(lambda x_, w_: conv2d_gradfix.conv_transpose2d(x_, w_, stride=2, padding=0, groups=groups), dev(x), dev(w))
    for name, a, r in zip(("y", "dx", "dw"), got, ref):
        close(a, r.float(), 3e-5, 3e-5, name)


def test_conv2d_wgrad_scales_and_plane_dot(H):
    """The fused form of a modulated layer: y = demod[b,co] * conv(x * s[b,ci], W).  dW with both per-sample scales inside the
    kernel, and the two scale gradients through vsp_plane_dot_f32, against float64 autograd."""
    B, cin, cout, S = 3, 20, 28, 14
    g_ = torch.Generator().manual_seed(9)
    x, w = torch.randn(B, cin, S, S, generator=g_), torch.randn(cout, cin, 3, 3, generator=g_) / math.sqrt(cin * 9)
    s, dm = torch.rand(B, cin, generator=g_) + 0.5, torch.rand(B, cout, generator=g_) + 0.5
    gy = torch.randn(B, cout, S, S, generator=g_)
    with torch.enable_grad():
        xd, wd, sd, dd = (t.double().requires_grad_(True) for t in (x, w, s, dm))
        y = F.conv2d(xd * sd[:, :, None, None], wd, padding=1) * dd[:, :, None, None]
        y.backward(gy.double())
    dw = H.conv2d_wgrad(dev(x), dev(gy), w.shape, 1, 1, 1, 1, x_scale=dev(s), dy_scale=dev(dm))
    close(dw, wd.grad.float(), 3e-5, 3e-5, "dw")
    # d demod[b,co] = <gy, y> / demod;  d s[b,ci] = <dxs, x> with dxs = the data gradient w.r.t. the scaled input
    close(H.plane_dot(dev(gy), dev(y.detach().float())) / dev(dm), dd.grad.float(), 3e-5, 3e-5, "d demod")
    dxs = F.conv_transpose2d(gy.double() * dm.double()[:, :, None, None], w.double(), padding=1).float()
    close(H.plane_dot(dev(dxs), dev(x)), sd.grad.float(), 3e-5, 3e-5, "d style")
    dws = H.conv2d_wgrad(dev(x), dev(gy), w.shape, 1, 1, 1, 1, x_scale=dev(s), dy_scale=dev(dm), scale=0.37)   # dw_scale: the equalized-lr factor
    close(dws, 0.37 * dw.cpu(), 2e-5, 2e-5 * float(dw.abs().max()), "scaled dw")
    assert H.conv2d_wgrad(dev(x[:0]), dev(gy[:0]), w.shape, 1, 1).abs().max().item() == 0.0     # empty batch: zeros
    with pytest.raises(RuntimeError):
        H.conv2d_wgrad(dev(x), dev(gy), (cout, cin, 5, 5), 1, 2)


@pytest.mark.parametrize("ish,osh", [((512, 512), (256, 256)), ((300, 420), (256, 256)), ((128, 96), (256, 256)), ((7, 5), (3, 11))])
def test_resize_bilinear_matches_interpolate(H, ish, osh):
    """vsp_resize_bilinear_f32 = F.interpolate(mode="bilinear", align_corners=False) (the reference's resize in front of the e4e
    encoder, Loss/e4e_embedding.py:91-100) for down- and up-scaling; from 512^2 to 256^2 it equals the 2x2 mean get_w_plus uses."""
    x = torch.randn(2, 3, *ish)
    close(H.resize_bilinear(dev(x), osh), F.interpolate(x, osh, mode="bilinear", align_corners=False), 1e-6, 2e-6)
    if ish == (512, 512):
        close(H.resize_bilinear(dev(x), osh), H.avgpool2x2(dev(x)), 1e-6, 1e-6)


def test_device_guard_second_device(golden):
    """Device guard at the boundary (reference op/fused_bias_act.cpp:25, op/upfirdn2d.cpp:23): tensors on cuda:1 while cuda:0 is the
    current device launch on cuda:1, through the pybind11 modules and through the ctypes path; mixed-device operands are refused.
    Needs two visible devices (the round-end box has one: skipped there; the refusal logic itself is CPU-tested in tests/test_abi.py)."""
    if torch.cuda.device_count() < 2:
        pytest.skip("one visible device")
    from vspbfr_amd.op import native
    from vspbfr_amd.op.fused_act import fused_leaky_relu
    fused, upfirdn2d_op = native.load()
    d1 = torch.device("cuda:1")
    name = next(n for n in cases.LRELU_CASES if cases.lrelu_inputs(n)[1] is not None)
    x, b = cases.lrelu_inputs(name)
    torch.cuda.set_device(0)
    y = fused_leaky_relu(x.to(d1), b.to(d1))
    assert y.device == d1 and torch.cuda.current_device() == 0
    close(y, golden("ops")[name], 1e-6, 1e-6, name)
    y = fused.fused_bias_act(x.to(d1), b.to(d1), torch.empty(0, device=d1), 3, 0, 0.2, math.sqrt(2))
    assert y.device == d1 and torch.cuda.current_device() == 0
    close(y, golden("ops")[name], 1e-6, 1e-6, name)
    xf, k, up, down, pad = cases.fir_inputs("fir_blur_after_up")
    B, C_, Hh, Ww = xf.shape
    y = upfirdn2d_op.upfirdn2d(xf.to(d1).reshape(-1, Hh, Ww, 1), k.to(d1), up[0], up[1], down[0], down[1], pad[0], pad[1], pad[2], pad[3])
    close(y.view(B, C_, y.shape[1], y.shape[2]), golden("ops")["fir_blur_after_up"], 1e-6, 1e-6, "fir on cuda:1")
    with pytest.raises(RuntimeError):
        fused.fused_bias_act(x.to(d1), b.to("cuda:0"), torch.empty(0, device=d1), 3, 0, 0.2, 1.0)
    with pytest.raises(RuntimeError, match="different devices"):
        H.fused_bias_act(x.to(d1), b.to("cuda:0"), torch.empty(0, device=d1), 3, 0, 0.2, 1.0)


def test_torch_extension_modules(golden):
    """The AOT pybind11 modules `fused` / `upfirdn2d` (vspbfr_amd/csrc/torch_ext) with the reference's native signatures
    (op/fused_bias_act.cpp:18-31, op/upfirdn2d.cpp:17-31) against the reference's golden outputs and the ctypes path."""
    from vspbfr_amd.op import native
    fused, upfirdn2d_op = native.load()
    e = torch.empty(0, device=DEV)
    for name in cases.LRELU_CASES:
        x, b = cases.lrelu_inputs(name)
        y = fused.fused_bias_act(dev(x), dev(b) if b is not None else e, e, 3, 0, 0.2, math.sqrt(2))
        close(y, golden("ops")[name], 1e-6, 1e-6, name)
    for name in ("fir_blur_after_up", "fir_upsample_rgb", "fir_generic_asym", "fir_tiles_129"):
        x, k, up, down, pad = cases.fir_inputs(name)
        B, C_, Hh, Ww = x.shape
        y = upfirdn2d_op.upfirdn2d(dev(x).reshape(-1, Hh, Ww, 1), dev(k), up[0], up[1], down[0], down[1], pad[0], pad[1], pad[2], pad[3])
        close(y.view(B, C_, y.shape[1], y.shape[2]), golden("ops")[name], 1e-6, 1e-6, name)
    with pytest.raises(RuntimeError):
        fused.fused_bias_act(torch.zeros(2, 3), torch.zeros(3), torch.zeros(0), 3, 0, 0.2, 1.0)      # CPU tensor: TORCH_CHECK
    # half and double tensors (the reference dispatches over float, double, half: op/fused_bias_act_kernel.cu:96,
    # op/upfirdn2d_kernel.cu:311): converted at the boundary, result in the input's type
    x, b = cases.lrelu_inputs(next(n for n in cases.LRELU_CASES if cases.lrelu_inputs(n)[1] is not None))
    want = golden("ops")[next(n for n in cases.LRELU_CASES if cases.lrelu_inputs(n)[1] is not None)]
    for dt, tol in ((torch.float64, 1e-6), (torch.float16, 2e-3)):
        y = fused.fused_bias_act(dev(x).to(dt), dev(b).to(dt), e.to(dt), 3, 0, 0.2, math.sqrt(2))
        assert y.dtype == dt
        close(y.float(), want, tol, tol * 4, f"fused {dt}")
    x, k, up, down, pad = cases.fir_inputs("fir_blur_after_up")
    B, C_, Hh, Ww = x.shape
    for dt, tol in ((torch.float64, 1e-6), (torch.float16, 2e-3)):
        y = upfirdn2d_op.upfirdn2d(dev(x).to(dt).reshape(-1, Hh, Ww, 1), dev(k).to(dt), up[0], up[1], down[0], down[1], pad[0], pad[1], pad[2], pad[3])
        assert y.dtype == dt
        close(y.float().view(B, C_, y.shape[1], y.shape[2]), golden("ops")["fir_blur_after_up"], tol, tol * 4, f"upfirdn2d {dt}")
    with pytest.raises(RuntimeError):
        fused.fused_bias_act(dev(x).to(torch.int32), e, e, 3, 0, 0.2, 1.0)                           # unsupported dtype


# ------------------------------------------------------------------------------------------------ loss-network operators
@pytest.mark.parametrize("k,s,p,hw", [(2, 2, 0, (20, 14)), (2, 2, 0, (9, 7)), (2, 2, 0, (20, 16)), (2, 2, 0, (64, 128)), (3, 2, 1, (56, 56)), (3, 2, 1, (13, 10))])
def test_maxpool2d_forward_backward(H, k, s, p, hw):
    """vsp_maxpool2d_f32 / _bwd against F.max_pool2d and its autograd (VGG16 2x2/2, ResNet 3x3/2 pad 1), ties included: the
    input is quantised to a few levels so that many windows hold their maximum more than once."""
    from vspbfr_amd.lpips import max_pool2d
    x = (torch.randn(2, 5, *hw, generator=torch.Generator().manual_seed(1)) * 2).round() / 2
    ref = _grads(lambda t: F.max_pool2d(t, k, s, p), x.double())
    got = _grads(lambda t: max_pool2d(t, k, s, p), dev(x))
    close(got[0], ref[0].float(), 0, 0, "y")
    close(got[1], ref[1].float(), 1e-6, 1e-6, "dx")
    assert torch.equal(H.maxpool2d(dev(x), k, s, p), got[0])


@pytest.mark.parametrize("C_,hw", [(64, (24, 20)), (128, (13, 9)), (256, (7, 5)), (512, (5, 3)), (7, (33, 1))])
def test_lpips_layer_forward_backward(H, C_, hw):
    """vsp_lpips_layer_f32 / _bwd against the reference's formula (my_lpips/__init__.py:44-46, networks_basic.py:73-83) evaluated by
    torch autograd in float64, including a pixel whose features are all zero (ReLU outputs) in either map."""
    from vspbfr_amd.lpips import _LayerDistance
    g_ = torch.Generator().manual_seed(2)
    f0, f1 = torch.randn(3, C_, *hw, generator=g_).relu(), torch.randn(3, C_, *hw, generator=g_).relu()
    f0[0, :, 0, 0] = 0
    f1[1, :, -1, -1] = 0
    w = torch.rand(C_, generator=g_)

    def ref_fn(a, b, w_):
        na = a / (torch.sqrt((a ** 2).sum(1, keepdim=True)) + 1e-10)
        nb = b / (torch.sqrt((b ** 2).sum(1, keepdim=True)) + 1e-10)
        return ((na - nb) ** 2 * w_.view(1, -1, 1, 1)).sum(1).mean([1, 2])
    with torch.enable_grad():
        a, b = f0.double().requires_grad_(True), f1.double().requires_grad_(True)
        r = ref_fn(a, b, w.double())
        gout = torch.randn(3, generator=g_)
        r.backward(gout.double())
        a2, b2 = dev(f0).requires_grad_(True), dev(f1).requires_grad_(True)
        y = _LayerDistance.apply(a2, b2, dev(w))
        y.backward(dev(gout))
    close(y, r.float(), 1e-6, 1e-5, "dist")
    # d/df at an all-zero pixel: sqrt'(0) * 0 is NaN in autograd; the kernel drops that term (the pixel's own gradient is g r)
    mask0, mask1 = torch.isfinite(a.grad), torch.isfinite(b.grad)
    close(torch.where(mask0, a2.grad.cpu(), torch.zeros(())), torch.nan_to_num(a.grad).float(), 1e-7, 2e-5, "df0")
    close(torch.where(mask1, b2.grad.cpu(), torch.zeros(())), torch.nan_to_num(b.grad).float(), 1e-7, 2e-5, "df1")
    assert torch.isfinite(a2.grad).all() and torch.isfinite(b2.grad).all()


@pytest.mark.parametrize("ish,osh", [((128, 128), (112, 112)), ((512, 512), (112, 112)), ((20, 31), (45, 17))])
def test_resize_bilinear_backward(H, ish, osh):
    from vspbfr_amd.id_loss import interpolate_bilinear
    x = torch.randn(2, 3, *ish, generator=torch.Generator().manual_seed(4))
    # (fp32 reference: the source coordinates are fp32 in both implementations; in float64 they differ by ~1e-5 of a pixel)
    ref = _grads(lambda t: F.interpolate(t, osh, mode="bilinear", align_corners=False), x)
    got = _grads(lambda t: interpolate_bilinear(t, osh), dev(x))
    close(got[0], ref[0], 1e-6, 2e-6, "y")
    close(got[1], ref[1], 1e-6, 1e-5, "dx")


def test_conv4x4_phase_stem_gradient():
    """The 7x7 stride-2 stem of the identity network as a 4x4 stride-1 convolution over sub-pixel phases (vspbfr_amd/id_loss.py):
    output and input gradient against F.conv2d(x, w, stride=2, padding=3) in float64."""
    from vspbfr_amd.id_loss import ResNet101
    net = ResNet101(num_classes=8, layers=(1, 1, 1, 1)).to(DEV).eval()
    g_ = torch.Generator().manual_seed(6)
    x = torch.randn(2, 3, 36, 28, generator=g_)
    with torch.no_grad():
        net.bn1.weight.copy_(torch.rand(64, generator=g_) + 0.5)
        net.bn1.bias.copy_(torch.randn(64, generator=g_) * 0.1)
        net.bn1.running_mean.copy_(torch.randn(64, generator=g_) * 0.1)
        net.bn1.running_var.copy_(torch.rand(64, generator=g_) + 0.5)
    w, bn = net.conv1.weight.detach().cpu().double(), net.bn1

    def ref_fn(t):
        y = F.conv2d(t, w, None, 2, 3)
        return F.relu(F.batch_norm(y, bn.running_mean.cpu().double(), bn.running_var.cpu().double(), bn.weight.detach().cpu().double(),
                                   bn.bias.detach().cpu().double(), False, 0.0, bn.eps))
    ref = _grads(ref_fn, x.double())
    got = _grads(lambda t: net._stem(t), dev(x))
    close(got[0], ref[0].float(), 2e-5, 2e-5, "y")
    close(got[1], ref[1].float(), 3e-5, 3e-5, "dx")
    with torch.no_grad():
        close(net._stem(dev(x)), ref[0].float(), 2e-5, 2e-5, "y (fused epilogue)")


@pytest.mark.parametrize("cfg", [
    dict(cin=64, cout=64, hw=(40, 72), k=3, stride=1, pad=1, dil=1),          # 64 co x 32 ci tiles, two row segments
    dict(cin=48, cout=32, hw=(33, 65), k=3, stride=1, pad=2, dil=2),          # 32 co x 64 ci tiles, ragged channels and columns
    dict(cin=40, cout=16, hw=(20, 130), k=3, stride=1, pad=8, dil=8),         # 16 co x 64 ci tiles, widest halo
    dict(cin=32, cout=24, hw=(37, 135), k=3, stride=2, pad=0, dil=1),         # stride 2: two staging items per lane
    dict(cin=16, cout=3, hw=(24, 24), k=1, stride=1, pad=0, dil=1),           # ToRGB
    dict(cin=16, cout=32, hw=(26, 26), k=1, stride=2, pad=0, dil=1),          # ResBlock skip
    dict(cin=32, cout=64, hw=(16, 16), k=3, stride=1, pad=1, dil=1),          # small maps: 4 rows x 16 columns per chunk
    dict(cin=32, cout=64, hw=(33, 33), k=3, stride=2, pad=0, dil=1),          # ... 16 x 16 outputs at stride 2 (dense slab rows)
    dict(cin=16, cout=16, hw=(9, 8), k=3, stride=1, pad=1, dil=1),            # 8 x 8 chunks over a ragged map
    dict(cin=16, cout=16, hw=(4, 4), k=3, stride=1, pad=1, dil=1),            # 4 x 4 map
    dict(cin=24, cout=40, hw=(19, 30), k=3, stride=1, pad=2, dil=2),          # 2 rows x 32 columns, dilation 2
])
def test_conv2d_wgrad_tile_shapes(H, cfg):
    """vsp_conv2d_wgrad_f32 over its tile shapes / staging forms against torch autograd in float64."""
    c = cfg
    g_ = torch.Generator().manual_seed(21)
    B = 3
    x = torch.randn(B, c["cin"], *c["hw"], generator=g_)
    w = torch.zeros(c["cout"], c["cin"], c["k"], c["k"], dtype=torch.float64, requires_grad=True)
    with torch.enable_grad():
        y = F.conv2d(x.double(), w, None, c["stride"], c["pad"], c["dil"])
        gy = torch.randn(y.shape, generator=g_)
        y.backward(gy.double())
    dw = H.conv2d_wgrad(dev(x), dev(gy), w.shape, c["stride"], c["pad"], c["dil"], 1)
    close(dw, w.grad.float(), 2e-5, 2e-5 * float(w.grad.abs().max()), "dw")


@pytest.mark.parametrize("B,cin,cout,k", [(3, 40, 24, 3), (4, 512, 128, 3), (16, 64, 3, 1), (1, 7, 5, 3)])
def test_demod_weight_and_gradient(H, B, cin, cout, k):
    """vsp_demod_weight_f32 / _bwd_f32 (training: demodulation coefficients from the weight, gradient in style and weight) against
    torch autograd of the reference expression in float64."""
    g_ = torch.Generator().manual_seed(41)
    w = torch.randn(1, cout, cin, k, k, generator=g_)
    s, gy = torch.randn(B, cin, generator=g_), torch.randn(B, cout, generator=g_)
    scale = 1 / math.sqrt(cin * k * k)
    wd, sd = w.double().requires_grad_(True), s.double().requires_grad_(True)
    with torch.enable_grad():
        ref = torch.rsqrt(F.linear(sd * sd, wd[0].pow(2).sum((2, 3))) * scale ** 2 + 1e-8)
        ref.backward(gy.double())
    out, wsq = H.demod_weight(dev(s), dev(w), scale)
    close(out, ref.detach().float(), 1e-5, 1e-6, "demod")
    close(wsq, w[0].pow(2).sum((2, 3)), 1e-5, 1e-6, "wsq")
    ds, dw = H.demod_weight_bwd(dev(gy), out, dev(s), wsq, dev(w), scale)
    close(ds, sd.grad.float(), 2e-5, 2e-5 * float(sd.grad.abs().max()), "dstyle")
    close(dw, wd.grad.float(), 2e-5, 2e-5 * float(wd.grad.abs().max()), "dweight")
    assert dw.shape == w.shape
    ds2, dw2 = H.demod_weight_bwd(dev(gy), out, dev(s), wsq, dev(w), scale, need_style=False)
    assert ds2 is None and torch.equal(dw2, dw)
    # column windows of wider tensors (one row pitch for g and out) + accumulation into existing buffers
    wide_g, wide_o = torch.randn(B, cout + 7, generator=g_), torch.rand(B, cout + 7, generator=g_)
    wide_g[:, 3:3 + cout], wide_o[:, 3:3 + cout] = gy, out.cpu()
    ds0, dw0 = torch.randn(B, cin, generator=g_), torch.randn(w.shape, generator=g_)
    dsa, dwa = dev(ds0).clone(), dev(dw0).clone()
    H.demod_weight_bwd(dev(wide_g)[:, 3:3 + cout], dev(wide_o)[:, 3:3 + cout], dev(s), wsq, dev(w), scale, ds_out=dsa, dw_out=dwa, accumulate=True)
    close(dsa, ds0 + ds.cpu(), 2e-5, 2e-5 * float((ds0 + ds.cpu()).abs().max()), "accumulated dstyle")
    close(dwa, dw0 + dw.cpu(), 2e-5, 2e-5 * float((dw0 + dw.cpu()).abs().max()), "accumulated dweight")


@pytest.mark.parametrize("cin,cout,hw", [(3, 16, (32, 32)), (3, 40, (23, 27)), (1, 5, (7, 9)), (4, 64, (64, 48))])
def test_conv2d_wgrad_few_input_channels(H, cin, cout, hw):
    """The stream form of the 1x1 weight gradient (FromRGB: at most 4 input channels): per-sample scales, a channel window into a wider
    dy, ragged planes (no 16-byte rows), accumulation."""
    g_ = torch.Generator().manual_seed(23)
    B = 3
    x, s = torch.randn(B, cin, *hw, generator=g_), torch.rand(B, cin, generator=g_) + 0.5
    gy, dm = torch.randn(B, cout + 5, *hw, generator=g_), torch.rand(B, cout + 5, generator=g_) + 0.5
    ref = torch.einsum("bohw,bihw->oi", (gy[:, 5:] * dm[:, 5:, None, None]).double(), (x * s[:, :, None, None]).double()).float()[:, :, None, None]
    dw = H.conv2d_wgrad(dev(x), dev(gy), (cout, cin, 1, 1), 1, 0, 1, 1, x_scale=dev(s), dy_scale=dev(dm), dy_coff=5)
    close(dw, ref, 2e-5, 2e-5 * float(ref.abs().max()), "dw")
    dw2 = H.conv2d_wgrad(dev(x), dev(gy), (cout, cin, 1, 1), 1, 0, 1, 1, x_scale=dev(s), dy_scale=dev(dm), dy_coff=5, out=dw.clone(), accumulate=True)
    close(dw2, 2 * ref, 2e-5, 4e-5 * float(ref.abs().max()), "accumulated dw")
    plain = H.conv2d_wgrad(dev(x), dev(gy[:, :cout].contiguous()), (cout, cin, 1, 1), 1, 0)
    ref0 = torch.einsum("bohw,bihw->oi", gy[:, :cout].double(), x.double()).float()[:, :, None, None]
    close(plain, ref0, 2e-5, 2e-5 * float(ref0.abs().max()), "dw without scales")


def test_conv2d_wgrad_shared_input_groups(H):
    """The four dilated SMART branches as one weight-gradient launch: shared input, per-group dilation / padding, per-sample scales;
    channel window into a wider dy; accumulation."""
    g_ = torch.Generator().manual_seed(22)
    B, cin, cg, Hh, Ww = 2, 24, 16, 30, 70
    rates = (1, 2, 4, 8)
    x, s = torch.randn(B, cin, Hh, Ww, generator=g_), torch.rand(B, cin, generator=g_) + 0.5
    gy, dm = torch.randn(B, 4 * cg + 8, Hh, Ww, generator=g_), torch.rand(B, 4 * cg + 8, generator=g_) + 0.5
    refs = []
    for i, r in enumerate(rates):
        w = torch.zeros(cg, cin, 3, 3, dtype=torch.float64, requires_grad=True)
        with torch.enable_grad():
            y = F.conv2d((x * s[:, :, None, None]).double(), w, None, 1, r, r) * dm[:, 8 + i * cg:8 + (i + 1) * cg, None, None].double()
            y.backward(gy[:, 8 + i * cg:8 + (i + 1) * cg].double())
        refs.append(w.grad.float())
    ref = torch.cat(refs, 0)
    dw = H.conv2d_wgrad(dev(x), dev(gy), (4 * cg, cin, 3, 3), 1, rates, rates, 4, x_scale=dev(s), dy_scale=dev(dm), x_shared=True, dy_coff=8)
    close(dw, ref, 2e-5, 2e-5 * float(ref.abs().max()), "dw")
    dw2 = H.conv2d_wgrad(dev(x), dev(gy), (4 * cg, cin, 3, 3), 1, rates, rates, 4, x_scale=dev(s), dy_scale=dev(dm), x_shared=True, dy_coff=8,
                         out=dw.clone(), accumulate=True)
    close(dw2, 2 * ref, 2e-5, 4e-5 * float(ref.abs().max()), "accumulated dw")


@pytest.mark.parametrize("shape", [(3, 5, 7, 9), (2, 64, 128, 128), (4, 3, 512, 512), (5, 16)])
def test_channel_sum_and_plane_dot_split(H, shape):
    """vsp_channel_sum_f32 and the split form of vsp_plane_dot_f32 (several workgroups per plane) against float64 sums."""
    g_ = torch.Generator().manual_seed(8)
    a, b = torch.randn(*shape, generator=g_), torch.randn(*shape, generator=g_)
    dims = [0] + list(range(2, a.dim()))
    close(H.channel_sum(dev(a)), a.double().sum(dims).float(), 1e-5, 1e-3, "channel_sum")
    if a.dim() == 4:
        close(H.plane_dot(dev(a), dev(b)), (a.double() * b.double()).sum((2, 3)).float(), 1e-5, 1e-3, "plane_dot")


@pytest.mark.parametrize("shape", [(2, 6, 9, 7), (3, 16, 64, 64)])
def test_noise_bias_act_autograd(H, shape):
    """NoiseInjection + FusedLeakyReLU as one op (vspbfr_amd/training.py) against the two-step torch statement in float64:
    y, dx, d noise_weight, d bias."""
    from vspbfr_amd.training import noise_bias_act
    g_ = torch.Generator().manual_seed(9)
    B, C_, Hh, Ww = shape
    x, noise = torch.randn(*shape, generator=g_), torch.randn(B, 1, Hh, Ww, generator=g_)
    nw, bias = torch.tensor([0.3]), torch.randn(C_, generator=g_) * 0.2

    def ref_fn(x_, nw_, b_):
        return F.leaky_relu(x_ + nw_ * noise.double() + b_.view(1, -1, 1, 1), 0.2) * math.sqrt(2)
    ref = _grads(ref_fn, x.double(), nw.double(), bias.double())
    got = _grads(lambda x_, nw_, b_: noise_bias_act(x_, dev(noise), nw_, b_), dev(x), dev(nw), dev(bias))
    for name, a, r in zip(("y", "dx", "dnw", "db"), got, ref):
        close(a, r.float(), 2e-5, 2e-5, name)


@pytest.mark.parametrize("cfg", [
    dict(cin=12, cout=64, hw=(27, 27), k=4, stride=1, pad=0),      # the sub-pixel stem of the identity network
    dict(cin=40, cout=24, hw=(13, 18), k=3, stride=1, pad=1),      # ragged channels / tiles
    dict(cin=32, cout=32, hw=(17, 17), k=3, stride=2, pad=0),
    dict(cin=64, cout=48, hw=(8, 8), k=1, stride=1, pad=0),
])
def test_conv_every_config_agrees(H, cfg):
    """Every tile configuration that accepts a shape must give the cost model's result (summation order aside): a variant that merely
    RUNS on a shape nobody tried it on is how a tuned table would ship a wrong kernel."""
    from vspbfr_amd._lib import lib
    c = cfg
    g_ = torch.Generator().manual_seed(31)
    x = dev(torch.randn(2, c["cin"], *c["hw"], generator=g_))
    w = dev(torch.randn(c["cout"], c["cin"], c["k"], c["k"], generator=g_) / math.sqrt(c["cin"] * c["k"] ** 2))
    pc = H.PackedConv(H.pack_weight(w), 1, c["cout"], c["cin"], c["k"], c["k"], c["stride"], (1,), (c["pad"],))
    ref = F.conv2d(x.cpu().double(), w.cpu().double(), None, c["stride"], c["pad"]).float()
    ran = 0
    for i in range(lib.vsp_conv2d_num_configs() + 1):
        try:
            y = H.conv2d_packed(x, pc, tile_hint=i, winograd=False)
        except RuntimeError:
            continue
        ran += 1
        close(y, ref, 2e-5, 2e-5, "auto" if i == 0 else lib.vsp_conv2d_config_name(i - 1).decode())
    assert ran > 10


@pytest.mark.parametrize("cout,cin,k,groups", [(64, 48, 3, 1), (3, 512, 1, 1), (35, 7, 3, 1), (64, 3, 7, 1), (96, 20, 3, 4), (512, 512, 3, 1)])
def test_pack_weight_kernel(H, cout, cin, k, groups):
    """vsp_pack_weight_f32 against the layout statement wp[g][tap][ci][co_g] = scale * w[g cout_g + co_g][ci][tap'] in torch --
    straight, tap-flipped, and the adjoint form (channels exchanged: the data-gradient weight) -- bit-exact (one fp32 multiply)."""
    g_ = torch.Generator().manual_seed(12)
    w = torch.randn(cout, cin, k, k, generator=g_)
    scale = 0.37
    for flip in (False, True):
        got = H.pack_weight(dev(w), groups, flip=flip, scale=scale).cpu()
        ref = H.pack_weight(w, groups, flip=flip, scale=scale)          # host tensors take the torch expression
        assert got.shape == ref.shape and torch.equal(got, ref), f"pack flip={flip}"
        if groups == 1:
            got = H.pack_weight(dev(w), adjoint=True, flip=flip, scale=scale).cpu()
            wt = (w * scale).transpose(0, 1)
            ref = (wt.flip(2, 3) if flip else wt).reshape(1, cin, cout, k * k).permute(0, 3, 2, 1).contiguous()
            assert got.shape == ref.shape and torch.equal(got, ref), f"adjoint flip={flip}"
    if groups == 1:
        st = H.pack_weight_stack([dev(w), dev(w * 2)], adjoint=True, flip=True).cpu()
        assert torch.equal(st[1], 2 * st[0]) and torch.equal(st[0], H.pack_weight(w, adjoint=True, flip=True)[0])


@pytest.mark.parametrize("ng,cin,cout", [(1, 64, 64), (1, 6, 3), (4, 30, 24), (1, 130, 40), (2, 512, 128)])
def test_winograd_weight_kernel(H, ng, cin, cout):
    """vsp_winograd_weight_f32 against U = G g G^T in float64 (einsum), laid out in the fragment order include/vspbfr_hip.h states
    for vsp_conv2d_winograd_f32, zero padding included."""
    g_ = torch.Generator().manual_seed(13)
    wp = torch.randn(ng, 9, cin, cout, generator=g_)
    Gm = torch.tensor(((1.0, 0.0, 0.0), (0.5, 0.5, 0.5), (0.5, -0.5, 0.5), (0.0, 0.0, 1.0)), dtype=torch.float64)
    U = torch.einsum("ay,bx,gyxio->gabio", Gm, Gm, wp.double().view(ng, 3, 3, cin, cout)).reshape(ng, 16, cin, cout)
    ck, mb = H.lib.vsp_conv2d_winograd_chunk(), H.lib.vsp_conv2d_winograd_mbw(cout)
    nch, nct = (cin + ck - 1) // ck, (cout + 16 * mb - 1) // (16 * mb)
    Up = U.new_zeros(ng, 16, nch * ck, nct * 16 * mb)
    Up[:, :, :cin, :cout] = U
    ref = Up.view(ng, 8, 2, nch, 4, nct, mb, 16).permute(0, 5, 3, 1, 2, 4, 7, 6).float().contiguous().view(-1)
    got = H.winograd_weight(dev(wp)).cpu()
    assert got.numel() == ref.numel() == H.lib.vsp_winograd_weight_floats(ng, cin, cout)
    close(got, ref, 1e-7, 1.2e-7, "winograd weight")


@pytest.mark.parametrize("cin,cout,hw,B", [(1024, 256, 7, 8), (256, 1024, 7, 8), (2048, 512, 4, 8), (64, 40, 5, 3), (512, 128, 14, 2),
                                           (16, 3, 1, 1), (128, 512, 14, 8)])
def test_conv1x1_small_gemm(H, cin, cout, hw, B):
    """vsp_conv1x1_small_f32 (1x1 conv on a small map as a K-split GEMM) against F.conv2d in float64: plain, with bias, with
    bias + ReLU; through hip_ops.conv2d (which routes these shapes to it) and through the data-gradient path of conv2d_gradfix."""
    from vspbfr_amd.op import conv2d_gradfix
    g_ = torch.Generator().manual_seed(21)
    x, w = torch.randn(B, cin, hw, hw, generator=g_), torch.randn(cout, cin, 1, 1, generator=g_) / math.sqrt(cin)
    b = torch.randn(cout, generator=g_)
    ref = F.conv2d(x.double(), w.double())
    close(H.conv1x1_small(dev(x), dev(w).view(cout, cin)), ref.float(), 2e-5, 1e-4, "plain")
    close(H.conv2d(dev(x), dev(w), dev(b)), (ref + b.double().view(1, -1, 1, 1)).float(), 2e-5, 1e-4, "bias")
    close(H.conv2d(dev(x), dev(w), None, act2=1, bias2=dev(b), slope2=0.0, gain2=1.0),
          F.relu(ref + b.double().view(1, -1, 1, 1)).float(), 2e-5, 1e-4, "bias+relu")
    if cout % 16 == 0:
        gy = torch.randn(B, cout, hw, hw, generator=g_)
        with torch.no_grad():
            dx = conv2d_gradfix._dgrad(dev(gy), dev(w), x.shape, 1, 0, 1, 1)
        close(dx, F.conv_transpose2d(gy.double(), w.double()).float(), 2e-5, 1e-4, "dgrad")


@pytest.mark.parametrize("case", [
    dict(B=8, cin=512, cout=512, hw=(4, 4), k=3, stride=1, G=1),
    dict(B=3, cin=64, cout=40, hw=(9, 7), k=3, stride=1, G=1),
    dict(B=4, cin=128, cout=96, hw=(8, 8), k=3, stride=2, G=1),
    dict(B=2, cin=32, cout=64, hw=(16, 16), k=3, stride=1, G=4, dil=(1, 2, 4, 8)),      # dilation groups over one input
    dict(B=2, cin=16, cout=48, hw=(6, 6), k=3, stride=2, G=3, true_groups=True),         # true groups (style heads)
    dict(B=1, cin=2048, cout=512, hw=(1, 1), k=1, stride=1, G=1),
    dict(B=5, cin=48, cout=20, hw=(5, 5), k=1, stride=1, G=1),
], ids=lambda c: f"{c['cin']}-{c['cout']}-{c['hw'][0]}-k{c['k']}s{c['stride']}G{c['G']}")
def test_conv_smallmap_kernel(H, case):
    """The K-split small-map kernel (conv_smallmap.hip, configuration "smallmap") against the tiled kernel on the same launch
    parameters -- every prologue / epilogue operand of the contract switched on -- and against F.conv2d in float64 for the plain
    convolution."""
    c = case
    g_ = torch.Generator().manual_seed(41)
    B, cin, cout, (Hh, Ww), k, st, G = c["B"], c["cin"], c["cout"], c["hw"], c["k"], c["stride"], c["G"]
    sm = H.CONFIG_IDS["smallmap"]
    cg = cout // G
    true_groups = c.get("true_groups", False)
    dil = c.get("dil", (1,) * G)
    xc = cin * G if true_groups else cin
    x = dev(torch.randn(B, xc, Hh, Ww, generator=g_))
    ws = [torch.randn(cg, cin, k, k, generator=g_) / math.sqrt(cin * k * k) for _ in range(G)]
    pad = tuple(d * (k // 2) for d in dil) if st == 1 else (0,) * G
    wp = H.pack_weight_stack([dev(w_) for w_ in ws])
    if G == 1:
        pc = H.PackedConv(wp, 1, cg, cin, k, k, st, (dil[0],), (pad[0],))
    elif true_groups:
        pc = H.PackedConv(wp, G, cg, cin, k, k, st, (1,), (pad[0],), x_group_stride=cin)
    else:
        pc = H.PackedConv(wp, G, cg, cin, k, k, st, dil, pad)
    # plain convolution against float64
    refs = []
    for gi in range(G):
        xi = x.cpu().double()[:, gi * cin:(gi + 1) * cin] if true_groups else x.cpu().double()
        refs.append(F.conv2d(xi, ws[gi].double(), None, st, pad[gi], dil[gi]))
    ref = torch.cat(refs, 1).float()
    y = H.conv2d_packed(x, pc, tile_hint=sm, winograd=False)
    close(y, ref, 2e-5, 2e-5, "plain")
    OH, OW = ref.shape[2:]
    # every operand of the contract, against the tiled kernel
    s_in = dev(torch.rand(B, xc, generator=g_) + 0.5)
    kw = dict(in_scale=s_in, out_scale=dev(torch.rand(B, cout, generator=g_) + 0.5), act1=True, bias1=dev(torch.randn(cout, generator=g_)),
              noise=dev(torch.randn(B, 1, OH, OW, generator=g_)), noise_w=dev(torch.tensor([0.3])), act2=1,
              bias2=dev(torch.randn(cout, generator=g_)), res1=dev(torch.randn(B, cout, OH, OW, generator=g_)),
              res2=dev(torch.randn(B, cout, OH, OW, generator=g_)))
    close(H.conv2d_packed(x, pc, tile_hint=sm, winograd=False, **kw), H.conv2d_packed(x, pc, winograd=False, bf16=False, **kw), 3e-5, 3e-5, "epilogue")
    if not true_groups:
        kw2 = dict(in_scale=dev(torch.rand(xc, generator=g_) + 0.5), in_scale_per_sample=False, in_shift=dev(torch.randn(xc, generator=g_)),
                   ch_scale=dev(torch.rand(cout, generator=g_) + 0.5), ch_bias=dev(torch.randn(cout, generator=g_)), act2=2,
                   prelu=dev(torch.rand(cout, generator=g_)))
        close(H.conv2d_packed(x, pc, tile_hint=sm, winograd=False, **kw2), H.conv2d_packed(x, pc, winograd=False, bf16=False, **kw2), 3e-5, 3e-5,
              "folded-BN operands")
    # strided placement into a larger output (sub-pixel phase form)
    out_a = torch.zeros(B, cout + 3, 2 * OH + 1, 2 * OW + 2, device=x.device)
    out_b = torch.zeros_like(out_a)
    H.conv2d_packed(x, pc, out=out_a, y_coff=2, out_stride=(2, 2), out_offset=(1, 1), tile_hint=sm, winograd=False)
    H.conv2d_packed(x, pc, out=out_b, y_coff=2, out_stride=(2, 2), out_offset=(1, 1), winograd=False, bf16=False)
    close(out_a, out_b, 3e-5, 3e-5, "placement")


@pytest.mark.parametrize("case", [
    dict(B=2, cin=32, cout=160, hw=(37, 41), stride=2, pad=1),                         # ragged tiles and channel tiles, stride 2
    dict(B=3, cin=16, cout=24, hw=(33, 33), stride=2, pad=0),                          # StyledConv_down geometry (odd map, no padding)
    dict(B=2, cin=24, cout=72, hw=(21, 50), stride=1, pad=1),
    dict(B=1, cin=8, cout=40, hw=(40, 24), stride=1, pad=3, dil=3),
    dict(B=2, cin=16, cout=64, hw=(48, 40), stride=1, G=4, dil=(1, 2, 4, 8)),          # the four dilated SMART branches
    dict(B=2, cin=8, cout=32, hw=(19, 23), stride=1, G=4, dil=(1, 2, 4, 8)),
    dict(B=2, cin=16, cout=48, hw=(22, 22), stride=2, pad=1, G=3, true_groups=True),   # true groups (style heads)
    dict(B=2, cin=16, cout=40, hw=(32, 32), transposed=True),                          # up-conv: tiles + edge strips
    dict(B=3, cin=8, cout=20, hw=(13, 21), transposed=True),                           # up-conv: ragged tiles
], ids=lambda c: f"{c['cin']}-{c['cout']}-{c['hw'][0]}x{c['hw'][1]}-s{c.get('stride', 1)}G{c.get('G', 1)}{'t' if c.get('transposed') else ''}")
def test_conv_pipelined_kernels(H, case):
    """Every configuration of the double-buffered pipeline kernels (conv_pipe.hip, names "...p3...") that accepts the launch: the
    plain convolution against F.conv2d / F.conv_transpose2d in float64, then every prologue / epilogue operand of the contract
    against the tiled kernel (conv_igemm_kernel) on the same launch parameters.

    A smoke test of the family through conv2d_packed: an instance that refuses a shape is skipped here, and y is allocated exactly.  Which of the
    33 instances serves which case, every refusal by its rule, the sentinel around the written region, separate strides and pads, channel
    windows, workgroup order 2 and every nchunk class of the `fd` interval are held by tests/test_conv_pipe_forms_gpu.py (each case on every
    instance by name against float64 under conv_tile_ref.bound), with tests/test_conv_pipe_ref.py proving the reach of its table."""
    from vspbfr_amd._lib import lib
    c = case
    g_ = torch.Generator().manual_seed(53)
    B, cin, cout, (Hh, Ww) = c["B"], c["cin"], c["cout"], c["hw"]
    st, G, tr = c.get("stride", 1), c.get("G", 1), c.get("transposed", False)
    true_groups = c.get("true_groups", False)
    cg = cout // G
    dil = c.get("dil", 1)
    dil = dil if isinstance(dil, tuple) else (dil,) * G
    pad = tuple(dil) if G == 4 and not true_groups else (c.get("pad", 0),) * G
    xc = cin * G if true_groups else cin
    x = dev(torch.randn(B, xc, Hh, Ww, generator=g_))
    ws = [torch.randn(cg, cin, 3, 3, generator=g_) / math.sqrt(cin * 9) for _ in range(G)]
    wp = H.pack_weight_stack([dev(w_) for w_ in ws])
    if tr:
        pc = H.PackedConv(wp, 1, cout, cin, 3, 3, 1, (1,), (0,))
        ref = F.conv_transpose2d(x.cpu().double(), ws[0].double().transpose(0, 1), stride=2).float()
    else:
        if G == 1:
            pc = H.PackedConv(wp, 1, cg, cin, 3, 3, st, (dil[0],), (pad[0],))
        elif true_groups:
            pc = H.PackedConv(wp, G, cg, cin, 3, 3, st, (1,), (pad[0],), x_group_stride=cin)
        else:
            pc = H.PackedConv(wp, G, cg, cin, 3, 3, st, dil, pad)
        refs = []
        for gi in range(G):
            xi = x.cpu().double()[:, gi * cin:(gi + 1) * cin] if true_groups else x.cpu().double()
            refs.append(F.conv2d(xi, ws[gi].double(), None, st, pad[gi], dil[gi]))
        ref = torch.cat(refs, 1).float()
    OH, OW = ref.shape[2:]
    s_in = dev(torch.rand(B, xc, generator=g_) + 0.5)
    kw = dict(in_scale=s_in, out_scale=dev(torch.rand(B, cout, generator=g_) + 0.5), act1=True, bias1=dev(torch.randn(cout, generator=g_)),
              act2=1, bias2=dev(torch.randn(cout, generator=g_)))
    if not tr:   # (the transposed mode has no noise / residual epilogue: they follow the blur)
        kw.update(noise=dev(torch.randn(B, 1, OH, OW, generator=g_)), noise_w=dev(torch.tensor([0.3])),
                  res1=dev(torch.randn(B, cout, OH, OW, generator=g_)), res2=dev(torch.randn(B, cout, OH, OW, generator=g_)))
    kw2 = dict(in_scale=dev(torch.rand(xc, generator=g_) + 0.5), in_scale_per_sample=False, ch_scale=dev(torch.rand(cout, generator=g_) + 0.5),
               ch_bias=dev(torch.randn(cout, generator=g_)), act2=2, prelu=dev(torch.rand(cout, generator=g_)))
    base = dict(transposed=tr, winograd=False, bf16=False)
    want, want2 = H.conv2d_packed(x, pc, **base, **kw), H.conv2d_packed(x, pc, **base, **kw2)

    # The same two operand chains restated in float64 torch from the contract of include/vspbfr_hip.h (the pipelined
    # kernels' operands were only checked against the tiled kernel): y = act2(act1(conv(x * in_scale) * out_scale * ch_scale + ch_bias + bias1)
    # + noise * noise_w + bias2) + res1 + res2
    def conv64(xs):
        if tr:
            return F.conv_transpose2d(xs, ws[0].double().transpose(0, 1), stride=2)
        outs = []
        for gi in range(G):
            xi = xs[:, gi * cin:(gi + 1) * cin] if true_groups else xs
            outs.append(F.conv2d(xi, ws[gi].double(), None, st, pad[gi], dil[gi]))
        return torch.cat(outs, 1)
    c64 = lambda t: t.cpu().double()
    v = conv64(c64(x) * c64(kw["in_scale"]).view(B, xc, 1, 1)) * c64(kw["out_scale"]).view(B, cout, 1, 1) + c64(kw["bias1"]).view(1, -1, 1, 1)
    v = F.leaky_relu(v, 0.2) * math.sqrt(2)
    if "noise" in kw:
        v = v + c64(kw["noise"]) * 0.3
    v = F.leaky_relu(v + c64(kw["bias2"]).view(1, -1, 1, 1), 0.2) * math.sqrt(2)
    if "res1" in kw:
        v = v + c64(kw["res1"]) + c64(kw["res2"])
    close(want, v.float(), 5e-5, 5e-5, "tiled kernel, epilogue chain vs float64")
    v2 = conv64(c64(x) * c64(kw2["in_scale"]).view(1, xc, 1, 1)) * c64(kw2["ch_scale"]).view(1, -1, 1, 1) + c64(kw2["ch_bias"]).view(1, -1, 1, 1)
    v2 = torch.where(v2 > 0, v2, v2 * c64(kw2["prelu"]).view(1, -1, 1, 1))
    close(want2, v2.float(), 5e-5, 5e-5, "tiled kernel, per-channel operands vs float64")
    ran = 0
    for i in range(lib.vsp_conv2d_num_configs()):
        name = lib.vsp_conv2d_config_name(i).decode()
        if "p3" not in name:
            continue
        try:
            y = H.conv2d_packed(x, pc, tile_hint=i + 1, **base)
        except RuntimeError:
            continue   # this configuration does not serve the launch (mode, patch rows, chunk size)
        ran += 1
        close(y, ref, 2e-5, 2e-5, name + " plain")
        close(H.conv2d_packed(x, pc, tile_hint=i + 1, **base, **kw), v.float(), 5e-5, 5e-5, name + " epilogue vs float64")
        close(H.conv2d_packed(x, pc, tile_hint=i + 1, **base, **kw2), v2.float(), 5e-5, 5e-5, name + " per-channel operands vs float64")
        if not tr and st == 1 and G == 1:   # strided placement into a larger tensor, channel window
            out_a = torch.zeros(B, cout + 3, 2 * OH + 1, 2 * OW + 2, device=x.device)
            out_b = torch.zeros_like(out_a)
            H.conv2d_packed(x, pc, out=out_a, y_coff=2, out_stride=(2, 2), out_offset=(1, 1), tile_hint=i + 1, **base)
            H.conv2d_packed(x, pc, out=out_b, y_coff=2, out_stride=(2, 2), out_offset=(1, 1), **base)
            close(out_a, out_b, 3e-5, 3e-5, name + " placement")
    assert ran >= 2, "no pipelined configuration accepted this launch"


@pytest.mark.parametrize("cin,cout,hw", [(64, 64, (40, 56)), (128, 32, (33, 20)), (64, 128, (16, 16))])
def test_conv_dilation_by_input_quarter(H, cin, cout, hw):
    """vsp_conv_params.dil_by_input_quarter (conv_pipe.hip MODE 3): y = sum_q conv(x[q-th quarter], W_q, dilation = padding = d_q) as
    ONE convolution -- the data gradient of the four dilated SMART branches -- with the per-sample input / output scales and a bias.

    tile_hint = 0 takes the first `a` instance of the table that fits, which is 4x2x1x8x4k1p3o2r8a for all three shapes; the four `a` instances
    by name, the (Cin / 4) % CK refusal, 12 channels per block, dilations other than 1, 2, 4, 8 and the whole epilogue chain are in
    tests/test_conv_pipe_forms_gpu.py (shapes a16 ... a128, a64d of tests/conv_pipe_ref.py)."""
    g_ = torch.Generator().manual_seed(31)
    B, rates, c = 2, (1, 2, 4, 8), cin // 4
    x = torch.randn(B, cin, *hw, generator=g_)
    ws = [torch.randn(cout, c, 3, 3, generator=g_) * 0.1 for _ in rates]
    s, dm, bias = torch.rand(B, cin, generator=g_) + 0.5, torch.rand(B, cout, generator=g_) + 0.5, torch.randn(cout, generator=g_)
    xs = (x * s[:, :, None, None]).double()
    ref = sum(F.conv2d(xs[:, q * c:(q + 1) * c], ws[q].double(), None, 1, r, r) for q, r in enumerate(rates))
    ref = (ref * dm[:, :, None, None].double() + bias[None, :, None, None].double()).float()
    wp = H.pack_weight(dev(torch.cat(ws, 1)))                                   # (1, 9, Cin, Cout)
    w4 = wp.view(9, cin, 4, cout // 4).permute(2, 0, 1, 3).contiguous()         # four blocks of Cout / 4 output channels
    pc = H.PackedConv(w4, 4, cout // 4, cin, 3, 3, 1, rates, rates, dil_by_input_quarter=True)
    y = H.conv2d_packed(dev(x), pc, in_scale=dev(s), out_scale=dev(dm), ch_bias=dev(bias))
    close(y, ref, 2e-5, 2e-5 * float(ref.abs().max()), "y")
    with pytest.raises(RuntimeError):   # the Winograd / bf16 entries do not serve it
        H.conv2d_packed(dev(x), pc, winograd=True)
    if cin == 64 and cout == 64:   # what the entry refuses: input channels that do not split into quarters of whole chunks, the transposed form
        bad = H.PackedConv(w4[:, :, :40].contiguous(), 4, cout // 4, 40, 3, 3, 1, rates, rates, dil_by_input_quarter=True)
        with pytest.raises(RuntimeError):
            H.conv2d_packed(dev(x[:, :40].contiguous()), bad)
        with pytest.raises(RuntimeError):
            H.conv2d_packed(dev(x), pc, transposed=True)


def test_conv_pipelined_refuses_what_it_does_not_serve(H):
    """A named pipelined configuration must refuse (not mis-compute) launches outside its contract: an input shift, Cin that is not a
    multiple of the chunk, a 1x1 kernel."""
    pid = next(v for k, v in H.CONFIG_IDS.items() if "p3" in k and not k.endswith(("t", "d")))
    g_ = torch.Generator().manual_seed(3)
    x = dev(torch.randn(1, 16, 20, 20, generator=g_))
    w = dev(torch.randn(32, 16, 3, 3, generator=g_))
    pc = H.PackedConv(H.pack_weight(w), 1, 32, 16, 3, 3, 1, (1,), (1,))
    with pytest.raises(RuntimeError):
        H.conv2d_packed(x, pc, tile_hint=pid, in_shift=dev(torch.randn(16, generator=g_)), winograd=False, bf16=False)
    x5 = dev(torch.randn(1, 5, 20, 20, generator=g_))
    pc5 = H.PackedConv(H.pack_weight(dev(torch.randn(32, 5, 3, 3, generator=g_))), 1, 32, 5, 3, 3, 1, (1,), (1,))
    with pytest.raises(RuntimeError):
        H.conv2d_packed(x5, pc5, tile_hint=pid, winograd=False, bf16=False)
    pc1 = H.PackedConv(H.pack_weight(dev(torch.randn(32, 16, 1, 1, generator=g_))), 1, 32, 16, 1, 1, 1, (1,), (0,))
    with pytest.raises(RuntimeError):
        H.conv2d_packed(x, pc1, tile_hint=pid, winograd=False, bf16=False)


def test_conv_smallmap_random_shapes(H):
    """Thirty seeded random small-map problems (ragged channel counts, odd maps, both strides, dilation, 1x1 / 3x3 / 5x5 kernels,
    batch 1..9): the small-map kernel against F.conv2d in float64, with the per-sample input scale folded in.  (G = 1 and in_scale only; which
    of the five instantiations a launch takes, groups, in_shift, placement and the epilogue chain: tests/test_conv_pipe_forms_gpu.py.)"""
    rng = np.random.default_rng(77)
    sm = H.CONFIG_IDS["smallmap"]
    for it in range(30):
        B, cin, cout = int(rng.integers(1, 10)), 16 * int(rng.integers(1, 9)), int(rng.integers(1, 70))
        Hh, Ww = int(rng.integers(1, 13)), int(rng.integers(1, 13))
        k = int(rng.choice([1, 3, 3, 5]))
        st = int(rng.choice([1, 1, 2]))
        dil = 1 if st == 2 or k == 1 else int(rng.choice([1, 2, 3]))
        pad = int(rng.integers(0, dil * (k // 2) + 1))
        if (Hh + 2 * pad - dil * (k - 1) - 1) < 0 or (Ww + 2 * pad - dil * (k - 1) - 1) < 0:
            continue
        g_ = torch.Generator().manual_seed(1000 + it)
        x, w = torch.randn(B, cin, Hh, Ww, generator=g_), torch.randn(cout, cin, k, k, generator=g_) / math.sqrt(cin * k * k)
        s_in = torch.rand(B, cin, generator=g_) + 0.5
        pc = H.PackedConv(H.pack_weight(dev(w)), 1, cout, cin, k, k, st, (dil,), (pad,))
        ref = F.conv2d(x.double() * s_in.double().view(B, cin, 1, 1), w.double(), None, st, pad, dil).float()
        y = H.conv2d_packed(dev(x), pc, in_scale=dev(s_in), tile_hint=sm, winograd=False, bf16=False)
        close(y, ref, 3e-5, 3e-5, f"case {it}: B{B} {cin}->{cout} {Hh}x{Ww} k{k} s{st} d{dil} p{pad}")


@pytest.mark.parametrize("shape", [(2, 6, 9, 7), (3, 16, 64, 64), (1, 3, 5, 5)])
def test_smart_tail_backward(H, shape):
    """vsp_smart_tail_bwd_f32 (FusedLeakyReLU(b1) -> NoiseInjection -> FusedLeakyReLU(b2), backward from the final output alone)
    against torch autograd over the three-step statement in float64: gradient entering the conv, d b1, d b2, d noise weight."""
    g_ = torch.Generator().manual_seed(17)
    B, C_, Hh, Ww = shape
    x, noise = torch.randn(*shape, generator=g_), torch.randn(B, 1, Hh, Ww, generator=g_)
    b1, b2, nw = torch.randn(C_, generator=g_) * 0.3, torch.randn(C_, generator=g_) * 0.3, torch.tensor([0.4])
    gy = torch.randn(*shape, generator=g_)
    s2 = math.sqrt(2)

    def tail(x_, b1_, nw_, b2_):
        y1 = F.leaky_relu(x_ + b1_.view(1, -1, 1, 1), 0.2) * s2
        return F.leaky_relu(y1 + nw_ * noise.double() + b2_.view(1, -1, 1, 1), 0.2) * s2
    with torch.enable_grad():
        args = [t.double().requires_grad_(True) for t in (x, b1, nw, b2)]
        y = tail(*args)
        dx, db1, dnw, db2 = torch.autograd.grad(y, args, gy.double())
    g1, gb1, gb2, gnw = H.smart_tail_bwd(dev(gy), dev(y.detach().float()), dev(noise), dev(nw), dev(b2))
    # elements whose first activation sits within rounding of zero may take the other slope: exclude |y1| < 1e-5 from the pointwise check
    y1 = (F.leaky_relu(x.double() + b1.double().view(1, -1, 1, 1), 0.2) * s2)
    safe = (y1.abs() > 1e-5)
    assert float(((g1.cpu().double() - dx).abs() * safe).max()) < 1e-5
    close(gb1, db1.float(), 1e-4, 1e-4, "d bias1")
    close(gb2, db2.float(), 1e-4, 1e-4, "d bias2")
    close(gnw, dnw.float(), 1e-4, 1e-4, "d noise weight")


@pytest.mark.gpu
def test_bf16_pair_staging_bit_identical():
    """bf16-activation conv kernel: pixel-pair staging tasks (one aligned 4-byte load for two neighbouring pixels) against the one-pixel tasks
    (VSP_BF16_PAIR=0) -- bit-identical over stride-1 (plain, dilation groups, ragged maps), stride-2 (padding 0 / 1) and transposed launches
    and their tile variants.  The switch is read once per process: tools/ab_bf16_pair.py runs both settings as child processes."""
    import os, subprocess, sys
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    r = subprocess.run([sys.executable, os.path.join(root, "tools", "ab_bf16_pair.py")], env=dict(os.environ, QUICK="1"), capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-2000:]
    assert r.stdout.count("bit-identical") >= 15, r.stdout[-3000:]
