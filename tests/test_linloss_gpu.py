"""GPU checks of csrc/gemm_small.hip, csrc/style_plan.hip and csrc/lossops.hip against the float64 restatements of
tests/linloss_ref.py, at the smallest shapes that reach every compiled form and loop body:
    gemm_nt_kernel<true,1> (vector loop with K % 16 and masked K % 4 tails, idle waves, K = 0, batched), gemm_nt_kernel<false,1>
    (misaligned base, k-major operand), gemm_nt_kernel<true,4> (wide: M = 1024 exactly, partial row groups / column blocks, K tail,
    Z = 2), gemm_nt_kernel<true,2> and gemm_nt_kernel<true,8> (child processes under VSP_TUNE=1 VSP_GEMM_MBK), gemv_rows_kernel<8> /
    gemv_rows_kernel<16> and the tiled kernel in their place (child process under VSP_GEMV_OFF);
    style_mods_kernel<8> / style_mods_kernel<16> + style_demods_kernel on a mixed table;
    maxpool_fwd_kernel / maxpool_bwd_kernel and maxpool2x2_fwd_kernel / maxpool2x2_bwd_kernel (geometries, fallbacks, second grid passes,
    NaN / inf); lpips_layer_reg_kernel<1>, <2>, <4> forward and backward with lpips_layer_fwd_kernel / lpips_layer_bwd_kernel (the
    generic pair), around a wave's pixel count and past the grid caps; resize_bilinear_bwd_kernel as a scatter and as the adjoint of
    resize_bilinear_kernel.

Bound (stream_ref.bound): max |HIP - float64| <= 4 e_ref + 2e-6 max |float64| with e_ref the error of the same restatement run in
float32 on the CPU; max-pool outputs and the element that receives a max-pool gradient are exact.  Every comparison prints its
e_ref / e_hip / ratio line under -s; one full run is kept in profiles/linloss_gputest.log.  tests/test_linloss_ref.py shows on the CPU
that wrong variants of each family miss this bound on these very inputs.  Every output lives in a buffer of the test's own with
GUARD sentinel elements behind it (between them, for the style plan).

Worst ratio e_hip / e_ref per family in the recorded run (the bound is 4 e_ref + the additive term):
    gemm_nt_kernel<*,1> 1.07 (the plain 2 x 5 x 7 x 16 launch of the refusal test; 17 x 33 x 20 0.97), wide form 0.61 -- MBK 2 and 8 the same
    bits, so the same figure --, gemv 0.57, the tiled kernel in its place 2.76 (13 x 32 x 4096: four chains of 1024 products);
    style mod 1.04, style demod 1.58; max-pool exact throughout;
    LPIPS forward 2.27 (work-buffer form) / 2.74 (atomic form, small maps), past the grid caps 1.00; LPIPS gradient 2.05 on ordinary
    pixels, 1.44 on all-zero pixels of f1, past the grid caps 1.01; resize adjoint 1.67, its forward 1.25.
One group prints more than 4 and passes through the 2e-6 max |ref| term: the LPIPS gradient at the planted pixel of tiny norm, 5.27
(C = 64, HW = 64) and 7.25 (C = 192, HW = 257), every other case <= 3.6.  There g r and f1 k2 are ~1e5 each and cancel; the kernels
add |f1|^2 and the dot product as fmaf chains over the channels, torch in blocks.  tests/test_linloss_ref.py::test_order_lpips_backward
evaluates those chains in float32 on the CPU, on these inputs: the identical 5.27 and 7.25, within the bound.
What this suite found: (1) max-pool sent the gradient of a window with several NaNs to the FIRST of them, ATen to the last
(two_nan_diag, two_nan_row, three_nan fail on the parent's library at 2x2/2 and 3x3/2 p1; fixed in window_argmax / argmax4);
(2) vsp_lpips_layer_f32 past its grid cap missed the bound on about every second run (C = 256, HW = 131142: 2.0e-6 of the result on
average over 300 launches, 2.4e-6 at worst, against 2e-6 allowed: 2048 atomics onto one float; over five other inputs the error
was +-0.2 ... 0.9e-6) -- hip_ops.lpips_layer now calls vsp_lpips_layer_ws_f32, which adds the block sums in a fixed order (5.8e-9)."""
import ctypes
import os
import subprocess
import sys

import pytest
import torch
import torch.nn.functional as F

import linloss_ref as R
from stream_ref import bound

pytestmark = pytest.mark.gpu
DEV = "cuda"
F64, F32 = torch.float64, torch.float32
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GUARD = 1024
SENTINEL = 7.0
EINVAL = -1


@pytest.fixture(autouse=True)
def _grad_on():
    """(other test modules switch autograd off for the process at import)"""
    with torch.enable_grad():
        yield


@pytest.fixture(scope="module")
def H():
    from vspbfr_amd import hip_ops
    return hip_ops


def dev(t):
    return None if t is None else t.to(DEV)


def to_dev(t):
    """a CPU view on the device with its WHOLE storage: pitches, gaps and the offset of the base pointer arrive as they are"""
    whole = torch.as_strided(t, (t.untyped_storage().nbytes() // t.element_size(),), (1,), 0)
    return torch.as_strided(whole.to(DEV), t.shape, t.stride(), t.storage_offset())


def _guarded(numel, offset=0, fill=SENTINEL):
    """(buffer, view of `numel` floats that starts `offset` floats into it) with at least GUARD sentinels behind the view"""
    buf = torch.full((offset + numel + GUARD,), fill, dtype=F32, device=DEV)
    return buf, buf[offset:offset + numel]


def _guard_intact(buf, numel, what, offset=0):
    torch.cuda.synchronize()
    assert bool((buf[offset + numel:] == SENTINEL).all()) and bool((buf[:offset] == SENTINEL).all()), f"{what}: wrote outside its output"


def _lib():
    from vspbfr_amd._lib import last_error, lib
    return lib, last_error


# ================================================================================================== small GEMM
def _gemm(H, kw, what):
    """one launch of the case through H.gemm_nt into a guarded buffer: the (Z?, M, N) result"""
    a, b = kw["a"], kw["b"]
    M, K, N = a.shape[-2], a.shape[-1], b.shape[-2]
    epi = dict(alpha=kw["alpha"], bias=dev(kw["bias"]), bias_scale=kw["bias_scale"], act=kw["act"], bias_zs=kw.get("bias_zs", 0))
    shape = (M, N) if a.dim() == 2 else (a.shape[0], M, N)
    numel = M * N * (1 if a.dim() == 2 else a.shape[0])
    buf, out = _guarded(numel)
    if K == 0:      # (an empty tensor has no pointer to hand over: explicit dims over operands of pitch 4)
        H.gemm_nt(torch.zeros(M, 4, device=DEV), torch.zeros(N, 4, device=DEV), out=out.view(1, M, N), dims=(1, M, N, 0), a_strides=(0, 4, 1),
                  b_strides=(0, 4, 1), **epi)
    else:
        H.gemm_nt(to_dev(a), to_dev(b), out=out.view(shape), **epi)
    _guard_intact(buf, numel, what)
    return out.view(shape)


@pytest.mark.parametrize("name", [n for n in R.GEMM_CASES if n not in R.WIDE_CASES])   # (each case's loop body / branch: beside its entry in
#                                                                                        linloss_ref.GEMM_CASES; the tiled_* ones take
#                                                                                        gemv_rows_kernel<8> / <16> here, K / 256 = 4 and 16)
def test_gemm_forms(H, name):
    kw = R.gemm_case(name)
    got = _gemm(H, kw, name)
    bound(got, R.gemm_nt(**kw, dtype=F64), R.gemm_nt(**kw, dtype=F32), f"gemm {name}")
    if name.startswith("k0"):
        N = kw["b"].shape[0]
        want = R.epilogue(kw["bias"][:N] * torch.tensor(kw["bias_scale"]), 1, torch.tensor(0.2), torch.tensor(R.SQRT2))
        assert float((got.cpu() - want.view(1, N)).abs().max()) <= 1e-6                # the epilogue of the bias, in every row


def _wide(H, name):
    kw = R.gemm_case(name)
    return kw, _gemm(H, kw, name)


@pytest.mark.parametrize("name", list(R.WIDE_CASES))   # gemm_nt_kernel<true,4>: see linloss_ref.WIDE_CASES for what each shape reaches
def test_gemm_wide_form(H, name):
    """against float64, nothing outside the output, and BIT-identical to the same rows launched in slices of 600 (< 1024: the one-block
    form gemm_nt_kernel<true,1>): the kernel comment promises the same arithmetic per element for every MBK"""
    kw, got = _wide(H, name)
    bound(got, R.gemm_nt(**kw, dtype=F64), R.gemm_nt(**kw, dtype=F32), f"gemm {name}")
    a, b, bias = dev(kw["a"]), dev(kw["b"]), dev(kw["bias"])
    epi = dict(alpha=kw["alpha"], bias_scale=kw["bias_scale"], act=kw["act"])
    M, zs = a.shape[-2], kw.get("bias_zs", 0)
    for z in range(a.shape[0] if a.dim() == 3 else 1):
        az, bz, gz = (a, b, got) if a.dim() == 2 else (a[z], b[z], got[z])
        parts = torch.cat([H.gemm_nt(az[i:i + 600], bz, bias=bias[z * zs:], **epi) for i in range(0, M, 600)], 0)
        assert torch.equal(gz, parts), f"{name} z={z}: {int((gz != parts).sum())} elements differ from the sliced launches"


def _gemm_params(H, a, b, out, Z, M, N, K, **over):
    from vspbfr_amd._lib import GemmParams
    p = GemmParams()
    p.A, p.Bm, p.C = (None if a is None else a.data_ptr()), (None if b is None else b.data_ptr()), (None if out is None else out.data_ptr())
    p.Z, p.M, p.N, p.K = Z, M, N, K
    p.a_zs, p.a_ms, p.a_ks, p.b_zs, p.b_ns, p.b_ks, p.c_zs, p.c_ms = M * K, K, 1, N * K, K, 1, M * N, N
    p.alpha, p.bias, p.bias_scale, p.act, p.slope, p.gain, p.bias_zs = 1.0, None, 1.0, 0, 0.2, R.SQRT2, 0
    for k, v in over.items():
        setattr(p, k, v)
    return p


def test_gemm_empty_launches_and_refusals(H):
    """Z = 0, M = 0, N = 0: VSP_OK without a launch (null pointers allowed); act = 3, a negative dimension, Z = 65536, a null operand with
    non-empty dims: VSP_EINVAL; the buffer keeps its sentinel throughout"""
    lib, last_error = _lib()
    g = R._gen(2, 5, 7, 16)
    a, b = torch.randn(2 * 5 * 16, generator=g).to(DEV), torch.randn(2 * 7 * 16, generator=g).to(DEV)
    buf, out = _guarded(2 * 5 * 7)
    for Z, M, N in ((0, 5, 7), (2, 0, 7), (2, 5, 0)):
        assert lib.vsp_gemm_f32(ctypes.byref(_gemm_params(H, a, b, out, Z, M, N, 16)), H._stream()) == 0, last_error()
        assert lib.vsp_gemm_f32(ctypes.byref(_gemm_params(H, None, None, None, Z, M, N, 16)), H._stream()) == 0, last_error()
    refused = {"unknown activation": _gemm_params(H, a, b, out, 2, 5, 7, 16, act=3),
               "negative dimension": _gemm_params(H, a, b, out, 2, 5, 7, -1),
               "negative dimension ": _gemm_params(H, a, b, out, 2, -5, 7, 16),
               "batch too large": _gemm_params(H, a, b, out, 65536, 5, 7, 16, a_zs=0, b_zs=0, c_zs=0),
               "null tensor pointer": _gemm_params(H, None, b, out, 2, 5, 7, 16),
               "null tensor pointer ": _gemm_params(H, a, b, None, 2, 5, 7, 16)}
    for msg, p in refused.items():
        assert lib.vsp_gemm_f32(ctypes.byref(p), H._stream()) == EINVAL and msg.strip() in last_error(), (msg, last_error())
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())
    assert lib.vsp_gemm_f32(ctypes.byref(_gemm_params(H, a, b, out, 2, 5, 7, 16)), H._stream()) == 0      # (the same operands do launch)
    _guard_intact(buf, 70, "gemm 2x5x7x16")
    bound(out.view(2, 5, 7), R.gemm_nt(a.cpu().view(2, 5, 16), b.cpu().view(2, 7, 16)), R.gemm_nt(a.cpu().view(2, 5, 16), b.cpu().view(2, 7, 16), dtype=F32),
          "gemm 2x5x7x16 plain")


# ================================================================================================== style plan
STRIP = 64


def _style_table(layers_dev, outs, B, K):
    from vspbfr_amd import layers as LY
    arr = (LY._StyleLayerC * len(layers_dev))()
    for i, ((w, bias, wsq, alpha, bs, ws), (mod, demod), (cin, cout, _d, _b, row)) in enumerate(zip(layers_dev, outs, R.STYLE_LAYERS)):
        t = arr[i]
        t.w, t.bias, t.wsq = w.data_ptr(), (None if bias is None else bias.data_ptr()), (None if wsq is None else wsq.data_ptr())
        t.mod, t.demod = mod.data_ptr(), (None if demod is None else demod.data_ptr())
        t.src_off, t.cin, t.cout = row * K, cin, (cout if wsq is not None else 0)
        w32 = ctypes.c_float(ws if wsq is not None else 0.0).value                  # (the table carries wscale^2 squared in float, as vsp_demod_f32 squares it)
        t.alpha, t.bias_scale, t.wscale2 = alpha, bs, ctypes.c_float(w32 * w32).value
    return torch.frombuffer(bytearray(bytes(arr)), dtype=torch.uint8).to(DEV)


def _style_setup(K, B):
    lat, layers = R.style_case(K, B)
    layers_dev = [(dev(w), dev(b), dev(q), al, bs, ws) for w, b, q, al, bs, ws in layers]
    sizes = []
    for (cin, cout, demod, _b, _r) in R.STYLE_LAYERS:
        sizes += [B * cin] + ([B * cout] if demod else [])
    buf = torch.full((sum(sizes) + STRIP * (len(sizes) + 1),), SENTINEL, dtype=F32, device=DEV)
    keep = torch.ones(buf.numel(), dtype=torch.bool, device=DEV)         # True on the sentinel strips
    outs, off = [], STRIP
    for (cin, cout, demod, _b, _r) in R.STYLE_LAYERS:
        pair = []
        for n, shape in ((B * cin, (B, cin)), (B * cout, (B, cout))) if demod else ((B * cin, (B, cin)),):
            pair.append(buf[off:off + n].view(shape))
            keep[off:off + n] = False
            off += n + STRIP
        outs.append((pair[0], pair[1] if demod else None))
    return lat, layers, layers_dev, buf, keep, outs


@pytest.mark.parametrize("B", R.STYLE_B)     # 1, 8: style_mods_kernel<8> (one row; all eight); 9, 16: style_mods_kernel<16> (first use; full)
@pytest.mark.parametrize("K", R.STYLE_K)     # 512: two pieces per lane; 1536: six (the decoder's concatenated style)
def test_style_plan_mixed_table(H, K, B):
    """vsp_style_plan_f32 on a table of four layers that differ in everything a layer can differ in (linloss_ref.STYLE_LAYERS), each
    reading another row of a (B, 18, K) latent: every mod and demod within the bound of float64, mod bit-identical to H.linear
    (gemv_rows_kernel) on the same row view, demod bit-identical to H.demod_coefs (demod_kernel) of it, sentinel strips intact"""
    lib, last_error = _lib()
    lat, layers, layers_dev, buf, keep, outs = _style_setup(K, B)
    latd = dev(lat)
    table = _style_table(layers_dev, outs, B, K)
    rc = lib.vsp_style_plan_f32(table.data_ptr(), len(outs), latd.data_ptr(), B, latd.stride(0), K, 512, 512, 1e-8, H._stream())
    assert rc == 0, last_error()
    torch.cuda.synchronize()
    assert bool((buf[keep] == SENTINEL).all()), "style_plan wrote between / behind its outputs"
    for layer, ld, (mod, demod), (cin, cout, has_demod, _b, row) in zip(layers, layers_dev, outs, R.STYLE_LAYERS):
        w, bias, wsq, alpha, bs, ws = ld
        m64, m32 = R.style_mod(lat, layer, row, F64), R.style_mod(lat, layer, row, F32)
        bound(mod, m64, m32, f"style mod K={K} B={B} cin={cin}")
        assert torch.equal(mod, H.linear(latd[:, row], w, bias, alpha=alpha, bias_scale=bs)), f"mod cin={cin} differs from the per-layer launch"
        if has_demod:
            bound(demod, R.demod_coefs(m64, layer[2], ws, 1e-8, F64), R.demod_coefs(m32, layer[2], ws, 1e-8, F32), f"style demod K={K} B={B} {cin}->{cout}")
            assert torch.equal(demod, H.demod_coefs(mod.contiguous(), wsq, ws)), f"demod {cin}->{cout} differs from the per-layer launch"


def test_style_plan_refusals(H):
    lib, last_error = _lib()
    K, B = 512, 2
    lat, _layers, layers_dev, buf, keep, outs = _style_setup(K, B)
    latd = torch.zeros(B * R.STYLE_ROWS * 768 + 4, device=DEV)
    table = _style_table(layers_dev, outs, B, K)
    p, bs = latd.data_ptr(), R.STYLE_ROWS * K
    calls = {"B = 0": (len(outs), p, 0, bs, K), "B = 17": (len(outs), p, 17, bs, K), "K = 767": (len(outs), p, B, R.STYLE_ROWS * 768, 767),
             "K = 256": (len(outs), p, B, bs, 256), "pitch % 4": (len(outs), p, B, bs + 2, K), "src misaligned": (len(outs), p + 4, B, bs, K),
             "L = 0": (0, p, B, bs, K)}
    for what, (L, src, b_, stride, k_) in calls.items():
        assert lib.vsp_style_plan_f32(table.data_ptr(), L, src, b_, stride, k_, 512, 512, 1e-8, H._stream()) == EINVAL, what
        assert "style_plan" in last_error(), what
    torch.cuda.synchronize()
    assert bool((buf == SENTINEL).all())


# ================================================================================================== max-pool
def _pool(H, x, dy, k, s, p, x_off=0, g_off=0):
    """vsp_maxpool2d_f32 / _bwd_f32 on guarded buffers: x and dx start x_off floats into theirs, y and dy g_off floats: (y, dx)"""
    lib, last_error = _lib()
    B, Cc, Hh, Ww = x.shape
    OH, OW = (Hh + 2 * p - k) // s + 1, (Ww + 2 * p - k) // s + 1
    assert tuple(dy.shape) == (B, Cc, OH, OW)
    n_in, n_out = x.numel(), dy.numel()
    xbuf, xd = _guarded(n_in, x_off)
    xd.copy_(x.reshape(-1))
    gbuf, gd = _guarded(n_out, g_off)
    gd.copy_(dy.reshape(-1))
    ybuf, y = _guarded(n_out, g_off)
    dbuf, dx = _guarded(n_in, x_off)
    assert xd.data_ptr() % 16 == 4 * (x_off % 4) and gd.data_ptr() % 16 == 4 * (g_off % 4)
    rc = lib.vsp_maxpool2d_f32(y.data_ptr(), xd.data_ptr(), B * Cc, Hh, Ww, OH, OW, k, s, p, H._stream())
    assert rc == 0, last_error()
    rc = lib.vsp_maxpool2d_bwd_f32(dx.data_ptr(), gd.data_ptr(), xd.data_ptr(), B * Cc, Hh, Ww, OH, OW, k, s, p, H._stream())
    assert rc == 0, last_error()
    what = f"maxpool {tuple(x.shape)} k{k} s{s} p{p}"
    _guard_intact(ybuf, n_out, what, g_off)
    _guard_intact(dbuf, n_in, what, x_off)
    return y.view(B, Cc, OH, OW).cpu(), dx.view(x.shape).cpu()


def _same_with_nan(a, b):
    return a.shape == b.shape and torch.equal(torch.isnan(a), torch.isnan(b)) and torch.equal(torch.nan_to_num(a, 12345.0), torch.nan_to_num(b, 12345.0))


def _pool_exact(H, x, dy, k, s, p, what, **off):
    y, dx = _pool(H, x, dy, k, s, p, **off)
    ry, rdx = R.maxpool_argmax(x, k, s, p, F64)[0], R.maxpool_bwd(dy, x, k, s, p, F64)
    assert _same_with_nan(y.double(), ry), f"{what}: {int((torch.nan_to_num(y.double(), 12345.0) != torch.nan_to_num(ry, 12345.0)).sum())} outputs differ"
    assert torch.equal(dx.double(), rdx), f"{what}: the gradient differs at {int((dx.double() != rdx).sum())} elements"
    print(f"STREAM {what}: exact ({y.numel()} outputs, {dx.numel()} gradient elements)")
    return y, dx


@pytest.mark.parametrize("hw", R.POOL_MAPS)            # 7x9 and 13x10: odd and even, neither a multiple of a stride on both axes
@pytest.mark.parametrize("k,s,p", R.POOL_GEOMETRIES)   # maxpool_fwd_kernel / maxpool_bwd_kernel: k < s (pixels in no window: empty gather range); s = 1
#                                                        (3 x 3 windows per pixel); k 4 p 2 (negative window origin, clipped at both ends); k = 1;
#                                                        k = s = 3 (ragged rim outside every window); k 2 s 1 (2 x 2 windows per pixel)
def test_maxpool_geometries(H, k, s, p, hw):
    x, dy = R.pool_case((2, 3, *hw), k, s, p)
    _pool_exact(H, x, dy, k, s, p, f"maxpool {hw} k{k} s{s} p{p}")


@pytest.mark.parametrize("which", R.POOL_FALLBACKS)    # odd_h: H & 1 with W % 4 == 0; x_off1: x / dx 4 bytes off 16-byte alignment; dy_off1: y / dy
#                                                        4 bytes off 8-byte alignment -- each refuses maxpool2x2_*_kernel and takes maxpool_*_kernel
def test_maxpool_2x2_fallbacks(H, which):
    """exact against float64, and bit-identical to the vector form (maxpool2x2_fwd_kernel / maxpool2x2_bwd_kernel) on an aligned copy"""
    shape = (2, 3, 9, 8) if which == "odd_h" else (2, 3, 8, 8)
    x, dy = R.pool_case(shape, 2, 2, 0)
    off = {"odd_h": {}, "x_off1": {"x_off": 1}, "dy_off1": {"g_off": 1}}[which]
    y, dx = _pool_exact(H, x, dy, 2, 2, 0, f"maxpool 2x2 fallback {which}", **off)
    xv = x[:, :, :8].contiguous()                                          # (odd H: the ninth row lies in no window)
    yv, dxv = _pool(H, xv, dy, 2, 2, 0)
    assert torch.equal(y, yv) and torch.equal(dx[:, :, :8], dxv) and float(dx[:, :, 8:].abs().sum()) == 0.0


@pytest.mark.parametrize("shape", [R.POOL_BIG_2X2,        # maxpool2x2_*_kernel: 655 360 threads > 524 288, the stride loop runs a second time
                                   R.POOL_BIG_GENERIC])   # maxpool_fwd_kernel (655 360 outputs) and maxpool_bwd_kernel (2 626 560 inputs): likewise
def test_maxpool_second_grid_pass(H, shape):
    x, dy = R.pool_case(shape, 2, 2, 0)
    _pool_exact(H, x, dy, 2, 2, 0, f"maxpool second pass {shape}")


@pytest.mark.parametrize("geometry", [(2, 2, 0), (3, 2, 1)])   # maxpool2x2_*_kernel (argmax4 / max4) and maxpool_*_kernel (window_argmax)
@pytest.mark.parametrize("kind", R.POOL_PLANTS)
def test_maxpool_planted_nan_inf(H, kind, geometry):
    """single NaNs, two and three NaNs in one window (ATen: the LAST NaN takes the gradient -- two_nan_diag sends it to element (1, 0) of
    the window, a first-NaN rule to (0, 1)), +inf twice, a window of -inf only, a finite value behind -inf: NaN positions of the output
    and the FULL gradient equal the restatement's and CPU torch's"""
    x, dy, (k, s, p) = R.pool_planted(kind, geometry)
    y, dx = _pool_exact(H, x, dy, k, s, p, f"maxpool planted {kind} k{k} s{s} p{p}")
    xt = x.clone().requires_grad_(True)
    ty = F.max_pool2d(xt, k, s, p)
    (tg,) = torch.autograd.grad(ty, xt, dy)
    assert _same_with_nan(y, ty.detach()) and torch.equal(dx, tg), f"{kind}: differs from CPU torch"


# ================================================================================================== LPIPS layer
def _lpips_launch(H, f0, f1, w, gout, atomic=False):
    """vsp_lpips_layer_ws_f32 (block sums in a work buffer of exactly B x grid floats, added in a fixed order; `atomic`: vsp_lpips_layer_f32,
    one atomic per block) and vsp_lpips_layer_bwd_f32 on device operands (B, C, HW) with guarded outputs: (d (B,), df1 (B, C, HW))"""
    lib, last_error = _lib()
    B, Cc, HW = f0.shape
    obuf, out = _guarded(B)
    if atomic:
        rc = lib.vsp_lpips_layer_f32(out.data_ptr(), f0.data_ptr(), f1.data_ptr(), w.data_ptr(), B, Cc, HW, H._stream())
    else:
        grid = min(-(-HW // R.lpips_block_pixels(Cc)), R.LPIPS_CAP[("reg" if Cc in R.LPIPS_REG_C else "gen", "fwd")])
        wbuf, work = _guarded(B * grid)
        rc = lib.vsp_lpips_layer_ws_f32(out.data_ptr(), work.data_ptr(), B * grid, f0.data_ptr(), f1.data_ptr(), w.data_ptr(), B, Cc, HW, H._stream())
        _guard_intact(wbuf, B * grid, f"lpips work {Cc} {HW}")
    assert rc == 0, last_error()
    gbuf, df1 = _guarded(f1.numel())
    df1.fill_(float("nan"))                                               # (every element must be written)
    assert lib.vsp_lpips_layer_bwd_f32(df1.data_ptr(), f0.data_ptr(), f1.data_ptr(), w.data_ptr(), gout.data_ptr(), B, Cc, HW, H._stream()) == 0, last_error()
    _guard_intact(obuf, B, f"lpips {Cc} {HW}")
    _guard_intact(gbuf, f1.numel(), f"lpips bwd {Cc} {HW}")
    return out, df1.view(B, Cc, HW)


def _lpips_bwd_bound(got, gout, f0, f1, w, what, hw=None):
    """the gradient per group of pixels (ordinary / tiny norm / all-zero f1: scales 1, 1e5, 1e10)"""
    assert bool(torch.isfinite(got).all()), f"{what}: an element is not finite or was not written"
    g64, g32 = R.lpips_layer_bwd(gout, f0, f1, w, F64, hw=hw), R.lpips_layer_bwd(gout, f0, f1, w, F32, hw=hw)
    for name, m in R.lpips_pixel_groups(f1):
        bound(R.lpips_grouped(got.cpu(), m), R.lpips_grouped(g64, m), R.lpips_grouped(g32, m), f"{what} [{name}]")


def _lpips_small_cases():
    return [(C, hw) for C in R.LPIPS_REG_C for hw in R.lpips_small_hw(C)] + R.LPIPS_GENERIC


@pytest.mark.parametrize("C,HW", _lpips_small_cases())
# lpips_layer_reg_kernel<1>, <2>, <4> (C = 64, 128, 256), forward and backward, at HW = 1 (every lane but one per part clamped to the last
# pixel), one below / on / one above a wave's 64 / LPP pixels (a second wave with one live lane per part) and 4 waves + 3 (a second block);
# C = 192 and 3 at HW = 257: lpips_layer_fwd_kernel / lpips_layer_bwd_kernel, a second block with one pixel
def test_lpips_layer_small(H, C, HW):
    """B = 3; all-zero pixels in either map and in both at once, and one pixel of f1 of norm ~1e-4 (linloss_ref.lpips_plant)"""
    f0, f1, w, gout = R.lpips_case(C, HW)
    d, df1 = _lpips_launch(H, dev(f0), dev(f1), dev(w), dev(gout))
    bound(d, R.lpips_layer(f0, f1, w, F64), R.lpips_layer(f0, f1, w, F32), f"lpips C={C} HW={HW}")
    _lpips_bwd_bound(df1, gout, f0, f1, w, f"lpips bwd C={C} HW={HW}")
    d_atomic, _ = _lpips_launch(H, dev(f0), dev(f1), dev(w), dev(gout), atomic=True)          # at most five atomics per sample here
    bound(d_atomic, R.lpips_layer(f0, f1, w, F64), R.lpips_layer(f0, f1, w, F32), f"lpips atomic form C={C} HW={HW}")
    assert torch.equal(H.lpips_layer(dev(f0).view(3, C, HW, 1), dev(f1).view(3, C, HW, 1), dev(w)), d)       # the wrapper is the work-buffer form


@pytest.mark.parametrize("C,direction", R.LPIPS_SECOND_PASS)
# HW = cap x pixels per block + 70: the pixel loop of lpips_layer_reg_kernel<4, false> (2048 blocks x 64), lpips_layer_fwd_kernel (1024 x 256),
# lpips_layer_bwd_kernel (4096 x 256) and lpips_layer_reg_kernel<4, true> (4096 x 64) runs a second time for the first 70 pixels' threads
def test_lpips_layer_second_pass(H, C, direction):
    """B = 1, inputs drawn on the device.  Forward (vsp_lpips_layer_ws_f32, the form hip_ops.lpips_layer calls): float64 on the device,
    e_ref from the float32 restatement on the CPU, and the same bits from a second launch.  The atomic form vsp_lpips_layer_f32 is NOT
    held to the bound here: its 2048 (1024) serial float additions onto one running sum measured, over inputs, a standard deviation of
    0.7e-6 of the result and 2.4e-6 at worst (profiles/linloss_gputest.log prints the figure of this input) -- the reason the
    work-buffer form exists.  Backward: per pixel, the float64 restatement (HW passed explicitly) on the first 256 pixels, 4096 random
    ones and EVERY pixel of the second pass."""
    HW = R.lpips_second_pass_hw(C, direction)
    g = torch.Generator(device=DEV).manual_seed(C * 10 + len(direction))
    f0, f1 = torch.randn(1, C, HW, device=DEV, generator=g).relu_(), torch.randn(1, C, HW, device=DEV, generator=g).relu_()
    R.lpips_plant_big(f0, f1)
    w, gout = torch.rand(C, generator=R._gen(C, HW)) + 0.05, torch.tensor([1.7])
    d, df1 = _lpips_launch(H, f0, f1, dev(w), dev(gout))
    if direction == "fwd":
        ref64 = R.lpips_layer(f0, f1, dev(w), F64).cpu()
        ref32 = R.lpips_layer(f0.cpu(), f1.cpu(), w, F32)
        bound(d, ref64, ref32, f"lpips second pass C={C} HW={HW}")
        again, _ = _lpips_launch(H, f0, f1, dev(w), dev(gout))
        assert torch.equal(again, d), "the fixed-order sum changed between two launches"
        d_atomic, _ = _lpips_launch(H, f0, f1, dev(w), dev(gout), atomic=True)
        e = abs(float(d_atomic) - float(ref64)) / abs(float(ref64))
        print(f"STREAM lpips second pass C={C} HW={HW} atomic form (figure only): relative error {e:.3e}, work-buffer form "
              f"{abs(float(d) - float(ref64)) / abs(float(ref64)):.3e}")
        assert e < 1e-5                                                     # (a lost block or a wrong divisor is 5e-4 and more)
    else:
        idx, first = R.lpips_subset(HW, C, direction)
        assert first == R.LPIPS_CAP[("reg" if C in R.LPIPS_REG_C else "gen", "bwd")] * R.lpips_block_pixels(C) and HW - first == R.LPIPS_EXTRA
        assert bool(torch.isin(torch.arange(first, HW), idx).all()), "the subset must cover every pixel of the second pass"
        assert bool(torch.isfinite(df1).all()), "an element of the gradient was not written"
        di = idx.to(DEV)
        _lpips_bwd_bound(df1[:, :, di], gout, f0[:, :, di].cpu(), f1[:, :, di].cpu(), w, f"lpips bwd second pass C={C} HW={HW} ({len(idx)} pixels)", hw=HW)


# ================================================================================================== resize adjoint
def _resize_adjoint(H, x, g, ihw, ohw, what):
    lib, last_error = _lib()
    planes = g.shape[0] * g.shape[1]
    gd = dev(g).contiguous()
    n = planes * ihw[0] * ihw[1]
    buf, dx = _guarded(n)
    rc = lib.vsp_resize_bilinear_bwd_f32(dx.data_ptr(), gd.data_ptr(), planes, ihw[0], ihw[1], ohw[0], ohw[1], H._stream())
    assert rc == 0, last_error()
    _guard_intact(buf, n, what)
    dx = dx.view(*g.shape[:2], *ihw)
    e_a, _, _ = bound(dx, R.resize_bilinear_bwd(g, ihw, F64), R.resize_bilinear_bwd(g, ihw, F32), f"{what} adjoint")
    y = H.resize_bilinear(dev(x), ohw)
    y64 = R.resize_bilinear(x, ohw, F64)
    e_f, _, _ = bound(y, y64, R.resize_bilinear(x, ohw, F32), f"{what} forward")
    # <A x, g> = <x, A^T g> from the two device results, summed in float64, within what the two bounds allow (Hoelder)
    tol_f = 4 * e_f + 2e-6 * float(y64.abs().max())
    tol_a = 4 * e_a + 2e-6 * float(R.resize_bilinear_bwd(g, ihw, F64).abs().max())
    lhs = float((y.cpu().double() * g.double()).sum())
    rhs = float((x.double() * dx.cpu().double()).sum())
    tol = tol_f * float(g.double().abs().sum()) + tol_a * float(x.double().abs().sum())
    print(f"STREAM {what} dot identity: <Ax,g>={lhs:.9e} <x,Atg>={rhs:.9e} |d|={abs(lhs - rhs):.3e} tol={tol:.3e}")
    assert abs(lhs - rhs) <= tol


@pytest.mark.parametrize("ihw,ohw", R.RESIZE_ADJ_SIZES)   # resize_bilinear_bwd_kernel: one input pixel (all four taps are it); one output pixel;
#                                                           a one-pixel axis (y1 = y0 with ly > 0); up / down mixed; x 24 (hundreds of atomics per
#                                                           input pixel); the ragged case of the existing fp32 test
def test_resize_bilinear_adjoint(H, ihw, ohw):
    x, g = R.resize_case(ihw, ohw)
    _resize_adjoint(H, x, g, ihw, ohw, f"resize {ihw}->{ohw}")


def test_resize_bilinear_adjoint_second_grid_pass(H):
    ihw, ohw, planes = R.RESIZE_ADJ_BIG                    # 540 000 outputs > 524 288: the stride loop runs a second time
    assert planes[0] * planes[1] * ohw[0] * ohw[1] > R.STREAM_ELEMS
    x, g = R.resize_case(ihw, ohw, planes)
    _resize_adjoint(H, x, g, ihw, ohw, f"resize {ihw}->{ohw} x{planes[0] * planes[1]}")


# ================================================================================================== tuning switches, one child process each
def _child_mbk(path):
    """fresh interpreter with VSP_TUNE=1 VSP_GEMM_MBK=2 | 8 (read once per process): the wide cases on gemm_nt_kernel<true,2> / <true,8>,
    within the bound and bit-identical to the default MBK results the parent left in `path`"""
    from vspbfr_amd import hip_ops as Hc
    want = torch.load(path)
    for name in R.WIDE_CASES:
        kw, got = _wide(Hc, name)
        bound(got, R.gemm_nt(**kw, dtype=F64), R.gemm_nt(**kw, dtype=F32), f"gemm {name} MBK={os.environ['VSP_GEMM_MBK']}")
        assert torch.equal(got.cpu(), want[name]), f"{name}: {int((got.cpu() != want[name]).sum())} elements differ from the MBK 4 result"
        print(f"CHILD {name} identical")


def _child_gemv_off():
    """fresh interpreter with VSP_TUNE=1 VSP_GEMV_OFF=1: the few-row deep-K cases on gemm_nt_kernel<true,1>"""
    from vspbfr_amd import hip_ops as Hc
    for name in R.GEMV_OFF_CASES:
        kw = R.gemm_case(name)
        got = _gemm(Hc, kw, name)
        bound(got, R.gemm_nt(**kw, dtype=F64), R.gemm_nt(**kw, dtype=F32), f"gemm {name} tiled (VSP_GEMV_OFF)")
        print(f"CHECKSUM {name} {float(got.double().sum()):.17g}")


def _run_child(args, **env):
    path = os.pathsep.join([ROOT] + ([os.environ["PYTHONPATH"]] if os.environ.get("PYTHONPATH") else []))
    p = subprocess.run([sys.executable, os.path.abspath(__file__)] + args, env=dict(os.environ, VSP_TUNE="1", PYTHONPATH=path, **env), cwd=ROOT,
                       capture_output=True, text=True, timeout=300)
    print(p.stdout)
    assert p.returncode == 0, p.stdout[-3000:] + p.stderr[-3000:]
    return p.stdout


@pytest.mark.parametrize("mbk", ["2", "8"])            # gemm_nt_kernel<true,2> (32 rows per workgroup) and gemm_nt_kernel<true,8> (128 rows)
def test_gemm_wide_mbk_in_child_process(H, tmp_path, mbk):
    path = str(tmp_path / "wide_default.pt")
    torch.save({name: _wide(H, name)[1].cpu() for name in R.WIDE_CASES}, path)
    out = _run_child(["mbk-child", path], VSP_GEMM_MBK=mbk)
    assert sum(ln.startswith("CHILD") for ln in out.splitlines()) == len(R.WIDE_CASES)


def test_gemm_tiled_few_rows_in_child_process(H):
    """(8, 130, 1024) and (13, 32, 4096) on the tiled kernel, the A/B partner of gemv_rows_kernel; its sums run in another order, so
    checksums that both equal the gemv form's would mean the switch selected nothing"""
    mine = {name: f"{float(_gemm(H, R.gemm_case(name), name).double().sum()):.17g}" for name in R.GEMV_OFF_CASES}
    out = _run_child(["gemv-off-child"], VSP_GEMV_OFF="1")
    sums = {ln.split()[1]: ln.split()[2] for ln in out.splitlines() if ln.startswith("CHECKSUM")}
    assert set(sums) == set(R.GEMV_OFF_CASES)
    assert sum(sums[n] == mine[n] for n in sums) < len(sums), "the child computed the gemv form's bits: VSP_GEMV_OFF was not honoured"


if __name__ == "__main__" and sys.argv[1:2] == ["mbk-child"]:
    _child_mbk(sys.argv[2])
if __name__ == "__main__" and sys.argv[1:] == ["gemv-off-child"]:
    _child_gemv_off()
