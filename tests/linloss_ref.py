"""Float64 restatements of the small GEMM (csrc/gemm_small.hip), the style plan (csrc/style_plan.hip) and the loss operators
(csrc/lossops.hip: max-pool, the LPIPS layer, the adjoint of the bilinear resize) in plain torch, the case lists that
tests/test_linloss_ref.py (CPU) and tests/test_linloss_gpu.py (GPU) share, and the size constants derived from the launch code.

As in tests/stream_ref.py: every function is written from the operation's definition, takes CPU tensors and a `dtype` and evaluates
in that dtype (float64 = the reference, float32 = `ref32`, whose distance from float64 is the `e_ref` of stream_ref.bound); `variant`
selects a deliberately WRONG statement (the teeth of test_linloss_ref.py), None is the definition.  The two `*_order` functions are no
definitions: they evaluate, in float32 on the CPU, the ORDER in which a kernel adds its products.  No device code here."""
import math

import torch

from stream_ref import STREAM_ELEMS, _c, _gen, demod_coefs  # noqa: F401  (re-exported: the GPU module reads them from here)

SQRT2 = math.sqrt(2.0)
F64, F32 = torch.float64, torch.float32


# ------------------------------------------------------------------------------------------------------------------ small GEMM
def epilogue(v, act, slope=0.2, gain=SQRT2):
    """act 0: nothing; 1: leaky relu * gain; 2: sigmoid (the three epilogues of vsp_gemm_f32)"""
    if act == 1:
        return torch.where(v > 0, v, v * slope) * gain
    if act == 2:
        return 1 / (1 + torch.exp(-v))
    assert act == 0
    return v


def gemm_nt(a, b, alpha=1.0, bias=None, bias_scale=1.0, act=0, slope=0.2, gain=SQRT2, bias_zs=0, dtype=F64, variant=None):
    """C[z, m, n] = epi(alpha sum_k A[z, m, k] B[z, n, k] + bias[z bias_zs + n] bias_scale): F.linear / matmul with the fused epilogue.
    a (M, K) or (Z, M, K), b (N, K) or (Z | 1, N, K); bias is a flat buffer.
    variants: "drop_k16" / "drop_k4" (the last K % 16 / K % 4 columns left out: a vector loop without its tail), "drop_wave" (the
    16-wide k-steps 1, 5, 9, ... left out: one of the four waves that split K), "bias_unscaled", "bias_zs0" (every batch entry takes
    the bias of entry 0)."""
    a, b = _c(a, dtype), _c(b, dtype)
    two_d = a.dim() == 2
    if two_d:
        a, b = a.unsqueeze(0), b.unsqueeze(0)
    Z, M, K = a.shape
    N = b.shape[1]
    keep = torch.ones(K, dtype=torch.bool)
    if variant == "drop_k16":
        keep[K - K % 16:] = False
    elif variant == "drop_k4":
        keep[K - K % 4:] = False
    elif variant == "drop_wave":
        keep[(torch.arange(K) // 16) % 4 == 1] = False
    v = torch.matmul(a[..., keep], b[..., keep].transpose(1, 2)) * alpha
    if bias is not None:
        bz = 0 if variant == "bias_zs0" else bias_zs
        rows = torch.stack([_c(bias, dtype)[z * bz:z * bz + N] for z in range(Z)])
        v = v + rows.unsqueeze(1) * (1.0 if variant == "bias_unscaled" else bias_scale)
    v = epilogue(v, act, slope, gain)
    return v[0] if two_d else v


def _fma32(a, b, c):
    """fmaf on float32 tensors: the product of two float32 is exact in float64, one rounding of the sum to float64 and one to float32
    (the double rounding differs from fmaf in rare ties of the last bit only)"""
    return (a.double() * b.double() + c.double()).float()


def gemm_tiled_order(a, b, vec=True):
    """alpha-free sum of gemm_nt_kernel in float32, in the kernel's order: wave w of four takes the 16-wide k-steps w, w + 4, ... of the
    vector loop (K & ~15 columns; none of them with vec False) -- inside a step MFMA j = 0..3 adds the products of columns
    k0 + 4 q + j, q = 0..3, to the accumulator, modelled as a chain over q -- then the 4-wide steps w, w + 4, ... of the tail, columns
    in turn; the four partial sums meet as ((w0 + w1) + w2) + w3.  a (M, K), b (N, K) float32."""
    a, b = a.float(), b.float()
    M, K = a.shape
    N = b.shape[0]
    kdone = (K & ~15) if vec else 0
    part = [torch.zeros(M, N) for _ in range(4)]

    def add(w, k):
        part[w] = _fma32(a[:, k].view(M, 1), b[:, k].view(1, N), part[w])
    for k0 in range(0, kdone, 16):
        for j in range(4):
            for q in range(4):
                add((k0 // 16) % 4, k0 + 4 * q + j)
    for k0 in range(kdone, K, 4):
        for k in range(k0, min(k0 + 4, K)):
            add(((k0 - kdone) // 4) % 4, k)
    return ((part[0] + part[1]) + part[2]) + part[3]


def wave_tree(v):
    """wave_sum_f of gemm_small.hip on (..., 64) float32: xor 1, xor 2 (quad permutes), mirror in rows of 8, mirror in rows of 16, then
    (lane 0 + lane 16) + (lane 32 + lane 48)"""
    lane = torch.arange(64)
    v = v + v[..., lane ^ 1]
    v = v + v[..., lane ^ 2]
    v = v + v[..., (lane & ~7) | (7 - (lane & 7))]
    v = v + v[..., (lane & ~15) | (15 - (lane & 15))]
    return (v[..., 0] + v[..., 16]) + (v[..., 32] + v[..., 48])


def gemv_order(a, b):
    """alpha-free sum of gemv_rows_kernel (and style_mods_kernel) in float32, in the kernel's order: lane l holds columns 256 i + 4 l + c;
    per piece i its chain is fma(x, fma(y, fma(z, fma(w, acc)))) -- K / 64 fmaf per lane -- then the DPP tree.  K a multiple of 256."""
    a, b = a.float(), b.float()
    M, K = a.shape
    N = b.shape[0]
    assert K % 256 == 0
    a4, b4 = a.view(M, 1, K // 256, 64, 4), b.view(1, N, K // 256, 64, 4)
    acc = torch.zeros(M, N, 64)
    for i in range(K // 256):
        for c in (3, 2, 1, 0):
            acc = _fma32(a4[:, :, i, :, c], b4[:, :, i, :, c], acc)
    return wave_tree(acc)


def strided_view(storage_floats, shape, strides, offset, g):
    """a float32 view of the given strides at element `offset` of a fresh flat buffer of normal deviates (what lies between the rows
    is not zero: a kernel that ignores a stride reads it)"""
    return torch.as_strided(torch.randn(storage_floats, generator=g), shape, strides, offset)


def gemm_case(name):
    """operands of one launch as keyword arguments of `gemm_nt` (a, b possibly views of a wider storage: the GPU module copies the
    whole storage and re-views it, so pitches and the base alignment arrive on the device as they are here)"""
    Z, M, N, K, kind, kw = GEMM_CASES[name]
    g = _gen(M, N, K, Z, len(name))
    sc = 1 / math.sqrt(max(K, 1))
    if kind == "plain":                    # contiguous rows of pitch K
        shape_a, shape_b = ((M, K), (N, K)) if Z == 0 else ((Z, M, K), (Z, N, K))
        a, b = torch.randn(*shape_a, generator=g), torch.randn(*shape_b, generator=g) * sc
    elif kind == "cols":                   # the first K columns of rows of pitch K + 3 (a multiple of 4): 16-byte aligned rows, K % 4 != 0
        assert (K + 3) % 4 == 0 and K % 4 != 0
        a, b = torch.randn(M, K + 3, generator=g)[:, :K], (torch.randn(N, K + 3, generator=g) * sc)[:, :K]
    elif kind == "offset1":                # one float into a flat buffer: base pointer 4 bytes off 16-byte alignment, pitch K
        assert K % 4 == 0
        a, b = strided_view(M * K + 1, (M, K), (K, 1), 1, g), torch.randn(N, K, generator=g) * sc
    elif kind == "kmajor":                 # a stored (Z, K, M): a_ks = M, the strided form
        a, b = torch.randn(Z, K, M, generator=g).transpose(1, 2), torch.randn(Z, N, K, generator=g) * sc
    else:
        raise KeyError(kind)
    out = dict(a=a, b=b, **kw)
    if kw.get("bias_scale") is not None or "bias_zs" in kw:
        zs = kw.get("bias_zs", 0)
        out["bias"] = torch.randn(max(Z, 1) * zs + N if zs else N, generator=g)
    return out


# name: (Z (0: two-dimensional operands), M, N, K, storage, keyword arguments).  Epilogues: alpha and bias_scale are never 1 where a bias is
# given, so that an unscaled bias shows.
_EPI1 = dict(alpha=0.7, bias_scale=0.3, act=1)
_EPI2 = dict(alpha=1.3, bias_scale=0.6, act=2)
GEMM_CASES = {
    "vec_tail_17x33x20": (0, 17, 33, 20, "plain", _EPI1),       # <true,1>: one 16-wide step (wave 0), K % 16 = 4: one tail step; partial tiles
    "vec_tail_5x40x76": (0, 5, 40, 76, "plain", _EPI2),         # <true,1>: four vector steps, K % 16 = 12: tail steps on waves 0..2
    "vec_masked_36x40x513": (0, 36, 40, 513, "cols", _EPI1),    # <true,1>: pitch 516, K % 4 = 1: the tail step's lanes kq 1..3 are masked (ok = k < K)
    "vec_idle_8x24x32": (0, 8, 24, 32, "plain", _EPI1),         # <true,1>: waves 2, 3 have no k-step and skip the prefetch
    "vec_idle_20x16x48": (0, 20, 16, 48, "plain", _EPI2),       # <true,1>: wave 3 has none
    "k0_bias_7x19x0": (0, 7, 19, 0, "plain", _EPI1),            # K = 0: no loop trip at all, the result is the epilogue of the bias
    "offset1_12x21x64": (0, 12, 21, 64, "offset1", _EPI1),      # A 4 bytes off alignment: falls from VEC to <false,1>
    "batched_vec_3x18x37x64": (3, 18, 37, 64, "plain", dict(_EPI2, bias_zs=40)),      # <true,1> with blockIdx.z, bias[z * bias_zs + n]
    "batched_strided_3x18x37x22": (3, 18, 37, 22, "kmajor", dict(_EPI2, bias_zs=40)),  # <false,1> with blockIdx.z, a_ks = M, masked last step
    "gemv_9x35x512": (0, 9, 35, 512, "plain", _EPI1),           # gemv_rows_kernel<16, 2>: the first row count past <8>
}
WIDE_CASES = {
    "wide_1024x32x64": (0, 1024, 32, 64, "plain", _EPI2),       # <true,4> at M = 1024 exactly: 16 whole row groups, one column block
    "wide_1040x17x84": (0, 1040, 17, 84, "plain", _EPI1),       # <true,4>: last group 16 of 64 rows, partial column block, K % 16 = 4 tail
    "wide_2x1100x50x128": (2, 1100, 50, 128, "plain", dict(_EPI2, bias_zs=64)),   # <true,4> with Z = 2, last group 12 rows, N = 32 + 18
}
GEMM_CASES.update(WIDE_CASES)
GEMV_OFF_CASES = {
    "tiled_8x130x1024": (0, 8, 130, 1024, "plain", _EPI1),      # with VSP_GEMV_OFF: <true,1>, 16 steps per wave
    "tiled_13x32x4096": (0, 13, 32, 4096, "plain", _EPI1),      # 64 steps per wave
}
GEMM_CASES.update(GEMV_OFF_CASES)


def gemm_is_vec(kw):
    """whether vsp_gemm_f32 takes the vector form for these (2-D or batched) operands: unit k stride, pitches multiples of 4 floats and
    a storage offset that is one (device allocations are aligned far beyond 16 bytes)"""
    a, b = kw["a"], kw["b"]
    return all(t.stride(-1) == 1 and all(s % 4 == 0 for s in t.stride()[:-1]) and t.storage_offset() % 4 == 0 for t in (a, b))


# ------------------------------------------------------------------------------------------------------------------ style plan
STYLE_K = [512, 1536]
STYLE_B = [1, 8, 9, 16]           # style_mods_kernel<8> at 1 and 8 (all rows used), <16> at 9 (first use) and 16 (the benchmark's batch)
STYLE_ROWS = 18
# (cin, cout, demodulates, has a bias, row of the latent).  max_cin = max_cout = 512: the grid of every other layer is mostly idle blocks.
STYLE_LAYERS = [(512, 512, True, True, 3),
                (64, 3, False, True, 17),       # no demodulation: its blocks of the second launch return at once
                (130, 35, True, False, 0),      # cin off the wave width on both sides (two full strides + 2), no bias
                (1, 1, True, True, 9)]          # one column: three of a block's four waves return, one lane of the demod wave works


def style_case(K, B):
    """latent (B, 18, K) and per layer (w (cin, K), bias (cin) or None, wsq (cout, cin) or None, alpha, bias_scale, wscale)"""
    g = _gen(K, B, 77)
    lat = torch.randn(B, STYLE_ROWS, K, generator=g)
    layers = []
    for cin, cout, demod, has_bias, _row in STYLE_LAYERS:
        w = torch.randn(cin, K, generator=g)
        bias = torch.randn(cin, generator=g) + 1.0 if has_bias else None
        wsq = torch.rand(cout, cin, generator=g) * 9 if demod else None
        layers.append((w, bias, wsq, 0.9 / math.sqrt(K), 0.37, 1 / math.sqrt(cin * 9)))
    return lat, layers


def style_mod(lat, layer, row, dtype=F64, variant=None):
    w, bias, _wsq, alpha, bias_scale, _ws = layer
    return gemm_nt(lat[:, row], w, alpha=alpha, bias=bias, bias_scale=bias_scale, dtype=dtype, variant=variant)


# ------------------------------------------------------------------------------------------------------------------ max-pool
def maxpool_argmax(x, k, s, p, dtype=F64, variant=None):
    """(out (B, C, OH, OW), index (B, C, OH, OW) of the chosen element in its (H W) plane) of F.max_pool2d(x, k, s, p), floor mode,
    with ATen's selection rule (max_pool2d_with_indices): scan the window's in-range elements in row-major order, starting from -inf at
    the first of them, and take an element when `val > max || isnan(val)` -- the FIRST of equal maxima, the LAST NaN.
    variants: "last_tie" (`>=`), "first_nan" (a NaN is kept once found), "range_off" (with k < s the window is one row and one column
    longer: it reaches into the pixels that belong to no window)."""
    x = _c(x, dtype)
    B, Cc, H, W = x.shape
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    kk = k + 1 if (variant == "range_off" and k < s) else k
    oy, ox = torch.arange(OH).view(OH, 1), torch.arange(OW).view(1, OW)
    y0, x0 = oy * s - p, ox * s - p
    m = torch.full((B, Cc, OH, OW), -math.inf, dtype=dtype)
    best = (y0.clamp_min(0) * W + x0.clamp_min(0)).expand(B, Cc, OH, OW).clone()
    flat = x.reshape(B, Cc, H * W)
    for dy in range(kk):
        for dx in range(kk):
            yy, xx = y0 + dy, x0 + dx
            ok = ((yy >= 0) & (yy < H) & (xx >= 0) & (xx < W)).expand(OH, OW)
            idx = (yy.clamp(0, H - 1) * W + xx.clamp(0, W - 1)).expand(OH, OW)
            v = flat[:, :, idx.reshape(-1)].view(B, Cc, OH, OW)
            if variant == "last_tie":
                take = (v >= m) | torch.isnan(v)
            elif variant == "first_nan":
                take = (v > m) | (torch.isnan(v) & ~torch.isnan(m))
            else:
                take = (v > m) | torch.isnan(v)
            take = take & ok
            m = torch.where(take, v, m)
            best = torch.where(take, idx.expand(B, Cc, OH, OW), best)
    return m, best


def maxpool_bwd(dy, x, k, s, p, dtype=F64, variant=None):
    """the gradient of the above: every output's cotangent goes to the element its window chose"""
    _, best = maxpool_argmax(x, k, s, p, dtype, variant)
    B, Cc, H, W = x.shape
    dx = torch.zeros(B, Cc, H * W, dtype=dtype)
    dx.scatter_add_(2, best.reshape(B, Cc, -1), _c(dy, dtype).reshape(B, Cc, -1))
    return dx.view(B, Cc, H, W)


POOL_GEOMETRIES = [(2, 3, 0),     # k < s: every third row and column lies in no window (their gradient is 0)
                   (3, 1, 1),     # s = 1: nine windows per interior pixel, padded
                   (4, 2, 2),     # the widest padding the entry admits (2 p <= k): corner windows hold 2 x 2 of 4 x 4
                   (1, 1, 0),     # the identity
                   (3, 3, 0),     # k = s: windows tile, a ragged rim of H % 3 rows stays outside
                   (2, 1, 0)]     # four windows per interior pixel, no padding
POOL_MAPS = [(7, 9), (13, 10)]
POOL_FALLBACKS = ["odd_h", "x_off1", "dy_off1"]    # 2x2/2 shapes that the vector form refuses: 9x8; x / dx and dy one float into a buffer
POOL_BIG_2X2 = (4, 5, 512, 512)    # 20 x 256 x 128 = 655 360 threads of maxpool2x2_*_kernel
POOL_BIG_GENERIC = (2, 5, 513, 512)  # odd H: 10 x 256 x 256 = 655 360 outputs (forward), 2 626 560 inputs (backward) of maxpool_*_kernel
assert 4 * 5 * 256 * 128 > STREAM_ELEMS and 2 * 5 * 256 * 256 > STREAM_ELEMS


def pool_case(shape, k, s, p, seed=0):
    """x quantised to half-integers (many windows hold their maximum more than once) and a cotangent of quarter-integers (the up to
    k^2 cotangents that meet in one pixel add exactly in float32: the gradient can be compared bit for bit)"""
    g = _gen(*shape, k, s, p, seed)
    H, W = shape[-2:]
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    x = (torch.randn(*shape, generator=g) * 2).round() / 2
    dy = (torch.randn(*shape[:2], OH, OW, generator=g) * 4).round() / 4 + 0.25
    return x, dy


NAN, INF = float("nan"), float("inf")
POOL_PLANTS = ["one_nan", "two_nan_diag", "two_nan_row", "three_nan", "plus_inf", "all_minus_inf", "finite_after_minus_inf"]


def pool_planted(kind, geometry):
    """(x, dy, (k, s, p)) on a (1, 2, 8, 8) map: the plant sits in the 2 x 2 block at rows 2..3, columns 4..5 -- one window of 2x2/2;
    at 3x3/2 p1 the block lies inside the window of output (1, 2) (rows 1..3, columns 3..5) and partly in its neighbours'.  Channel 1
    carries the plant mirrored (columns swapped) so that 'first' and 'last' in scan order are not tied to one corner."""
    k, s, p = geometry
    x, dy = pool_case((1, 2, 8, 8), k, s, p, seed=POOL_PLANTS.index(kind) + 1)
    blocks = {"one_nan": [[1.0, NAN], [0.5, 2.0]],
              "two_nan_diag": [[1.0, NAN], [NAN, 2.0]],           # ATen sends the gradient to (1, 0), the LAST NaN
              "two_nan_row": [[NAN, NAN], [3.0, 2.0]],
              "three_nan": [[NAN, 5.0], [NAN, NAN]],
              "plus_inf": [[1.0, INF], [INF, 2.0]],               # equal maxima: the first
              "all_minus_inf": [[-INF, -INF], [-INF, -INF]],
              "finite_after_minus_inf": [[-INF, -INF], [-INF, -7.0]]}
    blk = torch.tensor(blocks[kind])
    if kind in ("all_minus_inf", "finite_after_minus_inf"):       # the 3x3 window around the block as well
        x[:, :, 1:4, 3:6] = -INF
    x[0, 0, 2:4, 4:6] = blk
    x[0, 1, 2:4, 4:6] = blk.flip(1)
    return x, dy, geometry


# ------------------------------------------------------------------------------------------------------------------ LPIPS layer
LPIPS_EPS = 1e-10


def _lpips_terms(f0, f1, dtype, variant):
    a, c = _c(f0, dtype), _c(f1, dtype)
    s0, s1 = (a * a).sum(1, keepdim=True), (c * c).sum(1, keepdim=True)
    if variant == "eps_in_sqrt":
        r0, r1 = 1 / torch.sqrt(s0 + LPIPS_EPS), 1 / torch.sqrt(s1 + LPIPS_EPS)
    else:
        r0, r1 = 1 / (torch.sqrt(s0) + LPIPS_EPS), 1 / (torch.sqrt(s1) + LPIPS_EPS)
    return a, c, torch.sqrt(s1), r0, r1


def lpips_layer(f0, f1, w, dtype=F64, variant=None, hw=None):
    """d[b] = (1 / HW) sum_p sum_c w_c (f0 / (|f0| + eps) - f1 / (|f1| + eps))^2, |.| over the channels of a pixel (my_lpips/
    networks_basic.py:73-83, __init__.py:44-46).  f (B, C, P) or (B, C, H, W); `hw`: the pixel count of the map when f holds a subset.
    variant "eps_in_sqrt": 1 / sqrt(|f|^2 + eps)."""
    f0, f1 = f0.reshape(*f0.shape[:2], -1), f1.reshape(*f1.shape[:2], -1)
    a, c, _n1, r0, r1 = _lpips_terms(f0, f1, dtype, variant)
    e = a * r0 - c * r1
    return (e * e * _c(w, dtype).view(1, -1, 1)).sum((1, 2)) / (hw or f0.shape[2])


def lpips_layer_bwd(gout, f0, f1, w, dtype=F64, variant=None, hw=None):
    """d (sum_b gout[b] d[b]) / d f1, written out: with n = |f1|, r = 1 / (n + eps), e_c = f0_c r0 - f1_c r, g_c = -2 w_c e_c:
        d / d f1_k = (gout / HW) (g_k r - f1_k (r^2 / n) sum_c g_c f1_c),   the second term absent where n = 0
    (the derivative of |f1| at 0 is taken as 0: the pixel's own gradient is g r).  variants: "no_k2" (the second term left out
    everywhere), "eps_in_sqrt"."""
    shape = f1.shape
    f0, f1 = f0.reshape(*f0.shape[:2], -1), f1.reshape(*f1.shape[:2], -1)
    a, c, n1, r0, r1 = _lpips_terms(f0, f1, dtype, variant)
    gc = -2 * _c(w, dtype).view(1, -1, 1) * (a * r0 - c * r1)
    dot = (gc * c).sum(1, keepdim=True)
    k2 = torch.where(n1 > 0, dot * r1 * r1 / n1.clamp_min(torch.finfo(dtype).tiny), torch.zeros((), dtype=dtype))
    if variant == "no_k2":
        k2 = torch.zeros_like(k2)
    go = _c(gout, dtype).view(-1, 1, 1) / (hw or f0.shape[2])
    return (go * (gc * r1 - c * k2)).view(shape)


def lpips_bwd_order(gout, f0, f1, w, hw=None):
    """lpips_layer_bwd_kernel / lpips_layer_reg_kernel<LPP, true> in float32 in the kernels' order: |f|^2 and the dot product as fmaf
    chains over the channels in turn -- one chain of C (generic form) or LPP chains of 64 whose ends meet pairwise, (p0 + p1) + (p2 + p3)
    (register forms) -- where torch adds in blocks; e = fma(-f1, r1, f0 r0); the result go * fma(-f1, k2, (-2 w e) r1).  (B, C, P)."""
    f0, f1 = f0.reshape(*f0.shape[:2], -1).float(), f1.reshape(*f1.shape[:2], -1).float()
    B, Cc, P = f0.shape
    parts = LPIPS_REG_C.get(Cc, 1)
    per = Cc // parts

    def meet(chains):
        while len(chains) > 1:
            chains = [chains[i] + chains[i + 1] for i in range(0, len(chains), 2)]
        return chains[0]

    def chain_sum(x, y):
        out = []
        for q in range(parts):
            acc = torch.zeros(B, P)
            for ch in range(q * per, (q + 1) * per):
                acc = _fma32(x[:, ch], y[:, ch], acc)
            out.append(acc)
        return meet(out)
    eps = torch.tensor(LPIPS_EPS, dtype=F32)
    n1 = torch.sqrt(chain_sum(f1, f1))
    r0, r1 = 1 / (torch.sqrt(chain_sum(f0, f0)) + eps), 1 / (n1 + eps)
    e = _fma32(-f1, r1.unsqueeze(1), f0 * r0.unsqueeze(1))
    gw = (-2 * w.float()).view(1, Cc, 1) * e
    dot = chain_sum(gw, f1)
    k2 = torch.where(n1 > 0, dot * r1 * r1 / n1.clamp_min(1e-38), torch.zeros(()))
    go = gout.float().view(B, 1, 1) / torch.tensor(float(hw or P), dtype=F32)
    return go * _fma32(-f1, k2.unsqueeze(1), gw * r1.unsqueeze(1))


# launch constants of vsp_lpips_layer_f32 / _bwd_f32 (csrc/lossops.hip): grid caps in blocks and pixels per block of 256 threads
LPIPS_REG_C = {64: 1, 128: 2, 256: 4}                      # C -> LPP, the lanes that share a pixel
LPIPS_CAP = {("reg", "fwd"): 2048, ("reg", "bwd"): 4096, ("gen", "fwd"): 1024, ("gen", "bwd"): 4096}


def lpips_wave_pixels(C):
    return 64 // LPIPS_REG_C[C]


def lpips_block_pixels(C):
    return 4 * lpips_wave_pixels(C) if C in LPIPS_REG_C else 256


def lpips_first_pass(C, direction):
    """pixels that the capped grid covers in one trip of the pixel loop"""
    return LPIPS_CAP[("reg" if C in LPIPS_REG_C else "gen", direction)] * lpips_block_pixels(C)


def lpips_small_hw(C):
    pw = lpips_wave_pixels(C)
    return [1, pw - 1, pw, pw + 1, 4 * pw + 3]   # below a wave's pixels (clamped lanes); one short; exact; a second wave with one pixel;
#                                                   a second block with three


LPIPS_GENERIC = [(192, 257), (3, 257)]             # no register form: lpips_layer_fwd_kernel / _bwd_kernel, a second block with one pixel
LPIPS_SECOND_PASS = [(256, "fwd"), (3, "fwd"), (3, "bwd"), (256, "bwd")]
LPIPS_EXTRA = 70


def lpips_second_pass_hw(C, direction):
    return lpips_first_pass(C, direction) + LPIPS_EXTRA


LPIPS_TINY = 1e-5


def lpips_plant(f0, f1):
    """in place, on (B >= 3, C, HW) ReLU features: all-zero pixels in either map and in both at once in samples 0 and 1, and in sample 2
    ONE pixel of f1 scaled to a norm of ~1e-4 (|f|^2 ~ 1e-8: eps = 1e-10 inside the square root would move its unit vector by a percent;
    its gradient is ~1e5 times the others', which is why the gradient is bounded per sample)"""
    HW = f0.shape[2]
    f0[0, :, 0] = 0
    f1[1, :, HW - 1] = 0
    f0[1, :, HW // 2] = 0
    f1[1, :, HW // 2] = 0
    f1[2, :, HW // 3] = (f1[2, :, HW // 3] + 0.1) * LPIPS_TINY
    return f0, f1


def lpips_case(C, HW, B=3):
    g = _gen(C, HW, B)
    f0, f1 = torch.randn(B, C, HW, generator=g).relu(), torch.randn(B, C, HW, generator=g).relu()
    lpips_plant(f0, f1)
    return f0, f1, torch.rand(C, generator=g) + 0.05, torch.randn(B, generator=g) + 2.0


def lpips_pixel_groups(f1):
    """[(name, mask (B, P))] splitting the pixels of a gradient by its SCALE, which is 1 / |f1|: the pixels of ordinary norm, those of
    a norm below 1e-3 (the planted tiny one) and those where f1 is all zero (r = 1 / eps = 1e10: a gradient of ~1e10 that would
    otherwise set the 2e-6 max |ref| term for every other pixel).  Each group is bounded on its own."""
    n = f1.reshape(*f1.shape[:2], -1).double().pow(2).sum(1).sqrt()
    zero, tiny = n == 0, (n > 0) & (n < 1e-3)
    return [(name, m) for name, m in (("ordinary", ~zero & ~tiny), ("tiny", tiny), ("zero-f1", zero)) if bool(m.any())]


def lpips_grouped(t, mask):
    """the (n, C) rows of a (B, C, P) gradient at the pixels of a (B, P) mask"""
    return t.reshape(*t.shape[:2], -1).permute(0, 2, 1)[mask]


LPIPS_BIG_ZEROS = {"f0": (5, -3), "both": (7,), "f1": (11, -5)}     # pixels of a large one-sample map that are all zero, from either end


def lpips_plant_big(f0, f1):
    HW = f0.shape[2]
    for which, px in LPIPS_BIG_ZEROS.items():
        for q in px:
            if which in ("f0", "both"):
                f0[0, :, q % HW] = 0
            if which in ("f1", "both"):
                f1[0, :, q % HW] = 0
    return f0, f1


def lpips_subset(HW, C, direction, seed=0):
    """sorted pixel indices at which a large map's gradient is checked: the first 256, 4096 drawn at random, every pixel past the
    first trip of the capped grid"""
    first = lpips_first_pass(C, direction)
    rnd = torch.randint(0, HW, (4096,), generator=_gen(HW, C, seed))
    idx = torch.unique(torch.cat([torch.arange(min(256, HW)), rnd, torch.arange(min(first, HW), HW)]))
    return idx, first


# ------------------------------------------------------------------------------------------------------------------ resize adjoint
def resize_taps(I, Osz, tap_dtype=F32, variant=None):
    """(lower index, upper index, upper weight) of every output position along one axis of F.interpolate(mode="bilinear",
    align_corners=False).  tap_dtype float32: the kernels' own arithmetic -- s = (float) I / (float) O and
    fmaxf((o + 0.5f) * s - 0.5f, 0) with the product and the subtraction in ONE rounding (the compiler contracts them into an fma in
    resize_bilinear_kernel and resize_bilinear_bwd_kernel alike; evaluated here as the float64 product, exact, rounded once); float64:
    the definition.  variant "align_corners": source coordinate o (I - 1) / (O - 1)."""
    o = torch.arange(Osz, dtype=F64)
    if variant == "align_corners":
        src = o * ((I - 1) / (Osz - 1) if Osz > 1 else 0.0)
        if tap_dtype == F32:
            src = src.float()
    elif tap_dtype == F32:
        s = torch.tensor(I, dtype=F32) / torch.tensor(Osz, dtype=F32)
        src = ((o + 0.5) * s.double() - 0.5).float().clamp_min(0)
    else:
        src = ((o + 0.5) * (I / Osz) - 0.5).clamp_min(0)
    i0 = src.long().clamp(max=I - 1)
    i1 = (i0 + 1).clamp(max=I - 1)
    return i0, i1, src - i0.to(src.dtype)


def _resize_weights(in_hw, out_hw, dtype, tap_dtype, variant):
    """four (flat input index (OH OW), weight (OH OW)) pairs; the weights hy hx, hy lx, ly hx, ly lx are formed in tap_dtype first"""
    (IH, IW), (OH, OW) = in_hw, out_hw
    y0, y1, ly = resize_taps(IH, OH, tap_dtype, variant)
    x0, x1, lx = resize_taps(IW, OW, tap_dtype, variant)
    hy, hx = 1 - ly, 1 - lx
    out = []
    for yy, wy in ((y0, hy), (y1, ly)):
        for xx, wx in ((x0, hx), (x1, lx)):
            out.append(((yy.view(-1, 1) * IW + xx.view(1, -1)).reshape(-1), (wy.view(-1, 1) * wx.view(1, -1)).reshape(-1).to(dtype)))
    return out


def resize_bilinear(x, out_hw, dtype=F64, tap_dtype=F32, variant=None):
    x = _c(x, dtype)
    B, Cc, IH, IW = x.shape
    flat = x.reshape(B, Cc, IH * IW)
    out = torch.zeros(B, Cc, out_hw[0] * out_hw[1], dtype=dtype)
    for idx, wgt in _resize_weights((IH, IW), out_hw, dtype, tap_dtype, variant):
        out = out + flat[:, :, idx] * wgt
    return out.view(B, Cc, *out_hw)


def resize_bilinear_bwd(g, in_hw, dtype=F64, tap_dtype=F32, variant=None):
    """the adjoint as the scatter it is: dx[tap] += weight * g over the four taps of every output pixel (weight * g rounded first, as
    the kernel forms the addend), accumulated in `dtype`"""
    g = _c(g, dtype)
    B, Cc, OH, OW = g.shape
    dx = torch.zeros(B, Cc, in_hw[0] * in_hw[1], dtype=dtype)
    gf = g.reshape(B, Cc, OH * OW)
    for idx, wgt in _resize_weights(in_hw, (OH, OW), dtype, tap_dtype, variant):
        dx.index_add_(2, idx, gf * wgt)
    return dx.view(B, Cc, *in_hw)


RESIZE_ADJ_SIZES = [((1, 1), (3, 2)),      # one input pixel: both taps of both axes are it, the weights add to 1
                    ((5, 7), (1, 1)),      # one output pixel
                    ((1, 6), (4, 6)),      # a one-pixel axis beside an identity axis
                    ((2, 9), (7, 3)),      # up in one axis, down in the other
                    ((4, 4), (96, 96)),    # magnification 24: ~576 outputs x 4 atomics meet in every input pixel
                    ((20, 31), (45, 17))]  # the existing test's ragged case
RESIZE_ADJ_BIG = ((40, 50), (300, 300), (2, 3))      # 6 x 90 000 = 540 000 outputs: the stride loop runs a second time
assert 2 * 3 * 300 * 300 > STREAM_ELEMS


def resize_case(ihw, ohw, planes=(2, 3)):
    g = _gen(*ihw, *ohw, *planes, 5)
    return torch.randn(*planes, *ihw, generator=g), torch.randn(*planes, *ohw, generator=g)
