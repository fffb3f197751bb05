"""Float64 restatements of the HBM-stream kernels (csrc/pointwise.hip, csrc/augment.hip, the helpers of csrc/rowops.hip) in plain
torch, the inputs that tests/test_stream_ref.py (CPU) and tests/test_stream_kernels_gpu.py (GPU) share, and the one bound both use.

Every function is written from the operation's definition (the header comments of the .hip files and the reference statements they
cite), takes CPU tensors and a `dtype` and evaluates everything in that dtype: float64 is the reference, float32 is `ref32`, whose
distance from float64 is the `e_ref` of `bound`.  `variant` selects a deliberately WRONG statement (the teeth of test_stream_ref.py);
None is the definition.  No device code here."""
import math

import torch

from oracle import ops as O

SQRT2 = math.sqrt(2.0)
STREAM_ELEMS = 256 * 8 * 256          # one pass of a capped grid: kMaxStreamBlocks blocks of 256 threads


# ------------------------------------------------------------------------------------------------------------------ the bound
def bound(got, ref64, ref32, what="", slack=None):
    """The project's rule (tests/test_tacc_kernels.py, _row_close of tests/test_hip_ops.py):
        max |got - ref64| <= 4 e_ref + 2e-6 max |ref64|,   e_ref = max |ref32 - ref64|,
    ref32 = the same restatement run in float32 on the CPU.  Nothing in it comes from a kernel.  `slack`: an optional per-element
    allowance that follows from a number format alone (half a bf16 unit for a bf16 store).  Prints and returns (e_ref, e_hip, ratio);
    AssertionError when the bound is missed or `got` is not finite / of another shape."""
    got = got.detach().cpu().double()
    ref64 = ref64.detach().double()
    assert got.shape == ref64.shape, f"{what}: shape {tuple(got.shape)} != {tuple(ref64.shape)}"
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    if ref64.numel() == 0:
        return 0.0, 0.0, float("nan")
    e_ref = float((ref32.detach().double() - ref64).abs().max())
    err = (got - ref64).abs()
    if slack is not None:
        err = (err - slack).clamp_min(0.0)
    e_hip = float(err.max())
    tol = 4 * e_ref + 2e-6 * float(ref64.abs().max())
    ratio = e_hip / e_ref if e_ref else float("nan")
    print(f"STREAM {what}: e_ref={e_ref:.3e} e_hip={e_hip:.3e} ratio={ratio:.2f} tol={tol:.3e}")
    assert e_hip <= tol, f"{what}: max|d|={e_hip:.3e} tol={tol:.3e} (e_ref {e_ref:.3e})"
    return e_ref, e_hip, ratio


def bf16_half_ulp(ref64):
    """half the spacing of bfloat16 (8 significant bits) at |ref64|, normal range"""
    a = ref64.abs().clamp_min(2.0 ** -126)
    return 0.5 * torch.exp2(torch.floor(torch.log2(a)) - 7)


def _c(t, dtype):
    return None if t is None else t.detach().to(dtype)


# ------------------------------------------------------------------------------------------------------------------ pointwise
def skip(up_src, up_k, dtype, variant=None):
    """upfirdn2d(up_src, up_k (4x4), up=2, pad=(2, 1)) written out (reference op/upfirdn2d.py:346-406): with z the zero-inserted map
    (z[2i, 2j] = src[i, j]) padded by 2 in front, out[oy, ox] = sum_{a, b} z[oy + a - 2, ox + b - 2] * k[3 - a, 3 - b] -- a true
    convolution, so the taps are flipped; only the z positions with even coordinates inside the map contribute.
    variants: "parity" (the odd positions taken for the even ones), "noflip" (k[a, b]), "col_off" (source column + 1)."""
    s, k = _c(up_src, dtype), _c(up_k, dtype)
    B, Cc, h, w = s.shape
    oy = torch.arange(2 * h).view(-1, 1)
    ox = torch.arange(2 * w).view(1, -1)
    out = torch.zeros(B, Cc, 2 * h, 2 * w, dtype=dtype)
    par = 1 if variant == "parity" else 0
    for a in range(4):
        for b in range(4):
            zy, zx = oy + a - 2, ox + b - 2
            ok = (zy % 2 == par) & (zx % 2 == par) & (zy >= 0) & (zy < 2 * h) & (zx >= 0) & (zx < 2 * w)
            sy = torch.div(zy, 2, rounding_mode="floor").clamp(0, h - 1).expand(2 * h, 2 * w)
            sx = torch.div(zx, 2, rounding_mode="floor")
            if variant == "col_off":
                ok = ok & (sx + 1 < w)
                sx = sx + 1
            sx = sx.clamp(0, w - 1).expand(2 * h, 2 * w)
            tap = k[a, b] if variant == "noflip" else k[3 - a, 3 - b]
            out = out + torch.where(ok, s[:, :, sy, sx] * tap, torch.zeros((), dtype=dtype))
    return out


def fused_leaky_relu(v, bias, dtype):
    """FusedLeakyReLU (reference op/fused_act.py:216-233): the bias is added inside the stage, slope 0.2, gain sqrt 2"""
    v = v + _c(bias, dtype).view(1, -1, 1, 1)
    return torch.where(v > 0, v, v * 0.2) * SQRT2


def pointwise(x, w, in_scale=None, ch_bias=None, bias1=None, bias2=None, res=None, up_src=None, up_k=None, dtype=torch.float64,
              variant=None):
    """y[b, o] = act2(act1(sum_c x[b, c] (w[o, c] s[b, c]) + ch_bias[o])) + res[b, o] + upfirdn2d(up_src, up_k, up=2, pad=(2, 1))[b, o]
    (ToRGB, reference models/RestoreNet.py:647-666, and the 3 -> 64 input layer with its two FusedLeakyReLU stages).
    variants: "drop_last" (the last input channel left out), "style0" (every image scaled with the style of image 0), and skip's."""
    x, w = _c(x, dtype), _c(w, dtype)
    B, Cin = x.shape[:2]
    if in_scale is not None:
        s = _c(in_scale, dtype)
        if variant == "style0":
            s = s[:1].expand(B, Cin)
        x = x * s.view(B, Cin, 1, 1)
    if variant == "drop_last":
        x, w = x[:, :-1], w[:, :-1]
    y = torch.einsum("bchw,oc->bohw", x, w)
    if ch_bias is not None:
        y = y + _c(ch_bias, dtype).view(1, -1, 1, 1)
    if bias1 is not None:
        y = fused_leaky_relu(y, bias1, dtype)
    if bias2 is not None:
        y = fused_leaky_relu(y, bias2, dtype)
    if res is not None:
        y = y + _c(res, dtype)
    if up_src is not None:
        if variant in ("parity", "noflip", "col_off"):
            y = y + skip(up_src, up_k, dtype, variant)
        else:
            y = y + O.upfirdn2d(_c(up_src, dtype), _c(up_k, dtype), up=2, pad=(2, 1))
    return y


def pointwise_serial(x, w, in_scale=None, ch_bias=None, dtype=torch.float32):
    """the few-output sum as ONE chain over the channels in their order (acc += x[c] (w[c] s[c])), the order a thread that owns a pixel
    has; einsum's blocked sum has a smaller error over thousands of channels"""
    x, w = _c(x, dtype), _c(w, dtype)
    B, Cin = x.shape[:2]
    s = torch.ones(B, Cin, dtype=dtype) if in_scale is None else _c(in_scale, dtype)
    acc = torch.zeros(B, w.shape[0], *x.shape[2:], dtype=dtype)
    for c in range(Cin):
        acc = acc + x[:, c:c + 1] * (w[:, c].view(1, -1) * s[:, c:c + 1]).view(B, -1, 1, 1)
    return acc if ch_bias is None else acc + _c(ch_bias, dtype).view(1, -1, 1, 1)


# ------------------------------------------------------------------------------------------------------------------ augment
def _sampler_taps(theta, in_hw, out_hw, dtype, variant=None):
    """the four (flat input index (B, OH OW), inside (B, OH OW), weight (B, OH OW)) of every output pixel"""
    th = _c(theta, dtype)
    B = th.shape[0]
    (IH, IW), (OH, OW) = in_hw, out_hw
    ox = torch.arange(OW, dtype=dtype).view(1, 1, OW)
    oy = torch.arange(OH, dtype=dtype).view(1, OH, 1)
    if variant == "align_corners":
        xn, yn = 2 * ox / max(OW - 1, 1) - 1, 2 * oy / max(OH - 1, 1) - 1
    else:
        xn, yn = (2 * ox + 1) / OW - 1, (2 * oy + 1) / OH - 1
    t = th.view(B, 6, 1, 1)
    gx = t[:, 0] * xn + t[:, 1] * yn + t[:, 2]
    gy = t[:, 3] * xn + t[:, 4] * yn + t[:, 5]
    if variant == "align_corners":
        ix, iy = (gx + 1) * (IW - 1) / 2, (gy + 1) * (IH - 1) / 2
    else:
        ix, iy = ((gx + 1) * IW - 1) / 2, ((gy + 1) * IH - 1) / 2
    fx, fy = torch.floor(ix), torch.floor(iy)
    wx1, wy1 = ix - fx, iy - fy
    x0, y0 = fx.long(), fy.long()                                   # (B, OH, OW)
    taps = []
    for dy, dx, wgt in ((0, 0, (1 - wx1) * (1 - wy1)), (0, 1, wx1 * (1 - wy1)), (1, 0, (1 - wx1) * wy1), (1, 1, wx1 * wy1)):
        yy, xx = y0 + dy, x0 + dx
        ok = (yy >= 0) & (yy < IH) & (xx >= 0) & (xx < IW)
        if variant == "clamp_iw":
            ok = ok | ((yy >= 0) & (yy < IH) & (xx == IW))
        idx = yy.clamp(0, IH - 1) * IW + xx.clamp(0, IW - 1)
        taps.append((idx.view(B, OH * OW), ok.view(B, OH * OW), wgt.reshape(B, OH * OW)))
    return taps


def affine_sample(x, theta, out_hw, dtype=torch.float64, variant=None):
    """The header comment of csrc/augment.hip: F.grid_sample(x, F.affine_grid(theta, (B, C, OH, OW), align_corners=False), "bilinear",
    "zeros", align_corners=False):
        xn = (2 ox + 1) / OW - 1, yn = (2 oy + 1) / OH - 1;  gx = t00 xn + t01 yn + t02,  gy = t10 xn + t11 yn + t12
        ix = ((gx + 1) IW - 1) / 2,  iy = ((gy + 1) IH - 1) / 2;  bilinear over the four neighbours, zero outside.
    variants: "align_corners" (xn = 2 ox / (OW - 1) - 1, ix = (gx + 1) (IW - 1) / 2), "clamp_iw" (a tap on column IW reads column
    IW - 1 instead of zero)."""
    x = x.to(dtype)                                 # (x keeps its graph: the adjoint below differentiates through this)
    B, Cc, IH, IW = x.shape
    OH, OW = out_hw
    flat = x.reshape(B, Cc, IH * IW)
    out = torch.zeros(B, Cc, OH * OW, dtype=dtype)
    for idx, ok, wgt in _sampler_taps(theta, (IH, IW), out_hw, dtype, variant):
        val = torch.gather(flat, 2, idx.unsqueeze(1).expand(B, Cc, OH * OW))
        out = out + torch.where(ok.unsqueeze(1), val * wgt.unsqueeze(1), torch.zeros((), dtype=dtype))
    return out.view(B, Cc, OH, OW)


def affine_sample_adjoint_scatter(g, theta, in_hw, dtype=torch.float64, order_seed=0):
    """the same adjoint as an explicit scatter whose additions run in a shuffled order (what atomics do): the float32 form of this is
    an arithmetic the kernel is entitled to"""
    g = _c(g, dtype)
    B, Cc, OH, OW = g.shape
    n = OH * OW
    gx = torch.zeros(B, Cc, in_hw[0] * in_hw[1], dtype=dtype)
    taps = _sampler_taps(theta, in_hw, (OH, OW), dtype)
    idx = torch.cat([t[0] for t in taps], 1)                                             # (B, 4 n)
    val = torch.cat([torch.where(t[1], t[2], torch.zeros((), dtype=dtype)) for t in taps], 1).unsqueeze(1) * g.view(B, Cc, n).repeat(1, 1, 4)
    perm = torch.randperm(4 * n, generator=torch.Generator().manual_seed(order_seed))
    for b in range(B):
        gx[b].index_add_(1, idx[b, perm], val[b][:, perm])
    return gx.view(B, Cc, *in_hw)


def affine_sample_adjoint(g, theta, in_hw, dtype=torch.float64):
    """the adjoint of affine_sample w.r.t. x applied to g (B, C, OH, OW): autograd of the restatement above in `dtype`"""
    g = _c(g, dtype)
    B, Cc, OH, OW = g.shape
    with torch.enable_grad():
        x = torch.zeros(B, Cc, in_hw[0], in_hw[1], dtype=dtype, requires_grad=True)
        (gx,) = torch.autograd.grad(affine_sample(x, theta, (OH, OW), dtype), x, g)
    return gx


def color_affine(x, M, t=None, dtype=torch.float64):
    """y[b, c, p] = sum_k M[b, c, k] x[b, k, p] + t[b, c] (reference apply_color, non_leaking.py:910-918)"""
    y = torch.einsum("bck,bkhw->bchw", _c(M, dtype), x.to(dtype))      # (x keeps its graph: the gradient test differentiates through this)
    return y if t is None else y + _c(t, dtype).view(t.shape[0], 3, 1, 1)


# ------------------------------------------------------------------------------------------------------------------ row helpers
def film(h, gamma, beta, dtype=torch.float64):
    return _c(h, dtype) * (1 + _c(gamma, dtype)) + _c(beta, dtype)


def axpby_idx(x, y, a, b, idx, dtype=torch.float64):
    return _c(a, dtype)[idx] * _c(x, dtype) + _c(b, dtype)[idx] * _c(y, dtype)


def add3(a, b, c=None, dtype=torch.float64):
    y = _c(a, dtype) + _c(b, dtype)
    return y if c is None else y + _c(c, dtype)


def scale_add(x, gate, y=None, dtype=torch.float64):
    out = _c(x, dtype) * _c(gate, dtype).view(x.shape[0], x.shape[1], 1, 1)
    return out if y is None else out + _c(y, dtype)


def avgpool2x2(x, dtype=torch.float64):
    x = _c(x, dtype)
    return (x[..., 0::2, 0::2] + x[..., 0::2, 1::2] + x[..., 1::2, 0::2] + x[..., 1::2, 1::2]) / 4


def _bilinear(x, size, dtype, align):
    """separable linear interpolation: source coordinate dst (I - 1) / (O - 1) (align_corners=True; 0 when O = 1) or
    max((dst + 1/2) I / O - 1/2, 0) (False); lower neighbour floor(src) and the one above it, both clamped at I - 1"""
    x = _c(x, dtype)

    def axis(I, Osz):
        d = torch.arange(Osz, dtype=dtype)
        if align:
            src = d * ((I - 1) / (Osz - 1)) if Osz > 1 else d * 0
        else:
            src = ((d + 0.5) * (I / Osz) - 0.5).clamp_min(0)
        i0 = src.floor().long().clamp(max=I - 1)
        return i0, (i0 + 1).clamp(max=I - 1), src - i0.to(dtype)

    IH, IW = x.shape[-2:]
    y0, y1, ly = axis(IH, size[0])
    x0, x1, lx = axis(IW, size[1])
    rows = x[..., y0, :] * (1 - ly).view(-1, 1) + x[..., y1, :] * ly.view(-1, 1)
    return rows[..., x0] * (1 - lx) + rows[..., x1] * lx


def upsample_add(x, y, dtype=torch.float64, variant=None):
    """F.interpolate(x, y.shape[-2:], mode="bilinear", align_corners=True) + y.  variant "align_false": the other ratio."""
    return _bilinear(x, y.shape[-2:], dtype, align=variant != "align_false") + _c(y, dtype)


def resize_bilinear(x, size, dtype=torch.float64):
    """F.interpolate(x, size, mode="bilinear", align_corners=False) (the resize in front of the e4e encoder, Loss/e4e_embedding.py:91-100)"""
    return _bilinear(x, size, dtype, align=False)


def plane_mean_wave(x, dtype=torch.float32):
    """the mean as one 64-lane wave forms it: lane l sums elements l, l + 64, ... in turn, then a butterfly over the lanes"""
    x = _c(x, dtype)
    hw = x.shape[-1] * x.shape[-2]
    flat = torch.nn.functional.pad(x.reshape(*x.shape[:-2], hw), (0, -hw % 64)).reshape(*x.shape[:-2], -1, 64)
    lanes = torch.zeros(*x.shape[:-2], 64, dtype=dtype)
    for r in range(flat.shape[-2]):
        lanes = lanes + flat[..., r, :]
    o = 32
    while o:
        lanes = lanes + lanes[..., torch.arange(64) ^ o]
        o >>= 1
    return lanes[..., 0] / hw


def plane_mean(x, dtype=torch.float64, variant=None):
    """mean over each (H, W) plane.  variant "wave_padded": divided by 64 ceil(hw / 64), the count a padded wave loop would use."""
    x = _c(x, dtype)
    hw = x.shape[-1] * x.shape[-2]
    n = 64 * ((hw + 63) // 64) if variant == "wave_padded" else hw
    return x.sum((-2, -1)) / n


def subsample(x, s):
    return x[..., ::s, ::s]


def quantize_u8_nhwc(x, lo=-1.0, hi=1.0):
    """torchvision.utils.save_image(normalize=True, value_range=(lo, hi)) in its own float32 steps (torchvision 0.13 utils.py:
    clamp_, sub_(lo), div_(max(hi - lo, 1e-5)); then mul(255).add_(0.5).clamp_(0, 255).to(uint8)), NCHW -> NHWC"""
    lo32, hi32 = torch.tensor(lo, dtype=torch.float32), torch.tensor(hi, dtype=torch.float32)
    rng = torch.maximum(hi32 - lo32, torch.tensor(1e-5, dtype=torch.float32))
    y = (x.float().clamp(float(lo32), float(hi32)) - lo32) / rng
    return (y * 255 + 0.5).clamp(0, 255).to(torch.uint8).permute(0, 2, 3, 1).contiguous()


def e4e_codes(heads, latent_avg=None, dtype=torch.float64):
    """codes[b, t] = heads[t, b] + (t > 0 ? heads[0, b] : 0) + latent_avg[t] (reference psp_encoders.py:188-199, psp.py:159-165)"""
    h = _c(heads, dtype)
    out = h.clone()
    out[1:] = out[1:] + h[0:1]
    out = out.transpose(0, 1)
    return out if latent_avg is None else out + _c(latent_avg, dtype).unsqueeze(0)


def rows_concat(B, T, segments):
    """out[b, t] = [seg0 | seg1 | seg2]; a segment (tensor, width, per_token, flip) is tensor[b, t or T - 1 - t, :width] or, with
    per_token False, tensor[b, :width] for every token"""
    parts = []
    for t, width, per_token, flip in segments:
        if per_token:
            p = t[:, :T, :width]
            parts.append(p.flip(1) if flip else p)
        else:
            parts.append(t[:, None, :width].expand(B, T, width))
    return torch.cat(parts, 2).contiguous()


def demod_coefs(style, wsq, wscale, eps=1e-8, dtype=torch.float64):
    """rsqrt(wscale^2 sum_c style[b, c]^2 wsq[o, c] + eps): the demodulation of a modulated convolution (models/RestoreNet.py:190-224)"""
    return torch.rsqrt((wscale * wscale) * (_c(style, dtype) ** 2) @ _c(wsq, dtype).t() + eps)


# ------------------------------------------------------------------------------------------------------------------ shared inputs
def _gen(*key):
    seed = 0
    for k in key:
        seed = (seed * 1000003 + int(k) + 17) % (2 ** 31 - 1)
    return torch.Generator().manual_seed(seed)


UP_K = torch.tensor([[0.9, 2.1, 3.3, 1.2], [2.4, 8.7, 9.9, 3.6], [3.1, 9.3, 8.1, 2.2], [0.7, 3.4, 2.8, 1.4]])
UP_K = UP_K / UP_K.sum() * 4
"""a 4 x 4 FIR kernel of gain 4 that is neither symmetric nor an outer product: a flip or a transposition changes it"""

OPERAND_SETS = {"none": (), "scale": ("in_scale",), "bias_res": ("ch_bias", "res"), "all": ("in_scale", "ch_bias", "res")}
ACT_SETS = {"none": (), "b1": ("bias1",), "b2": ("bias2",), "both": ("bias1", "bias2")}


def pointwise_case(cin, cout, hh, ww, operands=(), with_skip=False, B=2):
    """float32 operands of one pointwise call, as keyword arguments of `pointwise` (x and w included).  The style scale differs between
    the images by more than a factor of 2 and ch_bias / res are of the size of the sum."""
    g = _gen(cin, cout, hh, ww, len(operands), with_skip)
    kw = {"x": torch.randn(B, cin, hh, ww, generator=g), "w": torch.randn(cout, cin, generator=g) / math.sqrt(cin)}
    for name in operands:
        if name == "in_scale":
            kw[name] = (torch.rand(B, cin, generator=g) + 0.5) * torch.linspace(0.6, 1.7, B).view(B, 1)
        elif name == "res":
            kw[name] = torch.randn(B, cout, hh, ww, generator=g)
        else:
            kw[name] = torch.randn(cout, generator=g)
    if with_skip:
        kw["up_src"] = torch.randn(B, cout, hh // 2, ww // 2, generator=g)
        kw["up_k"] = UP_K.clone()
    return kw


SAMPLER_MAPS = [((2, 3, 9, 7), (11, 13)), ((1, 2, 16, 16), (16, 16))]
SAMPLER_MATS = ["identity", "half_shift", "rot45", "shift3", "shift1e6", "zero"]


def sampler_theta(name, B, IH, IW):
    """(B, 2, 3) float32.  half_shift moves the sampling grid by half an input pixel, +x / -y for even images, -x / +y for odd ones: the
    last (first) column's taps lie half on column IW (-1)."""
    th = torch.zeros(B, 2, 3)
    for b in range(B):
        sg = 1.0 if b % 2 == 0 else -1.0
        if name != "zero":
            th[b, 0, 0] = th[b, 1, 1] = 1.0
        if name == "half_shift":
            th[b, 0, 2], th[b, 1, 2] = sg / IW, -sg / IH
        elif name == "rot45":
            c = 1.3 * math.cos(math.pi / 4 + 0.1 * b)
            s = 1.3 * math.sin(math.pi / 4 + 0.1 * b)
            th[b] = torch.tensor([[c, -s, 0.05], [s, c, -0.03]])
        elif name == "shift3":
            th[b, 0, 2] = 3.0 * sg
        elif name == "shift1e6":
            th[b, 0, 2], th[b, 1, 2] = 1e6 * sg, -1e6
        elif name == "magnify":
            th[b, 0, 0] = th[b, 1, 1] = 0.25
    return th


def sampler_case(shape, out_hw, mat):
    """x (offset from zero, so that a border pixel read for a zero shows), theta and a cotangent g for the adjoint"""
    g = _gen(*shape, *out_hw, SAMPLER_MATS.index(mat) if mat in SAMPLER_MATS else 99)
    B, Cc, IH, IW = shape
    x = torch.randn(*shape, generator=g) + 1.5
    return x, sampler_theta(mat, B, IH, IW), torch.randn(B, Cc, *out_hw, generator=g)


UPSAMPLE_SIZES = [((1, 1), (4, 5)), ((1, 6), (3, 6)), ((5, 1), (5, 4)), ((3, 4), (1, 1)), ((3, 4), (3, 4)), ((5, 7), (9, 16))]
RESIZE_SIZES = [((1, 1), (3, 2)), ((5, 7), (1, 1)), ((2, 9), (7, 3))]


def upsample_case(ihw, ohw, planes=(2, 3)):
    g = _gen(*ihw, *ohw, *planes)
    return torch.randn(*planes, *ihw, generator=g), torch.randn(*planes, *ohw, generator=g)


PLANE_HW = [1, 63, 64, 65, 4097]


def plane_mean_case(hw, planes, offset=0.0):
    """(1, planes, 1, hw) with mean 0.5 (+ offset): a wrong divisor moves the mean by a visible fraction"""
    return torch.randn(1, planes, 1, hw, generator=_gen(hw, planes, int(offset))) + 0.5 + offset


# the cases of tests/test_stream_kernels_gpu.py that test_stream_ref.py bites into (the lists live here so that both files walk the same)
FEW_OUT_COUT = [1, 2, 3, 4]
FEW_OUT_CIN = [1, 7, 8, 12, 24]
FEW_OUT_MAPS = [(4, 4), (5, 9), (34, 36)]
SKIP_MAPS = [(2, 2), (4, 4), (8, 12), (6, 6), (6, 10), (10, 14)]
SKIP_CIN = [8, 12]
SKIP_COUT = [1, 3, 4]
FEW_IN_CIN = [1, 2, 3, 4]
FEW_IN_COUT = [5, 64, 257]
FEW_IN_MAPS = [(5, 9), (33, 35)]
LDS_FLOATS = 64 * 1024 // 4        # neither pointwise kernel raises its dynamic-LDS attribute: 64 KB of weights is what launches
LDS_LIMIT_CASES = [(LDS_FLOATS // 4, 4), (LDS_FLOATS, 1), (4, LDS_FLOATS // 7), (1, LDS_FLOATS // 4)]     # (Cin, Cout)
