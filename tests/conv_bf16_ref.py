"""Float64 restatement of the bf16 convolution family (include/vspbfr_hip.h: vsp_conv2d_bf16, _bf16x3, _bf16rv, _bf16dg; csrc/conv_bf16.hip,
conv_bf16_rv.hip, conv_bf16_dg.hip) on top of tests/conv_tile_ref.py: that module's contract (reference, operands, inputs, written, bound,
SENTINEL) with the rounding points the bf16 kernels document, a restatement of the dispatch (`form`: which kernel form a launch gets, with
which workgroup order, or which refusal) and the case table that tests/test_conv_bf16_ref.py proves on the CPU and
tests/test_conv_bf16_forms_gpu.py launches on every form.

Rounding points (`rounding(case, entry)`):
    pixel    the general and the row-vector kernels: bf16(fmaf(x, in_scale, in_shift)) times bf16(w)
    weight   per-image weights (w_bstride: vsp_modulate_weight_bf16) and the dilation-group kernel: x (already bf16) times bf16(w * style[b])
    split    bf16x3: a_hi b_hi + a_hi b_lo + a_lo b_hi with hi = bf16(v), lo = bf16(v - hi)
Products are exact, the accumulation and the epilogue chain are fp32 (float64 / float32 here); a bf16 output is rounded once at the store
(the GPU test allows 2^-8 |float64| per element for it) and a bf16 residual once at the load (the residuals drawn here are bf16 values, so
both I/O forms read the same numbers).

Operands are drawn so that the staged value is exact in fp32 before its one bf16 rounding: x on the grid 1/64 with |x| < 4 (8 significant
bits: a bf16 value), scales on 1/16 in [0.5, 1.5] and shifts on 1/8 with |shift| < 4 (5 significant bits) -- x * scale + shift lies on the
grid 1/1024 below 2^4, 14 bits, so the kernel's fmaf, the float64 expression and the float32 expression are the same number.

A case is a SHAPE (conv_tile_ref.Shape) under an operand CHAIN and an I/O form:
    chains   plain | stylefp (style with scales of full precision, on a few shapes: x * scale is formed exactly in float64 -- 8 x 24 bits --
             and rounded to fp32 and then to bf16 as the kernel's fmaf and conversion do; there is no shift in it, so the restatement
             needs no allowance of a bf16 ulp of the staged operand, which a full-precision shift would call for) | style (per-sample in_scale, out_scale, act1 + bias1, noise, act2 = 1 + bias2, two residuals with res_coff 2) |
             demod (per-sample in_scale, out_scale, ch_scale, ch_bias and nothing else: the SMART branch launch, which the dilation-group
             kernel serves in its lean form; on the dilation-group, row-vector and shared-input group shapes and a few others) |
             bn (per-channel in_scale + in_shift, ch_scale, ch_bias, PReLU) | placed (y_coff 3 of Cout + 5 channels, a y plane one row and
             two columns larger than the output, noise, one residual with res_coff 1, and x a window of Cin channels from channel 3 of
             Cin + 5)
    io       f32 | bf (bf16 x, y, residuals) | bfoff (the same with x one element past its 4-byte boundary) | modw (bf: per-image weights
             carry the style; style chain only)"""
from collections import namedtuple
from dataclasses import dataclass, replace
from functools import lru_cache

import torch

import conv_tile_ref as T

F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
SENTINEL = T.SENTINEL
OK, EINVAL, ENOTSUP = 0, -1, -3
CHAINS = ("plain", "style", "bn", "placed")
DEMOD_GROUPS = ("dg", "rv", "dgroups")      # the shapes that also run the chain `demod`


@dataclass(frozen=True)
class Case:
    shape: T.Shape
    chain: str
    io: str = "f32"

    @property
    def name(self):
        return f"{self.shape.name}/{self.chain}" + ("" if self.io == "f32" else f"/{self.io}")

    @property
    def base(self):
        """the case its operands and references belong to: the I/O forms of a (shape, chain) share them"""
        return replace(self, io="f32")

    @property
    def x_coff(self):
        return 3 if self.chain == "placed" and self.shape.x_gs == 0 else 0

    @property
    def x_ch(self):
        return self.shape.x_ch or (self.shape.Cin + 5 if self.x_coff else 0)

    def __getattr__(self, k):
        return getattr(object.__getattribute__(self, "shape"), k)


def bf16(t):
    """round to nearest even to 8 significant bits, in the dtype of t"""
    return t.to(F32).to(BF).to(t.dtype)


def x_elem_offset(case):
    """elements between a 16-byte boundary and the first element of x the launch reads"""
    return case.x_coff * case.H * case.W + (1 if case.io == "bfoff" else 0)


def x_align(case):
    """bytes of x's address modulo 16"""
    return (x_elem_offset(case) * (4 if case.io == "f32" else 2)) % 16


# ------------------------------------------------------------------------------------------------------------ operands
@lru_cache(maxsize=None)
def inputs(base):
    """conv_tile_ref.inputs on the grids of the module docstring; residuals rounded to bf16"""
    assert base.io == "f32"
    d = dict(T.inputs(base))
    d["x"] = (d["x"] * 64).round().clamp(-255, 255) / 64
    if "in_scale" in d and base.chain != "stylefp":
        d["in_scale"] = (d["in_scale"] * 16).round() / 16
    if "in_shift" in d:
        d["in_shift"] = (d["in_shift"] * 8).round().clamp(-31, 31) / 8
    for k in ("res1", "res2"):
        if k in d:
            d[k] = bf16(d[k])
    return d


def rounding(case, entry):
    if entry == "x3":
        return "split"
    if entry == "dg" or case.io == "modw":
        return "weight"
    return "pixel"


def _window(case, d, ignore=False):
    """the operands as the launch sees them: x and in_scale from channel x_coff on (ignore: from channel 0, the mistake)"""
    if not case.x_coff:
        return d
    c = 0 if ignore else case.x_coff
    d = dict(d)
    d["x"] = d["x"][:, c:c + case.Cin]
    if "in_scale" in d:
        d["in_scale"] = d["in_scale"][..., c:c + case.Cin]
    return d


def _staged(d, dtype):
    """x * in_scale + in_shift, exact (module docstring) -> the value whose one rounding the kernels take"""
    x = d["x"].to(dtype)
    if "in_scale" in d:
        sc = d["in_scale"].to(dtype)
        x = x * (sc[:, :, None, None] if sc.dim() == 2 else sc[None, :, None, None])
    if "in_shift" in d:
        sh = d["in_shift"].to(dtype)
        pad = x.shape[1] - sh.shape[0]
        x = x + torch.cat([sh, sh.new_zeros(pad)])[None, :, None, None]
    return x


def _hi_lo(v):
    hi = bf16(v)
    return hi, bf16(v.to(F32) - hi.to(F32)).to(v.dtype)     # (v - hi is exact in fp32: Sterbenz / 16 significant bits)


def _parity_swapped(x, pad):
    """the image whose pixel (u, v), counted from the padded origin, is pixel (u - u % 2 + v % 2, v - v % 2 + u % 2) of x: what a stride-2
    patch holds when plane (row parity, column parity) is filed as plane (column parity, row parity)"""
    H, W = x.shape[-2:]
    xp = torch.nn.functional.pad(x, (pad, pad + 2, pad, pad + 2))
    u, v = torch.meshgrid(torch.arange(H) + pad, torch.arange(W) + pad, indexing="ij")
    return xp[..., (u - u % 2 + v % 2), (v - v % 2 + u % 2)]


def _plain_acc(case, x, wp, dtype, wrong):
    return T._accumulate(case, {"x": x, "wp": wp}, dtype, wrong)


def accumulate(case, d, how, dtype, wrong=None):
    """acc [B, Cout, OH, OW] of the contract with the operands rounded where `how` says.  wrong: a mistake of ACC_WRONG."""
    d = _window(case, d, wrong == "x_coff_ignored")
    tw = wrong if wrong in ("group_dil0", "group_slice0", "t_phase_swap", "taps_transposed") else None
    wp = d["wp"]
    if wrong == "group_w0":
        wp = wp[:1].expand_as(wp)
    if wrong == "style_in_weight" and how == "pixel":
        how = "weight"
    elif wrong == "style_in_pixel" and how == "weight":
        how = "pixel"
    def xf(x):      # the two mistakes of the patch staging, whatever the staged value is
        if wrong == "parity_swap":      # stride 2: the row-parity and column-parity planes of the staged patch exchanged
            return _parity_swapped(x, case.pad_y[0])
        if wrong == "s0_ignored" and x.shape[-1] % 2 == 0:       # every staged pixel is its pair's other pixel
            return x.view(*x.shape[:3], -1, 2).flip(-1).reshape(x.shape)
        return x

    if how == "weight":
        # bf16(w * style[b][ci]): an fp32 product rounded once (csrc/weight_pack.hip); x is copied
        assert "in_shift" not in d
        if "in_scale" not in d:
            return _plain_acc(case, xf(d["x"]), bf16(wp), dtype, tw)
        sc = d["in_scale"]
        if sc.dim() == 1:
            sc = sc[None].expand(case.B, -1)
        one = replace(case, shape=replace(case.shape, B=1))
        out = []
        for b in range(case.B):
            s = torch.cat([sc[b, g * case.x_gs:g * case.x_gs + case.Cin] for g in range(case.G)] if case.x_gs else [sc[b, :case.Cin]] * case.G)
            wb = bf16(wp.to(F32) * s.view(case.G, 1, case.Cin, 1).to(F32))
            out.append(_plain_acc(one, xf(d["x"][b:b + 1]), wb, dtype, tw))
        return torch.cat(out)
    st = _staged(d, F64)
    if how == "pixel":
        parts = [(bf16(st), bf16(wp))]
    else:
        assert how == "split"
        (xh, xl), (wh, wl) = _hi_lo(st), _hi_lo(wp)
        parts = [(xh, wl), (xl, wh), (xh, wh)]      # small terms first, as the kernel adds them
    acc = sum(_plain_acc(case, xf(x), w, dtype, tw) for x, w in parts)
    if wrong == "shift_on_pad" and "in_shift" in d:            # a staged pixel outside the image holds the shift instead of zero
        z = {"x": torch.zeros_like(d["x"]), "wp": bf16(wp), "in_shift": bf16(d["in_shift"])}
        acc = acc + T._accumulate(case, z, dtype, "shift_on_pad") - T._accumulate(case, z, dtype, None)
    return acc


# mistakes of the epilogue and the placement that conv_tile_ref.reference knows, mistakes of the accumulation (above), and two of this module
EPI_WRONG = ("res_coff_ignored", "prelu_ch0", "bias2_dropped", "bias2_after_act", "res_before_act2", "bias_before_scale", "noise_before_act1",
             "last_col_dropped")
ACC_WRONG = ("shift_on_pad", "group_dil0", "group_slice0", "group_w0", "t_phase_swap", "taps_transposed", "parity_swap", "s0_ignored",
             "x_coff_ignored", "style_in_pixel", "style_in_weight")
OWN_WRONG = ("noise_by_channel", "residue_tile_swap", "odd_col_dropped")
WRONG_VARIANTS = ACC_WRONG + EPI_WRONG + OWN_WRONG
# below the bf16 store term (2^-8 |y|): required where the output is fp32 only
FP32_ONLY = ("style_in_pixel", "style_in_weight")


def reference(case, how, dtype, wrong=None):
    """-> y [B, y_ch, y_h, y_w]: the contract's value under the rounding points `how`, SENTINEL where the launch must not write"""
    base = case.base
    d = inputs(base)
    acc = accumulate(base, d, how, dtype, wrong if wrong in ACC_WRONG else None)
    g = T.geom(base)
    if wrong == "residue_tile_swap" and not base.transposed:
        # output row t * d + r (tile row t of residue r) taken for row r * ceil(H / d) + t
        for grp in range(min(base.G, 4)):
            dl = base.dil[grp]
            if dl > 1 and base.sy == 1:
                sh = -(-base.H // dl)
                oy = torch.arange(g.OH)
                src = (oy % dl) * sh + oy // dl
                src = torch.where(src < g.OH, src, oy)
                sl = slice(grp * base.cout_g, (grp + 1) * base.cout_g)
                acc[:, sl] = acc[:, sl][:, :, src]
    dd = _window(base, d)
    if wrong == "noise_by_channel" and "noise" in dd:
        dd = dict(dd)
        nz = dd["noise"]
        dd["noise"] = nz.roll(1, dims=1)            # (a plane stride of the channel's: another row of the same plane stands in)
    y = T.reference(base, dd, dtype, wrong if wrong in EPI_WRONG else None, acc=acc)
    if wrong == "odd_col_dropped" and g.OW % 2 == 1 and not base.transposed:
        y[:, g.y_coff:g.y_coff + g.Cout, :g.OH, g.OW - 1] = SENTINEL
    return y


@lru_cache(maxsize=None)
def references(base, how):
    """(ref64, ref32, bound, e_ref): computed once per (shape, chain, rounding points), shared by the I/O forms, variants and entries"""
    r64, r32 = reference(base, how, F64), reference(base, how, F32)
    b, e = T.bound(r64, r32)
    return r64, r32, b, e


def applies(case, how, v):
    """whether mistake v could sit in the case"""
    o, g = T.operands(case), T.geom(case)
    tr, ng = case.transposed, (1 if case.G > 4 else case.G)
    return {
        "shift_on_pad": bool(o["in_shift"]) and how != "weight" and (tr or case.pad_y[0] > 0),
        "group_dil0": not tr and len(set(case.dil[:ng])) > 1,
        "group_slice0": case.x_gs > 0,
        "group_w0": case.G > 1,
        "t_phase_swap": tr,
        "taps_transposed": True,
        "s0_ignored": case.W % 2 == 0,
        "x_coff_ignored": case.x_coff > 0,
        "style_in_pixel": how == "weight" and o["in_scale"] is not None,
        "style_in_weight": how == "pixel" and o["in_scale"] is not None and not o["in_shift"],
        "res_coff_ignored": o["res"] > 0 and o["res_coff"] > 0,
        "prelu_ch0": o["act2"] == 2,
        "bias2_dropped": o["act2"] == 1,
        "bias2_after_act": o["act2"] == 1,
        "res_before_act2": o["res"] > 0 and o["act2"] != 0,
        "parity_swap": (case.sy, case.sx) == (2, 2),
        "bias_before_scale": o["ch_scale"] and o["ch_bias"],
        "noise_before_act1": o["noise"] and o["act1"],
        "last_col_dropped": tr,
        "noise_by_channel": o["noise"] and g.OH > 1,
        "residue_tile_swap": not tr and case.sy == 1 and any(1 < dl and -(-case.H // dl) > 1 for dl in case.dil[:ng]),
        "odd_col_dropped": not tr and g.OW % 2 == 1,
    }[v]


# ------------------------------------------------------------------------------------------------------------ weight images
def _pad_co(c):
    return (c + 31) // 32 * 32


def bf16_image(wp):
    """include/vspbfr_hip.h, vsp_conv2d_bf16: w[(((((g nchunk + chunk) 9 + tap) 2 + octet) co_pad + co) 8 + j] =
    bf16(W_g[tap][16 chunk + 8 octet + j][co]), zero past Cin / cout_g"""
    G, Tn, cin, cout = wp.shape
    nch, cop = (cin + 15) // 16, _pad_co(cout)
    g, c, t, o, co, j = torch.meshgrid(*[torch.arange(n) for n in (G, nch, Tn, 2, cop, 8)], indexing="ij")
    ci = 16 * c + 8 * o + j
    ok = (ci < cin) & (co < cout)
    v = wp[g, t, ci.clamp(max=cin - 1), co.clamp(max=cout - 1)]
    v = torch.where(ok, v, torch.zeros_like(v))      # (+0 in the padding, whatever the sign of the clamped element)
    return v.to(BF).reshape(-1)


def bf16x3_image(wp):
    """vsp_conv2d_bf16x3: w[((((((g nchunk + chunk) 2 + part) 9 + tap) 2 + octet) co_pad + co) 8 + j], part 0 = bf16(W), 1 = bf16(W - part 0)"""
    G, Tn, cin, cout = wp.shape
    nch, cop = (cin + 15) // 16, _pad_co(cout)
    hi = wp.to(BF)
    parts = torch.stack([hi.float(), (wp - hi.float()).to(BF).float()])
    g, c, p, t, o, co, j = torch.meshgrid(*[torch.arange(n) for n in (G, nch, 2, Tn, 2, cop, 8)], indexing="ij")
    ci = 16 * c + 8 * o + j
    ok = (ci < cin) & (co < cout)
    v = parts[p, g, t, ci.clamp(max=cin - 1), co.clamp(max=cout - 1)]
    v = torch.where(ok, v, torch.zeros_like(v))      # (+0 in the padding, whatever the sign of the clamped element)
    return v.to(BF).reshape(-1)


def bf16rv_image(wp):
    """vsp_conv2d_bf16rv: per group w[(((((chunk 3 + ky) 2 + quad) 2 + half) co_pad + co) 8 + e] =
    bf16(W[3 ky + kx][8 chunk + 4 quad + 2 half + (e >> 2)][co]) with kx = e & 3, zero for kx = 3 and past cout_g"""
    G, Tn, cin, cout = wp.shape
    assert Tn == 9 and cin % 8 == 0
    cop = _pad_co(cout)
    g, c, ky, q, h, co, e = torch.meshgrid(*[torch.arange(n) for n in (G, cin // 8, 3, 2, 2, cop, 8)], indexing="ij")
    kx, ci = e & 3, 8 * c + 4 * q + 2 * h + (e >> 2)
    ok = (kx < 3) & (co < cout)
    v = wp[g, 3 * ky + kx.clamp(max=2), ci, co.clamp(max=cout - 1)]
    v = torch.where(ok, v, torch.zeros_like(v))      # (+0 in the padding, whatever the sign of the clamped element)
    return v.to(BF).reshape(-1)


def modulated_image(wp, style):
    """vsp_modulate_weight_bf16: out[b] = the image of vsp_conv2d_bf16 of bf16(wp * style[b][ci]), the product in fp32"""
    return torch.stack([bf16_image(wp * style[b].view(1, 1, -1, 1)) for b in range(style.shape[0])])


# ------------------------------------------------------------------------------------------------------------ the dispatch, restated
TILES = {   # (mode, variant) -> MB, NB, WM, WN   (bf16_launch)
    ("s1", 1): (1, 2, 1, 4), ("s1", 2): (2, 2, 1, 4), ("s1", 3): (2, 2, 2, 2), ("s1", 4): (2, 1, 1, 4), ("s1", 6): (2, 1, 2, 2), ("s1", 7): (1, 1, 1, 4),
    ("s2", 3): (2, 2, 2, 2), ("s2", 4): (2, 1, 1, 4), ("s2", 6): (2, 1, 2, 2),
    ("tc", 4): (2, 1, 1, 4), ("tc", 5): (1, 1, 1, 4), ("tc", 8): (1, 2, 1, 4),
}
SPLIT_TILES = {   # bf16_launch_split
    ("s1", 1): (1, 2, 1, 4), ("s1", 4): (2, 1, 1, 4), ("s1", 7): (1, 1, 1, 4), ("s2", 7): (1, 1, 1, 4), ("s2", 6): (1, 1, 2, 2), ("tc", 5): (1, 1, 1, 4),
}
VARIANTS = {"bf16": {"s1": (0, 1, 2, 3, 4, 6, 7), "s2": (0, 3, 4, 6), "tc": (0, 4, 5, 8)},
            "x3": {"s1": (0, 1, 4, 7), "s2": (0, 6, 7), "tc": (0, 5)},
            "rv": {"s1": (0, 1, 2, 3)}, "dg": {"s1": (0,)}}
MAX_LDS = 150 * 1024
Form = namedtuple("Form", "code why name order facts")


def mode_of(case):
    return "tc" if case.transposed else ("s2" if (case.sy, case.sx) == (2, 2) else "s1")


def bf_pitch(twl, pc):
    if twl == 5:
        return pc
    if twl == 4:
        return (pc + 15) & ~15
    p = (pc & ~15) + 8
    return p if p >= pc else p + 16


BfGeom = namedtuple("BfGeom", "twl TW TH PR PC pitch plane pt pt2 lds")


def bf_geom(case, mode, co_t, npix, erows, npart):
    g = T.geom(case)
    sw = case.W + 1 if mode == "tc" else (g.OW if mode == "s2" else case.W)
    dmax = max([1] + list(case.dil[:1 if case.G > 4 else case.G])) if mode == "s1" else 1
    twl = 5 if sw >= 32 else (4 if sw > 8 else 3)
    TW, TH = 1 << twl, npix >> twl
    PR, PC = (TH + 2, TW + 2 * dmax) if mode == "s1" else (TH + 1, TW + 1)
    pitch = bf_pitch(twl, PC)
    plane = PR * pitch
    ntask, npl = plane, 1
    if mode == "s2":
        plane = (plane & ~15) + 8 if (plane & ~15) + 8 >= plane else (plane & ~15) + 24
        ntask, npl = (2 * PR - 1) * 2 * PC, 4
    pt = (ntask + 127) // 128
    pt2 = (((2 * PR - 1) * PC if mode == "s2" else PR * ((PC + 2) // 2)) + 127) // 128
    lds = (2 * 9 * 2 * co_t + 2 * 2 * npl * plane) * 16 * npart
    lds = max(lds, erows * npix * 4) + co_t * 16
    return BfGeom(twl, TW, TH, PR, PC, pitch, plane, pt, pt2, lds)


def _dils(case):
    return [case.dil[i] if i < len(case.dil) else case.dil[0] for i in range(1 if case.G > 4 else case.G)]


def _entry_rules(case, entry):
    """conv2d_bf16_impl and validate_conv (csrc/conv_igemm.hip), in their order, for what the case table can hold -> (code, message part)"""
    o, g, mode = T.operands(case), T.geom(case), mode_of(case)
    io_bf = case.io != "f32"
    if mode == "tc":
        if case.G != 1:
            return EINVAL, "transposed mode needs a 3x3 kernel and G = 1"
    elif mode == "s2":
        if case.dil[0] != 1 or case.pad_y[0] != case.pad_x[0] or case.pad_y[0] not in (0, 1):
            return EINVAL, "stride 2 needs dilation 1 and padding 0 or 1"
        if case.G != 1 and case.x_gs == 0:
            return EINVAL, "stride-2 groups need their own input slices"
    else:
        if (case.sy, case.sx) != (1, 1):
            return EINVAL, "stride must be 1 or 2"
        if case.G > 4 and case.x_gs == 0:
            return EINVAL, "more than four groups need their own input slices"
        for i, dl in enumerate(_dils(case)):
            if not (1 <= dl <= 64 and case.pad_y[i] == dl and case.pad_x[i] == dl):
                return EINVAL, "needs a dilation of 1 to 64 and padding = dilation"
    if case.Cin % 8:
        return EINVAL, "Cin must be a multiple of 8"
    if case.io == "modw":
        if entry != "bf16":
            return EINVAL, "per-image weights need the general bf16 kernel with bf16 activations"
        if case.W % 2 or x_align(case) % 4:
            return EINVAL, "per-image weights need even rows"
    if entry == "x3" and io_bf:
        return EINVAL, "the split-precision form keeps fp32 activations"
    if case.x_gs and o["in_shift"]:
        return EINVAL, "an input shift is not supported with grouped input"
    return OK, ""


def _wg_order(case, mode, co_t, gm, split):
    """launch_bf: the grid and the order the workgroups walk it in -> (order name, grid, facts)"""
    G, B, g = case.G, case.B, T.geom(case)
    co_tiles = -(-case.cout_g // co_t)
    TW, TH = gm.TW, gm.TH
    facts = {}
    if mode == "s1":
        per = [(-(-case.W // TW)) * (-(-(-(-case.H // dl)) // TH)) * dl for dl in _dils(case)]
        blocks = max(per)
        facts["spare"] = any(n < blocks for n in per)      # (a group with fewer blocks than the launch's x extent: its last blocks return at once)
    else:
        EH, EW = (case.H + 1, case.W + 1) if mode == "tc" else (g.OH, g.OW)
        blocks = (-(-EW // TW)) * (-(-EH // TH))
        facts["spare"] = False
    order = "launch"
    if mode == "s1" and 2 <= G <= 4 and case.x_gs == 0 and all(dl in (1, 2, 4, 8) for dl in _dils(case)):
        bands, cgroups = -(-case.H // (8 * TH)), (-(-case.W // TW) + 3) // 4
        blocks = bands * cgroups * 32
        order = "region"
        tiles_x = -(-case.W // TW)
        facts["unfilled"] = tiles_x % 4 != 0 or any((-(-(-(-case.H // dl)) // TH)) % (8 // dl) != 0 for dl in _dils(case))
        facts["spare"] = False                              # (the region order has its own early return: `unfilled`)
    if G == 1:
        order = "xcd"
        wtile = case.Cin * 9 * co_t * 2 * (2 if split else 1)
        wall = wtile * co_tiles
        xall = B * case.Cin * case.H * case.W * (2 if case.io != "f32" else 4)
        if wall > 8 * 1024 * 1024 and co_tiles >= 4 and wall * 2 > xall // 8:
            cgs = min(max((3 * 1024 * 1024 // 2) // wtile, 1), co_tiles)
            order = f"wheavy({cgs},{'tail' if co_tiles % cgs else 'even'})"
    grid = blocks * co_tiles * G * B
    facts["grid8"] = grid % 8 == 0
    return order, grid, facts


def form(case, entry, hint=0):
    """What the library does with the launch: Form(code, message part, form name, workgroup order, facts).  entry: bf16 | x3 | rv | dg."""
    code, why = _entry_rules(case, entry)
    if code:
        return Form(code, why, None, None, {})
    o, g, mode = T.operands(case), T.geom(case), mode_of(case)
    io_bf = case.io != "f32"
    x_al = x_align(case)
    if entry == "dg":
        ok = (mode == "s1" and io_bf and 1 <= case.G <= 4 and case.x_gs == 0 and case.cout_g <= 16 and case.Cin <= 64
              and all(dl in (1, 2, 4, 8) for dl in _dils(case)) and not o["in_shift"] and case.W % 8 == 0 and g.y_w % 2 == 0
              and (g.y_h * g.y_w) % 2 == 0 and x_al == 0)
        if not ok:
            return Form(ENOTSUP, "", None, None, {})
        full = bool(o["act1"] or o["act2"] != 0 or o["noise"] or o["res"] > 0)
        facts = {"ragged_row": any((-(-case.H // dl)) % 8 != 0 for dl in _dils(case)), "ragged_col": case.W % 32 != 0,
                 "ragged_co": case.cout_g != 16, "spare": any(case.H % dl for dl in _dils(case)), "scaled": o["in_scale"] is not None}
        return Form(OK, "", f"dg/nst{1 if case.Cin <= 32 else 2}/{'full' if full else 'lean'}", "items", facts)
    if entry == "rv":
        ok = (mode == "s1" and io_bf and 1 <= case.G <= 4 and (case.G == 1 or case.x_gs == 0)
              and all(dl == 1 or (case.G > 1 and dl in (2, 4, 8)) for dl in _dils(case))
              and case.Cin <= 256 and case.cout_g % (32 if case.G == 1 else 8) == 0 and case.W % 64 == 0 and x_al == 0 and g.y_w % 2 == 0)
        if not ok:
            return Form(ENOTSUP, "", None, None, {})
        if case.G == 1:
            v = hint or (2 if case.cout_g % 64 == 0 else 1)
            if v == 2 and case.cout_g % 64:
                return Form(EINVAL, "64-channel tiles need Cout", None, None, {})
            if v not in (1, 2, 3):
                return Form(EINVAL, "unknown variant", None, None, {})
            th = 16 if v == 3 else 8
            return Form(OK, "", f"rv/v{v}", "walk", {"ragged_row": case.H % th != 0, "spare": False})
        facts = {"ragged_row": any((-(-case.H // dl)) % 8 != 0 for dl in _dils(case)), "spare": any(case.H % dl for dl in _dils(case)),
                 "ragged_co": case.cout_g % 32 != 0}
        return Form(OK, "", "rv/dg/" + "+".join(f"d{dl}" for dl in _dils(case)), "walk", facts)
    split = entry == "x3"
    v = hint
    if split:
        if v == 0:
            v = {"s2": 6, "tc": 5}.get(mode) or (1 if case.G == 1 and case.H * case.W >= 64 * 64 else 7)
        tile = SPLIT_TILES.get((mode, v))
    else:
        if v == 0:
            if mode == "tc":
                v = 5
            elif mode == "s2":
                v = 3 if case.cout_g >= 2048 else (6 if case.cout_g >= 128 and g.OH * g.OW <= 256 else 4)
            else:
                px = (-(-case.H // max(_dils(case)))) * case.W
                if case.cout_g <= 32:
                    v = 1
                elif px <= 64 and case.cout_g >= 128:
                    v = 6
                elif case.G > 1:
                    v = 2 if px >= 512 else 4
                elif case.cout_g <= 64:
                    v = 2 if px >= 128 * 128 else 4
                else:
                    v = 2 if px >= 64 * 64 else 4
        tile = TILES.get((mode, v))
    if tile is None:
        return Form(EINVAL, "unknown", None, None, {})
    MB, NB, WM, WN = tile
    co_t, npix = 32 * MB * WM, 32 * NB * WN
    gm = bf_geom(case, mode, co_t, npix, 32 * WM, 2 if split else 1)
    if gm.lds > MAX_LDS:
        return Form(ENOTSUP, "tile does not fit LDS", None, None, {})
    if split:
        PT = 3 if gm.pt <= 3 else (5 if gm.pt <= 5 else None)
    else:
        PT = 3 if gm.pt <= 3 else (5 if mode != "tc" and gm.pt <= 5 else (7 if mode != "s2" and gm.pt <= 7 else None))
    if PT is None:
        return Form(ENOTSUP, "is too large", None, None, {})
    staging = "f32"
    if io_bf and not split:
        even = case.W % 2 == 0 and x_al % 4 == 0
        plain = o["in_scale"] is None and not o["in_shift"] and even
        modw = case.io == "modw"
        p2 = next((n for n in (1, 2, 3, 5) if gm.pt2 <= n), None)
        if (modw or plain) and p2 is not None:
            staging = f"pair{p2}/nosc"
        elif modw:
            return Form(ENOTSUP, "more than five pair tasks per thread", None, None, {})
        elif even and p2 is not None and (p2 <= 3 or PT >= 5):
            staging = f"pair{p2}"
        else:
            staging = "iob"
    name = ("x3/" if split else "") + f"{mode}/v{v}/pt{PT}" + ("" if split else f"/{staging}")
    order, grid, facts = _wg_order(case, mode, co_t, gm, split)
    dl0 = _dils(case)
    if mode == "s1":
        SW, SHs = case.W, [-(-case.H // dl) for dl in dl0]
        s0 = {dl & 1 for dl in dl0}
    elif mode == "s2":
        SW, SHs, s0 = g.OW, [g.OH], {case.pad_x[0] & 1}
    else:
        SW, SHs, s0 = case.W + 1, [case.H + 1], {1}
    tiles_x = -(-SW // gm.TW)
    facts.update(twl=gm.twl, ragged_row=any(s % gm.TH for s in SHs), ragged_col=SW % gm.TW != 0, ragged_co=case.cout_g % co_t != 0,
                 cin8=case.Cin % 16 == 8, pt2=gm.pt2)
    if staging.startswith("pair"):
        # the first patch column of EVERY column tile is the second pixel of its pair when s0 = 1 (tile origins are even)
        facts.update(s0=max(s0), s0_last_ragged=max(s0) == 1 and SW % gm.TW != 0, s0_last_ragged_odd=max(s0) == 1 and SW % gm.TW != 0 and tiles_x % 2 == 1)
    return Form(OK, "", name, order, facts)


# ------------------------------------------------------------------------------------------------------------ the case table
def _s(name, group, **kw):
    kw.setdefault("B", 2)
    return T.Shape(name, group, **kw)


def _dg(*dl):
    return dict(G=len(dl), dil=dl, pad_y=dl, pad_x=dl)


SHAPES = (
    # stride 1, one group, dilation 1: the three width classes at their edges, heights that no tile divides, cout_g 8 ... 160, Cin 8 ... 64
    _s("w5", "s1", H=7, W=5, Cin=8, cout_g=8, B=3),
    _s("w8", "s1", H=9, W=8, Cin=24, cout_g=12),
    _s("w9", "s1", H=5, W=9, Cin=8, cout_g=20, B=1),
    _s("w13", "s1", H=11, W=13, Cin=40, cout_g=36),
    _s("w24", "s1", H=10, W=24, Cin=24, cout_g=72, B=3),
    _s("w31", "s1", H=9, W=31, Cin=8, cout_g=8),
    _s("w32", "s1", H=17, W=32, Cin=64, cout_g=160, B=1),
    _s("w33", "s1", H=8, W=33, Cin=8, cout_g=12, B=3),
    _s("w45", "s1", H=19, W=45, Cin=24, cout_g=20, B=1),
    _s("w64", "s1", H=16, W=64, Cin=16, cout_g=36),
    _s("w70", "s1", H=21, W=70, Cin=8, cout_g=8, B=1),
    # one group of dilation 8: the widest halo of each class (PT 5 / 7, more than five pair tasks)
    _s("d8w8", "s1d", H=19, W=8, Cin=8, cout_g=8, **_dg(8)),
    _s("d8w24", "s1d", H=19, W=24, Cin=24, cout_g=20, B=3, **_dg(8)),
    _s("d8w45", "s1d", H=21, W=45, Cin=8, cout_g=12, B=1, **_dg(8)),
    _s("d8w64", "s1d", H=17, W=64, Cin=8, cout_g=36, B=1, **_dg(8)),
    # one group of dilation 48 on a small map: the patch planes the narrow tiles reach only through a wide halo (PT 7 on the 128-pixel
    # tiles, PT 5 on the 64-pixel one, a plane too large for the 256-pixel tiles)
    _s("d48w32", "s1d", H=9, W=32, Cin=8, cout_g=12, B=1, **_dg(48)),
    # dilation groups over one input: the four of the path, (2, 8), (8, 1, 2), and (1, 3) which the region order does not take
    _s("g4w8", "dgroups", H=11, W=8, Cin=16, cout_g=16, **_dg(1, 2, 4, 8)),
    _s("g4w24", "dgroups", H=19, W=24, Cin=16, cout_g=16, B=3, **_dg(1, 2, 4, 8)),
    _s("g4w45", "dgroups", H=21, W=45, Cin=8, cout_g=12, B=1, **_dg(1, 2, 4, 8)),
    _s("g4w64", "dgroups", H=34, W=64, Cin=8, cout_g=8, B=1, **_dg(1, 2, 4, 8)),
    _s("g28", "dgroups", H=17, W=31, Cin=8, cout_g=20, **_dg(2, 8)),
    _s("g812", "dgroups", H=13, W=64, Cin=24, cout_g=8, B=1, **_dg(8, 1, 2)),
    _s("g13", "dgroups", H=11, W=13, Cin=8, cout_g=8, **_dg(1, 3)),
    _s("g13e", "dgroups", H=11, W=24, Cin=8, cout_g=8, **_dg(1, 3)),
    # true groups out of a wider input
    _s("tg6", "tgroups", G=6, Cin=8, cout_g=8, H=9, W=12, x_gs=8, x_ch=48),
    _s("tg6o", "tgroups", G=6, Cin=8, cout_g=12, H=7, W=13, x_gs=8, x_ch=50, B=3),
    # stride 2: padding 0 and 1, odd and even maps, each output width class, true groups
    _s("s2p0w5", "s2", H=9, W=11, Cin=8, cout_g=8, sy=2, sx=2, pad_y=(0,), pad_x=(0,), B=3),
    _s("s2p1w6", "s2", H=10, W=12, Cin=8, cout_g=20, sy=2, sx=2, B=3),
    _s("s2p0w13", "s2", H=23, W=27, Cin=24, cout_g=36, sy=2, sx=2, pad_y=(0,), pad_x=(0,)),
    _s("s2p1w12", "s2", H=32, W=24, Cin=16, cout_g=128, sy=2, sx=2),
    _s("s2p1w35", "s2", H=17, W=70, Cin=8, cout_g=72, sy=2, sx=2, B=2),
    _s("s2p1w33", "s2", H=9, W=65, Cin=40, cout_g=8, sy=2, sx=2, B=1),
    _s("s2p0w32", "s2", H=17, W=66, Cin=16, cout_g=64, sy=2, sx=2, pad_y=(0,), pad_x=(0,), B=3),
    _s("s2tg3", "s2", G=3, Cin=8, cout_g=8, H=12, W=18, sy=2, sx=2, x_gs=8, x_ch=24, B=1, dil=(1, 1, 1), pad_y=(1, 1, 1), pad_x=(1, 1, 1)),
    # transposed: W + 1 in each width class; an odd W leaves bf16 planes 2-byte aligned
    _s("t4", "t", H=5, W=4, Cin=8, cout_g=8, transposed=True, B=3),
    _s("t7", "t", H=6, W=7, Cin=24, cout_g=36, transposed=True),
    _s("t8", "t", H=7, W=8, Cin=8, cout_g=12, transposed=True),
    _s("t12", "t", H=9, W=12, Cin=40, cout_g=20, transposed=True, B=1),
    _s("t30", "t", H=5, W=30, Cin=8, cout_g=72, transposed=True, B=1),
    _s("t31", "t", H=8, W=31, Cin=8, cout_g=8, transposed=True, B=1),
    _s("t32", "t", H=7, W=32, Cin=16, cout_g=64, transposed=True, B=2),
    _s("t44", "t", H=7, W=44, Cin=8, cout_g=12, transposed=True, B=1),
    # weight-heavy (the only large operands): more than 8 MiB of bf16 weights in at least four channel tiles
    _s("wh", "wheavy", H=6, W=5, Cin=512, cout_g=1024, B=2),
    _s("whs2", "wheavy", H=9, W=9, Cin=512, cout_g=1024, sy=2, sx=2, pad_y=(0,), pad_x=(0,), B=3),
    # the row-vector kernel: W 64 / 128, rows 9 / 16 / 19, its three variants, its per-group launches
    _s("rv9", "rv", H=9, W=64, Cin=8, cout_g=32),
    _s("rv16", "rv", H=16, W=128, Cin=24, cout_g=64, B=1),
    _s("rv19", "rv", H=19, W=64, Cin=64, cout_g=96, B=1),
    _s("rvg8", "rv", H=19, W=64, Cin=8, cout_g=8, B=1, **_dg(1, 2, 4, 8)),
    _s("rvg16", "rv", H=16, W=128, Cin=24, cout_g=16, B=1, **_dg(1, 2, 4, 8)),     # (the general kernel's 64-pixel tile fills its region bands here)
    _s("rvg12", "rv", H=16, W=64, Cin=8, cout_g=8, B=1, **_dg(1, 2)),      # (every residue class a whole number of 8-row tiles)
    _s("rvg32", "rv", H=9, W=64, Cin=8, cout_g=32, **_dg(8, 4, 2, 1)),
    # the dilation-group kernel: W 8 / 24 / 40 with odd heights, one or two 32-channel stages, 1 - 4 groups
    _s("dgw8", "dg", H=7, W=8, Cin=16, cout_g=8, B=3, **_dg(1, 2, 4, 8)),
    _s("dgw24", "dg", H=11, W=24, Cin=32, cout_g=12, B=1, **_dg(2, 8, 1)),
    _s("dgw40", "dg", H=19, W=40, Cin=40, cout_g=16, B=1, **_dg(1, 2, 4, 8)),
    _s("dgc64", "dg", H=9, W=24, Cin=64, cout_g=16, B=3, **_dg(4, 1)),
    _s("dg12", "dg", H=16, W=24, Cin=16, cout_g=16, B=1, **_dg(1, 2)),      # (the same for the dilation-group kernel: no ragged row block, no short residue)
    _s("dg1", "dg", H=13, W=40, Cin=16, cout_g=12, B=1, **_dg(2)),
)
SHAPE_BY_NAME = {s.name: s for s in SHAPES}
assert len(SHAPE_BY_NAME) == len(SHAPES)


FP_SHAPES = ("w24", "g4w24", "tg6", "s2p1w12", "t12", "rv9", "dgw24")


def _chains(s):
    if s.group == "wheavy":
        return ("style",)
    return CHAINS + (("demod",) if s.group in DEMOD_GROUPS or s.name in FP_SHAPES else ()) + (("stylefp",) if s.name in FP_SHAPES else ())


def _ios(s, chain):
    ios = ["f32", "bf", "bfoff"]
    if chain in ("style", "stylefp", "demod") and s.W % 2 == 0 and not s.x_gs:
        ios.append("modw")
    if s.group == "wheavy":
        return ("f32", "bf")
    return tuple(ios)


BASES = tuple(Case(s, c) for s in SHAPES for c in _chains(s))
CASES = tuple(Case(s, c, io) for s in SHAPES for c in _chains(s) for io in _ios(s, c))
CASE_BY_NAME = {c.name: c for c in CASES}


def entries(case):
    """the entries a case is launched on"""
    grp = case.shape.group
    if grp == "rv":
        return ("rv", "bf16") if case.io != "f32" else ("bf16",)
    if grp == "dg":
        return ("dg", "bf16") if case.io != "f32" else ("bf16",)
    if grp == "wheavy":
        return ("bf16",)
    return ("bf16", "x3") if case.io == "f32" else ("bf16",)


def launches(case):
    """(entry, hint) of every launch of a case"""
    m = mode_of(case)
    return [(e, h) for e in entries(case) for h in VARIANTS[e].get(m, ())]
