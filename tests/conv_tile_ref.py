"""Float64 restatement of the vsp_conv2d_f32 contract (include/vspbfr_hip.h, "conv2d as an fp32-MFMA implicit GEMM") for the tiled
instances of conv_igemm_kernel (csrc/conv_kernel.h): the instance table read from the VSP_CFG* lines of csrc/conv_inst_*.hip, a
restatement of make_plan (csrc/conv_igemm.hip) for the staging modes PF 0 / 1 / 2, the reference, the project's bound and the case table
that tests/test_conv_tile_ref.py proves on the CPU and tests/test_conv_tile_forms_gpu.py launches on every instance.

Nothing of the package is imported here: the library is only asked for its configuration names, by the CPU test.

A case is a SHAPE (geometry: one entry of SHAPES, grouped by the mode it exercises) under an operand CHAIN:
    plain      no operand
    style      in_scale per sample, out_scale, act1 + bias1, noise, act2 = 1 + bias2 (slope 0.2, gain sqrt 2), two residuals with
               res_coff = 2 and res_ch = Cout + 3
    bn         folded BatchNorm: in_scale per channel + in_shift, ch_scale, ch_bias, PReLU; a bias2 pointer is handed over as well and
               must be ignored (act2 = 2 has no bias: the header's chain)
    slope001 / slope0 / slope1   act2 = 1 + bias2 with slope2 0.01 / 0 / 1 and gain2 = 1
    place      y_coff = 3 in y_ch = Cout + 5 channels, output stride (2, 2) offset (1, 1), noise and one residual (res_coff 1)
    placexy    the same with output stride (1, 2) and offset (1, 0) -- the one chain in which swapped offsets differ
The transposed mode has no noise, no residual and no output lattice: its style / place chains keep what the mode allows (the whole
per-channel `fin` chain; a channel window), and a shape of its own carries the larger output plane.  True groups have no in_shift
(validate_conv): their bn chain keeps the scale only."""
import math
import os
import re
import zlib
from collections import namedtuple
from dataclasses import dataclass
from functools import lru_cache

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "vspbfr_amd", "csrc")
SQRT2 = math.sqrt(2.0)
SENTINEL = -7777.25          # exact in fp32; what y holds wherever the launch must not write
F64, F32 = torch.float64, torch.float32

# ------------------------------------------------------------------------------------------------------------ the instance table
Cfg = namedtuple("Cfg", "index name MB NB WM WN CK WK PMAX PF OCC kind")


@lru_cache(maxsize=None)
def configs():
    """Every conv_igemm_kernel instance in table order (units a..g, the order build_table concatenates them): index = tile_hint - 1.
    kind: "plain", "t" (transposed) or "d" (fused dilation groups).  The name is the one the macro builds."""
    out = []
    for unit in "abcdefg":
        src = open(os.path.join(CSRC, f"conv_inst_{unit}.hip")).read()
        src = re.sub(r"//[^\n]*", "", src)
        for m in re.finditer(r"\bVSP_CFG([MDT]?)\s*\(([^()]*)\)", src):
            a = [int(v) for v in m.group(2).split(",")]
            which = m.group(1)
            if which in ("", "M"):
                MB, NB, WM, WN, CK, WK, PMAX, PF, OCC = a
                name, kind = f"{MB}x{NB}x{WM}x{WN}x{CK}k{WK}p{PF}o{OCC}" + (f"m{PMAX}" if which == "M" else ""), "plain"
            elif which == "D":
                NB, WN, CK, PMAX, PF, OCC = a
                MB, WM, WK = 4, 1, 1
                name, kind = f"4x{NB}x1x{WN}x{CK}k1p{PF}o{OCC}d", "d"
            else:
                MB, NB, WM, WN, CK, PMAX, PF, OCC = a
                WK = 1
                name, kind = f"{MB}x{NB}x{WM}x{WN}x{CK}k1p{PF}o{OCC}t", "t"
            out.append(Cfg(len(out), name, MB, NB, WM, WN, CK, WK, PMAX, PF, OCC, kind))
    return tuple(out)


# ------------------------------------------------------------------------------------------------------------ cases
@dataclass(frozen=True)
class Shape:
    name: str
    group: str
    B: int = 2
    Cin: int = 16
    H: int = 12
    W: int = 12
    G: int = 1
    cout_g: int = 24
    KH: int = 3
    KW: int = 3
    sy: int = 1
    sx: int = 1
    dil: tuple = (1,)
    pad_y: tuple = (1,)
    pad_x: tuple = (1,)
    x_gs: int = 0                 # > 0: true groups, group g reads input channels [g * x_gs, g * x_gs + Cin)
    x_ch: int = 0                 # channels of x (0: Cin)
    transposed: bool = False
    t_margin: tuple = (0, 0)      # transposed: rows / columns of the output plane beyond (2H+1) x (2W+1)
    w_off: int = 0                # bytes between the weight's first element and a 16-byte boundary
    quarter: bool = False         # dil_by_input_quarter (tests/conv_pipe_ref.py): G = 4 blocks of output channels, dilation by input quarter


@dataclass(frozen=True)
class Case:
    shape: Shape
    chain: str

    @property
    def name(self):
        return f"{self.shape.name}/{self.chain}"

    def __getattr__(self, k):     # geometry fields read through
        return getattr(object.__getattribute__(self, "shape"), k)


CHAINS = ("plain", "style", "bn", "slope001", "slope0", "slope1", "place", "placexy")
T_CHAINS = ("plain", "style", "bn", "slope001", "slope0", "slope1", "place")
SLOPES = {"slope001": 0.01, "slope0": 0.0, "slope1": 1.0}


def _s(name, group, **kw):
    return Shape(name, group, **kw)


SHAPES = (
    # 3x3 stride 1: dilation 1, 2, 4, 8 with padding = dilation, dilation 3 with padding 1; dilation 16 is the smallest halo whose plane
    # exceeds 64 * PMAX on the 16- and 64-pixel tiles with PMAX = 12
    _s("d1", "s1", H=19, W=23),
    _s("d2", "s1", H=21, W=18, dil=(2,), pad_y=(2,), pad_x=(2,)),
    _s("d4", "s1", H=23, W=37, dil=(4,), pad_y=(4,), pad_x=(4,)),
    _s("d8", "s1", H=26, W=35, dil=(8,), pad_y=(8,), pad_x=(8,)),
    _s("d3p1", "s1", H=17, W=20, dil=(3,), pad_y=(1,), pad_x=(1,)),
    _s("d16", "s1", H=20, W=33, B=1, dil=(16,), pad_y=(16,), pad_x=(16,)),
    # 3x3 stride 2
    _s("s2p0", "s2", H=23, W=27, sy=2, sx=2, pad_y=(0,), pad_x=(0,)),
    _s("s2p1", "s2", H=22, W=25, sy=2, sx=2),
    _s("s2d8", "s2", B=1, H=35, W=48, sy=2, sx=2, dil=(8,), pad_y=(8,), pad_x=(8,)),
    # 1x1; the 64-channel x 64-pixel instances with 32-channel chunks hold no 3x3 slab in LDS and reach their forms here: a stride-2 plane
    # past their two prefetched words, 64 channels in and out, scalar weight rows on a grid of three blocks
    _s("k1", "k1", H=13, W=21, KH=1, KW=1, pad_y=(0,), pad_x=(0,)),
    _s("k1s2", "k1", Cin=64, cout_g=64, H=15, W=33, KH=1, KW=1, sy=2, sx=2, pad_y=(0,), pad_x=(0,)),
    _s("k1co7", "k1", B=3, Cin=3, cout_g=7, H=5, W=7, KH=1, KW=1, pad_y=(0,), pad_x=(0,)),
    # larger and non-square kernels
    _s("k4p0", "big", H=14, W=17, KH=4, KW=4, pad_y=(0,), pad_x=(0,)),
    _s("k5", "big", H=13, W=18, KH=5, KW=5, pad_y=(2,), pad_x=(2,)),
    _s("k7", "big", H=15, W=12, KH=7, KW=7, pad_y=(3,), pad_x=(3,)),
    _s("k3x5", "big", H=11, W=19, KH=3, KW=5, pad_y=(1,), pad_x=(2,)),
    _s("k5x3p", "big", H=16, W=10, KH=5, KW=3, pad_y=(0,), pad_x=(2,)),
    _s("k2x5", "big", H=9, W=18, KH=2, KW=5, pad_y=(0,), pad_x=(2,)),     # 10 taps: the fewest that reach the weight tail loop
    # stride_y != stride_x
    _s("s12", "sxy", H=17, W=22, sy=1, sx=2),
    _s("s21", "sxy", H=17, W=22, sy=2, sx=1),
    # input channels: a ragged last chunk for CK = 4, 8, 16, 32; 64 divides every CK
    _s("cin3", "cin", Cin=3, H=11, W=13),
    _s("cin12", "cin", Cin=12, H=11, W=13),
    _s("cin20", "cin", Cin=20, H=11, W=13),
    _s("cin40", "cin", Cin=40, H=11, W=13),
    _s("cin64", "cin", Cin=64, H=9, W=17, cout_g=16),
    # output channels: scalar weight rows (7), ragged channel tiles (36, 72), the one tile every instance fills (128), and a weight that
    # starts 4 bytes into its storage
    _s("co7", "cout", H=10, W=14, cout_g=7),
    _s("co36", "cout", H=10, W=14, cout_g=36),
    _s("co72", "cout", H=10, W=14, cout_g=72),
    _s("co128", "cout", B=1, Cin=8, H=9, W=11, cout_g=128),
    _s("woff4", "cout", H=10, W=14, cout_g=16, w_off=4),
    # batch
    _s("b1", "batch", B=1, H=16, W=16, cout_g=16),
    _s("b3", "batch", B=3, H=7, W=9, cout_g=16),
    # dilation groups over one input: plain instances serve them group by group, the d instances fused (G = 4, dilations = paddings)
    _s("g2", "dgroups", G=2, cout_g=16, H=19, W=23, dil=(1, 2), pad_y=(1, 2), pad_x=(1, 2)),
    _s("g4", "dgroups", G=4, cout_g=16, H=19, W=23, dil=(1, 2, 4, 8), pad_y=(1, 2, 4, 8), pad_x=(1, 2, 4, 8)),
    _s("g4sq", "dgroups", G=4, cout_g=16, H=32, W=32, B=2, dil=(1, 2, 4, 8), pad_y=(1, 2, 4, 8), pad_x=(1, 2, 4, 8)),
    _s("g4rag", "dgroups", G=4, cout_g=12, Cin=6, H=19, W=23, dil=(1, 2, 4, 8), pad_y=(1, 2, 4, 8), pad_x=(1, 2, 4, 8)),
    _s("g4co7", "dgroups", G=4, cout_g=7, H=12, W=15, dil=(2, 1, 3, 2), pad_y=(2, 1, 3, 2), pad_x=(2, 1, 3, 2)),
    _s("g4small", "dgroups", G=4, cout_g=20, Cin=8, B=1, H=8, W=8, dil=(1, 1, 2, 1), pad_y=(1, 1, 2, 1), pad_x=(1, 1, 2, 1)),
    # true groups read out of a wider input; G = 3 keeps per-group geometry, G = 6 is uniform
    _s("tg3", "tgroups", G=3, Cin=8, cout_g=8, H=13, W=15, x_gs=10, x_ch=34, dil=(1, 2, 1), pad_y=(1, 2, 1), pad_x=(1, 2, 1)),
    _s("tg6", "tgroups", G=6, Cin=4, cout_g=8, H=9, W=12, x_gs=4, x_ch=28),
    # deep K on a tiny map (the K-split instances)
    _s("deepk", "deepk", Cin=200, H=5, W=5, cout_g=16),
    # transposed: a map the tile divides, one it does not, H divides and W does not, a larger output plane, a narrow map
    _s("t16", "t", H=16, W=16, transposed=True),
    _s("t7x13", "t", H=7, W=13, transposed=True),
    _s("t16x13", "t", H=16, W=13, Cin=10, transposed=True),
    _s("t8x16m", "t", H=8, W=16, transposed=True, t_margin=(1, 2)),
    _s("t32", "t", B=1, H=32, W=32, transposed=True, cout_g=16),
    _s("t6x5", "t", H=6, W=5, Cin=12, cout_g=7, transposed=True),
    _s("t8co128", "t", H=8, W=8, Cin=8, cout_g=128, transposed=True),
    _s("t9x1", "t", H=9, W=1, cout_g=16, transposed=True),     # two columns: the 256-position tiles become 128 rows tall
)
SHAPE_BY_NAME = {s.name: s for s in SHAPES}
assert len(SHAPE_BY_NAME) == len(SHAPES)
GROUPS = tuple(dict.fromkeys(s.group for s in SHAPES))
CASES = tuple(Case(s, c) for s in SHAPES for c in (T_CHAINS if s.transposed else CHAINS))
CASE_BY_NAME = {c.name: c for c in CASES}


def operands(case):
    """which operands the case's chain hands over, and its scalars"""
    ch, tr, tg = case.chain, case.transposed, case.x_gs > 0
    o = dict(in_scale=None, in_shift=False, out_scale=False, ch_scale=False, ch_bias=False, act1=False, noise=False, act2=0, bias2=False,
             slope2=0.2, gain2=SQRT2, res=0, res_coff=0, res_pad=0, y_coff=0, y_pad=0, os=(1, 1), oo=(0, 0))
    if ch in ("style", "stylefp"):      # (stylefp: tests/conv_bf16_ref.py, the style chain with scales of full fp32 precision)
        o.update(in_scale="sample", out_scale=True, act1=True, act2=1, bias2=True)
        if not tr:
            o.update(noise=True, res=2, res_coff=2, res_pad=3)
    elif ch == "demod":     # (tests/conv_bf16_ref.py: what a modulated layer without activation hands over -- style, demodulation, scale and bias)
        o.update(in_scale="sample", out_scale=True, ch_scale=True, ch_bias=True)
    elif ch == "modonly":   # (tests/conv_pipe_ref.py: what an up-conv of the path hands over -- style and demodulation, nothing else)
        o.update(in_scale="sample", out_scale=True)
    elif ch == "bn":
        o.update(in_scale="channel", in_shift=not tg, ch_scale=True, ch_bias=True, act2=2, bias2=True)
    elif ch in SLOPES:
        o.update(act2=1, bias2=True, slope2=SLOPES[ch], gain2=1.0)
    elif ch in ("place", "placexy", "placed"):
        o.update(y_coff=3, y_pad=5)
        if not tr:
            o.update(noise=True, res=1, res_coff=1, res_pad=2)
            if ch != "placed":      # "placed" (tests/conv_bf16_ref.py: entries with a dense output only) keeps the unit lattice
                o.update(os=(2, 2), oo=(1, 1)) if ch == "place" else o.update(os=(1, 2), oo=(1, 0))
    return o


Geom = namedtuple("Geom", "Cout OH OW sy sx dil pad_y pad_x y_ch y_coff y_h y_w os oo res_ch res_coff x_ch")


def geom(case):
    """the launch's derived sizes; a transposed case in the normalised form of normalise_transposed (csrc/conv_igemm.hip)"""
    o = operands(case)
    Cout = case.G * case.cout_g
    x_ch = case.x_ch or case.Cin
    if case.transposed:
        OH, OW = case.H + 1, case.W + 1
        y_h, y_w = 2 * case.H + 1 + case.t_margin[0], 2 * case.W + 1 + case.t_margin[1]
        return Geom(Cout, OH, OW, 1, 1, (1,), (1,), (1,), Cout + o["y_pad"], o["y_coff"], y_h, y_w, (2, 2), (0, 0), 0, 0, x_ch)
    d, py, px = case.dil[0], case.pad_y[0], case.pad_x[0]
    OH = (case.H + 2 * py - d * (case.KH - 1) - 1) // case.sy + 1
    OW = (case.W + 2 * px - d * (case.KW - 1) - 1) // case.sx + 1
    (osy, osx), (ooy, oox) = o["os"], o["oo"]
    # one row and two columns beyond the last lattice position: what lies off the lattice must survive as well
    y_h, y_w = (OH - 1) * osy + ooy + 1 + (1 if o["y_pad"] else 0), (OW - 1) * osx + oox + 1 + (2 if o["y_pad"] else 0)
    return Geom(Cout, OH, OW, case.sy, case.sx, case.dil, case.pad_y, case.pad_x, Cout + o["y_pad"], o["y_coff"], y_h, y_w, o["os"], o["oo"],
                Cout + o["res_pad"] if o["res"] else 0, o["res_coff"], x_ch)


def _pack(w, G):
    """(Cout, Cin, KH, KW) -> Wp[G][KH*KW][Cin][Cout / G], the layout the header states"""
    cout, cin, kh, kw = w.shape
    return w.reshape(G, cout // G, cin, kh * kw).permute(0, 3, 2, 1).contiguous()


@lru_cache(maxsize=None)
def inputs(case):
    """seeded float32 operands with a nonzero mean: x = 1 + N(0, 1), shifts and biases N(0, 1), scales in [0.5, 1.5], PReLU slopes in
    [0.05, 0.55] -- a misplaced pad, tap or channel moves the result by far more than the bound"""
    o, g = operands(case), geom(case)
    gen = torch.Generator().manual_seed(zlib.crc32(case.name.encode()))
    rn = lambda *s: torch.randn(*s, generator=gen, dtype=F32)        # noqa: E731
    ru = lambda *s: torch.rand(*s, generator=gen, dtype=F32) + 0.5   # noqa: E731
    d = {"x": 1.0 + rn(case.B, g.x_ch, case.H, case.W)}
    d["w"] = rn(g.Cout, case.Cin, case.KH, case.KW) / math.sqrt(case.Cin * case.KH * case.KW)
    d["wp"] = _pack(d["w"], case.G)
    if o["in_scale"] == "sample":
        d["in_scale"] = ru(case.B, g.x_ch)
    elif o["in_scale"] == "channel":
        d["in_scale"] = ru(g.x_ch)
    if o["in_shift"]:
        d["in_shift"] = rn(case.Cin)
    if o["out_scale"]:
        d["out_scale"] = ru(case.B, g.Cout)
    if o["ch_scale"]:
        d["ch_scale"] = ru(g.Cout)
    if o["ch_bias"]:
        d["ch_bias"] = rn(g.Cout)
    if o["act1"]:
        d["bias1"] = rn(g.Cout)
    if o["noise"]:
        d["noise"] = rn(case.B, g.OH, g.OW)
        d["noise_w"] = torch.tensor([0.7], dtype=F32)
    if o["bias2"]:
        d["bias2"] = rn(g.Cout)
    if o["act2"] == 2:
        d["prelu"] = torch.rand(g.Cout, generator=gen, dtype=F32) * 0.5 + 0.05
    for i in range(o["res"]):
        d[f"res{i + 1}"] = rn(case.B, g.res_ch, g.y_h, g.y_w)
    return d


# ------------------------------------------------------------------------------------------------------------ the reference
def _lrelu(v, slope):
    return torch.where(v > 0, v, v * slope)


def _accumulate(case, d, dtype, wrong):
    """acc[b, co, oy, ox] of the header, tap by tap from the packed weight"""
    g = geom(case)
    B, Cin, H, W, KH, KW = case.B, case.Cin, case.H, case.W, case.KH, case.KW
    x = xraw = d["x"].to(dtype)
    scb = None
    if "in_scale" in d:
        sc = d["in_scale"].to(dtype)
        scb = sc[:, :, None, None] if sc.dim() == 2 else sc[None, :, None, None]
        x = x * scb
    sh = d["in_shift"].to(dtype)[None, :, None, None] if "in_shift" in d else None
    wp = d["wp"].to(dtype)
    if case.transposed:
        # y = conv_transpose2d(xin, W, stride 2, padding 0): input (m, n) times tap (ky, kx) lands on output (2m + ky, 2n + kx)
        xin = x if sh is None else x + sh
        if wrong == "shift_on_pad":     # the staged halo (positions -1 and H / W) carries the shift instead of zero
            xe = sh.expand(B, Cin, H + 2, W + 2).clone()
            xe[:, :, 1:-1, 1:-1] = xin
            full = torch.zeros(B, g.Cout, 2 * H + 8, 2 * W + 8, dtype=dtype)
            for ky in range(3):
                for kx in range(3):
                    full[:, :, ky:ky + 2 * H + 4:2, kx:kx + 2 * W + 4:2] += torch.einsum("bchw,co->bohw", xe, wp[0, ky * 3 + kx])
            return full[:, :, 2:2 * H + 3, 2:2 * W + 3]
        acc = torch.zeros(B, g.Cout, 2 * H + 4, 2 * W + 4, dtype=dtype)
        for ky in range(3):
            for kx in range(3):
                tap = kx * 3 + ky if wrong == "taps_transposed" else ky * 3 + kx
                c = torch.einsum("bchw,co->bohw", xin, wp[0, tap])
                oy, ox = (2 * (ky >> 1) + (kx & 1), 2 * (kx >> 1) + (ky & 1)) if wrong == "t_phase_swap" else (ky, kx)
                acc[:, :, oy:oy + 2 * H:2, ox:ox + 2 * W:2] += c
        return acc[:, :, :2 * H + 1, :2 * W + 1]
    acc = torch.zeros(B, g.Cout, g.OH, g.OW, dtype=dtype)
    sy, sx = (case.sx, case.sy) if wrong == "stride_swap" else (case.sy, case.sx)
    if case.quarter:
        # dil_by_input_quarter: y = sum_q conv(x[quarter q], W[:, quarter q], dilation = padding = d_q) over all G * cout_g output channels;
        # the weight image is Wp[block][tap][ci][co] with ci over the whole input (tests/test_hip_ops.py, vspbfr_amd/training.py)
        c4 = Cin // 4
        for q in range(4):
            dl = case.dil[0] if (wrong == "group_dil0" or (wrong == "quarter_dil0" and q == 3)) else case.dil[q]
            qw = {1: 2, 2: 1}.get(q, q) if wrong == "quarter_w_swap" else q      # quarters 1 and 2 read each other's weight rows
            xs = x[:, q * c4:(q + 1) * c4]
            for ky in range(3):
                iy = torch.arange(g.OH) + (ky - 1) * dl
                my = (iy >= 0) & (iy < H)
                rows = xs[:, :, iy.clamp(0, H - 1)]
                for kx in range(3):
                    ix = torch.arange(g.OW) + (kx - 1) * dl
                    m = (my[:, None] & ((ix >= 0) & (ix < W))[None, :]).to(dtype)
                    v = rows[:, :, :, ix.clamp(0, W - 1)] * m
                    if sh is not None:
                        v = v + sh[:, q * c4:(q + 1) * c4] * (1.0 if wrong == "shift_on_pad" else m)
                    tap = kx * 3 + ky if wrong == "taps_transposed" else ky * 3 + kx
                    for blk in range(4):
                        acc[:, blk * case.cout_g:(blk + 1) * case.cout_g] += torch.einsum("bchw,co->bohw", v, wp[blk, tap, qw * c4:(qw + 1) * c4])
        return acc
    for grp in range(case.G):
        gi = 0 if (case.G > 4 or wrong == "group_dil0") else grp      # more than four groups share the geometry of group 0
        dl, py, px = case.dil[gi], case.pad_y[gi], case.pad_x[gi]
        if wrong == "pad_swap":
            py, px = px, py
        c0 = 0 if wrong == "group_slice0" else grp * case.x_gs
        xs = x[:, c0:c0 + Cin]
        if wrong == "group_scale0" and scb is not None:      # the group's own input under the scale of group 0
            xs = xraw[:, c0:c0 + Cin] * scb[:, :Cin]
        og = (grp + 1) % case.G if wrong == "group_out_swap" else grp      # written to the channels of the next group
        out = acc[:, og * case.cout_g:(og + 1) * case.cout_g]
        for ky in range(KH):
            iy = torch.arange(g.OH) * sy + ky * dl - py
            my = (iy >= 0) & (iy < H)
            rows = xs[:, :, iy.clamp(0, H - 1)]
            for kx in range(KW):
                ix = torch.arange(g.OW) * sx + kx * dl - px
                mx = (ix >= 0) & (ix < W)
                m = (my[:, None] & mx[None, :]).to(dtype)
                v = rows[:, :, :, ix.clamp(0, W - 1)] * m             # zero outside the image
                if sh is not None:
                    v = v + (sh if wrong == "shift_on_pad" else sh * m)   # the shift belongs to in-image pixels only
                tap = kx * KH + ky if wrong == "taps_transposed" else ky * KW + kx
                out += torch.einsum("bchw,co->bohw", v, wp[grp, tap])
    return acc


def reference(case, d, dtype, wrong=None, acc=None):
    """-> y [B, y_ch, y_h, y_w] in `dtype`: the contract's value where the launch writes, SENTINEL everywhere else.
    wrong: one of WRONG_VARIANTS (a plausible mistake, for the CPU test of the inputs), None = the contract.
    acc: the accumulators [B, Cout, OH, OW] when the caller has summed them itself (tests/conv_bf16_ref.py: operands rounded where the
    bf16 kernels round them); the epilogue chain and the placement are then applied to it."""
    o, g = operands(case), geom(case)
    B = case.B
    v = _accumulate(case, d, dtype, wrong) if acc is None else acc.to(dtype)
    ch = lambda k: d[k].to(dtype)[None, :, None, None]       # noqa: E731
    if "out_scale" in d:
        v = v * d["out_scale"].to(dtype)[:, :, None, None]
    if "ch_scale" in d or "ch_bias" in d:
        cs = ch("ch_scale") if "ch_scale" in d else 1.0
        cb = ch("ch_bias") if "ch_bias" in d else 0.0
        v = (v + cb) * cs if wrong == "bias_before_scale" else v * cs + cb
    nz = None
    if "noise" in d:
        n3 = d["noise"].to(dtype)
        if wrong == "noise_by_output":      # read at the output tensor's coordinates (wrapped into the plane)
            iy = (torch.arange(g.OH) * g.os[0] + g.oo[0]) % g.OH
            ix = (torch.arange(g.OW) * g.os[1] + g.oo[1]) % g.OW
            n3 = n3[:, iy][:, :, ix]
        nz = n3[:, None] * d["noise_w"].to(dtype)[0]
    if nz is not None and wrong == "noise_before_act1":
        v = v + nz
    if o["act1"]:
        v = _lrelu(v + ch("bias1"), 0.2) * SQRT2
    if nz is not None and wrong != "noise_before_act1":
        v = v + nz
    (osy, osx), (ooy, oox) = g.os, g.oo
    if wrong == "offset_swap":
        ooy, oox = oox, ooy
    rows = slice(ooy, ooy + (g.OH - 1) * osy + 1, osy)
    cols = slice(oox, oox + (g.OW - 1) * osx + 1, osx)

    def add_res(v):
        for k in ("res1", "res2"):
            if k in d:
                rc = 0 if wrong == "res_coff_ignored" else g.res_coff
                v = v + d[k].to(dtype)[:, rc:rc + g.Cout, rows, cols]      # the residual has the layout of the written region
        return v

    # (two mistakes that only tests/conv_bf16_ref.py draws: the residuals added before the second activation, bias2 added after it)
    if wrong == "res_before_act2" and not case.transposed:
        v = add_res(v)
    if o["act2"] == 1:
        if wrong == "bias2_after_act":
            v = _lrelu(v, o["slope2"]) * o["gain2"] + ch("bias2")
        else:
            v = _lrelu(v if wrong == "bias2_dropped" else v + ch("bias2"), o["slope2"]) * o["gain2"]
    elif o["act2"] == 2:
        if wrong == "bias2_with_prelu":
            v = v + ch("bias2")
        sl = d["prelu"].to(dtype)
        sl = sl[0].expand_as(sl) if wrong == "prelu_ch0" else sl
        v = torch.where(v >= 0, v, v * sl[None, :, None, None])
    y = torch.full((B, g.y_ch, g.y_h, g.y_w), SENTINEL, dtype=dtype)
    if case.transposed:
        win = y[:, g.y_coff:g.y_coff + g.Cout, :2 * case.H + 1, :2 * case.W + 1]
        if wrong == "last_col_dropped":
            win[..., :2 * case.W] = v[..., :2 * case.W]
        elif wrong == "last_row_dropped":
            win[..., :2 * case.H, :] = v[..., :2 * case.H, :]
        else:
            win.copy_(v)
        return y
    if wrong != "res_before_act2":
        v = add_res(v)
    y[:, g.y_coff:g.y_coff + g.Cout, rows, cols] = v
    return y


def written(case):
    """bool [B, y_ch, y_h, y_w]: the elements the launch writes"""
    g = geom(case)
    m = torch.zeros(case.B, g.y_ch, g.y_h, g.y_w, dtype=torch.bool)
    if case.transposed:
        m[:, g.y_coff:g.y_coff + g.Cout, :2 * case.H + 1, :2 * case.W + 1] = True
    else:
        m[:, g.y_coff:g.y_coff + g.Cout, g.oo[0]:g.oo[0] + (g.OH - 1) * g.os[0] + 1:g.os[0], g.oo[1]:g.oo[1] + (g.OW - 1) * g.os[1] + 1:g.os[1]] = True
    return m


def bound(ref64, ref32):
    """the project's rule (tests/fir_ref.py, tests/stream_ref.py): 4 e_ref + 2e-6 max |ref64| with e_ref the error of the same restatement
    in float32; taken over the written elements (everywhere else both hold SENTINEL).  -> (bound, e_ref)"""
    m = ref64 != SENTINEL
    e_ref = float((ref32.to(F64) - ref64).abs().max())
    return 4.0 * e_ref + 2e-6 * float(ref64[m].abs().max()), e_ref


@lru_cache(maxsize=None)
def references(case):
    """(ref64, ref32, bound, e_ref) of a case: computed once, shared, never modified"""
    d = inputs(case)
    r64, r32 = reference(case, d, F64), reference(case, d, F32)
    b, e = bound(r64, r32)
    return r64, r32, b, e


def _applies(case, v):
    """whether mistake `v` could sit in the case: the operand or geometry it touches is there and not degenerate"""
    o, g = operands(case), geom(case)
    tr = case.transposed
    padded = tr or any(p > 0 for p in case.pad_y[:min(case.G, 4)] + case.pad_x[:min(case.G, 4)])
    ng = 1 if case.G > 4 else case.G
    return {
        "shift_on_pad": o["in_shift"] and padded,
        "pad_swap": not tr and case.pad_y[0] != case.pad_x[0],
        "stride_swap": not tr and case.sy != case.sx,
        "group_dil0": not tr and len(set(case.dil[:ng])) > 1,
        "group_slice0": case.x_gs > 0,
        "taps_transposed": case.KH * case.KW > 1,
        "noise_by_output": o["noise"] and (g.os, g.oo) != ((1, 1), (0, 0)),
        "noise_before_act1": o["noise"] and o["act1"],
        "bias_before_scale": o["ch_scale"] and o["ch_bias"],
        "bias2_with_prelu": o["act2"] == 2,
        "bias2_dropped": o["act2"] == 1,
        "res_coff_ignored": o["res"] > 0 and o["res_coff"] > 0,
        "offset_swap": g.oo[0] != g.oo[1] and not tr,
        "prelu_ch0": o["act2"] == 2,
        "t_phase_swap": tr,
        "last_col_dropped": tr,
    }[v]


# "bias2 dropped when act2 = 2" is what the contract DOES (the header's chain gives act2 = 2 no bias, fill_convk passes bias2 on for
# act2 = 1 only); the two mistakes beside it are a bias2 added under PReLU (the bn chain hands a bias2 pointer over for that) and a bias2
# dropped under act2 = 1
WRONG_VARIANTS = ("shift_on_pad", "pad_swap", "stride_swap", "group_dil0", "group_slice0", "taps_transposed", "noise_by_output",
                  "noise_before_act1", "bias_before_scale", "bias2_with_prelu", "bias2_dropped", "res_coff_ignored", "offset_swap",
                  "prelu_ch0", "t_phase_swap", "last_col_dropped")


def variant_cases(v):
    return [c for c in CASES if _applies(c, v)]


# ------------------------------------------------------------------------------------------------------------ make_plan, restated
Plan = namedtuple("Plan", "ok why TW TH tiles_x tiles_y strip_col strip_row co_tiles lds grid tail ragged_chunk ragged_co w_vec4 grid8 strips")
MAX_LDS = 100 * 1024
FACTS = ("tail", "ragged_chunk", "ragged_co", "w_vec4", "grid8", "strips")


def _ilog2_ceil(v):
    l = 0
    while (1 << l) < v:
        l += 1
    return l


def _round_pitch(n, odd):
    if odd:
        return n | 1
    p = (n & ~31) + 16
    return p if p >= n else p + 32


def _refuse(why):
    return Plan(False, why, *([None] * 15))


def plan(case, cfg):
    """What make_plan (csrc/conv_igemm.hip) decides for a named instance with PF != 3, and the facts the case table is built on."""
    o, g = operands(case), geom(case)
    tc, dg = cfg.kind == "t", cfg.kind == "d"
    if tc != case.transposed:
        return _refuse("kind")
    G = case.G
    if dg:
        if G != 4 or case.x_gs != 0 or case.sy != 1 or case.sx != 1 or case.KH != 3 or case.KW != 3:
            return _refuse("not four 3x3 stride-1 dilation groups")
        if any(case.pad_y[i] != case.dil[i] or case.pad_x[i] != case.dil[i] for i in range(4)):
            return _refuse("padding != dilation")
    KH, KW = case.KH, case.KW
    CO_T = 16 * cfg.MB * cfg.WM
    NPIX = 16 * cfg.WN * (cfg.NB // 4) if tc else 16 * cfg.NB * cfg.WN
    WS = CO_T + 16 if CO_T % 32 == 0 else CO_T
    twl = min(_ilog2_ceil(g.OW), 5 if NPIX >= 256 else 4)
    if (1 << twl) > NPIX:
        twl = _ilog2_ceil(NPIX)
    TW = 1 << twl
    TH = NPIX // TW
    ng = 1 if G > 4 else G
    dils = [g.dil[i] if i < len(g.dil) else 1 for i in range(ng)]
    dmax = max([1] + dils)

    def patch(d, th=TH, tw=TW):
        return (th + 1, tw + 1) if tc else ((th - 1) * g.sy + (KH - 1) * d + 1, (tw - 1) * g.sx + (KW - 1) * d + 1)

    PH, PW = patch(dmax)
    if PW > 256 or PH * PW >= 65536:
        return _refuse("patch too large")
    plane = PH * PW
    tiles_x, tiles_y = -(-g.OW // TW), -(-g.OH // TH)
    strip_col, strip_row = -1, 0
    planes = [PH * PW] if (tc or dg) else [math.prod(patch(d)) for d in dils]      # per block: a plain block stages its own group's halo
    if tc and NPIX <= 128 and case.H % TH == 0 and case.W % TW == 0:
        tiles_x, tiles_y = case.W // TW, case.H // TH
        strip_col, strip_row = -(-case.H // NPIX), -(-(case.W + 1) // NPIX)
        plane = max(plane, (NPIX + 1) * 2)
        planes.append((NPIX + 1) * 2)                                               # 1 x NPIX and NPIX x 1 strips: 2 x (NPIX + 1) words
    PS = _round_pitch(plane, (not tc) and g.sx != 1)
    w_aligned = case.w_off % 16 == 0
    if cfg.PF == 2:
        if o["in_shift"]:
            return _refuse("PF 2: in_shift")
        if case.cout_g % 4 != 0:
            return _refuse("PF 2: cout_g % 4")
        if not w_aligned:
            return _refuse("PF 2: weight alignment")
        if KH * KW > 9:
            return _refuse("PF 2: more than 9 taps")
    lds = (KH * KW * cfg.CK * WS + (2 if cfg.PF == 2 else 1) * cfg.CK * PS) * 4
    lds = max(lds, (cfg.WK - 1) * cfg.WM * cfg.WN * cfg.MB * cfg.NB * 4 * 64 * 4)
    if lds > MAX_LDS:
        return _refuse("LDS")
    co_tiles = -(-case.cout_g // (16 if dg else CO_T))
    gy = co_tiles if dg else co_tiles * G
    if gy > 65535:
        return _refuse("grid")
    grid = (tiles_x * tiles_y + (strip_col + strip_row if strip_col > 0 else 0)) * gy * case.B
    return Plan(True, "", TW, TH, tiles_x, tiles_y, strip_col, strip_row, co_tiles, lds, grid,
                tail=any(p > 64 * cfg.PMAX for p in planes), ragged_chunk=case.Cin % cfg.CK != 0,
                ragged_co=case.cout_g % (16 if dg else CO_T) != 0, w_vec4=case.cout_g % 4 == 0 and w_aligned,
                grid8=grid % 8 == 0, strips=strip_col >= 0)


def serves(cfg, group):
    """the mode groups an instance's kind can serve at all"""
    if cfg.kind == "t":
        return group == "t"
    if cfg.kind == "d":
        return group == "dgroups"
    if cfg.PF == 2 and group == "big":      # LDS-DMA staging refuses more than 9 taps (make_plan)
        return False
    return group != "t"
