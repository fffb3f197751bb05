"""The pipelined (`...k1p3...`, csrc/conv_pipe.hip) and small-map (csrc/conv_smallmap.hip) fp32 conv kernels under the discipline of
tests/conv_tile_ref.py, on whose contract restatement, operands, inputs, reference and bound this module is built (nothing of the contract is
restated a second time here): the instance table read from the VSP_CFGP* lines, a restatement of make_plan's PF 3 branch and of the launch
code after it in vsp_conv2d_f32 (csrc/conv_igemm.hip), of smallmap_eligible / smallmap_launch, of the three workgroup orders as index
arithmetic, and the case tables that tests/test_conv_pipe_ref.py proves on the CPU and tests/test_conv_pipe_forms_gpu.py launches.

Kinds: "plain" (MODE 0), "t" (transposed, MODE 1), "d" (four dilation groups from one patch, MODE 2), "fd" (the same with fixed geometry:
16 x 16 pixels, dilations exactly 1, 2, 4, 8, the interval unrolled per LDS-buffer parity) and "a" (MODE 3, dil_by_input_quarter: the data
gradient of the dilation groups, y = sum_q conv(x[quarter q], W_q, dilation = padding = d_q)).

Workgroup order 0 (VSP_CONV_DBG = 16777216, a debug switch read once per process) is unreached by rule: no test sets it."""
import os
import re
from collections import namedtuple
from functools import lru_cache

import conv_tile_ref as R
from conv_tile_ref import CHAINS, Case, Shape, T_CHAINS, bound, geom, inputs, operands, reference, references, written  # noqa: F401

# ------------------------------------------------------------------------------------------------------------ the instance table
PCfg = namedtuple("PCfg", "index name MB NB WM WN CK PROWS OCC kind")
_SUFFIX = {"": "", "T": "t", "D": "d", "DF": "fd", "K": "a"}
KINDS = ("plain", "t", "d", "fd", "a")


@lru_cache(maxsize=None)
def configs():
    """the 33 conv_pipe_kernel instances in table order; index = tile_hint - 1 (they follow the tiled instances in build_table)"""
    src = re.sub(r"//[^\n]*", "", open(os.path.join(R.CSRC, "conv_pipe.hip")).read())
    src = src[src.index("kCfgsP[]"):]
    base, out = len(R.configs()), []
    for m in re.finditer(r"\bVSP_CFGP(|T|D|DF|K)\s*\(([^()]*)\)", src):
        a = [int(v) for v in m.group(2).split(",")]
        sfx = _SUFFIX[m.group(1)]
        if m.group(1) in ("", "T"):
            MB, NB, WM, WN, CK, PROWS, OCC = a
        else:
            NB, WN, CK, PROWS, OCC = a
            MB, WM = 4, 1
        name = f"{MB}x{NB}x{WM}x{WN}x{CK}k1p3o{OCC}r{PROWS}{sfx}"
        out.append(PCfg(base + len(out), name, MB, NB, WM, WN, CK, PROWS, OCC, sfx or "plain"))
    return tuple(out)


def smallmap_index():
    return len(R.configs()) + len(configs())


# ------------------------------------------------------------------------------------------------------------ cases
P_T_CHAINS = T_CHAINS + ("modonly",)       # the one chain the shipped up-convs hand over: the scale-only path of the t epilogue with a real out_scale
_s = R._s
_D4 = dict(G=4, dil=(1, 2, 4, 8), pad_y=(1, 2, 4, 8), pad_x=(1, 2, 4, 8))
_REUSED = ("d1", "d2", "d8", "s2p0", "s2p1", "s12", "s21", "cin12", "cin20", "cin40", "co7", "co36", "co72", "co128", "woff4", "b1", "b3", "k1", "g2", "g4",
           "g4sq", "g4rag", "tg3", "tg6", "t16", "t7x13", "t8x16m", "t32", "t9x1")
P_SHAPES = tuple(R.SHAPE_BY_NAME[n] for n in _REUSED) + (
    # stride 2 without padding on an odd map: 33 x 33 -> 16 x 16, the patch (33 x 33 = 1089 words) that fills the 18 rows of `r18`
    _s("s2odd33", "s2", H=33, W=33, sy=2, sx=2, pad_y=(0,), pad_x=(0,)),
    _s("pyx", "s1", H=14, W=17, pad_y=(0,), pad_x=(1,)),
    # Cin = CK, 2 CK, 3 CK, 4 CK, 5 CK for both chunk sizes (16, 12, 20 and 40 are reused shapes): every nchunk class on every plain / t instance
    _s("cin4", "cin", Cin=4, H=11, W=13),
    _s("cin8", "cin", Cin=8, H=11, W=13),
    _s("cin24", "cin", Cin=24, H=11, W=13),
    _s("cin32", "cin", Cin=32, H=11, W=13),
    _s("co132", "cout", B=1, Cin=8, H=9, W=11, cout_g=132),
    _s("tg6c8", "tgroups", G=6, Cin=8, cout_g=8, H=9, W=12, x_gs=8, x_ch=52),
    # 16 x 13 with chunks every instance takes (the reused shape has Cin = 10): 17 x 14 positions, ragged tiles in more than one tile row
    _s("t16x13c8", "t", Cin=8, H=16, W=13, transposed=True),
    _s("tcin4", "t", Cin=4, H=6, W=7, transposed=True),
    _s("tcin8", "t", Cin=8, H=6, W=7, transposed=True),
    _s("tcin12", "t", Cin=12, H=6, W=7, transposed=True),
    _s("tcin20", "t", Cin=20, B=1, H=7, W=15, transposed=True),      # 8 x 16 positions: whole tiles without strips
    _s("tcin24", "t", Cin=24, H=6, W=7, cout_g=36, transposed=True),
    _s("tcin40", "t", Cin=40, B=1, H=5, W=9, cout_g=72, transposed=True),
    _s("tco132", "t", Cin=8, B=3, H=8, W=16, cout_g=132, transposed=True),
    # dilation groups for d / fd: the three maps with 16 and 12 channels per group; dilations fd must refuse
    _s("g4co12", "dgroups", Cin=8, cout_g=12, H=19, W=23, **_D4),
    _s("g4big", "dgroups", B=1, Cin=8, cout_g=16, H=48, W=40, **_D4),
    _s("g4big12", "dgroups", B=1, Cin=8, cout_g=12, H=48, W=40, **_D4),
    _s("g4sq12", "dgroups", B=1, Cin=8, cout_g=12, H=32, W=32, **_D4),
    _s("g4odd", "dgroups", G=4, Cin=8, cout_g=16, H=12, W=15, dil=(1, 3, 5, 7), pad_y=(1, 3, 5, 7), pad_x=(1, 3, 5, 7)),
    _s("g4perm", "dgroups", G=4, Cin=8, cout_g=16, H=12, W=15, dil=(2, 1, 8, 4), pad_y=(2, 1, 8, 4), pad_x=(2, 1, 8, 4)),
) + tuple(
    # nchunk 1 ... 7 on both parities of the fd interval: Cin = 4 ... 28 for CK = 4, 8 ... 56 for CK = 8 (16 is g4)
    _s(f"fdc{c}", "dgroups", B=1, Cin=c, cout_g=16, H=9, W=20, **_D4) for c in (4, 8, 12, 20, 24, 28, 32, 40, 48, 56)
) + (
    # the data gradient of the dilation groups
    _s("a16", "a", Cin=16, cout_g=16, H=19, W=23, quarter=True, **_D4),
    _s("a32", "a", Cin=32, cout_g=12, H=33, W=20, quarter=True, **_D4),
    _s("a64", "a", Cin=64, cout_g=16, H=33, W=20, B=1, quarter=True, **_D4),
    _s("a128", "a", Cin=128, cout_g=12, H=19, W=23, B=1, quarter=True, **_D4),
    # dilations of its own, out of order (the halo is the largest, 5: a 26 x 26 patch with a partial last row) on whole 16 x 16 tiles
    _s("a64d", "a", G=4, Cin=64, cout_g=16, H=16, W=16, B=1, quarter=True, dil=(1, 3, 2, 5), pad_y=(1, 3, 2, 5), pad_x=(1, 3, 2, 5)),
    # weight-heavy layers (more than 16 MiB of weights, at least four channel tiles): workgroup order 2.  A 9 x 9 map leaves a 4-wide tile
    # whose 129 x 9 patch fits no 256-pixel instance, so the map is 9 x 33 (4 x 16 out); 2048 = 32 and 2112 = 33 tiles of 64 channels
    # (cgs = 3: a tail group of 2 / none), B = 2 and 3 make the grid a multiple of 8 and not
    _s("hv2048", "heavy", B=2, Cin=256, cout_g=2048, H=9, W=33, sy=2, sx=2, pad_y=(0,), pad_x=(0,)),
    _s("hv2112", "heavy", B=3, Cin=256, cout_g=2112, H=9, W=33, sy=2, sx=2, pad_y=(0,), pad_x=(0,)),
    # 2176 = 34 tiles: a tail group of 1 on a grid of 102, not a multiple of 8; 33 tiles x B = 8: no tail on a multiple of 8
    _s("hv2176", "heavy", B=3, Cin=256, cout_g=2176, H=9, W=33, sy=2, sx=2, pad_y=(0,), pad_x=(0,)),
    _s("hv2112b8", "heavy", B=8, Cin=256, cout_g=2112, H=9, W=33, sy=2, sx=2, pad_y=(0,), pad_x=(0,)),
    _s("hvt1024", "theavy", B=2, Cin=512, cout_g=1024, H=4, W=4, transposed=True),
    _s("hvt1056", "theavy", B=3, Cin=512, cout_g=1056, H=4, W=4, transposed=True),
    _s("hvt1088", "theavy", B=3, Cin=512, cout_g=1088, H=4, W=4, transposed=True),
    _s("hvt1056b8", "theavy", B=8, Cin=512, cout_g=1056, H=4, W=4, transposed=True),
)
HEAVY = ("heavy", "theavy")
# shapes that are in the p3 table for a refusal: every instance refuses them under every chain, by the rule named
REFUSED_BY_RULE = {"k1": "3x3 only", "co7": "cout_g % 4", "woff4": "weight alignment", "g4rag": "Cin % CK"}
S_SHAPES = (
    _s("sm1x1", "sm", B=1, Cin=16, H=3, W=5, KH=1, KW=1, pad_y=(0,), pad_x=(0,)),              # N = 15; S = 1: fewer sub-steps than wavefronts
    _s("smn1", "sm", B=1, Cin=32, H=3, W=3, cout_g=36, pad_y=(0,), pad_x=(0,)),                # N = 1; the vector form's cout_g - NI clamp
    _s("smn17", "sm", B=1, Cin=16, H=17, W=1, cout_g=20),                                      # N = 17
    _s("sm5", "sm", Cin=16, H=6, W=7, KH=5, KW=5, pad_y=(2,), pad_x=(2,)),
    _s("sm3x5", "sm", Cin=16, H=7, W=6, KH=3, KW=5, pad_y=(0,), pad_x=(2,)),
    _s("sms2", "sm", Cin=32, H=9, W=11, sy=2, sx=2),
    _s("smd2", "sm", Cin=16, H=8, W=9, dil=(2,), pad_y=(2,), pad_x=(2,)),
    _s("smco7", "sm", Cin=16, H=5, W=6, cout_g=7),
    _s("smco22", "sm", Cin=16, H=5, W=6, cout_g=22),
    _s("smwoff", "sm", Cin=16, H=5, W=6, cout_g=20, w_off=4),
    _s("smn8192", "sm", B=2, Cin=16, H=64, W=64, cout_g=8),                                    # 512 x 1 workgroups: 1x4v
    _s("smn3072", "sm", B=3, Cin=16, H=32, W=32, cout_g=8, KH=1, KW=1, pad_y=(0,), pad_x=(0,)),  # 192: 1x4v
    _s("smn3050", "sm", B=2, Cin=16, H=25, W=61, cout_g=8, KH=1, KW=1, pad_y=(0,), pad_x=(0,)),  # 191: 1x2v
    _s("smn8192s", "sm", B=2, Cin=16, H=64, W=64, cout_g=7, KH=1, KW=1, pad_y=(0,), pad_x=(0,)),  # 256: 2x2s
    _s("smn8160s", "sm", B=2, Cin=16, H=60, W=68, cout_g=7, KH=1, KW=1, pad_y=(0,), pad_x=(0,)),  # 255: 1x2s
    _s("smg128", "sm", B=1, G=128, Cin=16, H=4, W=4, cout_g=36, x_gs=16, x_ch=2048),           # 1 x 2 x 128 = 256 under 192 x 64 channels: 2x2v
    _s("smg127", "sm", B=1, G=127, Cin=16, H=4, W=4, cout_g=36, x_gs=16, x_ch=2032),           # 254: 1x2v
    _s("smdg4", "sm", Cin=16, H=9, W=9, cout_g=8, **_D4),
    _s("smtg6", "sm", G=6, Cin=16, H=6, W=5, cout_g=8, x_gs=16, x_ch=100),
    # what a named smallmap refuses
    _s("smcin8", "sm", Cin=8, H=5, W=6),
    _s("smn8193", "sm", B=1, Cin=16, H=1, W=8193, cout_g=4, KH=1, KW=1, pad_y=(0,), pad_x=(0,)),
    _s("smt", "sm", Cin=16, H=4, W=4, transposed=True),
    _s("sma", "sm", Cin=16, cout_g=8, H=9, W=9, quarter=True, **_D4),
)


def chains_of(shape):
    return P_T_CHAINS if shape.transposed else CHAINS


P_CASES = tuple(Case(s, c) for s in P_SHAPES for c in chains_of(s))
S_CASES = tuple(Case(s, c) for s in S_SHAPES for c in (T_CHAINS if s.transposed else CHAINS))
CASES = P_CASES + S_CASES
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)
P_GROUPS = tuple(dict.fromkeys(s.group for s in P_SHAPES))


def serves(cfg, group):
    """the mode groups an instance's kind serves at all (k1 is in the table for its refusal)"""
    if cfg.kind == "t":
        return group in ("t", "theavy")
    if cfg.kind in ("d", "fd"):
        return group == "dgroups"
    if cfg.kind == "a":
        return group == "a"
    return group not in ("t", "theavy", "a", "k1")


# ------------------------------------------------------------------------------------------------------------ make_plan (PF 3) and the launch
PPlan = namedtuple("PPlan", "ok why TW TH tiles_x tiles_y strip_col strip_row co_tiles ps lds grid order cgs "
                            "nchunk ragged_co ragged_pix strips partial_row odd_pitch grid8 order2 t_fast")
MAX_LDS_PIPE = 160 * 1024
FACTS = ("ragged_co", "ragged_pix", "partial_row", "odd_pitch", "grid8")      # two-valued on every kind (strips, t_fast: kind t; order2: G = 1)
NCHUNK_CLASSES = ("1", "2", "3", "even", "odd")


def nchunk_class(n):
    return str(n) if n <= 3 else ("even" if n % 2 == 0 else "odd")


def _refuse(why):
    return PPlan(False, why, *([None] * 21))


def plan(case, cfg):
    """What make_plan decides for the named PF 3 instance `cfg`, and what vsp_conv2d_f32 launches after it."""
    o, g = operands(case), geom(case)
    tc, kg, fg = cfg.kind == "t", cfg.kind == "a", cfg.kind == "fd"
    dg = cfg.kind in ("d", "fd", "a")
    if tc != case.transposed:
        return _refuse("kind: transposed")
    if kg != case.quarter:
        return _refuse("kind: dil_by_input_quarter")
    G, KH, KW = case.G, case.KH, case.KW
    dil = [case.dil[i] if i < len(case.dil) else case.dil[0] for i in range(4)]
    pad_y = [case.pad_y[i] if i < len(case.pad_y) else case.pad_y[0] for i in range(4)]
    pad_x = [case.pad_x[i] if i < len(case.pad_x) else case.pad_x[0] for i in range(4)]
    if dg:
        if G != 4 or case.x_gs != 0 or g.sy != 1 or g.sx != 1 or KH != 3 or KW != 3:
            return _refuse("not four 3x3 stride-1 dilation groups")
        if any(pad_y[i] != dil[i] or pad_x[i] != dil[i] for i in range(4)):
            return _refuse("padding != dilation")
    CO_T = 16 * cfg.MB * cfg.WM
    NPIX = 16 * cfg.WN * (cfg.NB // 4) if tc else 16 * cfg.NB * cfg.WN
    WS = CO_T + 16 if CO_T % 32 == 0 else CO_T
    cap = 5 if NPIX >= 256 else 4
    if dg:
        cap = 5 if NPIX >= 512 else 4
    twl = min(R._ilog2_ceil(g.OW), cap)
    if (1 << twl) > NPIX:
        twl = R._ilog2_ceil(NPIX)
    if fg:
        twl = 4
        if tuple(dil) != (1, 2, 4, 8):
            return _refuse("fixed geometry: dilations are not 1, 2, 4, 8")
    TW = 1 << twl
    TH = NPIX // TW
    ng = 1 if G > 4 else G
    gdil = dil if not tc else [1]
    dmax = max([1] + gdil[:ng])
    PH = TH + 1 if tc else (TH - 1) * g.sy + (KH - 1) * dmax + 1
    PW = TW + 1 if tc else (TW - 1) * g.sx + (KW - 1) * dmax + 1
    if PW > 256 or PH * PW >= 65536:
        return _refuse("patch too large")
    plane = PH * PW
    tiles_x, tiles_y, strip_col, strip_row = -(-g.OW // TW), -(-g.OH // TH), -1, 0
    if tc and case.H % TH == 0 and case.W % TW == 0:      # PF 3: strips whatever the tile size
        tiles_x, tiles_y = case.W // TW, case.H // TH
        strip_col, strip_row = -(-case.H // NPIX), -(-(case.W + 1) // NPIX)
        plane = max(plane, (NPIX + 1) * 2)
    if KH != 3 or KW != 3:
        return _refuse("3x3 only")
    if case.cout_g % 4 != 0:
        return _refuse("cout_g % 4")
    if case.w_off % 16 != 0:
        return _refuse("weight alignment")
    if o["in_shift"]:
        return _refuse("in_shift")
    if case.Cin % cfg.CK != 0:
        return _refuse("Cin % CK")
    if kg and case.Cin % 16 != 0:
        return _refuse("Cin % 16")
    if kg and (case.Cin // 4) % cfg.CK != 0:
        return _refuse("(Cin / 4) % CK")
    NW = cfg.WM * cfg.WN
    wpc = 1 if cfg.CK >= NW else NW // cfg.CK
    nrow = -(-plane // 64)
    odd = (not tc) and g.sx != 1
    ps = R._round_pitch(cfg.PROWS * wpc * 64, odd)
    if nrow > cfg.PROWS * wpc:
        return _refuse("patch rows")
    lds = 2 * (9 * cfg.CK * WS + cfg.CK * ps) * 4
    if lds > MAX_LDS_PIPE:
        return _refuse("LDS")
    co_tiles = -(-case.cout_g // (16 if dg else CO_T))
    gy = co_tiles if dg else co_tiles * G
    if gy > 65535 or case.B > 65535:
        return _refuse("grid")
    gx = tiles_x * tiles_y + (strip_col + strip_row if strip_col > 0 else 0)
    order, cgs, order2 = 1, 0, None
    if G == 1:
        wtile = case.Cin * KH * KW * CO_T * 4
        wall = wtile * co_tiles
        xall = case.B * case.Cin * case.H * case.W * 4
        if wall > 16 * 1024 * 1024 and co_tiles >= 4 and wall * 2 > xall // 8:
            cgs = max(1, min((2 * 1024 * 1024) // wtile, co_tiles))
            order = 2
            order2 = "cgs1" if cgs == 1 else ("tail" if gy % cgs else "notail")
    grid = (gx, gy, case.B)
    return PPlan(True, "", TW, TH, tiles_x, tiles_y, strip_col, strip_row, co_tiles, ps, lds, grid, order, cgs,
                 nchunk=case.Cin // cfg.CK, ragged_co=case.cout_g % (16 if dg else CO_T) != 0,
                 ragged_pix=strip_col < 0 and (g.OW % TW != 0 or g.OH % TH != 0), strips=strip_col >= 0, partial_row=plane % 64 != 0,
                 odd_pitch=odd, grid8=(gx * gy * case.B) % 8 == 0, order2=order2,
                 t_fast=tc and not any(o[k] for k in ("ch_scale", "ch_bias", "act1", "bias2", "act2")))


# ------------------------------------------------------------------------------------------------------------ the small-map launch
SForm = namedtuple("SForm", "ok why inst grid ct")
S_INSTS = ("1x4v", "2x2v", "1x2v", "2x2s", "1x2s")      # MI x NI, v: one NI-float load per weight row, s: scalar weight loads
S_REFUSALS = {"transposed": "configuration smallmap does not fit", "Cin % 16": "configuration smallmap does not fit",
              "positions": "configuration smallmap does not fit",
              # the entry does not look at `smallmap` under dil_by_input_quarter, so the name falls through to the check of the table's range
              "dil_by_input_quarter": "out of range"}


def smallmap_form(case, w_off=None):
    """which conv_smallmap_kernel instantiation smallmap_launch takes for a named `smallmap` and its grid, or why the entry refuses"""
    g = geom(case)
    w_off = case.w_off if w_off is None else w_off
    if case.quarter:
        return SForm(False, "dil_by_input_quarter", None, None, None)
    if case.transposed:
        return SForm(False, "transposed", None, None, None)
    if case.Cin % 16 != 0:
        return SForm(False, "Cin % 16", None, None, None)
    N = case.B * g.OH * g.OW
    if N > 8192:
        return SForm(False, "positions", None, None, None)
    n16, n32, G = -(-N // 16), -(-N // 32), case.G
    if w_off % 16 == 0 and case.cout_g % 4 == 0:
        ct4, ct2 = -(-case.cout_g // 64), -(-case.cout_g // 32)
        if n16 * ct4 * G >= 192:
            return SForm(True, "", "1x4v", (n16, ct4 * G), ct4)
        if n32 * ct2 * G >= 256:
            return SForm(True, "", "2x2v", (n32, ct2 * G), ct2)
        return SForm(True, "", "1x2v", (n16, ct2 * G), ct2)
    ct = -(-case.cout_g // 32)
    if n32 * ct * G >= 256:
        return SForm(True, "", "2x2s", (n32, ct * G), ct)
    return SForm(True, "", "1x2s", (n16, ct * G), ct)


# ------------------------------------------------------------------------------------------------------------ the workgroup orders
def _xcd_lid(wgid, GT):
    """dispatch index -> position in the logical order: the dispatcher deals workgroups round-robin over eight XCDs, each XCD walks a
    contiguous range (the first GT % 8 ranges one longer)"""
    xcd, xq, xr = wgid & 7, GT >> 3, GT & 7
    return (xcd * (xq + 1) if xcd < xr else xr * (xq + 1) + (xcd - xr) * xq) + (wgid >> 3)


def order1(wgid, grid):
    """conv_pipe.hip wg_order 1 -> (tile, by, bz)"""
    GX, GY, GZ = grid
    GN = GX * GY
    lid = _xcd_lid(wgid, GN * GZ)
    bz = lid // GN
    lrem = lid - bz * GN
    tile = lrem // GY
    return tile, lrem - tile * GY, bz


def order2(wgid, grid, cgs):
    """conv_pipe.hip wg_order 2 -> (tile, by, bz): groups of cgs channel tiles sweep every pixel tile of the batch; the tail group is narrower"""
    GX, GY, GZ = grid
    lid = _xcd_lid(wgid, GX * GY * GZ)
    npt = GX * GZ
    full = (GY // cgs) * cgs * npt
    if lid < full:
        cgrp = lid // (cgs * npt)
        rem, cw = lid - cgrp * (cgs * npt), cgs
    else:
        cgrp = GY // cgs
        rem, cw = lid - full, GY - cgrp * cgs
    pt = rem // cw
    by = cgrp * cgs + (rem - pt * cw)
    bz = pt // GX
    return pt - bz * GX, by, bz


def order_smallmap(wgid, grid):
    """conv_smallmap.hip -> (bx, by): row tile fastest, then channel tile"""
    GX, GY = grid
    lid = _xcd_lid(wgid, GX * GY)
    by = lid // GX
    return lid - by * GX, by


# ------------------------------------------------------------------------------------------------------------ wrong variants
NEW_VARIANTS = ("quarter_dil0", "quarter_w_swap", "group_out_swap", "group_scale0", "last_row_dropped")
WRONG_VARIANTS = R.WRONG_VARIANTS + NEW_VARIANTS


def applies(case, v):
    """whether mistake `v` could sit in the case (conv_tile_ref._applies for its sixteen)"""
    o = operands(case)
    if v == "quarter_dil0" or v == "quarter_w_swap":
        return case.quarter
    if v == "group_out_swap":      # a dilation group written to the channels of another group
        return case.G > 1 and not case.quarter
    if v == "group_scale0":
        return case.x_gs > 0 and o["in_scale"] is not None
    if v == "last_row_dropped":
        return case.transposed
    if case.quarter and v == "group_slice0":
        return False
    if v == "noise_by_output" and geom(case).OH * geom(case).OW == 1:      # one output position: both read noise[0, 0]
        return False
    return R._applies(case, v)


def variant_cases(v):
    return [c for c in CASES if applies(c, v)]
