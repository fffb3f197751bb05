"""CPU proofs of tests/conv_bf16_ref.py: the restatement of the bf16 convolution family agrees with torch on the rounded operands, its weight
images follow the layouts include/vspbfr_hip.h documents, `form` (the dispatch, restated) is reached in every name and every fact by the case
table that tests/test_conv_bf16_forms_gpu.py launches, and wrong variants of the restatement miss the GPU test's bound on these very inputs.

Forms the table does not reach, by name, with the rule that makes them unreachable (test_unreachable_forms does the arithmetic):
    s2/v3/pt3, s2/v4/pt3, s2/v6/pt5   the stride-2 task count (2 PR - 1) * 2 PC depends on the tile alone: 594 or 578 tasks on the 128-pixel
                                      tiles (PT 5), 306 / 290 / 330 on the 64-pixel tile (PT 3), in every width class
    s2/*/pt7, tc/*/pt5, x3/*/pt7      launch_shape / launch_split have no such instance
    s1/v6/pt7                         a dilation above 64 (the entry refuses it)
    pt2 > 5 and the refusal "per-image weights: ... more than five pair tasks": a plane that launch_shape accepts has at most 896 positions
                                      and a pair task covers two of them: pt2 <= 5 wherever PT <= 7
    x3/s2 at tile widths 8 and 16     the doubled parity planes need 160 KB of LDS and more: refused ("tile does not fit LDS"), and the
                                      refusal is in the table
    tc pair forms, full last column   pairs need an even W, and W + 1 positions are never a multiple of the even tile width
    pair (with a scale) on a channel window: the window chain has no input scale and takes the copy-only staging
    a filled region band on the 128- and 256-pixel tiles, the persistent walks of the row-vector and dilation-group kernels over more
                                      tiles than workgroups: large maps only (test_conv2d_bf16_dilation_groups, test_conv2d_bf16rv_repeat
                                      and test_conv2d_bf16dg of tests/test_hip_ops.py keep them)
One mistake one might look for has no wrong variant: "the second channel octet of a Cin % 16 == 8 chunk read instead of zero" cannot show in a
result, because every weight image holds zeros past Cin (test_weight_images_follow_the_header) -- the octet's pixels are multiplied by zero
whatever they are.  The kernels do not read them (issue_p returns for an octet past Cin); the table holds Cin % 16 == 8 in every form."""
from collections import defaultdict

import pytest
import torch
import torch.nn.functional as F

import conv_bf16_ref as R
import conv_tile_ref as T

F64, F32 = torch.float64, torch.float32


def _hows(base):
    """the rounding points under which some launch of the (shape, chain) is accepted"""
    out = set()
    for c in R.CASES:
        if c.base == base:
            for e, h in R.launches(c):
                if R.form(c, e, h).code == R.OK:
                    out.add(R.rounding(c, e))
    return sorted(out)


SMALL = [b for b in R.BASES if b.shape.group != "wheavy"]


# ------------------------------------------------------------------------------------------------------------ against torch
def _torch_acc(case, x, wp_per_image):
    """F.conv2d / F.conv_transpose2d in float64, group by group; wp_per_image: [B or 1][G][9][Cin][cout_g]"""
    outs = []
    for b in range(case.B):
        wp = wp_per_image[b if wp_per_image.shape[0] > 1 else 0]
        per = []
        for g in range(case.G):
            w = wp[g].permute(2, 1, 0).reshape(case.cout_g, case.Cin, 3, 3).double()       # [tap][ci][co] -> OIHW
            xs = x[b:b + 1, g * case.x_gs:g * case.x_gs + case.Cin].double()
            if case.transposed:
                per.append(F.conv_transpose2d(xs, w.transpose(0, 1), stride=2))
            else:
                gi = 0 if case.G > 4 else g
                per.append(F.conv2d(xs, w, stride=(case.sy, case.sx), padding=(case.pad_y[gi], case.pad_x[gi]), dilation=case.dil[gi]))
        outs.append(torch.cat(per, 1))
    return torch.cat(outs)


@pytest.mark.parametrize("name", [b.name for b in SMALL])
def test_accumulation_equals_torch_on_the_rounded_operands(name):
    base = R.CASE_BY_NAME[name]
    d = R._window(base, R.inputs(base))
    st = R._staged(d, F64)
    for how in _hows(base):
        acc = R.accumulate(base, R.inputs(base), how, F64)
        if how == "pixel":
            ref = _torch_acc(base, R.bf16(st), R.bf16(d["wp"])[None])
        elif how == "weight":
            sc = d.get("in_scale")
            if sc is None:
                wpi = R.bf16(d["wp"])[None]
            else:
                sc = sc if sc.dim() == 2 else sc[None].expand(base.B, -1)
                wpi = torch.stack([R.bf16(d["wp"] * sc[b, :base.Cin].view(1, 1, -1, 1)) for b in range(base.B)])
            ref = _torch_acc(base, d["x"], wpi)
        else:
            (xh, xl), (wh, wl) = R._hi_lo(st), R._hi_lo(d["wp"])
            ref = _torch_acc(base, xh, wh[None]) + _torch_acc(base, xh, wl[None]) + _torch_acc(base, xl, wh[None])
            # the split products carry 16 significant bits: within the bound of test_conv2d_bf16x3 of the unrounded convolution
            full = _torch_acc(base, st, d["wp"][None])
            assert float(((acc - full).abs() - 6e-5 * full.abs()).max()) <= 6e-5, (name, float((acc - full).abs().max()))
        assert acc.shape == ref.shape
        assert float((acc - ref).abs().max()) <= 1e-12 * max(1.0, float(ref.abs().max())), (name, how)


def test_staged_operand_is_exact_before_its_rounding():
    """x * in_scale + in_shift is the same number in float32 and float64 on the grids the operands are drawn on (module docstring): the
    kernel's fmaf and the restatement cannot differ by a double rounding.  The full-precision chain has no shift: its product is exact in
    float64 and is rounded to fp32 once, as fmaf(x, s, 0) is."""
    for base in SMALL:
        d = R._window(base, R.inputs(base))
        assert torch.equal(R.bf16(d["x"]), d["x"]), base.name
        if base.chain == "stylefp":
            assert "in_shift" not in d
            continue
        assert torch.equal(R._staged(d, F32).double(), R._staged(d, F64)), base.name
        for k in ("res1", "res2"):
            if k in d:
                assert torch.equal(R.bf16(d[k]), d[k])


# ------------------------------------------------------------------------------------------------------------ weight images
@pytest.mark.parametrize("G,cin,cout", [(1, 8, 8), (1, 24, 36), (2, 40, 12), (3, 16, 72), (4, 8, 20), (1, 64, 160)])
def test_weight_images_follow_the_header(G, cin, cout):
    """every element of the three images is read back through the index formula of include/vspbfr_hip.h; rows past cout_g and channels
    past Cin are zero"""
    gen = torch.Generator().manual_seed(G * 1000 + cin + cout)
    wp = torch.randn(G, 9, cin, cout, generator=gen)
    nch, cop = (cin + 15) // 16, (cout + 31) // 32 * 32
    img = R.bf16_image(wp).float()
    assert img.numel() == G * nch * 9 * 2 * cop * 8
    x3 = R.bf16x3_image(wp).float()
    assert x3.numel() == 2 * img.numel()
    hi = wp.to(torch.bfloat16).float()
    lo = (wp - hi).to(torch.bfloat16).float()
    pick = torch.randint(0, img.numel(), (4000,), generator=gen).tolist() + [0, img.numel() - 1]
    for i in pick:
        j, r = i % 8, i // 8
        co, r = r % cop, r // cop
        octet, r = r % 2, r // 2
        tap, r = r % 9, r // 9
        chunk, g = r % nch, r // nch
        ci = 16 * chunk + 8 * octet + j
        inside = ci < cin and co < cout
        assert img[i] == (hi[g, tap, ci, co] if inside else 0.0)
        for part, src in ((0, hi), (1, lo)):
            k = ((((((g * nch + chunk) * 2 + part) * 9 + tap) * 2 + octet) * cop + co) * 8 + j)
            assert x3[k] == (src[g, tap, ci, co] if inside else 0.0)
    if cin % 8 == 0:
        rv = R.bf16rv_image(wp).float().view(G, -1)
        assert rv.shape[1] == (cin // 8) * 3 * 2 * 2 * cop * 8
        for i in torch.randint(0, rv.shape[1], (3000,), generator=gen).tolist():
            e, r = i % 8, i // 8
            co, r = r % cop, r // cop
            half, r = r % 2, r // 2
            quad, r = r % 2, r // 2
            ky, chunk = r % 3, r // 3
            kx, ci = e & 3, 8 * chunk + 4 * quad + 2 * half + (e >> 2)
            for g in range(G):
                assert rv[g, i] == (hi[g, 3 * ky + kx, ci, co] if kx < 3 and co < cout else 0.0)
    style = torch.rand(3, cin, generator=gen) + 0.5
    mod = R.modulated_image(wp, style)
    assert mod.shape == (3, img.numel())
    for b in range(3):
        assert torch.equal(mod[b], R.bf16_image((wp * style[b].view(1, 1, -1, 1))))      # the product in fp32, one rounding


# ------------------------------------------------------------------------------------------------------------ coverage
def _all_forms():
    out = []
    for c in R.CASES:
        for e, h in R.launches(c):
            out.append((c, e, h, R.form(c, e, h)))
    return out


def _kind(name):
    """staging kind of a general-kernel form name: f32 | iob | pair | nosc"""
    st = name.split("/")[3]
    return "nosc" if name.endswith("nosc") else ("pair" if st.startswith("pair") else st)


ALL = _all_forms()
ACCEPTED = [a for a in ALL if a[3].code == R.OK]


def test_table_size():
    assert 300 <= len(R.CASES) <= 900
    for s in R.SHAPES:
        if s.group != "wheavy":
            assert s.H <= 70 and s.W <= 128 and s.Cin <= 64, s.name
    assert [s.name for s in R.SHAPES if s.group == "wheavy"] == ["wh", "whs2"]


def test_every_form_name_is_reached():
    names = {f.name for _, _, _, f in ACCEPTED}
    # (variant, PT) of stride 1: the 256- and 128-pixel tiles at PT 3 / 5 / 7, the 64-pixel tile at 3 / 5 (PT 7 there: dilation > 64)
    want = {f"s1/v{v}/pt{pt}" for v in (1, 2, 3, 4, 6, 7) for pt in (3, 5, 7)} - {"s1/v6/pt7"}
    want |= {"s2/v3/pt5", "s2/v4/pt5", "s2/v6/pt3"} | {f"tc/v{v}/pt{pt}" for v in (4, 5, 8) for pt in (3, 7)}
    got = {"/".join(n.split("/")[:3]) for n in names if not n.startswith(("x3", "rv", "dg"))}
    assert got == want, (sorted(want - got), sorted(got - want))
    # every (variant, PT) in every staging form: fp32, one-pixel bf16 tasks (IOB without PAIR), pairs, copy-only pairs
    for vp in sorted(want):
        kinds = {_kind(n) for n in names if n.startswith(vp + "/")}
        assert kinds == {"f32", "iob", "pair", "nosc"}, (vp, sorted(kinds))
    pairs = {int(n.split("pair")[1].split("/")[0]) for n in names if "/pair" in n}
    assert pairs == {1, 2, 3, 5}        # PT of the pair forms: 1, 2, 3 and (for four or five tasks) 5
    assert {n for n in names if n.startswith("x3")} == {f"x3/s1/v{v}/pt{pt}" for v in (1, 4, 7) for pt in (3, 5)} | {
        "x3/s2/v6/pt3", "x3/s2/v7/pt5", "x3/tc/v5/pt3", "x3/tc/v5/pt5"}
    assert {n for n in names if n.startswith("rv/v")} == {"rv/v1", "rv/v2", "rv/v3"}
    assert any(n.startswith("rv/dg/") for n in names)
    assert {n for n in names if n.startswith("dg/")} == {f"dg/nst{n}/{k}" for n in (1, 2) for k in ("lean", "full")}
    # the lean form (scale and bias only: the SMART branch launch) with and without a style: its in-LDS weight modulation, out_scale, ch_scale
    # and ch_bias are compared with float64 in both stage counts, not only a bare convolution
    lean = {(f.name, f.facts["scaled"], c.chain) for c, e, h, f in ACCEPTED if e == "dg" and f.name.endswith("lean")}
    for nst in (1, 2):
        assert {(s, ch) for n, s, ch in lean if n == f"dg/nst{nst}/lean"} >= {(True, "demod"), (False, "plain")}, sorted(lean)
        assert {f.facts["scaled"] for c, e, h, f in ACCEPTED if f.name == f"dg/nst{nst}/full"} == {True, False}
    for c in R.CASES:       # the demod chain is what it says: a style, the demodulation, scale and bias, and nothing that makes a launch `full`
        if c.chain == "demod":
            o = T.operands(c)
            assert o["in_scale"] == "sample" and o["out_scale"] and o["ch_scale"] and o["ch_bias"]
            assert not (o["act1"] or o["act2"] or o["noise"] or o["res"] or o["in_shift"])
    # ... and the same chain runs on the general kernel (with and without per-image weights) and on the row-vector kernel
    assert {e for c, e, h, f in ACCEPTED if c.chain == "demod"} == {"bf16", "x3", "rv", "dg"}
    assert any(c.chain == "demod" and c.io == "modw" and f.name.endswith("nosc") for c, e, h, f in ACCEPTED)


def test_rv_and_dg_groups():
    """the per-group launches of the row-vector kernel run 8, 16 and 32 channels at each of the four dilations; the dilation-group kernel
    runs 1 - 4 groups, both stage counts, cout_g 8 / 12 / 16, batches 1 and 3"""
    seen, dgs = set(), set()
    for c, e, h, f in ACCEPTED:
        if e == "rv" and c.G > 1:
            seen |= {(c.cout_g, dl) for dl in c.dil}
        if e == "dg":
            dgs.add((c.G, c.Cin, c.cout_g, c.B, c.W))
    assert seen == {(cg, dl) for cg in (8, 16, 32) for dl in (1, 2, 4, 8)}
    assert {g for g, *_ in dgs} == {1, 2, 3, 4}
    assert {ci for _, ci, *_ in dgs} == {16, 32, 40, 64}
    assert {cg for _, _, cg, _, _ in dgs} == {8, 12, 16} and {b for *_, b, _ in dgs} == {1, 3} and {w for *_, w in dgs} == {8, 24, 40}
    # the facts of the two kernels, both ways wherever the served shapes let them vary
    vals = defaultdict(lambda: defaultdict(set))
    for c, e, h, f in ACCEPTED:
        if e in ("rv", "dg"):
            kind = "rv/dg" if f.name.startswith("rv/dg") else f.name.split("/")[0] if e == "dg" else "rv"
            for k, v in f.facts.items():
                vals[kind][k].add(v)
    assert vals["rv"]["ragged_row"] == {True, False}                    # rows 9 / 19 against 16 on the 8- and 16-row tiles
    assert vals["rv/dg"]["ragged_row"] == {True, False} and vals["rv/dg"]["spare"] == {True, False} and vals["rv/dg"]["ragged_co"] == {True, False}
    assert vals["dg"]["ragged_col"] == {True} and vals["dg"]["ragged_co"] == {True, False} and vals["dg"]["spare"] == {True, False}
    assert vals["dg"]["ragged_row"] == {True, False}


def test_workgroup_orders_and_their_facts():
    orders = defaultdict(list)
    for c, e, h, f in ACCEPTED:
        orders[f.order].append((c, e, h, f))
    assert {"xcd", "region", "launch", "wheavy(5,tail)", "wheavy(2,even)"} <= set(orders)
    # the two weight-heavy shapes against launch_bf's formula: 32-channel tiles -> groups of 5 with a last group of 2, 64-channel tiles -> 2
    for v, co_t in ((1, 32), (4, 64)):
        wtile = 512 * 9 * co_t * 2
        co_tiles = 1024 // co_t
        assert wtile * co_tiles > 8 << 20 and co_tiles >= 4
        cgs = (3 * 1024 * 1024 // 2) // wtile
        f = R.form(R.CASE_BY_NAME["wh/style"], "bf16", v)
        assert f.order == f"wheavy({cgs},{'tail' if co_tiles % cgs else 'even'})" == {1: "wheavy(5,tail)", 4: "wheavy(2,even)"}[v]
        assert co_tiles % cgs == {1: 2, 4: 0}[v]
    assert any(c.shape.name == "whs2" and f.order.startswith("wheavy") for c, e, h, f in ACCEPTED)
    assert {c.B for c, *_ in orders["wheavy(5,tail)"]} == {2} and {c.B for c, e, h, f in ACCEPTED if c.shape.name == "whs2"} == {3}
    # the XCD remap on grids that are and are not multiples of 8; the region order on filled and unfilled bands
    assert {f.facts["grid8"] for *_, f in orders["xcd"]} == {True, False}
    assert {f.facts["unfilled"] for *_, f in orders["region"]} == {True, False}
    assert {f.facts["grid8"] for *_, f in orders["launch"]} == {True, False}
    # G > 4 true groups in stride-1 mode, true groups in stride-2 mode, dilation groups the region order does not take
    assert {(c.G, R.mode_of(c)) for c, *_ in orders["launch"]} >= {(6, "s1"), (3, "s2"), (2, "s1")}


FACTS = ("ragged_row", "ragged_col", "ragged_co", "cin8", "spare", "grid8")


def test_every_fact_in_every_form():
    """both values of every fact the kernels branch on, per (mode, tile width class) and per staging kind; s0 = 1 on a ragged last column
    tile of an odd tile count; the channel window under the copy-only staging"""
    by = defaultdict(lambda: defaultdict(set))
    for c, e, h, f in ACCEPTED:
        if e not in ("bf16", "x3"):
            continue
        mode = R.mode_of(c)
        kind = "x3" if e == "x3" else _kind(f.name)
        for k in FACTS:
            by[(mode, kind)][k].add(f.facts[k])
        by[(mode, kind)]["twl"].add(f.facts["twl"])
        by[(mode, kind)]["window"].add(c.x_coff > 0)
        by[(mode, kind)]["B"].add(c.B)
        if "s0" in f.facts:
            for k in ("s0", "s0_last_ragged", "s0_last_ragged_odd"):
                by[(mode, kind)][k].add(f.facts[k])
    assert set(by) == {(m, k) for m in ("s1", "s2", "tc") for k in ("f32", "iob", "pair", "nosc", "x3")}
    for (mode, kind), facts in by.items():
        # (the doubled parity planes of the split form fit LDS on the widest class only: 160 KB and more at tile widths 8 and 16)
        assert facts["twl"] == ({5} if (mode, kind) == ("s2", "x3") else {3, 4, 5}), (mode, kind)
        assert facts["B"] == {1, 2, 3}, (mode, kind)
        # NOSC with x_ch > Cin among them.  (The window chain has no input scale, so on even rows it takes the copy-only staging: the pair
        # form with a scale computes the same image base and offsets and has no descriptor bound to get wrong.)
        assert facts["window"] == ({False} if kind == "pair" else {True, False}), (mode, kind)
        for k in FACTS:
            if k == "spare" and mode != "s1":
                continue        # only row-polyphase launches have spare blocks
            if k == "ragged_col" and mode == "tc" and kind in ("pair", "nosc"):
                assert facts[k] == {True}       # pairs need an even W: W + 1 positions are never a multiple of the (even) tile width
                continue
            assert facts[k] == {True, False}, (mode, kind, k)
        if kind in ("pair", "nosc"):
            assert True in facts["s0_last_ragged"] and True in facts["s0_last_ragged_odd"], (mode, kind)
            if mode != "tc":        # (the transposed patch always starts one column left of an even tile origin)
                assert facts["s0"] == {0, 1}, (mode, kind)
    # the epilogue forms on a ragged map: y_coff, res_coff, noise and both residuals on maps no tile divides, in every staging kind
    for kind in ("f32", "iob", "pair", "nosc"):
        hit = {c.chain for c, e, h, f in ACCEPTED if e == "bf16" and R.mode_of(c) == "s1" and f.facts["ragged_row"] and f.facts["ragged_col"]
               and _kind(f.name) == kind}
        assert ({"style"} if kind == "pair" else {"style", "placed"}) <= hit, (kind, hit)      # (the copy-only form: style in per-image weights)


def test_unreachable_forms():
    """the arithmetic behind the list of the module docstring, over every geometry bf_geom can produce"""
    s = R.SHAPE_BY_NAME
    for mode, shapes in (("s2", ("s2p0w5", "s2p1w12", "s2p1w35")),):
        for v, (MB, NB, WM, WN) in ((3, R.TILES[("s2", 3)]), (4, R.TILES[("s2", 4)]), (6, R.TILES[("s2", 6)])):
            pts = {R.bf_geom(R.Case(s[n], "plain"), mode, 32 * MB * WM, 32 * NB * WN, 32 * WM, 1).pt for n in shapes}
            assert pts == ({3} if v == 6 else {5}), (v, pts)
    # pt2 <= 5 wherever pt <= 7: every tile size, width class and dilation 1 .. 64
    for npix in (64, 128, 256):
        for twl in (3, 4, 5):
            TW, TH = 1 << twl, npix >> twl
            for dmax in range(1, 65):
                PR, PC = TH + 2, TW + 2 * dmax
                pt = (PR * R.bf_pitch(twl, PC) + 127) // 128
                pt2 = (PR * ((PC + 2) // 2) + 127) // 128
                assert pt > 7 or pt2 <= 5
            PR, PC = TH + 1, TW + 1
            assert ((2 * PR - 1) * PC + 127) // 128 <= 5 or ((2 * PR - 1) * 2 * PC + 127) // 128 > 5
    assert not any("five pair tasks" in f.why for *_, f in ALL)


def test_refusals_in_the_table():
    """every refusal the table meets, by entry: the GPU test requires the library's code and message for each"""
    seen = {(e, f.code, f.why) for c, e, h, f in ALL if f.code != R.OK}
    assert ("bf16", R.ENOTSUP, "tile does not fit LDS") in seen and ("bf16", R.ENOTSUP, "is too large") in seen
    assert ("x3", R.ENOTSUP, "tile does not fit LDS") in seen and ("x3", R.ENOTSUP, "is too large") in seen
    assert ("rv", R.ENOTSUP, "") in seen and ("dg", R.ENOTSUP, "") in seen and ("rv", R.EINVAL, "64-channel tiles need Cout") in seen


# ------------------------------------------------------------------------------------------------------------ wrong variants
def _tol(case, how, bf_out):
    r64, _, bound, _ = R.references(case, how)
    tol = torch.full_like(r64, bound)
    if bf_out:
        tol = tol + r64.abs() * 2.0 ** -8
    return r64, tol


WRONG_BASES = [b for b in SMALL if b.shape.name in ("w8", "w13", "w24", "w33", "w64", "d8w24", "g4w24", "g4w45", "g28", "g13", "tg6", "tg6o", "s2p0w13",
                                                    "s2p1w12", "s2tg3", "t7", "t12", "t31", "rv9", "dgw24", "dgc64")]


@pytest.mark.parametrize("v", R.WRONG_VARIANTS)
def test_wrong_variants_miss_the_bound(v):
    """each mistake, on every case of WRONG_BASES it could sit in and under each rounding the case is launched with, leaves the bound of the
    GPU test -- with the bf16 store term (2^-8 |float64| per element) wherever the case has a bf16 output form.  The two rounding-point
    mistakes move a result by a fraction of a bf16 ulp of the operands: they are required under the fp32-output bound only (R.FP32_ONLY), and
    so is any mistake on a case whose bf16 forms are all refused."""
    n = 0
    for base in WRONG_BASES:
        for how in _hows(base):
            if how == "weight" and "in_shift" in R.inputs(base):
                continue
            if not R.applies(base, how, v):
                continue
            bf_forms = any(c.base == base and c.io != "f32" and R.form(c, e, h).code == R.OK and R.rounding(c, e) == how
                           for c in R.CASES for e, h in R.launches(c))
            bf_out = bf_forms and v not in R.FP32_ONLY
            r64, tol = _tol(base, how, bf_out)
            y = R.reference(base, how, F64, wrong=v)
            m = T.written(base)
            miss = ((y - r64).abs() > tol) & m
            assert bool(miss.any()), (v, base.name, how)
            n += 1
    assert n >= 2, (v, n)
