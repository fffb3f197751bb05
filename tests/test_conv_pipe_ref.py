"""CPU checks of tests/conv_pipe_ref.py, the restatement behind tests/test_conv_pipe_forms_gpu.py: the 33 pipelined instances read from
csrc/conv_pipe.hip carry the names and table positions the library gives them; the reference (tests/conv_tile_ref.py with the
dil_by_input_quarter form added) equals torch's own convolutions where torch can express the case; the case table reaches every instance in
every mode group its kind serves, every nchunk class, both values of every fact a launch branches on, the three variants of workgroup order 2
and the five small-map instantiations -- or the gap is listed below by name with the arithmetic that closes it; the three workgroup orders map
every grid of the table one-to-one onto (tile, channel tile, sample); and every plausible mistake misses the bound by two orders of magnitude
on every case it could sit in.  No GPU: the library is loaded for its configuration names only."""
from collections import defaultdict

import pytest
import torch
import torch.nn.functional as F

import conv_pipe_ref as P
import conv_tile_ref as R
from test_conv_tile_ref import _fused_leaky_relu, _torch_conv

torch.set_grad_enabled(False)
CFGS = P.configs()
BY_NAME = {c.name: c for c in CFGS}


def _release(case):
    """the weight-heavy shapes hold 19 MB per tensor: their inputs are not kept once a test is through with them"""
    if case.group in P.HEAVY or case.G > 100:
        R.inputs.cache_clear()


def test_config_table_names_what_the_library_names():
    from vspbfr_amd import _lib
    n = _lib.lib.vsp_conv2d_num_configs()
    names = [_lib.lib.vsp_conv2d_config_name(i).decode() for i in range(n)]
    assert names[-1] == "smallmap" and n - 1 == P.smallmap_index()
    assert [(c.index, c.name) for c in CFGS] == [(i, s) for i, s in enumerate(names[:-1]) if "p3" in s]
    assert [c.index for c in CFGS] == list(range(len(R.configs()), n - 1))      # after the tiled instances, up to smallmap
    kinds = defaultdict(int)
    for c in CFGS:
        kinds[c.kind] += 1
        assert c.CK in (4, 8) and (c.kind in ("plain", "t") or (c.MB, c.WM) == (4, 1))
    assert dict(kinds) == {"plain": 12, "t": 9, "d": 5, "fd": 3, "a": 4} and len(CFGS) == 33
    assert names[CFGS[-4].index] == "4x2x1x8x4k1p3o2r8a"      # the first `a` instance: the one tile_hint = 0 takes for every launch it fits


@pytest.mark.parametrize("shape", [s.name for s in P.P_SHAPES + P.S_SHAPES])
def test_reference_equals_torch(shape):
    """every chain against F.conv2d / F.conv_transpose2d and leaky_relu / prelu (the bn chain on unpadded shapes, where the shift has no pad
    to miss); dil_by_input_quarter as the sum of four dilated convolutions of the input quarters"""
    sh = next(s for s in P.P_SHAPES + P.S_SHAPES if s.name == shape)
    for chain in (P.chains_of(sh) if sh in P.P_SHAPES else (R.T_CHAINS if sh.transposed else R.CHAINS)):
        case = P.CASE_BY_NAME[f"{shape}/{chain}"]
        o, g, d = R.operands(case), R.geom(case), R.inputs(case)
        if o["in_shift"]:
            if case.transposed or any(p for p in case.pad_y + case.pad_x):
                continue
            d = dict(d)
            d["x"] = d["x"].double() * d.pop("in_scale").double()[None, :, None, None] + d.pop("in_shift").double()[None, :, None, None]
        if case.quarter:
            x, c4 = d["x"].double(), case.Cin // 4
            if "in_scale" in d:
                sc = d["in_scale"].double()
                x = x * (sc[:, :, None, None] if sc.dim() == 2 else sc[None, :, None, None])
            w = d["w"].double()
            v = sum(F.conv2d(x[:, q * c4:(q + 1) * c4], w[:, q * c4:(q + 1) * c4], padding=case.dil[q], dilation=case.dil[q]) for q in range(4))
        else:
            v = _torch_conv(case, d)
        if "out_scale" in d:
            v = v * d["out_scale"].double()[:, :, None, None]
        if "ch_scale" in d:
            v = v * d["ch_scale"].double()[None, :, None, None] + d["ch_bias"].double()[None, :, None, None]
        if o["act1"]:
            v = _fused_leaky_relu(v, d["bias1"].double(), 0.2, R.SQRT2)
        if "noise" in d:
            v = v + d["noise"].double()[:, None] * d["noise_w"].double()[0]
        if o["act2"] == 1:
            v = _fused_leaky_relu(v, d["bias2"].double(), o["slope2"], o["gain2"])
        elif o["act2"] == 2:
            v = F.prelu(v, d["prelu"].double())
        ref, m = R.references(case)[0], R.written(case)
        assert int(m.sum()) == v.numel() and bool((ref[~m] == R.SENTINEL).all())
        got = ref[m].reshape(case.B, g.Cout, *v.shape[2:])
        if not case.transposed:
            rows = slice(g.oo[0], g.oo[0] + (g.OH - 1) * g.os[0] + 1, g.os[0])
            cols = slice(g.oo[1], g.oo[1] + (g.OW - 1) * g.os[1] + 1, g.os[1])
            for k in ("res1", "res2"):
                if k in d:
                    v = v + d[k].double()[:, g.res_coff:g.res_coff + g.Cout, rows, cols]
        err = float((got - v).abs().max())
        assert err <= 1e-12 * max(1.0, float(v.abs().max())), (case.name, err)
        _release(case)


def test_every_float32_restatement_is_inside_its_own_bound():
    """the conditions of the GPU check: e_ref is positive and finite on every case, so 4 e_ref + 2e-6 max |float64| holds the float32
    restatement itself with room, and the sentinel lies outside every reference's range"""
    for case in P.CASES:
        r64, r32, b, e = R.references(case)
        m = R.written(case)
        assert 0.0 < e < 1e-4 and e <= b / 4 and float((r32.double() - r64).abs().max()) <= b, case.name
        assert float(r64[m].abs().max()) < abs(R.SENTINEL) / 4 and bool((r64[~m] == R.SENTINEL).all()), case.name
        _release(case)


def test_no_case_is_left_out_of_the_gpu_module():
    import test_conv_pipe_forms_gpu as G
    assert G.P_NAMES == [c.name for c in P.P_CASES] and G.S_NAMES == [c.name for c in P.S_CASES]
    assert {s.name for s in P.P_SHAPES} >= {"s2odd33", "s2p1", "s12", "s21", "pyx", "d2", "d8", "co36", "co72", "co132", "b1", "b3", "tg3", "tg6c8",
                                            "t16", "t32", "t7x13", "t16x13c8", "t8x16m", "t9x1", "g4", "g4sq", "g4big", "g4co12", "g4odd", "a16", "a32",
                                            "a64", "a128", "hv2048", "hv2112", "hvt1024", "hvt1056"}


# ---------------------------------------------------------------------------------------------------------------- coverage
# (group, instance) pairs no shape can reach, with the arithmetic
_NO_S2_R9 = ("4 waves with 8-channel chunks stage 9 rows = 576 words of a channel plane; a 256-pixel tile under a stride of 2 needs "
             "((TH - 1) sy + 3) ((TW - 1) sx + 3) >= 578 words for every TW TH = 256 (16 x 16: 18 x 33 = 594, 8 x 32: 34 x 17 = 578, 32 x 8: 17 x 34 = 578)")
_NO_S2_512 = ("a 512-pixel tile (32 x 16, or narrower and taller) under stride 2 x 2 needs at least 33 x 65 = 2145 words, more than 18 rows = 1152; "
              "stride (2, 1) fits (33 x 34 = 1122), stride (1, 2) does not (18 x 65 = 1170)")
UNSERVED = {("4x4x1x4x8k1p3o1r9", "s2"): _NO_S2_R9, ("4x4x1x4x8k1p3o1r9", "sxy"): _NO_S2_R9, ("4x4x1x4x8k1p3o1r9", "heavy"): _NO_S2_R9,
            ("4x4x1x8x8k1p3o1r18", "s2"): _NO_S2_512, ("4x4x1x8x8k1p3o1r18", "heavy"): _NO_S2_512}
# facts, per kind: (kind, fact, value)
UNREACHED = {
    ("t", "partial_row", False): "a transposed patch is (TH + 1) x (TW + 1) with TH, TW powers of two: odd; a strip is 2 (NPIX + 1): twice an odd number",
    ("t", "odd_pitch", True): "the odd pitch belongs to stride_x != 1, which the transposed mode normalises away",
    ("d", "odd_pitch", True): "dilation groups have stride 1 (make_plan)",
    ("fd", "odd_pitch", True): "dilation groups have stride 1 (make_plan)",
    ("a", "odd_pitch", True): "dilation groups have stride 1 (make_plan)",
    ("fd", "partial_row", True): "fixed geometry: the patch is 32 x 32 = 16 rows of 64 words",
}
# nchunk classes per instance
_A_CHUNKS = "Cin % 16 == 0 and (Cin / 4) % CK == 0 make nchunk = Cin / CK a multiple of 4"
NCHUNK_UNREACHED = {(c.name, k): _A_CHUNKS for c in CFGS if c.kind == "a" for k in ("1", "2", "3", "odd")}
# strips on the transposed instances
STRIPS_UNREACHED = {
    ("2x8x1x4x8k1p3o2r3t", True): "4 waves, 8-channel chunks, 3 rows = 192 words; strips need H % 8 == 0 and W % 16 == 0 (a narrower map has W + 1 > TW / 2, so "
                                  "W % TW != 0) and then the plane is 2 (128 + 1) = 258 words: make_plan refuses every launch that would run strips",
}


@pytest.fixture(scope="module")
def table():
    served, reach, chunks, strips, fast, o2, pairs = (defaultdict(set), defaultdict(set), defaultdict(set), defaultdict(set), defaultdict(set),
                                                     defaultdict(set), [0, 0])
    grids = set()
    for cfg in CFGS:
        for c in P.P_CASES:
            p = P.plan(c, cfg)
            pairs[0 if p.ok else 1] += 1
            if not p.ok:
                continue
            served[cfg.name].add(c.group)
            for f in P.FACTS:
                reach[(cfg.kind, f)].add(getattr(p, f))
            chunks[cfg.name].add(P.nchunk_class(p.nchunk))
            strips[cfg.name].add(p.strips)
            fast[cfg.name].add(p.t_fast)
            o2[cfg.kind].add(p.order2)
            o2[(cfg.kind, c.shape.name)].add(p.order2)
            if p.order2:
                o2[(cfg.kind, "grid8")].add((p.order2, p.grid8))
            if cfg.kind == "t" and p.ragged_pix and p.tiles_y > 1:
                o2[("t rows", cfg.name)].add(c.shape.name)
            grids.add((p.grid, p.order, p.cgs))
    return served, reach, chunks, strips, fast, o2, pairs, grids


def test_every_instance_is_accepted_in_every_mode_group_of_its_kind(table):
    served, pairs = table[0], table[6]
    missing = {(cfg.name, grp) for cfg in CFGS for grp in P.P_GROUPS if P.serves(cfg, grp) and grp not in served[cfg.name]}
    assert missing == set(UNSERVED), (sorted(missing - set(UNSERVED)), sorted(set(UNSERVED) - missing))
    assert all(served[cfg.name] for cfg in CFGS) and len(served) == 33
    for cfg in CFGS:
        assert all(P.serves(cfg, grp) for grp in served[cfg.name]), cfg.name      # nothing is accepted outside its kind
    assert pairs[0] > 4000 and pairs[1] > 10000


def test_every_fact_is_reached_both_ways_per_kind(table):
    reach = table[1]
    missing = {(k, f, v) for k in P.KINDS for f in P.FACTS for v in (True, False) if v not in reach[(k, f)]}
    assert missing == set(UNREACHED), (sorted(missing - set(UNREACHED)), sorted(set(UNREACHED) - missing))


def test_every_nchunk_class_strip_form_and_epilogue_path_per_instance(table):
    _, _, chunks, strips, fast, _, _, _ = table
    missing = {(c.name, k) for c in CFGS for k in P.NCHUNK_CLASSES if k not in chunks[c.name]}
    assert missing == set(NCHUNK_UNREACHED), (sorted(missing - set(NCHUNK_UNREACHED)), sorted(set(NCHUNK_UNREACHED) - missing))
    for c in CFGS:
        if c.kind == "fd":      # 1 ... 7 chunks: both parities of nchunk = 1, 2, 3, the even / odd remainder and the two-interval main loop
            n = {P.plan(k, c).nchunk for k in P.P_CASES if P.plan(k, c).ok}
            assert n >= set(range(1, 8)), (c.name, n)
    missing = {(c.name, v) for c in CFGS if c.kind == "t" for v in (True, False) if v not in strips[c.name]}
    assert missing == set(STRIPS_UNREACHED), missing
    assert all(strips[c.name] == {False} for c in CFGS if c.kind != "t")
    assert all(fast[c.name] == ({True, False} if c.kind == "t" else {False}) for c in CFGS)


def test_workgroup_order_2_is_reached_in_its_three_variants(table):
    o2 = table[5]
    for kind in ("plain", "t"):
        assert o2[kind] == {None, "tail", "notail", "cgs1"}, (kind, o2[kind])
    for kind in ("d", "fd", "a"):      # G = 4: the launch code asks for G == 1
        assert o2[kind] == {None}
    # both weight-heavy shapes of each mode run with a tail group / without one on the narrow channel tiles and with cgs = 1 on the wide ones
    assert o2[("plain", "hv2048")] == {"tail", "cgs1"} and o2[("plain", "hv2112")] == {"notail", "cgs1"}
    assert o2[("t", "hvt1024")] == {"tail", "cgs1"} and o2[("t", "hvt1056")] == {"notail", "cgs1"}
    # every variant on a grid that is a multiple of 8 and on one that is not (GT & 7 != 0: XCD ranges of unequal length over a narrow tail group)
    for kind in ("plain", "t"):
        assert o2[(kind, "grid8")] == {(v, g8) for v in ("tail", "notail", "cgs1") for g8 in (True, False)}, (kind, o2[(kind, "grid8")])
    p = P.plan(P.CASE_BY_NAME["hv2176/plain"], BY_NAME["2x4x2x4x8k1p3o1r18"])      # 34 tiles: 11 groups of 3 and a tail of 1; 102 = 8 * 12 + 6
    assert (p.co_tiles, p.cgs, p.order2, p.grid, p.grid8) == (34, 3, "tail", (1, 34, 3), False)
    p = P.plan(P.CASE_BY_NAME["hvt1088/plain"], BY_NAME["1x16x2x4x8k1p3o1r9t"])
    assert (p.co_tiles, p.cgs, p.order2, p.grid, p.grid8) == (34, 3, "tail", (1, 34, 3), False)


def test_ragged_transposed_tiles_in_more_than_one_tile_row_on_every_t_instance(table):
    """the non-strip transposed path with a second tile row (16 x 13: 17 position rows over tiles of 16 or 8)"""
    o2 = table[5]
    for c in CFGS:
        if c.kind == "t":
            assert "t16x13c8" in o2[("t rows", c.name)], c.name
            p = P.plan(P.CASE_BY_NAME["t16x13c8/plain"], c)
            assert p.ok and not p.strips and p.tiles_x == 1 and p.tiles_y == (2 if 16 * c.WN * (c.NB // 4) == 256 else 3)


def test_cases_that_every_instance_refuses_are_the_named_ones():
    for case in P.P_CASES:
        none = not any(P.plan(case, c).ok for c in CFGS)
        assert none == bool(R.operands(case)["in_shift"] or case.shape.name in P.REFUSED_BY_RULE), case.name
        if case.shape.name in P.REFUSED_BY_RULE and not R.operands(case)["in_shift"]:
            whys = {P.plan(case, c).why for c in CFGS if c.kind == ("d" if case.G == 4 else "plain")}
            assert whys == {P.REFUSED_BY_RULE[case.shape.name]}, (case.name, whys)
    p = P.plan(P.CASE_BY_NAME["hv2048/plain"], BY_NAME["2x4x2x4x8k1p3o1r18"])      # 64-wide tiles: 589824 B each, 3 per 2 MiB, 32 tiles
    assert (p.co_tiles, p.cgs, p.order2, p.grid, p.grid8) == (32, 3, "tail", (1, 32, 2), True)
    p = P.plan(P.CASE_BY_NAME["hv2112/plain"], BY_NAME["2x4x2x4x8k1p3o1r18"])
    assert (p.co_tiles, p.cgs, p.order2, p.grid, p.grid8) == (33, 3, "notail", (1, 33, 3), False)
    p = P.plan(P.CASE_BY_NAME["hv2048/plain"], BY_NAME["4x4x2x4x8k1p3o1r18"])      # 128-wide: 1179648 B, one per 2 MiB
    assert (p.co_tiles, p.cgs, p.order2) == (16, 1, "cgs1")
    p = P.plan(P.CASE_BY_NAME["hvt1024/plain"], BY_NAME["1x16x2x4x8k1p3o1r9t"])
    assert (p.co_tiles, p.cgs, p.order2, p.grid) == (32, 3, "tail", (1, 32, 2))
    p = P.plan(P.CASE_BY_NAME["hvt1056/plain"], BY_NAME["4x8x2x4x8k1p3o1r5t"])     # 128-wide: 2359296 B, 2 MiB / tile = 0, clamped to 1
    assert (p.co_tiles, p.cgs, p.order2) == (9, 1, "cgs1")


def test_all_five_smallmap_instantiations_and_every_refusal(table):
    forms = defaultdict(set)
    for c in P.S_CASES:
        f = P.smallmap_form(c)
        forms[f.inst if f.ok else f.why].add(c.shape.name)
    assert set(forms) == set(P.S_INSTS) | set(P.S_REFUSALS)
    assert forms["2x2v"] == {"smg128"} and forms["2x2s"] == {"smn8192s"} and forms["1x4v"] == {"smn8192", "smn3072"}
    assert {"smn3050", "smg127"} <= forms["1x2v"] and {"smn8160s", "smco7", "smco22", "smwoff"} == forms["1x2s"]
    # both sides of the two thresholds
    assert P.smallmap_form(P.CASE_BY_NAME["smn3072/plain"]).grid == (192, 1) and P.smallmap_form(P.CASE_BY_NAME["smn3050/plain"]).grid == (191, 1)
    assert P.smallmap_form(P.CASE_BY_NAME["smg128/plain"]).grid == (1, 256) and P.smallmap_form(P.CASE_BY_NAME["smg127/plain"]).grid == (1, 254)
    assert P.smallmap_form(P.CASE_BY_NAME["smn8192s/plain"]).grid == (256, 1) and P.smallmap_form(P.CASE_BY_NAME["smn8160s/plain"]).grid == (510, 1)
    assert P.smallmap_form(P.CASE_BY_NAME["smco7/plain"], w_off=0).inst == "1x2s" and P.smallmap_form(P.CASE_BY_NAME["smwoff/plain"], w_off=0).inst == "1x2v"


def test_plan_rules():
    """the refusals the GPU module expects the library to share, one of each rule"""
    why = lambda case, cfg: P.plan(P.CASE_BY_NAME[case], BY_NAME[cfg]).why      # noqa: E731
    pl, t, d, fd, a4, a8 = ("2x4x2x4x8k1p3o1r18", "2x16x2x4x8k1p3o1r9t", "4x2x1x8x4k1p3o2r8d", "4x2x1x8x8k1p3o1r16fd", "4x2x1x8x4k1p3o2r8a",
                            "4x2x1x8x8k1p3o1r16a")
    assert why("d1/plain", pl) == "" and why("d1/bn", pl) == "in_shift" and why("t16/bn", t) == "in_shift" and why("g4/bn", d) == "in_shift"
    assert why("a64/bn", a4) == "in_shift"
    assert why("t16/plain", pl) == "kind: transposed" and why("d1/plain", t) == "kind: transposed"
    assert why("a16/plain", pl) == why("a16/plain", d) == why("g4/plain", a4) == "kind: dil_by_input_quarter"
    assert why("g2/plain", d) == "not four 3x3 stride-1 dilation groups" and why("g4/plain", pl) == ""
    assert why("g4odd/plain", fd) == why("g4perm/plain", fd) == "fixed geometry: dilations are not 1, 2, 4, 8" and why("g4odd/plain", d) == ""
    assert why("k1/plain", pl) == "3x3 only" and why("co7/plain", pl) == "cout_g % 4" and why("woff4/plain", pl) == "weight alignment"
    assert why("cin12/plain", pl) == "Cin % CK" and why("cin12/plain", "2x4x2x4x4k1p3o1r9") == ""
    # a chunk lies inside one input-channel quarter: Cin = 16 and 32 leave quarters of 4 and 8 channels
    assert why("a16/plain", a8) == "(Cin / 4) % CK" and why("a16/plain", a4) == "" and why("a32/plain", a8) == "" and why("a64/plain", a8) == ""
    assert [why(f"a{c}/plain", "4x2x1x8x8k1p3o1r16a") for c in (16, 32, 64, 128)] == ["(Cin / 4) % CK", "", "", ""]
    assert why("s2odd33/plain", "4x4x2x4x8k1p3o1r18") == "" and why("s2odd33/plain", "4x4x1x4x8k1p3o1r9") == "patch rows"
    p = P.plan(P.CASE_BY_NAME["s2odd33/plain"], BY_NAME["4x4x2x4x8k1p3o1r18"])     # 33 x 33 = 1089 words in 18 rows of 64; odd pitch 1153
    assert (p.TW, p.TH, p.ps, p.lds, p.odd_pitch, p.partial_row) == (16, 16, 1153, 2 * (9 * 8 * 144 + 8 * 1153) * 4, True, True)
    p = P.plan(P.CASE_BY_NAME["t32/plain"], BY_NAME[t])      # 32 x 8 tiles cover 32 x 32; one strip block each way, (256 + 1) * 2 = 514 words
    assert (p.TW, p.TH, p.tiles_x, p.tiles_y, p.strip_col, p.strip_row, p.strips, p.grid) == (32, 8, 1, 4, 1, 1, True, (6, 1, 1))
    p = P.plan(P.CASE_BY_NAME["g4big/plain"], BY_NAME["4x4x1x8x4k1p3o1r12d"])     # 512 pixels: 32 x 16 tile, 32 x 48 patch
    assert (p.TW, p.TH, p.partial_row) == (32, 16, False)


# ---------------------------------------------------------------------------------------------------------------- workgroup orders
def test_workgroup_orders_are_one_to_one_on_every_grid(table):
    """orders 1 and 2 of conv_pipe.hip and the order of conv_smallmap.hip, restated as index arithmetic: every grid of the table is mapped
    onto its (tile, channel tile, sample) triples without a repeat or a gap.  (Order 0 is the dispatch order itself.)"""
    grids = table[7]
    assert any(o == 2 for _, o, _ in grids) and any(o == 1 for _, o, _ in grids)
    for grid, order, cgs in grids:
        GX, GY, GZ = grid
        GT = GX * GY * GZ
        seen = {(P.order1(w, grid) if order == 1 else P.order2(w, grid, cgs)) for w in range(GT)}
        assert seen == {(t, y, z) for t in range(GX) for y in range(GY) for z in range(GZ)}, (grid, order, cgs)
    # order 2 with cgs = 1 and without a tail is a relabelling of whole groups; with a tail the last group is narrower
    assert [P.order2(w, (2, 5, 1), 2) for w in (0, 8)] == [(0, 0, 0), (0, 1, 0)]
    for c in P.S_CASES:
        f = P.smallmap_form(c)
        if f.ok:
            GX, GY = f.grid
            assert {P.order_smallmap(w, f.grid) for w in range(GX * GY)} == {(x, y) for x in range(GX) for y in range(GY)}, c.name


# ---------------------------------------------------------------------------------------------------------------- wrong variants
@pytest.mark.parametrize("variant", P.WRONG_VARIANTS)
def test_wrong_variant_misses_the_bound(variant):
    cases = P.variant_cases(variant)
    assert cases, variant
    for case in cases:
        ref64, _, b, _ = R.references(case)
        bad = R.reference(case, R.inputs(case), R.F64, wrong=variant)
        err = float((bad - ref64).abs().max())
        assert err > 100 * b, (variant, case.name, err, b)
        _release(case)


def test_wrong_variants_sit_where_they_could():
    where = {v: {c.group for c in P.variant_cases(v)} for v in P.WRONG_VARIANTS}
    assert where["quarter_dil0"] == where["quarter_w_swap"] == {"a", "sm"}
    assert where["group_out_swap"] >= {"dgroups", "tgroups", "sm"} and where["group_scale0"] == {"tgroups", "sm"}
    assert where["last_row_dropped"] == where["last_col_dropped"] == {"t", "theavy", "sm"}
    assert where["res_coff_ignored"] >= {"s1", "s2", "sxy", "cin", "cout", "dgroups", "tgroups", "a", "heavy", "sm"}
    assert where["noise_by_output"] >= {"s1", "s2", "dgroups", "a", "heavy", "sm"}
    assert where["stride_swap"] == {"sxy"} and "s1" in where["pad_swap"]
