"""CPU checks of tests/conv_tile_ref.py, the float64 restatement behind tests/test_conv_tile_forms_gpu.py: the instance table read from the
sources names what the library names; the restatement equals torch's own convolutions where torch can express the case; the case table
reaches, per instance, every mode group and both values of every fact its kernel branches on -- or the instance is listed below by name
with the reason no shape reaches it; and every plausible mistake of the restatement misses the bound on every case it could sit in,
which is what makes the seeded inputs discriminating.  No GPU: the library is loaded for its configuration names only."""
from collections import defaultdict

import pytest
import torch
import torch.nn.functional as F

import conv_tile_ref as R

torch.set_grad_enabled(False)
CFGS = R.configs()


def test_config_table_names_what_the_library_names():
    from vspbfr_amd import _lib
    n = _lib.lib.vsp_conv2d_num_configs()
    names = [_lib.lib.vsp_conv2d_config_name(i).decode() for i in range(n)]
    assert names[-1] == "smallmap"
    tiled = [(i, s) for i, s in enumerate(names[:-1]) if "p3" not in s]
    assert [(c.index, c.name) for c in CFGS] == tiled           # the same entries at the same indices, in number and spelling
    assert all("p3" in s for s in names[len(CFGS):-1])          # the pipelined kernels follow them
    assert len({c.name for c in CFGS}) == len(CFGS)             # a name identifies an instance
    kinds = defaultdict(int)
    for c in CFGS:
        kinds[c.kind] += 1
        assert c.PF in (0, 1, 2) and c.WK in (1, 2, 4) and c.CK in (4, 8, 16, 32)
        assert c.kind == "plain" or c.WK == 1
    assert kinds["plain"] >= 90 and kinds["t"] >= 25 and kinds["d"] == 5


def _torch_conv(case, d):
    """the case by torch's own operators in float64, where they can express it (one geometry for all groups, no per-group dilation)"""
    g = R.geom(case)
    x = d["x"].double()
    if "in_scale" in d:
        sc = d["in_scale"].double()
        x = x * (sc[:, :, None, None] if sc.dim() == 2 else sc[None, :, None, None])
    w = d["w"].double()
    if case.transposed:
        return F.conv_transpose2d(x, w.transpose(0, 1), stride=2)
    outs = []
    for grp in range(case.G):
        xs = x[:, grp * case.x_gs:grp * case.x_gs + case.Cin]
        outs.append(F.conv2d(xs, w[grp * case.cout_g:(grp + 1) * case.cout_g], stride=(case.sy, case.sx), padding=(case.pad_y[min(grp, 3)] if case.G <= 4 else case.pad_y[0],
                                                                                                                case.pad_x[min(grp, 3)] if case.G <= 4 else case.pad_x[0]),
                             dilation=case.dil[min(grp, 3)] if case.G <= 4 else case.dil[0]))
    return torch.cat(outs, 1)


def _fused_leaky_relu(v, bias, slope, scale):
    """the oracle's fused_leaky_relu (oracle/ops.py): scale * leaky_relu(v + bias)"""
    return F.leaky_relu(v + bias[None, :, None, None], slope) * scale


@pytest.mark.parametrize("shape", [s.name for s in R.SHAPES])
def test_reference_equals_torch(shape):
    """plain, style (without the in-image shift torch's padding cannot express), the slopes and the placement, against F.conv2d /
    F.conv_transpose2d and leaky_relu; the bn chain on unpadded shapes, where the shift has no pad to miss"""
    for chain in (R.T_CHAINS if R.SHAPE_BY_NAME[shape].transposed else R.CHAINS):
        case = R.CASE_BY_NAME[f"{shape}/{chain}"]
        o, g, d = R.operands(case), R.geom(case), R.inputs(case)
        if o["in_shift"]:
            if case.transposed or any(p for p in case.pad_y + case.pad_x):
                continue
            d = dict(d)
            x = d["x"].double() * d.pop("in_scale").double()[None, :, None, None] + d.pop("in_shift").double()[None, :, None, None]
            d["x"] = x
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
        ref = R.references(case)[0]
        m = R.written(case)
        assert int(m.sum()) == v.numel() and bool((ref[~m] == R.SENTINEL).all())
        got = ref[m].reshape(case.B, g.Cout, *v.shape[2:])
        if case.transposed:
            exp = v
        else:
            rows = slice(g.oo[0], g.oo[0] + (g.OH - 1) * g.os[0] + 1, g.os[0])
            cols = slice(g.oo[1], g.oo[1] + (g.OW - 1) * g.os[1] + 1, g.os[1])
            for k in ("res1", "res2"):
                if k in d:
                    v = v + d[k].double()[:, g.res_coff:g.res_coff + g.Cout, rows, cols]
            exp = v
        assert tuple(got.shape) == tuple(exp.shape), case.name
        err = float((got - exp).abs().max())
        assert err <= 1e-12 * max(1.0, float(exp.abs().max())), (case.name, err)


def test_inputs_are_stable_and_references_shared():
    c = R.CASE_BY_NAME["d4/style"]
    assert R.inputs(c) is R.inputs(c) and R.references(c)[0] is R.references(c)[0]
    assert abs(float(R.inputs(c)["x"].mean()) - 1.0) < 0.05
    b, e = R.references(c)[2:]
    assert 0 < e < 1e-4 and b >= 4 * e


# ---------------------------------------------------------------------------------------------------------------- coverage
# Instances that reach nothing of a mode group or of a fact, by name, with the reason (LDS figures: make_plan's 100 KiB budget).
_NO_3X3 = ("a 64-channel slab of 32-channel chunks takes 9 * 32 * 80 * 4 = 92160 B for a 3x3 kernel (and more for a larger one) and the smallest "
           "64-pixel patch plane (8 x 8 + halo = 100 words, pitch 112) another 14336 B: only kernels of at most four taps fit, the 1x1 group")
_NO_S2 = "a 3x3 stride-2 patch of its tile is at least 33 x 33 words per channel: with the weight slab it exceeds the LDS budget for every tile shape"
UNSERVED = {
    ("4x4x1x1x32k4p1o1", g): _NO_3X3 for g in ("s1", "s2", "big", "sxy", "cin", "cout", "batch", "dgroups", "tgroups", "deepk")
} | {
    ("4x4x1x1x32k4p0o2", g): _NO_3X3 for g in ("s1", "s2", "big", "sxy", "cin", "cout", "batch", "dgroups", "tgroups", "deepk")
} | {
    ("2x4x2x1x32k4p0o1", g): _NO_3X3 for g in ("s1", "s2", "big", "sxy", "cin", "cout", "batch", "dgroups", "tgroups", "deepk")
} | {
    ("4x4x1x4x16k2p0o2", "s2"): _NO_S2,      # 46080 B of weights + 16 * 1089 * 4 B
    ("1x8x1x4x8k1p2o3", "s2"): _NO_S2,       # 512 pixels: 2 buffers * 8 * 2145 * 4 B
}
_T_NO_TAIL = ("a transposed tile of N positions stages (TH + 1) x (TW + 1) words and a strip 2 (N + 1): at most 130 words against 192 for the "
              "64-position tiles with PMAX 3, at most 297 against 384 for PMAX 6 (the 256-position tiles reach 387 on a map one column wide)")
UNREACHED = {
    # every plane of a 512-pixel tile holds at least 512 words, more than 64 * 6
    ("2x8x1x4x8k1p0o4", "tail", False): "512-pixel tile, PMAX 6", ("1x8x1x4x4k1p2o4", "tail", False): "512-pixel tile, PMAX 6",
    ("1x8x1x4x8k1p2o3", "tail", False): "512-pixel tile, PMAX 6",
} | {
    (n, "tail", True): _T_NO_TAIL for n in (
        "4x4x1x4x8k1p0o3t", "4x4x1x4x4k1p0o4t", "4x4x1x4x4k1p0o3t", "4x4x1x4x8k1p0o2t", "4x4x2x2x8k1p0o2t", "2x4x1x4x8k1p0o4t", "1x4x1x4x8k1p0o4t",
        "4x4x1x1x8k1p0o2t", "2x4x4x1x8k1p0o3t", "4x8x1x4x8k1p0o2t", "4x8x1x4x4k1p0o2t", "2x8x1x4x8k1p0o3t", "2x8x1x4x8k1p0o4t", "2x8x2x4x8k1p0o2t",
        "2x8x2x4x4k1p0o2t", "4x4x1x4x8k1p1o2t", "4x4x1x4x8k1p1o1t", "4x4x1x4x16k1p0o2t", "4x4x1x4x16k1p0o3t", "2x8x1x4x16k1p0o2t", "4x4x1x4x8k1p2o2t",
        "4x4x1x4x8k1p2o3t")
} | {
    # strips belong to the transposed mode, and there to tiles of at most 128 positions (make_plan)
    (c.name, "strips", True): "no strips" for c in CFGS if c.kind != "t" or 16 * c.WN * (c.NB // 4) > 128
} | {
    # LDS-DMA staging reads whole aligned float4 weight rows: make_plan refuses the launches that would take the scalar path
    (c.name, "w_vec4", False): "PF 2 refuses scalar weight rows" for c in CFGS if c.PF == 2
}


@pytest.fixture(scope="module")
def table():
    served, reach, pairs = defaultdict(set), defaultdict(set), 0
    for cfg in CFGS:
        for c in R.CASES:
            p = R.plan(c, cfg)
            if p.ok:
                pairs += 1
                served[cfg.name].add(c.group)
                for f in R.FACTS:
                    reach[(cfg.name, f)].add(getattr(p, f))
    return served, reach, pairs


def test_every_instance_serves_every_mode_group_of_its_kind(table):
    served, _, pairs = table
    missing = {(cfg.name, grp) for cfg in CFGS for grp in R.GROUPS if R.serves(cfg, grp) and grp not in served[cfg.name]}
    assert missing == set(UNSERVED), (sorted(missing - set(UNSERVED)), sorted(set(UNSERVED) - missing))
    assert all(served[cfg.name] for cfg in CFGS)                 # no instance is left without any case
    assert pairs > 25000
    for cfg in CFGS:                                             # and nothing is accepted outside its kind
        assert all(R.serves(cfg, grp) for grp in served[cfg.name]), cfg.name


def test_every_fact_is_reached_both_ways(table):
    _, reach, _ = table
    missing = {(cfg.name, f, v) for cfg in CFGS for f in R.FACTS for v in (True, False) if v not in reach[(cfg.name, f)]}
    assert missing == set(UNREACHED), (sorted(missing - set(UNREACHED)), sorted(set(UNREACHED) - missing))


def test_plan_rules():
    """the refusals the GPU module expects the library to share"""
    by = {c.name: c for c in CFGS}
    pf2, pf0, t0, d0 = by["4x4x1x4x8k1p2o2"], by["4x4x1x4x8k1p0o3"], by["4x4x1x4x8k1p0o3t"], by["4x4x1x4x4k1p0o2d"]
    assert R.plan(R.CASE_BY_NAME["d1/style"], pf2).ok and R.plan(R.CASE_BY_NAME["d1/bn"], pf2).why == "PF 2: in_shift"
    assert R.plan(R.CASE_BY_NAME["co7/plain"], pf2).why == "PF 2: cout_g % 4" and R.plan(R.CASE_BY_NAME["woff4/plain"], pf2).why == "PF 2: weight alignment"
    assert R.plan(R.CASE_BY_NAME["k2x5/plain"], pf2).why == "PF 2: more than 9 taps" and R.plan(R.CASE_BY_NAME["k2x5/plain"], pf0).ok
    assert not R.plan(R.CASE_BY_NAME["woff4/plain"], pf0).w_vec4 and not R.plan(R.CASE_BY_NAME["co7/plain"], pf0).w_vec4
    assert R.plan(R.CASE_BY_NAME["t16/plain"], pf0).why == "kind" and R.plan(R.CASE_BY_NAME["d1/plain"], t0).why == "kind"
    assert R.plan(R.CASE_BY_NAME["g4/plain"], d0).ok and not R.plan(R.CASE_BY_NAME["g2/plain"], d0).ok and not R.plan(R.CASE_BY_NAME["d1/plain"], d0).ok
    p = R.plan(R.CASE_BY_NAME["t16/plain"], t0)                  # 64 positions: 16 x 4 tiles cover 16 x 16 exactly, one strip block each way
    assert (p.TW, p.TH, p.tiles_x, p.tiles_y, p.strip_col, p.strip_row, p.strips) == (16, 4, 1, 4, 1, 1, True)
    p = R.plan(R.CASE_BY_NAME["t16x13/plain"], t0)
    assert (p.tiles_x, p.tiles_y, p.strips) == (1, 5, False)
    p = R.plan(R.CASE_BY_NAME["d8/plain"], pf0)                  # 256 pixels as 32 x 8, halo 8: 24 x 48 words, past 64 * 12
    assert (p.TW, p.TH, p.tail, p.lds) == (32, 8, True, (9 * 8 * 80 + 8 * 1168) * 4)


# ---------------------------------------------------------------------------------------------------------------- wrong variants
@pytest.mark.parametrize("variant", R.WRONG_VARIANTS)
def test_wrong_variant_misses_the_bound(variant):
    cases = R.variant_cases(variant)
    assert cases, variant
    for case in cases:
        ref64, _, b, _ = R.references(case)
        bad = R.reference(case, R.inputs(case), R.F64, wrong=variant)
        err = float((bad - ref64).abs().max())
        assert err > 100 * b, (variant, case.name, err, b)       # not near the bound: two orders beyond it


def test_wrong_variants_sit_in_every_group_they_could():
    where = {v: {c.group for c in R.variant_cases(v)} for v in R.WRONG_VARIANTS}
    plain_groups = set(R.GROUPS) - {"t"}
    assert where["shift_on_pad"] >= (plain_groups - {"tgroups", "k1"}) | {"t"}
    assert where["taps_transposed"] == set(R.GROUPS) - {"k1"}
    for v in ("noise_by_output", "noise_before_act1", "res_coff_ignored", "offset_swap"):
        assert where[v] == plain_groups, v
    for v in ("bias_before_scale", "bias2_with_prelu", "bias2_dropped", "prelu_ch0"):
        assert where[v] == set(R.GROUPS), v
    assert where["pad_swap"] == {"big"} and where["stride_swap"] == {"sxy"} and where["group_slice0"] == {"tgroups"}
    assert where["group_dil0"] == {"dgroups", "tgroups"} and where["t_phase_swap"] == where["last_col_dropped"] == {"t"}
