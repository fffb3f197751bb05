"""CPU checks of tests/fir_ref.py, the float64 restatement tests/test_fir_forms_gpu.py holds the FIR kernels to:
  * it agrees with the fp32 oracle (oracle/ops.py) and with the reference's golden vectors on every cases.FIR_CASES entry;
  * its case table reaches every form the dispatch of csrc/upfirdn2d.hip can choose (fir_ref.form restates that dispatch);
  * it has teeth: each wrong variant of the restatement misses the bound on the shipped inputs, in every kernel family it could affect;
  * the tap sets are what the table says they are, by the rule of hip_ops.taps_separable;
  * the separable row / column order, evaluated in float32 here, lies within the bound (a kernel is entitled to that order)."""
import os

import pytest
import torch

import fir_ref as R
from oracle import cases, ops as O

torch.set_grad_enabled(False)
F64, F32 = torch.float64, torch.float32
RUNNABLE = [c for c in R.CASES if c.refuse is None and 0 not in R.case_out_size(c)]
_REFS = {}


def refs(case):
    """(operands, float64 reference, float32 reference) of a case, computed once"""
    if case.name not in _REFS:
        d = R.inputs(case)
        _REFS[case.name] = (d, R.reference(case, F64, ops=d), R.reference(case, F32, ops=d))
    return _REFS[case.name]


# ------------------------------------------------------------------------------------------------------------------ agreement
@pytest.mark.parametrize("name", list(cases.FIR_CASES))
def test_restatement_agrees_with_oracle_and_golden(golden, name):
    x, k, up, down, pad = cases.fir_inputs(name)
    ref64 = R.upfirdn2d_nchw(x, k, up, down, pad, F64)
    ref32 = R.upfirdn2d_nchw(x, k, up, down, pad, F32)
    R.bound(O.upfirdn2d(x, k, up, down, pad), ref64, ref32, what=f"oracle {name}")
    R.bound(torch.from_numpy(golden("ops")[name]), ref64, ref32, what=f"golden {name}")
    # the native layout with minor > 1 is the same operation on interleaved planes
    B, Cc, H, W = x.shape
    nat = R.upfirdn2d(x.permute(0, 2, 3, 1).contiguous(), k, up, down, pad, F64)
    assert torch.equal(nat.permute(0, 3, 1, 2), ref64[:, :, :, :])


# ------------------------------------------------------------------------------------------------------------------ coverage
def test_cases_reach_every_form():
    reached = {}
    for c in R.CASES:
        reached.setdefault(R.case_form(c), []).append(c.name)
    assert set(reached) == set(R.FORM_NAMES), (sorted(set(R.FORM_NAMES) - set(reached)), sorted(set(reached) - set(R.FORM_NAMES)))
    for c in R.CASES:
        if c.refuse is not None:
            assert R.case_form(c) in ("enotsup", "einval"), c.name
        else:
            assert R.case_form(c) not in ("enotsup", "einval"), c.name
    # what the issue's shapes are there for
    f = {c.name: R.case_form(c) for c in R.CASES}
    assert f["strip-2x3x5x17-asym4-sep-ps"] == "strip/sep/en" and R.case_out_size(R.CASE_BY_NAME["strip-2x3x5x17-asym4-sep-ps"]) == (4, 16)
    assert f["strip-2x3x3x15-asym4-sep-ps"] == "tile4/bf16/split-word" and R.case_out_size(R.CASE_BY_NAME["strip-2x3x3x15-asym4-sep-ps"]) == (4, 16)
    assert f["strip-2x2x35x19-asym4-sep-none"] == f["strip-2x5x33x24-asym4-sep-none"] == "strip/sep/plain+tail"
    assert f["strip-2x2x33x17-asym4-sep-none"] == f["strip-2x5x35x26-asym4-2d-none"] == "tile4/bf16/split-word"
    assert f["strip-2x3x34x25-asym4-sep-full"] == "strip/sep/en/act" and R.case_out_size(R.CASE_BY_NAME["strip-2x3x34x25-asym4-sep-full"]) == (33, 24)
    assert f["strip-2x3x34x21-asym4-2d-none"] == "strip/2d/plain+tail" and f["strip-2x3x34x21-asym4-sep-full"] == "tile4/bf16"
    assert f["strip-1x1x40x30-asym4-sep-none"] == "strip/major1"
    assert f["unaligned-res1"] == f["unaligned-noise"] == "tile4/bf16/unaligned"
    assert f["zero-corner-none"] == "strip/2d/plain" and f["zero-corner-full"] == "strip/2d/en/act"
    assert f["narrow-in-f32-full"] == f["narrow-in-bf16-full"] == "generic/epi" and f["refuse-bf16-narrow-in"] == "enotsup"
    assert f["short-plane-bf16"] == "tile4/bf16"
    assert f["pads-bf16--2_3_1_-2"] == "strip/2d/plain+tail" and f["pads-bf16-4_1_1_-2"] == "strip/2d/plain" and f["pads-f32-0_3_3_0"] == "tile4/f32"
    assert f["pads-bf16--1_2_1_-2"] == "tile4/bf16/split-word" and f["pads-bf16-2_1_2_1"] == f["pads-bf16-0_3_3_0"] == "strip/2d/plain+tail"
    assert f["pads-bf16-epi"] == "strip/2d/en/act"
    # every case stays small
    for c in RUNNABLE:
        assert c.B * c.C * c.H * c.W * c.minor * 4 <= 400 * 1024, c.name


def test_tile_plane_set_has_interior_inside_and_border_tiles():
    """72 x 200 planes: with pads (1, 1) / (2, 2) / (2, 1) and 2 ... 4 taps, tile (1, 1) of the 32 x 64 grid has its whole staged window inside
    the plane (the loader's fast path), tiles (0 ... 1, 0 ... 2) lie inside the output (the operand fast path) and the last row and column
    of tiles are cut."""
    for k in (2, 3, 4):
        for p0, p1 in ((1, 1), (2, 2), (2, 1)):
            in_h, in_w = 72, 200
            out_h, out_w = in_h + p0 + p1 - k + 1, in_w + p0 + p1 - k + 1
            tih, ldw = R.TOH + k - 1, 4 * ((R.TOW + k - 1 + 3) // 4)
            iy0, ix0 = R.TOH - p0, R.TOW - p0
            assert iy0 >= 0 and iy0 + tih <= in_h and ix0 >= 0 and ix0 + ldw <= in_w
            assert 2 * R.TOH <= out_h < 3 * R.TOH and 3 * R.TOW <= out_w < 4 * R.TOW


def test_dispatch_mirrors_the_python_gate():
    """hip_ops.fir_bf16_ok / blur_fused convert exactly the bf16 plane sets the library would refuse"""
    from vspbfr_amd import hip_ops as H
    for c in R.CASES:
        if c.entry != "blur" or c.dtype != "bf16":
            continue
        k = R.TAPS[c.taps]
        ok = H.fir_bf16_ok(k.shape[0], k.shape[1], 1, 1, 1, R.case_out_size(c)[1], c.W, c.H)
        assert ok == (not R.converts_to_f32(c)), c.name
        assert R.case_form(c) != "enotsup", c.name
    assert not H.fir_bf16_ok(4, 4, 1, 1, 1, 16, 3, 5) and H.fir_bf16_ok(4, 4, 1, 1, 1, 16, 4, 1) and H.fir_bf16_ok(4, 4, 1, 1, 1, 16)
    # from the library's side: no bf16 kernel below four input columns, whatever the pads make of the output
    assert R.form("bf16", 6, 5, 3, 4, 4, (1, 1), (1, 1), (8, 8, 8, 8), 1) == "enotsup"
    assert R.form("f32", 6, 5, 3, 4, 4, (1, 1), (1, 1), (8, 8, 8, 8), 1) == "generic"
    assert R.form("bf16", 6, 5, 4, 4, 4, (1, 1), (1, 1), (8, 8, 8, 8), 1).startswith("strip")


def test_header_states_the_separable_contract_on_the_last_tap():
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    src = open(os.path.join(root, "include", "vspbfr_hip.h")).read()
    at = src.index("VSP_FIR_SEPARABLE:")
    text = src[at:at + 900]
    assert "kernel[kh-1][kw-1] != 0" in text and "kernel[ky][kw-1] * kernel[kh-1][kx] / kernel[kh-1][kw-1]" in text
    assert "kernel[0][0]" not in text


# ------------------------------------------------------------------------------------------------------------------ taps
def test_tap_sets():
    from vspbfr_amd import hip_ops as H
    for name, k in R.TAPS.items():
        assert R.taps_separable(k) == R.SEPARABLE_TAPS[name], name
        assert H.taps_separable(k.clone()) == R.SEPARABLE_TAPS[name], name
    a = R.TAPS["asym4"]
    assert not torch.equal(a, a.t()) and not torch.equal(a, a.flip(0, 1)) and not torch.equal(a, a.flip(0)) and not torch.equal(a, a.flip(1))
    assert torch.equal(a, torch.outer(torch.tensor([1., 2., 4., 8.]), torch.tensor([1., 3., 5., 7.])) / 256)
    z = R.TAPS["zero4"]
    assert float(z[3, 3]) == 0.0 and float(z[0, 0]) != 0.0          # separable by the header's OLD wording, refused by the corner rule
    assert torch.equal(z * 49, torch.outer(torch.tensor([1., 3., 3., 0.]), torch.tensor([1., 3., 3., 0.])))
    for name in ("rand4", "rand3", "rand2"):
        k = R.TAPS[name]
        assert not torch.equal(k, k.t()) and not torch.equal(k, k.flip(0, 1))


# ------------------------------------------------------------------------------------------------------------------ mutants
FAMILIES = ("strip", "tile/f32", "tile/bf16", "generic")
AFFECTS = {v: FAMILIES for v in R.VARIANTS}
AFFECTS["sep_swap"] = ("strip",)


def _could_affect(variant, case, form):
    if variant == "sep_swap":
        return form.startswith("strip/sep")
    if variant in R.TAP_VARIANTS:
        return True
    ops = set(R.EPI[case.epi]) if case.epi is not None else set()
    need = {"scale_by_channel": {"plane_scale"}, "noise_by_plane": {"noise"}, "bias_after_act": {"act", "act_bias"},
            "res_before_act": {"act", "res1"}, "gain_pos_only": {"act"}}[variant]
    return need <= ops


@pytest.mark.parametrize("variant", R.VARIANTS)
def test_mutant_misses_the_bound(variant):
    """the wrong statement, evaluated in float32 (and rounded to bf16 where the kernel's output is), against the bound the GPU test uses,
    on the GPU test's inputs: missed at least once in every kernel family the mistake could sit in"""
    missed = {f: [] for f in AFFECTS[variant]}
    for c in RUNNABLE:
        form = R.case_form(c)
        fam = R.family(form)
        if fam not in missed or len(missed[fam]) >= 2 or not _could_affect(variant, c, form):
            continue
        d, ref64, ref32 = refs(c)
        bf = R.output_bf16(c)
        good = R.reference(c, F32, ops=d, order="sep" if form.startswith("strip/sep") else "2d")
        R.bound(R.round_bf16(good) if bf else good, ref64, ref32, bf16=bf, what=f"{c.name} definition")
        bad = R.reference(c, F32, variant=variant, ops=d)
        try:
            R.bound(R.round_bf16(bad) if bf else bad, ref64, ref32, bf16=bf, what=f"{c.name} {variant}")
        except AssertionError:
            missed[fam].append(c.name)
    assert all(missed.values()), {f: n for f, n in missed.items() if not n}


# ------------------------------------------------------------------------------------------------------------------ orders of the sum
@pytest.mark.parametrize("name", [c.name for c in RUNNABLE if R.case_form(c).startswith("strip/sep")])
def test_separable_order_in_float32_is_within_the_bound(name):
    """The strip kernel's separable form adds a row pass and a column pass where the definition adds sixteen products in one chain.
    That order, in float32 on the CPU, stays within the bound on every case that reaches the form (dyadic outer products: the two
    factors are exact, so it is the order alone)."""
    c = R.CASE_BY_NAME[name]
    d, ref64, ref32 = refs(c)
    sep32 = R.reference(c, F32, ops=d, order="sep")
    R.bound(sep32, ref64, ref32, what=f"{name} sep32")
    R.bound(R.round_bf16(sep32), ref64, ref32, bf16=True, what=f"{name} sep32 bf16")
    assert torch.equal(R.reference(c, F64, ops=d, order="sep"), ref64) or \
        float((R.reference(c, F64, ops=d, order="sep") - ref64).abs().max()) <= 1e-12 * float(ref64.abs().max())


def test_bf16_term_of_the_bound():
    """2^-8 |ref| is what a correctly rounded bf16 store needs: rounding the float64 reference itself reaches beyond 2^-9 |ref| and never
    beyond 2^-8 |ref|"""
    c = R.CASE_BY_NAME["tile-bf16-rand3-p11-full"]
    _, ref64, _ = refs(c)
    err = (ref64.float().to(torch.bfloat16).double() - ref64).abs()
    rel = (err / ref64.abs().clamp_min(1e-30)).max()
    assert 2.0 ** -9 < float(rel) <= 2.0 ** -8
