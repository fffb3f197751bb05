"""GPU checks of every tiled instance of conv_igemm_kernel (csrc/conv_kernel.h: the VSP_CFG / VSP_CFGM / VSP_CFGD / VSP_CFGT lines of
csrc/conv_inst_*.hip, every configuration that is neither pipelined (`p3`) nor `smallmap`) in every mode it serves, against the float64
restatement of tests/conv_tile_ref.py.  Every case of that module's table (a shape under an operand chain; tests/test_conv_tile_ref.py proves
on the CPU that the table reaches every instance, mode group and kernel branch, and that wrong variants of the restatement miss this bound on
these very inputs) is launched on EVERY instance with tile_hint = index + 1, through the C entry vsp_conv2d_f32 with a parameter block built
here (conv2d_packed has one stride and packs aligned weights only).  For each (case, instance) pair the library's verdict must equal
conv_tile_ref.plan's: "does not fit" exactly where plan refuses, otherwise

    max |HIP - float64| <= 4 e_ref + 2e-6 max |float64|        (conv_tile_ref.bound: the rule of tests/fir_ref.py and tests/stream_ref.py)

with e_ref the error of the same restatement in float32 on the CPU, and the sentinel intact in every element the launch must not write
(channels outside the window, positions off the output lattice, the margin of a larger transposed plane).  The reference of a case is
computed once and shared by the instances.  Every accepted pair prints its e_hip and its ratio to the case's e_ref under -s: one line per case, the instances by table index under the
figures they share.

Worst e_hip / e_ref per (kind, PF, WK) in the recorded run (profiles/conv_tile_forms_gputest.log: 395 passed in 8 s, 28843 accepted pairs):
    plain  PF 0: WK 1 7.56, WK 2 4.96, WK 4 2.48      PF 1: WK 1 7.56, WK 2 4.96, WK 4 2.34      PF 2: WK 1 7.56, WK 2 4.96
    t      PF 0 3.00, PF 1 2.82, PF 2 2.82            d     PF 0 4.05, PF 2 3.61
1288 pairs print more than 4 and so pass through the additive term of the bound alone, on 14 shapes (worst per shape): deepk 7.56 (K = 9 * 200, on
up to 78 of the 92 instances that serve it), cin40 6.54, cin64 5.71, d1 5.11, k3x5 4.98, co72 4.95, s21 4.91, k5 4.83, k5x3p 4.75, d8 4.53,
k7 4.26, co36 4.09, g4 4.05 (the one above 4 on a `d` instance; the plain instances with CK = 8 print the same 4.05 on that case), b1 4.03.  The
figure belongs to the summation order, not to an instance: an instance without K-split adds the K = Cin KH KW products of one output (operands of
mean 1) in ONE fp32 chain, the float32 restatement in KH KW blocked sums of Cin.  For one case the ratio is a function of (CK, WK) alone -- the same
on every staging mode, tile shape and kind -- and falls as the K-split shortens the chain (deepk/style: 7.56 / 6.98 with WK 1, 4.96 / 3.97 with WK 2,
2.17 / 1.67 with WK 4); the 1x1 shapes, where the restatement is one sum as well, print 1.00 on every instance, and no transposed pair (at most
4 * Cin products per output) exceeds 3.00.  In every one of the 1288 pairs e_hip is at most 1.07e-6 max |float64|, half the additive term: rounding
of a long fp32 sum, which is what that term is there for.

The first run of this table found one fault: the two fused dilation-group instances without LDS-DMA (4x4x1x4x4k1p0o2d, 4x4x1x4x8k1p0o2d) took the
scalar weight path for cout_g = 7 (and would for a weight off 16 bytes), and that path filled the slab as if its 64 columns were 64 channels of
group 0, not 16 channels of each of the four groups: groups 1 to 3 came out as if their weights were zero (8 cases of shape g4co7, errors of 5 to
6).  commit() in csrc/conv_kernel.h now addresses the scalar path by group as the vector path does; the cases stay in the table."""
import ctypes as C
from collections import defaultdict

import pytest
import torch

import conv_tile_ref as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
CFGS = R.configs()
BY_NAME = {c.name: c for c in CFGS}
WORST = {}            # (kind, PF, WK) -> (ratio e_hip / e_ref, pair, e_hip / max |float64|)
PAIRS = defaultdict(int)
OVER4 = defaultdict(int)      # shape -> pairs that pass through the additive term of the bound alone (e_hip > 4 e_ref)


@pytest.fixture(scope="module")
def L():
    from vspbfr_amd import _lib
    return _lib


def _place(t, off=0):
    """t on the device, contiguous; off > 0: a view that starts so many bytes past a 16-byte boundary"""
    if t is None:
        return None
    t = t.to(DEV).contiguous()
    if not off:
        assert t.data_ptr() % 16 == 0
        return t
    buf = torch.zeros(t.numel() + 8, dtype=t.dtype, device=DEV)
    skip = off // t.element_size()
    v = buf[skip:skip + t.numel()].view(t.shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == off and v.is_contiguous()
    return v


class Launch:
    """a case's operands on the device and its parameter block; run(hint) fills y with the sentinel and launches"""

    def __init__(self, L, case, slope2=None, w_off=None):
        o, g, d = R.operands(case), R.geom(case), R.inputs(case)
        self.L, self.case = L, case
        self.t = {k: _place(v, (case.w_off if w_off is None else w_off) if k == "wp" else 0) for k, v in d.items() if k != "w"}
        self.y = torch.empty(case.B, g.y_ch, g.y_h, g.y_w, device=DEV)
        t, p = self.t, L.ConvParams()
        ptr = lambda k: t[k].data_ptr() if k in t else None     # noqa: E731
        p.x, p.w, p.y = t["x"].data_ptr(), t["wp"].data_ptr(), self.y.data_ptr()
        p.B, p.Cin, p.H, p.W, p.G, p.cout_g = case.B, case.Cin, case.H, case.W, case.G, case.cout_g
        p.KH, p.KW = case.KH, case.KW
        p.transposed = 1 if case.transposed else 0
        if case.transposed:     # the entry ignores and normalises these: hand it values it must not use
            p.OH = p.OW = 1
            p.stride_y = p.stride_x = p.osy = p.osx = 1
        else:
            p.OH, p.OW, p.stride_y, p.stride_x = g.OH, g.OW, case.sy, case.sx
            (p.osy, p.osx), (p.ooy, p.oox) = g.os, g.oo
        for i in range(4):
            j = i if i < len(case.dil) else 0
            p.dil[i], p.pad_y[i], p.pad_x[i] = case.dil[j], case.pad_y[j], case.pad_x[j]
        p.y_ch, p.y_coff, p.y_h, p.y_w = g.y_ch, g.y_coff, g.y_h, g.y_w
        p.in_scale, p.in_shift = ptr("in_scale"), ptr("in_shift")
        p.in_scale_bstride = g.x_ch if o["in_scale"] == "sample" else 0
        p.out_scale, p.ch_scale, p.ch_bias = ptr("out_scale"), ptr("ch_scale"), ptr("ch_bias")
        p.act1, p.bias1, p.slope1, p.gain1 = (1 if o["act1"] else 0), ptr("bias1"), 0.2, R.SQRT2
        p.noise, p.noise_w = ptr("noise"), ptr("noise_w")
        p.act2, p.bias2, p.prelu = o["act2"], ptr("bias2"), ptr("prelu")
        p.slope2, p.gain2 = (o["slope2"] if slope2 is None else slope2), o["gain2"]
        p.res1, p.res2, p.res_ch, p.res_coff = ptr("res1"), ptr("res2"), g.res_ch, g.res_coff
        p.x_ch, p.x_group_stride = (g.x_ch if case.x_gs else 0), case.x_gs
        self.p = p

    def run(self, hint):
        self.y.fill_(R.SENTINEL)
        self.p.tile_hint = hint
        self.L.check(self.L.lib.vsp_conv2d_f32(C.byref(self.p), C.c_void_p(torch.cuda.current_stream().cuda_stream)), "conv2d")
        return self.y


def _runs(idx):
    """[0, 2, 3, 4, 7] -> '0,2-4,7'"""
    out, i = [], 0
    while i < len(idx):
        j = i
        while j + 1 < len(idx) and idx[j + 1] == idx[j] + 1:
            j += 1
        out.append(str(idx[i]) if j == i else f"{idx[i]}-{idx[j]}")
        i = j + 1
    return ",".join(out)


def _device_fault(e):
    return any(s in str(e) for s in ("HIP error", "illegal memory access", "hipError", "unspecified launch failure"))


class Checker:
    """the shared references of a case on the device; errors(y) -> (max error on the written elements, max change of the others)"""

    def __init__(self, case):
        self.ref64, _, self.bound, self.e_ref = R.references(case)
        self.top = (self.bound - 4.0 * self.e_ref) / 2e-6       # max |float64| over the written elements
        self.ref = self.ref64.to(DEV)
        self.m = R.written(case).to(DEV)

    def errors(self, y):
        diff = torch.nan_to_num((y.double() - self.ref).abs(), nan=float("inf"))
        zero = torch.zeros_like(diff)
        return torch.stack([torch.where(self.m, diff, zero).max(), torch.where(self.m, zero, diff).max()])


@pytest.mark.parametrize("name", [c.name for c in R.CASES])
def test_every_instance_matches_float64(L, name):
    case = R.CASE_BY_NAME[name]
    chk, launch = Checker(case), Launch(L, case)
    stats, ran, wrong_verdict = [], [], []
    try:
        for cfg in CFGS:
            pl = R.plan(case, cfg)
            try:
                y = launch.run(cfg.index + 1)
            except RuntimeError as e:
                if _device_fault(e):
                    raise
                fits = "does not fit" not in str(e)
                if fits or pl.ok:       # an error other than the refusal, or a refusal plan does not share
                    wrong_verdict.append((cfg.name, f"plan {'accepts' if pl.ok else 'refuses: ' + pl.why}", str(e)))
                continue
            if not pl.ok:
                wrong_verdict.append((cfg.name, f"plan refuses: {pl.why}", "the library launched"))
            stats.append(chk.errors(y))
            ran.append(cfg)
        res = torch.stack(stats).cpu().tolist() if stats else []
        torch.cuda.synchronize()
    except RuntimeError as e:
        if _device_fault(e):
            pytest.exit(f"{name}: the device reported a fault ({e}); no further case is launched on it", returncode=3)
        raise
    bad, cells = [], defaultdict(list)
    for cfg, (e_hip, e_out) in zip(ran, res):
        ratio = e_hip / chk.e_ref if chk.e_ref > 0 else float("nan")
        cells[f"{e_hip:.1e}/{ratio:.2f}"].append(cfg.index)
        key = (cfg.kind, cfg.PF, cfg.WK)
        PAIRS[key] += 1
        if ratio == ratio and ratio > WORST.get(key, (0.0, "", 0.0))[0]:
            WORST[key] = (ratio, f"{name} on {cfg.name}", e_hip / chk.top)
        if ratio > 4.0:
            OVER4[case.shape.name] += 1
        if not e_hip <= chk.bound:
            bad.append((cfg.name, "error", e_hip, "bound", chk.bound))
        if e_out != 0.0:
            bad.append((cfg.name, "wrote outside its elements", e_out))
    # every accepted instance, by table index (runs as a-b), under its e_hip / ratio to e_ref: instances that add in the same order print the
    # same figures and share an entry (the last test of the module prints the index -> name legend)
    print(f"\nCONV-TILE {name} e_ref {chk.e_ref:.3e} bound {chk.bound:.3e} instances {len(ran)}: "
          + "  ".join(f"{k}@{_runs(v)}" for k, v in cells.items()))
    assert not wrong_verdict, wrong_verdict[:8]
    assert not bad, bad[:8]
    assert ran, name


def _ok(chk, y):
    e_hip, e_out = chk.errors(y).cpu().tolist()
    return e_hip <= chk.bound and e_out == 0.0


@pytest.mark.parametrize("name,inst,why", [("d1/bn", "4x4x1x4x8k1p2o2", "PF 2: in_shift"), ("d1/style", "4x4x1x4x8k1p0o3t", "kind"),
                                          ("t16/style", "4x4x1x4x8k1p0o3", "kind"), ("g2/place", "4x4x1x4x4k1p0o2d", "not four 3x3 stride-1 dilation groups"),
                                          ("k5/plain", "4x4x1x4x8k1p2o2", "PF 2: more than 9 taps"), ("co7/style", "4x1x1x4x8k1p2o3", "PF 2: cout_g % 4"),
                                          ("deepk/bn", "4x4x1x1x32k4p0o2", "LDS")])
def test_preferred_instance_that_cannot_serve_falls_back(L, name, inst, why):
    """tile_hint = -(i + 1) is a preference: an instance that cannot serve the launch leaves it to the cost model, and so does tile_hint = 0;
    the same instance named (tile_hint = i + 1) is an error"""
    case, cfg = R.CASE_BY_NAME[name], BY_NAME[inst]
    assert R.plan(case, cfg).why == why
    chk, launch = Checker(case), Launch(L, case)
    assert _ok(chk, launch.run(-(cfg.index + 1)))
    assert _ok(chk, launch.run(0))
    with pytest.raises(RuntimeError, match="does not fit"):
        launch.run(cfg.index + 1)
    assert bool((launch.y == R.SENTINEL).all())       # a refused launch writes nothing


def test_preferred_instance_that_can_serve_is_used(L):
    case, cfg = R.CASE_BY_NAME["d1/style"], BY_NAME["4x4x1x4x8k1p2o2"]
    assert R.plan(case, cfg).ok
    assert _ok(Checker(case), Launch(L, case).run(-(cfg.index + 1)))


def test_unsupported_slope_is_refused(L):
    """fill_convk: a constant second slope other than 0.2, 0.01, 0 and 1 has no slot"""
    case = R.CASE_BY_NAME["d1/slope001"]
    launch = Launch(L, case, slope2=0.3)
    for hint in (0, BY_NAME["4x4x1x4x8k1p0o3"].index + 1):
        with pytest.raises(RuntimeError, match=r"unsupported act2 slope 0\.3"):
            launch.run(hint)
    assert bool((launch.y == R.SENTINEL).all())


def test_pf2_refuses_a_misaligned_weight(L):
    """the LDS-DMA instances read whole float4 weight rows: named on a weight 4 bytes past a 16-byte boundary they refuse, every other
    staging serves it on the scalar path"""
    case = R.CASE_BY_NAME["d1/style"]
    chk, launch = Checker(case), Launch(L, case, w_off=4)
    for cfg in CFGS:
        if cfg.kind != "plain":
            continue
        if cfg.PF == 2:
            with pytest.raises(RuntimeError, match="does not fit"):
                launch.run(cfg.index + 1)
    assert _ok(chk, launch.run(BY_NAME["4x4x1x4x8k1p0o3"].index + 1))
    assert _ok(chk, launch.run(-(BY_NAME["4x4x1x4x8k1p2o2"].index + 1)))


def test_zz_worst_ratio_per_kind_staging_and_split(L):
    """every (kind, PF, WK) of the instance table has run; prints the worst e_hip / e_ref of each (the figures of the module docstring),
    with that pair's error relative to max |float64|, and the shapes with pairs above 4 e_ref (inside the bound by its additive term)"""
    print("\nCONV-TILE-LEGEND " + " ".join(f"{c.index}={c.name}" for c in CFGS))
    for key in sorted(WORST):
        r, pair, rel = WORST[key]
        print(f"CONV-TILE-WORST kind {key[0]:5s} PF {key[1]} WK {key[2]}  {r:.2f}  {pair}  (e_hip = {rel:.2e} max|f64|; {PAIRS[key]} pairs)")
    print(f"CONV-TILE-OVER4 {sum(OVER4.values())} of {sum(PAIRS.values())} pairs: " + " ".join(f"{k}={v}" for k, v in sorted(OVER4.items())))
    assert PAIRS, "this test closes a run of the whole module"
    assert set(PAIRS) == set(WORST) == {(c.kind, c.PF, c.WK) for c in CFGS}
    assert sum(PAIRS.values()) == sum(1 for c in R.CASES for cfg in CFGS if R.plan(c, cfg).ok)      # every accepted pair was measured
    for key, (r, pair, rel) in WORST.items():
        assert 0.0 < r < float("inf") and rel < 2e-6 + 4.0 / r * rel * 1.0000001, (key, r, pair)      # (the bound, restated on the worst pair)
