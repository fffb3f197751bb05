"""GPU checks of the 33 pipelined instances of conv_pipe_kernel (csrc/conv_pipe.hip: the `...k1p3...` names -- plain, `t`, `d`, `fd`, `a`) and of
the five instantiations of conv_smallmap_kernel (csrc/conv_smallmap.hip), the two families tests/test_conv_tile_forms_gpu.py leaves out,
against the float64 restatement of tests/conv_tile_ref.py under the case tables of tests/conv_pipe_ref.py.  tests/test_conv_pipe_ref.py proves
on the CPU that those tables reach every instance in every mode its kind serves, every nchunk class of the fixed-geometry interval, the three
variants of workgroup order 2 and every small-map instantiation, and that wrong variants of the restatement miss this bound on these inputs.

Every case of P_CASES is launched on EVERY p3 instance by name (tile_hint = index + 1) and every case of S_CASES with `smallmap` named, through
the C entry vsp_conv2d_f32 with a parameter block built here.  For each pair the library's verdict must equal conv_pipe_ref.plan's /
smallmap_form's: the refusal (code VSP_EINVAL, "configuration <name> does not fit") exactly where the restated rule refuses, otherwise

    max |HIP - float64| <= 4 e_ref + 2e-6 max |float64|        (conv_tile_ref.bound)

with e_ref the error of the same restatement in float32, the sentinel intact in every element the launch must not write, and the same bits
from a second run (the kernels have no atomics).  Under -s every case prints its e_hip and e_hip / e_ref per instance, and the last test the
worst ratio per (kind, CK) and per small-map instantiation.  The recorded run is profiles/conv_pipe_forms_gputest.log."""
from collections import defaultdict

import pytest
import torch

import conv_pipe_ref as P
import conv_tile_ref as R
from test_conv_tile_forms_gpu import Checker, Launch, _device_fault, _runs

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
CFGS = P.configs()
BY_NAME = {c.name: c for c in CFGS}
P_NAMES = [c.name for c in P.P_CASES]
S_NAMES = [c.name for c in P.S_CASES]
EINVAL = -1
WORST = {}                    # (kind, CK) or ("smallmap", instantiation) -> (ratio, pair, e_hip / max |float64|)
PAIRS = defaultdict(int)
REFUSED = defaultdict(int)


@pytest.fixture(scope="module")
def L():
    from vspbfr_amd import _lib
    return _lib


class QLaunch(Launch):
    """Launch with the dil_by_input_quarter flag of the case; twice(hint) -> (y, whether a second run changed a bit)"""

    def __init__(self, L, case, **kw):
        super().__init__(L, case, **kw)
        self.p.dil_by_input_quarter = 1 if case.quarter else 0

    def twice(self, hint):
        first = self.run(hint).clone()
        y = self.run(hint)
        return y, (first.view(torch.int32) != y.view(torch.int32)).any()


def _release(case):
    if case.group in P.HEAVY or case.G > 100:
        R.inputs.cache_clear()


def _sweep(name, case, launch, chk, targets):
    """targets: (label, index, key, ok, message part a refusal must carry).  -> the printed cells; asserts verdicts, bound, sentinel, bits"""
    stats, ran, wrong_verdict, touched = [], [], [], []
    try:
        for label, index, key, ok, part in targets:
            try:
                y, changed = launch.twice(index + 1)
            except RuntimeError as e:
                if _device_fault(e):
                    raise
                shared = f"(code {EINVAL})" in str(e) and part in str(e)
                if ok or not shared:
                    wrong_verdict.append((label, "the restatement " + ("accepts" if ok else "refuses with " + part), str(e)))
                REFUSED[key] += 1
                touched.append((launch.y != R.SENTINEL).any())      # a refused launch writes nothing
                continue
            if not ok:
                wrong_verdict.append((label, "the restatement refuses", "the library launched"))
            stats.append(torch.cat([chk.errors(y), changed.double()[None]]))
            ran.append((label, index, key))
        res = torch.stack(stats).cpu().tolist() if stats else []
        wrote = bool(torch.stack(touched).any()) if touched else False
        torch.cuda.synchronize()
    except RuntimeError as e:
        if _device_fault(e):
            pytest.exit(f"{name}: the device reported a fault ({e}); no further case is launched on it", returncode=3)
        raise
    bad, cells = [], defaultdict(list)
    for (label, index, key), (e_hip, e_out, changed) in zip(ran, res):
        ratio = e_hip / chk.e_ref
        cells[f"{e_hip:.1e}/{ratio:.2f}"].append(index)
        PAIRS[key] += 1
        if ratio > WORST.get(key, (-1.0, "", 0.0))[0]:
            WORST[key] = (ratio, f"{name} on {label}", e_hip / chk.top)
        if not e_hip <= chk.bound:
            bad.append((label, "error", e_hip, "bound", chk.bound))
        if e_out != 0.0:
            bad.append((label, "wrote outside its elements", e_out))
        if changed:
            bad.append((label, "a second run gave other bits"))
    assert not wrong_verdict, wrong_verdict[:8]
    assert not bad, bad[:8]
    assert not wrote, f"{name}: a refused launch wrote into y"
    return cells, len(ran)


@pytest.mark.parametrize("name", P_NAMES)
def test_every_p3_instance_matches_float64(L, name):
    case = P.CASE_BY_NAME[name]
    chk, launch = Checker(case), QLaunch(L, case)
    targets = [(cfg.name, cfg.index, (cfg.kind, cfg.CK), P.plan(case, cfg).ok, f"configuration {cfg.name} does not fit") for cfg in CFGS]
    cells, n = _sweep(name, case, launch, chk, targets)
    print(f"\nCONV-PIPE {name} e_ref {chk.e_ref:.3e} bound {chk.bound:.3e} instances {n}: " + "  ".join(f"{k}@{_runs(v)}" for k, v in cells.items()))
    # a case every instance refuses is in the table for that refusal: an input shift (the chain), or a shape named in REFUSED_BY_RULE
    assert (n == 0) == bool(R.operands(case)["in_shift"] or case.shape.name in P.REFUSED_BY_RULE), name
    _release(case)


@pytest.mark.parametrize("name", S_NAMES)
def test_smallmap_matches_float64(L, name):
    case = P.CASE_BY_NAME[name]
    form = P.smallmap_form(case)
    chk, launch = Checker(case), QLaunch(L, case)
    key = ("smallmap", form.inst if form.ok else form.why)
    cells, n = _sweep(name, case, launch, chk, [(form.inst or "smallmap", P.smallmap_index(), key, form.ok, P.S_REFUSALS.get(form.why, ""))])
    print(f"\nCONV-SMALLMAP {name} {form.inst if form.ok else 'refused: ' + form.why} grid {form.grid} e_ref {chk.e_ref:.3e} bound {chk.bound:.3e}: "
          + "  ".join(cells))
    assert n == (1 if form.ok else 0)
    if not form.ok:
        assert bool((launch.y == R.SENTINEL).all())       # a refused launch writes nothing
    _release(case)


def _ok(chk, y):
    e_hip, e_out = chk.errors(y).cpu().tolist()
    return e_hip <= chk.bound and e_out == 0.0


@pytest.mark.parametrize("name,inst,why", [("d1/bn", "2x4x2x4x8k1p3o1r18", "in_shift"), ("d1/style", "2x16x2x4x8k1p3o1r9t", "kind: transposed"),
                                          ("g4odd/style", "4x2x1x8x8k1p3o1r16fd", "fixed geometry: dilations are not 1, 2, 4, 8"),
                                          ("smn8193/style", "smallmap", "positions")])
def test_preferred_instance_that_cannot_serve_falls_back(L, name, inst, why):
    """tile_hint = -(i + 1) is a preference: an instance that cannot serve the launch leaves it to the cost model; named, it is an error"""
    case = P.CASE_BY_NAME[name]
    if inst == "smallmap":
        index = P.smallmap_index()
        assert P.smallmap_form(case).why == why
    else:
        index = BY_NAME[inst].index
        assert P.plan(case, BY_NAME[inst]).why == why
    chk, launch = Checker(case), QLaunch(L, case)
    assert _ok(chk, launch.run(-(index + 1)))
    with pytest.raises(RuntimeError, match="does not fit"):
        launch.run(index + 1)
    assert bool((launch.y == R.SENTINEL).all())


@pytest.mark.parametrize("shape", ["a16", "a32", "a64", "a128", "a64d"])
def test_data_gradient_without_a_name_takes_the_first_instance_that_fits(L, shape):
    """tile_hint = 0 under dil_by_input_quarter: the `a` instances in table order; the result is that of the first one plan accepts, bit for bit"""
    case = P.CASE_BY_NAME[f"{shape}/style"]
    first = next(c for c in CFGS if c.kind == "a" and P.plan(case, c).ok)
    chk, launch = Checker(case), QLaunch(L, case)
    y0 = launch.run(0).clone()
    assert _ok(chk, y0) and torch.equal(y0, launch.run(first.index + 1))


def test_zz_worst_ratio_per_kind_and_chunk(L):
    """closes a run of the whole module: every accepted pair of the tables was measured; prints the worst e_hip / e_ref per (kind, CK) and per
    small-map instantiation with that pair's error relative to max |float64|"""
    print("\nCONV-PIPE-LEGEND " + " ".join(f"{c.index}={c.name}" for c in CFGS) + f" {P.smallmap_index()}=smallmap")
    for key in sorted(WORST):
        r, pair, rel = WORST[key]
        print(f"CONV-PIPE-WORST {key[0]:8s} {'CK ' + str(key[1]) if key[0] != 'smallmap' else key[1]:5s}  {r:.2f}  {pair}  (e_hip = {rel:.2e} max|f64|; {PAIRS[key]} pairs)")
    acc_p, acc_s = sum(v for k, v in PAIRS.items() if k[0] != "smallmap"), sum(v for k, v in PAIRS.items() if k[0] == "smallmap")
    ref_p, ref_s = sum(v for k, v in REFUSED.items() if k[0] != "smallmap"), sum(v for k, v in REFUSED.items() if k[0] == "smallmap")
    print(f"CONV-PIPE-PAIRS p3 accepted {acc_p} refused {ref_p}; smallmap accepted {acc_s} refused {ref_s}")
    assert PAIRS, "this test closes a run of the whole module"
    assert {k for k in PAIRS if k[0] != "smallmap"} == {(c.kind, c.CK) for c in CFGS}
    assert {k[1] for k in PAIRS if k[0] == "smallmap"} == set(P.S_INSTS)
    assert acc_p == sum(1 for c in P.P_CASES for cfg in CFGS if P.plan(c, cfg).ok) and acc_p + ref_p == len(P.P_CASES) * len(CFGS)
    assert acc_s == sum(1 for c in P.S_CASES if P.smallmap_form(c).ok) and acc_s + ref_s == len(P.S_CASES)
