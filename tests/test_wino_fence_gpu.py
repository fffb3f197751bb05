"""Conditioning fence for the Winograd conv kernels: every fp32 kernel that can run as Winograd -- the F(2x2) forms 1 / 2 / 3, the F(4x4) pair,
the fused F(4x4) kernel with its dilated bodies -- and the direct kernel as the control, each named through conv2d_packed, on operands
where F(4x4) loses its margin: a large DC part, post-activation maps, style scales over four decades with the true demodulation, a small
output under a large input.

The bound is NOT the output range.  A kernel is measured against float64 F.conv2d with two numbers (tests/wino_ref.py: E = max|y - ref|,
S = the same in units of 2^-24 (|x s| (*) |w|)), and so is a plain float32 model of its own algorithm on the same operands, with the same
points, the same dilation and the style scale folded where the kernel folds it (the control: F.conv2d in float32 on the CPU).  Then

    E_kernel <= 3 E_model   and   S_kernel <= 3 S_model.

3 = the 2x the model may move across its own evaluation orders (tests/test_wino_ref.py asserts that for every row used here) x 1.5 for
FMA contraction and the kernels' factoring of the dyadic constants.  No kernel is compared with another kernel.  `pytest -m gpu`."""
import numpy as np
import pytest
import torch

import wino_ref as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
FACTOR = 3.0
FAMILY_RAN = {"direct": "direct", "f2-form1": "wino", "f2-form2": "wino", "f2-form3": "wino", "f4-pair": "wino4", "f4-fused": "wino4f"}


@pytest.fixture(scope="module")
def H():
    from vspbfr_amd import hip_ops
    return hip_ops


def dev(t):
    return None if t is None else t.to(DEV).contiguous()


_operands, _models = {}, {}


def _shape_key(case, family, epi):
    return (case.B, case.Cin, case.Cg, case.H, case.W, case.dils, family, epi)


def _reference(case, family, epi):
    """operands, float64 reference and unit of a row: computed once, shared by every kernel on that shape, never written to"""
    k = _shape_key(case, family, epi)
    if k not in _operands:
        ops = R.operands(case, family, epi)
        _operands[k] = (ops,) + R.reference(case, ops)
    return _operands[k]


def _model(case, family, epi):
    """(E, S) of the float32 model of the kernel's algorithm (the F(2x2) forms share one)"""
    k = (R.points_of(case.kernel) and case.kernel[:2], R.fold_of(case.kernel)) + _shape_key(case, family, epi)
    if k not in _models:
        ops, ref, unit = _reference(case, family, epi)
        _models[k] = R.errors(R.model(case, ops), ref, unit)
    return _models[k]


def run_kernel(H, case, ops):
    """the launch on the kernel the case names; the profiler's record says which family ran it (the pair falls back silently)"""
    c = case
    wp = torch.stack([H.pack_weight(dev(w))[0] for w in ops["ws"]]).contiguous()
    pc = H.PackedConv(wp, len(c.dils), c.Cg, c.Cin, 3, 3, 1, c.dils, c.dils)
    kw = dict(in_scale=dev(ops["in_scale"]), out_scale=dev(ops["out_scale"]))
    if ops["bias"] is not None:
        kw.update(noise=dev(ops["noise"]), noise_w=dev(ops["noise_w"]), act2=1, bias2=dev(ops["bias"]))
    name = {"direct": dict(winograd=False, bf16=False), "f4-pair": dict(winograd=4), "f4-fused": dict(winograd=5)}.get(c.kernel)
    if name is None:
        name = dict(winograd=True, wino_form=int(c.kernel[-1]))
    prof = H.ConvProfiler()
    H.PROFILER = prof
    try:
        y = H.conv2d_packed(dev(ops["x"]), pc, **name, **kw)
    finally:
        H.PROFILER = None
    ran = [r[3][7] for r in prof.records]
    assert ran == [FAMILY_RAN[c.kernel]], (c.id, ran)
    return y.cpu().numpy()


def measure(H, case, family, epi=False):
    """One row of the fence: the kernel's and the model's E and S against float64, and both ratios."""
    ops, ref, unit = _reference(case, family, epi)
    Ek, Sk = R.errors(run_kernel(H, case, ops), ref, unit)
    Em, Sm = _model(case, family, epi)
    return dict(kernel=case.kernel, shape=[case.B, case.Cin, len(case.dils) * case.Cg, case.H, case.W], dilations=list(case.dils), family=family,
                epilogue=epi, E_kernel=Ek, E_model=Em, S_kernel=Sk, S_model=Sm, E_ratio=Ek / Em, S_ratio=Sk / Sm,
                ref_max=float(np.abs(ref).max()), E_kernel_of_range=Ek / float(np.abs(ref).max()))


ROWS = [(c, f, False) for c in R.CASES for f in R.FAMILIES] + [(c, f, True) for c in R.EPILOGUE_CASES for f in R.EPILOGUE_FAMILIES]


@pytest.mark.parametrize("case,family,epi", ROWS, ids=[f"{c.id}-{f}{'-epi' if e else ''}" for c, f, e in ROWS])
def test_fence(H, case, family, epi):
    r = measure(H, case, family, epi)
    msg = (f"{case.id} {family}{' + epilogue' if epi else ''}: E kernel {r['E_kernel']:.3e} / model {r['E_model']:.3e} = {r['E_ratio']:.2f}x, "
           f"S kernel {r['S_kernel']:.2f} / model {r['S_model']:.2f} = {r['S_ratio']:.2f}x (bound {FACTOR:g}x)")
    print(msg)
    assert r["E_kernel"] <= FACTOR * r["E_model"] and r["S_kernel"] <= FACTOR * r["S_model"], msg
