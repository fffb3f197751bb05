"""The float32 model of the Winograd kernels (tests/wino_ref.py) on the CPU: exact in float64, the kernels' documented matrices, and the
margin condition the conditioning fence (tests/test_wino_fence_gpu.py) rests on -- the model's own error moves by at most 2x across its
evaluation orders on every (launch, family) row the fence uses."""
import numpy as np
import pytest
import torch

import wino_ref as R

torch.set_grad_enabled(False)


def test_matrices_are_the_documented_ones():
    AT, G, BT = R.mats(**R.F4)
    Gm = np.array([[64 / 81, 0, 0], [-128 / 243, -32 / 81, -8 / 27], [-128 / 243, 32 / 81, -8 / 27], [32 / 243, 16 / 81, 8 / 27],
                   [32 / 243, -16 / 81, 8 / 27], [0, 0, 1]])          # tests/test_wino4f.py::test_winograd4f_weight_layout
    assert np.abs(G - Gm).max() < 1e-15
    assert AT.shape == (4, 6) and BT.shape == (6, 6)
    # conv_wino4f.hip's constants: a^2 b^2, -(a^2 + b^2), -b^2, -a^2, a, b -- all dyadic, exact in float32
    assert BT[0].tolist() == [1.265625, 0.0, -2.8125, 0.0, 1.0, 0.0]
    assert BT[1].tolist() == [0.0, -0.75 * 2.25, -2.25, 0.75, 1.0, 0.0]
    assert BT[3].tolist() == [0.0, -1.5 * 0.5625, -0.5625, 1.5, 1.0, 0.0]
    assert np.array_equal(BT.astype(np.float32).astype(np.float64), BT)
    AT, G, BT = R.mats(**R.F2)
    assert np.array_equal(G, np.array([[1, 0, 0], [.5, .5, .5], [.5, -.5, .5], [0, 0, 1]]))        # include/vspbfr_hip.h
    assert np.array_equal(AT, np.array([[1, 1, 1, 0], [0, 1, -1, 1]]))
    assert np.array_equal(BT, np.array([[1, 0, -1, 0], [0, 1, 1, 0], [0, -1, 1, 0], [0, -1, 0, 1]]))


@pytest.mark.parametrize("pts", [R.F2, R.F4], ids=["F2", "F4"])
@pytest.mark.parametrize("shape,d", [((2, 8, 6, 16, 24), 1), ((1, 5, 7, 13, 18), 1), ((1, 8, 4, 16, 16), 2), ((1, 6, 4, 19, 22), 2),
                                     ((1, 4, 4, 32, 16), 4), ((1, 4, 3, 32, 37), 8)])
def test_model_is_exact_in_float64(pts, shape, d):
    """dense and ragged maps (partial tiles, polyphase sub-images of unequal size), every order, both folds of the style scale"""
    B, Cin, Cout, H, W = shape
    g_ = torch.Generator().manual_seed(H * 31 + W + d)
    x, w = torch.randn(B, Cin, H, W, generator=g_).double().numpy(), torch.randn(Cout, Cin, 3, 3, generator=g_).double().numpy()
    s = (torch.rand(B, Cin, generator=g_) + 0.5).double().numpy()
    ref = R.conv64(x, w, d)
    for order in R.ORDERS:
        assert np.abs(R.wino_conv(x, w, pts, np.float64, d, order=order) - ref).max() < 1e-12, order
    refs = R.conv64(x * s[:, :, None, None], w, d)
    for fold in ("x", "U"):
        assert np.abs(R.wino_conv(x, w, pts, np.float64, d, in_scale=s, fold=fold) - refs).max() < 1e-12, fold


def test_float32_model_cost_ordering():
    """64 -> 32 at 32^2, x ~ N(0,1): direct fp32 < F(2x2) < F(4x4), all within a few 1e-6 (the F(4x4) model: ~6e-6, 1.2e-6 of the range)"""
    g_ = torch.Generator().manual_seed(0)
    x, w = torch.randn(1, 64, 32, 32, generator=g_).numpy(), (torch.randn(32, 64, 3, 3, generator=g_) / 24).numpy()
    ref = R.conv64(x, w)
    e = [np.abs(y - ref).max() for y in (R.direct_conv_f32(x, w), R.wino_conv(x, w, R.F2), R.wino_conv(x, w, R.F4))]
    assert e[0] < 4e-6 and e[1] < 4e-6 and e[1] < e[2] < 1.5e-5, e


def test_chain_control_is_a_convolution():
    """the direct kernel's "chain" variant: the same convolution as float64 F.conv2d to float32 accuracy, dilated and ragged, and dearer than
    the CPU's blocked float32 form at 128 input channels (what control_of rests on)"""
    g_ = torch.Generator().manual_seed(1)
    x, w = torch.randn(1, 128, 13, 18, generator=g_).numpy(), (torch.randn(8, 128, 3, 3, generator=g_) / 34).numpy()
    for d in (1, 2):
        ref = R.conv64(x, w, d)
        e_chain, e_cpu = np.abs(R.direct_conv_chain(x, w, d) - ref).max(), np.abs(R.direct_conv_f32(x, w, d) - ref).max()
        assert e_chain < 1e-5 and e_cpu < e_chain, (d, e_chain, e_cpu)


ROWS = [(c, f, False) for c in R.WINO_CASES for f in R.FAMILIES] + [(c, f, True) for c in R.EPILOGUE_CASES if c.kernel != "direct"
                                                                      for f in R.EPILOGUE_FAMILIES]
# the F(2x2) forms share a model: one row per (points, fold, shape, family)
_seen = {}
for c, f, e in ROWS:
    _seen.setdefault((c.kernel[:2], R.fold_of(c.kernel), c.B, c.Cin, c.Cg, c.H, c.W, c.dils, f, e), (c, f, e))
ROWS = list(_seen.values())


@pytest.mark.parametrize("case,family,epi", ROWS, ids=[f"{c.id}-{f}{'-epi' if e else ''}" for c, f, e in ROWS])
def test_model_spread_across_orders(case, family, epi):
    """The margin condition of the fence's factor 3: E and S of the float32 model differ by at most 2x between any two of its orders
    (three channel permutations x rows / columns first x sequential / bulk accumulation), on the very operands of the fence row."""
    ops = R.operands(case, family, epi)
    ref, unit = R.reference(case, ops)
    es = [R.errors(R.model(case, ops, np.float32, o), ref, unit) for o in R.ORDERS]
    E, S = [e for e, _ in es], [s for _, s in es]
    print(f"{case.id} {family}: E {min(E):.3e} .. {max(E):.3e} ({max(E) / min(E):.2f}x)  S {min(S):.3f} .. {max(S):.3f} ({max(S) / min(S):.2f}x)")
    assert max(E) <= 2.0 * min(E) and max(S) <= 2.0 * min(S), (E, S)
