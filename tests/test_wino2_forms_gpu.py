"""The three fp32 F(2x2,3x3) kernels that share conv_wino2.h -- task list (conv_wino.hip, wino_form = 1), row owner (conv_wino_ro.hip) and
row owner for dilation groups (conv_wino_rod.hip, both wino_form = 2) -- each NAMED, against float64 F.conv2d plus the operand chain.  A named
form that does not serve the launch raises, so the name proves which kernel ran.  Shapes are the smallest at which each shared piece (work
order decode, epilogue store forms, staging) takes another path; operands and bound are those of test_conv2d_winograd (tests/test_hip_ops.py).
`pytest -m gpu`."""
import math

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"

# (form, B, Cin, channels per group, H, W, dilations, output): output "" = a tensor of its own, "pad" = into (B, C, H + 2, W + 2), "window" = into
# the channel window y_coff = 3 of a wider tensor (both prefilled with 7.0)
ROWS = [
    # task list
    (1, 1, 8, 12, 7, 5, (1,), ""),               # <1,1>: two 64-tile halves, ragged channel block, odd width (scalar stores)
    (1, 2, 20, 24, 13, 29, (1,), ""),            # <2,1>, Cin % 8 != 0
    (1, 2, 20, 40, 20, 36, (1,), ""),            # <4,1>: two channel blocks per epilogue pass, pairs, 40 of 64 channels
    (1, 2, 16, 8, 19, 19, (1, 2, 4, 8), ""),     # dilated, region-major order, rows not divisible by d
    (1, 1, 24, 24, 24, 24, (1, 2, 4, 8), ""),    # dilated, region-major order
    (1, 1, 16, 40, 36, 32, (2,), ""),            # one dilated group above 1024 pixels: dispatch order
    (1, 1, 16, 40, 16, 16, (4,), ""),            # order 1
    # row owner
    (2, 2, 16, 24, 12, 20, (1,), ""),            # <2,1,8>, quads
    (2, 1, 24, 40, 12, 20, (1,), ""),            # <4,1,8>
    (2, 2, 16, 64, 10, 40, (1,), ""),            # <4,1,16>, ragged tile column
    (2, 2, 16, 24, 12, 20, (1,), "pad"),         # y_w != OW: the shared pairs path
    (2, 2, 16, 24, 12, 20, (1,), "window"),      # quads into a channel window
    # row owner, dilation groups
    (2, 2, 16, 24, 16, 24, (1, 2, 4, 8), ""),    # region-major
    (2, 1, 16, 40, 20, 20, (1, 2), ""),
    (2, 1, 16, 40, 36, 32, (4,), ""),            # one group, dispatch order
    (2, 1, 16, 24, 16, 16, (8,), ""),            # order 1, sub-images of two rows
]
WAYS = ("plain", "styled", "bn")
CASES = [(i, way) for i in range(len(ROWS)) for way in WAYS if way != "bn" or ROWS[i][6] == (1,)]


def case_id(case):
    form, B, Cin, Cg, Hh, Ww, dils, outv = ROWS[case[0]]
    return f"f{form}-{B}x{Cin}x{Cg}x{Hh}x{Ww}-d{''.join(map(str, dils))}{'-' + outv if outv else ''}-{case[1]}"


def dev(t):
    return t.to(DEV).contiguous()


@pytest.fixture(scope="module")
def H():
    from vspbfr_amd import hip_ops
    return hip_ops


def close(a, b, rtol, atol, what=""):
    a, b = a.detach().cpu().double().numpy(), b.detach().cpu().double().numpy()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.isfinite(a).all(), f"{what}: non-finite output"
    err = np.abs(a - b).max()
    tol = atol + rtol * np.abs(b).max()
    print(f"{what}: max|d|={err:.3e} tol={tol:.3e}")
    assert err <= tol, f"{what}: max|d|={err:.3e} tol={tol:.3e}"


def run_case(H, case):
    """One launch of the named form -> (the whole output tensor, its computed part, the float64 reference of that part).  Everything is drawn
    from one generator seeded by the case, so two processes compute the same launch."""
    i, way = case
    form, B, Cin, Cg, Hh, Ww, dils, outv = ROWS[i]
    g_ = torch.Generator().manual_seed(1000 + 3 * i + WAYS.index(way))
    G, C = len(dils), len(dils) * Cg
    x = torch.randn(B, Cin, Hh, Ww, generator=g_)
    ws = [torch.randn(Cg, Cin, 3, 3, generator=g_) / math.sqrt(Cin * 9) for _ in dils]
    wp = torch.stack([H.pack_weight(dev(w_))[0] for w_ in ws]).contiguous()
    pc = H.PackedConv(wp, G, Cg, Cin, 3, 3, 1, dils, dils)
    yh, yw = (Hh + 2, Ww + 2) if outv == "pad" else (Hh, Ww)
    kw, xd, post = {}, x.double(), lambda y: y
    if way == "styled":   # the whole StyledConv chain
        s_in, demod, bias = torch.rand(B, Cin, generator=g_) + 0.5, torch.rand(B, C, generator=g_) + 0.5, torch.randn(C, generator=g_)
        nz, nw = torch.randn(B, 1, Hh, Ww, generator=g_), torch.tensor([0.7])
        r1, r2 = torch.randn(B, C, yh, yw, generator=g_), torch.randn(B, C, yh, yw, generator=g_)
        kw = dict(in_scale=dev(s_in), out_scale=dev(demod), noise=dev(nz), noise_w=dev(nw), act2=1, bias2=dev(bias), res1=dev(r1), res2=dev(r2))
        xd = xd * s_in.double().view(B, Cin, 1, 1)

        def post(y):
            y = y * demod.double().view(B, C, 1, 1) + nz.double() * nw.double()
            y = F.leaky_relu(y + bias.double().view(1, -1, 1, 1), 0.2) * math.sqrt(2)
            return y + r1.double()[:, :, :Hh, :Ww] + r2.double()[:, :, :Hh, :Ww]
    elif way == "bn":     # folded BatchNorm input (zero padding AFTER the affine map) and PReLU
        a, sh, pr = torch.rand(Cin, generator=g_) + 0.5, torch.randn(Cin, generator=g_), torch.rand(C, generator=g_) * 0.3
        kw = dict(in_scale=dev(a), in_scale_per_sample=False, in_shift=dev(sh), act2=2, prelu=dev(pr))
        xd = xd * a.double().view(1, -1, 1, 1) + sh.double().view(1, -1, 1, 1)

        def post(y):
            return F.prelu(y, pr.double())
    ref = post(torch.cat([F.conv2d(xd, w_.double(), padding=d, dilation=d) for w_, d in zip(ws, dils)], dim=1))
    if outv:
        out = torch.full((B, C + 5 if outv == "window" else C, yh, yw), 7.0, device=DEV)
        H.conv2d_packed(dev(x), pc, out=out, y_coff=3 if outv == "window" else 0, winograd=True, wino_form=form, **kw)
    else:
        out = H.conv2d_packed(dev(x), pc, winograd=True, wino_form=form, **kw)
    c0 = 3 if outv == "window" else 0
    return out, out[:, c0:c0 + C, :Hh, :Ww], ref


@pytest.mark.parametrize("case", CASES, ids=case_id)
def test_wino2_named_form_vs_fp64(H, case):
    out, y, ref = run_case(H, case)
    close(y, ref, 5e-5, 5e-5, case_id(case))
    outv = ROWS[case[0]][7]
    if outv:   # nothing outside the computed part was written
        C, Hh, Ww = y.shape[1], y.shape[2], y.shape[3]
        c0 = 3 if outv == "window" else 0
        keep = torch.ones_like(out, dtype=torch.bool)
        keep[:, c0:c0 + C, :Hh, :Ww] = False
        assert int(keep.sum()) > 0 and bool((out[keep] == 7.0).all())
