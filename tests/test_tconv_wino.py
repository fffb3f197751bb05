"""The stride-2 transposed 3x3 conv as a fused Winograd F(2x2,2x2) phase kernel (vspbfr_amd/csrc/conv_tconv_wino.hip,
vsp_conv_transpose2d_s2_wino_f32): 25 products per tile of 2 x 2 positions where the direct form takes 36.

CPU: a float64 restatement of the algebra (weight transform, input transform, output transform, phase interleave, ragged edges) against
F.conv_transpose2d, hip_ops' host restatement of the weight transform against it, the eligibility mirror and the entry's refusals.

GPU (-m gpu): every case against F.conv_transpose2d in float64 on the CPU.  Bound per case: e_new <= 2 e_direct + 1e-6 max|ref|, with
e_direct the maximum error of the direct launch (hip_ops.TCONV_WINO = False) on the same operands against the same reference: the factor 2
allows for the extra additions of three exact transforms (every constant is 0 or +-1), the floor covers a direct kernel that happens to
be exact.  Both errors are printed per case (`pytest -s`); profiles/tconv_wino_gputest.log is such a run on an MI355X.

The `..._into` case: a 33 x 33 input has a 67 x 67 output, so the destinations are 67^2 (exact) and 68^2 (one zeroed row / column more); a
66^2 destination cannot hold it and is refused by the wrapper whatever the kernel."""
import ctypes as C
import math

import pytest
import torch
import torch.nn.functional as F

torch.set_grad_enabled(False)
SQRT2 = math.sqrt(2.0)


@pytest.fixture(scope="module")
def H():
    from vspbfr_amd import hip_ops
    return hip_ops


# ------------------------------------------------------------------------------------------------ the algebra, float64
G2 = torch.tensor([[0., 0., 1.], [1., 0., 1.], [1., 0., 0.]], dtype=torch.float64)   # g_0 = tap 2, g_1 = tap 2 + tap 0, g_2 = tap 0


def weight_transform(w):
    """w (Cout, Cin, 3, 3) float64 -> the 16 distinct transformed weights (16, Cin, Cout)"""
    wt = w.permute(2, 3, 1, 0)                                              # [ky][kx][ci][co]
    u00 = torch.einsum("ik,jl,klco->ijco", G2, G2, wt).reshape(9, *wt.shape[2:])
    u01 = torch.einsum("ik,kco->ico", G2, wt[:, 1])
    u10 = torch.einsum("jl,lco->jco", G2, wt[1])
    return torch.cat([u00, u01, u10, wt[1, 1][None]], 0)


PRODUCTS = []   # the weight operand of every product the restatement forms (test_product_count)


def tconv_wino_restatement(x, w):
    """conv_transpose2d(x, w^T, stride 2) through the 25-product form, float64: (B, Cin, H, W), (Cout, Cin, 3, 3) -> (B, Cout, 2H+1, 2W+1)"""
    B, Cin, Hh, Ww = x.shape
    Cout = w.shape[0]
    U = weight_transform(w)
    nty, ntx = (Hh + 2) // 2, (Ww + 2) // 2
    xp = torch.zeros(B, Cin, 2 * nty + 1, 2 * ntx + 1, dtype=torch.float64)   # xp[r, s] = x[r - 1, s - 1]: the implicit padding of the grid
    xp[:, :, 1:Hh + 1, 1:Ww + 1] = x
    y = torch.zeros(B, Cout, 4 * nty, 4 * ntx, dtype=torch.float64)
    def mm(u, v):                                                           # one product, summed over the input channels
        PRODUCTS.append(u.data_ptr())
        return torch.einsum("co,bc->bo", u, v)
    for ty in range(nty):
        for tx in range(ntx):
            d = xp[:, :, 2 * ty:2 * ty + 3, 2 * tx:2 * tx + 3]               # d[r][s] = x[m0 - 1 + r, c0 - 1 + s]
            A = torch.stack([d[:, :, 0] - d[:, :, 1], d[:, :, 1], d[:, :, 2] - d[:, :, 1]], 2)             # y transform: [b, ci, i, s]
            V = torch.stack([A[..., 0] - A[..., 1], A[..., 1], A[..., 2] - A[..., 1]], 3)                  # phase (0,0): [b, ci, i, j]
            R = torch.stack([d[..., 0] - d[..., 1], d[..., 1], d[..., 2] - d[..., 1]], 3)[:, :, 1:]        # phase (1,0): [b, ci, a, j]
            M00 = [[mm(U[3 * i + j], V[:, :, i, j]) for j in range(3)] for i in range(3)]
            M01 = [[mm(U[9 + i], A[:, :, i, 1 + c]) for c in range(2)] for i in range(3)]
            M10 = [[mm(U[12 + j], R[:, :, a, j]) for j in range(3)] for a in range(2)]
            M11 = [[mm(U[15], d[:, :, 1 + a, 1 + c]) for c in range(2)] for a in range(2)]
            for a in range(2):
                for c in range(2):
                    oy, ox = 4 * ty + 2 * a, 4 * tx + 2 * c
                    y[:, :, oy, ox] = M00[a][c] + M00[a][c + 1] + M00[a + 1][c] + M00[a + 1][c + 1]
                    y[:, :, oy, ox + 1] = M01[a][c] + M01[a + 1][c]
                    y[:, :, oy + 1, ox] = M10[a][c] + M10[a][c + 1]
                    y[:, :, oy + 1, ox + 1] = M11[a][c]
    return y[:, :, :2 * Hh + 1, :2 * Ww + 1]


@pytest.mark.parametrize("B,Cin,Cout,Hh,Ww", [(2, 3, 5, 4, 4), (1, 2, 3, 5, 7), (1, 4, 2, 1, 6)])
def test_algebra_matches_conv_transpose2d_float64(B, Cin, Cout, Hh, Ww):
    g = torch.Generator().manual_seed(7)
    x = torch.randn(B, Cin, Hh, Ww, generator=g, dtype=torch.float64)
    w = torch.randn(Cout, Cin, 3, 3, generator=g, dtype=torch.float64)
    ref = F.conv_transpose2d(x, w.transpose(0, 1), stride=2)
    got = tconv_wino_restatement(x, w)
    assert got.shape == ref.shape
    assert (got - ref).abs().max().item() <= 1e-12 * ref.abs().max().item()


def test_product_count():
    """the restatement forms 25 products per tile of 2 x 2 positions (the direct form: 4 positions x 9 taps = 36) and they read 16
    distinct transformed weights -- what the kernel's 25 MFMAs per k-step and its 16-value U image are built on"""
    del PRODUCTS[:]
    Hh, Ww = 6, 4
    tconv_wino_restatement(torch.randn(1, 2, Hh, Ww, dtype=torch.float64), torch.randn(3, 2, 3, 3, dtype=torch.float64))
    ntiles = ((Hh + 2) // 2) * ((Ww + 2) // 2)
    assert len(PRODUCTS) == 25 * ntiles
    assert len(set(PRODUCTS)) == 16


def test_host_weight_restatement_bit_for_bit(H):
    g = torch.Generator().manual_seed(3)
    w = torch.randn(10, 12, 3, 3, generator=g)
    wp = H.pack_weight(w)
    got = H.tconvw_weight_host(wp)
    want = weight_transform(w.double()).float()
    assert got.shape == (16, 12, 10) and torch.equal(got, want)
    assert torch.equal(H.tconvw_weight_host(wp, 0.5), weight_transform(w.double() * 0.5).float())


def test_eligibility_mirror(H):
    mk = lambda cin, G=1, k=3, **kw: H.PackedConv(None, G, 8, cin, k, k, 1, (1,), (1,), **kw)   # noqa: E731
    assert H.tconvw_eligible(mk(8)) and H.tconvw_eligible(mk(12)) and H.tconvw_eligible(mk(512))
    assert not H.tconvw_eligible(mk(6))                       # Cin % 4
    assert not H.tconvw_eligible(mk(8, G=2))                  # groups
    assert not H.tconvw_eligible(mk(8, k=1))
    assert not H.tconvw_eligible(mk(8), transposed=False)
    assert not H.tconvw_eligible(mk(8), in_shift=True)
    assert not H.tconvw_eligible(mk(8), io_bf16=True)
    assert not H.tconvw_eligible(mk(8, G=2, x_group_stride=8))


def test_allow_list_names_measured_up_conv_keys(H):
    """vspbfr_amd/tconv_wino_allow.json: shape keys of conv_tune.json's transposed entries whose recorded per-launch pair
    (profiles/tconv_wino_launch_ab.json) is at least 5 % faster; the route still answers `tconv` for them"""
    import json
    import os
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    allow = json.load(open(os.path.join(root, "vspbfr_amd", "tconv_wino_allow.json")))
    tune = json.load(open(os.path.join(root, "vspbfr_amd", "conv_tune.json")))
    rows = {r["key"]: r for r in json.load(open(os.path.join(root, "profiles", "tconv_wino_launch_ab.json")))["shapes"]}
    assert set(allow) <= {k for k, r in rows.items() if r["speedup_median"] >= 1.05}     # (tools/bench_tconv_wino.py HOLD: faster, held back)
    assert {"8,128,256,256,1,64,3,3,1,1,257,257,t", "8,256,128,128,1,128,3,3,1,1,129,129,t"} <= set(allow)
    assert set(allow) == set(H.TCONVW_ALLOW) and H.TCONV_WINO is True
    for key in allow:
        assert key.endswith(",t") and key in tune and rows[key]["launches"] >= 20
        B, cin, hh, ww, G, cout = (int(v) for v in key.split(",")[:6])
        pc = H.PackedConv(None, G, cout, cin, 3, 3, 1, (1,), (1,))
        assert H.tconvw_eligible(pc) and H.conv_route(pc, B, hh, ww, hh + 1, ww + 1, transposed=True).family == "tconv"


def _params(_lib, **kw):
    p = _lib.ConvParams()
    p.x = p.w = p.y = 256   # non-null, 16-byte aligned dummies: never dereferenced on the refusal paths
    p.B, p.Cin, p.H, p.W, p.G, p.cout_g, p.OH, p.OW = 1, 8, 4, 4, 1, 16, 5, 5
    p.KH = p.KW = 3
    p.stride_y = p.stride_x = p.osy = p.osx = 1
    p.y_ch, p.y_h, p.y_w = 16, 9, 9
    p.transposed = 1
    for g in range(4):
        p.dil[g], p.pad_y[g], p.pad_x[g] = 1, 1, 1
    for k, v in kw.items():
        setattr(p, k, v)
    return p


def test_entry_refusals_launch_nothing():
    """What the entry does not serve is VSP_ENOTSUP (-3) with its message prefix, decided before the device is touched"""
    from vspbfr_amd import _lib
    fn = _lib.lib.vsp_conv_transpose2d_s2_wino_f32
    assert fn(None, None) == -1 and "conv_transpose2d_s2_wino: null params" in _lib.last_error()
    for kw in ({"transposed": 0}, {"G": 2}, {"KH": 1, "KW": 1}, {"Cin": 6}, {"in_shift": 256}, {"io_bf16": 1}, {"x_group_stride": 8},
               {"Cin": 6, "G": 2, "in_shift": 256}):
        p = _params(_lib, **kw)
        assert fn(C.byref(p), None) == -3, kw
        assert _lib.last_error().startswith("conv_transpose2d_s2_wino:"), (kw, _lib.last_error())
    # an output that cannot hold (2H+1) x (2W+1) is an argument error, as in vsp_conv2d_f32
    assert fn(C.byref(_params(_lib, y_h=8)), None) == -1 and "transposed output must hold" in _lib.last_error()
    assert _lib.lib.vsp_tconvw_weight_floats(8, 16) == 2 * 1024 and _lib.lib.vsp_tconvw_weight_floats(6, 40) == 3 * 2 * 1024
    assert _lib.lib.vsp_tconvw_weight_f32(None, None, 8, 16, 1.0, None) == -1 and "tconvw_weight" in _lib.last_error()


# ------------------------------------------------------------------------------------------------ GPU
DEV = "cuda"


def dev(t):
    return t.to(DEV).contiguous()


def _lrelu(v, slope):
    return torch.where(v > 0, v, v * slope)


def _operands(B, Cin, Cout, Hh, Ww, seed, x=None, s_lo=0.5, s_hi=1.5):
    g = torch.Generator().manual_seed(seed)
    if x is None:
        x = torch.randn(B, Cin, Hh, Ww, generator=g)
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)
    s_in = torch.exp(torch.rand(B, Cin, generator=g) * (math.log(s_hi) - math.log(s_lo)) + math.log(s_lo))
    demod = torch.rand(B, Cout, generator=g) + 0.5
    return x, w, s_in, demod


def _ref(x, w, s_in, demod):
    B, Cin = s_in.shape
    return F.conv_transpose2d(x.double() * s_in.double().view(B, Cin, 1, 1), w.double().transpose(0, 1), stride=2) * demod.double().view(B, -1, 1, 1)


def _both(H, launch, ref, what):
    """launch() with the direct kernel, then twice with the new one -> asserts the bound and bit-identical repeats"""
    old = H.TCONV_WINO, H.PROFILER
    try:
        H.TCONV_WINO = False
        H.PROFILER = H.ConvProfiler()
        yd = launch().cpu()
        assert H.PROFILER.records[-1][3][7] == "tconv"
        H.TCONV_WINO = "all"
        y1 = launch()
        assert H.PROFILER.records[-1][3][7] == "tconvw", "the fused Winograd phase kernel did not serve this launch"
        y2 = launch()
        torch.cuda.synchronize()
    finally:
        H.TCONV_WINO, H.PROFILER = old
    assert torch.equal(y1.view(torch.int32), y2.view(torch.int32)), f"{what}: two launches differ"   # (bit patterns: NaN margins compare equal)
    y1 = y1.cpu()
    mask = torch.isfinite(ref)            # (a NaN in the reference marks what the launch must leave untouched)
    assert torch.equal(torch.isnan(y1), ~mask) and torch.equal(torch.isnan(yd), ~mask), f"{what}: wrote outside its extent or left a hole"
    r = torch.where(mask, ref, torch.zeros_like(ref))
    e_dir = (torch.where(mask, yd.double(), r) - r).abs().max().item()
    e_new = (torch.where(mask, y1.double(), r) - r).abs().max().item()
    bound = 2 * e_dir + 1e-6 * r.abs().max().item()
    print(f"tconv_wino {what}: e_direct {e_dir:.3e} e_new {e_new:.3e} bound {bound:.3e} max|ref| {r.abs().max().item():.3e}")
    assert e_new <= bound, f"{what}: e_new {e_new:.3e} > 2 e_direct + 1e-6 max|ref| = {bound:.3e}"


@pytest.mark.gpu
@pytest.mark.parametrize("B,Cin,Cout,Hh,Ww", [(1, 8, 16, 4, 4), (3, 12, 24, 5, 7), (2, 64, 40, 16, 16)])
def test_shapes(H, B, Cin, Cout, Hh, Ww):
    """two k-steps and a ragged tile column (5 x 5 positions) | ragged channel block, even position counts, odd map | several tiles per
    wave, ragged Cout, many k-steps"""
    x, w, s_in, demod = _operands(B, Cin, Cout, Hh, Ww, 11)
    pc = H.PackedConv(H.pack_weight(dev(w)), 1, Cout, Cin, 3, 3, 1, (1,), (1,))
    xd, sd, dd = dev(x), dev(s_in), dev(demod)
    _both(H, lambda: H.conv_transpose2d_s2_fused(xd, pc, in_scale=sd, out_scale=dd), _ref(x, w, s_in, demod), f"{B}x{Cin}->{Cout} {Hh}x{Ww}")


@pytest.mark.gpu
def test_output_extents_and_channel_offset(H):
    """B 2, 32 -> 32, 33 x 33: `_into` a 67^2 and a 68^2 destination (66^2 cannot hold the 67 x 67 output: refused), and a channel offset
    into a wider, larger tensor whose other elements stay untouched"""
    B, Cin, Cout, Hh = 2, 32, 32, 33
    x, w, s_in, demod = _operands(B, Cin, Cout, Hh, Hh, 12)
    pc = H.PackedConv(H.pack_weight(dev(w)), 1, Cout, Cin, 3, 3, 1, (1,), (1,))
    xd, sd, dd = dev(x), dev(s_in), dev(demod)
    ref = _ref(x, w, s_in, demod)
    for side in (67, 68):
        want = torch.zeros(B, Cout, side, side, dtype=torch.float64)
        want[:, :, :67, :67] = ref
        _both(H, lambda: H.conv_transpose2d_s2_into(xd, pc, (side, side), in_scale=sd, out_scale=dd), want, f"into {side}^2")
    with pytest.raises(RuntimeError, match="out_hw"):
        H.conv_transpose2d_s2_into(xd, pc, (66, 66), in_scale=sd, out_scale=dd)
    want = torch.full((B, Cout + 5, 68, 68), float("nan"), dtype=torch.float64)
    want[:, 3:3 + Cout, :67, :67] = ref

    def launch():
        out = torch.full((B, Cout + 5, 68, 68), float("nan"), device=DEV)
        return H.conv2d_packed(xd, pc, transposed=True, out=out, y_coff=3, bf16=False, in_scale=sd, out_scale=dd)
    _both(H, launch, want, "y_coff 3 of 37 channels, 68^2")


@pytest.mark.gpu
@pytest.mark.parametrize("chain", [False, True])
def test_scales_and_epilogue(H, chain):
    """B 2, 16 -> 16, 8 x 8, per-image input scales spanning 1e-2 .. 1e2 and the demodulation scale (the `only_os` fast path); once the
    full chain: channel scale and bias, first activation with its bias, second activation with bias, slope 0.01 and a gain"""
    B, Cin, Cout, Hh = 2, 16, 16, 8
    x, w, s_in, demod = _operands(B, Cin, Cout, Hh, Hh, 13, s_lo=1e-2, s_hi=1e2)
    s_in[0, 0], s_in[1, 1] = 1e-2, 1e2
    pc = H.PackedConv(H.pack_weight(dev(w)), 1, Cout, Cin, 3, 3, 1, (1,), (1,))
    xd, sd, dd = dev(x), dev(s_in), dev(demod)
    ref = _ref(x, w, s_in, demod)
    kw = {}
    if chain:
        g = torch.Generator().manual_seed(14)
        cs, cb, b1, b2 = (torch.randn(Cout, generator=g) for _ in range(4))
        cs = cs.abs() + 0.5
        v = ref * cs.double().view(1, -1, 1, 1) + cb.double().view(1, -1, 1, 1) + b1.double().view(1, -1, 1, 1)
        v = _lrelu(v, 0.2) * SQRT2 + b2.double().view(1, -1, 1, 1)
        ref = _lrelu(v, 0.01) * 1.5
        kw = dict(ch_scale=dev(cs), ch_bias=dev(cb), act1=True, bias1=dev(b1), act2=1, bias2=dev(b2), slope2=0.01, gain2=1.5)
    _both(H, lambda: H.conv_transpose2d_s2_fused(xd, pc, in_scale=sd, out_scale=dd, **kw), ref, "full chain" if chain else "only_os")


@pytest.mark.gpu
@pytest.mark.parametrize("kind", ["dc20", "lrelu3"])
def test_conditioning_fence_inputs(H, kind):
    """64 -> 32, 16 x 16 on inputs with a DC offset (20 + N(0,1), lrelu(N(3,1))): the transforms take differences of neighbours"""
    B, Cin, Cout, Hh = 2, 64, 32, 16
    g = torch.Generator().manual_seed(15)
    n = torch.randn(B, Cin, Hh, Hh, generator=g)
    x = 20 + n if kind == "dc20" else _lrelu(3 + n, 0.2)
    x, w, s_in, demod = _operands(B, Cin, Cout, Hh, Hh, 16, x=x)
    pc = H.PackedConv(H.pack_weight(dev(w)), 1, Cout, Cin, 3, 3, 1, (1,), (1,))
    xd, sd, dd = dev(x), dev(s_in), dev(demod)
    _both(H, lambda: H.conv_transpose2d_s2_fused(xd, pc, in_scale=sd, out_scale=dd), _ref(x, w, s_in, demod), kind)


@pytest.mark.gpu
def test_device_weight_transform_bit_for_bit(H):
    g = torch.Generator().manual_seed(17)
    for cout, cin in ((40, 12), (16, 8)):
        w = torch.randn(cout, cin, 3, 3, generator=g)
        wp = H.pack_weight(dev(w))
        for scale in (1.0, 0.37):
            U = H.tconvw_weight(wp, scale)
            assert U.numel() == ((cout + 15) // 16) * ((cin + 3) // 4) * 1024
            assert torch.equal(H.tconvw_unpack(U, cin, cout).cpu(), H.tconvw_weight_host(wp.cpu(), scale))
            full = U.view((cout + 15) // 16, (cin + 3) // 4, 4, 4, 16, 4)
            if cout % 16:
                assert full[-1, :, :, :, cout % 16:].abs().max().item() == 0      # channels past Cout are zeros


@pytest.mark.gpu
def test_refused_launches_leave_the_destination_untouched(H):
    """Cin = 6, two groups, an input shift: VSP_ENOTSUP from the entry, the NaN-filled destination untouched; through conv2d_packed the
    launcher owns the fall-back to vsp_conv2d_f32"""
    from vspbfr_amd import _lib
    x6, x8 = dev(torch.randn(1, 6, 4, 4)), dev(torch.randn(1, 8, 4, 4))
    wbuf = dev(torch.randn(4 * 1024))
    shift = dev(torch.randn(8))
    for kw, xin in (({"Cin": 6}, x6), ({"G": 2, "cout_g": 8, "Cin": 4}, x8), ({"in_shift": shift.data_ptr()}, x8)):
        y = torch.full((1, 16, 9, 9), float("nan"), device=DEV)
        p = _params(_lib, x=xin.data_ptr(), w=wbuf.data_ptr(), y=y.data_ptr(), **kw)
        assert _lib.lib.vsp_conv_transpose2d_s2_wino_f32(C.byref(p), None) == -3, kw
        torch.cuda.synchronize()
        assert torch.isnan(y).all(), kw
    x, w, s_in, demod = _operands(1, 6, 16, 4, 4, 18)
    pc = H.PackedConv(H.pack_weight(dev(w)), 1, 16, 6, 3, 3, 1, (1,), (1,))
    old = H.TCONV_WINO, H.PROFILER
    try:
        H.TCONV_WINO, H.PROFILER = "all", H.ConvProfiler()
        y = H.conv_transpose2d_s2_fused(dev(x), pc, in_scale=dev(s_in), out_scale=dev(demod))
        assert H.PROFILER.records[-1][3][7] == "tconv"
    finally:
        H.TCONV_WINO, H.PROFILER = old
    ref = _ref(x, w, s_in, demod)
    assert (y.cpu().double() - ref).abs().max().item() <= 2e-5 * ref.abs().max().item() + 2e-5


@pytest.mark.gpu
def test_without_an_input_scale_and_padded_k_steps(H):
    """no `in_scale` (the kernel reads the constant 1 behind stride 0) on Cin = 20: five k-steps, the loop body's other three are padding"""
    B, Cin, Cout, Hh, Ww = 2, 20, 16, 6, 9
    x, w, s_in, demod = _operands(B, Cin, Cout, Hh, Ww, 19)
    pc = H.PackedConv(H.pack_weight(dev(w)), 1, Cout, Cin, 3, 3, 1, (1,), (1,))
    xd, dd = dev(x), dev(demod)
    _both(H, lambda: H.conv_transpose2d_s2_fused(xd, pc, out_scale=dd), _ref(x, w, torch.ones(B, Cin), demod), "no in_scale, Cin 20")


@pytest.mark.gpu
def test_an_inf_stays_inside_its_tile(H):
    """Cin = 8 (two real k-steps, two padded ones) with one Inf in the last channel of image 0: the padded k-steps read zeros on both operands,
    so only the 4 x 4 outputs of the tile whose window holds the Inf may be non-finite; everything else keeps the bound"""
    B, Cin, Cout, Hh = 2, 8, 16, 6
    x, w, s_in, demod = _operands(B, Cin, Cout, Hh, Hh, 20)
    pc = H.PackedConv(H.pack_weight(dev(w)), 1, Cout, Cin, 3, 3, 1, (1,), (1,))
    ref = _ref(x, w, s_in, demod)
    x[0, 7, 0, 0] = float("inf")
    old = H.TCONV_WINO
    try:
        H.TCONV_WINO = "all"
        y = H.conv_transpose2d_s2_fused(dev(x), pc, in_scale=dev(s_in), out_scale=dev(demod)).cpu().double()
    finally:
        H.TCONV_WINO = old
    y[0, :, :4, :4] = ref[0, :, :4, :4]
    assert torch.isfinite(y).all()
    assert (y - ref).abs().max().item() <= 2e-5 * ref.abs().max().item()


@pytest.mark.gpu
def test_default_switch_takes_the_kernel_on_an_allow_listed_key(H):
    """TCONV_WINO = True (the default): an allow-listed shape key runs the new kernel and gives the bits of the "all" launch; the same layer at
    another batch size keeps the direct kernel"""
    key = sorted(H.TCONVW_ALLOW)[-1]
    B, Cin, Hh, Ww, _, Cout = (int(v) for v in key.split(",")[:6])
    g = torch.Generator().manual_seed(21)
    x = dev(torch.randn(B, Cin, Hh, Ww, generator=g))
    w = torch.randn(Cout, Cin, 3, 3, generator=g) / math.sqrt(Cin * 9)
    s_in, demod = dev(torch.rand(B, Cin, generator=g) + 0.5), dev(torch.rand(B, Cout, generator=g) + 0.5)
    pc = H.PackedConv(H.pack_weight(dev(w)), 1, Cout, Cin, 3, 3, 1, (1,), (1,))
    old = H.TCONV_WINO, H.PROFILER
    try:
        H.PROFILER = H.ConvProfiler()
        assert H.TCONV_WINO is True
        y = H.conv_transpose2d_s2_fused(x, pc, in_scale=s_in, out_scale=demod)
        assert H.PROFILER.records[-1][3][7] == "tconvw" and H.PROFILER.records[-1][3][8] == key
        H.conv_transpose2d_s2_fused(x[:1].contiguous(), pc, in_scale=s_in[:1].contiguous(), out_scale=demod[:1].contiguous())
        assert H.PROFILER.records[-1][3][7] == "tconv"
        H.TCONV_WINO = "all"
        ya = H.conv_transpose2d_s2_fused(x, pc, in_scale=s_in, out_scale=demod)
        H.TCONV_WINO = False
        yd = H.conv_transpose2d_s2_fused(x, pc, in_scale=s_in, out_scale=demod)
    finally:
        H.TCONV_WINO, H.PROFILER = old
    assert torch.equal(y, ya)
    assert (y - yd).abs().max().item() <= 2e-5 * yd.abs().max().item()
