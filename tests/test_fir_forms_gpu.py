"""GPU checks of every compiled form of csrc/upfirdn2d.hip -- fir_tile_kernel<2 | 3 | 4 taps, fp32 | bf16> with its interior-window and
tile_inside fast paths, the eight fir_strip_bf16_kernel instantiations, fir_generic_kernel -- against the float64 restatement of
tests/fir_ref.py, on the case table that module builds (fir_ref.form names the form each case reaches; tests/test_fir_ref.py asserts on
the CPU that the table reaches every form and that wrong variants of the restatement miss this bound on these very inputs).

Bound (fir_ref.bound, the rule of tests/stream_ref.py and tests/test_tacc_kernels.py): max |HIP - float64| <= 4 e_ref + 2e-6 max |float64|
with e_ref the error of the same restatement run in float32 on the CPU; a bf16 output per element within 2^-8 |float64| of that.  bf16
operands are rounded before the reference sees them.  Every case prints its e_ref / e_hip / ratio line under -s; one full run is kept in
profiles/fir_forms_gputest.log.  Every output here is allocated by the hip_ops wrappers (no case hands the C entry a buffer of its own).

Worst ratio e_hip / e_ref per form in the recorded run (the bound is 4 e_ref + the additive term; 322 passed in 3 s):
    fp32: tile4 1.47, tile3 1.41, tile2 1.22, generic 1.10, generic with an epilogue 1.46.
    bf16 (e_hip = what is left of the error beyond the 2^-8 |float64| of the store): every strip form 0.00 on all 65 strip cases, tile4 0.03,
    tile3 0.09, tile2 0.18.
No case prints more than 4, so none passes through the additive term alone.

The first run of this table found a fault of the strip walk's dispatch (30 cases up to 1.0 off): with in_w + pad_x0 odd the tensor's last
element shares a dword with two bytes past the end and the buffer range check returns the dword as zero.  Those shapes now take the tile
kernel (form `tile4/bf16/split-word`) and stay in the table, each beside a shape of the same output size that the strip walk serves."""
import pytest
import torch

import fir_ref as R

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
F64, F32, BF = torch.float64, torch.float32, torch.bfloat16
RUNNABLE = [c for c in R.CASES if c.refuse is None]
REFUSED = [c for c in R.CASES if c.refuse is not None]
WORST = {}


@pytest.fixture(scope="module")
def H():
    from vspbfr_amd import hip_ops
    return hip_ops


@pytest.fixture
def separable_switch(H):
    """hip_ops.SEPARABLE_BLUR, put back after the test"""
    prev = H.SEPARABLE_BLUR

    def switch(on):
        H.SEPARABLE_BLUR = on

    yield switch
    H.SEPARABLE_BLUR = prev


def _place(t, dtype, shape, offset_bytes=0):
    """t on the device as `dtype` and `shape`; offset_bytes > 0: a contiguous view that starts so many bytes into its storage"""
    if t is None:
        return None
    t = t.to(DEV).to(dtype).reshape(shape).contiguous()
    if not offset_bytes:
        assert t.data_ptr() % 16 == 0
        return t
    skip = offset_bytes // t.element_size()
    buf = torch.zeros(t.numel() + 16, dtype=dtype, device=DEV)
    v = buf[skip:skip + t.numel()].view(shape)
    v.copy_(t)
    assert v.data_ptr() % 16 == offset_bytes and v.is_contiguous()
    return v


def launch(H, case, d):
    """the case through its entry: hip_ops.blur_fused, or hip_ops.upfirdn2d_native_layout with an epilogue structure built here"""
    from vspbfr_amd._lib import FirEpilogue
    dt = BF if case.dtype == "bf16" else F32
    major = case.B * case.C
    oh, ow = R.case_out_size(case)
    k = d["k"].to(DEV)
    mis = case.misalign
    ps = _place(d.get("plane_scale"), F32, (case.B, case.C))
    nz = _place(d.get("noise"), F32, (case.B, 1, oh, ow), mis.get("noise", 0))
    nw = None if case.refuse == "noise_w" else _place(d.get("noise_w"), F32, (1,))
    ab = _place(d.get("act_bias"), F32, (case.C,))
    if case.entry == "blur":
        x = _place(d["x"], dt, (case.B, case.C, case.H, case.W))
        r1 = _place(d.get("res1"), dt, (case.B, case.C, oh, ow), mis.get("res1", 0))
        r2 = _place(d.get("res2"), dt, (case.B, case.C, oh, ow), mis.get("res2", 0))
        return H.blur_fused(x, k, case.pad, plane_scale=ps, noise=nz, noise_w=nw, act_bias=ab, act=d.get("act", False), res1=r1, res2=r2,
                            slope=R.SLOPE, gain=R.SQRT2)
    x = _place(d["x"], dt, (major, case.H, case.W, case.minor))
    epi = None
    keep = []
    if case.epi is not None:
        r1 = _place(d.get("res1"), dt, (major, oh, ow), mis.get("res1", 0))
        r2 = _place(d.get("res2"), dt, (major, oh, ow), mis.get("res2", 0))
        keep = [ps, nz, nw, ab, r1, r2]
        epi = FirEpilogue()
        epi.plane_scale, epi.noise, epi.noise_w, epi.act_bias, epi.res1, epi.res2 = [(t.data_ptr() if t is not None else None) for t in keep]
        epi.channels = case.C + 1 if case.refuse == "channels" else case.C
        epi.act, epi.slope, epi.gain, epi.flags = (1 if d.get("act") else 0), R.SLOPE, R.SQRT2, 0
    px0, px1, py0, py1 = R.pad4(case)
    out = H.upfirdn2d_native_layout(x, k, case.up[0], case.up[1], case.down[0], case.down[1], px0, px1, py0, py1, epilogue=epi)
    torch.cuda.synchronize()          # (the operands in `keep` live until the launch has run)
    del keep
    return out


@pytest.mark.parametrize("name", [c.name for c in RUNNABLE])
def test_form_matches_float64(H, separable_switch, name):
    case = R.CASE_BY_NAME[name]
    form = R.case_form(case)
    d = R.inputs(case)
    ref64, ref32 = R.reference(case, F64, ops=d), R.reference(case, F32, ops=d)
    if case.force2d:
        separable_switch(False)
    else:
        assert H.SEPARABLE_BLUR
    try:
        got = launch(H, case, d)
        torch.cuda.synchronize()
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):
            pytest.exit(f"{name}: the device reported a fault ({e}); no further case is launched on it", returncode=3)
        raise
    bf = R.output_bf16(case)
    assert got.dtype == (BF if bf else F32), (name, got.dtype)
    e_ref, e_hip, ratio = R.bound(got.float(), ref64, ref32, bf16=bf, what=f"{form:22s} {name}")
    fam = form.replace("+tail", "")
    if ratio == ratio and ratio > WORST.get(fam, (0.0, ""))[0]:
        WORST[fam] = (ratio, name)


def test_zero_corner_taps_are_left_to_the_2d_form(H):
    """outer([1, 3, 3, 0], [1, 3, 3, 0]): an outer product whose flipped corner -- the tap the separable form divides by -- is zero.  The
    host gate refuses the flag (a flagged call would divide by zero: inf / NaN, which test_form_matches_float64[zero-corner-*] would show)."""
    for name, k in R.TAPS.items():
        assert H.taps_separable(k.to(DEV)) == R.SEPARABLE_TAPS[name], name
    assert not H.taps_separable(R.TAPS["zero4"].to(DEV))
    assert R.case_form(R.CASE_BY_NAME["zero-corner-full"]) == "strip/2d/en/act"


@pytest.mark.parametrize("name", [c.name for c in REFUSED])
def test_refusals(H, name):
    """what no kernel serves is an error, never another kernel: bf16 planes with up = 2 or with fewer than four columns, an epilogue on
    interleaved planes (minor != 1), channels that do not divide major, noise without noise_w"""
    case = R.CASE_BY_NAME[name]
    assert R.case_form(case) in ("enotsup", "einval")
    with pytest.raises(RuntimeError):
        launch(H, case, R.inputs(case))


def test_blur_fused_converts_narrow_bf16_planes(H):
    """planes of fewer than four columns have no bf16 kernel (the tile kernel's loads are four elements wide): blur_fused runs them in fp32,
    as it does narrow outputs"""
    x = torch.randn(2, 3, 5, 3, device=DEV).to(BF)
    y = H.blur_fused(x, R.TAPS["asym4"].to(DEV), (8, 8))
    assert y.dtype == F32 and y.shape == (2, 3, 18, 16)
    x4 = torch.randn(2, 3, 5, 4, device=DEV).to(BF)
    assert H.blur_fused(x4, R.TAPS["asym4"].to(DEV), (8, 8)).dtype == BF


def test_zz_worst_ratio_per_form(H):
    """(prints the worst e_hip / e_ref of this run per form family: the figures of the module docstring)"""
    for fam in sorted(WORST):
        print(f"FIR-WORST {fam:24s} {WORST[fam][0]:.2f}  {WORST[fam][1]}")
