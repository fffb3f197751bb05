"""Every compiled route of the conv weight-gradient kernel (csrc/conv_wgrad.hip, vsp_conv2d_wgrad_f32) against float64 on the CPU:
autograd of F.conv2d(x * xs, w = 0, stride, pad, dil) * dys per group.  The bound is the project's own (test_conv2d_wgrad_tile_shapes):

    max|HIP - float64| <= 2e-5 * max|ref| + 2e-5 * max|ref|        (accumulation onto an equal-sized buffer: 2e-5 * max|dw0 + ref| + 4e-5 * max|ref|)

and every comparison prints its split, e_hip, e_ref = max|torch fp32 on the CPU - float64| and their ratio first (`pytest -s`).

Every case asserts the split the planner gives it, split = vsp_conv2d_wgrad_work_floats(p) / dw_elems, so that a planner change
cannot move a case off its route unnoticed.  The listed values assume vsp::kNumCU = 256 (the split is min(ceil(per_cu * kNumCU /
(tiles * G)), chunks / 8), per_cu = 2 or 3); test_planned_splits checks them without a GPU.

Routes and what tests them.  <NTAP, WCO, NB, XJ, S, TCL> are the template arguments of conv_wgrad_kernel (S = 0: the generic loop):

    instantiation / host path                               case
    <9,4,2,1,1,6>  sliced reducer (split 32), no memset     A
    <9,1,1,1,1,6>  plain reducer, n % 4 != 0, memset        B
    <9,4,1,1,1,6>                                           C
    <9,2,2,1,1,5>                                           D1
    <9,1,1,1,1,4>                                           D2
    <9,2,1,1,1,5>  dilation 2 on dense slab rows            D3
    <9,4,2,2,2,5>                                           E
    <9,4,1,2,2,4>  true groups, x window                    W (test_input_window)
    <1,4,2,1>                                               F1
    <1,4,1,1>                                               F2
    <1,2,2,1>      ragged channels                          F3
    <9,4,1,2>      generic loop, XJ = 2 at stride 1         G16 (75 quads), G48 (123 quads)
    <9,1,1,1,1,6>  dense chunk refused -> row segments      K (shared input, four dilations)
    wgrad_fewin_kernel + fewin_reduce_kernel                FEW
    fp32 atomics, dw memset, accumulate                     test_atomic_route: A, B, E, K, FEW
    split clamp, workspace errors, repeatability, guards    test_workspace_*: A, B
    x_ch / x_coff                                           test_input_window: W, K, FEW"""
import ctypes as C
import functools

import pytest
import torch
import torch.nn.functional as F

gpu = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
GUARD = 64            # floats behind a buffer that must stay as they were
SENTINEL = -1234.5


def case(B, cin, cout, hw, k, s, p, d, split, G=1, shared=False):
    return dict(B=B, cin_g=cin, cout_g=cout, hw=hw, k=k, s=s, p=p, d=d, split=split, G=G, shared=shared)


# id -> geometry (per group) and the split the planner must give it
CASES = {
    "A": case(4, 32, 64, (64, 64), 3, 1, 1, 1, 32),
    "B": case(3, 17, 5, (24, 70), 3, 1, 1, 1, 18),
    "C": case(2, 16, 64, (20, 40), 3, 1, 1, 1, 5),
    "D1": case(3, 48, 32, (12, 32), 3, 1, 1, 1, 2),
    "D2": case(3, 16, 16, (16, 16), 3, 1, 1, 1, 1),
    "D3": case(3, 24, 24, (30, 32), 3, 1, 2, 2, 5),
    "E": case(2, 32, 48, (65, 65), 3, 2, 0, 1, 4),
    "F1": case(2, 64, 128, (24, 24), 1, 1, 0, 1, 3),
    "F2": case(2, 16, 64, (24, 24), 1, 1, 0, 1, 3),
    "F3": case(2, 48, 32, (13, 20), 1, 1, 0, 1, 1),
    "G16": case(2, 16, 16, (20, 66), 3, 1, 16, 16, 10),
    "G48": case(2, 16, 16, (20, 66), 3, 1, 48, 48, 10),
    "K": case(2, 24, 16, (16, 32), 3, 1, (1, 2, 4, 8), (1, 2, 4, 8), 4, G=4, shared=True),
    "W": case(3, 16, 24, (18, 20), 3, 2, 1, 1, 1, G=2),
    "FEW": case(3, 3, 16, (23, 27), 1, 1, 0, 1, 3),     # the stream form: one copy per (image, pixel range) = B copies
}
MAIN = ["A", "B", "C", "D1", "D2", "D3", "E", "F1", "F2", "F3", "G16", "G48", "K"]
X_LEAD, X_TRAIL = 5, 3      # channels in front of / behind the window of test_input_window


def geom(c):
    """(pads, dils, OH, OW, x channels read, dw elements)"""
    pads = tuple(c["p"]) if isinstance(c["p"], tuple) else (c["p"],) * c["G"]
    dils = tuple(c["d"]) if isinstance(c["d"], tuple) else (c["d"],) * c["G"]
    H, W = c["hw"]
    OH = (H + 2 * pads[0] - dils[0] * (c["k"] - 1) - 1) // c["s"] + 1
    OW = (W + 2 * pads[0] - dils[0] * (c["k"] - 1) - 1) // c["s"] + 1
    xc = c["cin_g"] if c["shared"] else c["G"] * c["cin_g"]
    return pads, dils, OH, OW, xc, c["G"] * c["cout_g"] * c["cin_g"] * c["k"] ** 2


def reference(c, x, xs, gy, dys, dtype):
    """dW per group by autograd of the forward expression in `dtype`; x / xs are the window's channels only."""
    pads, dils, _, _, _, _ = geom(c)
    cin, cout = c["cin_g"], c["cout_g"]
    out = []
    for g in range(c["G"]):
        sl = slice(0, cin) if c["shared"] else slice(g * cin, (g + 1) * cin)
        so = slice(g * cout, (g + 1) * cout)
        w = torch.zeros(cout, cin, c["k"], c["k"], dtype=dtype, requires_grad=True)
        with torch.enable_grad():
            y = F.conv2d((x[:, sl].to(dtype) * xs[:, sl, None, None].to(dtype)), w, None, c["s"], pads[g], dils[g]) * dys[:, so, None, None].to(dtype)
            y.backward(gy[:, so].to(dtype))
        out.append(w.grad)
    return torch.cat(out, 0)


@functools.lru_cache(maxsize=None)
def data(cid, window=False):
    """Operands and references of a case, built once and shared (read-only).  `window`: x and its scale carry X_LEAD / X_TRAIL more
    channels of their own values around the ones the layer reads."""
    c = CASES[cid]
    _, _, OH, OW, xc, _ = geom(c)
    g_ = torch.Generator().manual_seed(1000 + sorted(CASES).index(cid))
    lead, trail = (X_LEAD, X_TRAIL) if window else (0, 0)
    x = torch.randn(c["B"], lead + xc + trail, *c["hw"], generator=g_)
    xs = torch.rand(c["B"], lead + xc + trail, generator=g_) + 0.5
    gy = torch.randn(c["B"], c["G"] * c["cout_g"], OH, OW, generator=g_)
    dys = torch.rand(c["B"], c["G"] * c["cout_g"], generator=g_) + 0.5
    xin, xsin = x[:, lead:lead + xc], xs[:, lead:lead + xc]
    ref64 = reference(c, xin, xsin, gy, dys, torch.float64)
    ref32 = reference(c, xin, xsin, gy, dys, torch.float32)
    dw0 = torch.randn(ref64.shape, generator=g_) * float(ref64.std())     # an equal-sized buffer to accumulate onto
    return dict(x=x, xs=xs, gy=gy, dys=dys, ref64=ref64, ref32=ref32, dw0=dw0)


def dev(t):
    return t.to(DEV).contiguous()


def check(got, d, what, split, dw0=None):
    """The project bound against float64 (see the module docstring); prints the figures before it asserts."""
    ref64, mx = d["ref64"], float(d["ref64"].abs().max())
    want = ref64 if dw0 is None else dw0.double() + ref64
    want32 = d["ref32"] if dw0 is None else dw0 + d["ref32"]
    got = got.detach().cpu().double().reshape(want.shape)
    assert torch.isfinite(got).all(), f"{what}: non-finite output"
    e_ref = float((want32.double() - want).abs().max())
    err = float((got - want).abs().max())
    tol = 2e-5 * float(want.abs().max()) + (2e-5 if dw0 is None else 4e-5) * mx
    print(f"WGRAD {what}: split={split} e_hip={err:.3e} e_ref={e_ref:.3e} ratio={err / e_ref if e_ref else float('nan'):.2f} "
          f"tol={tol:.3e} max|ref|={mx:.4g}")
    assert err <= tol, f"{what}: max|d|={err:.3e} tol={tol:.3e} (e_ref {e_ref:.3e})"


def fill_params(c, x=None, gy=None, dw=None, xs=None, dys=None, x_ch=0, x_coff=0, work=None, work_floats=0, accumulate=False, B=None):
    """A vsp_conv_wgrad_params block for the case; operands are device pointers (ints) or None."""
    from vspbfr_amd._lib import ConvWgradParams
    pads, dils, OH, OW, _, _ = geom(c)
    p = ConvWgradParams()
    p.x, p.dy, p.dw, p.x_scale, p.dy_scale = x, gy, dw, xs, dys
    p.B, p.Cin_g, p.G, p.Cout_g = c["B"] if B is None else B, c["cin_g"], c["G"], c["cout_g"]
    p.H, p.W = c["hw"]
    p.OH, p.OW, p.KH, p.KW, p.stride = OH, OW, c["k"], c["k"], c["s"]
    p.dil, p.pad = dils[0], pads[0]
    if isinstance(c["d"], tuple):
        p.per_group_geometry = 1
        for g in range(min(c["G"], 4)):
            p.dil_g[g], p.pad_g[g] = dils[g], pads[g]
    p.x_shared, p.x_ch, p.x_coff = int(c["shared"]), x_ch, x_coff
    p.accumulate, p.work, p.work_floats, p.dw_scale = int(accumulate), work, work_floats, 1.0
    return p


def planned_split(lib, c):
    _, _, _, _, _, n = geom(c)
    wf = int(lib.vsp_conv2d_wgrad_work_floats(C.byref(fill_params(c))))
    assert wf % n == 0 and wf > 0, (wf, n)
    return wf // n


def wrapper_args(c):
    pads, dils, _, _, _, _ = geom(c)
    per_group = isinstance(c["d"], tuple)
    return dict(weight_shape=(c["G"] * c["cout_g"], c["cin_g"], c["k"], c["k"]), stride=c["s"], padding=pads if per_group else pads[0],
                dilation=dils if per_group else dils[0], groups=c["G"], x_shared=c["shared"])


def run_wrapper(H, cid, d, **kw):
    return H.conv2d_wgrad(dev(d["x"]), dev(d["gy"]), x_scale=dev(d["xs"]), dy_scale=dev(d["dys"]), **wrapper_args(CASES[cid]), **kw)


@pytest.fixture(scope="module")
def H():
    from vspbfr_amd import hip_ops
    return hip_ops


# ------------------------------------------------------------------------------------------------ the plan (no GPU)
def test_planned_splits():
    """The planner's split of every case (vsp_conv2d_wgrad_work_floats is host code), for vsp::kNumCU = 256: A reaches the sliced
    reducer's split >= 32, B has 18 unaligned copies of 765 floats."""
    from vspbfr_amd import _lib
    got = {cid: planned_split(_lib.lib, c) for cid, c in CASES.items()}
    assert got == {cid: c["split"] for cid, c in CASES.items()}, got
    assert geom(CASES["B"])[5] == 765 and geom(CASES["A"])[5] % 4 == 0
    assert geom(CASES["E"])[2:4] == (32, 32)


def test_references_agree_with_an_explicit_sum():
    """The autograd reference against an einsum over unfolded taps (per-group dilation, shared input, scales, window): case K."""
    c, d = CASES["K"], data("K", True)
    x = (d["x"].double() * d["xs"][:, :, None, None].double())[:, X_LEAD:X_LEAD + c["cin_g"]]
    gy = d["gy"].double() * d["dys"][:, :, None, None].double()
    Hh, Ww = c["hw"]
    for g, r in enumerate(c["d"]):
        cols = F.unfold(x, 3, dilation=r, padding=r).reshape(c["B"], c["cin_g"], 9, Hh * Ww)
        dw = torch.einsum("bop,bitp->oit", gy[:, g * 16:(g + 1) * 16].reshape(c["B"], 16, -1), cols).reshape(16, c["cin_g"], 3, 3)
        assert float((dw - d["ref64"][g * 16:(g + 1) * 16]).abs().max()) <= 1e-12 * float(dw.abs().max())


# ------------------------------------------------------------------------------------------------ every route, workspace form
@gpu
@pytest.mark.parametrize("cid", MAIN)
def test_route(H, cid):
    """Each instantiation of the table above through hip_ops.conv2d_wgrad (workspace route) with per-sample scales on both sides, and
    accumulation onto an equal-sized buffer; the split is the listed one."""
    c, d = CASES[cid], data(cid)
    split = planned_split(H.lib, c)
    assert split == c["split"], (cid, split)
    dw = run_wrapper(H, cid, d)
    check(dw, d, cid, split)
    dw2 = run_wrapper(H, cid, d, out=dev(d["dw0"]), accumulate=True)
    check(dw2, d, cid + " accumulate", split, dw0=d["dw0"])


# ------------------------------------------------------------------------------------------------ workspace handling (C entry)
class Owned:
    """Device operands of a case plus a workspace and a dw buffer the test owns, each with GUARD sentinel floats behind it."""

    def __init__(self, H, cid, work_floats, poison=float("nan"), dw_fill=float("nan")):
        self.H, self.c, self.d = H, CASES[cid], data(cid)
        self.n = geom(self.c)[5]
        self.t = {k: dev(self.d[k]) for k in ("x", "gy", "xs", "dys")}
        self.wf = work_floats
        self.wbuf = torch.full((work_floats + 1 + GUARD,), poison, device=DEV)       # (+ 1: room for the misaligned view)
        self.wbuf[work_floats:] = SENTINEL
        self.dbuf = torch.full((self.n + GUARD,), dw_fill, device=DEV)
        self.dbuf[self.n:] = SENTINEL

    @property
    def dw(self):
        return self.dbuf[:self.n]

    def launch(self, work_floats=None, work_offset=0, accumulate=False):
        t = self.t
        p = fill_params(self.c, t["x"].data_ptr(), t["gy"].data_ptr(), self.dbuf.data_ptr(), t["xs"].data_ptr(), t["dys"].data_ptr(),
                        work=self.wbuf.data_ptr() + 4 * work_offset, work_floats=self.wf if work_floats is None else work_floats,
                        accumulate=accumulate)
        rc = self.H.lib.vsp_conv2d_wgrad_f32(C.byref(p), self.H._stream())
        torch.cuda.synchronize()
        return rc

    def guards_intact(self, work_floats=None):
        wf = self.wf if work_floats is None else work_floats
        s = torch.tensor(SENTINEL).view(torch.int32).item()
        return bool((self.wbuf[wf:].view(torch.int32) == s).all()) and bool((self.dbuf[self.n:].view(torch.int32) == s).all())


@gpu
@pytest.mark.parametrize("cid", ["A", "B"])
def test_workspace_poisoned_guarded_repeatable(H, cid):
    """A workspace full of NaN: dw is finite and within the bound, so every element of every copy is stored (A: full tiles, the entry
    skips the memset) or zeroed first (B: ragged tiles, 18 copies of 765 floats, the entry clears them).  The floats behind the
    workspace and behind dw keep their bits, and a second launch gives the same bits (the copies are summed in a fixed order).
    Measured once on an MI355X with the entry's `holes` condition forced to false: B passes as well -- a copy holds only the valid
    (co, ci) pairs and every workgroup, even one without a chunk, stores all of its tile's, so the memset is a safety margin and
    this test pins the kernel's side of that claim only for A."""
    c = CASES[cid]
    split = planned_split(H.lib, c)
    assert split == c["split"]
    o = Owned(H, cid, split * geom(c)[5])
    assert o.launch() == 0
    check(o.dw, o.d, f"{cid} poisoned workspace", split)
    assert o.guards_intact()
    first = o.dw.clone()
    o.wbuf[:o.wf] = float("nan")
    o.dbuf[:o.n] = float("nan")
    assert o.launch() == 0
    assert torch.equal(o.dw, first) and o.guards_intact()


@gpu
@pytest.mark.parametrize("cid", ["A", "B"])
def test_workspace_clamps_the_split(H, cid):
    """A workspace of three copies: the split clamps to 3, nothing is written behind the third copy, the result is within the bound."""
    n = geom(CASES[cid])[5]
    o = Owned(H, cid, 3 * n)
    assert o.launch() == 0
    check(o.dw, o.d, f"{cid} three copies", 3)
    assert o.guards_intact()
    assert torch.isfinite(o.wbuf[:3 * n]).all()            # and all three copies were used
    # not a whole number of copies: 2 n + n / 2 floats hold two
    o2 = Owned(H, cid, 3 * n)
    o2.wbuf[2 * n:] = SENTINEL
    assert o2.launch(work_floats=2 * n + n // 2) == 0
    check(o2.dw, o2.d, f"{cid} two copies and a half", 2)
    assert o2.guards_intact(2 * n)


@gpu
@pytest.mark.parametrize("cid", ["A", "B"])
def test_workspace_errors(H, cid):
    """One float less than a copy, or a workspace off a 16-byte boundary: an error with a message, and neither dw nor the workspace is
    touched."""
    from vspbfr_amd import _lib
    n = geom(CASES[cid])[5]
    o = Owned(H, cid, 2 * n, poison=SENTINEL, dw_fill=SENTINEL)
    assert o.launch(work_floats=n - 1) != 0
    assert "workspace holds" in _lib.last_error() and str(n) in _lib.last_error()
    with pytest.raises(RuntimeError, match="workspace holds"):
        H.check(o.launch(work_floats=n - 1), "conv2d_wgrad")
    assert o.launch(work_offset=1) != 0
    assert "16-byte aligned" in _lib.last_error()
    assert o.guards_intact(0) and bool((o.dbuf == SENTINEL).all())
    assert o.launch() == 0                                  # the same block, whole and aligned, runs
    check(o.dw, o.d, f"{cid} after refused calls", 2)


@gpu
@pytest.mark.parametrize("cid", ["A", "B"])
def test_workspace_accumulate(H, cid):
    """accumulate on both reducers through the C entry (A: sliced, B: plain with its scalar tail): dw0 + ref."""
    c = CASES[cid]
    split = planned_split(H.lib, c)
    o = Owned(H, cid, split * geom(c)[5])
    o.dbuf[:o.n] = dev(o.d["dw0"]).reshape(-1)
    assert o.launch(accumulate=True) == 0
    check(o.dw, o.d, f"{cid} accumulate, poisoned workspace", split, dw0=o.d["dw0"])
    assert o.guards_intact()


# ------------------------------------------------------------------------------------------------ atomics
@gpu
@pytest.mark.parametrize("cid", ["A", "B", "E", "K", "FEW"])
def test_atomic_route(H, cid, monkeypatch):
    """hip_ops.WGRAD_WORKSPACE = False: fp32 atomics into dw.  `out` arrives full of NaN, so the entry's memset is what makes the result
    finite; accumulate adds onto dw0.  (No bit equality here: the order of the atomics is not fixed.)"""
    monkeypatch.setattr(H, "WGRAD_WORKSPACE", False)
    c, d = CASES[cid], data(cid)
    n = geom(c)[5]
    buf = torch.full((n + GUARD,), float("nan"), device=DEV)
    buf[n:] = SENTINEL
    out = buf[:n].view(c["G"] * c["cout_g"], c["cin_g"], c["k"], c["k"])
    dw = run_wrapper(H, cid, d, out=out)
    assert dw.data_ptr() == buf.data_ptr()
    check(dw, d, f"{cid} atomics", 0)
    dw2 = run_wrapper(H, cid, d, out=dev(d["dw0"]), accumulate=True)
    check(dw2, d, f"{cid} atomics accumulate", 0, dw0=d["dw0"])
    assert bool((buf[n:] == SENTINEL).all())


@gpu
def test_fewin_small_workspace_falls_back_to_atomics(H):
    """The stream form with a workspace of one copy where it needs B = 3: it adds with atomics instead, so it must zero dw itself
    (accumulate = False) or leave dw0 in it (accumulate = True), and it does not touch the workspace."""
    c = CASES["FEW"]
    n = geom(c)[5]
    assert planned_split(H.lib, c) == 3
    o = Owned(H, "FEW", n, poison=SENTINEL)
    assert o.launch() == 0
    check(o.dw, o.d, "FEW one-copy workspace", 0)
    o.dbuf[:n] = dev(o.d["dw0"]).reshape(-1)
    assert o.launch(accumulate=True) == 0
    check(o.dw, o.d, "FEW one-copy workspace, accumulate", 0, dw0=o.d["dw0"])
    assert o.guards_intact(0)
    # and with all three copies: the workspace form, repeatable
    o3 = Owned(H, "FEW", 3 * n)
    assert o3.launch() == 0
    check(o3.dw, o3.d, "FEW poisoned workspace", 3)
    first = o3.dw.clone()
    o3.dbuf[:n] = float("nan")
    assert o3.launch() == 0
    assert torch.equal(o3.dw, first) and o3.guards_intact()


# ------------------------------------------------------------------------------------------------ the input channel window
@gpu
@pytest.mark.parametrize("cid", ["W", "K", "FEW"])
@pytest.mark.parametrize("workspace", [True, False])
def test_input_window(H, cid, workspace, monkeypatch):
    """x_coff = 5 into an x with 5 more channels in front and 3 behind (values and per-sample scales of their own): true groups, the
    shared input of the four dilations, the stream form.  The scale is indexed by the channel of the whole tensor."""
    monkeypatch.setattr(H, "WGRAD_WORKSPACE", workspace)
    c, d = CASES[cid], data(cid, True)
    split = planned_split(H.lib, c)
    assert split == c["split"]
    assert d["x"].shape[1] == X_LEAD + geom(c)[4] + X_TRAIL and d["xs"].shape == d["x"].shape[:2]
    dw = run_wrapper(H, cid, d, x_coff=X_LEAD)
    check(dw, d, f"{cid} window, {'workspace' if workspace else 'atomics'}", split if workspace else 0)
    if workspace:
        # a window that overruns x: refused by the wrapper and by the entry
        with pytest.raises(RuntimeError, match="do not match"):
            run_wrapper(H, cid, d, x_coff=X_LEAD + X_TRAIL + 1)
        run_wrapper(H, cid, d, x_coff=X_LEAD + X_TRAIL)            # the last window that fits
        from vspbfr_amd import _lib
        o = Owned(H, cid, split * geom(c)[5], dw_fill=SENTINEL)
        t = {k: dev(d[k]) for k in ("x", "gy", "xs", "dys")}
        p = fill_params(c, t["x"].data_ptr(), t["gy"].data_ptr(), o.dbuf.data_ptr(), t["xs"].data_ptr(), t["dys"].data_ptr(),
                        x_ch=d["x"].shape[1], x_coff=X_LEAD + X_TRAIL + 1, work=o.wbuf.data_ptr(), work_floats=o.wf)
        assert H.lib.vsp_conv2d_wgrad_f32(C.byref(p), H._stream()) != 0
        assert "channel window exceeds" in _lib.last_error()
        torch.cuda.synchronize()
        assert bool((o.dbuf == SENTINEL).all())


# ------------------------------------------------------------------------------------------------ edges
@gpu
@pytest.mark.parametrize("workspace", [True, False])
def test_empty_batch(H, workspace, monkeypatch):
    """B = 0: accumulate leaves dw as it is, bit for bit; without it dw is zero.  Through the wrapper on both routes, and through the C
    entry with a workspace in hand."""
    monkeypatch.setattr(H, "WGRAD_WORKSPACE", workspace)
    for cid in ("B", "FEW"):
        c, d = CASES[cid], data(cid)
        e = {k: d[k][:0] for k in ("x", "xs", "gy", "dys")}
        dw0 = dev(d["dw0"])
        got = run_wrapper(H, cid, e, out=dw0.clone(), accumulate=True)
        assert torch.equal(got, dw0)
        got = run_wrapper(H, cid, e, out=torch.full_like(dw0, float("nan")))
        assert got.shape == dw0.shape and not got.any()
        if workspace:
            n = geom(c)[5]
            o = Owned(H, cid, n, poison=SENTINEL)
            p = fill_params(c, None, None, o.dbuf.data_ptr(), work=o.wbuf.data_ptr(), work_floats=n, B=0)
            assert H.lib.vsp_conv2d_wgrad_f32(C.byref(p), H._stream()) == 0
            torch.cuda.synchronize()
            assert not o.dw.any() and o.guards_intact(0)
            o.dbuf[:n] = dw0.reshape(-1)
            p.accumulate = 1
            assert H.lib.vsp_conv2d_wgrad_f32(C.byref(p), H._stream()) == 0
            torch.cuda.synchronize()
            assert torch.equal(o.dw, dw0.reshape(-1)) and o.guards_intact(0)


@gpu
@pytest.mark.parametrize("workspace", [True, False])
def test_refused_geometry_writes_nothing(H, workspace, monkeypatch):
    """Geometry the staging layout cannot hold is an error, on either route, and dw keeps its contents: dilation 64 on a 70-wide map
    (147 quads), per-group geometry for 5 groups, rows of 3 pixels."""
    from vspbfr_amd import _lib
    monkeypatch.setattr(H, "WGRAD_WORKSPACE", workspace)
    g_ = torch.Generator().manual_seed(5)
    x, gy = dev(torch.randn(2, 16, 8, 70, generator=g_)), dev(torch.randn(2, 16, 8, 70, generator=g_))
    out = torch.full((16, 16, 3, 3), SENTINEL, device=DEV)
    with pytest.raises(RuntimeError, match="too wide for the staging layout"):
        H.conv2d_wgrad(x, gy, (16, 16, 3, 3), 1, 64, 64, out=out)
    torch.cuda.synchronize()
    assert bool((out == SENTINEL).all())
    H.conv2d_wgrad(x, gy, (16, 16, 3, 3), 1, 48, 48, out=out)            # (dilation 48 on the same map is served: case G48)
    assert torch.isfinite(out).all() and not bool((out == SENTINEL).any())
    served = out.clone()
    # five groups with a dilation each: the wrapper refuses, and so does the entry
    x5, gy5 = dev(torch.randn(2, 16, 8, 16, generator=g_)), dev(torch.randn(2, 5 * 16, 8, 16, generator=g_))
    out5 = torch.full((5 * 16, 16, 3, 3), SENTINEL, device=DEV)
    with pytest.raises(RuntimeError, match="at most 4 groups"):
        H.conv2d_wgrad(x5, gy5, (5 * 16, 16, 3, 3), 1, (1,) * 5, (1,) * 5, 5, x_shared=True, out=out5)
    c5 = case(2, 16, 16, (8, 16), 3, 1, (1,) * 5, (1,) * 5, 0, G=5, shared=True)
    p = fill_params(c5, x5.data_ptr(), gy5.data_ptr(), out5.data_ptr())
    assert H.lib.vsp_conv2d_wgrad_f32(C.byref(p), H._stream()) != 0
    assert "at most 4 groups" in _lib.last_error()
    torch.cuda.synchronize()
    assert bool((out5 == SENTINEL).all())
    # W = 3
    x3, gy3 = dev(torch.randn(2, 16, 8, 3, generator=g_)), dev(torch.randn(2, 16, 8, 3, generator=g_))
    with pytest.raises(RuntimeError, match="shorter than 4 pixels"):
        H.conv2d_wgrad(x3, gy3, (16, 16, 3, 3), 1, 1, 1, out=out)
    torch.cuda.synchronize()
    assert torch.equal(out, served)
