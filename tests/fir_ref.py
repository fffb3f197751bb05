"""Float64 restatement of upfirdn2d and its fused epilogue (csrc/upfirdn2d.hip), the case table that tests/test_fir_ref.py (CPU) and
tests/test_fir_forms_gpu.py (GPU) share, the one bound both use, and a restatement of the dispatch of `upfirdn2d_impl` that names the
compiled form a case reaches.

Every function is written from the operation's definition (the header comment of csrc/upfirdn2d.hip, include/vspbfr_hip.h, the fp32
statement oracle/ops.py:37-55), takes CPU tensors and a `dtype` and evaluates everything in that dtype: float64 is the reference, float32
is `ref32`, whose distance from float64 is the `e_ref` of `bound`.  `variant` selects a deliberately WRONG statement (the teeth of
test_fir_ref.py); None is the definition.  No device code and no import of the package here."""
import math
import zlib
from collections import namedtuple

import torch

SQRT2 = math.sqrt(2.0)
SLOPE = 0.2
NOISE_W = 0.37
F64, F32 = torch.float64, torch.float32

VARIANTS = ("noflip", "transpose", "sep_swap", "swap_pad", "scale_by_channel", "noise_by_plane", "bias_after_act", "res_before_act",
            "gain_pos_only")
TAP_VARIANTS = ("noflip", "transpose", "sep_swap", "swap_pad")


# ------------------------------------------------------------------------------------------------------------------ the operation
def upfirdn2d(x, k, up=(1, 1), down=(1, 1), pad4=(0, 0, 0, 0), dtype=F64, variant=None, order="2d"):
    """x [major, H, W, minor], k [kh, kw], up = (up_x, up_y), down = (down_x, down_y), pad4 = (pad_x0, pad_x1, pad_y0, pad_y1):
        1. zero insertion   U[s, t] = x[s / up_y, t / up_x] where both divide, else 0
        2. pad; a negative pad crops
        3. true convolution: out[oy, ox] = sum_{ky, kx} k[kh - 1 - ky][kw - 1 - kx] P[oy + ky, ox + kx]
        4. keep every down-th sample
    order "sep" (outer-product taps only) evaluates step 3 as the strip kernel's separable form does: with f the flipped taps,
    tx = f[0, :], ty = f[:, 0] / f[0, 0], a row pass sum_kx tx[kx] P[., ox + kx] and then a column pass over the row sums.
    variants: "noflip" (k[ky][kx]), "transpose" (k[kx][ky], square taps), "sep_swap" (tx and ty exchanged in the separable evaluation),
    "swap_pad" (the window offset of x taken from pad_y0 and that of y from pad_x0; the output size stays the host's)."""
    x, k = x.detach().to(dtype), k.detach().to(dtype)
    up_x, up_y = up
    down_x, down_y = down
    px0, px1, py0, py1 = pad4
    if variant == "swap_pad":
        px0, px1, py0, py1 = py0, px0 + px1 - py0, px0, py0 + py1 - px0
    major, H, W, minor = x.shape
    kh, kw = k.shape
    z = torch.zeros(major, H * up_y, W * up_x, minor, dtype=dtype)
    z[:, ::up_y, ::up_x] = x
    z = torch.nn.functional.pad(z, [0, 0, max(px0, 0), max(px1, 0), max(py0, 0), max(py1, 0)])
    z = z[:, max(-py0, 0): z.shape[1] - max(-py1, 0), max(-px0, 0): z.shape[2] - max(-px1, 0)]
    oh, ow = z.shape[1] - kh + 1, z.shape[2] - kw + 1
    if oh < 0 or ow < 0:
        raise ValueError(f"negative output size {oh}x{ow}")
    if variant == "transpose" and kh == kw:
        k = k.t()
    f = k if variant == "noflip" else k.flip(0, 1)
    if order == "sep" or variant == "sep_swap":
        tx, ty = f[0, :], f[:, 0] / f[0, 0]
        if variant == "sep_swap":
            tx, ty = f[:, 0], f[0, :] / f[0, 0]
        rows = torch.zeros(major, z.shape[1], ow, minor, dtype=dtype)
        for kx in range(kw):
            rows = rows + tx[kx] * z[:, :, kx:kx + ow]
        out = torch.zeros(major, oh, ow, minor, dtype=dtype)
        for ky in range(kh):
            out = out + ty[ky] * rows[:, ky:ky + oh]
    else:
        out = torch.zeros(major, oh, ow, minor, dtype=dtype)
        for ky in range(kh):
            for kx in range(kw):
                out = out + f[ky, kx] * z[:, ky:ky + oh, kx:kx + ow]
    return out[:, ::down_y, ::down_x].contiguous()


def upfirdn2d_nchw(x, k, up=(1, 1), down=(1, 1), pad4=(0, 0, 0, 0), dtype=F64, variant=None, order="2d"):
    """the same on [B, C, H, W] (every plane on its own: major = B C, minor = 1)"""
    B, Cc, H, W = x.shape
    y = upfirdn2d(x.reshape(B * Cc, H, W, 1), k, up, down, pad4, dtype, variant, order)
    return y.view(B, Cc, y.shape[1], y.shape[2])


def epilogue(v, plane_scale=None, noise=None, noise_w=None, act_bias=None, act=False, slope=SLOPE, gain=SQRT2, res1=None, res2=None,
             channels=1, dtype=F64, variant=None):
    """v [major, oh, ow] with plane = b channels + c, in the order of `epi_apply` (include/vspbfr_hip.h):
        v = v plane_scale[plane] + noise[b] noise_w;  if act: v = lrelu(v + act_bias[c], slope) gain;  v = v + res1 + res2
    act_bias is ignored without act.
    variants: "scale_by_channel" (plane_scale[c]), "noise_by_plane" (noise[plane mod B]), "bias_after_act", "res_before_act",
    "gain_pos_only" (the gain on the positive side only)."""
    c = lambda t: None if t is None else t.detach().to(dtype)      # noqa: E731
    v = v.to(dtype)
    major = v.shape[0]
    B = major // channels
    plane = torch.arange(major)
    ch, b = plane % channels, plane // channels
    if plane_scale is not None:
        ps = c(plane_scale).reshape(-1)
        v = v * ps[ch if variant == "scale_by_channel" else plane].view(major, 1, 1)
    if noise is not None:
        nz = c(noise).reshape(B, v.shape[1], v.shape[2])
        v = v + nz[plane % B if variant == "noise_by_plane" else b] * c(noise_w).reshape(())
    if variant == "res_before_act":
        for t in (res1, res2):
            if t is not None:
                v = v + c(t).reshape(v.shape)
    if act:
        bias = torch.zeros(major, 1, 1, dtype=dtype) if act_bias is None else c(act_bias)[ch].view(major, 1, 1)
        if variant != "bias_after_act":
            v = v + bias
        if variant == "gain_pos_only":
            v = torch.where(v > 0, v * gain, v * slope)
        else:
            v = torch.where(v > 0, v, v * slope) * gain
        if variant == "bias_after_act":
            v = v + bias
    if variant != "res_before_act":
        for t in (res1, res2):
            if t is not None:
                v = v + c(t).reshape(v.shape)
    return v


# ------------------------------------------------------------------------------------------------------------------ the bound
def bound(got, ref64, ref32, bf16=False, what=""):
    """The project's rule (stream_ref.bound, tests/test_tacc_kernels.py):
        max |got - ref64| <= 4 e_ref + 2e-6 max |ref64|,   e_ref = max |ref32 - ref64|,
    ref32 = the same restatement run in float32 on the CPU; nothing in it comes from a kernel.  A bf16 output is held per element to
        |got - ref64| <= 2^-8 |ref64| + 4 e_ref + 2e-6 max |ref64|
    (2^-8: half a unit of an 8-bit significand, relative to the value at the least).  Prints and returns (e_ref, e_hip, ratio), e_hip
    being what remains of the error beyond the bf16 term; AssertionError when the bound is missed or `got` is not finite / of another
    shape."""
    got = got.detach().cpu().double()
    ref64 = ref64.detach().double()
    assert got.shape == ref64.shape, f"{what}: shape {tuple(got.shape)} != {tuple(ref64.shape)}"
    assert bool(torch.isfinite(got).all()), f"{what}: not finite"
    if ref64.numel() == 0:
        return 0.0, 0.0, float("nan")
    e_ref = float((ref32.detach().double() - ref64).abs().max())
    err = (got - ref64).abs()
    if bf16:
        err = (err - 2.0 ** -8 * ref64.abs()).clamp_min(0.0)
    e_hip = float(err.max())
    tol = 4 * e_ref + 2e-6 * float(ref64.abs().max())
    ratio = e_hip / e_ref if e_ref else float("nan")
    print(f"FIR {what}: e_ref={e_ref:.3e} e_hip={e_hip:.3e} ratio={ratio:.2f} tol={tol:.3e}")
    if e_hip > tol:
        worst = [int(i) for i in torch.unravel_index(err.argmax(), err.shape)]
        raise AssertionError(f"{what}: max|d|={e_hip:.3e} tol={tol:.3e} (e_ref {e_ref:.3e}) at {worst} of {list(err.shape)}, "
                             f"{int((err > tol).sum())} elements beyond the bound")
    return e_ref, e_hip, ratio


def round_bf16(t):
    return t.to(torch.bfloat16).to(F32)


# ------------------------------------------------------------------------------------------------------------------ taps
def taps_separable(k):
    """the predicate of hip_ops.taps_separable: the FLIPPED taps are exactly (first column / corner) x (first row) in float32, the
    corner -- the last tap of the caller's matrix -- not zero"""
    f = k.detach().float().flip(0, 1)
    return bool(float(f[0, 0]) != 0.0 and torch.equal(f, ((f[:, :1] / f[0, 0]) * f[:1, :]).float()))


def _rand_taps(kh, kw, seed):
    return torch.randn(kh, kw, generator=torch.Generator().manual_seed(seed)) * 0.3


def _outer(a, b, div):
    return torch.outer(torch.tensor(a, dtype=F32), torch.tensor(b, dtype=F32)) / div


TAPS = {
    "asym4": _outer([1, 2, 4, 8], [1, 3, 5, 7], 256.0),      # an outer product that is neither symmetric nor its own flip (all dyadic)
    "blur4": _outer([1, 3, 3, 1], [1, 3, 3, 1], 16.0),       # the path's make_kernel([1, 3, 3, 1]) * 4
    "zero4": _outer([1, 3, 3, 0], [1, 3, 3, 0], 49.0),       # an outer product whose last tap is zero: must run in the 2-D form
    "rand4": _rand_taps(4, 4, 44),
    "rand3": _rand_taps(3, 3, 33),
    "rand2": _rand_taps(2, 2, 22),
    "rand3x5": _rand_taps(3, 5, 35),
}
SEPARABLE_TAPS = {"asym4": True, "blur4": True, "zero4": False, "rand4": False, "rand3": False, "rand2": False, "rand3x5": False}

EPI = {
    "none": (),
    "ps": ("plane_scale",),
    "nz": ("noise",),
    "r2": ("res2",),
    "ps_nz_r1": ("plane_scale", "noise", "res1"),
    "act_nobias": ("plane_scale", "act", "res1"),
    "full": ("plane_scale", "noise", "act_bias", "act", "res1", "res2"),
}
SUBSETS = ("none", "ps", "nz", "r2", "ps_nz_r1", "full")


# ------------------------------------------------------------------------------------------------------------------ the dispatch
FORM_NAMES = (["strip/%s/%s" % (s, e) for s in ("sep", "2d") for e in ("plain", "en", "en/act")] +
              ["strip/sep/plain+tail", "strip/2d/plain+tail", "strip/major1", "tile4/bf16/unaligned", "tile4/bf16/split-word"] +
              ["tile%d/%s" % (n, t) for n in (2, 3, 4) for t in ("f32", "bf16")] + ["generic", "generic/epi", "enotsup", "einval", "empty"])
TOW, TOH, RC = 64, 32, 32


def out_size(in_h, in_w, kh, kw, up, down, pads):
    return ((in_h * up[1] + pads[2] + pads[3] - kh + down[1]) // down[1], (in_w * up[0] + pads[0] + pads[1] - kw + down[0]) // down[0])


def form(dtype, major, in_h, in_w, kh, kw, up, down, pads, minor, epi_flags=None, alignments=None):
    """Which kernel form `upfirdn2d_impl` launches (csrc/upfirdn2d.hip), restated condition by condition.  dtype "f32" / "bf16";
    up = (up_x, up_y), down likewise, pads = (x0, x1, y0, y1); epi_flags None (no epilogue structure) or a dict {operands: the set of
    operand names given, act, separable, channels, noise_w}; alignments {"out" / "res1" / "res2" / "noise": address mod 16} (absent: 0).
    A restatement checked by reading; its only use is the coverage assertion of tests/test_fir_ref.py."""
    al = alignments or {}
    out_h, out_w = out_size(in_h, in_w, kh, kw, up, down, pads)
    if min(major, in_h, in_w, minor) < 0 or kh < 1 or kw < 1 or kh * kw > 1024 or min(up + down) < 1 or out_h < 0 or out_w < 0:
        return "einval"
    if major * out_h * out_w * minor == 0:
        return "empty"
    enabled = act = sep = False
    ops = set()
    if epi_flags is not None:
        ops = set(epi_flags.get("operands", ()))
        ch = epi_flags.get("channels", 1)
        if minor != 1 or ch < 1 or major % ch != 0 or ("noise" in ops and not epi_flags.get("noise_w", True)):
            return "einval"
        act = bool(epi_flags.get("act"))
        sep = bool(epi_flags.get("separable"))
        enabled = bool(ops & {"plane_scale", "noise", "res1", "res2"}) or act
    tile_ok = up == (1, 1) and down == (1, 1) and minor == 1 and out_w >= 16 and in_w >= 4 and in_h >= 1
    if dtype == "bf16":
        xb, ob = major * in_h * in_w * 2, major * out_h * out_w * 2
        ragged = out_w % 8 != 0
        geometry = (tile_ok and kh == 4 and kw == 4 and (not ragged or not enabled) and out_h >= 4 and xb < 0x7ffffff0 and ob < 0x7ffffff0 and
                    pads[0] <= in_h * in_w)
        if geometry and (in_w + pads[0]) % 2 != 0:
            return "tile4/bf16/split-word"                  # the tensor's last element would share a dword with two bytes past the end
        aligned = (ragged or al.get("out", 0) == 0) and all(al.get(n, 0) == 0 for n in ("res1", "res2", "noise") if n in ops)
        strips_x, chunks_y = out_w // 8, (out_h + RC - 1) // RC
        if geometry and not aligned:
            return "tile4/bf16/unaligned"
        if geometry and (major - 1) * chunks_y * strips_x < 2 ** 31:
            if major == 1:
                return "strip/major1"                       # plane 0 alone: the tile kernel on one plane, no strip launch
            name = "strip/" + ("sep" if sep else "2d") + "/" + ("plain" if not enabled else "en/act" if act else "en")
            return name + ("+tail" if ragged else "")
    if tile_ok and kh == kw and kh in (2, 3, 4):
        return "tile%d/%s" % (kh, dtype)
    if dtype == "bf16":
        return "enotsup"
    return "generic/epi" if enabled else "generic"


def family(name):
    """the kernel a form name belongs to (a strip case runs the tile kernel on plane 0 as well)"""
    if name.startswith("strip"):
        return "strip"
    if name.startswith("tile"):
        return "tile/" + ("bf16" if "bf16" in name else "f32")
    return "generic" if name.startswith("generic") else name


# ------------------------------------------------------------------------------------------------------------------ the cases
Case = namedtuple("Case", "name entry dtype B C H W minor taps up down pad epi force2d misalign refuse")
"""entry "blur": hip_ops.blur_fused on [B, C, H, W] with pad = (p0, p1) on both axes; "native": hip_ops.upfirdn2d_native_layout on
[B C, H, W, minor] with pad = (x0, x1, y0, y1) and an epilogue structure of the test's own (epi None: no structure).  force2d: run with
hip_ops.SEPARABLE_BLUR = False.  misalign: {operand: bytes} -- the operand is a view that starts so many bytes into its storage.  refuse:
None, or what makes the call a RuntimeError ("noise_w": noise without noise_w; "channels": channels = C + 1 not dividing major)."""


def _case(name, entry, dtype, shape, taps, pad, epi="none", up=(1, 1), down=(1, 1), minor=1, force2d=False, misalign=None, refuse=None):
    B, Cc, H, W = shape
    return Case(name, entry, dtype, B, Cc, H, W, minor, taps, up, down, tuple(pad), epi, force2d, misalign or {}, refuse)


def _build_cases():
    cs = []
    add = lambda *a, **kw: cs.append(_case(*a, **kw))      # noqa: E731
    # bf16 strip walk: 4 x 16 is the smallest plane it takes; 33 x 24 has a second 32-row chunk of one row and an odd input width;
    # 33 x 20 / 34 x 18 / 34 x 25 have tails of 4 / 2 / 1 columns (with an epilogue those rows fall to the tile kernel); major = 1
    # leaves plane 0 alone, which is the tile kernel's.  Each output size twice: with in_w + pad even (the strip walk) and odd (the
    # walk would lose the tensor's last element to the dword range check: the dispatch hands those to the tile kernel)
    strip_shapes = [((2, 3, 5, 17), (1, 1)), ((2, 3, 3, 15), (2, 2)), ((2, 3, 34, 25), (1, 1)), ((2, 3, 34, 21), (1, 1)), ((1, 1, 40, 30), (2, 2)),
                    ((2, 2, 35, 19), (1, 1)), ((2, 2, 33, 17), (2, 2)), ((2, 5, 33, 24), (2, 2)), ((2, 5, 35, 26), (1, 1))]
    for shape, pad in strip_shapes:
        tag = "%dx%dx%dx%d" % shape
        for taps, forms, subsets in (("asym4", (False, True), SUBSETS), ("blur4", (False, True), ("none", "full")),
                                     ("rand4", (False,), ("none", "full"))):
            for f2 in forms:
                for e in subsets:
                    add(f"strip-{tag}-{taps}-{'2d' if f2 else 'sep'}-{e}", "blur", "bf16", shape, taps, pad, e, force2d=f2)
    add("strip-2x3x34x25-asym4-sep-act_nobias", "blur", "bf16", (2, 3, 34, 25), "asym4", (1, 1), "act_nobias")
    add("strip-2x3x34x25-asym4-2d-act_nobias", "blur", "bf16", (2, 3, 34, 25), "asym4", (1, 1), "act_nobias", force2d=True)
    # an operand that is not 16-byte aligned: the strip walk's 16-byte operand loads are refused, the tile kernel serves the call
    add("unaligned-res1", "blur", "bf16", (2, 3, 34, 25), "asym4", (1, 1), "ps_nz_r1", misalign={"res1": 2})
    add("unaligned-noise", "blur", "bf16", (2, 3, 34, 25), "asym4", (1, 1), "full", misalign={"noise": 4})
    # the zero-corner outer product: the host gate must leave it in the 2-D form
    for e in ("none", "full"):
        add(f"zero-corner-{e}", "blur", "bf16", (2, 3, 39, 33), "zero4", (1, 1), e)
    # crop and asymmetric pads through the native entry, fp32 (tile kernel) and bf16 (strip + tail; 72 columns: whole strips)
    for dt in ("f32", "bf16"):
        for pad in ((-1, 2, 1, -2), (2, 1, 2, 1), (0, 3, 3, 0), (4, 1, 1, -2), (-2, 3, 1, -2)):
            add(f"pads-{dt}-{'_'.join(map(str, pad))}", "native", dt, (3, 1, 40, 70), "rand4", pad, None)
        add(f"pads-{dt}-epi", "native", dt, (2, 3, 40, 70), "asym4", (4, 1, 1, -2), "full")
        add(f"pads-{dt}-k3", "native", dt, (3, 1, 40, 70), "rand3", (-1, 2, 2, 0), None)
    # tile kernel: 72 x 200 planes have an interior window (tile (1, 1)), tile_inside tiles and border tiles at once
    for dt, tapsets in (("f32", ("rand4", "rand3", "rand2")), ("bf16", ("rand3", "rand2"))):
        for taps in tapsets:
            kk = int(taps[-1])
            for e in SUBSETS:
                add(f"tile-{dt}-{taps}-p11-{e}", "blur", dt, (2, 3, 72, 200), taps, (1, 1), e)
                add(f"tile-{dt}-{taps}-p22-{e}", "blur", dt, (2, 3, 72, 200), taps, (2, 2), e)
                add(f"tile-{dt}-{taps}-p21-{e}", "native", dt, (2, 3, 72, 200), taps, (2, 1, 2, 1), e)
            # the narrow end: 5 x 16 and 5 x 17 outputs
            for ow in (16, 17):
                for e in ("none", "full"):
                    add(f"tile-{dt}-{taps}-5x{ow}-{e}", "native", dt, (2, 3, 5 + kk - 1 - 2, ow + kk - 1 - 2), taps, (1, 1, 1, 1), e)
    add("tile-f32-asym4-p11-full", "blur", "f32", (2, 3, 72, 200), "asym4", (1, 1), "full")
    # generic kernel: every fused blur on maps narrower than 16, and every up / down / minor > 1
    for hw in (8, 4):
        for e in ("none", "ps_nz_r1", "full"):
            add(f"generic-{hw}-rand4-{e}", "blur", "f32", (2, 3, hw, hw), "rand4", (2, 1), e)
        add(f"generic-{hw}-rand3-full", "blur", "f32", (2, 3, hw, hw), "rand3", (1, 1), "full")
        add(f"generic-{hw}-asym4-full", "blur", "bf16", (2, 3, hw, hw), "asym4", (2, 1), "full")     # bf16 callers convert
    add("generic-minor3", "native", "f32", (2, 1, 7, 10), "rand3x5", (2, 1, 0, 3), None, up=(2, 3), down=(3, 2), minor=3)
    add("generic-up2", "native", "f32", (1, 3, 8, 9), "blur4", (2, 1, 2, 1), None, up=(2, 2))
    add("generic-up2-rand4", "native", "f32", (1, 3, 8, 9), "rand4", (2, 1, 2, 1), None, up=(2, 2))
    add("generic-down2", "native", "f32", (1, 2, 16, 17), "rand4", (1, 1, 1, 1), None, down=(2, 2))
    # planes narrower than the tile kernel's four-element loads, under wide pads: generic kernel (bf16 callers convert), and a one-row
    # plane whose left pad exceeds a whole plane (no strip walk)
    for dt in ("f32", "bf16"):
        for e in ("none", "full"):
            add(f"narrow-in-{dt}-{e}", "blur", dt, (2, 3, 5, 3), "asym4", (8, 8), e)
    add("short-plane-bf16", "blur", "bf16", (2, 3, 1, 4), "asym4", (8, 8), "none")
    add("short-plane-f32", "blur", "f32", (2, 3, 1, 4), "asym4", (8, 8), "full")
    add("empty-output", "native", "f32", (2, 3, 8, 3), "rand4", (0, 0, 0, 0), None)       # out_w = 0: nothing is launched
    # refusals
    add("refuse-bf16-up2", "native", "bf16", (1, 3, 8, 8), "blur4", (2, 1, 2, 1), None, up=(2, 2), refuse="enotsup")
    add("refuse-bf16-narrow-in", "native", "bf16", (2, 3, 5, 3), "asym4", (8, 8, 8, 8), None, refuse="enotsup")
    add("refuse-epi-minor", "native", "f32", (2, 1, 8, 8), "rand4", (2, 1, 2, 1), "ps", minor=3, refuse="minor")
    add("refuse-channels", "native", "f32", (2, 3, 8, 8), "rand4", (2, 1, 2, 1), "ps", refuse="channels")
    add("refuse-noise-w", "native", "f32", (2, 3, 8, 8), "rand4", (2, 1, 2, 1), "nz", refuse="noise_w")
    return cs


CASES = _build_cases()
CASE_BY_NAME = {c.name: c for c in CASES}
assert len(CASE_BY_NAME) == len(CASES)


def pad4(case):
    return case.pad if len(case.pad) == 4 else (case.pad[0], case.pad[1], case.pad[0], case.pad[1])


def case_out_size(case):
    k = TAPS[case.taps]
    return out_size(case.H, case.W, k.shape[0], k.shape[1], case.up, case.down, pad4(case))


def converts_to_f32(case):
    """hip_ops.blur_fused runs a bf16 plane set the bf16 entry does not serve in fp32 (the values stay the bf16-rounded ones)"""
    k = TAPS[case.taps]
    ok = case.W >= 4 and case.H >= 1 and case_out_size(case)[1] >= 16 and tuple(k.shape) in ((4, 4), (3, 3), (2, 2))
    return case.entry == "blur" and case.dtype == "bf16" and not ok


def kernel_dtype(case):
    return "f32" if converts_to_f32(case) else case.dtype


def case_form(case):
    k = TAPS[case.taps]
    flags = None
    if case.epi is not None:
        ops = set(EPI[case.epi])
        flags = {"operands": ops - {"act"}, "act": "act" in ops, "channels": case.C + 1 if case.refuse == "channels" else case.C,
                 "noise_w": case.refuse != "noise_w",
                 "separable": case.entry == "blur" and not case.force2d and taps_separable(k)}
    al = dict(case.misalign)
    return form(kernel_dtype(case), case.B * case.C, case.H, case.W, k.shape[0], k.shape[1], case.up, case.down, pad4(case), case.minor,
                flags, al)


def inputs(case):
    """float32 CPU operands of a case: x [B C, H, W, minor], k, and the epilogue operands its subset names.  bf16 cases round x and the
    residuals to bf16 first (the kernels read exactly these values).  B != C and H != W in every family, plane_scale differs between
    the planes by up to 3x, bias and residuals are of the size of the blurred values."""
    g = torch.Generator().manual_seed(zlib.crc32(case.name.encode()) & 0x7fffffff)
    major = case.B * case.C
    rnd = round_bf16 if case.dtype == "bf16" else (lambda t: t)
    d = {"x": rnd(torch.randn(major, case.H, case.W, case.minor, generator=g)), "k": TAPS[case.taps].clone()}
    if case.epi is None:
        return d
    oh, ow = case_out_size(case)
    ops = EPI[case.epi]
    if "plane_scale" in ops:
        d["plane_scale"] = torch.rand(case.B, case.C, generator=g) * 1.0 + 0.5
    if "noise" in ops:
        d["noise"] = torch.randn(case.B, 1, oh, ow, generator=g)
        d["noise_w"] = torch.tensor([NOISE_W])
    if "act_bias" in ops:
        d["act_bias"] = torch.randn(case.C, generator=g)
    for r in ("res1", "res2"):
        if r in ops:
            d[r] = rnd(torch.randn(major, oh, ow, generator=g))
    d["act"] = "act" in ops
    return d


def reference(case, dtype=F64, variant=None, order="2d", ops=None):
    """the case's result in `dtype`: [B, C, oh, ow] for the blur entry, [B C, oh, ow, minor] for the native one"""
    d = inputs(case) if ops is None else ops
    v = upfirdn2d(d["x"], d["k"], case.up, case.down, pad4(case), dtype, variant if variant in TAP_VARIANTS else None, order)
    if case.epi is not None and case.minor == 1:
        e = {n: d.get(n) for n in ("plane_scale", "noise", "noise_w", "act_bias", "res1", "res2")}
        v = epilogue(v[..., 0], act=d["act"], channels=case.C, dtype=dtype, variant=variant, **e).unsqueeze(-1)
    if case.entry == "blur":
        return v.view(case.B, case.C, v.shape[1], v.shape[2])
    return v


def output_bf16(case):
    return kernel_dtype(case) == "bf16"
