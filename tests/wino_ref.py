"""A plain model of the Winograd convolutions F(2x2,3x3) and F(4x4,3x3) in a chosen floating-point type (numpy, CPU, nothing of the
project imported), the operand families and the launch table of the conditioning fence (tests/test_wino_fence_gpu.py), and its two
error measures.

The model answers one question: what does the ALGORITHM cost in float32 on these operands?  A kernel is then bounded against that cost
and not against the output range.  Every elementwise numpy operation rounds once, so a transform written as a left-to-right sum of
products is exactly a chain of float32 multiplies and adds (no contraction).

    U = G g G^T          summed in float64 and rounded once (what the weight kernels do)
    V = B^T d B          in `dtype`
    M = sum_ci U . V     in `dtype`, one input channel after another (the chain of fp32 MFMAs over the k-steps)
    Y = A^T M A          in `dtype`

A dilation d is d x d dense convolutions on the polyphase sub-images x[py::d, px::d] (conv_wino4f.hip / conv_wino_rs.hip headers)."""
import itertools
import math

import numpy as np
import torch
import torch.nn.functional as F

# finite interpolation points (infinity is implied) and the sign the kernels' headers give each row of G
F2 = dict(points=(0.0, 1.0, -1.0), row_sign=(-1.0, 1.0, 1.0))      # G = [[1,0,0],[.5,.5,.5],[.5,-.5,.5],[0,0,1]]  (include/vspbfr_hip.h)
F4 = dict(points=(0.0, 0.75, -0.75, 1.5, -1.5), row_sign=None)     # G = the Gm of tests/test_wino4f.py::test_winograd4f_weight_layout
U24 = 2.0 ** -24                                                     # unit roundoff of float32


def mats(points, row_sign=None):
    """(A^T, G, B^T) in float64 for F(m x m, 3 x 3) with n = len(points) + 1 = m + 2 interpolation points, the last one at infinity.
    A^T is the Vandermonde matrix of the points; row p of G is (1, p, p^2) / prod_{q != p} (p - q) (times row_sign[p]); B^T is SOLVED from
    the exactness condition  sum_p A^T[i, p] G[p, k] B^T[p, j] = [j == i + k]  (y_i = sum_k g_k d_{i + k} for every g and d)."""
    pts = np.asarray(points, dtype=np.float64)
    n, m = len(pts) + 1, len(pts) - 1
    AT = np.zeros((m, n))
    for i in range(m):
        AT[i, :n - 1] = pts ** i
    AT[m - 1, n - 1] = 1.0
    G = np.zeros((n, 3))
    for p in range(n - 1):
        den = np.prod([pts[p] - pts[q] for q in range(n - 1) if q != p])
        G[p] = np.array([1.0, pts[p], pts[p] ** 2]) / den * (1.0 if row_sign is None else row_sign[p])
    G[n - 1, 2] = 1.0
    K = np.zeros((m * 3, n))
    R = np.zeros((m * 3, n))
    for i in range(m):
        for k in range(3):
            K[3 * i + k] = AT[i] * G[:, k]
            R[3 * i + k, i + k] = 1.0
    BT = np.linalg.lstsq(K, R, rcond=None)[0]
    BT = np.round(BT * 2.0 ** 40) / 2.0 ** 40          # the solver's 1e-16 off the dyadic constants (and off the zeros, which _apply skips)
    assert np.abs(K @ BT - R).max() < 1e-12, "no exact B^T for these points"
    return AT, G, BT


def _apply(Mx, T, axis, dt):
    """out[i] = sum_j Mx[i, j] T[j] along `axis`: left to right, one rounding per multiply and per add, zero entries skipped."""
    T = np.moveaxis(T, axis, 0)
    out = []
    for i in range(Mx.shape[0]):
        acc = None
        for j in range(Mx.shape[1]):
            c = Mx[i, j]
            if c == 0.0:
                continue
            term = T[j] if c == 1.0 else (-T[j] if c == -1.0 else dt(c) * T[j])
            acc = term if acc is None else acc + term
        out.append(acc)
    return np.moveaxis(np.stack(out), 0, axis)


def _two_sided(Mx, T, dt, rows_first):
    """Mx T Mx^T on the last two axes"""
    a, b = (-2, -1) if rows_first else (-1, -2)
    return _apply(Mx, _apply(Mx, T, a, dt), b, dt)


# `order`: (channel permutation, transform order, accumulation)
#   permutation   "id" | "rev" | "rand": the order in which the input channels enter the sum
#   transform     "rows" | "cols": which axis of the tile B^T / A^T meets first
#   accumulation  "seq": M += U_ci V_ci, a multiply and an add per channel;  "bulk": one float32 matrix product per position (blocked, fused)
PLAIN = ("id", "rows", "seq")
ORDERS = tuple(itertools.product(("id", "rev", "rand"), ("rows", "cols"), ("seq", "bulk")))


def _perm(kind, cin):
    if kind == "id":
        return np.arange(cin)
    if kind == "rev":
        return np.arange(cin)[::-1].copy()
    return np.random.default_rng(cin).permutation(cin)


def _dense(x, U, AT, BT, dt, order):
    """one dense 3x3 / padding 1 convolution: x (B, Cin, H, W) in dt, U (Cout, Cin, n, n) in dt -> (B, Cout, H, W) in dt"""
    perm, tr, acc = order
    Bn, Cin, H, W = x.shape
    Cout = U.shape[0]
    m, n = AT.shape
    ty, tx = -(-H // m), -(-W // m)
    xp = np.zeros((Bn, Cin, m * ty + 2, m * tx + 2), dtype=dt)
    xp[:, :, 1:H + 1, 1:W + 1] = x
    d = np.lib.stride_tricks.sliding_window_view(xp, (n, n), axis=(-2, -1))[:, :, ::m, ::m]       # (B, Cin, ty, tx, n, n)
    V = _two_sided(BT, d, dt, tr == "rows").reshape(Bn, Cin, ty * tx, n * n)
    pm = _perm(perm, Cin)
    Uf = U.reshape(Cout, Cin, n * n)
    if acc == "seq":
        M = np.zeros((Bn, Cout, ty * tx, n * n), dtype=dt)
        for ci in pm:
            M += Uf[None, :, ci, None, :] * V[:, None, ci, :, :]
    else:
        Up = np.ascontiguousarray(Uf[:, pm].transpose(2, 0, 1))                                   # (nn, Cout, Cin)
        Vp = np.ascontiguousarray(V[:, pm].transpose(0, 3, 1, 2))                                 # (B, nn, Cin, T)
        M = np.matmul(Up[None], Vp).transpose(0, 2, 3, 1)                                         # (B, Cout, T, nn)
    Y = _two_sided(AT, np.ascontiguousarray(M).reshape(Bn, Cout, ty * tx, n, n), dt, tr == "rows")
    Y = Y.reshape(Bn, Cout, ty, tx, m, m).transpose(0, 1, 2, 4, 3, 5).reshape(Bn, Cout, ty * m, tx * m)
    return np.ascontiguousarray(Y[:, :, :H, :W])


def wino_conv(x, w, points=F4, dtype=np.float32, dilation=1, in_scale=None, fold="x", order=PLAIN):
    """The 3x3 / stride 1 / padding = dilation convolution of x (B, Cin, H, W) with w (Cout, Cin, 3, 3) by Winograd in `dtype`.
    `points`: F2 or F4.  `in_scale` (B, Cin) or (Cin,): the style scale, applied to x (fold = "x": one rounded multiply per input
    value, the F(2x2) kernels and the F(4x4) pair) or folded into the ROUNDED U (fold = "U": one more rounded multiply per weight,
    per sample -- the fused kernel folds it while it stages U)."""
    dt = np.dtype(dtype).type
    AT, G, BT = mats(**points)
    x = np.asarray(x, dtype=dt)
    U = np.einsum("ia,ocab,jb->ocij", G, np.asarray(w, dtype=np.float64), G).astype(dt)
    AT, BT = AT.astype(dt), BT.astype(dt)
    Bn, Cin, H, W = x.shape
    s = None
    if in_scale is not None:
        s = np.broadcast_to(np.asarray(in_scale, dtype=dt).reshape(-1, Cin), (Bn, Cin))
        if fold == "x":
            x, s = x * s[:, :, None, None], None
    y = np.empty((Bn, U.shape[0], H, W), dtype=dt)
    for b in (range(Bn) if s is not None else [slice(None)]):
        xb, yb = (x[b:b + 1], y[b:b + 1]) if s is not None else (x, y)
        Ub = U * s[b][None, :, None, None] if s is not None else U
        for py in range(dilation):
            for px in range(dilation):
                sub = xb[:, :, py::dilation, px::dilation]
                if sub.shape[2] and sub.shape[3]:
                    yb[:, :, py::dilation, px::dilation] = _dense(sub, Ub, AT, BT, dt, order)
    return y


def direct_conv_f32(x, w, dilation=1):
    """The control: F.conv2d in float32 on the CPU."""
    xt, wt = torch.as_tensor(np.asarray(x, dtype=np.float32)), torch.as_tensor(np.asarray(w, dtype=np.float32))
    return F.conv2d(xt, wt, padding=dilation, dilation=dilation).numpy()


def direct_conv_chain(x, w, dilation=1, chunk=32):
    """The control's named variant "chain": the direct convolution as ONE float32 fma chain per output over K = 9 Cin products, in the
    order conv_kernel.h's header gives for the direct kernel -- K walked in chunks of `chunk` input channels, per chunk tap after tap,
    per tap channel after channel, every step an exact fused multiply-add (v_mfma_f32_16x16x4_f32 is an exact fp32 fma chain).  The
    product of two float32 values is exact in float64, so float32(acc + w x) computed there is the fused operation."""
    x, w = np.asarray(x, dtype=np.float32), np.asarray(w, dtype=np.float32).astype(np.float64)
    Bn, Cin, H, W = x.shape
    d = dilation
    xp = np.zeros((Bn, Cin, H + 2 * d, W + 2 * d))
    xp[:, :, d:d + H, d:d + W] = x
    acc = np.zeros((Bn, w.shape[0], H, W), dtype=np.float32)
    for c0 in range(0, Cin, chunk):
        for ky in range(3):
            for kx in range(3):
                for ci in range(c0, min(Cin, c0 + chunk)):
                    acc = (acc + w[None, :, ci, ky, kx, None, None] * xp[:, None, ci, ky * d:ky * d + H, kx * d:kx * d + W]).astype(np.float32)
    return acc


def conv64(x, w, dilation=1):
    return F.conv2d(torch.as_tensor(np.asarray(x, dtype=np.float64)), torch.as_tensor(np.asarray(w, dtype=np.float64)), padding=dilation,
                    dilation=dilation).numpy()


# ------------------------------------------------------------------------------------------------ operand families and the launch table
FAMILIES = ("control", "dc", "postact", "style", "smallout")
SQRT2 = math.sqrt(2.0)


class Case:
    """One launch of the fence: x (B, Cin, H, W), one weight (Cg, Cin, 3, 3) per dilation in `dils` (a dilation-group launch has several)."""

    def __init__(self, kernel, B, Cin, Cg, H, W, dils=(1,)):
        self.kernel, self.B, self.Cin, self.Cg, self.H, self.W, self.dils = kernel, B, Cin, Cg, H, W, tuple(dils)

    @property
    def id(self):
        return f"{self.kernel}-{self.B}x{self.Cin}x{self.H}x{self.W}-{len(self.dils)}x{self.Cg}-d{'.'.join(map(str, self.dils))}"


_F2_SHAPES = [(2, 64, 64, 32, 64, (1,)), (1, 40, 16, 37, 20, (1,)), (1, 64, 16, 64, 64, (1, 2, 4, 8))]
_F4P_SHAPES = [(2, 128, 64, 16, 32, (1,)), (1, 64, 64, 32, 32, (1,))]
_F4F_SHAPES = [(2, 64, 64, 32, 64, (1,)), (1, 40, 48, 16, 80, (1,)), (1, 64, 3, 32, 64, (1,)),
               (1, 32, 32, 64, 64, (2,)), (1, 32, 32, 64, 64, (4,)), (1, 32, 32, 128, 128, (8,)), (1, 128, 32, 64, 64, (1, 2, 4, 8))]
# (dilation 8 runs at 128^2: at 64^2 its sub-images are 8 x 8, two tiles a side and mostly padding -- the transforms then cost so little
#  that the accumulation decides, and the model's sequential and fused accumulations alone differ by 1.4x in rms, 2 .. 2.9x in the
#  maximum on every draw: no order-independent cost to bound a kernel against.  At 16 x 16 sub-images the spread is 1.2 .. 1.6x.)


def f2_form_serves(form, c):
    """The eligibility rules of the named F(2x2) forms (include/vspbfr_hip.h, conv_wino.hip wino_launch): 1 = task list, everything;
    2 = row owner, more than 16 channels per group and rows of whole 16-byte segments; 3 = register-resident U, Cin <= 64 and such rows."""
    quads = c.W % 4 == 0 and (c.H * c.W) % 4 == 0
    return form == 1 or (form == 2 and c.Cg > 16 and quads) or (form == 3 and c.Cin <= 64 and quads)


WINO_CASES = ([Case(f"f2-form{f}", *s) for f in (1, 2, 3) for s in _F2_SHAPES if f2_form_serves(f, Case("", *s))]
              + [Case("f4-pair", *s) for s in _F4P_SHAPES] + [Case("f4-fused", *s) for s in _F4F_SHAPES])
# the control runs on every distinct shape of the table
DIRECT_CASES = [Case("direct", *s) for s in dict.fromkeys(_F2_SHAPES + _F4P_SHAPES + _F4F_SHAPES)]
CASES = DIRECT_CASES + WINO_CASES
# families 1..3 once more with the StyledConv epilogue (noise, bias, leaky relu), on the first shape of every kernel
EPILOGUE_CASES = [next(c for c in CASES if c.kernel == k) for k in dict.fromkeys(c.kernel for c in CASES)]
EPILOGUE_FAMILIES = FAMILIES[:3]


def points_of(kernel):
    return None if kernel == "direct" else (F2 if kernel.startswith("f2") else F4)


CHAIN_FROM_CIN = 128


def control_of(case):
    """Which model bounds the direct kernel.  F.conv2d in float32 on the CPU blocks its reduction, so its error grows more slowly with K
    than a single accumulator's; the kernel is entitled to its chain (conv_kernel.h: one accumulator per output, K = 9 Cin fused steps).
    Through 64 input channels the two cost the same (kernel / CPU = 0.5 .. 1.3x on MI355X); at 128 the CPU form is 4 .. 5x below the chain
    and the kernel lies between them (2.2 .. 3.1x the CPU form on 128 -> 4 x 32, 0.6x the chain): that layer class is bounded against
    the chain, the rest against direct_conv_f32."""
    return direct_conv_chain if case.Cin >= CHAIN_FROM_CIN else direct_conv_f32


def fold_of(kernel):
    return "U" if kernel == "f4-fused" else "x"


# Reseeded rows: the float32 model's own E or S moved by more than 2x across its evaluation orders on the first draw of these operands
# (tests/test_wino_ref.py::test_model_spread_across_orders -- a maximum over ~1e5 outputs is heavy-tailed); the fence needs a row whose
# cost the model pins down, so such a row draws again.  (B, Cin, Cg, H, W, dilations, family, epilogue) -> draw
RESEED = {
    (1, 40, 16, 37, 20, (1,), "postact", False): 1, (1, 40, 16, 37, 20, (1,), "smallout", False): 5,
    (2, 128, 64, 16, 32, (1,), "dc", False): 1, (2, 128, 64, 16, 32, (1,), "dc", True): 2,
    (1, 64, 64, 32, 32, (1,), "dc", False): 1, (1, 64, 64, 32, 32, (1,), "smallout", False): 1,
    (2, 64, 64, 32, 64, (1,), "dc", False): 1, (2, 64, 64, 32, 64, (1,), "dc", True): 1, (2, 64, 64, 32, 64, (1,), "postact", True): 1,
    (1, 40, 48, 16, 80, (1,), "dc", False): 2, (1, 40, 48, 16, 80, (1,), "smallout", False): 4,
    (1, 64, 3, 32, 64, (1,), "dc", False): 2, (1, 64, 3, 32, 64, (1,), "style", False): 1,
    (1, 32, 32, 64, 64, (2,), "dc", False): 1, (1, 32, 32, 64, 64, (4,), "postact", False): 2,
    (1, 32, 32, 128, 128, (8,), "style", False): 1, (1, 128, 32, 64, 64, (1, 2, 4, 8), "smallout", False): 1,
}


def operands(case, family, epilogue=False):
    """The operands of one fence row as float32 torch tensors (seeded: the same on the CPU and the GPU box): x, ws (one per dilation),
    in_scale / out_scale (family "style" only), noise / noise_w / bias (with `epilogue` only)."""
    c = case
    draw = RESEED.get((c.B, c.Cin, c.Cg, c.H, c.W, c.dils, family, epilogue), 0)
    g_ = torch.Generator().manual_seed(100003 * draw + 1000 * FAMILIES.index(family) + 7 * c.Cin + 3 * c.H + c.W + c.Cg + sum(c.dils))
    n = torch.randn(c.B, c.Cin, c.H, c.W, generator=g_)
    if family in ("dc", "smallout"):
        x = 20.0 + n
    elif family == "postact":
        x = SQRT2 * F.leaky_relu(n + 3.0, 0.2)
    else:
        x = n
    ws = [torch.randn(c.Cg, c.Cin, 3, 3, generator=g_) / math.sqrt(9 * c.Cin) for _ in c.dils]
    if family == "smallout":      # zero-sum filters: the DC part of x cancels in the output, max|ref| ~ 1 under |x| (*) |w| ~ 400
        ws = [w - w.mean(dim=(1, 2, 3), keepdim=True) for w in ws]
    ops = dict(x=x, ws=ws, in_scale=None, out_scale=None, noise=None, noise_w=None, bias=None)
    if family == "style":         # per-sample style scales over four decades, and the true demodulation
        s = torch.exp(math.log(1e-2) + (math.log(1e2) - math.log(1e-2)) * torch.rand(c.B, c.Cin, generator=g_))
        wcat = torch.cat(ws).double()
        dem = 1.0 / torch.sqrt(((s.double()[:, None, :, None, None] * wcat[None]) ** 2).sum(dim=(2, 3, 4)) + 1e-8)
        ops["in_scale"], ops["out_scale"] = s, dem.float()
    if epilogue:
        ops["noise"], ops["noise_w"] = torch.randn(c.B, 1, c.H, c.W, generator=g_), torch.tensor([0.7])
        ops["bias"] = torch.randn(len(c.dils) * c.Cg, generator=g_)
    return ops


def _np(t, dt):
    return None if t is None else t.numpy().astype(dt)


def epilogue(y, ops, dtype):
    """out_scale, then noise_w * noise, then bias + leaky relu (slope 0.2, gain sqrt 2): in `dtype`, an operation at a time."""
    dt = np.dtype(dtype).type
    y = np.asarray(y, dtype=dt)
    if ops["out_scale"] is not None:
        y = y * _np(ops["out_scale"], dt)[:, :, None, None]
    if ops["noise"] is not None:
        y = y + _np(ops["noise"], dt) * _np(ops["noise_w"], dt)[0]
    if ops["bias"] is not None:
        y = y + _np(ops["bias"], dt)[None, :, None, None]
        y = np.where(y >= 0, y, y * dt(0.2)) * dt(SQRT2)
    return y


def reference(case, ops):
    """(ref, unit) in float64: the launch's exact result, and the absolute-value launch  2^-24 (|x s| (*) |w|) |out_scale| (+ |noise_w noise|
    + |bias|, times the gain) -- what one float32 rounding of every operand's contribution could move the output by."""
    x = ops["x"].double().numpy()
    if ops["in_scale"] is not None:
        x = x * ops["in_scale"].double().numpy()[:, :, None, None]
    ref = np.concatenate([conv64(x, w.double().numpy(), d) for w, d in zip(ops["ws"], case.dils)], axis=1)
    mag = np.concatenate([conv64(np.abs(x), np.abs(w.double().numpy()), d) for w, d in zip(ops["ws"], case.dils)], axis=1)
    ref = epilogue(ref, ops, np.float64)
    aops = {k: (None if v is None else v.abs()) for k, v in ops.items() if k in ("out_scale", "noise", "noise_w", "bias")}
    mag = epilogue(mag, aops, np.float64)
    return ref, U24 * mag


def model(case, ops, dtype=np.float32, order=PLAIN):
    """The launch in `dtype` on the CPU: the Winograd model with the kernel's points and fold (the control: control_of), then the epilogue."""
    pts = points_of(case.kernel)
    x = ops["x"].numpy()
    ys = []
    for w, d in zip(ops["ws"], case.dils):
        if pts is None:
            xs = x if ops["in_scale"] is None else x * ops["in_scale"].numpy()[:, :, None, None]
            ys.append(control_of(case)(xs, w.numpy(), d))
        else:
            ys.append(wino_conv(x, w.numpy(), pts, dtype, d, _np(ops["in_scale"], dtype), fold_of(case.kernel), order))
    return epilogue(np.concatenate(ys, axis=1), ops, dtype)


def errors(y, ref, unit):
    """E = max|y - ref|;  S = max(|y - ref| / unit): the error in units of the absolute-value convolution, so that a quiet region beside
    a loud one is not hidden by the maximum."""
    d = np.abs(np.asarray(y, dtype=np.float64) - ref)
    assert np.isfinite(d).all(), "non-finite output"
    return float(d.max()), float((d / unit).max())
