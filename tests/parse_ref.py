"""facexlib's ParseNet as a plain torch.nn tree on the CPU under the public key names, in float64 or float32, unfused (the
tree itself, BatchNorm in eval mode) and folded with the rounding points of csrc/parse.hip: the input is (u8 / 255 - 0.5) / 0.5; head
weights and every bias keep their fp32 values; every other weight is the float64 fold rounded to f16 once; every stored tensor (head,
shortcut, conv1, block output) is rounded to f16 once, residuals are added before that rounding; logits are never rounded.  Each layer
function returns the value BEFORE the f16 rounding, so that a test can take the rounding allowance at the float64 value.

Argmax, keep table, blur and border are NumPy int64; the masked paste stands on tests/photo_ref.py and tests/photo_aa_ref.py.  Nothing
here imports the package."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import photo_aa_ref as A
import photo_ref as P0

CLASSES = 19
KEEP = np.array([0 if c in (0, 14, 16, 17, 18) else 1 for c in range(CLASSES)], dtype=np.uint8)
BN_EPS = 1e-5


# ----------------------------------------------------------------------------------------------------------- the public definition
class NormLayer(nn.Module):
    def __init__(self, channels):
        super().__init__()
        self.norm = nn.BatchNorm2d(channels, affine=True)

    def forward(self, x):
        return self.norm(x)


class ConvLayer(nn.Module):
    """[nearest x2] + ReflectionPad2d(1) + conv3x3 (stride 2 for 'down'; a bias only without a norm) + [BatchNorm2d] + [LeakyReLU(0.2)]"""

    def __init__(self, cin, cout, scale="none", norm=False, relu=False):
        super().__init__()
        self.scale, self.relu = scale, relu
        self.conv2d = nn.Conv2d(cin, cout, 3, 2 if scale == "down" else 1, bias=not norm)
        if norm:
            self.norm = NormLayer(cout)

    def forward(self, x):
        if self.scale == "up":
            x = F.interpolate(x, scale_factor=2, mode="nearest")
        x = self.conv2d(F.pad(x, (1, 1, 1, 1), mode="reflect"))
        if hasattr(self, "norm"):
            x = self.norm(x)
        return F.leaky_relu(x, 0.2) if self.relu else x


class ResidualBlock(nn.Module):
    def __init__(self, cin, cout, scale="none"):
        super().__init__()
        if scale != "none" or cin != cout:
            self.shortcut_func = ConvLayer(cin, cout, scale)
        s0, s1 = {"down": ("none", "down"), "up": ("up", "none"), "none": ("none", "none")}[scale]
        self.conv1 = ConvLayer(cin, cout, s0, norm=True, relu=True)
        self.conv2 = ConvLayer(cout, cout, s1, norm=True, relu=False)

    def forward(self, x):
        sc = self.shortcut_func(x) if hasattr(self, "shortcut_func") else x
        return sc + self.conv2(self.conv1(x))


ENCODER = ((64, 128), (128, 256), (256, 256), (256, 256))
DECODER = ((256, 256), (256, 256), (256, 128), (128, 64))


class ParseNet(nn.Module):
    def __init__(self):
        super().__init__()
        self.encoder = nn.Sequential(ConvLayer(3, 64), *[ResidualBlock(ci, co, "down") for ci, co in ENCODER])
        self.body = nn.Sequential(*[ResidualBlock(256, 256) for _ in range(10)])
        self.decoder = nn.Sequential(*[ResidualBlock(ci, co, "up") for ci, co in DECODER])
        self.out_img_conv = ConvLayer(64, 3)
        self.out_mask_conv = ConvLayer(64, CLASSES)

    def forward(self, x):
        feat = self.encoder(x)
        x = feat + self.body(feat)
        return self.out_mask_conv(self.decoder(x))


def block_names():
    return [f"encoder.{i}" for i in range(1, 5)] + [f"body.{i}" for i in range(10)] + [f"decoder.{i}" for i in range(4)]


def make_state(seed=0):
    """A well-conditioned random checkpoint under the public keys: convolutions N(0, 1 / fan_in), shortcut convolutions N(0, 0.5 / fan_in);
    BatchNorm scale uniform 0.75 .. 1.25, 0.3 .. 0.5 on every conv2; biases N(0, 0.05^2); running mean N(0, 0.1^2); running variance
    uniform 0.75 .. 1.25.  (N(0, 1.6 / fan_in) with scales around 1 on conv2 drives the logits to 2e4 through the residual chain.)"""
    g = torch.Generator().manual_seed(seed)
    sd = ParseNet().state_dict()
    for k in sd:
        v = sd[k]
        if k.endswith("conv2d.weight"):
            var = (0.5 if "shortcut_func" in k else 1.0) / (9 * v.shape[1])
            sd[k] = torch.randn(v.shape, generator=g) * var ** 0.5
        elif k.endswith("conv2d.bias") or k.endswith("norm.norm.bias"):
            sd[k] = torch.randn(v.shape, generator=g) * 0.05
        elif k.endswith("norm.norm.weight"):
            lo, hi = (0.3, 0.5) if ".conv2." in k else (0.75, 1.25)
            sd[k] = lo + (hi - lo) * torch.rand(v.shape, generator=g)
        elif k.endswith("running_mean"):
            sd[k] = torch.randn(v.shape, generator=g) * 0.1
        elif k.endswith("running_var"):
            sd[k] = 0.75 + 0.5 * torch.rand(v.shape, generator=g)
    return sd


def unfused(sd, dtype=torch.float64):
    """the tree itself with sd loaded, in eval mode"""
    net = ParseNet().to(dtype)
    net.load_state_dict({k: v.to(dtype) if v.is_floating_point() else v for k, v in sd.items()})
    return net.eval()


def crops_f(crops_u8, dtype):
    """uint8 (F, S, S, 3) -> (F, 3, S, S): (u8 / 255 - 0.5) / 0.5"""
    x = torch.from_numpy(np.ascontiguousarray(crops_u8)).to(dtype).permute(0, 3, 1, 2)
    return (x / 255 - 0.5) / 0.5


def test_crops(n, size, seed=0):
    """uniform random bytes"""
    return np.random.default_rng(seed).integers(0, 256, (n, size, size, 3), dtype=np.uint8)


test_crops.__test__ = False


# ------------------------------------------------------------------------------------------------------------- folded restatement
def fold(sd):
    """{name: (w float64, b float64)}: BatchNorm folded in float64, nothing rounded"""
    d = {k: v.double() for k, v in sd.items() if v.is_floating_point()}
    out = {"head": (d["encoder.0.conv2d.weight"], d["encoder.0.conv2d.bias"])}
    for p in block_names():
        if f"{p}.shortcut_func.conv2d.weight" in d:
            out[f"{p}.shortcut"] = (d[f"{p}.shortcut_func.conv2d.weight"], d[f"{p}.shortcut_func.conv2d.bias"])
        for c in ("conv1", "conv2"):
            n = f"{p}.{c}.norm.norm."
            g = d[n + "weight"] / torch.sqrt(d[n + "running_var"] + BN_EPS)
            out[f"{p}.{c}"] = (d[f"{p}.{c}.conv2d.weight"] * g.view(-1, 1, 1, 1), d[n + "bias"] - d[n + "running_mean"] * g)
    out["mask"] = (d["out_mask_conv.conv2d.weight"], d["out_mask_conv.conv2d.bias"])
    return out


def f16(t):
    """round to f16 (nearest even), back in t's dtype"""
    return t.to(torch.float16).to(t.dtype)


def up_index(n):
    """source index of every position of the nearest x2 of n: i >> 1"""
    return np.arange(2 * n) >> 1


def reflect_index(n):
    """source index of positions -1 .. n of a reflection padding of 1: -1 -> 1, n -> n - 2"""
    i = np.arange(-1, n + 1)
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def gather_input(x, up):
    """(F, C, H, W) -> the padded tensor the 3x3 convolution reads, by index: nearest x2 (if up), then the reflection in that domain"""
    h, w = x.shape[2:]
    if up:
        x = x[:, :, torch.from_numpy(up_index(h))][:, :, :, torch.from_numpy(up_index(w))]
        h, w = 2 * h, 2 * w
    return x[:, :, torch.from_numpy(reflect_index(h))][:, :, :, torch.from_numpy(reflect_index(w))]


def head_pre(crops_u8, w, b, dtype):
    """-> (F, 64, S, S) before the f16 rounding: fp32 weights and bias as they are"""
    return F.conv2d(gather_input(crops_f(crops_u8, dtype), False), w.float().to(dtype), b.float().to(dtype))


def conv_pre(x, w, b, dtype, stride=1, up=False, act=False, res=()):
    """x (F, Cin, H, W) holding f16 values -> (F, Cout, OH, OW) before the f16 rounding: w rounded to f16 here, b to fp32; LeakyReLU(0.2)
    if act; then the residuals (f16 values) are added"""
    y = F.conv2d(gather_input(x.to(dtype), up), f16(w.float()).to(dtype), b.float().to(dtype), stride=stride)
    if act:
        y = F.leaky_relu(y, 0.2)
    for r in res:
        y = y + r.to(dtype)
    return y


def features(folded, crops_u8, dtype):
    """the decoder's last activation (F, 64, S, S), f16 values in `dtype`"""
    x = f16(head_pre(crops_u8, *folded["head"], dtype))
    feat = None
    for p in block_names():
        kind = "down" if p.startswith("encoder") else "up" if p.startswith("decoder") else "none"
        if p == "body.0":
            feat = x
        if kind == "none":
            sc = x
        else:
            sc = f16(conv_pre(x, *folded[f"{p}.shortcut"], dtype, stride=2 if kind == "down" else 1, up=kind == "up"))
        t = f16(conv_pre(x, *folded[f"{p}.conv1"], dtype, up=kind == "up", act=True))
        res = (sc, feat) if p == "body.9" else (sc,)
        x = f16(conv_pre(t, *folded[f"{p}.conv2"], dtype, stride=2 if kind == "down" else 1, res=res))
    return x


def mask_logits(x, w, b, dtype):
    """x (F, 64, H, W) f16 values -> (F, H, W, 19) logits, never rounded"""
    return conv_pre(x, w, b, dtype).permute(0, 2, 3, 1).contiguous()


def logits(folded, crops_u8, dtype):
    return mask_logits(features(folded, crops_u8, dtype), *folded["mask"], dtype)


def f16_ulp(v):
    """the f16 unit in the last place at the magnitude of the float64 values v (2^-24 in the subnormal range)"""
    a = np.abs(np.asarray(v, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return 2.0 ** (e - 10)


# ----------------------------------------------------------------------------------------------------- argmax, keep, blur, border
def argmax_classes(lg):
    """(..., 19) logits -> (classes uint8: the first maximum, class 0 where a logit is not finite; per-pixel non-finite flag)"""
    lg = np.asarray(lg)
    bad = ~np.isfinite(lg).all(axis=-1)
    cls = np.argmax(np.where(np.isfinite(lg), lg, -np.inf), axis=-1)      # np.argmax takes the first of equal maxima
    return np.where(bad, 0, cls).astype(np.uint8), bad


def top_two_gap(lg):
    s = np.sort(np.asarray(lg, dtype=np.float64), axis=-1)
    return s[..., -1] - s[..., -2]


def reflect101(i, n):
    i = np.where(i < 0, -i, i)
    return np.where(i >= n, 2 * (n - 1) - i, i)


def blur_pass(m, taps, axis):
    """one 1-D pass along `axis` of an int64 array: (sum_k g[|k|] m[reflect101(i + k)] + 2^15) >> 16"""
    g = np.asarray(taps, dtype=np.int64)
    n, r = m.shape[axis], g.size - 1
    acc = np.zeros_like(m)
    for k in range(-r, r + 1):
        acc += g[abs(k)] * np.take(m, reflect101(np.arange(n) + k, n), axis=axis)
    return (acc + 32768) >> 16


def paste_weights(keep, taps, border):
    """keep (F, S, S) 0 / 1 -> uint16 (F, S, S): m0 = 16384 keep, passes along x, y, x, y, (m + 32) >> 6, the border zeroed"""
    m = np.asarray(keep, dtype=np.int64) * 16384
    for axis in (2, 1, 2, 1):
        m = blur_pass(m, taps, axis)
    w = (m + 32) >> 6
    s = w.shape[1]
    if border > 0:
        w[:, :border] = 0
        w[:, s - border:] = 0
        w[:, :, :border] = 0
        w[:, :, s - border:] = 0
    return w.astype(np.uint16)


# --------------------------------------------------------------------------------------------------------------------- masked paste
def paste_masked(photo, faces, S, ramp=None, antialias=False):
    """photo_ref.paste / photo_aa_ref.paste through a mask: `faces` = [(restored crop uint8 (S, S, 3), P, mask uint16 (S, S)), ...] in
    list order; wm = the mask through the colour's four taps, w = (ramp wm + 128) >> 8"""
    out = np.array(photo, dtype=np.uint8)
    H, W = out.shape[:2]
    ramp = P0.default_ramp() if ramp is None else np.asarray(ramp)
    L, lim = ramp.shape[0], (S - 1) * 32
    for restored, P, mask in faces:
        P = np.asarray(P, dtype=np.float64)
        x0, y0, x1, y1 = P0.bbox(P, S, H, W)
        if x1 <= x0 or y1 <= y0:
            continue
        xs, ys = np.arange(x0, x1), np.arange(y0, y1)
        X, Y = P0._coords(P, xs, ys)
        d = np.minimum(np.minimum(X, Y), np.minimum(lim - X, lim - Y))
        touch = d >= 0
        Xc, Yc = np.clip(X, 0, lim), np.clip(Y, 0, lim)
        w = ramp[np.minimum(np.maximum(d, 0) >> 2, L - 1)].astype(np.int64)
        m3 = np.repeat(np.asarray(mask, dtype=np.uint16)[..., None], 3, axis=2)
        wm = P0._bilinear(m3, Xc, Yc)[..., 0]
        w = (w * wm + 128) >> 8
        restored = np.asarray(restored, dtype=np.uint8)
        rch = 0
        if antialias:
            m = A.paste_minify(P)
            A.check_minify(m)
            rch = A.reach(P, m)
        if rch == 0:
            f = P0._bilinear(restored, Xc, Yc)
        else:
            f = A.filtered(restored, P0.invert(P), Xc, Yc, xs, ys, rch, mask=touch)
        bg = out[y0:y1, x0:x1].astype(np.int64)
        mixed = (w[..., None] * f + (256 - w[..., None]) * bg + 128) >> 8
        out[y0:y1, x0:x1] = np.where(touch[..., None], mixed, bg).astype(np.uint8)
    return out


# ------------------------------------------------------------------------------------------------ the cases the GPU tests run on
NET_CASES = ((32, 3), (64, 2))                 # (crop side, faces) of the whole-network tests
NET_LEFT_OUT_CAP = 0.10                        # share of pixels whose float64 top-two gap may lie within twice the logit bound
TAIL_LEFT_OUT_CAP = 0.005
TIE = (3, 7)                                   # the tail case's two classes with identical weights and bias
_cache = {}


def net_case(size, faces):
    """-> (state dict, crops uint8 (faces, size, size, 3), logits float64, logits float32) of one whole-network case, computed once"""
    key = ("net", size, faces)
    if key not in _cache:
        sd, crops = make_state(seed=100 + size), test_crops(faces, size, seed=200 + size)
        folded = fold(sd)
        with torch.no_grad():
            _cache[key] = (sd, crops, logits(folded, crops, torch.float64).numpy(), logits(folded, crops, torch.float32).double().numpy())
    return _cache[key]


def logit_bound(l64, l32):
    """the project's 4 e_ref + 2e-6 max |ref64| and e_ref"""
    e_ref = float(np.abs(l32 - l64).max())
    return 4 * e_ref + 2e-6 * float(np.abs(l64).max()), e_ref


def left_out(l64, tol, drop=None):
    """mask of the pixels whose float64 top-two gap does not exceed twice the logit bound (class `drop` left aside)"""
    lg = l64 if drop is None else np.delete(l64, drop, axis=-1)
    return top_two_gap(lg) <= 2 * tol


def tail_case(h=9, w=33, faces=2, seed=7):
    """-> (x (faces, 64, h, w) float64 holding f16 values, w (19, 64, 3, 3), b (19)): the tail alone, with classes TIE[0] and TIE[1] given
    identical weights and bias and a lift that makes them the maximum at many pixels"""
    g = torch.Generator().manual_seed(seed)
    x = (torch.randn(faces, 64, h, w, generator=g) * 0.5).to(torch.float16).to(torch.float64)
    wt = torch.randn(CLASSES, 64, 3, 3, generator=g) * (1.0 / 576) ** 0.5
    b = torch.randn(CLASSES, generator=g) * 0.05
    b[TIE[0]] += 0.25
    wt[TIE[1]], b[TIE[1]] = wt[TIE[0]], b[TIE[0]]
    return x, wt, b
