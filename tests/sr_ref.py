"""SRVGGNetCompact as plain torch on the CPU, in float64 or float32, with the rounding points of csrc/sr.hip: the input is
u8 / 255; head weights, every bias and every PReLU slope keep their fp32 values; body and tail weights are rounded to f16; every
activation is rounded to f16 behind its PReLU; the shuffle, the nearest-neighbour skip and the quantisation are written out by index.
Each layer function returns the value BEFORE the f16 rounding, so that a test can take the rounding allowance at the float64 value."""
import numpy as np
import torch
import torch.nn.functional as F


def make_state(num_conv, scale, seed=0, gain=1.6):
    """A well-conditioned random checkpoint in the public key layout: weights N(0, gain / fan_in) for head and body, the tail a quarter
    of that variance, biases N(0, 0.05^2), slopes uniform in -0.25 .. 0.5 (negative slopes occur)"""
    g = torch.Generator().manual_seed(seed)
    sd = {}

    def conv(i, co, ci, var):
        sd[f"body.{i}.weight"] = torch.randn(co, ci, 3, 3, generator=g) * (var / (9 * ci)) ** 0.5
        sd[f"body.{i}.bias"] = torch.randn(co, generator=g) * 0.05

    def prelu(i):
        sd[f"body.{i}.weight"] = torch.rand(64, generator=g) * 0.75 - 0.25

    conv(0, 64, 3, gain)
    prelu(1)
    for k in range(1, num_conv + 1):
        conv(2 * k, 64, 64, gain)
        prelu(2 * k + 1)
    conv(2 * num_conv + 2, 3 * scale * scale, 64, gain / 4)
    return sd


def test_photo(h, w, seed=0):
    """uint8 (h, w, 3): smooth gradients plus noise"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    base = np.stack([127 + 90 * np.sin(0.21 * xx + 0.13 * yy + c) for c in range(3)], axis=-1)
    return np.clip(base + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)


def f16(t):
    """round to f16 (nearest even), back in t's dtype"""
    return t.to(torch.float16).to(t.dtype)


def prelu(y, a):
    return torch.where(y >= 0, y, a.view(1, -1, 1, 1) * y)


def head_pre(x_u8, w, b, a, dtype):
    """uint8 (h, w, 3) -> (1, 64, h, w) before the f16 rounding"""
    x = torch.from_numpy(np.ascontiguousarray(x_u8)).to(dtype).permute(2, 0, 1)[None] / 255
    return prelu(F.conv2d(x, w.to(dtype), b.to(dtype), padding=1), a.to(dtype))


def body_pre(act, w, b, a, dtype):
    """act (1, 64, h, w) holding f16 values -> (1, 64, h, w) before the f16 rounding; w is rounded to f16 here"""
    return prelu(F.conv2d(act.to(dtype), f16(w.to(torch.float32)).to(dtype), b.to(dtype), padding=1), a.to(dtype))


def shuffle(t, s):
    """(1, C s^2, h, w) -> (1, C, s h, s w): channel c s^2 + dy s + dx -> pixel (s y + dy, s x + dx)"""
    _, cs, h, w = t.shape
    c = cs // (s * s)
    out = t.new_zeros((1, c, s * h, s * w))
    for dy in range(s):
        for dx in range(s):
            out[:, :, dy::s, dx::s] = t[:, [k * s * s + dy * s + dx for k in range(c)]]
    return out


def nearest(x, s):
    """(1, C, h, w) -> (1, C, s h, s w): output pixel (Y, X) takes input pixel (Y // s, X // s)"""
    _, _, h, w = x.shape
    yi, xi = torch.arange(s * h) // s, torch.arange(s * w) // s
    return x[:, :, yi][:, :, :, xi]


def tail_pre(act, x_u8, w, b, s, dtype):
    """act (1, 64, h, w) f16 values, x_u8 (h, w, 3) -> (s h, s w, 3): the unclamped output"""
    y = F.conv2d(act.to(dtype), f16(w.to(torch.float32)).to(dtype), b.to(dtype), padding=1)
    x = torch.from_numpy(np.ascontiguousarray(x_u8)).to(dtype).permute(2, 0, 1)[None] / 255
    return (shuffle(y, s) + nearest(x, s))[0].permute(1, 2, 0).contiguous()


def quantise(v):
    """unclamped (H, W, 3) -> uint8: rint(255 clamp(v, 0, 1)), half to even"""
    return np.rint((v.clamp(0, 1) * 255).numpy()).astype(np.uint8)


def net(sd, x_u8, dtype, upto=None):
    """The whole network on one photo -> the unclamped (s h, s w, 3) output in `dtype`.  upto = k: the f16-rounded activation behind
    convolution k (0 = head) instead, (1, 64, h, w)."""
    num_conv = (max(int(k.split(".")[1]) for k in sd) - 2) // 2
    last = 2 * num_conv + 2
    s = {12: 2, 48: 4}[sd[f"body.{last}.weight"].shape[0]]
    act = f16(head_pre(x_u8, sd["body.0.weight"], sd["body.0.bias"], sd["body.1.weight"], dtype))
    if upto == 0:
        return act
    for k in range(1, num_conv + 1):
        act = f16(body_pre(act, sd[f"body.{2 * k}.weight"], sd[f"body.{2 * k}.bias"], sd[f"body.{2 * k + 1}.weight"], dtype))
        if upto == k:
            return act
    return tail_pre(act, x_u8, sd[f"body.{last}.weight"], sd[f"body.{last}.bias"], s, dtype)


def net_banded(sd, x_u8, dtype, band_rows, bands):
    """net() band by band: `bands` = upscale.plan_bands(h, band_rows, halo) -> the unclamped output assembled from the bands' kept rows"""
    num_conv = (max(int(k.split(".")[1]) for k in sd) - 2) // 2
    s = {12: 2, 48: 4}[sd[f"body.{2 * num_conv + 2}.weight"].shape[0]]
    rows = []
    for r0, r1, a0, a1 in bands:
        v = net(sd, x_u8[a0:a1], dtype)
        rows.append(v[s * (r0 - a0):s * (r1 - a0)])
    return torch.cat(rows)


def f16_ulp(v):
    """the f16 unit in the last place at the magnitude of the float64 values v (2^-24 in the subnormal range)"""
    a = np.abs(np.asarray(v, dtype=np.float64))
    e = np.floor(np.log2(np.maximum(a, 2.0 ** -14)))
    return 2.0 ** (e - 10)
