"""Restatement of the landmark network (csrc/fan.hip, vspbfr_amd/fan.py) for the tests: face_alignment's 2D-FAN as a plain
torch.nn tree under the checkpoint's key names (unfused, float64), its own BatchNorm reduction, and the reduced network with the
kernels' rounding points -- f16 weights, f16 activations between layers, the activated operand f16(relu(float32(a x + b))), fp32 stem
weights, biases and heatmaps -- evaluated in float64 or float32 on the CPU.  The heatmap decode and lmd / nme are restated in NumPy.
Nothing here imports the product."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

BN_EPS = 1e-5
POINTS = 68


# ------------------------------------------------------------------------------------------------------------------ the unfused tree
class ConvBlock(nn.Module):
    def __init__(self, cin, cout):
        super().__init__()
        self.bn1, self.conv1 = nn.BatchNorm2d(cin), nn.Conv2d(cin, cout // 2, 3, 1, 1, bias=False)
        self.bn2, self.conv2 = nn.BatchNorm2d(cout // 2), nn.Conv2d(cout // 2, cout // 4, 3, 1, 1, bias=False)
        self.bn3, self.conv3 = nn.BatchNorm2d(cout // 4), nn.Conv2d(cout // 4, cout // 4, 3, 1, 1, bias=False)
        self.downsample = None
        if cin != cout:
            self.downsample = nn.Sequential(nn.BatchNorm2d(cin), nn.ReLU(True), nn.Conv2d(cin, cout, 1, bias=False))

    def forward(self, x):
        o1 = self.conv1(F.relu(self.bn1(x)))
        o2 = self.conv2(F.relu(self.bn2(o1)))
        o3 = self.conv3(F.relu(self.bn3(o2)))
        return torch.cat((o1, o2, o3), 1) + (x if self.downsample is None else self.downsample(x))


class HourGlass(nn.Module):
    def __init__(self, depth, features=256):
        super().__init__()
        self.depth = depth
        for level in range(depth, 0, -1):
            self.add_module(f"b1_{level}", ConvBlock(features, features))
            self.add_module(f"b2_{level}", ConvBlock(features, features))
            if level == 1:
                self.add_module(f"b2_plus_{level}", ConvBlock(features, features))
            self.add_module(f"b3_{level}", ConvBlock(features, features))

    def level(self, level, x):
        up1 = self._modules[f"b1_{level}"](x)
        low1 = self._modules[f"b2_{level}"](F.avg_pool2d(x, 2, stride=2))
        low2 = self.level(level - 1, low1) if level > 1 else self._modules[f"b2_plus_{level}"](low1)
        low3 = self._modules[f"b3_{level}"](low2)
        return up1 + F.interpolate(low3, scale_factor=2, mode="nearest")

    def forward(self, x):
        return self.level(self.depth, x)


class FAN(nn.Module):
    def __init__(self, num_modules=4, depth=4):
        super().__init__()
        self.num_modules = num_modules
        self.conv1, self.bn1 = nn.Conv2d(3, 64, 7, 2, 3), nn.BatchNorm2d(64)
        self.conv2, self.conv3, self.conv4 = ConvBlock(64, 128), ConvBlock(128, 128), ConvBlock(128, 256)
        for i in range(num_modules):
            self.add_module(f"m{i}", HourGlass(depth))
            self.add_module(f"top_m_{i}", ConvBlock(256, 256))
            self.add_module(f"conv_last{i}", nn.Conv2d(256, 256, 1))
            self.add_module(f"bn_end{i}", nn.BatchNorm2d(256))
            self.add_module(f"l{i}", nn.Conv2d(256, POINTS, 1))
            if i < num_modules - 1:
                self.add_module(f"bl{i}", nn.Conv2d(256, 256, 1))
                self.add_module(f"al{i}", nn.Conv2d(POINTS, 256, 1))

    def forward(self, x):
        x = self.conv2(F.relu(self.bn1(self.conv1(x))))
        x = self.conv4(self.conv3(F.avg_pool2d(x, 2, stride=2)))
        previous, out = x, None
        for i in range(self.num_modules):
            ll = self._modules[f"top_m_{i}"](self._modules[f"m{i}"](previous))
            ll = F.relu(self._modules[f"bn_end{i}"](self._modules[f"conv_last{i}"](ll)))
            out = self._modules[f"l{i}"](ll)
            if i < self.num_modules - 1:
                previous = previous + self._modules[f"bl{i}"](ll) + self._modules[f"al{i}"](out)
        return out


def r16(t):
    """the rounding of an fp32 value to f16, kept in t's dtype"""
    return t.float().half().to(t.dtype)


def make_model(seed, num_modules=4, depth=4):
    """A float64 FAN in eval mode with well-conditioned random weights: convolutions N(0, 1 / fan_in) rounded to f16, their biases
    N(0, 0.1^2), BatchNorm scale and variance in 0.75..1.25 with small shift and mean"""
    g = torch.Generator().manual_seed(seed)
    net = FAN(num_modules, depth).double().eval()
    with torch.no_grad():
        for m in net.modules():
            if isinstance(m, nn.Conv2d):
                fan_in = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]
                m.weight.copy_(r16(torch.randn(m.weight.shape, generator=g, dtype=torch.float64) / fan_in ** 0.5))
                if m.bias is not None:
                    m.bias.copy_(0.1 * torch.randn(m.bias.shape, generator=g, dtype=torch.float64))
            elif isinstance(m, nn.BatchNorm2d):
                n = m.weight.shape[0]
                m.weight.copy_(0.75 + 0.5 * torch.rand(n, generator=g, dtype=torch.float64))
                m.bias.copy_(0.1 * torch.randn(n, generator=g, dtype=torch.float64))
                m.running_mean.copy_(0.1 * torch.randn(n, generator=g, dtype=torch.float64))
                m.running_var.copy_(0.75 + 0.5 * torch.rand(n, generator=g, dtype=torch.float64))
    return net


def state_of(net, tracked=False):
    """the checkpoint of a FAN: without the BatchNorm counters, as the old file is, unless `tracked`"""
    return {k: v.clone() for k, v in net.state_dict().items() if tracked or not k.endswith("num_batches_tracked")}


# ------------------------------------------------------------------------------------------------------------------ the reduction
def affine(sd, p):
    a = sd[p + ".weight"].double() / torch.sqrt(sd[p + ".running_var"].double() + BN_EPS)
    return a, sd[p + ".bias"].double() - sd[p + ".running_mean"].double() * a


def block_names(num_modules, depth):
    """[(prefix, cin, cout)] of every ConvBlock"""
    out = [("conv2", 64, 128), ("conv3", 128, 128), ("conv4", 128, 256)]
    for i in range(num_modules):
        for level in range(depth, 0, -1):
            out += [(f"m{i}.b{k}_{level}", 256, 256) for k in (1, 2, 3)]
        out += [(f"m{i}.b2_plus_1", 256, 256), (f"top_m_{i}", 256, 256)]
    return out


def reduce(sd, num_modules, depth):
    """{name: float64}: `<bn>.a` / `.b` of every BatchNorm in front of a convolution, `<conv>.w` [/ `.b`] of every convolution with
    `bn1` folded into `conv1` and `bn_end{i}` into `conv_last{i}` (weights and biases as given: nothing is rounded here)"""
    sd = {k: v.double() for k, v in sd.items()}
    out = {}
    a, s = affine(sd, "bn1")
    out["conv1.w"], out["conv1.b"] = sd["conv1.weight"] * a.view(-1, 1, 1, 1), sd["conv1.bias"] * a + s
    for p, cin, cout in block_names(num_modules, depth):
        for k in (1, 2, 3):
            out[f"{p}.bn{k}.a"], out[f"{p}.bn{k}.b"] = affine(sd, f"{p}.bn{k}")
            out[f"{p}.conv{k}.w"] = sd[f"{p}.conv{k}.weight"]
        if cin != cout:
            out[f"{p}.downsample.0.a"], out[f"{p}.downsample.0.b"] = affine(sd, f"{p}.downsample.0")
            out[f"{p}.downsample.2.w"] = sd[f"{p}.downsample.2.weight"]
    for i in range(num_modules):
        a, s = affine(sd, f"bn_end{i}")
        out[f"conv_last{i}.w"], out[f"conv_last{i}.b"] = sd[f"conv_last{i}.weight"] * a.view(-1, 1, 1, 1), sd[f"conv_last{i}.bias"] * a + s
        for n in ("l", "bl", "al"):
            if f"{n}{i}.weight" in sd:
                out[f"{n}{i}.w"], out[f"{n}{i}.b"] = sd[f"{n}{i}.weight"], sd[f"{n}{i}.bias"]
    return out


# ------------------------------------------------------------------------------------------------------ the kernels' arithmetic
def f16_half_ulp(v):
    """half an f16 ulp at the magnitudes v (normal range: 2^-11 of the power of two below; subnormal: 2^-25)"""
    return 2.0 ** (np.floor(np.log2(np.maximum(np.abs(np.asarray(v, dtype=np.float64)), 2.0 ** -14))) - 11)


def activate(x, a, b):
    """the input affine's operand: f16(relu(float32(float64 a . float64 x + float64 b))) of f16 values x and fp32 coefficients a, b --
    the fused multiply-add's single rounding; returned as float64 (both precisions read these same f16 values)"""
    a, b = a.float().double().view(1, -1, 1, 1), b.float().double().view(1, -1, 1, 1)
    return torch.relu((a * x.double() + b).float()).half().double()


def nearest2(t):
    return t.repeat_interleave(2, dim=2).repeat_interleave(2, dim=3)


def conv_ref(x, w, dtype, b=None, aff=None, relu=False, rounded=True):
    """v = conv(x') [+ b] [relu] of vsp_fan_conv_f16 before any rounding of the result: x holds f16 values, w is rounded to f16 and b to fp32
    here (rounded=False: everything as given, the affine in plain arithmetic)"""
    if aff is not None:
        x = activate(x, *aff) if rounded else torch.relu(aff[0].view(1, -1, 1, 1) * x + aff[1].view(1, -1, 1, 1))
    w, b = (r16(w), None if b is None else b.float()) if rounded else (w, b)
    v = F.conv2d(x.to(dtype), w.to(dtype), None if b is None else b.to(dtype), padding=w.shape[2] // 2)
    return torch.relu(v) if relu else v


def tail_ref(v, dtype, res1=None, res2=None, up=None):
    """the output behind v: ((v + res1) + res2) + nearest2(up), before its rounding"""
    for r in (res1, res2):
        if r is not None:
            v = v + r.to(dtype)
    return v if up is None else v + nearest2(up.to(dtype))


def pool_ref(x):
    """f16(((a + b) + (c + d)) / 4) in fp32 of f16 values: the kernel's order, exactly"""
    x = x.float()
    return r16(((x[:, :, 0::2, 0::2] + x[:, :, 0::2, 1::2]) + (x[:, :, 1::2, 0::2] + x[:, :, 1::2, 1::2])) * 0.25)


def crop_ref(photos, boxes, side, dtype):
    """the crop the stem samples: photos (B, H, W, 3) uint8, boxes (B, 3) float32 values -> (B, 3, side, side) in `dtype`: bilinear at
    half-pixel centres, no anti-aliasing, zero outside the photo, divided by 255"""
    photos = torch.as_tensor(np.asarray(photos))
    B, H, W, _ = photos.shape
    boxes = torch.as_tensor(np.asarray(boxes, dtype=np.float32)).to(dtype)
    out = torch.zeros(B, 3, side, side, dtype=dtype)
    j = torch.arange(side, dtype=dtype)
    for b in range(B):
        x0, y0, sc = boxes[b, 0], boxes[b, 1], boxes[b, 2] / side
        px = photos[b].permute(2, 0, 1).to(dtype)

        def axis(o, n):
            f = o + (j + 0.5) * sc - 0.5
            lo = torch.floor(f)
            return lo.long(), f - lo

        iy, wy = axis(y0, H)
        ix, wx = axis(x0, W)
        acc = torch.zeros(3, side, side, dtype=dtype)
        for dy in (0, 1):
            yy, fy = iy + dy, (wy if dy else 1 - wy)
            for dx in (0, 1):
                xx, fx = ix + dx, (wx if dx else 1 - wx)
                ok = ((yy >= 0) & (yy < H)).view(-1, 1) & ((xx >= 0) & (xx < W)).view(1, -1)
                v = px[:, yy.clamp(0, H - 1)][:, :, xx.clamp(0, W - 1)]
                acc = acc + torch.where(ok, fy.view(-1, 1) * fx.view(1, -1), torch.zeros((), dtype=dtype)) * v
        out[b] = acc / 255
    return out


def stem_ref(photos, boxes, side, w, b, dtype, rounded=True):
    """relu(conv7x7/2/pad3(crop) + b) with fp32 weights, before the rounding to f16"""
    w, b = (w.float(), b.float()) if rounded else (w, b)
    return torch.relu(F.conv2d(crop_ref(photos, boxes, side, dtype), w.to(dtype), b.to(dtype), stride=2, padding=3))


def forward(red, photos, boxes, side, num_modules, depth, dtype, rounded=True, watch=None):
    """The reduced network of reduce() -> heatmaps (B, 68, side / 4, side / 4).  rounded: with the kernels' rounding points (the result
    is the fp32 store's value before it: `dtype` arithmetic on f16 operands); else plain arithmetic in `dtype`.  watch: a list that
    receives max|.| of every activation tensor."""
    q = r16 if rounded else (lambda t: t)

    def see(t):
        if watch is not None:
            watch.append(float(t.abs().max()))
        return t

    def conv(name, x, bn=None, bias=False, relu=False):
        return conv_ref(x, red[name + ".w"], dtype, red[name + ".b"] if bias else None,
                        None if bn is None else (red[bn + ".a"], red[bn + ".b"]), relu, rounded)

    def block(p, x, up=None):
        res = q(conv(p + ".downsample.2", x, p + ".downsample.0")) if p + ".downsample.2.w" in red else x
        v1 = conv(p + ".conv1", x, p + ".bn1")
        v2 = conv(p + ".conv2", q(v1), p + ".bn2")
        v3 = conv(p + ".conv3", q(v2), p + ".bn3")
        return see(q(tail_ref(torch.cat((v1, v2, v3), 1), dtype, res1=res, up=up)))

    def hourglass(p, level, x):
        pooled = pool_ref(x).to(x.dtype) if rounded else F.avg_pool2d(x, 2, stride=2)
        low = block(f"{p}.b2_{level}", pooled)
        low = hourglass(p, level - 1, low) if level > 1 else block(f"{p}.b2_plus_{level}", low)
        low = block(f"{p}.b3_{level}", low)
        return block(f"{p}.b1_{level}", x, up=low)

    x = see(q(stem_ref(photos, boxes, side, red["conv1.w"], red["conv1.b"], dtype, rounded)))
    x = block("conv2", x)
    x = pool_ref(x).to(x.dtype) if rounded else F.avg_pool2d(x, 2, stride=2)
    prev = block("conv4", block("conv3", x))
    heat = None
    for i in range(num_modules):
        ll = block(f"top_m_{i}", hourglass(f"m{i}", depth, prev))
        t = see(q(conv(f"conv_last{i}", ll, bias=True, relu=True)))
        heat = conv(f"l{i}", t, bias=True)
        if i < num_modules - 1:
            branch = q(conv(f"bl{i}", t, bias=True))
            prev = see(q(tail_ref(conv(f"al{i}", q(heat), bias=True), dtype, res1=prev, res2=branch)))
    return heat


def pack_index(co, ci, t, cin, cout):
    """flat index into the weight image (taps, cin / 32, cp / 16, 64, 8) of w[co][ci][tap t], cp = cout rounded up to 32, restated from
    include/vspbfr_hip.h"""
    cp = (cout + 31) // 32 * 32
    nb, lp, kc, lg, j = co // 16, co % 16, ci // 32, (ci % 32) // 8, ci % 8
    return (((t * (cin // 32) + kc) * (cp // 16) + nb) * 64 + lg * 16 + lp) * 8 + j


# -------------------------------------------------------------------------------------------------------------- decode, lmd, nme
def decode_ref(heat, boxes):
    """heat (B, K, n, n) float32 bits, boxes (B, 3) float32 -> (landmarks (B, K, 2) float32, peaks (B, K) float32, nonfinite (B,) bool):
    argmax with the lowest flat index among equals, a non-finite value counted as -inf and flagged; the quarter-pixel offset is the sign
    of the neighbours' difference (none on the border, none for a zero or unordered difference); the point is
    x0 + (px + 0.5 + dx) (s / n), every operation rounded to float32 on its own"""
    heat, boxes = np.asarray(heat, dtype=np.float32), np.asarray(boxes, dtype=np.float32)
    B, K, n, _ = heat.shape
    f = np.float32
    lm, peak, bad = np.zeros((B, K, 2), f), np.zeros((B, K), f), np.zeros(B, bool)
    with np.errstate(invalid="ignore"):
        for b in range(B):
            sc = f(boxes[b, 2] / f(n))
            for k in range(K):
                m = heat[b, k]
                fin = np.isfinite(m)
                bad[b] |= not fin.all()
                at = int(np.argmax(np.where(fin, m, f(-np.inf)).reshape(-1)))       # numpy's argmax returns the first of equals
                py, px = divmod(at, n)
                off = [f(0), f(0)]
                if 0 < px < n - 1:
                    d = f(m[py, px + 1] - m[py, px - 1])
                    off[0] = f(0.25) if d > 0 else (f(-0.25) if d < 0 else f(0))
                if 0 < py < n - 1:
                    d = f(m[py + 1, px] - m[py - 1, px])
                    off[1] = f(0.25) if d > 0 else (f(-0.25) if d < 0 else f(0))
                lm[b, k, 0] = f(boxes[b, 0] + f(f(f(f(px) + f(0.5)) + off[0]) * sc))
                lm[b, k, 1] = f(boxes[b, 1] + f(f(f(f(py) + f(0.5)) + off[1]) * sc))
                peak[b, k] = m[py, px] if fin[py, px] else f(-np.inf)
    return lm, peak, bad


def lmd_nme_ref(lm, lm_gt):
    """float64: the mean over the points of the Euclidean distance, and that over the distance of ground-truth points 36 and 45"""
    a, g = np.asarray(lm, dtype=np.float64), np.asarray(lm_gt, dtype=np.float64)
    d = np.sqrt(((a - g) ** 2).sum(axis=2)).mean(axis=1)
    with np.errstate(divide="ignore", invalid="ignore"):
        return d, d / np.sqrt(((g[:, 36] - g[:, 45]) ** 2).sum(axis=1))


def test_photo(h, w, seed):
    """a smooth uint8 photo with some texture"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([127 + 100 * np.sin(xx / (5 + c) + seed) * np.cos(yy / (7 - c)) for c in range(3)], axis=2)
    return np.clip(base + rng.normal(0, 12, (h, w, 3)), 0, 255).astype(np.uint8)
