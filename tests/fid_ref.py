"""Restatement of pytorch-fid's Inception-v3 as a plain torch.nn tree under torchvision's key names, written from the public
definition (torchvision is not installed).  Float64 and float32, unfused (conv + BatchNorm + ReLU) and folded, with the resize.  The
three pool rules, `stats` and `frechet_distance` are restated here independently of vspbfr_amd.fid.

Also the test weights and the inputs the GPU tests use (CASES), with their references computed once per process."""
import functools

import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

BN_EPS = 1e-3


# ------------------------------------------------------------------------------------------------------------------------ pools
def avg_pool_valid(x):
    """3x3 / 1 / pad 1 average that divides by the number of in-bounds taps (count_include_pad=False), written with unfold-free sums"""
    B, C, H, W = x.shape
    p = F.pad(x, (1, 1, 1, 1))
    ones = F.pad(torch.ones((1, 1, H, W), dtype=x.dtype), (1, 1, 1, 1))
    s, n = torch.zeros_like(x), torch.zeros((1, 1, H, W), dtype=x.dtype)
    for ky in range(3):
        for kx in range(3):
            s = s + p[:, :, ky:ky + H, kx:kx + W]
            n = n + ones[:, :, ky:ky + H, kx:kx + W]
    return s / n


def max_pool_s1(x):
    """3x3 / 1 / pad 1 max"""
    B, C, H, W = x.shape
    p = F.pad(x, (1, 1, 1, 1), value=float("-inf"))
    out = p[:, :, 0:H, 0:W]
    for ky in range(3):
        for kx in range(3):
            out = torch.maximum(out, p[:, :, ky:ky + H, kx:kx + W])
    return out


def max_pool_s2(x):
    """3x3 / 2 without padding"""
    B, C, H, W = x.shape
    oh, ow = (H - 3) // 2 + 1, (W - 3) // 2 + 1
    out = None
    for ky in range(3):
        for kx in range(3):
            v = x[:, :, ky:ky + 2 * (oh - 1) + 1:2, kx:kx + 2 * (ow - 1) + 1:2]
            out = v if out is None else torch.maximum(out, v)
    return out


def resize_bilinear(x, size):
    """(B, C, H, W) -> (B, C, size, size) as F.interpolate(mode="bilinear", align_corners=False) defines it: no anti-aliasing"""
    oh, ow = (size, size) if isinstance(size, int) else size

    def axis(n_in, n_out):
        scale = torch.tensor(n_in, dtype=x.dtype) / torch.tensor(n_out, dtype=x.dtype)
        src = (scale * (torch.arange(n_out, dtype=x.dtype) + 0.5) - 0.5).clamp(min=0)
        i0 = src.floor().long().clamp(max=n_in - 1)
        i1 = (i0 + 1).clamp(max=n_in - 1)
        l1 = src - i0.to(x.dtype)
        return i0, i1, 1 - l1, l1

    y0, y1, wy0, wy1 = axis(x.shape[2], oh)
    x0, x1, wx0, wx1 = axis(x.shape[3], ow)
    top = x[:, :, y0][:, :, :, x0] * wx0 + x[:, :, y0][:, :, :, x1] * wx1
    bot = x[:, :, y1][:, :, :, x0] * wx0 + x[:, :, y1][:, :, :, x1] * wx1
    return top * wy0.view(-1, 1) + bot * wy1.view(-1, 1)


# ---------------------------------------------------------------------------------------------------------------------- the tree
class BasicConv2d(nn.Module):
    def __init__(self, cin, cout, **kw):
        super().__init__()
        self.conv = nn.Conv2d(cin, cout, bias=False, **kw)
        self.bn = nn.BatchNorm2d(cout, eps=BN_EPS)
        self.folded_bias = None

    def forward(self, x):
        if self.folded_bias is not None:
            return F.relu(self.conv(x) + self.folded_bias.view(1, -1, 1, 1))
        return F.relu(self.bn(self.conv(x)))


class InceptionA(nn.Module):
    def __init__(self, cin, pool_features):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 64, kernel_size=1)
        self.branch5x5_1 = BasicConv2d(cin, 48, kernel_size=1)
        self.branch5x5_2 = BasicConv2d(48, 64, kernel_size=5, padding=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, padding=1)
        self.branch_pool = BasicConv2d(cin, pool_features, kernel_size=1)

    def forward(self, x):
        b5 = self.branch5x5_2(self.branch5x5_1(x))
        b3 = self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x)))
        return torch.cat([self.branch1x1(x), b5, b3, self.branch_pool(avg_pool_valid(x))], 1)


class InceptionB(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch3x3 = BasicConv2d(cin, 384, kernel_size=3, stride=2)
        self.branch3x3dbl_1 = BasicConv2d(cin, 64, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(64, 96, kernel_size=3, padding=1)
        self.branch3x3dbl_3 = BasicConv2d(96, 96, kernel_size=3, stride=2)

    def forward(self, x):
        b3 = self.branch3x3dbl_3(self.branch3x3dbl_2(self.branch3x3dbl_1(x)))
        return torch.cat([self.branch3x3(x), b3, max_pool_s2(x)], 1)


class InceptionC(nn.Module):
    def __init__(self, cin, c7):
        super().__init__()
        self.branch1x1 = BasicConv2d(cin, 192, kernel_size=1)
        self.branch7x7_1 = BasicConv2d(cin, c7, kernel_size=1)
        self.branch7x7_2 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7_3 = BasicConv2d(c7, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_1 = BasicConv2d(cin, c7, kernel_size=1)
        self.branch7x7dbl_2 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_3 = BasicConv2d(c7, c7, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7dbl_4 = BasicConv2d(c7, c7, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7dbl_5 = BasicConv2d(c7, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch_pool = BasicConv2d(cin, 192, kernel_size=1)

    def forward(self, x):
        b7 = self.branch7x7_3(self.branch7x7_2(self.branch7x7_1(x)))
        bd = self.branch7x7dbl_5(self.branch7x7dbl_4(self.branch7x7dbl_3(self.branch7x7dbl_2(self.branch7x7dbl_1(x)))))
        return torch.cat([self.branch1x1(x), b7, bd, self.branch_pool(avg_pool_valid(x))], 1)


class InceptionD(nn.Module):
    def __init__(self, cin):
        super().__init__()
        self.branch3x3_1 = BasicConv2d(cin, 192, kernel_size=1)
        self.branch3x3_2 = BasicConv2d(192, 320, kernel_size=3, stride=2)
        self.branch7x7x3_1 = BasicConv2d(cin, 192, kernel_size=1)
        self.branch7x7x3_2 = BasicConv2d(192, 192, kernel_size=(1, 7), padding=(0, 3))
        self.branch7x7x3_3 = BasicConv2d(192, 192, kernel_size=(7, 1), padding=(3, 0))
        self.branch7x7x3_4 = BasicConv2d(192, 192, kernel_size=3, stride=2)

    def forward(self, x):
        b3 = self.branch3x3_2(self.branch3x3_1(x))
        b7 = self.branch7x7x3_4(self.branch7x7x3_3(self.branch7x7x3_2(self.branch7x7x3_1(x))))
        return torch.cat([b3, b7, max_pool_s2(x)], 1)


class InceptionE(nn.Module):
    def __init__(self, cin, pool):
        super().__init__()
        self.pool = pool                      # "avg" (Mixed_7b) or "max" (Mixed_7c: the FID variant)
        self.branch1x1 = BasicConv2d(cin, 320, kernel_size=1)
        self.branch3x3_1 = BasicConv2d(cin, 384, kernel_size=1)
        self.branch3x3_2a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3_2b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch3x3dbl_1 = BasicConv2d(cin, 448, kernel_size=1)
        self.branch3x3dbl_2 = BasicConv2d(448, 384, kernel_size=3, padding=1)
        self.branch3x3dbl_3a = BasicConv2d(384, 384, kernel_size=(1, 3), padding=(0, 1))
        self.branch3x3dbl_3b = BasicConv2d(384, 384, kernel_size=(3, 1), padding=(1, 0))
        self.branch_pool = BasicConv2d(cin, 192, kernel_size=1)

    def forward(self, x):
        b3 = self.branch3x3_1(x)
        b3 = torch.cat([self.branch3x3_2a(b3), self.branch3x3_2b(b3)], 1)
        bd = self.branch3x3dbl_2(self.branch3x3dbl_1(x))
        bd = torch.cat([self.branch3x3dbl_3a(bd), self.branch3x3dbl_3b(bd)], 1)
        pooled = avg_pool_valid(x) if self.pool == "avg" else max_pool_s1(x)
        return torch.cat([self.branch1x1(x), b3, bd, self.branch_pool(pooled)], 1)


class FidInceptionRef(nn.Module):
    def __init__(self):
        super().__init__()
        self.Conv2d_1a_3x3 = BasicConv2d(3, 32, kernel_size=3, stride=2)
        self.Conv2d_2a_3x3 = BasicConv2d(32, 32, kernel_size=3)
        self.Conv2d_2b_3x3 = BasicConv2d(32, 64, kernel_size=3, padding=1)
        self.Conv2d_3b_1x1 = BasicConv2d(64, 80, kernel_size=1)
        self.Conv2d_4a_3x3 = BasicConv2d(80, 192, kernel_size=3)
        self.Mixed_5b = InceptionA(192, 32)
        self.Mixed_5c = InceptionA(256, 64)
        self.Mixed_5d = InceptionA(288, 64)
        self.Mixed_6a = InceptionB(288)
        self.Mixed_6b = InceptionC(768, 128)
        self.Mixed_6c = InceptionC(768, 160)
        self.Mixed_6d = InceptionC(768, 160)
        self.Mixed_6e = InceptionC(768, 192)
        self.Mixed_7a = InceptionD(768)
        self.Mixed_7b = InceptionE(1280, "avg")
        self.Mixed_7c = InceptionE(2048, "max")

    def forward(self, images_u8, resize=True, sizes=None):
        """(B, H, W, 3) uint8 -> (B, 2048) in the tree's dtype; `sizes`: a list that receives the map side after every layer of the
        stem and every block"""
        dtype = self.Conv2d_1a_3x3.conv.weight.dtype
        x = images_u8.permute(0, 3, 1, 2).to(dtype)
        if resize:
            x = resize_bilinear(x, 299)
        x = x / 127.5 - 1
        chain = [self.Conv2d_1a_3x3, self.Conv2d_2a_3x3, self.Conv2d_2b_3x3, max_pool_s2, self.Conv2d_3b_1x1, self.Conv2d_4a_3x3, max_pool_s2,
                 self.Mixed_5b, self.Mixed_5c, self.Mixed_5d, self.Mixed_6a, self.Mixed_6b, self.Mixed_6c, self.Mixed_6d, self.Mixed_6e,
                 self.Mixed_7a, self.Mixed_7b, self.Mixed_7c]
        for layer in chain:
            x = layer(x)
            if sizes is not None:
                sizes.append(int(x.shape[2]))
        return x.mean(dim=(2, 3))


def make_state(seed=0):
    """Well-conditioned He-style test weights under the public key names: convolutions N(0, 2 / fan_in), BatchNorm scale and variance
    uniform in 0.75 .. 1.25, mean and bias small."""
    g = torch.Generator().manual_seed(seed)
    net = FidInceptionRef()
    sd = {}
    for k, v in net.state_dict().items():
        if k.endswith("conv.weight"):
            fan_in = v.shape[1] * v.shape[2] * v.shape[3]
            sd[k] = torch.randn(v.shape, generator=g) * (2.0 / fan_in) ** 0.5
        elif k.endswith(("bn.weight", "bn.running_var")):
            sd[k] = 0.75 + 0.5 * torch.rand(v.shape, generator=g)
        elif k.endswith(("bn.bias", "bn.running_mean")):
            sd[k] = 0.05 * torch.randn(v.shape, generator=g) + (0.05 if k.endswith("bn.bias") else 0.0)
        else:
            sd[k] = v.clone()                                     # num_batches_tracked
    return sd


def build(state, dtype=torch.float64, folded=False):
    """the tree in eval mode with `state` loaded; folded: BatchNorm folded in float64 (rounded once to `dtype`)"""
    net = FidInceptionRef().double()
    net.load_state_dict({k: v.double() if v.is_floating_point() else v for k, v in state.items()})
    net.eval()
    if folded:
        for m in net.modules():
            if isinstance(m, BasicConv2d):
                g = m.bn.weight.data / torch.sqrt(m.bn.running_var + BN_EPS)
                m.conv.weight.data = m.conv.weight.data * g.view(-1, 1, 1, 1)
                m.folded_bias = (m.bn.bias.data - m.bn.running_mean * g).to(dtype)
    return net.to(dtype)


# ------------------------------------------------------------------------------------------------------ statistics and distance
def stats_ref(features):
    f = np.asarray(features, dtype=np.float64)
    mu = f.sum(0) / f.shape[0]
    d = f - mu
    return mu, d.T @ d / (f.shape[0] - 1)


def frechet_ref(mu1, s1, mu2, s2):
    """through the symmetric form: tr sqrt(s1 s2) = tr sqrt(s1^1/2 s2 s1^1/2), by eigendecompositions"""
    w, v = np.linalg.eigh(s1)
    r1 = (v * np.sqrt(np.clip(w, 0, None))) @ v.T
    ev = np.linalg.eigvalsh(r1 @ s2 @ r1)
    return float(((mu1 - mu2) ** 2).sum() + np.trace(s1) + np.trace(s2) - 2 * np.sqrt(np.clip(ev, 0, None)).sum())


# -------------------------------------------------------------------------------------------------------------------------- cases
CASES = {"n75": dict(n=3, h=75, w=75, resize=False, seed=11), "n107": dict(n=2, h=107, w=107, resize=False, seed=12),
         "full": dict(n=1, h=512, w=512, resize=True, seed=13)}
STATE_SEED = 5


def case_images(name):
    c = CASES[name]
    g = torch.Generator().manual_seed(c["seed"])
    return torch.randint(0, 256, (c["n"], c["h"], c["w"], 3), generator=g, dtype=torch.uint8)


@functools.lru_cache(maxsize=None)
def shared_state():
    return make_state(STATE_SEED)


@functools.lru_cache(maxsize=None)
def case_reference(name):
    """-> (float64 features of the unfused tree, float32 features of the folded tree) as CPU tensors; computed once, never changed"""
    imgs, sd = case_images(name), shared_state()
    with torch.no_grad():
        r64 = build(sd, torch.float64)(imgs, resize=CASES[name]["resize"])
        r32 = build(sd, torch.float32, folded=True)(imgs, resize=CASES[name]["resize"])
    return r64, r32


def bound(e_ref, ref64):
    """the project's bound: 4 e_ref + 2e-6 max |ref64|"""
    return 4.0 * float(e_ref) + 2e-6 * float(ref64.abs().max())
