"""Restatement of the ResNet-50 face detector (csrc/detect_r50.hip, vspbfr_amd/detect_r50.py) for the tests: RetinaFace's
`Resnet50` network as a plain torch.nn tree under the checkpoint's key names (unfused, float64), its own BatchNorm fold, and the folded
network with the kernels' rounding points -- f16 weights, f16 activations between layers, fp32 stem weights, biases and head outputs --
evaluated in float64 or float32 on the CPU.  Priors, decode, selection and NMS are those of tests/detect_ref.py.  Nothing here imports
the product."""
import numpy as np
import torch
import torch.nn as nn
import torch.nn.functional as F

import detect_ref as R

LAYERS = ((1, 64, 3, 1), (2, 128, 4, 2), (3, 256, 6, 2), (4, 512, 3, 2))
BN3_SCALE = 0.25      # the last BatchNorm of every bottleneck: 16 residual additions then add at most a few units to an O(1) stream
BN_EPS = 1e-5


class Bottleneck(nn.Module):
    def __init__(self, cin, planes, stride, down):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(cin, planes, 1, bias=False), nn.BatchNorm2d(planes)
        self.conv2, self.bn2 = nn.Conv2d(planes, planes, 3, stride, 1, bias=False), nn.BatchNorm2d(planes)
        self.conv3, self.bn3 = nn.Conv2d(planes, 4 * planes, 1, bias=False), nn.BatchNorm2d(4 * planes)
        if down:
            self.downsample = nn.Sequential(nn.Conv2d(cin, 4 * planes, 1, stride, bias=False), nn.BatchNorm2d(4 * planes))

    def forward(self, x):
        t = torch.relu(self.bn1(self.conv1(x)))
        t = torch.relu(self.bn2(self.conv2(t)))
        t = self.bn3(self.conv3(t))
        return torch.relu(t + (self.downsample(x) if hasattr(self, "downsample") else x))


class Body(nn.Module):
    """torchvision's resnet50 without avgpool and fc, as an IntermediateLayerGetter keeps it: layer2, layer3 and layer4 are returned"""

    def __init__(self):
        super().__init__()
        self.conv1, self.bn1 = nn.Conv2d(3, 64, 7, 2, 3, bias=False), nn.BatchNorm2d(64)
        cin = 64
        for li, planes, blocks, stride in LAYERS:
            setattr(self, f"layer{li}", nn.Sequential(*[Bottleneck(cin if k == 0 else 4 * planes, planes, stride if k == 0 else 1, k == 0)
                                                        for k in range(blocks)]))
            cin = 4 * planes

    def forward(self, x):
        x = F.max_pool2d(torch.relu(self.bn1(self.conv1(x))), 3, 2, 1)
        b = self.layer2(self.layer1(x))
        c = self.layer3(b)
        return b, c, self.layer4(c)


class FPN(nn.Module):
    def __init__(self):
        super().__init__()
        self.output1, self.output2, self.output3 = R.c1(512, 256, 0.0), R.c1(1024, 256, 0.0), R.c1(2048, 256, 0.0)
        self.merge1, self.merge2 = R.cbl(256, 256, 1, 0.0), R.cbl(256, 256, 1, 0.0)

    def forward(self, a, b, c):
        o3 = self.output3(c)
        o2 = self.output2(b)
        o2 = self.merge2(o2 + R.nearest(o3, o2.shape[2], o2.shape[3]))
        o1 = self.output1(a)
        o1 = self.merge1(o1 + R.nearest(o2, o1.shape[2], o1.shape[3]))
        return o1, o2, o3


class SSH(nn.Module):
    def __init__(self):
        super().__init__()
        self.conv3X3 = R.cb(256, 128)
        self.conv5X5_1 = R.cbl(256, 64, 1, 0.0)
        self.conv5X5_2 = R.cb(64, 64)
        self.conv7X7_2 = R.cbl(64, 64, 1, 0.0)
        self.conv7x7_3 = R.cb(64, 64)

    def forward(self, x):
        t = self.conv5X5_1(x)
        return torch.relu(torch.cat([self.conv3X3(x), self.conv5X5_2(t), self.conv7x7_3(self.conv7X7_2(t))], dim=1))


class Head(nn.Module):
    def __init__(self, n):
        super().__init__()
        self.conv1x1 = nn.Conv2d(256, n, 1)

    def forward(self, x):
        y = self.conv1x1(x).permute(0, 2, 3, 1).contiguous()
        return y.view(y.shape[0], -1, y.shape[3] // 2)


class RetinaFaceR50(nn.Module):
    def __init__(self):
        super().__init__()
        self.body, self.fpn = Body(), FPN()
        self.ssh1, self.ssh2, self.ssh3 = SSH(), SSH(), SSH()
        self.ClassHead = nn.ModuleList([Head(4) for _ in range(3)])
        self.BboxHead = nn.ModuleList([Head(8) for _ in range(3)])
        self.LandmarkHead = nn.ModuleList([Head(20) for _ in range(3)])

    def forward(self, x):
        f = [ssh(v) for ssh, v in zip((self.ssh1, self.ssh2, self.ssh3), self.fpn(*self.body(x)))]
        return tuple(torch.cat([h(v) for h, v in zip(heads, f)], dim=1) for heads in (self.ClassHead, self.BboxHead, self.LandmarkHead))


def make_model(seed, class_bias=0.0):
    """A float64 RetinaFaceR50 in eval mode with well-conditioned random weights, as detect_ref.make_model: convolutions N(0, 1 / fan_in)
    (the stem divided by 64: its input is in grey levels), BatchNorm scale and variance in 0.75..1.25 with small shift and mean, the last
    BatchNorm of every bottleneck scaled by BN3_SCALE, head biases N(0, 0.3^2); class_bias is added to the background logit's bias."""
    g = torch.Generator().manual_seed(seed)
    net = RetinaFaceR50().double().eval()
    first = True
    with torch.no_grad():
        for name, m in net.named_modules():
            if isinstance(m, nn.Conv2d):
                fan_in = m.weight.shape[1] * m.weight.shape[2] * m.weight.shape[3]
                m.weight.copy_(torch.randn(m.weight.shape, generator=g, dtype=torch.float64) / fan_in ** 0.5 / (64.0 if first else 1.0))
                first = False
                if m.bias is not None:
                    m.bias.copy_(0.3 * torch.randn(m.bias.shape, generator=g, dtype=torch.float64))
            elif isinstance(m, nn.BatchNorm2d):
                n = m.weight.shape[0]
                m.weight.copy_((0.75 + 0.5 * torch.rand(n, generator=g, dtype=torch.float64)) * (BN3_SCALE if name.endswith(".bn3") else 1.0))
                m.bias.copy_(0.1 * torch.randn(n, generator=g, dtype=torch.float64))
                m.running_mean.copy_(0.1 * torch.randn(n, generator=g, dtype=torch.float64))
                m.running_var.copy_(0.75 + 0.5 * torch.rand(n, generator=g, dtype=torch.float64))
        for h in net.ClassHead:
            h.conv1x1.bias[0::2] += class_bias
    return net


def conv_bn_names(sd):
    """[(conv prefix, bn prefix)] of every conv + BatchNorm pair of a state dict, found by key: `convN` / `bnN` in the backbone, `.0` / `.1`
    of a Sequential everywhere else"""
    out = []
    for k in sd:
        if not k.endswith(".weight") or sd[k].dim() != 4 or "conv1x1" in k:
            continue
        p = k[:-len(".weight")]
        head, _, last = p.rpartition(".")
        out.append((p, f"{head}.bn{last[4:]}" if last.startswith("conv") else f"{head}.1"))
    return out


def fold(sd):
    """{conv prefix: (weight (Cout, Cin, k, k), bias)} in float64 with the BatchNorm folded in, and `heads.<k>`: (weight (32, 256, 1, 1),
    bias) with the class, box and landmark heads side by side"""
    sd = {k: v.double() for k, v in sd.items()}
    out = {}
    for conv, bn in conv_bn_names(sd):
        g = sd[bn + ".weight"] / torch.sqrt(sd[bn + ".running_var"] + BN_EPS)
        out[conv] = (sd[conv + ".weight"] * g.view(-1, 1, 1, 1), sd[bn + ".bias"] - sd[bn + ".running_mean"] * g)
    for k in range(3):
        out[f"heads.{k}"] = (torch.cat([sd[f"{h}.{k}.conv1x1.weight"] for h in ("ClassHead", "BboxHead", "LandmarkHead")]),
                             torch.cat([sd[f"{h}.{k}.conv1x1.bias"] for h in ("ClassHead", "BboxHead", "LandmarkHead")]))
    return out


def r16(t):
    """the rounding of an fp32 value to f16, kept in t's dtype"""
    return t.float().half().to(t.dtype)


def f16_half_ulp(v):
    """half an f16 ulp at the magnitude v (normal range: 2^-11 of the power of two below; subnormal: 2^-25)"""
    return 2.0 ** (np.floor(np.log2(max(float(v), 2.0 ** -14))) - 11)


def conv_ref(x, w, b, dtype, stride=1, relu=False, res=None, up=None, rounded=True):
    """One convolution of vsp_det50_conv_f16 before its final rounding: x, res, up hold f16 values, w is rounded to f16 and b to fp32 here
    (rounded=False: everything as given); (relu)(conv(x) + b (+ res)) (+ nearest x2 of up), in `dtype`"""
    w, b = (r16(w), b.float()) if rounded else (w, b)
    y = F.conv2d(x.to(dtype), w.to(dtype), b.to(dtype), stride=stride, padding=w.shape[2] // 2)
    if res is not None:
        y = y + res.to(dtype)
    if relu:
        y = torch.relu(y)
    if up is not None:
        y = y + R.nearest(up.to(dtype), y.shape[2], y.shape[3])
    return y


def stem_ref(photos, Hc, Wc, w, b, dtype, rounded=True):
    """relu(conv7x7/2/pad3(canvas) + b) with fp32 weights, before the rounding to f16"""
    w, b = (w.float(), b.float()) if rounded else (w, b)
    return torch.relu(F.conv2d(R.canvas(photos, Hc, Wc, dtype), w.to(dtype), b.to(dtype), stride=2, padding=3))


def heads_ref(x, w, b, dtype, rounded=True):
    """w (32, 256, 1, 1) and b in fp32 -> (conf, loc, lm) in the priors' layout"""
    w, b = (w.float(), b.float()) if rounded else (w, b)
    return R.heads_ref(x, w, b, dtype)


def forward(fw, photos, Hc, Wc, dtype, rounded=True):
    """The folded network of fold() on the canvas of `photos` -> (conf, loc, lm).  rounded: with the kernels' rounding points; else plain
    arithmetic in `dtype` (the fold's check against the unfused tree)."""
    q = r16 if rounded else (lambda t: t)

    def conv(name, x, **kw):
        return q(conv_ref(x, *fw[name], dtype, rounded=rounded, **kw))

    x = F.max_pool2d(q(stem_ref(photos, Hc, Wc, *fw["body.conv1"], dtype, rounded)), 3, 2, 1)
    feats = []
    for li, _, blocks, stride in LAYERS:
        for k in range(blocks):
            p, s = f"body.layer{li}.{k}", (stride if k == 0 else 1)
            t = conv(p + ".conv2", conv(p + ".conv1", x, relu=True), stride=s, relu=True)
            idn = conv(p + ".downsample.0", x, stride=s) if k == 0 else x
            x = conv(p + ".conv3", t, relu=True, res=idn)
        feats.append(x)
    o3 = conv("fpn.output3.0", feats[3], relu=True)
    o2 = conv("fpn.merge2.0", conv("fpn.output2.0", feats[2], relu=True, up=o3), relu=True)
    o1 = conv("fpn.merge1.0", conv("fpn.output1.0", feats[1], relu=True, up=o2), relu=True)
    outs = []
    for k, f in enumerate((o1, o2, o3)):
        n = f"ssh{k + 1}."
        t = conv(n + "conv5X5_1.0", f, relu=True)
        s = torch.cat([conv(n + "conv3X3.0", f, relu=True), conv(n + "conv5X5_2.0", t, relu=True),
                       conv(n + "conv7x7_3.0", conv(n + "conv7X7_2.0", t, relu=True), relu=True)], dim=1)
        outs.append(heads_ref(s, *fw[f"heads.{k}"], dtype, rounded))
    return tuple(torch.cat([o[i] for o in outs], dim=1) for i in range(3))


def pack_index(co, ci, t, cin, cout):
    """flat index into the weight image (taps, cin / 32, cout / 16, 64, 8) of w[co][ci][tap t], restated from include/vspbfr_hip.h"""
    nb, lp, kc, lg, j = co // 16, co % 16, ci // 32, (ci % 32) // 8, ci % 8
    return (((t * (cin // 32) + kc) * (cout // 16) + nb) * 64 + lg * 16 + lp) * 8 + j
