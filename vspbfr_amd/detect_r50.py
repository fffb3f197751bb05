"""Face detection for whole photos with the ResNet-50 backbone: RetinaFace's `Resnet50` network -- the detector GFPGAN,
CodeFormer and Real-ESRGAN's face helper load by default -- on the device, the host side of csrc/detect_r50.hip.  detect.load_detector
sends a checkpoint that holds `body.layer1.0.conv1.weight` here; the CLIs, the canvas, the post-processing and the landmark file are
those of vspbfr_amd.detect.

    expected_state / check_state_dict   the key layout of the public `Resnet50_Final.pth` (456 entries) and the loader's rules (detect.py's)
    fold_state                          BatchNorm folded into weight and bias in float64, in the kernels' layouts
    pack_conv_weight / unpack_conv_weight, pack_stem
    RetinaFaceR50Detector               weights -> network(), postprocess(), canvas(), detect() as RetinaFaceDetector

No weights are shipped.  The key layout is written from the public model definition (torchvision's resnet50 under `body.` through an
IntermediateLayerGetter, the 256-channel FPN and SSH, three times three 1x1 heads) and could not be checked against a real checkpoint
file; a file that deviates is refused by key name, never half-loaded.

Arithmetic: the stem (7x7 / 2, fp32 weights) and the heads (fp32 weights) are fmaf chains; the 70 convolutions between them run on
v_mfma_f32_16x16x32_f16 with f16 weights, f16 NHWC activations, fp32 accumulation and fp32 biases.  The output width is 256 > 64, so
every FPN and SSH activation is LeakyReLU with slope 0: ReLU.  An image's result depends neither on the batch size nor on its place in
the batch, so a group whose activations would reach 2 GiB runs in chunks of images and gives the same bits."""
import os

import torch

from . import detect as D
from .detect import BN_KEYS, HEADS, level_sizes, num_priors

WHAT = "RetinaFace resnet50 checkpoint"
LAYERS = ((1, 64, 3, 1), (2, 128, 4, 2), (3, 256, 6, 2), (4, 512, 3, 2))     # (layer, planes, blocks, stride of block 0's conv2)
FPN_IN, OUT = (512, 1024, 2048), 256
SSH = (("conv3X3", 256, 128), ("conv5X5_1", 256, 64), ("conv5X5_2", 64, 64), ("conv7X7_2", 64, 64), ("conv7x7_3", 64, 64))


def conv_units():
    """[(prefix of the conv, prefix of its BatchNorm, weight shape, stride)] of every conv + BN pair, in checkpoint order: 73"""
    units = [("body.conv1", "body.bn1", (64, 3, 7, 7), 2)]
    cin = 64
    for li, planes, blocks, stride in LAYERS:
        for k in range(blocks):
            p, s = f"body.layer{li}.{k}", (stride if k == 0 else 1)
            units.append((f"{p}.conv1", f"{p}.bn1", (planes, cin, 1, 1), 1))
            units.append((f"{p}.conv2", f"{p}.bn2", (planes, planes, 3, 3), s))
            units.append((f"{p}.conv3", f"{p}.bn3", (4 * planes, planes, 1, 1), 1))
            if k == 0:
                units.append((f"{p}.downsample.0", f"{p}.downsample.1", (4 * planes, cin, 1, 1), s))
            cin = 4 * planes
    for k, ci in zip((1, 2, 3), FPN_IN):
        units.append((f"fpn.output{k}.0", f"fpn.output{k}.1", (OUT, ci, 1, 1), 1))
    for k in (1, 2):
        units.append((f"fpn.merge{k}.0", f"fpn.merge{k}.1", (OUT, OUT, 3, 3), 1))
    for k in (1, 2, 3):
        for name, ci, co in SSH:
            units.append((f"ssh{k}.{name}.0", f"ssh{k}.{name}.1", (co, ci, 3, 3), 1))
    return units


def expected_state(with_tracked=True):
    """{key: shape} of the checkpoint: 73 conv + BN pairs and nine 1x1 heads, 456 entries with the BatchNorm counters"""
    out = {}
    for conv, bn, shape, _ in conv_units():
        out[conv + ".weight"] = shape
        for k in BN_KEYS:
            out[f"{bn}.{k}"] = (shape[0],)
        if with_tracked:
            out[bn + ".num_batches_tracked"] = ()
    for head, n in HEADS:
        for k in range(3):
            out[f"{head}.{k}.conv1x1.weight"] = (n, OUT, 1, 1)
            out[f"{head}.{k}.conv1x1.bias"] = (n,)
    return out


def check_state_dict(sd):
    """detect.check_state_dict's rules on this layout -> {key: float64 CPU tensor}"""
    return D.check_state_dict(sd, expected_state(with_tracked=False), WHAT)


def pack_conv_weight(w):
    """(Cout, Cin, k, k), Cout a multiple of 16 and Cin of 32 -> the image (k k, Cin / 32, Cout / 16, 64, 8) vsp_det50_conv_f16 reads:
    element j of lane l of block nb of step kc of tap t = w[16 nb + (l & 15)][32 kc + 8 (l >> 4) + j][t // k][t % k]"""
    co, ci, kh, kw = w.shape
    if co % 16 or ci % 32 or kh != kw:
        raise ValueError(f"pack_conv_weight: weight {tuple(w.shape)}")
    v = w.reshape(co // 16, 16, ci // 32, 4, 8, kh * kw)            # nb, l & 15, kc, l >> 4, j, t
    return v.permute(5, 2, 0, 3, 1, 4).reshape(kh * kw, ci // 32, co // 16, 64, 8).contiguous()


def unpack_conv_weight(img):
    """the inverse of pack_conv_weight"""
    t, nkc, nb = img.shape[:3]
    k = int(round(t ** 0.5))
    v = img.reshape(t, nkc, nb, 4, 16, 8).permute(2, 4, 1, 3, 5, 0)  # nb, l & 15, kc, l >> 4, j, t
    return v.reshape(16 * nb, 32 * nkc, k, k).contiguous()


def pack_stem(w):
    """(64, 3, 7, 7) -> (147, 64), row (7 ky + kx) 3 + channel: the layout of vsp_det50_stem_u8"""
    return w.permute(2, 3, 1, 0).reshape(147, 64).contiguous()


def fold_state(sd):
    """Checked state dict -> {name: float64 tensor} in the kernels' layouts: `<conv prefix>.w` / `.b` for every conv + BN pair (the stem
    through pack_stem, every other through pack_conv_weight) and `heads.<k>.w` (256, 32) / `.b` (32) with the class, box and landmark
    heads of level k side by side, as detect.fold_state lays them"""
    out = {}
    for conv, bn, shape, _ in conv_units():
        w, b = D.fold_bn(sd, conv, bn)
        out[conv + ".w"], out[conv + ".b"] = (pack_stem(w) if shape[1] == 3 else pack_conv_weight(w)), b
    for k in range(3):
        out[f"heads.{k}.w"] = D.pack_pointwise(torch.cat([sd[f"{h}.{k}.conv1x1.weight"] for h, _ in HEADS]))
        out[f"heads.{k}.b"] = torch.cat([sd[f"{h}.{k}.conv1x1.bias"] for h, _ in HEADS])
    return out


def image_bytes(Hc, Wc):
    """bytes of the largest activation tensor of one image of an (Hc, Wc) canvas: the stem's output, (Hc / 2, Wc / 2, 64) f16 (layer1's
    (Hc / 4, Wc / 4, 256) is as large)"""
    return ((Hc + 1) // 2) * ((Wc + 1) // 2) * 64 * 2


class RetinaFaceR50Detector(D.RetinaFaceDetector):
    """weights: a path (torch.load) or a state dict in the `Resnet50` RetinaFace layout -> the detector on `device`, with
    RetinaFaceDetector's interface; canvas(), postprocess() and detect() are its own.  BatchNorm is folded once, here, in float64; the
    convolutions' weights are then rounded to f16.  There is no fallback: a layer the kernels refuse raises."""
    backbone = "resnet50"
    GUARD_BYTES = 1 << 31            # an activation tensor must stay below this: larger batches run in chunks of images

    def __init__(self, weights, device):
        if isinstance(weights, (str, os.PathLike)):
            weights = torch.load(weights, map_location="cpu")
        self.device = torch.device(device)
        self.folded = fold_state(check_state_dict(weights))
        self.p = {}
        for k, v in self.folded.items():
            half = k.endswith(".w") and v.dim() == 5
            self.p[k] = v.to(torch.float16 if half else torch.float32).contiguous().to(self.device)
        self.device = self.p["heads.0.b"].device               # with its index

    # ------------------------------------------------------------------------------------------------------------------- network
    def network(self, sources, B, Hc, Wc):
        """sources: [(flat uint8 device buffer, [(byte offset, h, w, slot), ...]), ...] that together fill slots 0 .. B - 1 of the
        canvas batch -> (conf (B, P, 2), loc (B, P, 4), lm (B, P, 10)) on the device.  Hc and Wc are multiples of 32 (canvas() makes
        them so): each pyramid level is then exactly twice the next."""
        B, Hc, Wc = int(B), int(Hc), int(Wc)
        if Hc < 32 or Wc < 32 or Hc % 32 or Wc % 32:
            raise ValueError(f"RetinaFaceR50Detector.network: canvas {Hc} x {Wc}, the sides must be multiples of 32")
        slots = sorted(s for _, items in sources for *_, s in items)
        if slots != list(range(B)):
            raise ValueError(f"RetinaFaceR50Detector.network: the sources fill slots {slots}, not 0..{B - 1}")
        per = (self.GUARD_BYTES - 1) // image_bytes(Hc, Wc)
        if per < 1:
            raise ValueError(f"RetinaFaceR50Detector.network: one image of a {Hc} x {Wc} canvas has activation tensors of "
                             f"{image_bytes(Hc, Wc)} bytes, {self.GUARD_BYTES} or more are not served")
        if B <= per:
            return self._network(sources, B, Hc, Wc)
        parts = []
        for lo in range(0, B, per):
            hi = min(lo + per, B)
            sub = [(buf, [(off, h, w, s - lo) for off, h, w, s in items if lo <= s < hi]) for buf, items in sources]
            parts.append(self._network(sub, hi - lo, Hc, Wc))
        return tuple(torch.cat([q[i] for q in parts], dim=0) for i in range(3))

    def _conv(self, name, x, B, stride=1, relu=True, res=None, up=None, out=None, y_off=0):
        """x, res, up, out: (flat f16 tensor, pitch, H, W) -> the output in the same form (a new dense tensor unless `out` is given)"""
        from . import hip_ops as H
        w, b = self.p[name + ".w"], self.p[name + ".b"]
        oh, ow = H.det50_out_size(x[2], x[3], stride)
        if out is None:
            cout = 16 * int(w.shape[2])
            out = (torch.empty(B * oh * ow * cout, device=self.device, dtype=torch.float16), cout, oh, ow)
        H.det50_conv_f16(out[0], out[1], y_off, x[0], x[1], 0, B, x[2], x[3], w, b, stride, relu,
                         res=None if res is None else (res[0], res[1], 0), up=None if up is None else (up[0], up[1], 0))
        return out

    def _network(self, sources, B, Hc, Wc):
        from . import _lib, hip_ops as H
        p, dev = self.p, self.device
        h2, w2 = H.det50_out_size(Hc, Wc, 2)
        stem = torch.empty(B * h2 * w2 * 64, device=dev, dtype=torch.float16)
        for buf, items in sources:
            if not items:
                continue
            tab = (_lib.DetSrc * len(items))()
            for t, (off, h, w, slot) in zip(tab, items):
                t.off, t.h, t.w, t.slot = int(off), int(h), int(w), int(slot)
            tab_dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(dev)
            H.det50_stem_u8(stem, buf, tab, tab_dev, len(items), p["body.conv1.w"], p["body.conv1.b"], B, Hc, Wc)
        h4, w4 = H.det50_out_size(h2, w2, 2)
        x = (H.det50_pool_f16(torch.empty(B * h4 * w4 * 64, device=dev, dtype=torch.float16), stem, B, h2, w2, 64), 64, h4, w4)
        del stem
        feats = []
        for li, _, blocks, stride in LAYERS:
            for k in range(blocks):
                q, s = f"body.layer{li}.{k}", (stride if k == 0 else 1)
                t = self._conv(q + ".conv2", self._conv(q + ".conv1", x, B), B, stride=s)
                idn = self._conv(q + ".downsample.0", x, B, stride=s, relu=False) if k == 0 else x
                x = self._conv(q + ".conv3", t, B, res=idn, out=idn)          # relu(conv3 + identity) replaces the identity
            feats.append(x)
        o3 = self._conv("fpn.output3.0", feats[3], B)
        o2 = self._conv("fpn.merge2.0", self._conv("fpn.output2.0", feats[2], B, up=o3), B)
        o1 = self._conv("fpn.merge1.0", self._conv("fpn.output1.0", feats[1], B, up=o2), B)
        P = num_priors(Hc, Wc)
        conf = torch.empty((B, P, 2), device=dev, dtype=torch.float32)
        loc = torch.empty((B, P, 4), device=dev, dtype=torch.float32)
        lm = torch.empty((B, P, 10), device=dev, dtype=torch.float32)
        p0 = 0
        for k, f in enumerate((o1, o2, o3)):
            assert (f[2], f[3]) == level_sizes(Hc, Wc)[k]
            s = self.ssh(k + 1, f, B)
            H.det50_heads(s[0], s[1], B, s[2], s[3], p[f"heads.{k}.w"], p[f"heads.{k}.b"], conf, loc, lm, p0)
            p0 += 2 * f[2] * f[3]
        return conf, loc, lm

    def ssh(self, k, x, B):
        """relu(cat[conv3X3(x), conv5X5_2(t), conv7x7_3(conv7X7_2(t))]), t = relu(conv5X5_1(x)): the three branches write their channel
        windows 0..127, 128..191, 192..255 of one tensor"""
        out = (torch.empty(B * x[2] * x[3] * OUT, device=self.device, dtype=torch.float16), OUT, x[2], x[3])
        self._conv(f"ssh{k}.conv3X3.0", x, B, out=out, y_off=0)
        t = self._conv(f"ssh{k}.conv5X5_1.0", x, B)
        self._conv(f"ssh{k}.conv5X5_2.0", t, B, out=out, y_off=128)
        self._conv(f"ssh{k}.conv7x7_3.0", self._conv(f"ssh{k}.conv7X7_2.0", t, B), B, out=out, y_off=192)
        return out
