"""Facial landmarks for the LMD column: face_alignment's 2D-FAN -- 68 points from stacked hourglasses of pre-activated
residual blocks -- on the device, the host side of csrc/fan.hip.

    expected_state / check_state_dict   the key layout of the public `2DFAN4-11f355bf06.pth.tar` (945 entries, 1129 with the BatchNorm
                                        counters a newer torch would add) and the loader's rules (detect.check_state_dict's)
    reduce_state                        every BatchNorm as a per-channel (a, b) pair in float64; the two kinds that FOLLOW a convolution
                                        (`bn1`, `bn_end{i}`) folded into it
    pack_conv_weight / unpack_conv_weight, pack_stem, pack_image
    FanLandmarks                        weights -> heatmaps(), landmarks(), describe()
    lmd_nme                             the per-image landmark distance of two landmark sets, on the device
    python -m vspbfr_amd.fan --faces DIR --weights W --out landmarks68.json [--box X0,Y0,SIDE]

No weights are shipped.  The key layout is written from the public model definition (face_alignment/models.py: ConvBlock, HourGlass,
FAN) and could not be checked against a real checkpoint file; a file that deviates is refused by key name, never half-loaded.  The
TorchScript archives that newer face_alignment releases ship hold no state dict under these names and are refused with a message
that says so.

Arithmetic: the stem (7x7 / 2 on the sampled crop, fp32 weights) is an fmaf chain; every other convolution runs on
v_mfma_f32_16x16x32_f16 with f16 weights, f16 NHWC activations and fp32 accumulation.  FAN is pre-activated: BatchNorm + ReLU stand
in FRONT of a convolution, on a tensor that also feeds the residual, so they are the convolution's input affine
f16(relu(a x + b)) -- a rounding point -- and no weight absorbs them.  Rounding points of a ConvBlock: o1 and o2 are stored as
f16(acc) for the next convolution, and the block's output window takes f16(acc + residual [+ coarser level]) from the same fp32 sum.
An hourglass level runs its lower branch first, so `up1 + nearest2(low)` is the epilogue of `b1_l`'s three convolutions.
`previous + bl(ll) + al(heatmaps)` is f16(al(..) + bias + previous + f16(bl(ll) + bias)).  An image's bits depend neither on the batch
size nor on its place in the batch, so a group whose activations would reach 2 GiB runs in chunks of images with the same bits.

Crop protocol (ours): a box (x0, y0, s) per image, default the whole image (0, 0, max(H, W)).  The stem samples the box to
side x side bilinearly at half-pixel centres, without anti-aliasing, zero outside the image, and divides by 255; for a 512 x 512 aligned
face and side 256 that is the exact 2 x 2 mean.  A landmark is x0 + (px + 0.5 +- 0.25) s / (side / 4): face_alignment's get_preds_fromhm
followed by its inverse transform."""
import argparse
import json
import os
import zipfile

import torch

from . import detect as D
from .detect import BN_KEYS

WHAT = "2D-FAN checkpoint"
BN_EPS = 1e-5
POINTS = 68
POINTS_PAD = 96             # the 68-channel input of `al` as a window of 96 channels, the last 28 zero


def block_units(prefix, cin, cout):
    """[(key prefix, kind, shape)] of a ConvBlock(cin, cout): kind `bn` (shape = channels) or `conv` (weight shape, no bias)"""
    u = [(f"{prefix}.bn1", "bn", cin), (f"{prefix}.conv1", "conv", (cout // 2, cin, 3, 3)),
         (f"{prefix}.bn2", "bn", cout // 2), (f"{prefix}.conv2", "conv", (cout // 4, cout // 2, 3, 3)),
         (f"{prefix}.bn3", "bn", cout // 4), (f"{prefix}.conv3", "conv", (cout // 4, cout // 4, 3, 3))]
    if cin != cout:
        u += [(f"{prefix}.downsample.0", "bn", cin), (f"{prefix}.downsample.2", "conv", (cout, cin, 1, 1))]
    return u


def hourglass_blocks(prefix, depth):
    """the ConvBlock prefixes of an HourGlass in the order the reference registers them"""
    out = []
    for level in range(depth, 0, -1):
        out += [f"{prefix}.b1_{level}", f"{prefix}.b2_{level}"]
        if level == 1:
            out.append(f"{prefix}.b2_plus_{level}")
        out.append(f"{prefix}.b3_{level}")
    return out


def expected_state(num_modules=4, depth=4, with_tracked=False):
    """{key: shape} of the checkpoint: 945 entries for 2D-FAN-4 (1129 with the BatchNorm counters)"""
    out = {}

    def bn(p, n):
        for k in BN_KEYS:
            out[f"{p}.{k}"] = (n,)
        if with_tracked:
            out[p + ".num_batches_tracked"] = ()

    def conv(p, shape, bias):
        out[p + ".weight"] = tuple(shape)
        if bias:
            out[p + ".bias"] = (shape[0],)

    def block(p, cin, cout):
        for name, kind, shape in block_units(p, cin, cout):
            bn(name, shape) if kind == "bn" else conv(name, shape, False)

    conv("conv1", (64, 3, 7, 7), True), bn("bn1", 64)
    block("conv2", 64, 128), block("conv3", 128, 128), block("conv4", 128, 256)
    for i in range(num_modules):
        for p in hourglass_blocks(f"m{i}", depth):
            block(p, 256, 256)
        block(f"top_m_{i}", 256, 256)
        conv(f"conv_last{i}", (256, 256, 1, 1), True), bn(f"bn_end{i}", 256)
        conv(f"l{i}", (POINTS, 256, 1, 1), True)
        if i < num_modules - 1:
            conv(f"bl{i}", (256, 256, 1, 1), True), conv(f"al{i}", (256, POINTS, 1, 1), True)
    return out


def modules_of(sd):
    """the number of hourglass modules and their depth that a state dict's keys name (after `module.` stripping)"""
    keys = [k[len("module."):] if str(k).startswith("module.") else str(k) for k in sd]
    mods = {int(k[1:k.index(".")]) for k in keys if k.startswith("l") and k[1:k.find(".")].isdigit() and k.endswith(".weight")}
    depths = {int(k.split(".")[1][3:]) for k in keys if k.startswith("m0.b1_") and k.split(".")[1][3:].isdigit()}
    return (max(mods) + 1 if mods else 0), (max(depths) if depths else 0)


def is_torchscript_archive(path):
    """a zip archive with TorchScript's `code/` tree or `constants.pkl`: what torch.jit.save writes"""
    if not zipfile.is_zipfile(path):
        return False
    with zipfile.ZipFile(path) as z:
        return any("/code/" in "/" + n or n.endswith("constants.pkl") for n in z.namelist())


SCRIPT_MESSAGE = ("a TorchScript archive (the format newer face_alignment releases ship) holds no state dict under the model "
                  "definition's key names and is not served; supply the state dict of 2DFAN4-11f355bf06.pth.tar")


def load_weights(weights):
    """a path or a state dict -> the state dict; a TorchScript archive or module is refused"""
    if isinstance(weights, (str, os.PathLike)):
        if not os.path.isfile(weights):
            raise ValueError(f"{WHAT}: no such file: {weights}")
        if is_torchscript_archive(weights):
            raise ValueError(f"{WHAT}: {weights}: {SCRIPT_MESSAGE}")
        weights = torch.load(weights, map_location="cpu")
    if isinstance(weights, torch.jit.ScriptModule):
        raise ValueError(f"{WHAT}: {SCRIPT_MESSAGE}")
    if not isinstance(weights, dict):
        raise ValueError(f"{WHAT}: expected a state dict, got {type(weights).__name__}")
    return weights


def check_state_dict(sd, num_modules=None, depth=None):
    """detect.check_state_dict's rules on this layout -> ({key: float64 CPU tensor}, num_modules, depth); num_modules and depth come
    from the keys unless given"""
    sd = load_weights(sd)
    if isinstance(sd, dict) and "state_dict" in sd and not any(str(k).endswith(".weight") for k in sd):
        sd = sd["state_dict"]
    nm, dp = modules_of(sd)
    nm, dp = (nm if num_modules is None else int(num_modules)), (dp if depth is None else int(depth))
    if nm < 1 or dp < 1:
        raise ValueError(f"{WHAT}: missing keys l0.weight, m0.b1_1.conv1.weight: no hourglass module found")
    return D.check_state_dict(sd, expected_state(nm, dp), WHAT), nm, dp


def bn_affine(sd, p):
    """BatchNorm (eval) as y = a x + b per channel, float64"""
    a = sd[p + ".weight"] / torch.sqrt(sd[p + ".running_var"] + BN_EPS)
    return a, sd[p + ".bias"] - sd[p + ".running_mean"] * a


def pack_conv_weight(w):
    """(Cout, Cin, k, k), Cin a multiple of 32 -> the image (k k, Cin / 32, Cp / 16, 64, 8) vsp_fan_conv_f16 reads, Cp = Cout rounded up
    to 32 with zero rows: element j of lane l of block nb of step kc of tap t = w[16 nb + (l & 15)][32 kc + 8 (l >> 4) + j][t // k][t % k]"""
    co, ci, kh, kw = w.shape
    if ci % 32 or kh != kw:
        raise ValueError(f"pack_conv_weight: weight {tuple(w.shape)}")
    cp = (co + 31) // 32 * 32
    if cp != co:
        w = torch.cat([w, w.new_zeros(cp - co, ci, kh, kw)])
    v = w.reshape(cp // 16, 16, ci // 32, 4, 8, kh * kw)            # nb, l & 15, kc, l >> 4, j, t
    return v.permute(5, 2, 0, 3, 1, 4).reshape(kh * kw, ci // 32, cp // 16, 64, 8).contiguous()


def unpack_conv_weight(img, cout=None):
    """the inverse of pack_conv_weight (the first `cout` rows)"""
    t, nkc, nb = img.shape[:3]
    k = int(round(t ** 0.5))
    v = img.reshape(t, nkc, nb, 4, 16, 8).permute(2, 4, 1, 3, 5, 0)  # nb, l & 15, kc, l >> 4, j, t
    w = v.reshape(16 * nb, 32 * nkc, k, k)
    return (w if cout is None else w[:cout]).contiguous()


def pad_cin(w, cin):
    """zero input channels up to cin: `al`'s 68 -> 96"""
    return torch.cat([w, w.new_zeros(w.shape[0], cin - w.shape[1], *w.shape[2:])], dim=1) if w.shape[1] != cin else w


def pack_stem(w):
    """(64, 3, 7, 7) -> (147, 64), row (7 ky + kx) 3 + channel: the layout of vsp_fan_stem_u8"""
    return w.permute(2, 3, 1, 0).reshape(147, 64).contiguous()


def reduce_state(sd, num_modules, depth):
    """Checked state dict -> {name: float64 tensor}: `<conv>.w` (Cout, Cin, k, k) [+ `<conv>.b`] of every convolution -- `conv1` with `bn1`
    and `conv_last{i}` with `bn_end{i}` folded in, `al{i}` padded to 96 input channels -- and `<bn>.a` / `<bn>.b` of every BatchNorm
    that stands in front of a convolution"""
    out = {}
    w, b = D.fold_bn(sd, "conv1", "bn1")
    a = sd["bn1.weight"] / torch.sqrt(sd["bn1.running_var"] + BN_EPS)
    out["conv1.w"], out["conv1.b"] = w, b + sd["conv1.bias"] * a

    def block(p, cin, cout):
        for name, kind, _ in block_units(p, cin, cout):
            if kind == "bn":
                out[name + ".a"], out[name + ".b"] = bn_affine(sd, name)
            else:
                out[name + ".w"] = sd[name + ".weight"]

    block("conv2", 64, 128), block("conv3", 128, 128), block("conv4", 128, 256)
    for i in range(num_modules):
        for p in hourglass_blocks(f"m{i}", depth) + [f"top_m_{i}"]:
            block(p, 256, 256)
        a, s = bn_affine(sd, f"bn_end{i}")
        out[f"conv_last{i}.w"] = sd[f"conv_last{i}.weight"] * a.view(-1, 1, 1, 1)
        out[f"conv_last{i}.b"] = sd[f"conv_last{i}.bias"] * a + s
        out[f"l{i}.w"], out[f"l{i}.b"] = sd[f"l{i}.weight"], sd[f"l{i}.bias"]
        if i < num_modules - 1:
            out[f"bl{i}.w"], out[f"bl{i}.b"] = sd[f"bl{i}.weight"], sd[f"bl{i}.bias"]
            out[f"al{i}.w"], out[f"al{i}.b"] = pad_cin(sd[f"al{i}.weight"], POINTS_PAD), sd[f"al{i}.bias"]
    return out


def pack_image(red):
    """reduce_state's output -> (one flat float16 tensor with every MFMA convolution's packed image, {name: (offset, image shape, Cout)},
    {name: float32 tensor} of the stem's weights, the biases and the affines)"""
    parts, index, f32, at = [], {}, {}, 0
    for k, v in red.items():
        if k.endswith(".w") and k != "conv1.w":
            img = pack_conv_weight(v).to(torch.float16)
            index[k[:-2]] = (at, tuple(img.shape), int(v.shape[0]))
            parts.append(img.reshape(-1))
            at += img.numel()
        else:
            f32[k] = (pack_stem(v) if k == "conv1.w" else v).to(torch.float32).contiguous()
    return torch.cat(parts), index, f32


def image_bytes(side):
    """bytes of the largest activation tensor of one image: conv2's output, (side / 2, side / 2, 128) f16"""
    return (side // 2) * (side // 2) * 128 * 2


def parse_box(text):
    """`X0,Y0,SIDE` -> (x0, y0, s); ValueError otherwise"""
    try:
        x0, y0, s = (float(v) for v in str(text).split(","))
    except ValueError:
        raise ValueError(f"a box is X0,Y0,SIDE (got {text!r})") from None
    if not (s > 0 and all(abs(v) < 1e6 for v in (x0, y0, s))):
        raise ValueError(f"a box needs a positive side and finite corners (got {text!r})")
    return x0, y0, s


def lmd_nme(lm, lm_gt):
    """(B, 68, 2) landmarks of the restored image and of its ground truth, on one device -> (lmd, nme) float64 (B,): the mean over the
    points of the Euclidean distance in image pixels, and that divided by the distance between ground-truth points 36 and 45 (the
    outer eye corners).  torch ops on the tensors' device: no host copy."""
    a, g = lm.to(torch.float64), lm_gt.to(torch.float64)
    d = torch.sqrt(((a - g) ** 2).sum(dim=2)).mean(dim=1)
    return d, d / torch.sqrt(((g[:, 36] - g[:, 45]) ** 2).sum(dim=1))


class FanLandmarks:
    """weights: a path (torch.load) or a state dict in 2D-FAN's layout -> the landmark network on `device`.  num_modules and depth come
    from the keys unless given (a narrower network at full channel widths serves the tests); side is the crop's side, a multiple of
    2^(depth + 2).  BatchNorm is reduced once, here, in float64; the weights are then rounded to f16.  There is no fallback: a layer
    the kernels refuse raises."""
    GUARD_BYTES = 1 << 31            # an activation tensor must stay below this: larger batches run in chunks of images

    def __init__(self, state, device, num_modules=None, depth=None, side=256):
        sd, self.num_modules, self.depth = check_state_dict(state, num_modules, depth)
        self.side = int(side)
        if self.side < 8 << self.depth or self.side % (4 << self.depth) or self.side > 1024:      # the bottom level is at least 2 x 2
            raise ValueError(f"FanLandmarks: side {side} must be a multiple of {4 << self.depth} in {8 << self.depth}..1024 for depth {self.depth}")
        self.reduced = reduce_state(sd, self.num_modules, self.depth)
        image, self.index, f32 = pack_image(self.reduced)
        self.device = torch.device(device)
        self.image = image.to(self.device)
        self.p = {k: v.to(self.device) for k, v in f32.items()}
        self.device = self.image.device               # with its index
        self.launches = 0

    def describe(self):
        return {"network": "2D-FAN", "num_modules": self.num_modules, "depth": self.depth, "side": self.side, "points": POINTS,
                "convolutions": len(self.index) + 1, "weight_image_bytes": int(self.image.numel()) * 2,
                "parameters": int(sum(v.numel() for k, v in self.reduced.items() if k.endswith(".w")))}

    # ----------------------------------------------------------------------------------------------------------------- launches
    def _w(self, name):
        at, shape, cout = self.index[name]
        n = 1
        for s in shape:
            n *= s
        return self.image[at:at + n].view(shape), cout

    def _new(self, B, h, w, c, dtype=torch.float16, zero=False):
        make = torch.zeros if zero else torch.empty
        return make(B * h * w * c, device=self.device, dtype=dtype)

    def _conv(self, name, x, B, y, bn=None, bias=False, **kw):
        """x: (buffer, pitch, H, W); y: (buffer, pitch, offset)"""
        from . import hip_ops as H
        w, cout = self._w(name)
        aff = None if bn is None else (self.p[bn + ".a"], self.p[bn + ".b"])
        self.launches += 1
        H.fan_conv_f16(y, (x[0], x[1], 0), B, x[2], x[3], w, cout, b=self.p[name + ".b"] if bias else None, affine=aff, **kw)

    def _block(self, p, x, B, cin, cout, up=None):
        """ConvBlock: cat(o1, o2, o3) + (downsample(x) or x) [+ nearest2(up)] -> (buffer, cout, H, W)"""
        h, w = x[2], x[3]
        out = self._new(B, h, w, cout)
        half, quarter = cout // 2, cout // 4
        if cin != cout:      # the residual is written first and replaced in place
            self._conv(p + ".downsample.2", x, B, (out, cout, 0), bn=p + ".downsample.0")
            res = (out, cout)
        else:
            res = (x[0], x[1])
        o1, o2 = self._new(B, h, w, half), self._new(B, h, w, quarter)
        u = (lambda off: None) if up is None else (lambda off: (up[0], up[1], off))
        self._conv(p + ".conv1", x, B, (out, cout, 0), bn=p + ".bn1", raw=(o1, half, 0), res1=(*res, 0), up=u(0))
        self._conv(p + ".conv2", (o1, half, h, w), B, (out, cout, half), bn=p + ".bn2", raw=(o2, quarter, 0), res1=(*res, half), up=u(half))
        self._conv(p + ".conv3", (o2, quarter, h, w), B, (out, cout, half + quarter), bn=p + ".bn3", res1=(*res, half + quarter),
                   up=u(half + quarter))
        return (out, cout, h, w)

    def _pool(self, x, B, c):
        from . import hip_ops as H
        y = self._new(B, x[2] // 2, x[3] // 2, c)
        self.launches += 1
        H.fan_pool_f16((y, c, 0), (x[0], x[1], 0), B, x[2], x[3], c)
        return (y, c, x[2] // 2, x[3] // 2)

    def _hourglass(self, p, level, x, B):
        """the lower branch first: up1 + nearest2(low) is then the epilogue of b1_l's convolutions"""
        low = self._block(f"{p}.b2_{level}", self._pool(x, B, 256), B, 256, 256)
        low = self._hourglass(p, level - 1, low, B) if level > 1 else self._block(f"{p}.b2_plus_{level}", low, B, 256, 256)
        low = self._block(f"{p}.b3_{level}", low, B, 256, 256)
        return self._block(f"{p}.b1_{level}", x, B, 256, 256, up=low)

    def _network(self, u8, box):
        """(B, H, W, 3) u8 and (B, 3) boxes -> the last module's heatmaps as a flat fp32 buffer (B, n, n, 68)"""
        from . import hip_ops as H
        B, s2 = int(u8.shape[0]), self.side // 2
        stem = self._new(B, s2, s2, 64)
        self.launches += 1
        H.fan_stem_u8(stem, u8, box, self.p["conv1.w"], self.p["conv1.b"], self.side)
        x = self._block("conv2", (stem, 64, s2, s2), B, 64, 128)
        x = self._pool(x, B, 128)
        x = self._block("conv3", x, B, 128, 128)
        prev = self._block("conv4", x, B, 128, 256)
        n = prev[2]
        heat = None
        for i in range(self.num_modules):
            last = i == self.num_modules - 1
            ll = self._block(f"top_m_{i}", self._hourglass(f"m{i}", self.depth, prev, B), B, 256, 256)
            t = self._new(B, n, n, 256)
            self._conv(f"conv_last{i}", ll, B, (t, 256, 0), bias=True, relu=True)
            heat = self._new(B, n, n, POINTS, torch.float32)
            h16 = None if last else self._new(B, n, n, POINTS_PAD, zero=True)
            self._conv(f"l{i}", (t, 256, n, n), B, (heat, POINTS, 0), bias=True, out_f32=True, raw=None if last else (h16, POINTS_PAD, 0))
            if not last:
                branch = self._new(B, n, n, 256)
                self._conv(f"bl{i}", (t, 256, n, n), B, (branch, 256, 0), bias=True)
                nxt = self._new(B, n, n, 256)
                self._conv(f"al{i}", (h16, POINTS_PAD, n, n), B, (nxt, 256, 0), bias=True, res1=(prev[0], prev[1], 0), res2=(branch, 256, 0))
                prev = (nxt, 256, n, n)
        return heat

    # ------------------------------------------------------------------------------------------------------------------ interface
    def boxes(self, u8, boxes=None):
        """None (the whole image: (0, 0, max(H, W))), one (x0, y0, s) for every image, or a (B, 3) tensor -> (B, 3) fp32 on the device.
        One box for every image -- the default and the Evaluator's `lmd_box` -- is written on the device by three fills: a copy from
        host memory would make the host wait for the stream.  A (B, 3) tensor on the device is used where it lies; per-image boxes in
        host memory (a list, a CPU tensor) are copied, and that copy does wait."""
        B = int(u8.shape[0])
        if boxes is None:
            boxes = (0.0, 0.0, float(max(u8.shape[1], u8.shape[2])))
        if not isinstance(boxes, torch.Tensor) and len(boxes) == 3 and not any(isinstance(v, (list, tuple)) for v in boxes):
            out = torch.empty((B, 3), device=self.device, dtype=torch.float32)
            for k, v in enumerate(boxes):
                out[:, k].fill_(float(v))
            return out
        if not isinstance(boxes, torch.Tensor):
            boxes = torch.tensor(boxes, dtype=torch.float32)
        if tuple(boxes.shape) != (B, 3):
            raise ValueError(f"FanLandmarks: boxes {tuple(boxes.shape)} for a batch of {B}; (x0, y0, s) per image")
        return boxes.to(self.device, torch.float32).contiguous()

    def _heat(self, u8, boxes=None):
        if not isinstance(u8, torch.Tensor) or u8.dtype != torch.uint8 or u8.dim() != 4 or u8.shape[3] != 3 or u8.device != self.device:
            raise RuntimeError("FanLandmarks takes (B, H, W, 3) uint8 tensors on its device")
        u8, box = u8.contiguous(), self.boxes(u8, boxes)
        B, n = int(u8.shape[0]), self.side // 4
        # a chunk's photos count like its activations: the stem refuses 2 GiB of them
        largest = max(image_bytes(self.side), int(u8.shape[1]) * int(u8.shape[2]) * 3)
        per = (self.GUARD_BYTES - 1) // largest
        if per < 1:
            raise ValueError(f"FanLandmarks: one image at side {self.side} has a photo or an activation tensor of {largest} bytes, "
                             f"{self.GUARD_BYTES} or more are not served")
        if B == 0:
            return torch.empty((0, n, n, POINTS), device=self.device, dtype=torch.float32), box
        parts = [self._network(u8[lo:lo + per], box[lo:lo + per]).view(-1, n, n, POINTS) for lo in range(0, B, per)]
        return (parts[0] if len(parts) == 1 else torch.cat(parts)), box

    def heatmaps(self, u8, boxes=None):
        """(B, H, W, 3) uint8 on the device -> (B, 68, side / 4, side / 4) fp32 (a view of the channels-last buffer)"""
        return self._heat(u8, boxes)[0].permute(0, 3, 1, 2)

    def decode(self, heat, box):
        """(B, n, n, 68) fp32 contiguous heatmaps and (B, 3) boxes -> (landmarks (B, 68, 2), peaks (B, 68), nonfinite (B,) bool)"""
        from . import hip_ops as H
        lm, peak, flag = H.fan_decode(heat.reshape(-1), POINTS, box, heat.shape[0], heat.shape[1], POINTS)
        return lm, peak, flag.ne(0).any(dim=1)

    def landmarks(self, u8, boxes=None):
        """-> (landmarks (B, 68, 2) fp32 in image pixels, peak values (B, 68) fp32, nonfinite (B,) bool: a heatmap of the image held
        a NaN or an infinity), all on the device, without a host synchronisation"""
        heat, box = self._heat(u8, boxes)
        return self.decode(heat, box)


def landmarks68_json(entries):
    """{name: (68, 2) float32 array} -> the text of a landmarks68 file, floats through detect.format_f32"""
    lines = []
    for name, pts in entries.items():
        body = ", ".join(f"[{D.format_f32(x)}, {D.format_f32(y)}]" for x, y in pts)
        lines.append(f" {json.dumps(name)}: [{body}]")
    return "{\n" + ",\n".join(lines) + "\n}\n"


def add_lmd_arguments(ap):
    """the two LMD options of the metric CLIs"""
    ap.add_argument("--lmd_weights", type=str, default=None,
                    help="extension: 2D-FAN state dict (2DFAN4-11f355bf06.pth.tar layout, not shipped); adds the lmd and nme columns")
    ap.add_argument("--lmd_box", type=str, default=None,
                    help="extension, with --lmd_weights: X0,Y0,SIDE, the square of every image the landmark network sees (default: the whole image)")


def check_lmd_arguments(ap, args, metrics_on, has_gt):
    """parser errors of the LMD options -> the box or None"""
    if args.lmd_box and not args.lmd_weights:
        ap.error("--lmd_box only has a meaning with --lmd_weights")
    if args.lmd_weights and not metrics_on:
        ap.error("--lmd_weights only has a meaning with --metrics")
    if args.lmd_weights and not has_gt:
        ap.error("--lmd_weights measures against ground truth; none given")
    if args.lmd_weights and not os.path.isfile(args.lmd_weights):
        ap.error(f"--lmd_weights: no such file: {args.lmd_weights}")
    try:
        return parse_box(args.lmd_box) if args.lmd_box else None
    except ValueError as e:
        ap.error("--lmd_box: " + str(e))


def main(argv=None):
    ap = argparse.ArgumentParser(description="Find the 68 facial landmarks of aligned faces with 2D-FAN and write them as JSON")
    ap.add_argument("--faces", type=str, required=True, help="directory of aligned face images (searched recursively)")
    ap.add_argument("--weights", type=str, required=True, help="2D-FAN state dict (2DFAN4-11f355bf06.pth.tar layout, not shipped)")
    ap.add_argument("--out", type=str, required=True, help="the landmarks68 JSON to write: {name: [[x, y] x 68]} in image pixels")
    ap.add_argument("--box", type=str, default=None, help="X0,Y0,SIDE: the square of every image the network sees (default: the whole image)")
    args = ap.parse_args(argv)
    try:
        box = parse_box(args.box) if args.box else None
        from .restore_photos import _decode, list_photos
        names = list_photos(args.faces)
        if not os.path.isfile(args.weights):
            raise ValueError(f"--weights: no such file: {args.weights}")
    except (ValueError, OSError) as e:
        ap.error(str(e))
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(device)
    try:
        net = FanLandmarks(args.weights, device)
    except ValueError as e:
        ap.error(str(e))
    found = {}
    for n in names:
        lm, _, bad = net.landmarks(torch.from_numpy(_decode(os.path.join(args.faces, n))).unsqueeze(0).to(device), box)
        if bool(bad[0]):
            print(f"{n}: a heatmap is not finite, left out")
            continue
        found[n] = lm[0].cpu().numpy()
        print(f"{n}: 68 points")
    os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
    with open(args.out, "w") as f:
        f.write(landmarks68_json(found))


if __name__ == "__main__":
    main()
