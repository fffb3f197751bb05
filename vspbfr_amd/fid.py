"""FID on the device: pytorch-fid's Inception-v3 in fp32 HIP, the Frechet distance on the host.

    python -m vspbfr_amd.fid --images DIR --weights W (--stats S | --ref_images DIR) [--save_stats OUT] [--batch 16] [--out report.json]

    expected_state / check_state_dict / load   the key layout of the public checkpoint (94 x 5 entries) and the loader's rules
    fold_state                                 BatchNorm (eps 1e-3) folded into the convolutions in float64
    FidInception                               weights -> features(): (N, 2048) float32 on the device
    stats / frechet_distance                   mean and covariance, and the distance, in NumPy float64 on the host
    load_stats / save_stats                    .npz with mu / sigma, or a torch file holding a dict with those two names

**No weights and no reference statistics are shipped.  The key layout is written from the public model definition (torchvision's
Inception3 names, which pytorch-fid's `pt_inception-2015-12-05` file uses) and could not be checked against a real checkpoint file**; a
file that deviates is refused by key name, never half-loaded.

The network: u8 RGB of any size -> bilinear resize to 299 x 299 (align_corners False, NO anti-aliasing: what the published numbers use) ->
x / 127.5 - 1 -> Conv2d_1a_3x3 .. Conv2d_4a_3x3 with two max pools -> Mixed_5b/5c/5d (InceptionA) -> Mixed_6a (B) -> Mixed_6b..6e (C) ->
Mixed_7a (D) -> Mixed_7b/7c (E) -> global average.  Every convolution is conv (no bias) + BatchNorm + ReLU.  Against torchvision's
network: the 3x3 average pools of A, C and Mixed_7b divide by the number of in-bounds taps, Mixed_7c's pool branch is a MAX pool, and
there is no fc, no aux head and no transform_input.

Everything on the device is fp32: weights and biases are folded in float64 and rounded once, the products run on the fp32-input MFMA
(an fmaf chain per output), and the epilogue is fp32."""
import argparse
import json
import os
from collections import namedtuple

import numpy as np
import torch

MODEL_NAME = "FID Inception-v3"
DIMS = 2048
BN_EPS = 1e-3
SIZE = 299
ACT_LIMIT = (1 << 31) - 4096                  # bytes of one activation tensor: the entries refuse 2 GiB or more
MAX_CHUNK = 64                                # images per pass at most
IGNORED_PREFIXES = ("fc.", "AuxLogits.")

FidState = namedtuple("FidState", "tensors")
Conv = namedtuple("Conv", "name cin cout kh kw stride ph pw")


def _c(name, cin, cout, k=1, stride=1, pad=0):
    kh, kw = (k, k) if isinstance(k, int) else k
    ph, pw = (pad, pad) if isinstance(pad, int) else pad
    return Conv(name, cin, cout, kh, kw, stride, ph, pw)


def _block_a(p, cin, pf):
    return [_c(p + ".branch1x1", cin, 64), _c(p + ".branch5x5_1", cin, 48), _c(p + ".branch5x5_2", 48, 64, 5, pad=2),
            _c(p + ".branch3x3dbl_1", cin, 64), _c(p + ".branch3x3dbl_2", 64, 96, 3, pad=1), _c(p + ".branch3x3dbl_3", 96, 96, 3, pad=1),
            _c(p + ".branch_pool", cin, pf)]


def _block_b(p, cin):
    return [_c(p + ".branch3x3", cin, 384, 3, stride=2), _c(p + ".branch3x3dbl_1", cin, 64), _c(p + ".branch3x3dbl_2", 64, 96, 3, pad=1),
            _c(p + ".branch3x3dbl_3", 96, 96, 3, stride=2)]


def _block_c(p, cin, c7):
    r, c = ((1, 7), (0, 3)), ((7, 1), (3, 0))
    return [_c(p + ".branch1x1", cin, 192), _c(p + ".branch7x7_1", cin, c7), _c(p + ".branch7x7_2", c7, c7, r[0], pad=r[1]),
            _c(p + ".branch7x7_3", c7, 192, c[0], pad=c[1]), _c(p + ".branch7x7dbl_1", cin, c7),
            _c(p + ".branch7x7dbl_2", c7, c7, c[0], pad=c[1]), _c(p + ".branch7x7dbl_3", c7, c7, r[0], pad=r[1]),
            _c(p + ".branch7x7dbl_4", c7, c7, c[0], pad=c[1]), _c(p + ".branch7x7dbl_5", c7, 192, r[0], pad=r[1]),
            _c(p + ".branch_pool", cin, 192)]


def _block_d(p, cin):
    return [_c(p + ".branch3x3_1", cin, 192), _c(p + ".branch3x3_2", 192, 320, 3, stride=2), _c(p + ".branch7x7x3_1", cin, 192),
            _c(p + ".branch7x7x3_2", 192, 192, (1, 7), pad=(0, 3)), _c(p + ".branch7x7x3_3", 192, 192, (7, 1), pad=(3, 0)),
            _c(p + ".branch7x7x3_4", 192, 192, 3, stride=2)]


def _block_e(p, cin):
    return [_c(p + ".branch1x1", cin, 320), _c(p + ".branch3x3_1", cin, 384), _c(p + ".branch3x3_2a", 384, 384, (1, 3), pad=(0, 1)),
            _c(p + ".branch3x3_2b", 384, 384, (3, 1), pad=(1, 0)), _c(p + ".branch3x3dbl_1", cin, 448),
            _c(p + ".branch3x3dbl_2", 448, 384, 3, pad=1), _c(p + ".branch3x3dbl_3a", 384, 384, (1, 3), pad=(0, 1)),
            _c(p + ".branch3x3dbl_3b", 384, 384, (3, 1), pad=(1, 0)), _c(p + ".branch_pool", cin, 192)]


BLOCKS = (("Mixed_5b", "A", 192, 32), ("Mixed_5c", "A", 256, 64), ("Mixed_5d", "A", 288, 64), ("Mixed_6a", "B", 288, None),
          ("Mixed_6b", "C", 768, 128), ("Mixed_6c", "C", 768, 160), ("Mixed_6d", "C", 768, 160), ("Mixed_6e", "C", 768, 192),
          ("Mixed_7a", "D", 768, None), ("Mixed_7b", "E", 1280, "avg"), ("Mixed_7c", "E", 2048, "max"))
BLOCK_OUT = {"Mixed_5b": 256, "Mixed_5c": 288, "Mixed_5d": 288, "Mixed_6a": 768, "Mixed_6b": 768, "Mixed_6c": 768, "Mixed_6d": 768,
             "Mixed_6e": 768, "Mixed_7a": 1280, "Mixed_7b": 2048, "Mixed_7c": 2048}


def convs():
    """the 94 convolutions in network order as Conv(name, cin, cout, kh, kw, stride, ph, pw)"""
    out = [_c("Conv2d_1a_3x3", 3, 32, 3, stride=2), _c("Conv2d_2a_3x3", 32, 32, 3), _c("Conv2d_2b_3x3", 32, 64, 3, pad=1),
           _c("Conv2d_3b_1x1", 64, 80), _c("Conv2d_4a_3x3", 80, 192, 3)]
    for name, kind, cin, arg in BLOCKS:
        out += {"A": lambda: _block_a(name, cin, arg), "B": lambda: _block_b(name, cin), "C": lambda: _block_c(name, cin, arg),
                "D": lambda: _block_d(name, cin), "E": lambda: _block_e(name, cin)}[kind]()
    return out


def expected_state():
    """{key: shape} of the entries the loader asks for: 94 x 5"""
    out = {}
    for c in convs():
        out[c.name + ".conv.weight"] = (c.cout, c.cin, c.kh, c.kw)
        for k in ("weight", "bias", "running_mean", "running_var"):
            out[f"{c.name}.bn.{k}"] = (c.cout,)
    return out


def check_state_dict(sd):
    """The loader's rules -> FidState(tensors {key: float32 CPU tensor}).  A leading `module.` is stripped; `num_batches_tracked`, `fc.*`
    and `AuxLogits.*` entries are ignored (present or not); any other missing or unexpected key and any wrong shape is a ValueError that
    names the key."""
    what = "FID Inception checkpoint"
    if isinstance(sd, FidState):
        return sd
    if not isinstance(sd, dict):
        raise ValueError(f"{what}: expected a state dict, got {type(sd).__name__}")
    clean = {(k[len("module."):] if str(k).startswith("module.") else str(k)): v for k, v in sd.items()}
    clean = {k: v for k, v in clean.items() if not k.endswith(".num_batches_tracked") and not k.startswith(IGNORED_PREFIXES)}
    want = expected_state()
    missing, extra = sorted(set(want) - set(clean)), sorted(set(clean) - set(want))
    if missing or extra:
        raise ValueError(f"{what}: " + "; ".join(f"{name} {', '.join(ks[:8])}{' ...' if len(ks) > 8 else ''}"
                                                 for name, ks in (("missing keys", missing), ("unexpected keys", extra)) if ks))
    out = {}
    for k, shape in want.items():
        t = torch.as_tensor(clean[k]).detach().to("cpu", torch.float32)
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{what}: {k} has shape {tuple(t.shape)}, expected {tuple(shape)}")
        out[k] = t.contiguous()
    return FidState(out)


def load(path):
    """torch.load + check_state_dict"""
    return check_state_dict(torch.load(path, map_location="cpu"))


def fold_state(state):
    """BatchNorm folded into its convolution in float64 -> {layer name: (weight float64 (Cout, Cin, KH, KW), bias float64 (Cout))}:
    w' = w g / sqrt(var + eps), b' = beta - mean g / sqrt(var + eps), eps = 1e-3.  Nothing is rounded here; FidInception rounds to fp32,
    once."""
    t = check_state_dict(state).tensors
    out = {}
    for c in convs():
        n = c.name + ".bn."
        g = t[n + "weight"].double() / torch.sqrt(t[n + "running_var"].double() + BN_EPS)
        out[c.name] = (t[c.name + ".conv.weight"].double() * g.view(-1, 1, 1, 1), t[n + "bias"].double() - t[n + "running_mean"].double() * g)
    return out


def pack_weight(w):
    """(Cout, Cin, KH, KW) -> (KH, KW, Cin, Cout) float32: the layout of vsp_fid_conv_f32; the stem's (32, 3, 3, 3) becomes (27, 32)"""
    return torch.as_tensor(w).permute(2, 3, 1, 0).to(torch.float32).contiguous()


# ------------------------------------------------------------------------------------------------------------------------ the plan
class _Plan:
    """The launches of one pass over images whose first layer sees (H0, W0): a list of ("conv", layer, src, dst, H, W) and
    ("pool", mode, src, dst, H, W, C) with src / dst = (buffer name, channel offset, pitch), and the floats each buffer needs per image.
    Buffers: x / y hold the block inputs and outputs in turn, t1 / t2 the intermediates of a branch, feat the (B, 2048) result."""

    def __init__(self, H0, W0):
        from .hip_ops import FID_POOL_AVG_S1, FID_POOL_GLOBAL_AVG, FID_POOL_MAX_S1, FID_POOL_MAX_S2
        self.specs = {c.name: c for c in convs()}
        self.ops, self.need, self.maps = [], {}, []
        if H0 < 3 or W0 < 3:
            raise ValueError(f"FID Inception: a {H0} x {W0} input is too small")
        H, W = (H0 - 3) // 2 + 1, (W0 - 3) // 2 + 1
        self.stem = (H, W)
        self._use(("x", 0, 32), H, W)
        self.maps.append((H, W))
        for step in (lambda: self.conv("Conv2d_2a_3x3", ("x", 0, 32), ("y", 0, 32), H, W),
                     lambda: self.conv("Conv2d_2b_3x3", ("y", 0, 32), ("x", 0, 64), H, W),
                     lambda: self.pool(FID_POOL_MAX_S2, ("x", 0, 64), ("y", 0, 64), H, W, 64),
                     lambda: self.conv("Conv2d_3b_1x1", ("y", 0, 64), ("x", 0, 80), H, W),
                     lambda: self.conv("Conv2d_4a_3x3", ("x", 0, 80), ("y", 0, 192), H, W),
                     lambda: self.pool(FID_POOL_MAX_S2, ("y", 0, 192), ("x", 0, 192), H, W, 192)):
            H, W = step()
            self.maps.append((H, W))
        cur, oth = "x", "y"
        for name, kind, cin, arg in BLOCKS:
            co = BLOCK_OUT[name]
            s, d = (lambda off, c=cin: (cur, off, c)), (lambda off, c=co: (oth, off, c))
            t1, t2 = (lambda c: ("t1", 0, c)), (lambda c: ("t2", 0, c))
            if kind == "A":
                self.conv(name + ".branch1x1", s(0), d(0), H, W)
                self.conv(name + ".branch5x5_1", s(0), t1(48), H, W)
                self.conv(name + ".branch5x5_2", t1(48), d(64), H, W)
                self.conv(name + ".branch3x3dbl_1", s(0), t1(64), H, W)
                self.conv(name + ".branch3x3dbl_2", t1(64), t2(96), H, W)
                self.conv(name + ".branch3x3dbl_3", t2(96), d(128), H, W)
                self.pool(FID_POOL_AVG_S1, s(0), t1(cin), H, W, cin)
                self.conv(name + ".branch_pool", t1(cin), d(224), H, W)
                nH, nW = H, W
            elif kind == "B":
                nH, nW = self.conv(name + ".branch3x3", s(0), d(0), H, W)
                self.conv(name + ".branch3x3dbl_1", s(0), t1(64), H, W)
                self.conv(name + ".branch3x3dbl_2", t1(64), t2(96), H, W)
                self.conv(name + ".branch3x3dbl_3", t2(96), d(384), H, W)
                self.pool(FID_POOL_MAX_S2, s(0), d(480), H, W, cin)
            elif kind == "C":
                c7 = arg
                self.conv(name + ".branch1x1", s(0), d(0), H, W)
                self.conv(name + ".branch7x7_1", s(0), t1(c7), H, W)
                self.conv(name + ".branch7x7_2", t1(c7), t2(c7), H, W)
                self.conv(name + ".branch7x7_3", t2(c7), d(192), H, W)
                self.conv(name + ".branch7x7dbl_1", s(0), t1(c7), H, W)
                self.conv(name + ".branch7x7dbl_2", t1(c7), t2(c7), H, W)
                self.conv(name + ".branch7x7dbl_3", t2(c7), t1(c7), H, W)
                self.conv(name + ".branch7x7dbl_4", t1(c7), t2(c7), H, W)
                self.conv(name + ".branch7x7dbl_5", t2(c7), d(384), H, W)
                self.pool(FID_POOL_AVG_S1, s(0), t1(cin), H, W, cin)
                self.conv(name + ".branch_pool", t1(cin), d(576), H, W)
                nH, nW = H, W
            elif kind == "D":
                self.conv(name + ".branch3x3_1", s(0), t1(192), H, W)
                nH, nW = self.conv(name + ".branch3x3_2", t1(192), d(0), H, W)
                self.conv(name + ".branch7x7x3_1", s(0), t1(192), H, W)
                self.conv(name + ".branch7x7x3_2", t1(192), t2(192), H, W)
                self.conv(name + ".branch7x7x3_3", t2(192), t1(192), H, W)
                self.conv(name + ".branch7x7x3_4", t1(192), d(320), H, W)
                self.pool(FID_POOL_MAX_S2, s(0), d(512), H, W, cin)
            else:
                self.conv(name + ".branch1x1", s(0), d(0), H, W)
                self.conv(name + ".branch3x3_1", s(0), t1(384), H, W)
                self.conv(name + ".branch3x3_2a", t1(384), d(320), H, W)
                self.conv(name + ".branch3x3_2b", t1(384), d(704), H, W)
                self.conv(name + ".branch3x3dbl_1", s(0), t1(448), H, W)
                self.conv(name + ".branch3x3dbl_2", t1(448), t2(384), H, W)
                self.conv(name + ".branch3x3dbl_3a", t2(384), d(1088), H, W)
                self.conv(name + ".branch3x3dbl_3b", t2(384), d(1472), H, W)
                self.pool(FID_POOL_AVG_S1 if arg == "avg" else FID_POOL_MAX_S1, s(0), t1(cin), H, W, cin)
                self.conv(name + ".branch_pool", t1(cin), d(1856), H, W)
                nH, nW = H, W
            if (nH, nW) != (H, W):
                self.maps.append((nH, nW))
            H, W, cur, oth = nH, nW, oth, cur
        self.pool(FID_POOL_GLOBAL_AVG, (cur, 0, DIMS), ("feat", 0, DIMS), H, W, DIMS)
        self.per_image = max(v for k, v in self.need.items() if k != "feat")

    def _use(self, t, H, W):
        if H < 1 or W < 1:
            raise ValueError("FID Inception: the input is too small, a map of the chain is empty (75 x 75 is the smallest input)")
        self.need[t[0]] = max(self.need.get(t[0], 0), H * W * t[2])

    def conv(self, name, src, dst, H, W):
        from .hip_ops import fid_conv_out
        c = self.specs[name]
        oh, ow = fid_conv_out(H, W, c.kh, c.kw, c.ph, c.pw, c.stride)
        self._use(src, H, W), self._use(dst, oh, ow)
        self.ops.append(("conv", name, src, dst, H, W))
        return oh, ow

    def pool(self, mode, src, dst, H, W, C):
        from .hip_ops import fid_pool_out
        oh, ow = fid_pool_out(H, W, mode)
        self._use(src, H, W), self._use(dst, oh, ow)
        self.ops.append(("pool", mode, src, dst, H, W, C))
        return oh, ow


def map_chain(H0, W0=None):
    """the sizes of the maps from the stem's output on, one entry per change of size: 299 -> 149, 147, 147, 73, 73, 71, 35, 17, 8"""
    return [m if W0 is not None else m[0] for m in _Plan(H0, H0 if W0 is None else W0).maps]


class FidInception:
    """The FID Inception on one device.

        net = FidInception(fid.load(path), "cuda")
        f = net.features(images_u8)                       # (N, H, W, 3) uint8 on the device, or a list of (h, w, 3) uint8 tensors / arrays
        f = net.features(device_photos=(buffer, offsets, sizes))      # a flat uint8 device buffer, byte offsets, [(h, w), ...]

    -> (N, 2048) float32 on the device, without a host synchronisation.  The batch is cut into chunks so that the largest activation
    stays below 2 GiB (and below `chunk` images); the workspace is kept between calls.  Image i has the same bits at any batch size
    and position.  resize=False feeds the images to Conv2d_1a as they are (all of one size, 75 x 75 at least): for tests."""

    def __init__(self, state, device="cuda", chunk=MAX_CHUNK):
        self.device = torch.device(device)
        folded = fold_state(state)
        self.weights = {}
        for c in convs():
            w, b = folded[c.name]
            wp = pack_weight(w)
            if c.name == "Conv2d_1a_3x3":
                wp = wp.reshape(27, 32)
            self.weights[c.name] = (wp.to(self.device), b.to(torch.float32).contiguous().to(self.device))
        self.device = self.weights["Conv2d_1a_3x3"][0].device      # with its index
        self.chunk = int(chunk)
        if self.chunk < 1:
            raise ValueError(f"FidInception: chunk {chunk}")
        self._plans, self._work = {}, {}

    def _plan(self, H0, W0):
        key = (int(H0), int(W0))
        if key not in self._plans:
            self._plans[key] = _Plan(*key)
        return self._plans[key]

    def chunk_for(self, plan):
        """images per pass: the largest activation of the plan stays below the 2 GiB guard"""
        return max(1, min(self.chunk, ACT_LIMIT // (4 * plan.per_image)))

    def _buffers(self, plan, n):
        out = {}
        for name, per in plan.need.items():
            if name == "feat":
                continue
            have = self._work.get(name)
            if have is None or have.numel() < n * per:
                have = self._work[name] = torch.empty(n * per, dtype=torch.float32, device=self.device)
            out[name] = have
        return out

    def _sources(self, images, device_photos):
        """-> (flat uint8 device buffer, [offset], [(h, w)])"""
        if (images is None) == (device_photos is None):
            raise ValueError("FidInception.features: give images or device_photos")
        if device_photos is not None:
            buffer, offsets, sizes = device_photos
            if not isinstance(buffer, torch.Tensor) or buffer.dtype != torch.uint8 or buffer.dim() != 1 or not buffer.is_contiguous() \
                    or buffer.device != self.device:
                raise ValueError(f"FidInception.features: device_photos takes a flat contiguous uint8 tensor on {self.device}")
            offsets, sizes = [int(o) for o in offsets], [(int(h), int(w)) for h, w in sizes]
            if len(offsets) != len(sizes):
                raise ValueError("FidInception.features: device_photos needs one offset per size")
            return buffer, offsets, sizes
        if isinstance(images, torch.Tensor):
            if images.dtype != torch.uint8 or images.dim() != 4 or images.shape[3] != 3:
                raise ValueError(f"FidInception.features: images must be (N, H, W, 3) uint8 (got {images.dtype} {tuple(images.shape)})")
            t = images.to(self.device).contiguous()
            n, h, w = (int(v) for v in t.shape[:3])
            return t.view(-1), [i * h * w * 3 for i in range(n)], [(h, w)] * n
        parts, offsets, sizes, at = [], [], [], 0
        for im in images:
            t = im if isinstance(im, torch.Tensor) else torch.from_numpy(np.array(im))           # a copy: Pillow's arrays are read-only
            if t.dtype != torch.uint8 or t.dim() != 3 or t.shape[2] != 3:
                raise ValueError(f"FidInception.features: an image must be (h, w, 3) uint8 (got {t.dtype} {tuple(t.shape)})")
            parts.append(t.contiguous().view(-1))
            offsets.append(at)
            sizes.append((int(t.shape[0]), int(t.shape[1])))
            at += parts[-1].numel()
        buffer = torch.cat(parts).to(self.device) if parts else torch.empty(0, dtype=torch.uint8, device=self.device)
        return buffer, offsets, sizes

    def features(self, images=None, device_photos=None, resize=True, chunk=None):
        from . import _lib
        from . import hip_ops as H
        buffer, offsets, sizes = self._sources(images, device_photos)
        n = len(sizes)
        out = torch.empty((n, DIMS), dtype=torch.float32, device=self.device)
        if n == 0:
            return out
        if any(h < 1 or w < 1 for h, w in sizes):
            raise ValueError("FidInception.features: an empty image")
        if resize:
            th, tw = SIZE, SIZE
        else:
            if len(set(sizes)) != 1:
                raise ValueError("FidInception.features: resize=False takes images of one size")
            th, tw = sizes[0]
        plan = self._plan(th, tw)
        step = self.chunk_for(plan) if chunk is None else max(1, min(int(chunk), self.chunk_for(plan)))
        for at in range(0, n, step):
            m = min(step, n - at)
            bufs = self._buffers(plan, m)
            bufs["feat"] = out[at:at + m]
            items = (_lib.DetSrc * m)()
            for i in range(m):
                items[i].off, items[i].h, items[i].w, items[i].slot = offsets[at + i], sizes[at + i][0], sizes[at + i][1], i
            items_dev = torch.frombuffer(bytearray(bytes(items)), dtype=torch.uint8).to(self.device)
            w, b = self.weights["Conv2d_1a_3x3"]
            sh, sw = plan.stem
            H.fid_stem_u8(bufs["x"][:m * sh * sw * 32], buffer, items, items_dev, m, m, th, tw, w, b)
            for op in plan.ops:
                self.launch(plan, op, bufs, m)
        return out

    def launch(self, plan, op, bufs, m):
        """one launch of a plan on m images: bufs maps the plan's buffer names to float32 tensors"""
        from . import hip_ops as H
        if op[0] == "conv":
            _, name, src, dst, hh, ww = op
            c = plan.specs[name]
            w, b = self.weights[name]
            H.fid_conv_f32((bufs[dst[0]], dst[1], dst[2]), (bufs[src[0]], src[1], src[2]), w, b, m, hh, ww, c.stride, (c.ph, c.pw))
        else:
            _, mode, src, dst, hh, ww, ch = op
            H.fid_pool_f32((bufs[dst[0]], dst[1], dst[2]), (bufs[src[0]], src[1], src[2]), m, hh, ww, ch, mode)


# ------------------------------------------------------------------------------------------------- statistics and distance (host)
def stats(features):
    """(N, D) features -> (mu (D,), sigma (D, D)) in float64 on the host: the mean and np.cov(rowvar=False) (divisor N - 1)"""
    f = features.detach().cpu().numpy() if isinstance(features, torch.Tensor) else np.asarray(features)
    f = f.astype(np.float64)
    if f.ndim != 2 or f.shape[0] < 2:
        raise ValueError(f"fid.stats: features {f.shape}: (N, D) with N of at least 2")
    if not np.isfinite(f).all():
        raise ValueError("fid.stats: a feature is not finite")
    return f.mean(axis=0), np.atleast_2d(np.cov(f, rowvar=False))


def _check_stats(mu, sigma, what):
    mu, sigma = np.asarray(mu, dtype=np.float64), np.asarray(sigma, dtype=np.float64)
    if mu.ndim != 1 or sigma.shape != (mu.shape[0], mu.shape[0]):
        raise ValueError(f"{what}: mu {mu.shape} and sigma {sigma.shape}: expected (D,) and (D, D)")
    if not (np.isfinite(mu).all() and np.isfinite(sigma).all()):
        raise ValueError(f"{what}: a value is not finite")
    return mu, sigma


def frechet_distance(mu1, sigma1, mu2, sigma2, eps=1e-6):
    """|mu1 - mu2|^2 + tr sigma1 + tr sigma2 - 2 tr sqrtm(sigma1 sigma2) in float64.  When the root of the product is not finite, eps I
    is added to both covariances; an imaginary part below 1e-3 (relative, on the diagonal) is dropped, a larger one is a ValueError."""
    from scipy import linalg
    mu1, sigma1 = _check_stats(mu1, sigma1, "frechet_distance: first")
    mu2, sigma2 = _check_stats(mu2, sigma2, "frechet_distance: second")
    if mu1.shape != mu2.shape:
        raise ValueError(f"frechet_distance: dimensions {mu1.shape[0]} and {mu2.shape[0]}")
    diff = mu1 - mu2
    root = linalg.sqrtm(sigma1.dot(sigma2))
    if isinstance(root, tuple):
        root = root[0]
    if not np.isfinite(root).all():
        off = np.eye(sigma1.shape[0]) * eps
        root = linalg.sqrtm((sigma1 + off).dot(sigma2 + off))
        if isinstance(root, tuple):
            root = root[0]
    if np.iscomplexobj(root):
        d = np.diagonal(root)
        if not np.allclose(d.imag, 0, atol=1e-3 * max(1.0, float(np.abs(d.real).max()))):
            raise ValueError(f"frechet_distance: imaginary component {float(np.max(np.abs(root.imag)))} in the root of the product")
        root = root.real
    return float(diff.dot(diff) + np.trace(sigma1) + np.trace(sigma2) - 2.0 * np.trace(root))


def save_stats(path, mu, sigma):
    """.npz with mu / sigma, or (any other suffix) a torch file holding {"mu", "sigma"}"""
    mu, sigma = _check_stats(mu, sigma, "fid.save_stats")
    if str(path).endswith(".npz"):
        with open(path, "wb") as f:
            np.savez(f, mu=mu, sigma=sigma)
    else:
        torch.save({"mu": torch.from_numpy(mu.copy()), "sigma": torch.from_numpy(sigma.copy())}, path)


def load_stats(path, dims=DIMS):
    """-> (mu, sigma) float64 from an .npz with mu / sigma or a torch file holding a dict with those two names (the layout of the widely
    used inception_FFHQ_512.pth); shapes are checked against `dims` (None: any)"""
    if str(path).endswith(".npz"):
        with np.load(path) as z:
            if "mu" not in z.files or "sigma" not in z.files:
                raise ValueError(f"{path}: an .npz with mu and sigma is expected (it holds {sorted(z.files)})")
            mu, sigma = z["mu"], z["sigma"]
    else:
        # the public files hold NumPy arrays: allow exactly what an ndarray of floats unpickles through, nothing else
        ma = (getattr(np, "_core", None) or np.core).multiarray
        allowed = [ma._reconstruct, np.ndarray, np.dtype] + [type(np.dtype(t)) for t in (np.float32, np.float64)]
        with torch.serialization.safe_globals(allowed):
            d = torch.load(path, map_location="cpu", weights_only=True)
        if not isinstance(d, dict) or "mu" not in d or "sigma" not in d:
            raise ValueError(f"{path}: a dict with mu and sigma is expected")
        mu, sigma = (v.detach().cpu().numpy() if isinstance(v, torch.Tensor) else np.asarray(v) for v in (d["mu"], d["sigma"]))
    mu, sigma = _check_stats(mu, sigma, str(path))
    if dims is not None and mu.shape[0] != dims:
        raise ValueError(f"{path}: statistics of dimension {mu.shape[0]}, expected {dims}")
    return mu, sigma


# ------------------------------------------------------------------------------------------------------------------------------ CLI
IMAGE_SUFFIXES = (".png", ".jpg", ".jpeg", ".bmp")


def list_images(root):
    out = []
    for dp, _, fs in sorted(os.walk(root)):
        out += [os.path.join(dp, f) for f in sorted(fs) if f.lower().endswith(IMAGE_SUFFIXES)]
    if not out:
        raise ValueError(f"no images under {root}")
    return out


def features_of_files(net, paths, batch=16):
    """features of image files, read on the host with Pillow, `batch` at a time"""
    from PIL import Image
    out = []
    for at in range(0, len(paths), batch):
        out.append(net.features([np.asarray(Image.open(p).convert("RGB")) for p in paths[at:at + batch]]))
    return torch.cat(out)


def parse_args(argv=None):
    ap = argparse.ArgumentParser(prog="python -m vspbfr_amd.fid", description="FID of a directory of images against statistics or another directory")
    ap.add_argument("--images", required=True)
    ap.add_argument("--weights", required=True)
    ap.add_argument("--stats")
    ap.add_argument("--ref_images")
    ap.add_argument("--save_stats")
    ap.add_argument("--batch", type=int, default=16)
    ap.add_argument("--out")
    ap.add_argument("--device", default="cuda")
    args = ap.parse_args(argv)
    if (args.stats is None) == (args.ref_images is None):
        ap.error("give exactly one of --stats and --ref_images")
    if args.batch < 1:
        ap.error("--batch must be at least 1")
    return args


def main(argv=None):
    args = parse_args(argv)
    net = FidInception(load(args.weights), args.device)
    paths = list_images(args.images)
    mu, sigma = stats(features_of_files(net, paths, args.batch))
    if args.save_stats:
        save_stats(args.save_stats, mu, sigma)
    if args.stats:
        rmu, rsigma = load_stats(args.stats)
    else:
        rmu, rsigma = stats(features_of_files(net, list_images(args.ref_images), args.batch))
    report = {"fid": frechet_distance(mu, sigma, rmu, rsigma), "count": len(paths), "against": "stats" if args.stats else "images",
              "ref": args.stats or args.ref_images}
    print("fid %.6f (%d images against %s)" % (report["fid"], report["count"], report["ref"]))
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1, allow_nan=False)
            f.write("\n")
    return report


if __name__ == "__main__":
    main()
