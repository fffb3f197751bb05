"""Face-parsing paste masks for whole photos: facexlib's ParseNet on the device -- the host side of csrc/parse.hip.

    python -m vspbfr_amd.parse --faces DIR --weights W --out DIR [--sigma F] [--border PX]

parses every aligned square crop under DIR without any restoration and writes OUT/<relative stem>_mask.png (grey, the paste weight as
(wm 255 + 128) >> 8) and OUT/<relative stem>_parse.png (the class indices 0 .. 18).

    expected_state / check_state_dict / load   the key layout of the public checkpoint (238 entries) and the loader's rules
    fold_state                                 BatchNorm folded into the convolutions in float64
    pack_head_weight / pack_conv_weight        the weight images the kernels read (unpack_conv_weight is the inverse)
    default_taps / default_border              the integer Gaussian and the border of the paste weights at a crop size
    FaceParser                                 weights -> logits() / classes() / mask()

**No weights are shipped.  The key layout is written from the public model definition and could not be checked against a real checkpoint
file**; a file that deviates is refused by key name, never half-loaded.

The network, `ParseNet(in_size=512, out_size=512, parsing_ch=19)`: ConvLayer = [nearest x2] + ReflectionPad2d(1) + conv3x3 (stride 2 for
'down'; a bias only without a norm) + [BatchNorm2d] + [LeakyReLU(0.2)]; ResidualBlock = shortcut_func(x) + conv2(conv1(x)) with
(conv1, conv2) scales (none, down), (up, none) or (none, none).  encoder.0 3 -> 64 without activation, four down blocks 64 -> 128 -> 256
-> 256 -> 256, ten body blocks at 256 with x = feat + body(feat), four up blocks 256 -> 256 -> 256 -> 128 -> 64, out_mask_conv 64 -> 19;
out_img_conv is never computed.  It runs fully convolutionally at a crop side S, a multiple of 16 of at least 32.

Rounding points of the kernels (tests/parse_ref.py restates them): the input is (u8 / 255 - 0.5) / 0.5 in fp32; head weights and every
bias are fp32; every other weight is f16, BatchNorm folded in float64 and rounded once, here; f16 x f16 products are accumulated in fp32;
the epilogue (+ bias, LeakyReLU, + residuals read as f16) is fp32 and every stored tensor is rounded to f16 once; logits stay fp32."""
import argparse
import os
from collections import namedtuple

import numpy as np
import torch

MODEL_NAME = "ParseNet"
CLASSES = 19
BN_EPS = 1e-5                                  # torch.nn.BatchNorm2d's default, which the public definition does not change
KEEP = tuple(0 if c in (0, 14, 16, 17, 18) else 1 for c in range(CLASSES))
MAX_RADIUS = 64                                # VSP_PARSE_MAX_RADIUS
ACT_LIMIT = (1 << 31) - 128                    # bytes of one activation buffer: the entries refuse 2 GiB or more
MAX_CHUNK = 16                                 # faces per pass at most: the workspace is three buffers of the largest layer

ENCODER = ((64, 128), (128, 256), (256, 256), (256, 256))      # down blocks: encoder.1 .. 4
BODY = 10
DECODER = ((256, 256), (256, 256), (256, 128), (128, 64))      # up blocks: decoder.0 .. 3

ParseState = namedtuple("ParseState", "tensors")


def blocks():
    """[(prefix, cin, cout, scale), ...] of the 18 residual blocks in network order, scale in 'down', 'none', 'up'"""
    out = [(f"encoder.{i + 1}", ci, co, "down") for i, (ci, co) in enumerate(ENCODER)]
    out += [(f"body.{i}", 256, 256, "none") for i in range(BODY)]
    out += [(f"decoder.{i}", ci, co, "up") for i, (ci, co) in enumerate(DECODER)]
    return out


def expected_state():
    """{key: shape} of a ParseNet checkpoint: 238 entries"""
    out = {"encoder.0.conv2d.weight": (64, 3, 3, 3), "encoder.0.conv2d.bias": (64,)}
    for prefix, ci, co, scale in blocks():
        if scale != "none":
            out[f"{prefix}.shortcut_func.conv2d.weight"] = (co, ci, 3, 3)
            out[f"{prefix}.shortcut_func.conv2d.bias"] = (co,)
        for name, cin in (("conv1", ci), ("conv2", co)):
            out[f"{prefix}.{name}.conv2d.weight"] = (co, cin, 3, 3)
            for k in ("weight", "bias", "running_mean", "running_var"):
                out[f"{prefix}.{name}.norm.norm.{k}"] = (co,)
            out[f"{prefix}.{name}.norm.norm.num_batches_tracked"] = ()
    out["out_img_conv.conv2d.weight"], out["out_img_conv.conv2d.bias"] = (3, 64, 3, 3), (3,)
    out["out_mask_conv.conv2d.weight"], out["out_mask_conv.conv2d.bias"] = (CLASSES, 64, 3, 3), (CLASSES,)
    return out


def check_state_dict(sd):
    """The loader's rules -> ParseState(tensors {key: float32 CPU tensor}).  A leading `module.` is stripped and `num_batches_tracked`
    entries are ignored (present or not); any other missing or unexpected key and any wrong shape is a ValueError that names the key.
    out_img_conv's keys are checked like the others although the layer is never computed."""
    what = "ParseNet checkpoint"
    if isinstance(sd, ParseState):
        return sd
    if not isinstance(sd, dict):
        raise ValueError(f"{what}: expected a state dict, got {type(sd).__name__}")
    clean = {(k[len("module."):] if str(k).startswith("module.") else str(k)): v for k, v in sd.items()}
    clean = {k: v for k, v in clean.items() if not k.endswith(".num_batches_tracked")}
    want = {k: s for k, s in expected_state().items() if not k.endswith(".num_batches_tracked")}
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
    return ParseState(out)


def load(path):
    """torch.load + check_state_dict"""
    return check_state_dict(torch.load(path, map_location="cpu"))


def check_size(size):
    """the crop sides the network serves: multiples of 16 from 32 (the body map must be at least 2 x 2 for the reflection)"""
    if isinstance(size, bool) or int(size) != size or int(size) < 32 or int(size) % 16:
        raise ValueError(f"ParseNet: crop side {size!r}: a multiple of 16 of at least 32")
    return int(size)


# --------------------------------------------------------------------------------------------------------------------------- fold
def fold_state(state):
    """BatchNorm folded into its convolution in float64 -> {name: (weight float64 (Cout, Cin, 3, 3), bias float64 (Cout))} for `head`,
    `<block>.shortcut`, `<block>.conv1`, `<block>.conv2` and `mask`:  w' = w g / sqrt(var + eps), b' = beta - mean g / sqrt(var + eps).
    Nothing is rounded here; FaceParser rounds w' to f16 (head: fp32) and b' to fp32, once."""
    t = check_state_dict(state).tensors
    out = {"head": (t["encoder.0.conv2d.weight"].double(), t["encoder.0.conv2d.bias"].double())}
    for prefix, _, _, scale in blocks():
        if scale != "none":
            out[f"{prefix}.shortcut"] = (t[f"{prefix}.shortcut_func.conv2d.weight"].double(), t[f"{prefix}.shortcut_func.conv2d.bias"].double())
        for name in ("conv1", "conv2"):
            n = f"{prefix}.{name}.norm.norm."
            g = t[n + "weight"].double() / torch.sqrt(t[n + "running_var"].double() + BN_EPS)
            out[f"{prefix}.{name}"] = (t[f"{prefix}.{name}.conv2d.weight"].double() * g.view(-1, 1, 1, 1),
                                       t[n + "bias"].double() - t[n + "running_mean"].double() * g)
    out["mask"] = (t["out_mask_conv.conv2d.weight"].double(), t["out_mask_conv.conv2d.bias"].double())
    return out


# ------------------------------------------------------------------------------------------------------------------- weight images
def pack_head_weight(w):
    """(64, 3, 3, 3) -> (27, 64) float32, row (3 ky + kx) 3 + c: the layout of vsp_parse_head_u8"""
    w = torch.as_tensor(w)
    if tuple(w.shape) != (64, 3, 3, 3):
        raise ValueError(f"pack_head_weight: weight {tuple(w.shape)}, expected (64, 3, 3, 3)")
    return w.to(torch.float32).permute(2, 3, 1, 0).reshape(27, 64).contiguous()


def pack_conv_weight(w, nb=4):
    """(Cout, Cin, 3, 3), Cin a multiple of 64 -> the float16 image (CB, KC, 18, nb, 64, 8) that vsp_parse_conv_f16 (nb = 4, Cout a multiple
    of 64) and vsp_parse_mask_u8 (nb = 2, Cout = 19) read, CB = ceil(Cout / 16 nb), KC = Cin / 64:

        image[cb][kc][s][n][l][j] = f16(w[co = 16 nb cb + 16 n + (l & 15)][ci = 64 kc + 32 (s & 1) + 8 (l >> 4) + j][ky = (s >> 1) // 3][kx = (s >> 1) % 3])

    cb is the workgroup's block of output channels, kc the chunk of 64 input channels it stages, s the K-step of 32 inside the chunk
    (tap-major: two channel halves per tap), l the lane that reads the 16 bytes as its MFMA operand, j the element; output channels
    past Cout are zero.  Rounding to f16 (nearest even) happens here, once."""
    w = torch.as_tensor(w)
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or w.shape[0] < 1 or w.shape[1] < 64 or w.shape[1] % 64 or nb not in (2, 4):
        raise ValueError(f"pack_conv_weight: weight {tuple(w.shape)} with {nb} blocks, expected (Cout, 64 k, 3, 3)")
    cout, cin = int(w.shape[0]), int(w.shape[1])
    cb, kc = -(-cout // (16 * nb)), cin // 64
    wp = torch.zeros((cb * nb * 16, cin, 3, 3), dtype=torch.float16)
    wp[:cout] = w.to(torch.float16)
    v = wp.view(cb, nb, 16, kc, 2, 4, 8, 3, 3)               # cb, n, l & 15, kc, half, l >> 4, j, ky, kx
    return v.permute(0, 3, 7, 8, 4, 1, 5, 2, 6).reshape(cb, kc, 18, nb, 64, 8).contiguous()


def unpack_conv_weight(image, cout):
    """the inverse of pack_conv_weight -> (cout, Cin, 3, 3) float16"""
    cb, kc, _, nb = (int(v) for v in image.shape[:4])
    v = image.view(cb, kc, 3, 3, 2, nb, 4, 16, 8).permute(0, 5, 7, 1, 4, 6, 8, 2, 3)      # cb, n, l & 15, kc, half, l >> 4, j, ky, kx
    return v.reshape(cb * nb * 16, kc * 64, 3, 3)[:cout].contiguous()


# ----------------------------------------------------------------------------------------------------------------- paste weights
def taps_for(sigma, radius):
    """R + 1 int32 taps of a Gaussian of `sigma` cut at `radius`: 2^16 exp(-k^2 / 2 sigma^2) / sum over -R .. R, rounded half to even, the
    remainder to 2^16 put on the centre tap"""
    radius = int(radius)
    if not (sigma > 0) or radius < 0 or radius > MAX_RADIUS:
        raise ValueError(f"taps_for: sigma {sigma}, radius {radius} (sigma > 0, radius 0..{MAX_RADIUS})")
    k = np.arange(radius + 1, dtype=np.float64)
    e = np.exp(-k * k / (2.0 * float(sigma) ** 2))
    g = np.rint(65536.0 * e / (e[0] + 2.0 * e[1:].sum())).astype(np.int64)
    g[0] += 65536 - (g[0] + 2 * g[1:].sum())
    check_taps(g)
    return g.astype(np.int32)


def check_taps(taps):
    """what vsp_parse_blur_u16 asks of a tap table: 1 .. 65 non-negative entries with g[0] + 2 sum g[k >= 1] = 2^16"""
    g = np.asarray(taps, dtype=np.int64)
    total = int(g[0] + 2 * g[1:].sum()) if g.ndim == 1 and g.size else 0
    if g.ndim != 1 or not 1 <= g.size <= MAX_RADIUS + 1 or (g < 0).any() or total != 65536:
        raise ValueError(f"taps: {g.size} entries summing to {total}; 1..{MAX_RADIUS + 1} non-negative entries with g[0] + 2 sum g[1:] = 65536")
    return g


def default_sigma(size):
    return 11.0 * size / 512.0


def default_radius(size):
    return min(int(round(50.0 * size / 512.0)), int(size) - 1, MAX_RADIUS)


def default_taps(size, sigma=None):
    """the blur of the toolchains' paste mask (two Gaussian blurs of a 101 x 101 kernel with sigma 11 at 512) scaled to `size`:
    sigma = 11 size / 512, R = min(round(50 size / 512), size - 1)"""
    return taps_for(default_sigma(size) if sigma is None else sigma, default_radius(size))


def default_border(size):
    """the toolchains zero 10 pixels at each side of the 512^2 mask: round(10 size / 512)"""
    return int(round(10.0 * size / 512.0))


# -------------------------------------------------------------------------------------------------------------------------- network
class FaceParser:
    """state: a path, a state dict in the public layout or a checked ParseState -> the network on `device`.  There is no fallback: what
    the kernels refuse raises.  The workspace (three activation buffers of the largest layer of a chunk of faces, the body's `feat`, the
    blur's two planes) grows to the largest call seen and is kept."""

    def __init__(self, state, device, max_chunk=MAX_CHUNK):
        if isinstance(state, (str, os.PathLike)):
            state = load(state)
        folded = fold_state(state)
        dev = torch.device(device)
        w, b = folded["head"]
        self.head = (pack_head_weight(w).to(dev), b.to(torch.float32).to(dev))
        self.layers = {}
        for name, (w, b) in folded.items():
            if name not in ("head", "mask"):
                self.layers[name] = (pack_conv_weight(w).to(dev), b.to(torch.float32).to(dev))
        w, b = folded["mask"]
        bias = torch.zeros(32, dtype=torch.float32)
        bias[:CLASSES] = b.to(torch.float32)
        self.tail = (pack_conv_weight(w, nb=2).to(dev), bias.to(dev))
        self.device = self.tail[1].device
        self.max_chunk = int(max_chunk)
        self.act_limit = ACT_LIMIT
        self._act = [None, None, None]
        self._feat = None
        self._work = None
        self.launches = 0

    # ------------------------------------------------------------------------------------------------------------------ plumbing
    def _crops(self, crops_u8):
        if (not isinstance(crops_u8, torch.Tensor) or crops_u8.dtype != torch.uint8 or crops_u8.dim() != 4 or crops_u8.shape[3] != 3
                or crops_u8.shape[1] != crops_u8.shape[2] or crops_u8.device != self.device):
            raise ValueError(f"FaceParser: crops must be a (F, S, S, 3) uint8 tensor on {self.device}")
        check_size(int(crops_u8.shape[1]))
        return crops_u8.contiguous()

    def chunk_of(self, size):
        """faces per pass: the largest layer (128 channels at the full map) must stay below the 2 GiB guard"""
        per_face = size * size * 128 * 2
        if per_face > self.act_limit:
            raise ValueError(f"FaceParser: one face of side {size} needs an activation of {per_face} bytes, {self.act_limit} are served")
        return max(1, min(self.max_chunk, self.act_limit // per_face))

    def _workspace(self, n, size):
        need = n * size * size * 128
        for i in range(3):
            if self._act[i] is None or self._act[i].numel() < need:
                self._act[i] = torch.empty(need, dtype=torch.float16, device=self.device)
        nf = n * (size // 16) ** 2 * 256
        if self._feat is None or self._feat.numel() < nf:
            self._feat = torch.empty(nf, dtype=torch.float16, device=self.device)

    def _features(self, crops):
        """the decoder's last activation of one chunk: a (F, S, S, 64) float16 view of the workspace"""
        from . import hip_ops as H
        n, size = int(crops.shape[0]), int(crops.shape[1])
        self._workspace(n, size)
        x, p, q = self._act
        h = size
        c = 64
        H.parse_head_u8(x[:n * h * h * 64], crops, *self.head)
        self.launches += 1

        def conv(dst, src, hh, name, cin, cout, **kw):
            oh, ow = H.parse_conv_out(hh, hh, kw.get("stride", 1), kw.get("up", False))
            w_img, b = self.layers[name]
            kw = {k: (v[:n * oh * ow * cout] if k in ("res1", "res2") else v) for k, v in kw.items()}
            H.parse_conv_f16(dst[:n * oh * ow * cout], src[:n * hh * hh * cin], n, hh, hh, w_img, b, **kw)
            self.launches += 1
            return oh

        for prefix, ci, co, scale in blocks():
            if scale == "down":                               # conv1 at the input's resolution, conv2 and the shortcut stride 2
                conv(p, x, h, f"{prefix}.shortcut", ci, co, stride=2)
                conv(q, x, h, f"{prefix}.conv1", ci, co, act=True)
                h2 = conv(p, q, h, f"{prefix}.conv2", co, co, stride=2, res1=p)
                x, p, h = p, x, h2
            elif scale == "up":                               # conv1 and the shortcut read the nearest x2 of the input
                conv(p, x, h, f"{prefix}.shortcut", ci, co, up=True)
                conv(q, x, h, f"{prefix}.conv1", ci, co, up=True, act=True)
                h2 = conv(p, q, 2 * h, f"{prefix}.conv2", co, co, res1=p)
                x, p, h = p, x, h2
            else:
                if prefix == "body.0":
                    self._feat[:n * h * h * 256].copy_(x[:n * h * h * 256])
                conv(q, x, h, f"{prefix}.conv1", ci, co, act=True)
                last = prefix == f"body.{BODY - 1}"            # x = feat + body(feat): the last block adds feat as well
                conv(p, q, h, f"{prefix}.conv2", co, co, res1=x, **({"res2": self._feat} if last else {}))
                x, p = p, x
            c = co
        assert h == size and c == 64
        self._act = [x, p, q]
        return x[:n * size * size * 64]

    def _run(self, crops_u8, keep, want_logits):
        from . import hip_ops as H
        crops = self._crops(crops_u8)
        n, size = int(crops.shape[0]), int(crops.shape[1])
        keep = KEEP if keep is None else tuple(int(v) for v in keep)
        cls = torch.empty((n, size, size), dtype=torch.uint8, device=self.device)
        kmap = torch.empty((n, size, size), dtype=torch.uint8, device=self.device)
        info = torch.zeros(n, dtype=torch.int32, device=self.device)
        logits = torch.empty((n, size, size, CLASSES), dtype=torch.float32, device=self.device) if want_logits else None
        step = self.chunk_of(size)
        for i in range(0, n, step):
            m = min(step, n - i)
            feats = self._features(crops[i:i + m])
            H.parse_mask_u8(feats, m, size, size, *self.tail, keep=keep, info=info[i:i + m], logits=logits[i:i + m] if want_logits else False,
                            out=(cls[i:i + m], kmap[i:i + m]))                 # straight into the call's maps: no copy per chunk
            self.launches += 1
        return cls, kmap, info, logits

    # ----------------------------------------------------------------------------------------------------------------------- run
    def logits(self, crops_u8):
        """(F, S, S, 3) uint8 on the device -> the (F, S, S, 19) fp32 logits (never rounded to f16)"""
        return self._run(crops_u8, None, True)[3]

    def classes(self, crops_u8):
        """-> (F, S, S) uint8: the argmax of the logits, a tie to the lowest class, class 0 where a logit is not finite"""
        return self._run(crops_u8, None, False)[0]

    def mask(self, crops_u8, taps=None, border=None, keep=None, classes=False):
        """-> (paste weights (F, S, S) torch.uint16 in 0 .. 256, flags (F) int32 with hip_ops.PARSE_NONFINITE); classes=True adds the class
        maps.  keep: 19 values 0 / 1 (default KEEP: everything but background, neck, clothes, hair and hat); taps, border: default_taps(S),
        default_border(S)."""
        from . import hip_ops as H
        cls, kmap, info, _ = self._run(crops_u8, keep, False)
        n, size = int(kmap.shape[0]), int(kmap.shape[1])
        taps = default_taps(size) if taps is None else check_taps(taps)
        border = default_border(size) if border is None else int(border)
        if self._work is None or self._work.numel() < 2 * n * size * size:
            self._work = torch.empty(2 * n * size * size, dtype=torch.uint16, device=self.device)
        out = torch.empty((n, size, size), dtype=torch.uint16, device=self.device)
        if n:
            H.parse_blur_u16(kmap, taps, border, out=out, work=self._work)
            self.launches += 4
        return (out, info, cls) if classes else (out, info)

    def describe(self, size, taps=None, border=None, sigma=None, nonfinite=()):
        """the `parse` block of report.json"""
        taps = default_taps(size, sigma) if taps is None else taps
        return {"model": MODEL_NAME, "sigma": float(default_sigma(size) if sigma is None else sigma), "radius": int(len(taps) - 1),
                "border": int(default_border(size) if border is None else border), "nonfinite": list(nonfinite)}


def mask_png(mask_u16):
    """paste weights 0 .. 256 -> the grey bytes of <stem>_mask.png: (wm 255 + 128) >> 8"""
    m = mask_u16.view(torch.int16) if mask_u16.dtype == torch.uint16 else mask_u16      # 0 .. 256: the same bits
    return ((m.to(torch.int32) * 255 + 128) >> 8).to(torch.uint8)


def check_parse_arguments(ap, weights, size, sigma=None, border=None):
    """The checks both CLIs make before any model goes to the device -> (ParseState, taps, border); ap.error for a missing file, a
    checkpoint the loader refuses, a crop side the network does not serve, a sigma that is not positive, a border outside 0 .. size / 2."""
    try:
        check_size(size)
    except ValueError as e:
        ap.error(str(e))
    if sigma is not None and not sigma > 0:
        ap.error(f"parse sigma {sigma} must be positive")
    if border is not None and not 0 <= 2 * border <= size:
        ap.error(f"parse border {border} outside 0..{size // 2}")
    if not os.path.isfile(weights):
        ap.error(f"no such file: {weights}")
    try:
        state = load(weights)
    except ValueError as e:
        ap.error(str(e))
    return state, default_taps(size, sigma), default_border(size) if border is None else int(border)


def main(argv=None):
    ap = argparse.ArgumentParser(description="Parse aligned face crops with ParseNet on the device and write their paste masks")
    ap.add_argument("--faces", type=str, required=True, help="directory of aligned square crops (searched recursively)")
    ap.add_argument("--weights", type=str, required=True, help="ParseNet checkpoint (not shipped)")
    ap.add_argument("--out", type=str, required=True, help="output directory")
    ap.add_argument("--sigma", type=float, default=None, help="sigma of the two Gaussian blurs (default 11 S / 512; the radius is round(50 S / 512) but at most 64: above S = 655 the taps are cut below 3 sigma)")
    ap.add_argument("--border", type=int, default=None, help="rows and columns at each side that are set to 0 (default round(10 S / 512))")
    args = ap.parse_args(argv)
    from PIL import Image

    from .restore_photos import _decode, list_photos
    try:
        names = list_photos(args.faces)
    except (ValueError, OSError) as e:
        ap.error(str(e))
    crops = [_decode(os.path.join(args.faces, n)) for n in names]
    sizes = {c.shape[:2] for c in crops}
    if len(sizes) != 1 or next(iter(sizes))[0] != next(iter(sizes))[1]:
        ap.error(f"the crops must be square and of one size, got {sorted(sizes)[:4]}")
    size = next(iter(sizes))[0]
    state, taps, border = check_parse_arguments(ap, args.weights, size, args.sigma, args.border)
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(device)
    net = FaceParser(state, device)
    os.makedirs(args.out, exist_ok=True)
    step = net.chunk_of(size)
    for i in range(0, len(names), step):
        batch = torch.from_numpy(np.stack(crops[i:i + step])).to(device)
        mask, flags, cls = net.mask(batch, taps=taps, border=border, classes=True)
        grey, cls, flags = mask_png(mask).cpu().numpy(), cls.cpu().numpy(), flags.cpu().tolist()
        for k, n in enumerate(names[i:i + step]):
            stem = os.path.join(args.out, os.path.splitext(n)[0])
            os.makedirs(os.path.dirname(stem) or ".", exist_ok=True)
            Image.fromarray(grey[k]).save(stem + "_mask.png")
            Image.fromarray(cls[k]).save(stem + "_parse.png")
            print(f"{n}: mask mean {float(mask[k].view(torch.int16).float().mean()) / 256:.4f}" + (" (non-finite logits: those pixels are class 0)" if flags[k] else ""))


if __name__ == "__main__":
    main()
