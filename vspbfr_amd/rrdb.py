"""Background upscaling with Real-ESRGAN's RRDBNet: RealESRGAN_x4plus, RealESRGAN_x2plus and the 6-block anime model on the
device -- the host side of csrc/rrdb.hip.  Both CLIs (vspbfr_amd.upscale, vspbfr_amd.restore_photos --bg_weights) reach it through the
keys of the checkpoint they are given: a file with `conv_first.weight` is an RRDBNet, anything else goes the way of DESIGN 23.

    expected_state / check_state_dict / load     the key layout of the public checkpoints (x4plus: 702 entries) and the loader's rules
    pack_head_weight / pack_conv_weight          the weight images the kernels read (unpack_* are the inverses)
    net_halo / TAIL_HALO                         the halos of the trunk's row bands and of the bands of the 4x maps
    RrdbUpscaler                                 weights -> upscale() / upscale_to() / describe(), the interface of upscale.SrUpscaler

**No weights are shipped.  The key layout is written from the public model definition and could not be checked against a real checkpoint
file**; a file that deviates is refused by key name, never half-loaded.

The network (num_feat 64, num_grow_ch 32, nb blocks; every convolution 3x3, zero padding 1, with bias; lrelu = LeakyReLU(0.2)):

    x = u8 / 255; x2plus: reflect-pad right / bottom to even sides, pixel_unshuffle(2) (channel 4 c + 2 dy + dx)
    feat = conv_first(x)
    RRDB (nb times), input f:  three dense blocks d -> 0.2 conv5(cat d, x1 .. x4) + d with xk = lrelu(convk(cat d, x1 .. x(k-1)));
                               f <- 0.2 (third block's output) + f
    f = feat + conv_body(f); f = lrelu(conv_up1(nearest x2 of f)); f = lrelu(conv_up2(nearest x2 of f)); out = conv_last(lrelu(conv_hr(f)))
    x2plus: crop to (2 h, 2 w)

Rounding points of the kernels (tests/rrdb_ref.py restates them): the input and conv_first's weights are fp32, every bias is fp32; all
other weights are rounded to f16 once, here; products of f16 operands are accumulated in fp32; the epilogue is fp32 (v = acc + b, lrelu,
v = fmaf(s1, v, r1), v = fmaf(s2, v, r2)) and every activation is rounded to f16 once behind it -- the third dense block's conv5 applies
both residuals before its one rounding; the output is clamped to [0, 1] and written as rintf(255 v); a non-finite value is written as 0
and sets hip_ops.RRDB_NONFINITE.

Memory of a unit of n network-input pixels: three 192-channel dense tensors that rotate (a dense block reads one and writes the next;
the block's input f stays in the third until the block's last convolution has used it), feat, conv_body's output and the 2x map --
3 x 384 + 128 + 128 + 512 = 1 920 B per pixel.  The 4x maps (2 x 16 n x 128 B) are never held whole: conv_up2 -> conv_hr -> conv_last run
in row bands of their own over the finished 2x map (halo TAIL_HALO rows of it), so the trunk never runs again because of them."""
import os
from collections import namedtuple

import numpy as np
import torch

from .upscale import ACT_LIMIT, SrUpscaler, plan_bands

FEATURES, GROWTH = 64, 32
MODEL_NAME = "RRDBNet"
TAIL_HALO = 2                                # rows of the 2x map on each inner side of a band of conv_up2 -> conv_hr -> conv_last

RrdbState = namedtuple("RrdbState", "tensors num_block scale")


def conv_names(num_block):
    """the 15 nb + 6 convolutions in network order"""
    return (["conv_first"] + [f"body.{i}.rdb{j}.conv{k}" for i in range(num_block) for j in (1, 2, 3) for k in (1, 2, 3, 4, 5)]
            + ["conv_body", "conv_up1", "conv_up2", "conv_hr", "conv_last"])


def conv_shape(name, scale):
    """(Cout, Cin) of a convolution by name"""
    if name == "conv_first":
        return FEATURES, 3 if scale == 4 else 12
    if name == "conv_last":
        return 3, FEATURES
    if name.startswith("body."):
        k = int(name[-1])
        return (GROWTH if k < 5 else FEATURES), FEATURES + (k - 1) * GROWTH
    return FEATURES, FEATURES


def expected_state(num_block=23, scale=4):
    """{key: shape} of an RRDBNet checkpoint with 64 features and growth 32: 15 nb + 6 convolutions, 30 nb + 12 entries"""
    out = {}
    for name in conv_names(num_block):
        cout, cin = conv_shape(name, scale)
        out[name + ".weight"] = (cout, cin, 3, 3)
        out[name + ".bias"] = (cout,)
    return out


def check_state_dict(sd):
    """The loader's rules -> RrdbState(tensors {key: float32 CPU tensor}, num_block, scale).  A `params_ema` or `params` wrapper is opened
    and a leading `module.` stripped; num_block comes from the `body.N.` keys, the scale from conv_first's Cin (3 -> x4, 12 -> x2).  Any
    missing or unexpected key, any wrong shape, a feature count other than 64, a growth other than 32 and num_block < 1 is a ValueError
    that names the key."""
    what = "RRDBNet checkpoint"
    if isinstance(sd, RrdbState):
        return sd
    if not isinstance(sd, dict):
        raise ValueError(f"{what}: expected a state dict, got {type(sd).__name__}")
    for wrapper in ("params_ema", "params"):
        if wrapper in sd and isinstance(sd[wrapper], dict):
            sd = sd[wrapper]
            break
    clean = {(k[len("module."):] if str(k).startswith("module.") else str(k)): v for k, v in sd.items()}
    if "conv_first.weight" not in clean:
        raise ValueError(f"{what}: no conv_first.weight key (keys: {', '.join(sorted(clean)[:4])} ...)")
    first = torch.as_tensor(clean["conv_first.weight"])
    if first.dim() != 4 or tuple(first.shape[2:]) != (3, 3):
        raise ValueError(f"{what}: conv_first.weight has shape {tuple(first.shape)}, expected (64, 3 | 12, 3, 3)")
    if first.shape[0] != FEATURES:
        raise ValueError(f"{what}: conv_first.weight has {first.shape[0]} features, only {FEATURES} are built")
    scale = {3: 4, 12: 2}.get(int(first.shape[1]))
    if scale is None:
        raise ValueError(f"{what}: conv_first.weight has shape {tuple(first.shape)}; Cin must be 3 (x4) or 12 (x2)")
    idx = [int(k.split(".")[1]) for k in clean if k.startswith("body.") and len(k.split(".")) > 2 and k.split(".")[1].isdigit()]
    if not idx:
        raise ValueError(f"{what}: no body.N. key: a network has at least one block (num_block >= 1)")
    num_block = max(idx) + 1
    grow = clean.get("body.0.rdb1.conv1.weight")
    if grow is not None and torch.as_tensor(grow).dim() == 4 and torch.as_tensor(grow).shape[0] != GROWTH:
        raise ValueError(f"{what}: body.0.rdb1.conv1.weight has a growth of {torch.as_tensor(grow).shape[0]}, only {GROWTH} is built")
    want = expected_state(num_block, scale)
    missing, extra = sorted(set(want) - set(clean)), sorted(set(clean) - set(want))
    if missing or extra:
        raise ValueError(f"{what} (num_block {num_block}, x{scale}): " + "; ".join(
            f"{name} {', '.join(ks[:8])}{' ...' if len(ks) > 8 else ''}" for name, ks in (("missing keys", missing), ("unexpected keys", extra)) if ks))
    out = {}
    for k, shape in want.items():
        t = torch.as_tensor(clean[k]).detach().to("cpu", torch.float32)
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{what}: {k} has shape {tuple(t.shape)}, expected {tuple(shape)}")
        out[k] = t.contiguous()
    return RrdbState(out, num_block, scale)


def load(path):
    """torch.load + check_state_dict"""
    return check_state_dict(torch.load(path, map_location="cpu"))


# ------------------------------------------------------------------------------------------------------------------- weight images
def pack_head_weight(w):
    """(64, Cin, 3, 3), Cin = 3 | 12 -> (9 Cin, 64) float32, row (3 ky + kx) Cin + c: the layout of vsp_rrdb_head_u8"""
    w = torch.as_tensor(w)
    if w.dim() != 4 or w.shape[0] != FEATURES or w.shape[1] not in (3, 12) or tuple(w.shape[2:]) != (3, 3):
        raise ValueError(f"pack_head_weight: weight {tuple(w.shape)}, expected ({FEATURES}, 3 | 12, 3, 3)")
    return w.to(torch.float32).permute(2, 3, 1, 0).reshape(9 * w.shape[1], FEATURES).contiguous()


def unpack_head_weight(image):
    """the inverse of pack_head_weight"""
    cin = int(image.shape[0]) // 9
    return image.view(3, 3, cin, FEATURES).permute(3, 2, 0, 1).contiguous()


def pack_conv_weight(w):
    """(Cout, Cin, 3, 3), Cin a multiple of 32 -> the float16 image (Cin / 32, 9, NB, 64, 8) that vsp_rrdb_conv_f16 / vsp_rrdb_tail_u8 read
    as MFMA operands, NB = ceil(Cout / 16):

        image[kc][t][nb][l][j] = f16(w[co = 16 nb + (l & 15)][ci = 32 kc + 8 (l >> 4) + j][ky = t // 3][kx = t % 3])

    kc is the chunk of 32 input channels, t the tap (one K-step of 32 each), l the lane that reads the 16 bytes, j the element; output
    channels past Cout are zero.  Rounding to f16 (nearest even) happens here, once."""
    w = torch.as_tensor(w)
    if w.dim() != 4 or tuple(w.shape[2:]) != (3, 3) or w.shape[0] < 1 or w.shape[1] < 32 or w.shape[1] % 32:
        raise ValueError(f"pack_conv_weight: weight {tuple(w.shape)}, expected (Cout, a multiple of 32, 3, 3)")
    cout, cin = int(w.shape[0]), int(w.shape[1])
    nb = -(-cout // 16)
    wp = torch.zeros((nb * 16, cin, 3, 3), dtype=torch.float16)
    wp[:cout] = w.to(torch.float16)
    v = wp.view(nb, 16, cin // 32, 4, 8, 3, 3)                # nb, l & 15, kc, l >> 4, j, ky, kx
    return v.permute(2, 5, 6, 0, 3, 1, 4).reshape(cin // 32, 9, nb, 64, 8).contiguous()


def unpack_conv_weight(image, cout):
    """the inverse of pack_conv_weight -> (cout, Cin, 3, 3) float16"""
    nkc, nb = int(image.shape[0]), int(image.shape[2])
    v = image.view(nkc, 3, 3, nb, 4, 16, 8).permute(3, 5, 0, 4, 6, 1, 2)      # nb, l & 15, kc, l >> 4, j, ky, kx
    return v.reshape(nb * 16, nkc * 32, 3, 3)[:cout].contiguous()


# ---------------------------------------------------------------------------------------------------------------------------- bands
def net_halo(num_block, scale):
    """The halo of a trunk band in PHOTO rows: the receptive radius of the network in rows of its own input is 1 (conv_first) + 15 nb
    (the dense blocks) + 1 (conv_body) + 1/2 (conv_up1, at twice the resolution) + 3/4 (conv_up2, conv_hr, conv_last at four times) =
    15 nb + 3.25, rounded up to 15 nb + 4; a x2 network's input row is two photo rows."""
    return (15 * int(num_block) + 4) * (1 if int(scale) == 4 else 2)


def net_rows(h, scale):
    """rows (or columns) of the network's input map for a photo side"""
    return int(h) if scale == 4 else (int(h) + 1) // 2


class RrdbUpscaler(SrUpscaler):
    """state: a path, a state dict in the public layout or a checked RrdbState -> the network on `device`, with the interface of
    upscale.SrUpscaler (_sources and upscale_to are its own).  band_rows: the default of upscale().  There is no fallback: what the
    kernels refuse raises.  act_limit bounds one trunk tensor, tail_limit one 4x map (tests scale them down)."""

    def __init__(self, state, device, band_rows=None):
        if isinstance(state, (str, os.PathLike)):
            state = load(state)
        st = check_state_dict(state)
        self.num_block, self.scale, self.band_rows = st.num_block, st.scale, band_rows
        self.halo = net_halo(self.num_block, self.scale)
        self.act_limit = self.tail_limit = ACT_LIMIT
        t = st.tensors
        dev = torch.device(device)
        self.head = (pack_head_weight(t["conv_first.weight"]).to(dev), t["conv_first.bias"].to(dev))
        self.convs = {n: (pack_conv_weight(t[n + ".weight"]).to(dev), t[n + ".bias"].to(dev)) for n in conv_names(self.num_block)[1:-1]}
        bias = torch.zeros(16, dtype=torch.float32)
        bias[:3] = t["conv_last.bias"]
        self.tail = (pack_conv_weight(t["conv_last.weight"]).to(dev), bias.to(dev))
        self.device = self.tail[1].device                     # with its index
        self._work = {}

    # ------------------------------------------------------------------------------------------------------------------ planning
    def _units(self, shapes, band_rows):
        """[(photo, r0, r1, a0, a1), ...] in photo rows and per photo whether it is banded: a photo is cut when band_rows is given or
        when its largest trunk tensor (the 2x map, 512 B per network-input pixel) would reach act_limit; band starts fall on even rows"""
        sp = 1 if self.scale == 4 else 2
        units, banded = [], []
        for k, (h, w) in enumerate(shapes):
            nh, nw = net_rows(h, self.scale), net_rows(w, self.scale)
            rows = band_rows
            if rows is None and nh * nw * 512 > self.act_limit:
                rows = (self.act_limit // (nw * 512) - 2 * (self.halo // sp) - 1) * sp
                if rows < 1:
                    raise ValueError(f"upscale: photo {k}: a band of a {w} pixel wide photo with its halo does not fit {self.act_limit} bytes")
            if rows is None:
                units.append((k, 0, h, 0, h))
            else:
                if int(rows) < 1:
                    raise ValueError(f"upscale: band_rows {rows}")
                rows = int(rows) + (int(rows) & 1)
                units += [(k,) + b for b in plan_bands(h, rows, self.halo)]
            banded.append(rows is not None)
        for k, _, _, a0, a1 in units:
            if (-(-a1 // sp) - a0 // sp) * net_rows(shapes[k][1], self.scale) * 512 > self.act_limit:
                raise ValueError(f"upscale: photo {k}: band_rows {band_rows} with its halo does not fit {self.act_limit} bytes")
        return units, banded

    def tail_bands(self, q0, q1, rows2, nw):
        """Bands of conv_up2 -> conv_hr -> conv_last over rows q0 .. q1 - 1 of a 2x map of rows2 rows whose network input is nw pixels
        wide -> [(r0, r1, a0, a1), ...] in rows of the 2x map.  A band's 4x maps hold 2 (a1 - a0) rows of 4 nw pixels of 128 B.  The
        halo: a 4x output row y needs conv_hr's rows y - 1 .. y + 1, those conv_up2's rows y - 2 .. y + 2, and those rows
        (y - 3) >> 1 .. (y + 3) >> 1 of the 2x map -- for y = 2 r0 that is r0 - 2, for y = 2 r1 - 1 it is r1 + 1: TAIL_HALO = 2."""
        rows = self.tail_limit // (1024 * nw) - 2 * TAIL_HALO
        if rows < 1:
            raise ValueError(f"upscale: a band of the 4x maps of a {4 * nw} pixel wide output does not fit {self.tail_limit} bytes")
        return [(q0 + r0, q0 + r1, max(0, q0 + r0 - TAIL_HALO), min(rows2, q0 + r1 + TAIL_HALO))
                for r0, r1, _, _ in plan_bands(q1 - q0, rows, 0)]

    def _buf(self, name, numel):
        b = self._work.get(name)
        if b is None or b.numel() < numel:
            b = self._work[name] = torch.empty(numel, dtype=torch.float16, device=self.device)
        return b

    # ---------------------------------------------------------------------------------------------------------------------- run
    def _run_unit(self, buffer, src_off, h, w, unit, out, out_off, flag, out_f32):
        """one photo or band: rows r0 .. r1 - 1 of the photo's output from photo rows a0 .. a1 - 1 -> the number of launches"""
        from . import hip_ops as H
        _, r0, r1, a0, a1 = unit
        s, sp = self.scale, (1 if self.scale == 4 else 2)
        n0, n1 = a0 // sp, -(-a1 // sp)
        R, nw = n1 - n0, net_rows(w, s)
        px = R * nw
        dense = [self._buf(f"dense{i}", px * 192) for i in range(3)]
        feat, body, up1 = self._buf("feat", px * 64), self._buf("body", px * 64), self._buf("up1", 4 * px * 64)
        H.rrdb_head_u8(feat, 64, buffer, src_off, h, w, s, *self.head, row0=n0, rows=R)
        H.rrdb_head_u8(dense[0], 192, buffer, src_off, h, w, s, *self.head, row0=n0, rows=R)
        launches = 2
        cur = 0
        for i in range(self.num_block):
            a, b, c = cur, (cur + 1) % 3, (cur + 2) % 3
            for j, (src, dst) in enumerate(((a, b), (b, c), (c, b)), 1):
                x, y = dense[src], dense[dst]
                for k in (1, 2, 3, 4):
                    H.rrdb_conv_f16(x, 192, 32 + 32 * k, x, 192, R, nw, *self.convs[f"body.{i}.rdb{j}.conv{k}"], act=True)
                H.rrdb_conv_f16(y, 192, 0, x, 192, R, nw, *self.convs[f"body.{i}.rdb{j}.conv5"], res1=(x, 192, 0.2),
                                res2=(dense[a], 192, 0.2) if j == 3 else None)
            launches += 15
            cur = b
        H.rrdb_conv_f16(body, 64, 0, dense[cur], 192, R, nw, *self.convs["conv_body"], res1=(feat, 64, 1.0))
        H.rrdb_conv_f16(up1, 64, 0, body, 64, R, nw, *self.convs["conv_up1"], act=True, up=True)
        launches += 2
        # the unit's 4x rows K0 .. K1 - 1 are the photo's output rows s r0 .. s r1 - 1; they come from rows K0 >> 1 .. of the 2x map
        K0, K1 = s * (r0 - a0), s * (r1 - a0)
        pitch, W2 = 3 * s * w, 2 * nw
        for q0, q1, b0, b1 in self.tail_bands(K0 >> 1, (K1 + 1) >> 1, 2 * R, nw):
            n4 = 2 * (b1 - b0) * 2 * W2
            v1, v2 = self._buf("up2", n4 * 64), self._buf("hr", n4 * 64)
            H.rrdb_conv_f16(v1, 64, 0, up1[b0 * W2 * 64:b1 * W2 * 64], 64, b1 - b0, W2, *self.convs["conv_up2"], act=True, up=True)
            H.rrdb_conv_f16(v2, 64, 0, v1, 64, 2 * (b1 - b0), 2 * W2, *self.convs["conv_hr"], act=True)
            k0, k1 = max(K0, 2 * q0), min(K1, 2 * q1)
            H.rrdb_tail_u8(out, out_off + (k0 - K0) * pitch, pitch, s * w, flag, v2, 64, 2 * (b1 - b0), 2 * W2, k0 - 2 * b0, k1 - k0,
                           *self.tail, out_f32=out_f32)
            launches += 3
        return launches

    def upscale(self, photos=None, device_photos=None, out=None, out_offsets=None, band_rows=None, out_f32=None):
        """As upscale.SrUpscaler.upscale: photos or device_photos = (flat uint8 device buffer, byte offsets, [(h, w), ...]) -> (out, info);
        out holds photo k as packed (s h, s w, 3) bytes at out_offsets[k], s the network's scale.  info: `flags` (hip_ops.RRDB_NONFINITE
        per photo), `banded` per photo, `offsets`, `shapes`, `launches`.  band_rows: the trunk runs in bands of that many photo rows
        (rounded up to even) with a halo of net_halo() rows -- the same bytes.  A photo takes 15 nb + 4 launches and 3 per band of the
        4x maps."""
        buffer, offsets, shapes = self._sources(photos, device_photos)
        s = self.scale
        if s == 2 and any((h % 2 and h < 2) or (w % 2 and w < 2) for h, w in shapes):
            raise ValueError("upscale: a x2 network reflects an odd side, which needs at least 2 pixels")
        out_shapes = [(s * h, s * w) for h, w in shapes]
        if out_offsets is None:
            out_offsets = np.concatenate([[0], np.cumsum([3 * h * w for h, w in out_shapes])])[:-1].tolist()
        out_offsets = [int(o) for o in out_offsets]
        if len(out_offsets) != len(shapes) or any(o < 0 for o in out_offsets):
            raise ValueError("upscale: one output offset per photo")
        need = max(o + 3 * h * w for o, (h, w) in zip(out_offsets, out_shapes))
        if out is None:
            out = torch.empty(need, dtype=torch.uint8, device=self.device)
        if (not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous() or out.numel() < need
                or out.device != self.device):
            raise ValueError(f"upscale: out must be a flat contiguous uint8 tensor of at least {need} bytes on {self.device}")
        units, banded = self._units(shapes, self.band_rows if band_rows is None else band_rows)
        flags = torch.zeros(len(shapes), dtype=torch.int32, device=self.device)
        launches = 0
        for unit in units:
            k, r0 = unit[0], unit[1]
            h, w = shapes[k]
            launches += self._run_unit(buffer, offsets[k], h, w, unit, out, out_offsets[k] + s * r0 * 3 * s * w, flags[k:k + 1], out_f32)
        return out, {"flags": flags, "banded": banded, "offsets": out_offsets, "shapes": out_shapes, "launches": launches}

    def describe(self, banded=False, nonfinite=()):
        """the `background` block of report.json"""
        return {"model": MODEL_NAME, "num_block": self.num_block, "scale": self.scale, "banded": bool(banded), "nonfinite": list(nonfinite)}
