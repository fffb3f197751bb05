"""Background upscaling for whole photos: Real-ESRGAN's compact network, SRVGGNetCompact, on the device -- the host side of
csrc/sr.hip.

    python -m vspbfr_amd.upscale --photos DIR --weights W --out DIR [--scale 2|4] [--format png|jpg] [--band_rows N]

upscales every photo under DIR without any face work and writes OUT/<relative stem>.png (or .jpg) through the writers of the other CLIs.
--scale defaults to the network's own; a x4 network at --scale 2 goes through the ragged device LANCZOS resize down from its
x4 output, as Real-ESRGAN does for an `outscale` below the network's.

    expected_state / check_state_dict / load   the key layout of the public checkpoints (realesr-general-x4v3: 101 entries) and the loader's rules
    pack_head_weight / pack_body_weight        the weight images the kernels read (unpack_body_weight is the inverse)
    plan_bands                                 row bands with a halo of the network's receptive radius: a banded run equals the unbanded bytes
    SrUpscaler                                 weights -> upscale() / upscale_to()

A checkpoint with RRDBNet's keys (`conv_first.weight`: RealESRGAN_x4plus, RealESRGAN_x2plus) is handed to vspbfr_amd.rrdb by
check_background_arguments and make_upscaler; check_state_dict and load here serve the compact network alone.

**No weights are shipped.  The key layout is written from the public model definition and could not be checked against a real checkpoint
file**; a file that deviates is refused by key name, never half-loaded.

The network: conv3x3 3 -> 64, PReLU; num_conv x (conv3x3 64 -> 64, PReLU); conv3x3 64 -> 3 s^2; pixel shuffle by s; plus the nearest-neighbour
upsampling of the input.  Rounding points of the kernels (tests/sr_ref.py restates them): the input is u8 / 255 in fp32; head weights,
every bias and every PReLU slope are fp32; body and tail weights are rounded to f16 once, here; every activation is rounded to f16 behind
its PReLU; products of f16 operands are accumulated in fp32; the output is clamped to [0, 1] and written as rintf(255 v)."""
import argparse
import os
from collections import namedtuple

import numpy as np
import torch

FEATURES = 64
MODEL_NAME = "SRVGGNetCompact"
TILE_H, TILE_W = 8, 32                       # include/vspbfr_hip.h VSP_SR_TILE_*
MAX_ITEMS = 65536                            # VSP_SR_MAX_ITEMS
ACT_LIMIT = (1 << 31) - 128                  # bytes of one activation buffer: the entries refuse 2 GiB or more

SrState = namedtuple("SrState", "tensors num_conv scale")


def expected_state(num_conv=32, scale=4):
    """{key: shape} of an SRVGGNetCompact checkpoint with 64 features: num_conv + 2 convolutions at the even `body` indices, PReLU
    weights at the odd ones -- 3 num_conv + 5 entries"""
    out = {"body.0.weight": (FEATURES, 3, 3, 3), "body.0.bias": (FEATURES,), "body.1.weight": (FEATURES,)}
    for i in range(1, num_conv + 1):
        out[f"body.{2 * i}.weight"] = (FEATURES, FEATURES, 3, 3)
        out[f"body.{2 * i}.bias"] = (FEATURES,)
        out[f"body.{2 * i + 1}.weight"] = (FEATURES,)
    last = 2 * num_conv + 2
    out[f"body.{last}.weight"] = (3 * scale * scale, FEATURES, 3, 3)
    out[f"body.{last}.bias"] = (3 * scale * scale,)
    return out


def check_state_dict(sd):
    """The loader's rules -> SrState(tensors {key: float32 CPU tensor}, num_conv, scale).  A `params_ema` or `params` wrapper is opened and
    a leading `module.` stripped; num_conv comes from the largest `body.N.weight` index (N = 2 num_conv + 2), the scale from that
    convolution's Cout (12 -> 2, 48 -> 4).  Any missing or unexpected key, any wrong shape, a feature count other than 64, num_conv < 1
    and any other Cout is a ValueError that names the key."""
    what = "SRVGGNetCompact checkpoint"
    if isinstance(sd, SrState):
        return sd
    if not isinstance(sd, dict):
        raise ValueError(f"{what}: expected a state dict, got {type(sd).__name__}")
    for wrapper in ("params_ema", "params"):
        if wrapper in sd and isinstance(sd[wrapper], dict):
            sd = sd[wrapper]
            break
    clean = {(k[len("module."):] if str(k).startswith("module.") else str(k)): v for k, v in sd.items()}
    idx = []
    for k in clean:
        parts = k.split(".")
        if len(parts) == 3 and parts[0] == "body" and parts[1].isdigit() and parts[2] == "weight":
            idx.append(int(parts[1]))
    if not idx:
        raise ValueError(f"{what}: no body.N.weight key (keys: {', '.join(sorted(clean)[:4])} ...)")
    last = max(idx)
    if last % 2 or last < 4:
        raise ValueError(f"{what}: the last entry body.{last}.weight gives num_conv {(last - 2) / 2:g}; a network has at least one body "
                         f"convolution and its convolutions at even indices")
    num_conv = (last - 2) // 2
    first = torch.as_tensor(clean.get("body.0.weight", torch.empty(0)))
    if first.dim() == 4 and first.shape[0] != FEATURES:
        raise ValueError(f"{what}: body.0.weight has {first.shape[0]} features, only {FEATURES} are built")
    tail = torch.as_tensor(clean[f"body.{last}.weight"])
    cout = int(tail.shape[0]) if tail.dim() == 4 else -1
    scale = {12: 2, 48: 4}.get(cout)
    if scale is None:
        raise ValueError(f"{what}: body.{last}.weight has shape {tuple(tail.shape)}; Cout must be 12 (x2) or 48 (x4)")
    want = expected_state(num_conv, scale)
    missing, extra = sorted(set(want) - set(clean)), sorted(set(clean) - set(want))
    if missing or extra:
        raise ValueError(f"{what} (num_conv {num_conv}, x{scale}): " + "; ".join(
            f"{name} {', '.join(ks[:8])}{' ...' if len(ks) > 8 else ''}" for name, ks in (("missing keys", missing), ("unexpected keys", extra)) if ks))
    out = {}
    for k, shape in want.items():
        t = torch.as_tensor(clean[k]).detach().to("cpu", torch.float32)
        if tuple(t.shape) != tuple(shape):
            raise ValueError(f"{what}: {k} has shape {tuple(t.shape)}, expected {tuple(shape)}")
        out[k] = t.contiguous()
    return SrState(out, num_conv, scale)


def load(path):
    """torch.load + check_state_dict"""
    return check_state_dict(torch.load(path, map_location="cpu"))


# ------------------------------------------------------------------------------------------------------------------- weight images
def pack_head_weight(w):
    """(64, 3, 3, 3) -> (27, 64) float32, row (3 ky + kx) 3 + c: the layout of vsp_sr_head_u8"""
    return w.to(torch.float32).permute(2, 3, 1, 0).reshape(27, FEATURES).contiguous()


def pack_body_weight(w):
    """(Cout, 64, 3, 3) -> the float16 image (18, NB, 64, 8) that vsp_sr_body_f16 / vsp_sr_tail_u8 copy to LDS, NB = ceil(Cout / 16):

        image[s][nb][l][j] = f16(w[co = 16 nb + (l & 15)][ci = 32 (s & 1) + 8 (l >> 4) + j][ky = (s >> 1) // 3][kx = (s >> 1) % 3])

    s is the K-step of 32 (tap-major: two channel halves per tap), l the lane that reads the 16 bytes as its MFMA operand, j the element;
    output channels past Cout are zero.  Rounding to f16 (nearest even) happens here, once."""
    w = torch.as_tensor(w)
    if w.dim() != 4 or tuple(w.shape[1:]) != (FEATURES, 3, 3) or w.shape[0] < 1:
        raise ValueError(f"pack_body_weight: weight {tuple(w.shape)}, expected (Cout, {FEATURES}, 3, 3)")
    cout = int(w.shape[0])
    nb = -(-cout // 16)
    wp = torch.zeros((nb * 16, FEATURES, 3, 3), dtype=torch.float16)
    wp[:cout] = w.to(torch.float16)
    v = wp.view(nb, 16, 2, 4, 8, 3, 3)                       # nb, l & 15, half, l >> 4, j, ky, kx
    return v.permute(5, 6, 2, 0, 3, 1, 4).reshape(18, nb, 64, 8).contiguous()


def unpack_body_weight(image, cout):
    """the inverse of pack_body_weight -> (cout, 64, 3, 3) float16"""
    nb = int(image.shape[1])
    v = image.view(3, 3, 2, nb, 4, 16, 8).permute(3, 5, 2, 4, 6, 0, 1)      # nb, l & 15, half, l >> 4, j, ky, kx
    return v.reshape(nb * 16, FEATURES, 3, 3)[:cout].contiguous()


# ---------------------------------------------------------------------------------------------------------------------------- bands
def plan_bands(h, band_rows, halo):
    """Row bands of a photo of h rows -> [(r0, r1, a0, a1), ...]: the band writes rows r0 .. r1 - 1 (band_rows of them, the last band
    fewer) and reads rows a0 .. a1 - 1, `halo` more on each inner side, clipped at the photo's edges.  With halo = the number of
    convolutions (the network's receptive radius) every written row sees exactly what it sees in the whole photo."""
    h, band_rows, halo = int(h), int(band_rows), int(halo)
    if h < 1 or band_rows < 1 or halo < 0:
        raise ValueError(f"plan_bands: h {h}, band_rows {band_rows}, halo {halo}")
    return [(r0, min(h, r0 + band_rows), max(0, r0 - halo), min(h, r0 + band_rows + halo)) for r0 in range(0, h, band_rows)]


def tiles_of(h, w):
    return (-(-h // TILE_H)) * (-(-w // TILE_W))


def item_table(units, shapes, src_offsets, out_offsets, scale):
    """units [(photo, r0, r1, a0, a1), ...] (whole photos: (k, 0, h, 0, h)) -> (the _lib.SrItem array of one launch, its activation
    pixels): activations back to back in unit order, the tile list running across the units"""
    from ._lib import SrItem
    tab = (SrItem * len(units))()
    px = tiles = 0
    for t, (k, r0, r1, a0, a1) in zip(tab, units):
        w = shapes[k][1]
        t.src_off, t.act_off = src_offsets[k] + 3 * a0 * w, px
        t.out_off = out_offsets[k] + 3 * scale * w * scale * r0
        t.h, t.w, t.keep0, t.keepn, t.tile0, t.slot = a1 - a0, w, r0 - a0, r1 - r0, tiles, k
        px += (a1 - a0) * w
        tiles += tiles_of(a1 - a0, w)
    return tab, px


class SrUpscaler:
    """state: a path, a state dict in the public layout or a checked SrState -> the network on `device`.  band_rows: the default of
    upscale().  There is no fallback: what the kernels refuse raises."""

    def __init__(self, state, device, band_rows=None):
        if isinstance(state, (str, os.PathLike)):
            state = load(state)
        st = check_state_dict(state)
        self.num_conv, self.scale, self.band_rows = st.num_conv, st.scale, band_rows
        self.halo = self.num_conv + 2
        self.act_limit = ACT_LIMIT
        t = st.tensors
        dev = torch.device(device)
        last = 2 * self.num_conv + 2
        self.head = tuple(v.to(dev) for v in (pack_head_weight(t["body.0.weight"]), t["body.0.bias"], t["body.1.weight"]))
        self.body = [tuple(v.to(dev) for v in (pack_body_weight(t[f"body.{2 * i}.weight"]), t[f"body.{2 * i}.bias"], t[f"body.{2 * i + 1}.weight"]))
                     for i in range(1, self.num_conv + 1)]
        img = pack_body_weight(t[f"body.{last}.weight"])
        bias = torch.zeros(16 * img.shape[1], dtype=torch.float32)
        bias[:3 * self.scale ** 2] = t[f"body.{last}.bias"]
        self.tail = (img.to(dev), bias.to(dev))
        self.device = self.tail[1].device                     # with its index
        self._act = [None, None]

    # -------------------------------------------------------------------------------------------------------------------- sources
    def _sources(self, photos, device_photos):
        if (photos is None) == (device_photos is None):
            raise ValueError("upscale: give photos or device_photos")
        if photos is not None:
            arrs = []
            for k, a in enumerate(photos):
                a = np.asarray(a)
                if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
                    raise ValueError(f"upscale: photo {k} must be uint8 (h, w, 3), got {a.dtype} {a.shape}")
                arrs.append(np.ascontiguousarray(a))
            if not arrs:
                raise ValueError("upscale: at least one photo")
            shapes = [a.shape[:2] for a in arrs]
            offsets = np.concatenate([[0], np.cumsum([a.size for a in arrs])])[:-1].tolist()
            buffer = torch.from_numpy(np.concatenate([a.reshape(-1) for a in arrs])).to(self.device)
        else:
            buffer, offsets, shapes = device_photos
            if (not isinstance(buffer, torch.Tensor) or buffer.dtype != torch.uint8 or buffer.dim() != 1 or not buffer.is_contiguous()
                    or buffer.device != self.device):
                raise ValueError(f"upscale: device_photos takes a flat contiguous uint8 tensor on {self.device}")
        shapes = [(int(h), int(w)) for h, w in shapes]
        offsets = [int(o) for o in offsets]
        if not shapes or len(offsets) != len(shapes) or any(h < 1 or w < 1 for h, w in shapes):
            raise ValueError("upscale: at least one photo, one byte offset per photo, sides of at least 1")
        for o, (h, w) in zip(offsets, shapes):
            if o < 0 or o + 3 * h * w > buffer.numel():
                raise ValueError(f"upscale: a photo of {h} x {w} at byte {o} lies outside the buffer of {buffer.numel()} bytes")
        return buffer, offsets, shapes

    def _units(self, shapes, band_rows):
        """[(photo, r0, r1, a0, a1), ...] and per photo whether it is banded: a photo is cut when band_rows is given or when its
        activation would reach act_limit; a band takes as many rows as fit then"""
        units, banded = [], []
        for k, (h, w) in enumerate(shapes):
            rows = band_rows
            if rows is None and h * w * 128 > self.act_limit:
                rows = self.act_limit // (w * 128) - 2 * self.halo
                if rows < 1:
                    raise ValueError(f"upscale: photo {k}: a band of a {w} pixel wide photo with its halo does not fit {self.act_limit} bytes")
            if rows is None:
                units.append((k, 0, h, 0, h))
            else:
                if int(rows) < 1:
                    raise ValueError(f"upscale: band_rows {rows}")
                units += [(k,) + b for b in plan_bands(h, rows, self.halo)]
            banded.append(rows is not None)
        for k, _, _, a0, a1 in units:
            if (a1 - a0) * shapes[k][1] * 128 > self.act_limit:
                raise ValueError(f"upscale: photo {k}: band_rows {band_rows} with its halo does not fit {self.act_limit} bytes")
        return units, banded

    def _groups(self, units, shapes):
        """consecutive units whose activations fit one buffer together"""
        group, px = [], 0
        for u in units:
            n = (u[4] - u[3]) * shapes[u[0]][1]
            if group and ((px + n) * 128 > self.act_limit or len(group) == MAX_ITEMS):
                yield group
                group, px = [], 0
            group.append(u)
            px += n
        if group:
            yield group

    # ---------------------------------------------------------------------------------------------------------------------- run
    def upscale(self, photos=None, device_photos=None, out=None, out_offsets=None, band_rows=None, out_f32=None):
        """photos: uint8 (h, w, 3) arrays, packed and uploaded -- or device_photos = (flat uint8 device buffer, byte offsets, [(h, w),
        ...]) as jpeg.decode_files and FacePlan hold them -> (out, info).  out: a flat uint8 device buffer that holds photo k as packed
        (s h, s w, 3) bytes at out_offsets[k] (default: a new buffer, back to back), s the network's scale.  info: `flags`, a device int32
        tensor with hip_ops.SR_NONFINITE set for a photo that had a non-finite value before the clamp (its byte is 0); `banded` per photo;
        `offsets`, `shapes` of the outputs; `launches`.  band_rows (default: the constructor's): every photo is processed in bands of
        that many rows with a halo of num_conv + 2 rows -- the same bytes.  out_f32: a flat float32 tensor of out's size that takes the
        unclamped values (tests).  A group whose activations fit one buffer takes num_conv + 2 launches whatever its photo count."""
        from . import hip_ops as H
        buffer, offsets, shapes = self._sources(photos, device_photos)
        s = self.scale
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
        for group in self._groups(units, shapes):
            tab, px = item_table(group, shapes, offsets, out_offsets, s)
            for i in (0, 1):                                   # the ping-pong pair, grown to the largest group seen and reused
                if self._act[i] is None or self._act[i].numel() < px * FEATURES:
                    self._act[i] = torch.empty(px * FEATURES, dtype=torch.float16, device=self.device)
            a, b = self._act
            tab_dev = torch.frombuffer(bytearray(bytes(tab)), dtype=torch.uint8).to(self.device)
            n = len(group)
            H.sr_head_u8(a, buffer, tab, tab_dev, n, *self.head)
            for img, bias, slope in self.body:
                H.sr_body_f16(b, a, tab, tab_dev, n, img, bias, slope)
                a, b = b, a
            H.sr_tail_u8(out, flags, a, buffer, tab, tab_dev, n, self.tail[0], self.tail[1], s, out_f32=out_f32)
            launches += self.num_conv + 2
        return out, {"flags": flags, "banded": banded, "offsets": out_offsets, "shapes": out_shapes, "launches": launches}

    def upscale_to(self, scale, photos=None, device_photos=None, out=None, out_offsets=None, band_rows=None):
        """upscale() for an output scale that may lie below the network's: equal scales write straight into `out`; a x4 network at scale 2
        writes its x4 photos into a buffer of its own and one ragged LANCZOS resize (resample.ResamplePlan with device_sources and
        out_sizes) brings them down into `out`.  A scale above the network's, or 1, is a ValueError."""
        scale = int(scale)
        if scale not in (2, 4) or scale > self.scale:
            raise ValueError(f"upscale: a x{self.scale} network cannot fill an upscale of {scale} (2 or 4, at most the network's scale)")
        if scale == self.scale:
            return self.upscale(photos, device_photos, out, out_offsets, band_rows)
        from .resample import ResamplePlan
        big, info = self.upscale(photos, device_photos, band_rows=band_rows)
        sizes = [(h * scale // self.scale, w * scale // self.scale) for h, w in info["shapes"]]
        plan = ResamplePlan(info["shapes"], [(w, h) for h, w in sizes], [(0, 0)] * len(sizes), None, device_sources=(big, info["offsets"]),
                            out_sizes=sizes, out_offsets=out_offsets)
        if out is None:
            out = torch.empty(plan.out_bytes, dtype=torch.uint8, device=self.device)
        plan.run_into(out)
        return out, dict(info, offsets=plan.out_offsets, shapes=sizes, net_out=big, net_offsets=info["offsets"], net_shapes=info["shapes"])

    def describe(self, banded=False, nonfinite=()):
        """the `background` block of report.json"""
        return {"model": MODEL_NAME, "num_conv": self.num_conv, "scale": self.scale, "banded": bool(banded), "nonfinite": list(nonfinite)}


def is_rrdb_state(sd):
    """whether a loaded checkpoint, behind its optional wrapper and `module.` prefix, has RRDBNet's `conv_first.weight`"""
    if not isinstance(sd, dict):
        return False
    for wrapper in ("params_ema", "params"):
        if wrapper in sd and isinstance(sd[wrapper], dict):
            sd = sd[wrapper]
            break
    return any(str(k) in ("conv_first.weight", "module.conv_first.weight") for k in sd)


def make_upscaler(state, device, band_rows=None):
    """the upscaler of a checked state: rrdb.RrdbUpscaler for an RrdbState, SrUpscaler for an SrState"""
    if isinstance(state, SrState):
        return SrUpscaler(state, device, band_rows=band_rows)
    from .rrdb import RrdbUpscaler
    return RrdbUpscaler(state, device, band_rows=band_rows)


def check_background_arguments(ap, weights, upscale, band_rows=None):
    """The checks both CLIs make before any model goes to the device -> SrState, or rrdb.RrdbState for a checkpoint with RRDBNet's keys
    (the file is opened once); ap.error for a missing file, a checkpoint the loader refuses, an output scale the network cannot fill
    (None: the network's own) and a band of less than one row."""
    if upscale is not None and upscale not in (2, 4):
        ap.error(f"background upscaling needs an upscale of 2 or 4, not {upscale}")
    if band_rows is not None and band_rows < 1:
        ap.error(f"band rows {band_rows} must be at least 1")
    if not os.path.isfile(weights):
        ap.error(f"no such file: {weights}")
    try:
        sd = torch.load(weights, map_location="cpu")
        if is_rrdb_state(sd):
            from . import rrdb
            state = rrdb.check_state_dict(sd)
        else:
            state = check_state_dict(sd)
    except ValueError as e:
        ap.error(str(e))
    if upscale is not None and state.scale < upscale:
        ap.error(f"{weights} is a x{state.scale} network: it cannot fill an upscale of {upscale}")
    return state


def main(argv=None):
    ap = argparse.ArgumentParser(description="Upscale photos with Real-ESRGAN's compact network or its RRDBNet on the device")
    ap.add_argument("--photos", type=str, required=True, help="directory of photos (searched recursively)")
    ap.add_argument("--weights", type=str, required=True,
                    help="SRVGGNetCompact checkpoint, 64 features, or RRDBNet checkpoint (x4plus, x2plus: 64 features, growth 32); not shipped")
    ap.add_argument("--out", type=str, required=True, help="output directory")
    ap.add_argument("--scale", type=int, choices=[2, 4], default=None, help="output scale (default: the network's)")
    ap.add_argument("--format", choices=["png", "jpg"], default="png", help="file format of the output photos")
    ap.add_argument("--band_rows", type=int, default=None, help="process every photo in bands of this many rows (the same bytes)")
    args = ap.parse_args(argv)
    from .imageio import JpegWriter, PngWriter
    from .restore_photos import MAX_PHOTOS_PER_CALL, _decode, list_photos
    state = check_background_arguments(ap, args.weights, args.scale, args.band_rows)
    scale = state.scale if args.scale is None else args.scale
    try:
        names = list_photos(args.photos)
    except (ValueError, OSError) as e:
        ap.error(str(e))
    device = torch.device("cuda", int(os.environ.get("LOCAL_RANK", "0")))
    torch.cuda.set_device(device)
    net = make_upscaler(state, device, band_rows=args.band_rows)
    if args.format == "jpg":
        from .jpeg import DEFAULT_QUALITY
        writer = JpegWriter(quality=DEFAULT_QUALITY, subsampling="420", encode="device")
    else:
        writer = PngWriter()
    ext = "." + args.format
    os.makedirs(args.out, exist_ok=True)
    for i in range(0, len(names), MAX_PHOTOS_PER_CALL):
        group = names[i:i + MAX_PHOTOS_PER_CALL]
        out, info = net.upscale_to(scale, photos=[_decode(os.path.join(args.photos, n)) for n in group])
        flags = info["flags"].cpu().tolist()
        for n, o, (h, w), f in zip(group, info["offsets"], info["shapes"], flags):
            stem = os.path.join(args.out, os.path.splitext(n)[0])
            os.makedirs(os.path.dirname(stem) or ".", exist_ok=True)
            writer.submit(out[o:o + 3 * h * w].view(1, h, w, 3), [stem + ext])
            print(f"{n}: {w} x {h}" + (" (non-finite values were written as 0)" if f else ""))
    writer.drain()


if __name__ == "__main__":
    main()
