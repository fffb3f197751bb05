"""Host side of the device LANCZOS resize (csrc/resample.hip): Pillow's coefficient tables, the cover-and-crop geometry of the loaders,
and the plan of one ragged batch.

Pillow resamples 8-bit images in integer arithmetic (libImaging/Resample.c): float64 filter weights, normalised by their sequential
sum, rounded to 22-bit fixed point; a horizontal and then a vertical pass of `clip8((2**21 + sum(pixel * k)) >> 22)` with a uint8 image
between them.  The tables are built here with `math.sin` (libm, the function Pillow calls) and the device does only the integer
multiply-adds, so the kernel's bytes are Pillow's bytes.  `tests/resample_ref.py` restates the passes in NumPy.

No torch / HIP import at module level: the tables and the geometry are testable without the library."""
import ctypes as C
import math

import numpy as np

PRECISION_BITS = 22            # Resample.c: 32 - 8 - 2
MAX_TAPS = 97                  # include/vspbfr_hip.h VSP_RESAMPLE_MAX_TAPS: reductions up to 16x
MAX_SIDE = 8192                # VSP_RESAMPLE_MAX_SIDE
MAX_ITEMS = 65535              # VSP_RESAMPLE_MAX_ITEMS
FLIP, COPY = 1, 2              # vsp_resample_item.flags (VSP_RESAMPLE_FLIP / VSP_RESAMPLE_COPY)

_TABLES = {}


def _lanczos(x):
    if -3.0 <= x < 3.0:
        if x == 0.0:
            return 1.0
        a, b = x * math.pi, x / 3.0 * math.pi
        return (math.sin(a) / a) * (math.sin(b) / b) if b != 0.0 else math.sin(a) / a
    return 0.0


def lanczos_ksize(in_size, out_size):
    """taps per output coordinate of Pillow's table for this size pair"""
    return int(math.ceil(3.0 * max(1.0, in_size / out_size))) * 2 + 1


def lanczos_coeffs(in_size, out_size):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the LANCZOS filter over the whole axis:
    (xmin int32 (out,), count int32 (out,), taps int32 (out, ksize)), cached by (in, out).  The arrays are shared: do not write to them."""
    key = (int(in_size), int(out_size))
    got = _TABLES.get(key)
    if got is not None:
        return got
    in_size, out_size = key
    if in_size < 1 or out_size < 1:
        raise ValueError(f"lanczos_coeffs: sizes {key}")
    scale = in_size / out_size
    filterscale = max(1.0, scale)
    support = 3.0 * filterscale
    ksize = int(math.ceil(support)) * 2 + 1
    ss = 1.0 / filterscale
    xmin = np.zeros(out_size, dtype=np.int32)
    count = np.zeros(out_size, dtype=np.int32)
    taps = np.zeros((out_size, ksize), dtype=np.int32)
    one = float(1 << PRECISION_BITS)
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        lo = max(int(center - support + 0.5), 0)
        n = min(int(center + support + 0.5), in_size) - lo
        w = [_lanczos((x + lo - center + 0.5) * ss) for x in range(n)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        xmin[xx], count[xx] = lo, n
        for x, v in enumerate(w):
            taps[xx, x] = int(-0.5 + v * one) if v < 0 else int(0.5 + v * one)
    got = (xmin, count, taps)
    for a in got:
        a.setflags(write=False)
    _TABLES[key] = got
    return got


def cover_geometry(w, h, im_size, origin=None):
    """(new_w, new_h, box) of imageio._cover_and_crop for a (w, h) image and im_size = (H, W): the LANCZOS target that covers im_size and
    the centre crop box (left, top, right, bottom).  A source of the target size is kept as it is: (w, h, (0, 0, W, H)).
    origin = (x0, y0): the crop origin of the training loader's random crop instead of the centre."""
    H, W = int(im_size[0]), int(im_size[1])
    if h == H and w == W:
        return w, h, (0, 0, W, H)
    ratio = max(1.0 * H / h, 1.0 * W / w)
    new_w, new_h = int(ratio * w), int(ratio * h)
    if origin is None:
        h_idx = (new_h - H) // 2 if new_h - H > 0 else 0
        w_idx = (new_w - W) // 2 if new_w - W > 0 else 0
    else:
        w_idx, h_idx = int(origin[0]), int(origin[1])
    return new_w, new_h, (w_idx, h_idx, int(w_idx + W), int(h_idx + H))


def kernel_serves(sw, sh, nw, nh, box, im_size):
    """True when vsp_lanczos_resize_u8 takes this item: sides and taps within the header's limits and the crop inside the resized image
    (int(ratio * w) can fall one short of the target; PIL pads such a crop with black)."""
    H, W = im_size
    if not (1 <= sw <= MAX_SIDE and 1 <= sh <= MAX_SIDE and 1 <= nw <= MAX_SIDE and 1 <= nh <= MAX_SIDE):
        return False
    if box[0] < 0 or box[1] < 0 or box[0] + W > nw or box[1] + H > nh:
        return False
    return lanczos_ksize(sw, nw) <= MAX_TAPS and lanczos_ksize(sh, nh) <= MAX_TAPS


def host_resize(arr, nw, nh, box, flip=False):
    """The PIL path for an item the kernel refuses: uint8 (h, w, 3) -> the cropped uint8 (H, W, 3)."""
    from PIL import Image
    img = Image.fromarray(arr)
    if flip:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    return np.asarray(img.resize((nw, nh), Image.Resampling.LANCZOS).crop(box), dtype=np.uint8)


class ResampleItem(C.Structure):
    """include/vspbfr_hip.h vsp_resample_item"""
    _fields_ = [("src_off", C.c_int64), ("work_off", C.c_int64), ("hco", C.c_int64), ("vco", C.c_int64)] + [
        (n, C.c_int32) for n in ("sw", "sh", "nw", "nh", "x0", "y0", "row0", "row1", "hk", "vk", "flags", "pad_")]


class ResampleDst(C.Structure):
    """include/vspbfr_hip.h vsp_resample_dst"""
    _fields_ = [("out_off", C.c_int64), ("W", C.c_int32), ("H", C.c_int32)]


def work_row_bytes(W):
    """row stride of the intermediate image: vsp_lanczos_work_bytes(1, W)"""
    return (3 * int(W) + 3) // 4 * 4


class ResamplePlan:
    """One ragged batch: item i = source image sources[i] (uint8 (sh, sw, 3)), resized to targets[i] = (nw, nh), cropped at origins[i] =
    (x0, y0) to im_size = (H, W), read mirrored where flips[i].  Builds the item table, the coefficient buffer (one table per distinct
    (in, out) pair of the batch) and the packed source bytes, and checks every offset against the buffer sizes.  An item the kernel does
    not serve (kernel_serves) is resized by PIL here and joins the batch as a source of the target size (`self.host_items` lists them).

    device_sources = (buffer, offsets): the pixels are on the device already -- item i's (sh, sw, 3) image at byte offsets[i] of the flat
    uint8 tensor `buffer` (jpeg.decode_files' packed output, FacePlan's photos section) --, sources[i] is its (sh, sw), pack() holds
    the tables alone (`upload_bytes`) and run() passes the buffer as `src`.  Only an item the kernel does not serve comes back to the
    host: its slice alone, resized by PIL and uploaded behind the tables.

    out_sizes = [(H_i, W_i), ...] with im_size = None: every item has a window of its own and writes it as packed (H_i, W_i, 3) bytes at
    out_offsets[i] (default: back to back) of one uint8 buffer -- vsp_lanczos_resize_ragged_u8, run_into(out).  The destination table
    is `self.dst`; a host-resized item is not in the kernel's tables (`self.kernel_items` are the others) and is copied into its slot."""

    def __init__(self, sources, targets, origins, im_size, flips=None, device_sources=None, out_sizes=None, out_offsets=None):
        n = len(sources)
        if not 0 < n <= MAX_ITEMS or len(targets) != n or len(origins) != n:
            raise ValueError(f"ResamplePlan: 1..{MAX_ITEMS} items with one target and one crop origin each")
        self.n, self.ragged = n, out_sizes is not None
        if self.ragged:
            if im_size is not None or len(out_sizes) != n or (out_offsets is not None and len(out_offsets) != n):
                raise ValueError("ResamplePlan: out_sizes takes im_size=None and one (H, W) (and one offset) per item")
            sizes = [(int(h), int(w)) for h, w in out_sizes]
            self.H = self.W = None
        else:
            if out_offsets is not None:
                raise ValueError("ResamplePlan: out_offsets belongs to out_sizes")
            sizes = [(int(im_size[0]), int(im_size[1]))] * n
            self.H, self.W = sizes[0]
        for H, W in sizes:                                   # a ragged plan resizes a window above MAX_SIDE on the host
            if H < 1 or W < 1 or (not self.ragged and max(H, W) > MAX_SIDE):
                raise ValueError(f"ResamplePlan: output size {(H, W)}")
        self.out_sizes = sizes
        flips = [False] * n if flips is None else [bool(f) for f in flips]
        self.buffer = None
        if device_sources is not None:
            self.buffer, offsets = device_sources
            if (not hasattr(self.buffer, "data_ptr") or str(self.buffer.dtype) != "torch.uint8" or self.buffer.dim() != 1
                    or not self.buffer.is_contiguous()):
                raise ValueError("ResamplePlan: device_sources takes a flat contiguous uint8 tensor")
            if len(offsets) != n:
                raise ValueError("ResamplePlan: device_sources takes one byte offset per item")
            offsets = [int(o) for o in offsets]
        held = self.buffer is not None
        self.host_items, self.host_pixels, self.kernel_items = [], {}, []
        self.sources = []                                    # what pack() uploads: (src_off, pixels)
        rows = []                                            # the vsp_resample_item fields of every kernel item
        tables, coef, coef_ints = {}, [], 0
        src_off = work_off = 0
        up_off = self.buffer.numel() if held else 0          # uploaded pixels of a held plan follow the buffer (run)

        def table(in_size, out_size):
            """int32 offset of the (in, out) table in the coefficient buffer: xmin[out], count[out], taps[ksize][out] (tap-major)"""
            nonlocal coef_ints
            key = (in_size, out_size)
            if key not in tables:
                xmin, count, taps = lanczos_coeffs(in_size, out_size)
                tables[key] = (coef_ints, taps.shape[1])
                coef.extend((xmin, count, np.ascontiguousarray(taps.T).reshape(-1)))
                coef_ints += out_size * (2 + taps.shape[1])
            return tables[key]

        for i, (a, (nw, nh), (x0, y0)) in enumerate(zip(sources, targets, origins)):
            H, W = sizes[i]
            if held:                                         # the pixels are in the buffer: `a` is the image's (sh, sw)
                if hasattr(a, "dtype") or len(tuple(a)) != 2:
                    raise ValueError(f"item {i}: with device_sources the sources are given as (h, w), not as pixels")
                sh, sw = (int(v) for v in a)
                if sh < 1 or sw < 1:
                    raise ValueError(f"item {i}: source shape {tuple(a)}")
                if offsets[i] < 0 or offsets[i] + 3 * sw * sh > self.buffer.numel():
                    raise ValueError(f"item {i}: source bytes outside the device buffer")
                a, at = None, offsets[i]
            else:
                a = np.asarray(a)
                if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
                    raise ValueError(f"item {i}: source must be uint8 (h, w, 3), got {a.dtype} {a.shape}")
                sh, sw = int(a.shape[0]), int(a.shape[1])
                at = src_off
            nw, nh, x0, y0 = int(nw), int(nh), int(x0), int(y0)
            flip = flips[i]
            copy = (sw, sh) == (W, H) and (nw, nh) == (W, H) and (x0, y0) == (0, 0)
            if not (copy and max(W, H) <= MAX_SIDE) and not kernel_serves(sw, sh, nw, nh, (x0, y0, x0 + W, y0 + H), (H, W)):
                if nw < 1 or nh < 1:
                    raise ValueError(f"item {i}: resized size {(nw, nh)}")
                if held:                                     # this item's slice alone comes back
                    a = self.buffer[at:at + 3 * sw * sh].cpu().numpy().reshape(sh, sw, 3)
                a = host_resize(a, nw, nh, (x0, y0, x0 + W, y0 + H), flip)
                self.host_items.append(i)
                if self.ragged:                              # not an item of the launch: run_into copies it into its slot
                    self.host_pixels[i] = np.array(a)
                    continue
                sh, sw, nw, nh, x0, y0, flip, copy = H, W, W, H, 0, 0, False, True
                if held:
                    at = up_off
                    up_off += 3 * sw * sh
            self.kernel_items.append(i)
            f = dict(src_off=at, sw=sw, sh=sh, nw=nw, nh=nh, x0=x0, y0=y0, flags=(FLIP if flip else 0) | (COPY if copy else 0),
                     work_off=0, hco=0, vco=0, row0=0, row1=-1, hk=0, vk=0)
            if not copy:
                f["hco"], f["hk"] = table(sw, nw)
                f["vco"], f["vk"] = table(sh, nh)
                ymin, ycount, _ = lanczos_coeffs(sh, nh)
                f["row0"], f["row1"] = int(ymin[y0]), int(ymin[y0 + H - 1] + ycount[y0 + H - 1] - 1)
                if not 0 <= f["row0"] <= f["row1"] < sh:
                    raise ValueError(f"item {i}: source rows {f['row0']}..{f['row1']} outside 0..{sh - 1}")
                f["work_off"] = work_off
                work_off += (f["row1"] - f["row0"] + 1) * work_row_bytes(W)
            rows.append(f)
            if a is not None:
                self.sources.append((at - (self.buffer.numel() if held else 0), np.ascontiguousarray(a)))
                if not held:
                    src_off += 3 * sw * sh
        self.items = (ResampleItem * max(len(rows), 1))()
        for it, f in zip(self.items, rows):
            for name, v in f.items():
                setattr(it, name, v)
        self.nk = len(rows)                                  # items of the launch (n, but for the host items of a ragged plan)
        self.up_bytes = (up_off - self.buffer.numel()) if held else src_off      # pixels that pack() uploads
        self.src_bytes = up_off if held else src_off         # bytes of the `src` the entry is given
        self.work_bytes, self.coef_ints = work_off, coef_ints
        self.coef = np.concatenate(coef).astype(np.int32, copy=False) if coef else np.zeros(0, dtype=np.int32)
        self.dst = None
        if self.ragged:
            if out_offsets is None:
                out_offsets, at = [], 0
                for H, W in sizes:
                    out_offsets.append(at)
                    at += 3 * H * W
            self.out_offsets = [int(o) for o in out_offsets]
            self.dst = (ResampleDst * max(self.nk, 1))()
            for d, i in zip(self.dst, self.kernel_items):
                d.out_off, d.H, d.W = self.out_offsets[i], sizes[i][0], sizes[i][1]
            self.out_bytes = max(o + 3 * H * W for o, (H, W) in zip(self.out_offsets, sizes))
        self.check()
        self._host = None

    def check(self):
        """every offset of the tables against the sizes of the buffers this plan allocates or was given"""
        for k in range(self.nk):
            it, i = self.items[k], self.kernel_items[k]
            H, W = self.out_sizes[i]
            if it.src_off < 0 or it.src_off + 3 * it.sw * it.sh > self.src_bytes:
                raise ValueError(f"item {i}: source bytes outside the " + ("device buffer" if self.buffer is not None else "packed buffer"))
            if it.flags & COPY:
                continue
            for off, k_, out, what in ((it.hco, it.hk, it.nw, "horizontal"), (it.vco, it.vk, it.nh, "vertical")):
                if off < 0 or not 1 <= k_ <= MAX_TAPS or off + out * (2 + k_) > self.coef_ints:
                    raise ValueError(f"item {i}: {what} table outside the coefficient buffer")
            if it.work_off < 0 or it.work_off % 4 or it.work_off + (it.row1 - it.row0 + 1) * work_row_bytes(W) > self.work_bytes:
                raise ValueError(f"item {i}: rows outside the work buffer")
        if self.ragged:
            end = 0
            for i, (o, (H, W)) in enumerate(zip(self.out_offsets, self.out_sizes)):
                if o < end:
                    raise ValueError(f"item {i}: destination at byte {o} " + ("is negative" if o < 0 else f"descends or overlaps the one before (which ends at {end})"))
                end = o + 3 * H * W

    def pack(self):
        """items + coefficients (+ the destination table of a ragged plan, at `self.dst_at`) + sources in ONE pinned uint8 buffer
        (16-byte aligned sections; the sources packed without padding, so an odd-width image leaves the next one off dword alignment)
        -> (buffer, items bytes, coef offset, src offset).  With device_sources the source section holds host-resized items only and
        `upload_bytes`, the buffer's size, counts no other source byte."""
        import torch
        if self._host is None:
            nb = self.nk * C.sizeof(ResampleItem)
            c0 = (nb + 15) // 16 * 16
            s0 = (c0 + self.coef.nbytes + 15) // 16 * 16
            self.dst_at = s0
            if self.ragged:
                s0 = (s0 + self.nk * C.sizeof(ResampleDst) + 15) // 16 * 16
            host = torch.empty(s0 + self.up_bytes, dtype=torch.uint8, pin_memory=torch.cuda.is_available())
            hv = host.numpy()
            hv[:nb] = np.frombuffer(bytes(self.items), dtype=np.uint8)[:nb]
            hv[c0:c0 + self.coef.nbytes] = self.coef.view(np.uint8)
            if self.ragged:
                hv[self.dst_at:self.dst_at + self.nk * C.sizeof(ResampleDst)] = np.frombuffer(bytes(self.dst), dtype=np.uint8)[:self.nk * C.sizeof(ResampleDst)]
            for off, a in self.sources:
                hv[s0 + off:s0 + off + a.size] = a.reshape(-1)
            self._host = (host, nb, c0, s0)
        return self._host

    @property
    def upload_bytes(self):
        return self.pack()[0].numel()

    def _sections(self, device):
        """upload (one copy, current stream) -> (items, coef, dst or None, src) on `device`"""
        import torch
        host, nb, c0, s0 = self.pack()
        dev = host.to(device, non_blocking=True)
        src = dev[s0:]
        if self.buffer is not None:
            if self.buffer.device != dev.device:
                raise ValueError(f"ResamplePlan: device_sources is on {self.buffer.device}, the plan goes to {dev.device}")
            src = torch.cat([self.buffer, src]) if self.up_bytes else self.buffer      # host-resized items sit behind the buffer
        dst = dev[self.dst_at:self.dst_at + self.nk * C.sizeof(ResampleDst)] if self.ragged else None
        return dev[:nb], dev[c0:c0 + self.coef.nbytes], dst, src

    def run(self, device, u8=True, f32=False):
        """Upload (one copy, current stream) and resize on `device` -> (u8 (n, H, W, 3) or None, f32 (n, 3, H, W) or None)."""
        from . import hip_ops
        if self.ragged:
            raise ValueError("ResamplePlan: a plan with out_sizes runs through run_into(out)")
        items, coef, _, src = self._sections(device)
        return hip_ops.lanczos_resize_u8(self, items, coef, src, u8=u8, f32=f32)

    def run_into(self, out):
        """Upload (one copy, current stream) and write every item's window into its place in `out`, a flat uint8 device tensor of at
        least out_bytes, on out's device -> out.  Bytes of `out` outside the windows are left alone."""
        import torch

        from . import hip_ops
        if not self.ragged:
            raise ValueError("ResamplePlan: run_into belongs to a plan with out_sizes")
        if not isinstance(out, torch.Tensor) or out.dtype != torch.uint8 or out.dim() != 1 or not out.is_contiguous() or out.numel() < self.out_bytes:
            raise ValueError(f"ResamplePlan: out must be a flat contiguous uint8 tensor of at least {self.out_bytes} bytes")
        if self.nk:
            items, coef, dst, src = self._sections(out.device)
            hip_ops.lanczos_resize_ragged_u8(self, items, coef, src, dst, out)
        for i, a in self.host_pixels.items():
            o = self.out_offsets[i]
            out[o:o + a.size].copy_(torch.from_numpy(a).reshape(-1), non_blocking=False)
        return out
