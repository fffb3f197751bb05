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


def work_row_bytes(W):
    """row stride of the intermediate image: vsp_lanczos_work_bytes(1, W)"""
    return (3 * int(W) + 3) // 4 * 4


class ResamplePlan:
    """One ragged batch: item i = source image sources[i] (uint8 (sh, sw, 3)), resized to targets[i] = (nw, nh), cropped at origins[i] =
    (x0, y0) to im_size = (H, W), read mirrored where flips[i].  Builds the item table, the coefficient buffer (one table per distinct
    (in, out) pair of the batch) and the packed source bytes, and checks every offset against the buffer sizes.  An item the kernel does
    not serve (kernel_serves) is resized by PIL here and joins the batch as a source of the target size (`self.host_items` lists them)."""

    def __init__(self, sources, targets, origins, im_size, flips=None):
        n = len(sources)
        if not 0 < n <= MAX_ITEMS or len(targets) != n or len(origins) != n:
            raise ValueError(f"ResamplePlan: 1..{MAX_ITEMS} items with one target and one crop origin each")
        self.n, self.H, self.W = n, int(im_size[0]), int(im_size[1])
        if not (1 <= self.H <= MAX_SIDE and 1 <= self.W <= MAX_SIDE):
            raise ValueError(f"ResamplePlan: output size {im_size}")
        flips = [False] * n if flips is None else [bool(f) for f in flips]
        H, W = self.H, self.W
        stride = work_row_bytes(W)
        self.items = (ResampleItem * n)()
        self.host_items = []
        self.sources = []
        tables, coef, coef_ints = {}, [], 0
        src_off = work_off = 0

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
            a = np.asarray(a)
            if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
                raise ValueError(f"item {i}: source must be uint8 (h, w, 3), got {a.dtype} {a.shape}")
            sh, sw = int(a.shape[0]), int(a.shape[1])
            nw, nh, x0, y0 = int(nw), int(nh), int(x0), int(y0)
            flip = flips[i]
            it = self.items[i]
            copy = (sw, sh) == (W, H) and (nw, nh) == (W, H) and (x0, y0) == (0, 0)
            if not copy and not kernel_serves(sw, sh, nw, nh, (x0, y0, x0 + W, y0 + H), (H, W)):
                if nw < 1 or nh < 1:
                    raise ValueError(f"item {i}: resized size {(nw, nh)}")
                a = host_resize(a, nw, nh, (x0, y0, x0 + W, y0 + H), flip)
                sh, sw, nw, nh, x0, y0, flip, copy = H, W, W, H, 0, 0, False, True
                self.host_items.append(i)
            it.src_off, it.sw, it.sh, it.nw, it.nh, it.x0, it.y0 = src_off, sw, sh, nw, nh, x0, y0
            it.flags = (FLIP if flip else 0) | (COPY if copy else 0)
            if copy:
                it.work_off, it.hco, it.vco, it.row0, it.row1, it.hk, it.vk = 0, 0, 0, 0, -1, 0, 0
            else:
                it.hco, it.hk = table(sw, nw)
                it.vco, it.vk = table(sh, nh)
                ymin, ycount, _ = lanczos_coeffs(sh, nh)
                it.row0, it.row1 = int(ymin[y0]), int(ymin[y0 + H - 1] + ycount[y0 + H - 1] - 1)
                if not 0 <= it.row0 <= it.row1 < sh:
                    raise ValueError(f"item {i}: source rows {it.row0}..{it.row1} outside 0..{sh - 1}")
                it.work_off = work_off
                work_off += (it.row1 - it.row0 + 1) * stride
            self.sources.append(np.ascontiguousarray(a))
            src_off += 3 * sw * sh
        self.src_bytes, self.work_bytes, self.coef_ints = src_off, work_off, coef_ints
        self.coef = np.concatenate(coef).astype(np.int32, copy=False) if coef else np.zeros(0, dtype=np.int32)
        self.check()
        self._host = None

    def check(self):
        """every offset of the table against the sizes of the buffers this plan allocates"""
        stride = work_row_bytes(self.W)
        for i, it in enumerate(self.items):
            if it.src_off < 0 or it.src_off + 3 * it.sw * it.sh > self.src_bytes:
                raise ValueError(f"item {i}: source bytes outside the packed buffer")
            if it.flags & COPY:
                continue
            for off, k, out, what in ((it.hco, it.hk, it.nw, "horizontal"), (it.vco, it.vk, it.nh, "vertical")):
                if off < 0 or not 1 <= k <= MAX_TAPS or off + out * (2 + k) > self.coef_ints:
                    raise ValueError(f"item {i}: {what} table outside the coefficient buffer")
            if it.work_off < 0 or it.work_off % 4 or it.work_off + (it.row1 - it.row0 + 1) * stride > self.work_bytes:
                raise ValueError(f"item {i}: rows outside the work buffer")

    def pack(self):
        """items + coefficients + sources in ONE pinned uint8 buffer (16-byte aligned sections; the sources packed without padding, so an
        odd-width image leaves the next one off dword alignment) -> (buffer, items offset, coef offset, src offset)"""
        import torch
        if self._host is None:
            nb = C.sizeof(self.items)
            c0 = (nb + 15) // 16 * 16
            s0 = (c0 + self.coef.nbytes + 15) // 16 * 16
            host = torch.empty(s0 + self.src_bytes, dtype=torch.uint8, pin_memory=torch.cuda.is_available())
            hv = host.numpy()
            hv[:nb] = np.frombuffer(bytes(self.items), dtype=np.uint8)
            hv[c0:c0 + self.coef.nbytes] = self.coef.view(np.uint8)
            for it, a in zip(self.items, self.sources):
                hv[s0 + it.src_off:s0 + it.src_off + a.size] = a.reshape(-1)
            self._host = (host, nb, c0, s0)
        return self._host

    def run(self, device, u8=True, f32=False):
        """Upload (one copy, current stream) and resize on `device` -> (u8 (n, H, W, 3) or None, f32 (n, 3, H, W) or None)."""
        from . import hip_ops
        host, nb, c0, s0 = self.pack()
        dev = host.to(device, non_blocking=True)
        return hip_ops.lanczos_resize_u8(self, dev[:nb], dev[c0:c0 + self.coef.nbytes], dev[s0:], u8=u8, f32=f32)
