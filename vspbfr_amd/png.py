"""PNG files from a uint8 batch on the device (csrc/png.hip, format in include/vspbfr_hip.h): the kernel filters the rows and writes
each image's deflate stream in segments; this module frames them on the host -- zlib header, the segments, the combined Adler-32, the
PNG chunks with `zlib.crc32` -- which is not the hot path: the bytes are on the host by then.

    encode_batch(u8) -> [bytes]     complete files for a (B, H, W, C) uint8 device tensor, C = 3 or 1
    enqueue(u8) -> Job              the asynchronous form imageio.PngWriter uses: job.files() waits for the job's event
    assemble(...)                   the host framing alone

A shape above the kernel's limits is encoded by PIL, so a caller always gets valid files.

Whole photos -- any width, each its own size inside one packed buffer, as photo.FacePlan holds them -- take the ragged entry
(vsp_png_encode_ragged_u8), which cuts an image's filtered stream into segments of RAGGED_SEG_BYTES bytes instead of rows:

    encode_ragged(buffer, sizes, offsets) -> [bytes]     packed (h, w, C) images of different sizes
    enqueue_ragged(buffer, sizes, offsets) -> RaggedJob  the asynchronous form imageio.PngWriter.submit_photos uses
    ragged_serves(sizes, C)                              whether one call of the entry takes these images

Its files differ in bytes from encode_batch's for the same pixels (the segmentation differs); both are valid PNGs of those pixels."""
import io
import zlib

import numpy as np
import torch

SEG_ROWS = 8             # include/vspbfr_hip.h VSP_PNG_SEG_ROWS
MAX_ROW_BYTES = 3072     # VSP_PNG_MAX_ROW_BYTES
MAX_H = 32768            # VSP_PNG_MAX_H
MAX_BATCH = 65535        # VSP_PNG_MAX_BATCH
_ADLER = 65521
_SIGNATURE = b"\x89PNG\r\n\x1a\n"


def kernel_serves(shape):
    """True when vsp_png_encode_u8 takes a (B, H, W, C) batch of this shape"""
    if len(shape) != 4:
        return False
    B, H, W, C = (int(v) for v in shape)
    return C in (1, 3) and 1 <= B <= MAX_BATCH and 1 <= H <= MAX_H and 1 <= W and W * C <= MAX_ROW_BYTES


def _chunk(tag, data):
    return len(data).to_bytes(4, "big") + tag + data + zlib.crc32(tag + data).to_bytes(4, "big")


def assemble(slots, seg_bytes, seg_adler, slot, H, W, C):
    """One image's file.  slots: its uint8 output row of the kernel (host), seg_bytes (nseg,), seg_adler (nseg, 2) as the kernel wrote
    them, slot: the segment stride.  Signature, IHDR, one IDAT (zlib header 78 01, the segments, Adler-32), IEND."""
    rowlen = 1 + C * W
    nseg = (H + SEG_ROWS - 1) // SEG_ROWS
    a, b = 1, 0
    parts = [b"\x78\x01"]
    for k in range(nseg):
        nb = int(seg_bytes[k])
        n = min(SEG_ROWS, H - k * SEG_ROWS) * rowlen
        if not 0 < nb <= slot:
            raise RuntimeError(f"png.assemble: segment {k} reports {nb} bytes in a slot of {slot}")
        parts.append(slots[k * slot:k * slot + nb].tobytes())
        b = (b + n * a + (int(seg_adler[k][1]) & 0xFFFFFFFF)) % _ADLER
        a = (a + (int(seg_adler[k][0]) & 0xFFFFFFFF)) % _ADLER
    parts.append((b << 16 | a).to_bytes(4, "big"))
    ihdr = W.to_bytes(4, "big") + H.to_bytes(4, "big") + bytes([8, 2 if C == 3 else 0, 0, 0, 0])
    return _SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", b"".join(parts)) + _chunk(b"IEND", b"")


class Job:
    """One batch in flight: the encoder's outputs on their way to pinned memory and the event behind the copies."""

    def __init__(self, u8):
        from . import hip_ops
        self.shape = tuple(int(v) for v in u8.shape)
        out, seg_bytes, seg_adler, self.slot = hip_ops.png_encode(u8)
        self.host = []
        for t in (out, seg_bytes, seg_adler):
            h = torch.empty(t.shape, dtype=t.dtype, pin_memory=True)
            h.copy_(t, non_blocking=True)
            self.host.append(h)
        self.event = torch.cuda.Event()
        self.event.record()

    def files(self):
        self.event.synchronize()
        out, seg_bytes, seg_adler = (h.numpy() for h in self.host)
        B, H, W, C = self.shape
        return [assemble(out[i], seg_bytes[i], seg_adler[i], self.slot, H, W, C) for i in range(B)]


def enqueue(u8):
    """encoder + asynchronous device-to-host copies on the current stream; no host synchronisation"""
    return Job(u8)


RAGGED_SEG_BYTES = 24576      # VSP_PNG_RAGGED_SEG_BYTES


def _sizes(sizes):
    return [(int(h), int(w)) for h, w in sizes]


def ragged_serves(sizes, C=3):
    """True when one vsp_png_encode_ragged_u8 call takes packed (h, w, C) images of these sizes: C 1 or 3, rows of at most 2^20 bytes,
    every buffer below 2 GiB, the image and segment counts within the header's caps"""
    from . import hip_ops
    sizes = _sizes(sizes)
    if C not in (1, 3) or not 1 <= len(sizes) <= hip_ops.PNG_RAGGED_MAX_IMAGES or any(h < 1 or w < 1 for h, w in sizes):
        return False
    layout = hip_ops.png_ragged_layout(sizes, None, C)
    if layout is None or layout[3] > hip_ops.PNG_RAGGED_MAX_SEGMENTS:
        return False
    return max(sum(C * h * w for h, w in sizes), layout[1], layout[2]) < hip_ops.PNG_LIMIT_BYTES


def assemble_ragged(payload, seg_adler, h, w, C):
    """One image's file around its zlib payload (the segments back to back, as the compact kernel leaves them): seg_adler (nseg, 2) as
    the kernel wrote them, segment k covering bytes k * RAGGED_SEG_BYTES .. of the h (1 + C w) filtered bytes"""
    n = h * (1 + C * w)
    a, b = 1, 0
    for k in range((n + RAGGED_SEG_BYTES - 1) // RAGGED_SEG_BYTES):
        nk = min(RAGGED_SEG_BYTES, n - k * RAGGED_SEG_BYTES)
        b = (b + nk * a + (int(seg_adler[k][1]) & 0xFFFFFFFF)) % _ADLER
        a = (a + (int(seg_adler[k][0]) & 0xFFFFFFFF)) % _ADLER
    ihdr = w.to_bytes(4, "big") + h.to_bytes(4, "big") + bytes([8, 2 if C == 3 else 0, 0, 0, 0])
    stream = b"\x78\x01" + bytes(payload) + (b << 16 | a).to_bytes(4, "big")
    return _SIGNATURE + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", stream) + _chunk(b"IEND", b"")


_side = {}


def _side_stream(device):
    """the stream of the payload copies: a worker thread's copy must not queue behind the next batch on the compute stream"""
    key = torch.device(device).index
    if key not in _side:
        _side[key] = torch.cuda.Stream(device=device)
    return _side[key]


class RaggedJob:
    """One ragged call in flight: the payloads on the device, their byte counts and the Adler parts on the way to pinned memory and the
    event behind them.  files() waits for the event, copies only the used bytes of every payload and frames the files."""

    def __init__(self, buffer, sizes, offsets=None, C=3):
        from . import hip_ops
        self.sizes, self.C = _sizes(sizes), C
        self.out, idat, seg_adler, self.offsets, _, layout = hip_ops.png_encode_ragged(buffer, self.sizes, offsets, C)
        self.seg0 = [r[4] for r in layout[0]] + [layout[3]]
        self.idat = torch.empty(idat.shape, dtype=torch.int32, pin_memory=True)
        self.idat.copy_(idat, non_blocking=True)
        self.adler = torch.empty(seg_adler.shape, dtype=torch.int32, pin_memory=True)
        self.adler.copy_(seg_adler, non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record()

    def files(self):
        self.event.synchronize()
        totals = [int(v) for v in self.idat.numpy()]
        host = torch.empty(max(sum(totals), 1), dtype=torch.uint8, pin_memory=True)
        side = _side_stream(self.out.device)
        with torch.cuda.stream(side):
            at = 0
            for off, nb in zip(self.offsets, totals):
                host[at:at + nb].copy_(self.out[off:off + nb], non_blocking=True)
                at += nb
            side.synchronize()
        data, adler, files, at = host.numpy(), self.adler.numpy(), [], 0
        for i, ((h, w), nb) in enumerate(zip(self.sizes, totals)):
            files.append(assemble_ragged(data[at:at + nb].tobytes(), adler[self.seg0[i]:self.seg0[i + 1]], h, w, self.C))
            at += nb
        self.out = None
        return files


def enqueue_ragged(buffer, sizes, offsets=None, C=3):
    """the three kernels + the asynchronous copies of the byte counts and Adler parts on the current stream; no host synchronisation"""
    return RaggedJob(buffer, sizes, offsets, C)


def encode_ragged(buffer, sizes, offsets=None, C=3):
    """flat uint8 device tensor holding (h, w, C) images of `sizes` = [(h, w), ...] at the byte `offsets` (default: back to back) -> the
    files; PIL encodes a call the entry does not take"""
    sizes = _sizes(sizes)
    if not isinstance(buffer, torch.Tensor) or buffer.dtype != torch.uint8 or buffer.dim() != 1 or not buffer.is_contiguous():
        raise RuntimeError("png.encode_ragged: a flat contiguous uint8 tensor")
    if C not in (1, 3) or any(h < 1 or w < 1 for h, w in sizes):
        raise RuntimeError(f"png.encode_ragged: sizes {sizes}, {C} channels")
    if offsets is None:
        offsets = [0] * len(sizes)
        for i in range(1, len(sizes)):
            offsets[i] = offsets[i - 1] + C * sizes[i - 1][0] * sizes[i - 1][1]
    offsets = [int(o) for o in offsets]
    if len(offsets) != len(sizes) or any(o < 0 or o + C * h * w > buffer.numel() for o, (h, w) in zip(offsets, sizes)):
        raise RuntimeError(f"png.encode_ragged: {buffer.numel()} bytes for the sizes {sizes} at {offsets}")
    if not sizes:
        return []
    if ragged_serves(sizes, C):
        try:
            return RaggedJob(buffer, sizes, offsets, C).files()
        except NotImplementedError:
            pass
    arr = buffer.cpu().numpy()
    return [_pil_file(arr[o:o + C * h * w].reshape(h, w, C)) for o, (h, w) in zip(offsets, sizes)]


def _pil_file(arr):
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(arr[:, :, 0] if arr.shape[2] == 1 else arr).save(buf, format="PNG")
    return buf.getvalue()


def encode_batch(u8):
    """(B, H, W, C) uint8 device tensor -> the B PNG files; PIL encodes a shape the kernel does not take"""
    if not isinstance(u8, torch.Tensor) or u8.dtype != torch.uint8 or u8.dim() != 4 or not u8.is_contiguous():
        raise RuntimeError("png.encode_batch: a contiguous (B, H, W, C) uint8 tensor")
    if u8.shape[3] not in (1, 3):
        raise RuntimeError("png.encode_batch: 1 or 3 channels")
    if not kernel_serves(u8.shape):
        arr = u8.cpu().numpy()
        return [_pil_file(arr[i]) for i in range(arr.shape[0])]
    return Job(u8).files()
