"""PNG files from a uint8 batch on the device (csrc/png.hip, format in include/vspbfr_hip.h): the kernel filters the rows and writes
each image's deflate stream in segments; this module frames them on the host -- zlib header, the segments, the combined Adler-32, the
PNG chunks with `zlib.crc32` -- which is not the hot path: the bytes are on the host by then.

    encode_batch(u8) -> [bytes]     complete files for a (B, H, W, C) uint8 device tensor, C = 3 or 1
    enqueue(u8) -> Job              the asynchronous form imageio.PngWriter uses: job.files() waits for the job's event
    assemble(...)                   the host framing alone

A shape above the kernel's limits is encoded by PIL, so a caller always gets valid files."""
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
