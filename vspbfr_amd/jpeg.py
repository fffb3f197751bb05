"""JPEG files from uint8 RGB images on the device (csrc/jpeg.hip, format in include/vspbfr_hip.h): the kernels write each image's
entropy-coded segment -- colour transform, downsampling, DCT, quantisation, Huffman coding, byte stuffing, restart markers -- and this
module frames it on the host with the fixed headers, which is not the hot path: the bytes are on the host by then.  The files equal
Pillow's `save(format="JPEG", quality=, subsampling=, restart_marker_blocks=)` byte for byte (tests/jpeg_ref.py restates every step).

    encode_batch(u8, quality, subsampling, restart) -> [bytes]       a dense (B, H, W, 3) uint8 device tensor
    encode_ragged(buffer, sizes, ...) -> [bytes]                     packed images of different sizes, as photo.FacePlan holds them
    enqueue(buffer, sizes, ...) -> Job                               the asynchronous form imageio.JpegWriter uses
    assemble(segment, h, w, quality, subsampling, restart)           the host framing alone

A call the kernel refuses for its size (a buffer of 2 GiB or more) is encoded by Pillow with the same parameters: the bytes a caller
gets do not depend on the route."""
import io

import numpy as np
import torch

DEFAULT_QUALITY = 90
DEFAULT_RESTART = 8          # MCUs per restart interval: the unit of parallel work of the kernel, 2.x bytes of overhead each
SUBSAMPLING = {"444": 0, "420": 2}

_ZIGZAG = (0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
           35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55, 62, 63)
_Q_LUMA = (16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87, 80, 62,
           18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92, 95, 98, 112, 100,
           103, 99)
_Q_CHROMA = (17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99, 99, 99,
             99) + (99,) * 32
# T.81 Annex K.3: the sixteen code counts, then the symbols
_DC_LUMA = bytes.fromhex("00010501010101010100000000000000") + bytes(range(12))
_DC_CHROMA = bytes.fromhex("00030101010101010101010000000000") + bytes(range(12))
_AC_LUMA = bytes.fromhex(
    "0002010303020403050504040000017d"
    "01020300041105122131410613516107227114328191a1082342b1c11552d1f02433627282090a161718191a25262728292a3435363738393a43444546474849"
    "4a535455565758595a636465666768696a737475767778797a838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3c4c5"
    "c6c7c8c9cad2d3d4d5d6d7d8d9dae1e2e3e4e5e6e7e8e9eaf1f2f3f4f5f6f7f8f9fa")
_AC_CHROMA = bytes.fromhex(
    "00020102040403040705040400010277"
    "000102031104052131061241510761711322328108144291a1b1c109233352f0156272d10a162434e125f11718191a262728292a35363738393a434445464748"
    "494a535455565758595a636465666768696a737475767778797a82838485868788898a92939495969798999aa2a3a4a5a6a7a8a9aab2b3b4b5b6b7b8b9bac2c3"
    "c4c5c6c7c8c9cad2d3d4d5d6d7d8d9dae2e3e4e5e6e7e8e9eaf2f3f4f5f6f7f8f9fa")


def check_params(quality, subsampling, restart):
    """the encoder's parameters, validated (ValueError): quality 1..100, subsampling '444' / '420', restart 1..65535 MCUs"""
    if str(subsampling) not in SUBSAMPLING:
        raise ValueError(f"jpeg: subsampling {subsampling!r} ('420' or '444')")
    if not 1 <= int(quality) <= 100:
        raise ValueError(f"jpeg: quality {quality} outside 1..100")
    if not 1 <= int(restart) <= 65535:
        raise ValueError(f"jpeg: restart interval {restart} outside 1..65535")
    return int(quality), str(subsampling), int(restart)


def quant_table(quality, chroma):
    """64 divisors in natural order: the Annex K table scaled as libjpeg's jpeg_set_quality(q, force_baseline=TRUE) scales it"""
    scale = 5000 // quality if quality < 50 else 200 - 2 * quality
    return [min(max((v * scale + 50) // 100, 1), 255) for v in (_Q_CHROMA if chroma else _Q_LUMA)]


def _marker(code, payload):
    return bytes([0xFF, code]) + (len(payload) + 2).to_bytes(2, "big") + payload


def assemble(segment, h, w, quality=DEFAULT_QUALITY, subsampling="420", restart=DEFAULT_RESTART):
    """One image's file around its entropy-coded segment, laid out as libjpeg writes it for Pillow: SOI, JFIF APP0 (1.01, no density
    unit, 1 x 1, no thumbnail), DQT luma and chroma (zig-zag order), SOF0, DHT DC0 AC0 DC1 AC1, DRI, SOS, the segment, EOI -- payload
    lengths 16, 67, 67, 17, 31, 181, 31, 181, 4, 12."""
    quality, subsampling, restart = check_params(quality, subsampling, restart)
    if not (1 <= h <= 65535 and 1 <= w <= 65535):
        raise ValueError(f"jpeg.assemble: {h} x {w}")
    out = [b"\xFF\xD8", _marker(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")]
    for t in (0, 1):
        q = quant_table(quality, t)
        out.append(_marker(0xDB, bytes([t]) + bytes(q[i] for i in _ZIGZAG)))
    out.append(_marker(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big")
                       + bytes([3, 1, 0x22 if subsampling == "420" else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1])))
    for tc_th, table in ((0x00, _DC_LUMA), (0x10, _AC_LUMA), (0x01, _DC_CHROMA), (0x11, _AC_CHROMA)):
        out.append(_marker(0xC4, bytes([tc_th]) + table))
    out.append(_marker(0xDD, restart.to_bytes(2, "big")))
    out.append(_marker(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0])))
    out.append(bytes(segment))
    out.append(b"\xFF\xD9")
    return b"".join(out)


def pillow_file(arr, quality=DEFAULT_QUALITY, subsampling="420", restart=DEFAULT_RESTART):
    """the host route: Pillow's file for an (H, W, 3) uint8 array at the same parameters (baseline, the standard Huffman tables)"""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(arr, dtype=np.uint8)).save(buf, format="JPEG", quality=int(quality), subsampling=SUBSAMPLING[str(subsampling)],
                                                                     restart_marker_blocks=int(restart), optimize=False, progressive=False)
    return buf.getvalue()


def _sizes(sizes):
    return [(int(h), int(w)) for h, w in sizes]


def kernel_serves(sizes, subsampling="420", restart=DEFAULT_RESTART):
    """True when vsp_jpeg_encode_u8 takes these packed images in one call: sizes 1..65535 and every buffer below 2 GiB"""
    from . import hip_ops
    sizes = _sizes(sizes)
    layout = hip_ops.jpeg_layout(sizes, str(subsampling), restart)
    if layout is None or not 1 <= len(sizes) <= 65535:
        return False
    return max(layout[1:4]) < hip_ops.JPEG_LIMIT_BYTES


_side = {}


def _side_stream(device):
    """the stream of the segment copies: a worker thread's copy must not queue behind the next batch on the compute stream"""
    key = torch.device(device).index
    if key not in _side:
        _side[key] = torch.cuda.Stream(device=device)
    return _side[key]


class Job:
    """One call in flight: the segments on the device, their byte counts on the way to pinned memory and the event behind them.
    files() waits for the event, copies only the used bytes of every segment and frames the files."""

    def __init__(self, buffer, sizes, quality=DEFAULT_QUALITY, subsampling="420", restart=DEFAULT_RESTART):
        from . import hip_ops
        self.params = check_params(quality, subsampling, restart)
        self.sizes = _sizes(sizes)
        self.out, totals, self.offsets = hip_ops.jpeg_encode(buffer, self.sizes, *self.params)
        self.totals = torch.empty(totals.shape, dtype=torch.int32, pin_memory=True)
        self.totals.copy_(totals, non_blocking=True)
        self.event = torch.cuda.Event()
        self.event.record()

    def files(self):
        self.event.synchronize()
        totals = [int(v) for v in self.totals.numpy()]
        host = torch.empty(max(sum(totals), 1), dtype=torch.uint8, pin_memory=True)
        side = _side_stream(self.out.device)
        with torch.cuda.stream(side):
            at = 0
            for off, nb in zip(self.offsets, totals):
                host[at:at + nb].copy_(self.out[off:off + nb], non_blocking=True)
                at += nb
            side.synchronize()
        data, files, at = host.numpy(), [], 0
        for (h, w), nb in zip(self.sizes, totals):
            files.append(assemble(data[at:at + nb].tobytes(), h, w, *self.params))
            at += nb
        self.out = None
        return files


def enqueue(buffer, sizes, quality=DEFAULT_QUALITY, subsampling="420", restart=DEFAULT_RESTART):
    """encoder + the asynchronous copy of the byte counts on the current stream; no host synchronisation"""
    return Job(buffer, sizes, quality, subsampling, restart)


def encode_ragged(buffer, sizes, quality=DEFAULT_QUALITY, subsampling="420", restart=DEFAULT_RESTART):
    """flat uint8 device tensor of (h, w, 3) images back to back + their [(h, w), ...] -> the files; Pillow encodes a call the kernel
    does not take"""
    quality, subsampling, restart = check_params(quality, subsampling, restart)
    sizes = _sizes(sizes)
    if not isinstance(buffer, torch.Tensor) or buffer.dtype != torch.uint8 or buffer.dim() != 1 or not buffer.is_contiguous():
        raise RuntimeError("jpeg.encode_ragged: a flat contiguous uint8 tensor")
    if buffer.numel() != sum(3 * h * w for h, w in sizes) or any(h < 1 or w < 1 for h, w in sizes):
        raise RuntimeError(f"jpeg.encode_ragged: {buffer.numel()} bytes for the sizes {sizes}")
    if not sizes:
        return []
    if kernel_serves(sizes, subsampling, restart):
        try:
            return Job(buffer, sizes, quality, subsampling, restart).files()
        except NotImplementedError:
            pass
    arr, files, at = buffer.cpu().numpy(), [], 0
    for h, w in sizes:
        files.append(pillow_file(arr[at:at + 3 * h * w].reshape(h, w, 3), quality, subsampling, restart))
        at += 3 * h * w
    return files


def encode_batch(u8, quality=DEFAULT_QUALITY, subsampling="420", restart=DEFAULT_RESTART):
    """(B, H, W, 3) uint8 device tensor -> the B JPEG files"""
    if not isinstance(u8, torch.Tensor) or u8.dtype != torch.uint8 or u8.dim() != 4 or u8.shape[3] != 3 or not u8.is_contiguous():
        raise RuntimeError("jpeg.encode_batch: a contiguous (B, H, W, 3) uint8 tensor")
    B, H, W, _ = u8.shape
    return encode_ragged(u8.reshape(-1), [(H, W)] * B, quality, subsampling, restart)
