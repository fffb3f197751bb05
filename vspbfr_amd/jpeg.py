"""JPEG files from uint8 RGB images on the device (csrc/jpeg.hip, format in include/vspbfr_hip.h): the kernels write each image's
entropy-coded segment -- colour transform, downsampling, DCT, quantisation, Huffman coding, byte stuffing, restart markers -- and this
module frames it on the host with the fixed headers, which is not the hot path: the bytes are on the host by then.  The files equal
Pillow's `save(format="JPEG", quality=, subsampling=, restart_marker_blocks=)` byte for byte (tests/jpeg_ref.py restates every step).

    encode_batch(u8, quality, subsampling, restart) -> [bytes]       a dense (B, H, W, 3) uint8 device tensor
    encode_ragged(buffer, sizes, ...) -> [bytes]                     packed images of different sizes, as photo.FacePlan holds them
    enqueue(buffer, sizes, ...) -> Job                               the asynchronous form imageio.JpegWriter uses
    assemble(segment, h, w, quality, subsampling, restart)           the host framing alone

A call the kernel refuses for its size (a buffer of 2 GiB or more) is encoded by Pillow with the same parameters: the bytes a caller
gets do not depend on the route.

The other direction (csrc/jpeg_decode.hip): the host reads the markers in front of the scan, the kernels decode the scan.
The pixels equal Pillow's `Image.open(f).convert("RGB")` byte for byte (tests/jpeg_dec_ref.py restates every step).

    parse(data) -> (Scan, None) | (None, reason)                     the markers in front of the scan; a reason = the host decodes
    decode_batch(datas, device) -> (packed, sizes, offsets, how)     file contents -> (h, w, 3) images back to back on the device
    decode_files(paths, device)                                      the same from paths

A file the parser refuses (progressive, greyscale, 4:2:2, CMYK, ..., or no JPEG at all) and one whose scan the kernels flag (status word
not 0) is decoded by Pillow and copied into its slot: results and exceptions are those of the host path, whatever the route."""
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


# ---------------------------------------------------------------------------------------------------------------------- decoder
class Scan:
    """what the kernels need of one baseline file: h, w, subsampling ('444' / '420'), restart (MCUs, 0 = none), qt (3, 64) uint8 in
    natural order, huff [(BITS, HUFFVAL)] x 6 -- DC and AC table of component 0, of 1, of 2 -- and offset / length of the
    entropy-coded data (to the end of the file: the kernel finds the EOI)"""
    __slots__ = ("h", "w", "subsampling", "restart", "qt", "huff", "offset", "length")

    def tables(self):
        """VSP_JPEG_DEC_TABLE_BYTES: the quantisers, then 16 BITS + 256 HUFFVAL per table"""
        out = np.zeros(3 * 64 + 6 * 272, dtype=np.uint8)
        out[:192] = self.qt.reshape(-1)
        for k, (bits, vals) in enumerate(self.huff):
            at = 192 + k * 272
            out[at:at + 16] = np.frombuffer(bits, dtype=np.uint8)
            out[at + 16:at + 16 + len(vals)] = np.frombuffer(vals, dtype=np.uint8)
        return out


_SOF_REFUSED = {0xC1: "extended sequential (SOF1)", 0xC2: "progressive (SOF2)", 0xC3: "lossless (SOF3)", 0xCC: "arithmetic coding (DAC)"}
_SOF_REFUSED.update({c: "hierarchical or arithmetic coding (SOF%d)" % (c - 0xC0) for c in (0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF)})


def _huff_refusal(bits, vals):
    code = 0
    for length in range(1, 17):
        code += bits[length - 1]
        if code > 1 << length:
            return "a Huffman table overfills the code space"
        if code == 1 << length:
            return "a Huffman table uses the all-ones code"       # the padding of an interval could not be told from it
        code <<= 1
    if len(vals) != sum(bits) or sum(bits) > 256:
        return "a Huffman table is cut short"
    return None


def parse(data):
    """The markers in front of the scan of a JPEG file -> (Scan, None), or (None, reason) for a file the device path does not serve:
    anything but SOF0 with 8 bits, components 1 2 3 sampled (1,1)(1,1)(1,1) or (2,2)(1,1)(1,1), 8-bit quantisers, one interleaved scan
    and no Adobe APP14.  The entropy-coded data is never walked in Python: one vectorised search finds the marker that ends it."""
    data = bytes(data)
    if data[:2] != b"\xFF\xD8":
        return None, "not a JPEG file (no SOI)"
    qts, huff, pos, restart, frame, n = {}, {}, 2, 0, None, len(data)
    while True:
        while pos < n and data[pos] == 0xFF:
            pos += 1
        if pos + 3 > n or data[pos - 1] != 0xFF:
            return None, "no SOS where a marker is expected"
        code = data[pos]
        pos += 1
        if code == 0x01 or 0xD0 <= code <= 0xD7:
            continue
        size = int.from_bytes(data[pos:pos + 2], "big")
        if code == 0xD9 or size < 2 or pos + size > n:
            return None, "a segment runs past the end of the file"
        seg = data[pos + 2:pos + size]
        pos += size
        if code in _SOF_REFUSED:
            return None, _SOF_REFUSED[code]
        if code == 0xEE and seg[:5] == b"Adobe":
            return None, "Adobe APP14 (RGB, CMYK or YCCK coding)"
        if code == 0xDC:
            return None, "DNL"
        if code == 0xDB:
            for i in range(0, len(seg), 65):
                if seg[i] >> 4:
                    return None, "16-bit quantisation table"
                if len(seg) - i < 65:
                    return None, "a quantisation table is cut short"
                qts[seg[i] & 15] = np.frombuffer(seg[i + 1:i + 65], dtype=np.uint8)
        elif code == 0xC4:
            i = 0
            while i + 17 <= len(seg):
                bits = seg[i + 1:i + 17]
                huff[seg[i]] = (bits, seg[i + 17:i + 17 + sum(bits)])
                i += 17 + sum(bits)
        elif code == 0xC0:
            frame = seg
        elif code == 0xDD and len(seg) >= 2:
            restart = int.from_bytes(seg[:2], "big")
        elif code == 0xDA:
            break
    if frame is None or len(frame) < 6:
        return None, "SOS before SOF"
    if frame[0] != 8:
        return None, f"{frame[0]}-bit samples"
    h, w, nf = int.from_bytes(frame[1:3], "big"), int.from_bytes(frame[3:5], "big"), frame[5]
    if h == 0 or w == 0:
        return None, "a side of 0 (DNL)"
    if nf != 3 or len(frame) != 15:
        return None, "greyscale" if nf == 1 else f"{nf} components (CMYK / YCCK)"
    comps = [(frame[6 + 3 * i], frame[7 + 3 * i] >> 4, frame[7 + 3 * i] & 15, frame[8 + 3 * i]) for i in range(3)]
    if [c[0] for c in comps] != [1, 2, 3]:
        return None, "component ids other than 1, 2, 3 (RGB-coded)"
    sampling = [c[1:3] for c in comps]
    if sampling not in ([(1, 1)] * 3, [(2, 2), (1, 1), (1, 1)]):
        return None, "sampling factors %s (4:2:2, 4:4:0, ...)" % sampling
    if len(seg) != 10 or seg[0] != 3:
        return None, "a scan of %d components (several scans)" % (seg[0] if seg else 0)
    if [seg[1], seg[3], seg[5]] != [1, 2, 3] or tuple(seg[7:10]) != (0, 63, 0):
        return None, "a reordered or progressive scan"
    s = Scan()
    s.h, s.w, s.subsampling, s.restart, s.huff, qt = h, w, "420" if sampling[0] == (2, 2) else "444", restart, [], []
    for i in range(3):
        td, ta = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
        if td not in huff or (0x10 | ta) not in huff or comps[i][3] not in qts:
            return None, "a table the scan selects is missing"
        for t in (huff[td], huff[0x10 | ta]):
            why = _huff_refusal(*t)
            if why:
                return None, why
            s.huff.append(t)
        nat = np.zeros(64, dtype=np.uint8)
        nat[list(_ZIGZAG)] = qts[comps[i][3]]
        qt.append(nat)
    s.qt, s.offset, s.length = np.stack(qt), pos, n - pos
    from .hip_ops import JPEG_DEC_MAX_SCAN_BYTES
    if not 1 <= s.length <= JPEG_DEC_MAX_SCAN_BYTES:
        return None, f"{s.length} bytes of entropy-coded data"
    a = np.frombuffer(data, dtype=np.uint8, offset=pos)
    nx = a[1:]
    hit = np.flatnonzero((a[:-1] == 0xFF) & (nx != 0) & (nx != 0xFF) & ((nx & 0xF8) != 0xD0))
    if hit.size and nx[hit[0]] != 0xD9:
        return None, "marker %02X behind the scan (several scans, DNL)" % nx[hit[0]]
    return s, None


def host_pixels(data):
    """the host route: Pillow's default decode of a file's contents"""
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"), dtype=np.uint8)


def decode_batch(datas, device, sub_bytes=None, want_rounds=False, pool=None):
    """File contents -> (packed uint8 device tensor of (h, w, 3) images back to back, [(h, w), ...], byte offsets, how) with how[i] in
    {"device", "host"}; with want_rounds a fifth value, the kernel's round count per file (0 for a host file).  The compressed bytes
    and one pinned block of items and tables go up on the current stream; the status words are read once, and a refused or flagged
    file is decoded by Pillow -- whose exception, if it raises one, is the caller's -- and copied into its slot.  pool: an executor
    whose map() decodes the files of the host route side by side instead of one after the other on the calling thread."""
    from . import hip_ops
    datas = [bytes(d) for d in datas]
    scans = [parse(d)[0] for d in datas]
    hmap = map if pool is None else pool.map

    def on_host(which):
        return dict(zip(which, hmap(host_pixels, [datas[i] for i in which])))
    host = on_host([i for i, s in enumerate(scans) if s is None])
    sizes = [host[i].shape[:2] if s is None else (s.h, s.w) for i, s in enumerate(scans)]
    offsets = [0] * len(datas)
    for i in range(1, len(datas)):
        offsets[i] = offsets[i - 1] + 3 * sizes[i - 1][0] * sizes[i - 1][1]
    total = offsets[-1] + 3 * sizes[-1][0] * sizes[-1][1] if datas else 0
    packed = torch.empty(total, device=device, dtype=torch.uint8)
    rounds = [0] * len(datas)
    dev = [i for i, s in enumerate(scans) if s is not None]
    if dev and sum(scans[i].length for i in dev) >= hip_ops.JPEG_LIMIT_BYTES:
        host.update(on_host(dev))
        dev = []
    if dev:
        comp = torch.empty(sum(scans[i].length for i in dev), dtype=torch.uint8, pin_memory=True)
        view, specs, at = comp.numpy(), [], 0
        for i in dev:
            s = scans[i]
            view[at:at + s.length] = np.frombuffer(datas[i], dtype=np.uint8, offset=s.offset)
            specs.append((at, s.length, s.h, s.w, SUBSAMPLING[s.subsampling], s.restart))
            at += s.length
        tables = np.concatenate([scans[i].tables() for i in dev])
        with torch.cuda.device(device):
            try:
                _, status, rnd, _ = hip_ops.jpeg_decode(comp.to(device, non_blocking=True), specs, tables, sub_bytes, out=packed,
                                                        out_offsets=[offsets[i] for i in dev], want_rounds=want_rounds)
                words = torch.stack([status, rnd]).cpu().numpy() if want_rounds else status.cpu().numpy()[None]
            except NotImplementedError:
                words = np.ones((1, len(dev)), dtype=np.int32)
        host.update(on_host([i for k, i in enumerate(dev) if words[0, k]]))
        for k, i in enumerate(dev):
            if words[0, k]:
                assert host[i].shape[:2] == sizes[i]
            elif want_rounds:
                rounds[i] = int(words[1, k])
    for i, arr in host.items():
        packed[offsets[i]:offsets[i] + arr.size].copy_(torch.from_numpy(np.array(arr)).reshape(-1))
    how = ["host" if i in host else "device" for i in range(len(datas))]
    return (packed, sizes, offsets, how, rounds) if want_rounds else (packed, sizes, offsets, how)


def decode_files(paths, device, sub_bytes=None, pool=None):
    """decode_batch over the contents of `paths` (a file that is no JPEG, a PNG for instance, takes the host decode in the same call;
    pool: decode_batch's)"""
    datas = []
    for p in paths:
        with open(p, "rb") as f:
            datas.append(f.read())
    return decode_batch(datas, device, sub_bytes, pool=pool)
