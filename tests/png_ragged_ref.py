"""NumPy restatement of the ragged device PNG encoder (vsp_png_encode_ragged_u8, csrc/png.hip; format in include/vspbfr_hip.h): whole
photos of any width, each with its own size.  Filters, tokens, codes, the stored-block rule and the Adler parts are tests/png_ref.py's,
imported, not copied; what differs is the cut of the filtered stream:

  segments   an image's filtered stream -- n = H (1 + C W) bytes, `png_ref.filter_image` flattened -- is cut into segments of SEG_BYTES
             bytes, the last one shorter.  A boundary may fall inside a row, inside a pixel, on a filter-type byte or right behind one;
             a run of equal bytes is cut there.  Each segment is `png_ref.encode_segment(bytes, final)` on its own
  payload    the segments back to back (each non-final one ends on a byte boundary); the host adds 78 01 in front and the Adler-32
             combined from the segments' parts behind

The files differ in bytes from png_ref.encode_png's for the same pixels, because the segmentation differs; both are valid PNGs."""
import io
import zlib

import numpy as np

from png_ref import adler_combine, adler_parts, assemble, encode_segment, filter_image, named_image, size_cap  # noqa: F401

SEG_BYTES = 24576             # VSP_PNG_RAGGED_SEG_BYTES
SLOT_BYTES = 24588            # VSP_PNG_RAGGED_SLOT_BYTES
MAX_ROW_BYTES = 1 << 20       # VSP_PNG_RAGGED_MAX_ROW_BYTES


def segments(H, W, C):
    return (H * (1 + C * W) + SEG_BYTES - 1) // SEG_BYTES


def segment_bound(n_seg):
    """capacity one segment of n_seg filtered bytes needs: its stored form (5 + n) and the empty stored block (5), up to a dword"""
    return (n_seg + 10 + 3) // 4 * 4


def image_bound(H, W, C):
    """vsp_png_ragged_image_bound: the stored form of every segment, no rounding (the payload is compacted to bytes)"""
    return H * (1 + C * W) + 10 * segments(H, W, C)


def encode_image(img):
    """uint8 (H, W, C) -> dict: filtered (H, 1 + C * W), types, segments [bytes], adler [(a, b, n)], payload, zlib (the whole stream)"""
    img = np.asarray(img, dtype=np.uint8)
    filt, types = filter_image(img)
    flat = filt.reshape(-1)
    nseg = (flat.size + SEG_BYTES - 1) // SEG_BYTES
    segs, parts = [], []
    for k in range(nseg):
        s = flat[k * SEG_BYTES:(k + 1) * SEG_BYTES]
        segs.append(encode_segment(s, k == nseg - 1))
        parts.append(adler_parts(s))
    payload = b"".join(segs)
    stream = b"\x78\x01" + payload + adler_combine(parts).to_bytes(4, "big")
    return {"filtered": filt, "types": types, "segments": segs, "adler": parts, "payload": payload, "zlib": stream}


def encode_png(img):
    img = np.asarray(img, dtype=np.uint8)
    return assemble(encode_image(img)["zlib"], *img.shape)


# (kind, H, W, C): the nine shapes of the prototype run, then the boundary shapes
CASES = [
    ("smooth", 5, 4099, 3), ("smooth", 3, 8200, 3), ("twolevel", 9, 4099, 3), ("noise", 4, 5000, 3), ("constant", 3, 9000, 3),
    ("ramp", 2, 30000, 1), ("smooth", 67, 130, 3), ("smooth", 1, 1, 3), ("constant", 40, 3000, 3),
    ("smooth", 25, 341, 3),        # rows of 1024 filtered bytes divide SEG_BYTES: segment 1 starts on a filter byte
    ("smooth", 26, 982, 1),        # rows of 983 and 25 x 983 = 24575: a filter byte is segment 0's last byte
    ("smooth", 1, 8192, 3),        # a stream of SEG_BYTES + 1 bytes
    ("smooth", 1, 8191, 3),        # and one just under: 24574
    ("smooth", 2, 24576, 1),       # the first row alone is 24577 bytes
    ("constant", 30, 1000, 3),     # a run crosses a segment boundary and is cut there
]


def case_id(case):
    return "%s-%dx%dx%d" % case


_cache = {}


def case_image(case):
    """the case's input, made once and shared (read-only)"""
    if case not in _cache:
        kind, H, W, C = case
        img = named_image(kind, H, W, C)
        img.setflags(write=False)
        _cache[case] = (img, encode_image(img))
    return _cache[case]


def check_image(img, enc, png):
    """the assertions every ragged encoding of `img` has to meet (shared with the GPU tests) -> (IDAT bytes, cap, zlib-RLE bytes)"""
    from PIL import Image
    H, W, C = img.shape
    filt = enc["filtered"]
    assert zlib.decompress(enc["zlib"]) == filt.tobytes()
    got = np.asarray(Image.open(io.BytesIO(png)))
    assert got.shape == ((H, W, 3) if C == 3 else (H, W)) and np.array_equal(got.reshape(H, W, C), img)
    assert int.from_bytes(enc["zlib"][-4:], "big") == zlib.adler32(filt.tobytes())
    nseg = segments(H, W, C)
    assert len(enc["segments"]) == nseg
    for k, s in enumerate(enc["segments"]):
        n_seg = min(SEG_BYTES, filt.size - k * SEG_BYTES)
        assert len(s) <= n_seg + 10 and len(s) <= segment_bound(n_seg) <= SLOT_BYTES
    assert len(enc["payload"]) <= image_bound(H, W, C)
    cap, ref = size_cap(filt, nseg)
    return len(enc["zlib"]), cap, ref
