"""Host restatement of the device JPEG encoder (csrc/jpeg.hip, vspbfr_amd/jpeg.py) in NumPy int64, without importing the package:
colour transform, 4:2:0 downsampling, edge replication, ISLOW forward DCT, quantisation, the dummy blocks of a partial MCU, Annex K
Huffman coding with restart intervals, byte stuffing and the file's framing.  `encode` returns the file Pillow writes for the same
pixels with save(format="JPEG", quality, subsampling, restart_marker_blocks) and counters of what the scan exercised."""
import io

import numpy as np

SUB = {"444": 0, "420": 2, 0: 0, 2: 2}         # Pillow's subsampling numbers

ZIGZAG = np.array([0, 1, 8, 16, 9, 2, 3, 10, 17, 24, 32, 25, 18, 11, 4, 5, 12, 19, 26, 33, 40, 48, 41, 34, 27, 20, 13, 6, 7, 14, 21, 28,
                   35, 42, 49, 56, 57, 50, 43, 36, 29, 22, 15, 23, 30, 37, 44, 51, 58, 59, 52, 45, 38, 31, 39, 46, 53, 60, 61, 54, 47, 55,
                   62, 63])

Q_LUMA = np.array([16, 11, 10, 16, 24, 40, 51, 61, 12, 12, 14, 19, 26, 58, 60, 55, 14, 13, 16, 24, 40, 57, 69, 56, 14, 17, 22, 29, 51, 87,
                   80, 62, 18, 22, 37, 56, 68, 109, 103, 77, 24, 35, 55, 64, 81, 104, 113, 92, 49, 64, 78, 87, 103, 121, 120, 101, 72, 92,
                   95, 98, 112, 100, 103, 99])
Q_CHROMA = np.array([17, 18, 24, 47, 99, 99, 99, 99, 18, 21, 26, 66, 99, 99, 99, 99, 24, 26, 56, 99, 99, 99, 99, 99, 47, 66, 99, 99, 99,
                     99, 99, 99] + [99] * 32)

# ITU-T T.81 Annex K.3: BITS (codes per length 1..16) and HUFFVAL
DC_LUMA = ([0, 1, 5, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0, 0, 0], list(range(12)))
DC_CHROMA = ([0, 3, 1, 1, 1, 1, 1, 1, 1, 1, 1, 0, 0, 0, 0, 0], list(range(12)))
AC_LUMA = ([0, 2, 1, 3, 3, 2, 4, 3, 5, 5, 4, 4, 0, 0, 1, 0x7d], [
    0x01, 0x02, 0x03, 0x00, 0x04, 0x11, 0x05, 0x12, 0x21, 0x31, 0x41, 0x06, 0x13, 0x51, 0x61, 0x07, 0x22, 0x71, 0x14, 0x32, 0x81, 0x91, 0xa1,
    0x08, 0x23, 0x42, 0xb1, 0xc1, 0x15, 0x52, 0xd1, 0xf0, 0x24, 0x33, 0x62, 0x72, 0x82, 0x09, 0x0a, 0x16, 0x17, 0x18, 0x19, 0x1a, 0x25, 0x26,
    0x27, 0x28, 0x29, 0x2a, 0x34, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55, 0x56,
    0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x83, 0x84, 0x85,
    0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8, 0xa9, 0xaa,
    0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4, 0xd5, 0xd6,
    0xd7, 0xd8, 0xd9, 0xda, 0xe1, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf1, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa])
AC_CHROMA = ([0, 2, 1, 2, 4, 4, 3, 4, 7, 5, 4, 4, 0, 1, 2, 0x77], [
    0x00, 0x01, 0x02, 0x03, 0x11, 0x04, 0x05, 0x21, 0x31, 0x06, 0x12, 0x41, 0x51, 0x07, 0x61, 0x71, 0x13, 0x22, 0x32, 0x81, 0x08, 0x14, 0x42,
    0x91, 0xa1, 0xb1, 0xc1, 0x09, 0x23, 0x33, 0x52, 0xf0, 0x15, 0x62, 0x72, 0xd1, 0x0a, 0x16, 0x24, 0x34, 0xe1, 0x25, 0xf1, 0x17, 0x18, 0x19,
    0x1a, 0x26, 0x27, 0x28, 0x29, 0x2a, 0x35, 0x36, 0x37, 0x38, 0x39, 0x3a, 0x43, 0x44, 0x45, 0x46, 0x47, 0x48, 0x49, 0x4a, 0x53, 0x54, 0x55,
    0x56, 0x57, 0x58, 0x59, 0x5a, 0x63, 0x64, 0x65, 0x66, 0x67, 0x68, 0x69, 0x6a, 0x73, 0x74, 0x75, 0x76, 0x77, 0x78, 0x79, 0x7a, 0x82, 0x83,
    0x84, 0x85, 0x86, 0x87, 0x88, 0x89, 0x8a, 0x92, 0x93, 0x94, 0x95, 0x96, 0x97, 0x98, 0x99, 0x9a, 0xa2, 0xa3, 0xa4, 0xa5, 0xa6, 0xa7, 0xa8,
    0xa9, 0xaa, 0xb2, 0xb3, 0xb4, 0xb5, 0xb6, 0xb7, 0xb8, 0xb9, 0xba, 0xc2, 0xc3, 0xc4, 0xc5, 0xc6, 0xc7, 0xc8, 0xc9, 0xca, 0xd2, 0xd3, 0xd4,
    0xd5, 0xd6, 0xd7, 0xd8, 0xd9, 0xda, 0xe2, 0xe3, 0xe4, 0xe5, 0xe6, 0xe7, 0xe8, 0xe9, 0xea, 0xf2, 0xf3, 0xf4, 0xf5, 0xf6, 0xf7, 0xf8, 0xf9,
    0xfa])


def huff_codes(table):
    """(BITS, HUFFVAL) -> {symbol: (code, length)}: canonical codes in HUFFVAL order (T.81 Annex C)"""
    bits, vals = table
    out, code, k = {}, 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            out[vals[k]] = (code, length)
            code += 1
            k += 1
        code <<= 1
    return out


DC_CODES = (huff_codes(DC_LUMA), huff_codes(DC_CHROMA))
AC_CODES = (huff_codes(AC_LUMA), huff_codes(AC_CHROMA))


def quant_table(quality, chroma):
    """natural order; jpeg_set_quality(q, force_baseline=TRUE)"""
    q = min(max(int(quality), 1), 100)
    scale = 5000 // q if q < 50 else 200 - 2 * q
    return np.clip(((Q_CHROMA if chroma else Q_LUMA).astype(np.int64) * scale + 50) // 100, 1, 255)


def planes(img, sub):
    """(H, W, 3) uint8 -> Y, Cb, Cr as int64 planes padded to whole MCUs, level-shifted by -128"""
    h, w, _ = img.shape
    p = img.astype(np.int64)
    R, G, B = p[..., 0], p[..., 1], p[..., 2]
    Y = (19595 * R + 38470 * G + 7471 * B + 32768) >> 16
    Cb = (-11059 * R - 21709 * G + 32768 * B + (128 << 16) + 32767) >> 16
    Cr = (32768 * R - 27439 * G - 5329 * B + (128 << 16) + 32767) >> 16
    m = 16 if sub == 2 else 8
    ph, pw = -(-h // m) * m, -(-w // m) * m
    ys, xs = np.minimum(np.arange(ph), h - 1), np.minimum(np.arange(pw), w - 1)
    Yp = Y[ys][:, xs]
    if sub == 0:
        return Yp - 128, Cb[ys][:, xs] - 128, Cr[ys][:, xs] - 128
    ch = (h + 1) // 2
    cy = np.minimum(np.arange(ph // 2), ch - 1)
    cx = np.arange(pw // 2)
    out = []
    for C in (Cb, Cr):
        s = 0
        for a in (0, 1):
            for b in (0, 1):
                s = s + C[np.minimum(2 * cy + a, h - 1)][:, np.minimum(2 * cx + b, w - 1)]
        out.append(((s + np.where(cx & 1, 2, 1)[None, :]) >> 2) - 128)
    return Yp - 128, out[0], out[1]


def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _fdct_pass(d, pass2):
    """ISLOW forward DCT along the last axis of an int64 array (jfdctint.c)"""
    F = dict(a=2446, b=3196, c=4433, d=6270, e=7373, f=9633, g=12299, h=15137, i=16069, j=16819, k=20995, m=25172)
    x = [d[..., i] for i in range(8)]
    t0, t7, t1, t6 = x[0] + x[7], x[0] - x[7], x[1] + x[6], x[1] - x[6]
    t2, t5, t3, t4 = x[2] + x[5], x[2] - x[5], x[3] + x[4], x[3] - x[4]
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    sh = 15 if pass2 else 11
    o = [None] * 8
    if pass2:
        o[0], o[4] = _descale(t10 + t11, 2), _descale(t10 - t11, 2)
    else:
        o[0], o[4] = (t10 + t11) << 2, (t10 - t11) << 2
    z1 = (t12 + t13) * F["c"]
    o[2], o[6] = _descale(z1 + t13 * F["d"], sh), _descale(z1 - t12 * F["h"], sh)
    z5 = (t4 + t5 + t6 + t7) * F["f"]
    a1, a2 = -(t4 + t7) * F["e"], -(t5 + t6) * F["k"]
    a3, a4 = -(t4 + t6) * F["i"] + z5, -(t5 + t7) * F["b"] + z5
    o[7] = _descale(t4 * F["a"] + a1 + a3, sh)
    o[5] = _descale(t5 * F["j"] + a2 + a4, sh)
    o[3] = _descale(t6 * F["m"] + a2 + a3, sh)
    o[1] = _descale(t7 * F["g"] + a1 + a4, sh)
    return np.stack(o, axis=-1)


def block_coefficients(plane, qt):
    """padded plane -> (rows of blocks, blocks per row, 64) quantised coefficients in zig-zag order"""
    ph, pw = plane.shape
    b = plane.reshape(ph // 8, 8, pw // 8, 8).transpose(0, 2, 1, 3)
    b = _fdct_pass(b, False)                                          # rows
    b = _fdct_pass(b.swapaxes(-1, -2), True).swapaxes(-1, -2)         # columns
    c = b.reshape(ph // 8, pw // 8, 64)
    d = qt.astype(np.int64) << 3
    k = np.where(c < 0, -((-c + (d >> 1)) // d), (c + (d >> 1)) // d)
    return k[..., ZIGZAG]


def mcu_blocks(img, quality, sub):
    """-> (M, nb, 64) int64 zig-zag coefficients in scan order (nb = 6: Y00 Y01 Y10 Y11 Cb Cr, or 3: Y Cb Cr), comps (nb,) 0 luma / 1 Cb / 2 Cr.
    A luma block of a 4:2:0 MCU that starts past the component's ceil(w / 8) x ceil(h / 8) blocks is the compressor's dummy
    (jccoefct.c compress_data): AC zero, DC of the previous block of the MCU (right edge), or of the last block of the row above it."""
    h, w, _ = img.shape
    Y, Cb, Cr = planes(img, sub)
    ky = block_coefficients(Y, quant_table(quality, 0))
    kb = block_coefficients(Cb, quant_table(quality, 1))
    kr = block_coefficients(Cr, quant_table(quality, 1))
    if sub == 0:
        mh, mw = ky.shape[:2]
        return np.stack([ky, kb, kr], axis=2).reshape(mh * mw, 3, 64), np.array([0, 1, 2])
    mh, mw = kb.shape[:2]
    hb, wb = -(-h // 8), -(-w // 8)
    out = np.zeros((mh, mw, 6, 64), dtype=np.int64)
    for my in range(mh):
        for mx in range(mw):
            for by in (0, 1):
                for bx in (0, 1):
                    i = by * 2 + bx
                    if my * 2 + by < hb and mx * 2 + bx < wb:
                        out[my, mx, i] = ky[my * 2 + by, mx * 2 + bx]
                    else:
                        out[my, mx, i, 0] = out[my, mx, i - 1 if my * 2 + by < hb else 1, 0]
    out[:, :, 4], out[:, :, 5] = kb, kr
    return out.reshape(mh * mw, 6, 64), np.array([0, 0, 0, 0, 1, 2])


class BitWriter:
    def __init__(self):
        self.acc, self.n, self.out, self.stuffed = 0, 0, bytearray(), 0

    def put(self, code, length):
        self.acc = (self.acc << length) | (code & ((1 << length) - 1))
        self.n += length
        while self.n >= 8:
            byte = (self.acc >> (self.n - 8)) & 255
            self.out.append(byte)
            if byte == 255:
                self.out.append(0)
                self.stuffed += 1
            self.n -= 8
        self.acc &= (1 << self.n) - 1

    def flush(self):
        if self.n:
            self.put(0x7F, 8 - self.n)


def encode_scan(blocks, comps, restart):
    """-> (segment bytes with the RSTm markers, [interval bytes], counters)"""
    M = blocks.shape[0]
    cnt = dict(zrl=0, stuffed=0, dc_cat=0, ac_cat=0, intervals=-(-M // restart), last_interval_mcus=M - (-(-M // restart) - 1) * restart)
    seg, pieces = bytearray(), []
    for k0 in range(0, M, restart):
        bw, pred = BitWriter(), [0, 0, 0]
        for m in range(k0, min(k0 + restart, M)):
            for b, comp in enumerate(comps):
                z = blocks[m, b]
                tbl = 1 if comp else 0
                diff = int(z[0]) - pred[comp]
                pred[comp] = int(z[0])
                cat = abs(diff).bit_length()
                cnt["dc_cat"] = max(cnt["dc_cat"], cat)
                bw.put(*DC_CODES[tbl][cat])
                if cat:
                    bw.put(diff if diff > 0 else diff - 1, cat)
                last = 0
                for k in (np.flatnonzero(z[1:]) + 1).tolist():
                    v = int(z[k])
                    run = k - last - 1
                    while run > 15:
                        bw.put(*AC_CODES[tbl][0xF0])
                        cnt["zrl"] += 1
                        run -= 16
                    cat = abs(v).bit_length()
                    cnt["ac_cat"] = max(cnt["ac_cat"], cat)
                    bw.put(*AC_CODES[tbl][(run << 4) | cat])
                    bw.put(v if v > 0 else v - 1, cat)
                    last = k
                if last < 63:
                    bw.put(*AC_CODES[tbl][0x00])
        bw.flush()
        cnt["stuffed"] += bw.stuffed
        if k0:
            seg += bytes([0xFF, 0xD0 + ((k0 // restart - 1) & 7)])
        seg += bw.out
        pieces.append(bytes(bw.out))
    return bytes(seg), pieces, cnt


def _marker(code, payload):
    return bytes([0xFF, code]) + (len(payload) + 2).to_bytes(2, "big") + payload


def _dht(tc_th, table):
    return _marker(0xC4, bytes([tc_th]) + bytes(table[0]) + bytes(table[1]))


def header(h, w, quality, sub, restart):
    """everything in front of the entropy-coded segment, as libjpeg lays it out for Pillow's defaults: SOI, JFIF APP0 (1.01, no density
    unit, 1 x 1), DQT luma, DQT chroma, SOF0, DHT DC0 AC0 DC1 AC1, DRI, SOS"""
    out = b"\xFF\xD8" + _marker(0xE0, b"JFIF\x00\x01\x01\x00\x00\x01\x00\x01\x00\x00")
    for t in (0, 1):
        out += _marker(0xDB, bytes([t]) + bytes(quant_table(quality, t)[ZIGZAG].astype(np.uint8).tolist()))
    out += _marker(0xC0, bytes([8]) + h.to_bytes(2, "big") + w.to_bytes(2, "big") + bytes([3, 1, 0x22 if sub == 2 else 0x11, 0, 2, 0x11, 1, 3, 0x11, 1]))
    out += _dht(0x00, DC_LUMA) + _dht(0x10, AC_LUMA) + _dht(0x01, DC_CHROMA) + _dht(0x11, AC_CHROMA)
    out += _marker(0xDD, restart.to_bytes(2, "big"))
    out += _marker(0xDA, bytes([3, 1, 0x00, 2, 0x11, 3, 0x11, 0, 63, 0]))
    return out


def frame(segment, h, w, quality, sub, restart):
    return header(h, w, quality, sub, restart) + segment + b"\xFF\xD9"


def encode(img, quality=90, subsampling="420", restart=8):
    """-> dict(file, segment, pieces, counters)"""
    sub = SUB[subsampling]
    img = np.ascontiguousarray(img, dtype=np.uint8)
    blocks, comps = mcu_blocks(img, quality, sub)
    seg, pieces, cnt = encode_scan(blocks, comps, int(restart))
    h, w, _ = img.shape
    return dict(file=frame(seg, h, w, quality, sub, int(restart)), segment=seg, pieces=pieces, counters=cnt)


def pillow_file(img, quality=90, subsampling="420", restart=8):
    """the reference: Pillow's own file for the same pixels and parameters (baseline, fixed Huffman tables)"""
    from PIL import Image
    buf = io.BytesIO()
    Image.fromarray(np.ascontiguousarray(img, dtype=np.uint8)).save(buf, format="JPEG", quality=int(quality), subsampling=SUB[subsampling],
                                                                     restart_marker_blocks=int(restart), optimize=False, progressive=False)
    return buf.getvalue()


# ------------------------------------------------------------------------------------------------------------------ test images
KINDS = ("noise", "flat0", "flat128", "flat255", "ramp", "sparse", "blocks")


def named_image(kind, h, w, seed=0):
    """(h, w, 3) uint8: uniform noise (long codes, FF bytes); flat 0 / 128 / 255; a smooth ramp; `sparse`: every 8 x 8 block holds the
    (7, 7) DCT basis function alone at amplitude 40, which leaves a lone last zig-zag coefficient behind a zero run of 62 (three ZRL);
    `blocks`: the top half black and white 8 x 8 blocks in a checker (DC differences of 2040: category 11 at quality 100), the bottom
    half black / white stripes 4 px wide (AC coefficients near 1000: category 10) -- the largest categories 8-bit samples can reach,
    since |DC| <= 1024 and |AC| < 1024 after the quantiser of 1."""
    rng = np.random.RandomState(1000 + seed)
    if kind == "noise":
        return rng.randint(0, 256, (h, w, 3)).astype(np.uint8)
    if kind.startswith("flat"):
        return np.full((h, w, 3), int(kind[4:]), dtype=np.uint8)
    y, x = np.mgrid[0:h, 0:w]
    if kind == "ramp":
        return np.stack([(x * 255) // max(w - 1, 1), (y * 255) // max(h - 1, 1), ((x + y) * 255) // max(h + w - 2, 1)], axis=-1).astype(np.uint8)
    if kind == "sparse":
        v = np.rint(128 + 40 * np.cos((2 * (x & 7) + 1) * 7 * np.pi / 16) * np.cos((2 * (y & 7) + 1) * 7 * np.pi / 16))
        return np.stack([v, v, v], axis=-1).astype(np.uint8)
    if kind == "blocks":
        v = np.where(y < h // 2, 255 * (((x >> 3) + (y >> 3)) & 1), 255 * ((x >> 2) & 1))
        return np.stack([v, 255 - v, v], axis=-1).astype(np.uint8)
    raise ValueError(kind)


# width-first sizes of the issue, as (h, w): 1100 x 37 is wider than the PNG kernel's row limit
SIZES = [(1, 1), (8, 8), (9, 7), (16, 16), (33, 17), (53, 37), (300, 1), (1, 300), (131, 67), (37, 1100), (512, 512)]
QUALITIES = [1, 25, 50, 75, 90, 95, 100]
DEFAULT_RESTART = 8


def restart_values(h, w, subsampling):
    """the restart intervals a size is tried with: 1, 4, the default, one MCU row exactly, more than the image's MCU count"""
    m = 16 if SUB[subsampling] == 2 else 8
    mw, mh = -(-w // m), -(-h // m)
    return [1, 4, DEFAULT_RESTART, mw, min(mw * mh + 3, 65535)]


def thinned_cases():
    """the cross sizes x qualities x subsampling x restart x content, thinned to a few dozen cases in which every value of every
    list appears: a diagonal walk with coprime strides, plus the cases the coverage conditions need"""
    cases, k = [], 0
    n = max(len(SIZES), len(QUALITIES), len(KINDS), 5) * 4
    for i in range(n):
        h, w = SIZES[i % len(SIZES)]
        if (h, w) == (512, 512) and i >= len(SIZES):
            continue                     # one 512 x 512
        sub = ("420", "444")[(i // 2 + i) % 2]
        kind = KINDS[(3 * i + 1) % len(KINDS)]
        cases.append((kind, h, w, QUALITIES[(5 * i + 2) % len(QUALITIES)], sub, restart_values(h, w, sub)[(2 * i + 1) % 5]))
    cases += [("blocks", 53, 37, 100, "444", 4), ("blocks", 53, 37, 100, "420", 8), ("sparse", 131, 67, 75, "420", 4), ("noise", 33, 17, 100, "444", 1),
              ("noise", 131, 67, 100, "420", 8)]
    return cases
