"""NumPy restatement of the device PNG encoder (csrc/png.hip, format in include/vspbfr_hip.h): the specification the kernel is held to,
byte for byte.  Every step is integer arithmetic.

  filters    per row the PNG filter type (0 None, 1 Sub, 2 Up, 3 Average, 4 Paeth) with the smallest sum of |residual as int8|, ties to the
             lowest type; the row above is the image's real previous row (zeros above row 0), also across segment boundaries
  segments   the filtered stream (H rows of 1 + C * W bytes) in segments of ROWS rows, each compressed on its own into ONE deflate block:
             dynamic Huffman, or a stored block when the coded segment would not be smaller.  A non-final segment ends with an empty
             stored block (3 header bits, padding, 00 00 FF FF); the last segment's block carries BFINAL
  tokens     literals and distance-1 matches.  A stretch is a maximal run of positions whose byte equals the byte before it inside the
             segment; it is cut into chunks of 258 from its start; a chunk of 3 or more is one match, a shorter one is literals
  codes      Huffman code lengths from the block's histogram: symbols sorted by (count, symbol), the two-queue merge taking a leaf before
             an internal node of the same weight, depths clipped to the limit (15; 7 for the code-length code) and repaired as zlib does
             (a leaf from the deepest level below the limit gets a sibling from the limit level, Kraft sum - 1 per step), the lengths then
             handed out longest first in sorted order; canonical codes.  The only distance symbol is 0 (length 1, or 0 without a match)
  adler      per segment (sum of bytes, sum of (n - i) * byte[i]) mod 65521, combined in order
"""
import zlib

import numpy as np

ROWS = 8                 # rows per segment: VSP_PNG_SEG_ROWS
MAX_ROW_BYTES = 3072     # C * W the kernel takes: VSP_PNG_MAX_ROW_BYTES
MAX_H = 32768            # VSP_PNG_MAX_H
ADLER = 65521
CL_ORDER = (16, 17, 18, 0, 8, 7, 9, 6, 10, 5, 11, 4, 12, 3, 13, 2, 14, 1, 15)
_LEN_BASE = (3, 4, 5, 6, 7, 8, 9, 10, 11, 13, 15, 17, 19, 23, 27, 31, 35, 43, 51, 59, 67, 83, 99, 115, 131, 163, 195, 227, 258)
_LEN_EXTRA = (0, 0, 0, 0, 0, 0, 0, 0, 1, 1, 1, 1, 2, 2, 2, 2, 3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5, 0)
_LEN_SYM = np.zeros(259, dtype=np.int64)      # match length -> index into the two tables above
for _k, _b in enumerate(_LEN_BASE):
    _LEN_SYM[_b:] = _k


def segment_bound(rows, W, C):
    """capacity of one segment's slot: its stored form (5 + n) and the 5 bytes of the empty stored block, rounded up to a dword"""
    return (rows * (1 + C * W) + 10 + 3) // 4 * 4


def image_bound(H, W, C):
    return ((H + ROWS - 1) // ROWS) * segment_bound(ROWS, W, C)


def filter_image(img):
    """uint8 (H, W, C) -> (filtered uint8 (H, 1 + C * W), types (H,))"""
    img = np.asarray(img, dtype=np.uint8)
    H, W, C = img.shape
    cur = img.reshape(H, W * C).astype(np.int32)
    up = np.zeros_like(cur)
    up[1:] = cur[:-1]
    left = np.zeros_like(cur)
    left[:, C:] = cur[:, :-C]
    ul = np.zeros_like(cur)
    ul[1:, C:] = cur[:-1, :-C]
    p = left + up - ul
    pa, pb, pc = np.abs(p - left), np.abs(p - up), np.abs(p - ul)
    paeth = np.where((pa <= pb) & (pa <= pc), left, np.where(pb <= pc, up, ul))
    res = np.stack([cur, cur - left, cur - up, cur - ((left + up) >> 1), cur - paeth]) & 255
    cost = np.where(res < 128, res, 256 - res).sum(axis=2)
    types = np.argmin(cost, axis=0)                     # the first minimum: ties go to the lowest type
    out = np.empty((H, 1 + W * C), dtype=np.uint8)
    out[:, 0] = types
    out[:, 1:] = res[types, np.arange(H)]
    return out, types


def tokens(s):
    """segment bytes -> (literal mask, match-start mask, match length per position)"""
    n = len(s)
    i = np.arange(n)
    eq = np.zeros(n, dtype=bool)
    eq[1:] = s[1:] == s[:-1]
    q = np.maximum.accumulate(np.where(~eq, i, -1)) + 1            # start of the stretch a position belongs to
    e = np.minimum.accumulate(np.where(~eq, i, n)[::-1])[::-1]     # first position behind it
    j = i - q
    clen = np.minimum(258, (e - q) - 258 * (j // 258))
    long = eq & (clen >= 3)
    return ~long, long & (j % 258 == 0), clen


def code_lengths(freq, maxbits):
    """length-limited Huffman code lengths; see the module text for the rule"""
    used = sorted((s for s in range(len(freq)) if freq[s] > 0), key=lambda s: (freq[s], s))
    m = len(used)
    lens = [0] * len(freq)
    if m == 0:
        return lens
    if m == 1:
        lens[used[0]] = 1
        return lens
    lw = [int(freq[s]) for s in used]
    nw, leafpar, nodepar = [], [0] * m, [0] * (m - 1)
    li = ni = 0
    for t in range(m - 1):
        w = 0
        for _ in range(2):
            if li < m and (ni >= len(nw) or lw[li] <= nw[ni]):
                w += lw[li]
                leafpar[li] = t
                li += 1
            else:
                w += nw[ni]
                nodepar[ni] = t
                ni += 1
        nw.append(w)
    depth = [0] * (m - 1)
    for k in range(m - 3, -1, -1):
        depth[k] = depth[nodepar[k]] + 1
    count = [0] * (maxbits + 1)
    kraft = 0
    for a in range(m):
        d = min(depth[leafpar[a]] + 1, maxbits)
        count[d] += 1
        kraft += 1 << (maxbits - d)
    while kraft > (1 << maxbits):
        bits = maxbits - 1
        while count[bits] == 0:
            bits -= 1
        count[bits] -= 1
        count[bits + 1] += 2
        count[maxbits] -= 1
        kraft -= 1
    a = 0
    for bits in range(maxbits, 0, -1):
        for _ in range(count[bits]):
            lens[used[a]] = bits
            a += 1
    return lens


def canonical_codes(lens, maxbits):
    """bit-reversed canonical codes (deflate sends Huffman codes most significant bit first)"""
    count = [0] * (maxbits + 2)
    for v in lens:
        count[v] += 1
    count[0] = 0
    nxt, code = [0] * (maxbits + 2), 0
    for bits in range(1, maxbits + 1):
        code = (code + count[bits - 1]) << 1
        nxt[bits] = code
    out = [0] * len(lens)
    for s, v in enumerate(lens):
        if v:
            out[s] = int(format(nxt[v], "0%db" % v)[::-1], 2)
            nxt[v] += 1
    return out


def cl_tokens(seq):
    """run-length form of the code-length sequence: [(symbol, extra value, extra bits)]"""
    out, i, n = [], 0, len(seq)
    while i < n:
        v, run = seq[i], 1
        while i + run < n and seq[i + run] == v:
            run += 1
        if v == 0:
            if run >= 11:
                r = min(run, 138)
                out.append((18, r - 11, 7))
            elif run >= 3:
                r = run
                out.append((17, r - 3, 3))
            else:
                r = 1
                out.append((0, 0, 0))
        elif i > 0 and seq[i - 1] == v and run >= 3:
            r = min(run, 6)
            out.append((16, r - 3, 2))
        else:
            r = 1
            out.append((v, 0, 0))
        i += r
    return out


class _Bits:
    def __init__(self):
        self.vals, self.nbits = [], []

    def put(self, v, n):
        self.vals.append(int(v))
        self.nbits.append(int(n))


def _pack(vals, nbits):
    """values (< 2**40) of nbits bits each, least significant bit first -> (bytes, bit count)"""
    vals = np.asarray(vals, dtype=np.uint64)
    nbits = np.asarray(nbits, dtype=np.int64)
    off = np.concatenate([[0], np.cumsum(nbits)])
    total = int(off[-1])
    off = off[:-1]
    nbytes = (total + 7) // 8
    sh = vals << (off & 7).astype(np.uint64)                    # < 2**47
    acc = np.zeros(nbytes + 8, dtype=np.float64)
    for k in range(6):
        part = ((sh >> np.uint64(8 * k)) & np.uint64(255)).astype(np.float64)
        acc += np.bincount((off >> 3) + k, weights=part, minlength=nbytes + 8)      # disjoint bits: a sum is an or
    return acc[:nbytes].astype(np.uint8).tobytes(), total


def encode_segment(s, final):
    """one segment's filtered bytes -> its deflate bytes"""
    s = np.asarray(s, dtype=np.uint8)
    n = len(s)
    lit, start, clen = tokens(s)
    lsym = 257 + _LEN_SYM[clen[start]]
    hist = np.bincount(s[lit], minlength=286) + np.bincount(lsym, minlength=286)
    hist[256] = 1
    nmatch = int(start.sum())
    lens = code_lengths(hist, 15)
    codes = canonical_codes(lens, 15)
    dlen = 1 if nmatch else 0
    nlit = max(257, max(k for k in range(286) if lens[k]) + 1)
    cl = cl_tokens(lens[:nlit] + [dlen])
    clh = [0] * 19
    for sym, _, _ in cl:
        clh[sym] += 1
    cll = code_lengths(clh, 7)
    clc = canonical_codes(cll, 7)
    ncl = max(4, max(k for k in range(19) if cll[CL_ORDER[k]]) + 1)
    head = _Bits()
    head.put(1 if final else 0, 1)
    head.put(2, 2)
    head.put(nlit - 257, 5)
    head.put(0, 5)
    head.put(ncl - 4, 4)
    for k in range(ncl):
        head.put(cll[CL_ORDER[k]], 3)
    for sym, ev, eb in cl:
        head.put(clc[sym] | ev << cll[sym], cll[sym] + eb)
    lens_a, codes_a = np.asarray(lens, dtype=np.int64), np.asarray(codes, dtype=np.int64)
    vals = np.zeros(n, dtype=np.int64)
    nb = np.zeros(n, dtype=np.int64)
    vals[lit], nb[lit] = codes_a[s[lit]], lens_a[s[lit]]
    k = _LEN_SYM[clen[start]]
    extra = clen[start] - np.asarray(_LEN_BASE)[k]
    eb = np.asarray(_LEN_EXTRA)[k]
    vals[start] = codes_a[257 + k] | extra << lens_a[257 + k]            # the distance code (symbol 0) is one 0 bit behind them
    nb[start] = lens_a[257 + k] + eb + 1
    keep = nb > 0
    body, bits = _pack(head.vals + vals[keep].tolist() + [codes[256]], head.nbits + nb[keep].tolist() + [lens[256]])
    tail = b""
    if not final:
        body = body + (b"\0" if (bits & 7) == 0 or (bits & 7) > 5 else b"")   # the 3 header bits of the empty stored block, padded
        tail = b"\0\0\xff\xff"
    coded = body + tail
    stored = bytes([1 if final else 0, n & 255, n >> 8, ~n & 255, (~n >> 8) & 255]) + s.tobytes() + (b"" if final else b"\0\0\0\xff\xff")
    return coded if len(coded) < len(stored) else stored


def adler_parts(s):
    s = np.asarray(s, dtype=np.int64)
    n = len(s)
    return int(s.sum() % ADLER), int((s * (n - np.arange(n))).sum() % ADLER), n


def adler_combine(parts):
    a, b = 1, 0
    for pa, pb, n in parts:
        b = (b + n * a + pb) % ADLER
        a = (a + pa) % ADLER
    return b << 16 | a


def encode_image(img):
    """uint8 (H, W, C) -> dict: filtered (H, 1 + C * W), segments [bytes], adler [(a, b, n)], zlib (the whole stream)"""
    img = np.asarray(img, dtype=np.uint8)
    H, W, C = img.shape
    filt, types = filter_image(img)
    nseg = (H + ROWS - 1) // ROWS
    segs, parts = [], []
    for k in range(nseg):
        s = filt[k * ROWS:(k + 1) * ROWS].reshape(-1)
        segs.append(encode_segment(s, k == nseg - 1))
        parts.append(adler_parts(s))
    stream = b"\x78\x01" + b"".join(segs) + adler_combine(parts).to_bytes(4, "big")
    return {"filtered": filt, "types": types, "segments": segs, "adler": parts, "zlib": stream}


def _chunk(tag, data):
    return len(data).to_bytes(4, "big") + tag + data + zlib.crc32(tag + data).to_bytes(4, "big")


def assemble(stream, H, W, C):
    """signature, IHDR (8 bit, colour type 2 for C = 3 and 0 for C = 1, no interlace), one IDAT, IEND"""
    ihdr = W.to_bytes(4, "big") + H.to_bytes(4, "big") + bytes([8, {3: 2, 1: 0}[C], 0, 0, 0])
    return b"\x89PNG\r\n\x1a\n" + _chunk(b"IHDR", ihdr) + _chunk(b"IDAT", stream) + _chunk(b"IEND", b"")


def encode_png(img):
    img = np.asarray(img, dtype=np.uint8)
    return assemble(encode_image(img)["zlib"], *img.shape)


# ---- the named inputs of the tests ------------------------------------------------------------------------------------------------
KINDS = ("smooth", "noise", "twolevel", "constant", "ramp")


def named_image(kind, H, W, C, seed=0):
    """uint8 (H, W, C), C-contiguous"""
    return np.ascontiguousarray(_named_image(kind, H, W, C, seed))


def _named_image(kind, H, W, C, seed):
    rng = np.random.default_rng([seed, H, W, C, KINDS.index(kind)])
    if kind in ("smooth", "twolevel"):       # a 16x-upsampled Gaussian field (bilinear), plus N(0, 3^2) / thresholded
        gh, gw = H // 16 + 2, W // 16 + 2
        g = rng.normal(0.0, 1.0, (gh, gw, C))
        y, x = np.arange(H) / 16.0, np.arange(W) / 16.0
        y0, x0 = y.astype(int), x.astype(int)
        fy, fx = (y - y0)[:, None, None], (x - x0)[None, :, None]
        f = (g[y0][:, x0] * (1 - fy) * (1 - fx) + g[y0 + 1][:, x0] * fy * (1 - fx) + g[y0][:, x0 + 1] * (1 - fy) * fx
             + g[y0 + 1][:, x0 + 1] * fy * fx)
        if kind == "twolevel":
            return np.where(f > 0, 255, 0).astype(np.uint8)
        return np.clip(np.rint(128 + 48 * f + rng.normal(0.0, 3.0, (H, W, C))), 0, 255).astype(np.uint8)
    if kind == "noise":
        return rng.integers(0, 256, (H, W, C), dtype=np.uint8)
    if kind == "constant":
        return np.full((H, W, C), 77, dtype=np.uint8)
    if kind == "ramp":
        return np.broadcast_to((np.arange(W) * 255 // max(W - 1, 1)).astype(np.uint8)[None, :, None], (H, W, C)).copy()
    raise ValueError(kind)


def size_cap(filtered, nseg):
    """the issue's cap on the IDAT length: 1.01 x zlib level 6 with Z_RLE on the same filtered bytes + 291 bytes per segment"""
    c = zlib.compressobj(6, zlib.DEFLATED, 15, 8, zlib.Z_RLE)
    ref = len(c.compress(np.asarray(filtered, dtype=np.uint8).tobytes()) + c.flush())
    return 1.01 * ref + 291 * nseg, ref


def check_image(img, enc, png):
    """the assertions every encoding of `img` has to meet (shared with the GPU tests)"""
    import io

    from PIL import Image
    H, W, C = img.shape
    filt = enc["filtered"]
    assert zlib.decompress(enc["zlib"]) == filt.tobytes()
    got = np.asarray(Image.open(io.BytesIO(png)))
    assert got.shape == ((H, W, 3) if C == 3 else (H, W)) and np.array_equal(got.reshape(H, W, C), img)
    assert int.from_bytes(enc["zlib"][-4:], "big") == zlib.adler32(filt.tobytes())
    nseg = (H + ROWS - 1) // ROWS
    assert len(enc["segments"]) == nseg
    for k, s in enumerate(enc["segments"]):
        assert len(s) <= segment_bound(min(ROWS, H - k * ROWS), W, C)
    cap, ref = size_cap(filt, nseg)
    return len(enc["zlib"]), cap, ref
