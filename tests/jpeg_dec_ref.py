"""Host restatement of the device JPEG decoder (csrc/jpeg_decode.hip, vspbfr_amd/jpeg.py) in NumPy / plain Python, without importing the
package: the marker parser, the unstuffing pass, a serial entropy decoder, the subsequence / round scheme emulated for a given
sub_bytes, DC prediction, dequantisation, the ISLOW inverse DCT, fancy h2v2 upsampling and the colour transform.  `decode` returns
Pillow's `Image.open(f).convert("RGB")` pixels for a file the parser accepts, the status word the kernels report, the round count and
counters of what the scan exercised."""
import functools
import io

import numpy as np

import jpeg_ref as E

ZIGZAG = E.ZIGZAG

NO_EOI, STRAY_MARKER, RST_ORDER, RST_COUNT, BAD_CODE, BAD_CATEGORY, RUN, BLOCK_COUNT, COEF_RANGE = 1, 2, 4, 8, 16, 32, 64, 128, 256
COEF_LIMIT = 16383


class Refused(Exception):
    """a file the device path hands to the host decoder; str() is the reason"""


# ------------------------------------------------------------------------------------------------------------------------ parse
def _scan_end(data, off):
    """index (from `off`) of the first marker inside the entropy data that is not RSTm, a stuffed FF or a fill FF; None without one"""
    a = np.frombuffer(data, dtype=np.uint8, offset=off)
    if a.size < 2:
        return None
    nx = a[1:]
    hit = np.flatnonzero((a[:-1] == 0xFF) & (nx != 0) & (nx != 0xFF) & ((nx & 0xF8) != 0xD0))
    return int(hit[0]) if hit.size else None


def parse(data):
    """the markers in front of the scan -> dict(h, w, sub, restart, qt (3, 64) natural order, dc / ac [(bits, vals)] x 3, off, length);
    raises Refused with the reason for a file the device does not serve"""
    data = bytes(data)
    if data[:2] != b"\xFF\xD8":
        raise Refused("no SOI")
    qts, huff, pos, restart, frame = {}, {}, 2, 0, None
    while True:
        if pos + 4 > len(data):
            raise Refused("no SOS before the end of the file")
        if data[pos] != 0xFF:
            raise Refused(f"byte {pos}: expected a marker")
        while pos < len(data) and data[pos] == 0xFF:
            pos += 1
        code = data[pos]
        pos += 1
        if code == 0x01 or 0xD0 <= code <= 0xD7:
            continue
        if code == 0xD9:
            raise Refused("EOI before SOS")
        n = int.from_bytes(data[pos:pos + 2], "big")
        seg = data[pos + 2:pos + n]
        if n < 2 or pos + n > len(data):
            raise Refused("a segment runs past the end of the file")
        pos += n
        if code == 0xEE and seg[:5] == b"Adobe":
            raise Refused("Adobe APP14 (RGB, CMYK or YCCK coding)")
        if code == 0xDB:
            i = 0
            while i < len(seg):
                pq, tq = seg[i] >> 4, seg[i] & 15
                if pq:
                    raise Refused("16-bit quantisation table")
                nat = np.zeros(64, dtype=np.int64)
                nat[ZIGZAG] = np.frombuffer(seg[i + 1:i + 65], dtype=np.uint8)
                qts[tq] = nat
                i += 65
        elif code == 0xC4:
            i = 0
            while i < len(seg):
                bits = list(seg[i + 1:i + 17])
                huff[seg[i]] = (bits, list(seg[i + 17:i + 17 + sum(bits)]))
                i += 17 + sum(bits)
        elif code == 0xC0:
            frame = seg
        elif code in (0xC1, 0xC2, 0xC3, 0xC5, 0xC6, 0xC7, 0xC9, 0xCA, 0xCB, 0xCD, 0xCE, 0xCF, 0xCC):
            raise Refused({0xC1: "extended sequential (SOF1)", 0xC2: "progressive (SOF2)"}.get(code, f"SOF / DAC marker {code:02X}: lossless, hierarchical or arithmetic coding"))
        elif code == 0xDD:
            restart = int.from_bytes(seg[:2], "big")
        elif code == 0xDC:
            raise Refused("DNL")
        elif code == 0xDA:
            break
    if frame is None:
        raise Refused("SOS before SOF")
    if frame[0] != 8:
        raise Refused(f"{frame[0]}-bit samples")
    h, w, nf = int.from_bytes(frame[1:3], "big"), int.from_bytes(frame[3:5], "big"), frame[5]
    if h == 0 or w == 0:
        raise Refused("a side of 0 (DNL)")
    if nf == 1:
        raise Refused("greyscale")
    if nf != 3:
        raise Refused(f"{nf} components (CMYK / YCCK)")
    comps = [(frame[6 + 3 * i], frame[7 + 3 * i] >> 4, frame[7 + 3 * i] & 15, frame[8 + 3 * i]) for i in range(3)]
    if [c[0] for c in comps] != [1, 2, 3]:
        raise Refused("component ids other than 1, 2, 3 (RGB-coded)")
    samp = [(c[1], c[2]) for c in comps]
    if samp == [(1, 1)] * 3:
        sub = 0
    elif samp == [(2, 2), (1, 1), (1, 1)]:
        sub = 2
    else:
        raise Refused("sampling factors %s (4:2:2, 4:4:0, ...)" % samp)
    if seg[0] != 3 or len(seg) != 10:
        raise Refused("a scan of %d components (several scans)" % seg[0])
    if [seg[1], seg[3], seg[5]] != [1, 2, 3] or tuple(seg[7:10]) != (0, 63, 0):
        raise Refused("scan parameters of a progressive or reordered scan")
    dc, ac, qt = [], [], []
    for i in range(3):
        td, ta = seg[2 + 2 * i] >> 4, seg[2 + 2 * i] & 15
        if td not in huff or (0x10 | ta) not in huff or comps[i][3] not in qts:
            raise Refused("a table the scan selects is missing")
        dc.append(huff[td]), ac.append(huff[0x10 | ta]), qt.append(qts[comps[i][3]])
    for bits, vals in dc + ac:
        code = 0
        for length in range(1, 17):
            code += bits[length - 1]
            if code > 1 << length:
                raise Refused("a Huffman table overfills the code space")
            if code == 1 << length:
                raise Refused("a Huffman table that uses the all-ones code")
            code <<= 1
        if len(vals) != sum(bits) or sum(bits) > 256:
            raise Refused("a Huffman table that is cut short")
    end = _scan_end(data, pos)
    if end is not None and data[pos + end + 1] != 0xD9:
        raise Refused("marker %02X behind the scan (several scans, DNL)" % data[pos + end + 1])
    if len(data) - pos < 1:
        raise Refused("no entropy-coded data")
    return dict(h=h, w=w, sub=sub, restart=restart, qt=np.stack(qt), dc=dc, ac=ac, off=pos, length=len(data) - pos)


def geometry(h, w, sub, restart):
    m, bpm = (16, 6) if sub == 2 else (8, 3)
    mw, mh = -(-w // m), -(-h // m)
    nint = -(-(mw * mh) // restart) if restart else 1
    return dict(m=m, bpm=bpm, mw=mw, mh=mh, mcus=mw * mh, nint=nint)


# ---------------------------------------------------------------------------------------------------------------------- unstuff
def unstuff(data, nint):
    """entropy data (bytes to the end of the file) -> ([clean bytes of interval 0 .. nint - 1], status)"""
    a = np.frombuffer(bytes(data), dtype=np.uint8).astype(np.int64)
    n, status = a.size, 0
    end = _scan_end(bytes(data), 0)
    if end is None:
        end, status = n, status | NO_EOI
    elif a[end + 1] != 0xD9:
        status |= STRAY_MARKER
    prev = np.concatenate([[0], a[:-1]])
    nxt = np.concatenate([a[1:], [0xD9]])
    inside = np.arange(n) < end
    keep = inside & np.where(a == 0xFF, nxt == 0, prev != 0xFF)
    mark = inside & (a == 0xFF) & ((nxt & 0xF8) == 0xD0)
    clean = a[keep].astype(np.uint8).tobytes()
    at = np.cumsum(keep) - keep                      # clean bytes in front of each position
    starts = [0]
    for k, p in enumerate(np.flatnonzero(mark)):
        if (int(nxt[p]) & 7) != (k & 7):
            status |= RST_ORDER
        if k + 1 < nint:
            starts.append(int(at[p]))
    if int(mark.sum()) != nint - 1:
        status |= RST_COUNT
    starts += [len(clean)] * (nint + 1 - len(starts))
    return [clean[starts[i]:starts[i + 1]] for i in range(nint)], status


# --------------------------------------------------------------------------------------------------------------- entropy decode
@functools.lru_cache(maxsize=64)
def _lookup(bits, vals):
    """16-bit prefix -> length << 8 | symbol (0: no code has this prefix)"""
    t = np.zeros(65536, dtype=np.int32)
    code, k = 0, 0
    for length in range(1, 17):
        for _ in range(bits[length - 1]):
            t[code << (16 - length):(code + 1) << (16 - length)] = length << 8 | vals[k]
            code, k = code + 1, k + 1
        code <<= 1
    return t.tolist()


class Scan:
    """one interval's clean bytes + the tables: decode_sub mirrors the kernel's symbol loop"""

    def __init__(self, clean, hdr):
        self.len = len(clean)
        self.buf = bytes(clean) + b"\xFF" * 16
        self.bpm = 6 if hdr["sub"] == 2 else 3
        comp = [0, 0, 0, 0, 1, 2] if self.bpm == 6 else [0, 1, 2]
        dc = [_lookup(tuple(b), tuple(v)) for b, v in hdr["dc"]]
        ac = [_lookup(tuple(b), tuple(v)) for b, v in hdr["ac"]]
        self.tables = [(dc[c], ac[c]) for c in comp]
        self.seen = dict(zrl=0, dc_cat=0, ac_cat=0, code16=0, straddle=0)

    def peek(self, pos, n):
        """n <= 32 bits at bit `pos`; bits past the interval read as 1"""
        if pos >= self.len * 8:
            return (1 << n) - 1
        b = pos >> 3
        return (int.from_bytes(self.buf[b:b + 5], "big") >> (40 - (pos & 7) - n)) & ((1 << n) - 1)

    def decode_sub(self, pos, state, end_bit, last, store=None, blk=0, blk_end=0):
        """-> (pos, state, blocks completed, err); store: dict block -> 64 ints (natural order), filled for blk < blk_end"""
        b, k, nblk, err = state >> 8, state & 255, 0, 0
        seen = self.seen if store is not None else None
        while pos < end_bit:
            left = end_bit - pos
            if last and b == 0 and k == 0 and left < 8 and self.peek(pos, left) == (1 << left) - 1:
                pos = end_bit
                break
            e = self.tables[b][1 if k else 0][self.peek(pos, 16)]
            if e == 0:
                err |= BAD_CODE
                pos += 1
                continue
            clen, sym = e >> 8, e & 255
            s, r = sym & 15, sym >> 4
            raw = self.peek(pos + clen, s) if s else 0
            if seen is not None:
                seen["code16"] += clen == 16
                seen["straddle"] += pos < end_bit < pos + clen + s
            pos += clen + s
            value = raw - (1 << s) + 1 if s and raw < (1 << (s - 1)) else raw
            if k == 0:
                if sym > 11:
                    err |= BAD_CATEGORY
                if store is not None and blk < blk_end:
                    store.setdefault(blk, [0] * 64)[0] = value
                    seen["dc_cat"] = max(seen["dc_cat"], s)
                k = 1
            elif s == 0:
                if r == 15:
                    k += 16
                    if seen is not None:
                        seen["zrl"] += 1
                    if k > 63:
                        err |= RUN
                        k = 64
                else:
                    if r:
                        err |= RUN
                    k = 64
            else:
                if s > 10:
                    err |= BAD_CATEGORY
                k += r
                if k > 63:
                    err |= RUN
                    k = 64
                else:
                    if store is not None and blk < blk_end:
                        store.setdefault(blk, [0] * 64)[int(ZIGZAG[k])] = value
                        seen["ac_cat"] = max(seen["ac_cat"], s)
                    k += 1
            if k >= 64:
                k, b = 0, (b + 1) % self.bpm
                nblk += 1
                blk += 1
        return pos, b << 8 | k, nblk, err


def decode_interval_serial(scan, blk0, blk_end, store):
    """the whole interval from its first bit -> status bits"""
    pos, state, nblk, err = scan.decode_sub(0, 0, scan.len * 8, True, store, blk0, blk_end)
    if blk0 + nblk != blk_end or state != 0 or pos != scan.len * 8:
        err |= BLOCK_COUNT
    return err


def decode_interval_parallel(scan, sb, blk0, blk_end, store, stats):
    """the kernel's scheme: round 0 from (first bit, state 0), later rounds from the neighbour's exit of the round before, then the true
    pass -> (status bits, rounds)"""
    n = scan.len
    nsub = -(-n // sb)
    if nsub == 0:
        return BLOCK_COUNT, 0
    ends = [min((i + 1) * sb, n) * 8 for i in range(nsub)]
    ex = [scan.decode_sub(i * sb * 8, 0, ends[i], i == nsub - 1)[:3] for i in range(nsub)]
    first = list(ex)
    chg, rounds = [True] * nsub, 1
    while nsub > 1 and rounds <= nsub:
        new, nchg = list(ex), [False] * nsub
        for i in range(1, nsub):
            if chg[i - 1]:
                new[i] = scan.decode_sub(ex[i - 1][0], ex[i - 1][1], ends[i], i == nsub - 1)[:3]
                nchg[i] = new[i] != ex[i]
        ex, chg, rounds = new, nchg, rounds + 1
        if not any(chg):
            break
    err, blk = 0, blk0
    for i in range(nsub):
        pos, state = ex[i - 1][:2] if i else (0, 0)
        e = scan.decode_sub(pos, state, ends[i], i == nsub - 1, store, blk, blk_end)
        assert e[:3] == ex[i]
        blk += e[2]
        err |= e[3]
        stats["max_blocks_in_sub"] = max(stats["max_blocks_in_sub"], e[2])
        stats["wrong_round0"] += first[i] != ex[i]
        if i and scan.buf[i * sb - 1] == 0xFF and i * sb <= n:
            stats["ff_last_byte"] += 1
    if blk != blk_end or ex[-1][1] != 0 or ex[-1][0] != n * 8:
        err |= BLOCK_COUNT
    stats["max_subs"] = max(stats["max_subs"], nsub)
    stats["max_rounds"] = max(stats["max_rounds"], rounds)
    # a block that spans three or more subsequences: subsequence i starts inside a block and completes none
    for i in range(1, nsub - 1):
        if ex[i][2] == 0 and ex[i - 1][1] & 255 and ex[i - 1][0] < ends[i]:
            stats["block_spans3"] += 1
    return err, rounds


def decode_coefficients(data, hdr, sub_bytes=None):
    """-> (coef (blocks, 64) int64 natural order with DC still a difference, status, rounds, stats); sub_bytes None: the serial decoder"""
    g = geometry(hdr["h"], hdr["w"], hdr["sub"], hdr["restart"])
    pieces, status = unstuff(data[hdr["off"]:], g["nint"])
    nblocks = g["mcus"] * g["bpm"]
    store, rounds = {}, 0
    stats = dict(max_blocks_in_sub=0, wrong_round0=0, ff_last_byte=0, max_subs=0, max_rounds=0, block_spans3=0, zrl=0, dc_cat=0, ac_cat=0,
                 code16=0, straddle=0, intervals=g["nint"], last_interval_mcus=g["mcus"] - (g["nint"] - 1) * (hdr["restart"] or g["mcus"]))
    for i, clean in enumerate(pieces):
        scan = Scan(clean, hdr)
        m0 = i * hdr["restart"]
        mcus_in = min(hdr["restart"], g["mcus"] - m0) if hdr["restart"] else g["mcus"]
        blk0, blk_end = m0 * g["bpm"], (m0 + mcus_in) * g["bpm"]
        if sub_bytes is None:
            status |= decode_interval_serial(scan, blk0, blk_end, store)
        else:
            err, r = decode_interval_parallel(scan, sub_bytes, blk0, blk_end, store, stats)
            status, rounds = status | err, max(rounds, r)
        for key in ("zrl", "code16", "straddle"):
            stats[key] += scan.seen[key]
        for key in ("dc_cat", "ac_cat"):
            stats[key] = max(stats[key], scan.seen[key])
    coef = np.zeros((nblocks, 64), dtype=np.int64)
    for blk, row in store.items():
        coef[blk] = row
    coef = ((coef + 32768) & 65535) - 32768          # the kernel stores int16
    return coef, status, rounds, stats


# ----------------------------------------------------------------------------------------------------------------------- pixels
def _descale(x, n):
    return (x + (1 << (n - 1))) >> n


def _idct_pass(d, pass2):
    """ISLOW inverse DCT along the last axis (jidctint.c); pass 2 descales by 18 and applies the range limit"""
    x = [d[..., i] for i in range(8)]
    z1 = (x[2] + x[6]) * 4433
    t2, t3 = z1 - x[6] * 15137, z1 + x[2] * 6270
    t0, t1 = (x[0] + x[4]) << 13, (x[0] - x[4]) << 13
    t10, t13, t11, t12 = t0 + t3, t0 - t3, t1 + t2, t1 - t2
    o0, o1, o2, o3 = x[7], x[5], x[3], x[1]
    z5 = (o0 + o1 + o2 + o3) * 9633
    y1, y2 = -(o0 + o3) * 7373, -(o1 + o2) * 20995
    y3, y4 = -(o0 + o2) * 16069 + z5, -(o1 + o3) * 3196 + z5
    o0, o1, o2, o3 = o0 * 2446 + y1 + y3, o1 * 16819 + y2 + y4, o2 * 25172 + y2 + y3, o3 * 12299 + y1 + y4
    sh = 18 if pass2 else 11
    r = np.stack([_descale(v, sh) for v in (t10 + o3, t11 + o2, t12 + o1, t13 + o0, t13 - o0, t12 - o1, t11 - o2, t10 - o3)], axis=-1)
    if pass2:
        i = r & 1023
        r = np.where(i < 128, i + 128, np.where(i < 512, 255, np.where(i < 896, 0, i - 896)))
    return r


def pixels(coef, hdr):
    """coefficients (DC as differences) -> ((h, w, 3) uint8, status bits of the pixel path)"""
    h, w, sub, restart = hdr["h"], hdr["w"], hdr["sub"], hdr["restart"]
    g = geometry(h, w, sub, restart)
    bpm, mcus = g["bpm"], g["mcus"]
    comp = np.array([0, 0, 0, 0, 1, 2] if bpm == 6 else [0, 1, 2])
    c = coef.reshape(mcus, bpm, 64).copy()
    per = restart or mcus
    for k in range(3):                                # DC prediction per component, restarted at every interval
        idx = np.flatnonzero(comp == k)
        d = c[:, idx, 0].reshape(-1)
        seg = np.repeat(np.arange(mcus) // per, len(idx))
        run = np.cumsum(d)
        first = np.flatnonzero(np.r_[True, seg[1:] != seg[:-1]])
        base = np.repeat((run - d)[first], np.diff(np.r_[first, d.size]))
        c[:, idx, 0] = (((run - base + 32768) & 65535) - 32768).reshape(mcus, len(idx))
    deq = c * hdr["qt"][comp][None, :, :]
    status = COEF_RANGE if np.abs(deq).max(initial=0) > COEF_LIMIT else 0
    b = deq.reshape(mcus, bpm, 8, 8)
    b = _idct_pass(b.swapaxes(-1, -2), False).swapaxes(-1, -2)        # columns
    b = _idct_pass(b, True)                                           # rows
    b = b.reshape(g["mh"], g["mw"], bpm, 8, 8)
    ph, pw = g["mh"] * g["m"], g["mw"] * g["m"]
    if bpm == 3:
        pl = [b[:, :, k].transpose(0, 2, 1, 3).reshape(ph, pw)[:h, :w] for k in range(3)]
        Y, Cb, Cr = pl
    else:
        Y = b[:, :, :4].reshape(g["mh"], g["mw"], 2, 2, 8, 8).transpose(0, 2, 4, 1, 3, 5).reshape(ph, pw)[:h, :w]
        ch, cw = (h + 1) // 2, (w + 1) // 2
        ys, xs = np.arange(h), np.arange(w)
        cy, cx = ys >> 1, xs >> 1
        cn = np.where(ys & 1, np.minimum(cy + 1, ch - 1), np.maximum(cy - 1, 0))
        nx = np.where(xs & 1, np.minimum(cx + 1, cw - 1), np.maximum(cx - 1, 0))
        up = []
        for k in (4, 5):
            C = b[:, :, k].transpose(0, 2, 1, 3).reshape(ph // 2, pw // 2)
            if cw <= 2:                                               # jdsample.c: no fancy filter for one or two chroma columns
                up.append(C[cy][:, cx])
                continue
            col = 3 * C[cy] + C[cn]                                   # (h, chroma columns)
            up.append((3 * col[:, cx] + col[:, nx] + np.where(xs & 1, 7, 8)[None, :]) >> 4)
        Cb, Cr = up
    cb, cr = Cb - 128, Cr - 128
    R = Y + ((91881 * cr + 32768) >> 16)
    G = Y + ((-22554 * cb + 32768 - 46802 * cr) >> 16)
    B = Y + ((116130 * cb + 32768) >> 16)
    return np.clip(np.stack([R, G, B], axis=-1), 0, 255).astype(np.uint8), status


@functools.lru_cache(maxsize=None)
def decode(data, sub_bytes=None):
    """file bytes -> dict(pixels, status, rounds, stats, header); raises Refused"""
    hdr = parse(data)
    coef, status, rounds, stats = decode_coefficients(data, hdr, sub_bytes)
    px, more = pixels(coef, hdr)
    return dict(pixels=px, coef=coef, status=status | more, rounds=rounds, stats=stats, header=hdr)


def pillow_pixels(data):
    from PIL import Image
    return np.asarray(Image.open(io.BytesIO(data)).convert("RGB"), dtype=np.uint8)


# ------------------------------------------------------------------------------------------------------------------- test files
CUSTOM_QT = [[(3 + (7 * i) % 29) for i in range(64)], [(5 + (11 * i) % 61) for i in range(64)]]      # zig-zag order, as Pillow takes them


@functools.lru_cache(maxsize=None)
def make_file(kind, h, w, quality, sub, restart, optimize=False, custom_qt=False, seed=0):
    """Pillow's JPEG of jpeg_ref.named_image; restart in MCUs (0 = none; -1 = one MCU row)"""
    from PIL import Image
    img = E.named_image(kind, h, w, seed)
    m = 16 if sub == "420" else 8
    kw = dict(format="JPEG", quality=quality, subsampling=E.SUB[sub], optimize=optimize)
    if restart:
        kw["restart_marker_blocks"] = -(-w // m) if restart < 0 else restart
    if custom_qt:
        kw["qtables"] = CUSTOM_QT
    buf = io.BytesIO()
    from PIL import ImageFile
    keep = ImageFile.MAXBLOCK                        # an optimised file is written in one piece: Pillow's buffer must hold it
    ImageFile.MAXBLOCK = max(keep, 6 * h * w + 65536)
    try:
        Image.fromarray(img).save(buf, **kw)
    finally:
        ImageFile.MAXBLOCK = keep
    return buf.getvalue()


def noisy_padding_file(h=33, w=17, quality=90, seed=5):
    """a 4:2:0 file whose padding blocks and padding samples are not replicas of the edge: the blocks of a LARGER noise image, framed
    with the smaller size (jpeg_ref.encode_scan / frame write what Pillow will not)"""
    ph, pw = -(-h // 16) * 16, -(-w // 16) * 16
    big = E.named_image("noise", ph, pw, seed)
    blocks, comps = E.mcu_blocks(big, quality, 2)
    restart = blocks.shape[0]
    seg, _, _ = E.encode_scan(blocks, comps, restart)
    return E.frame(seg, h, w, quality, 2, restart)


SIZES = [(1, 1), (8, 8), (16, 16), (33, 17), (37, 53), (96, 96), (1100, 37), (200, 260)]      # (h, w): 17 x 33 ... as width x height
KINDS = ("noise", "flat128", "ramp", "sparse", "blocks")
QUALITIES = (1, 50, 90, 95, 100)
RESTARTS = (0, 1, 3, 8, -1)


def thinned_cases():
    """(kind, h, w, quality, sub, restart, optimize, custom_qt): a diagonal walk with coprime strides in which every value of every list
    appears, plus the cases the coverage conditions need"""
    cases = []
    for i in range(24):
        h, w = SIZES[i % len(SIZES)]
        kind = KINDS[(2 * i + 1) % len(KINDS)]
        q = QUALITIES[(3 * i + 2) % len(QUALITIES)]
        if h * w > 20000 and kind == "noise":
            q = min(q, 50)                           # the large sizes stay cheap for the Python restatement
        cases.append((kind, h, w, q, ("420", "444")[(i + i // 3) % 2], RESTARTS[(i + i // 5) % len(RESTARTS)], i % 3 == 1, i % 4 == 2))
    cases += [("noise", 96, 96, 100, "444", 0, False, False),      # more than 1024 subsequences at sub_bytes 16, 16-bit codes
              ("blocks", 37, 53, 100, "444", 0, False, False),     # DC category 11, AC category 10
              ("blocks", 37, 53, 100, "420", 3, True, False),
              ("sparse", 96, 96, 90, "420", 0, False, False),      # ZRL; many blocks per subsequence
              ("flat128", 200, 260, 90, "420", 0, False, False),   # more than 16 whole blocks in a subsequence
              ("noise", 33, 17, 100, "420", 1, False, False),      # RSTm wraps past 7
              ("noise", 37, 53, 95, "420", 8, True, True),         # a short last interval
              ("noise", 16, 2, 90, "420", 0, False, False),        # at most two chroma columns: replication, not the fancy filter
              ("noise", 16, 3, 90, "420", 0, False, False), ("noise", 16, 4, 90, "420", 1, False, False),
              ("noise", 16, 5, 90, "420", 0, False, False), ("noise", 40, 1, 90, "420", 0, False, False),
              ("ramp", 3, 4, 90, "420", 0, True, False), ("noise", 16, 4, 90, "444", 0, False, False)]
    return cases


def corrupt_files():
    """[(name, file)]: scans a decoder must report, not trust -- cut short; a byte range overwritten with noise (no FF: the damage
    stays inside the entropy coding); a stray marker in the middle; one RSTm taken out"""
    good = make_file("noise", 37, 53, 90, "420", 3)
    off = parse(good)["off"]
    mid = off + (len(good) - off) // 2
    rng = np.random.RandomState(7)
    noise = bytearray(good)
    noise[mid:mid + 40] = rng.randint(0, 255, 40).astype(np.uint8).tobytes()
    if noise[mid - 1] == 0xFF:
        noise[mid] = 0
    rst = good.index(b"\xFF\xD1", off)
    return [("truncated", good[:mid]), ("noise", bytes(noise)), ("stray_marker", good[:mid] + b"\xFF\xC4" + good[mid:]),
            ("rst_missing", good[:rst] + good[rst + 2:])]


def corrupt_header():
    """the header the corrupt files share (their own parse may refuse them: the stray marker ends the scan early)"""
    return parse(make_file("noise", 37, 53, 90, "420", 3))


def refused_files():
    """[(name, file, word the reason holds)]: files the parser hands to the host"""
    from PIL import Image
    img = E.named_image("ramp", 24, 40)

    def save(im, **kw):
        buf = io.BytesIO()
        im.save(buf, format="JPEG", **kw)
        return buf.getvalue()

    good = save(Image.fromarray(img), quality=90, subsampling=2)
    sof = good.index(b"\xFF\xC0")
    dqt = good.index(b"\xFF\xDB")
    wide = good[:dqt] + b"\xFF\xDB" + (131).to_bytes(2, "big") + b"\x10" + bytes(128) + good[dqt:]
    adobe = good[:sof] + b"\xFF\xEE\x00\x0EAdobe\x00\x64\x00\x00\x00\x00\x00" + good[sof:]
    sos = good.index(b"\xFF\xDA")
    two = good[:-2] + good[sos:]
    return [("progressive", save(Image.fromarray(img), progressive=True), "progressive"),
            ("422", save(Image.fromarray(img), subsampling=1), "sampling"),
            ("greyscale", save(Image.fromarray(img[..., 0])), "greyscale"),
            ("cmyk", save(Image.fromarray(np.concatenate([img, img[..., :1]], axis=-1), mode="CMYK")), "Adobe"),
            ("adobe_rgb", adobe, "Adobe"), ("dqt16", wide, "16-bit"), ("two_scans", two, "several scans")]
