"""CPU checks of tests/png_ref.py, the host restatement of the device PNG encoder: zlib inflates its stream to the filtered bytes it
claims, PIL decodes the assembled file to the input, the combined Adler-32 is zlib's, no segment exceeds its bound, and the IDAT stays
under the size cap (1.01 x zlib level 6 / Z_RLE on the same filtered bytes + 291 bytes per segment)."""
import zlib

import numpy as np
import pytest

import png_ref as R

# width x height
SMALL = [(1, 1), (1, 7), (7, 1), (33, 65), (130, 67), (40, 33), (33, 40)]
CASES = [(k, w, h, c) for (w, h) in SMALL for k in R.KINDS for c in (3, 1)]
CASES += [("constant", 64, 300, 3), ("constant", 300, 64, 3), ("constant", 300, 64, 1)]
CASES += [(k, 512, 512, 3) for k in R.KINDS] + [("smooth", 512, 512, 1), ("twolevel", 512, 512, 1)]


@pytest.mark.parametrize("kind,W,H,C", CASES, ids=lambda v: str(v))
def test_restatement(kind, W, H, C):
    img = R.named_image(kind, H, W, C)
    enc = R.encode_image(img)
    size, cap, ref = R.check_image(img, enc, R.assemble(enc["zlib"], H, W, C))
    print(f"{kind} {W}x{H}x{C}: IDAT {size} zlib-RLE {ref} cap {cap:.0f} raw {enc['filtered'].size}")
    assert ref <= cap           # zlib itself is inside the cap
    assert size <= cap


def test_filter_choice_is_minimal_and_ties_go_low():
    img = R.named_image("smooth", 19, 23, 3)
    filt, types = R.filter_image(img)
    cur = img.reshape(19, -1).astype(int)
    for y in range(19):
        up = cur[y - 1] if y else np.zeros_like(cur[y])
        costs = []
        for t in range(5):
            res = []
            for x in range(cur.shape[1]):
                a = cur[y, x - 3] if x >= 3 else 0
                b, c = up[x], (up[x - 3] if x >= 3 else 0)
                p = a + b - c
                pa, pb, pc = abs(p - a), abs(p - b), abs(p - c)
                pred = (0, a, b, (a + b) // 2, a if pa <= pb and pa <= pc else (b if pb <= pc else c))[t]
                res.append((cur[y, x] - pred) & 255)
            costs.append(sum(r if r < 128 else 256 - r for r in res))
            if t == types[y]:
                assert list(filt[y, 1:]) == res
        assert types[y] == costs.index(min(costs))
    assert list(R.filter_image(np.full((3, 4, 1), 0, np.uint8))[1]) == [0, 0, 0]       # all five tie at 0


@pytest.mark.parametrize("maxbits,nsym", [(15, 286), (7, 19)])
def test_length_limit_repair_gives_complete_codes(maxbits, nsym):
    """Fibonacci-like counts force depths past the limit: the repaired lengths stay within it, satisfy Kraft with equality (zlib refuses
    an incomplete literal code) and never give a rarer symbol a shorter code."""
    for n_used in (2, 3, maxbits + 1, maxbits + 6, nsym):
        fib = [1, 1]
        while len(fib) < n_used:
            fib.append(min(fib[-1] + fib[-2], 1 << 40))
        freq = [0] * nsym
        for k, f in enumerate(fib[:n_used]):
            freq[(7 * k) % nsym if nsym == 286 else k] = f
        lens = R.code_lengths(freq, maxbits)
        used = [s for s in range(nsym) if freq[s]]
        assert all(1 <= lens[s] <= maxbits for s in used) and all(lens[s] == 0 for s in range(nsym) if not freq[s])
        assert sum(1 << (maxbits - lens[s]) for s in used) == 1 << maxbits
        order = sorted(used, key=lambda s: (freq[s], s))
        assert all(lens[a] >= lens[b] for a, b in zip(order, order[1:]))


def test_degenerate_distance_codes_and_stored_segments():
    # no match at all: one zero-length distance code; zlib accepts the block
    s = np.arange(200, dtype=np.uint8) * 7
    assert zlib.decompress(R.encode_segment(s, True), -15) == s.tobytes()
    # exactly one distance code
    s = np.zeros(600, dtype=np.uint8)
    seg = R.encode_segment(s, True)
    assert zlib.decompress(seg, -15) == s.tobytes() and len(seg) < 40
    # incompressible: the stored form, final and not
    s = R.named_image("noise", 8, 100, 3).reshape(-1)
    assert R.encode_segment(s, True) == bytes([1, 2400 & 255, 2400 >> 8, ~2400 & 255, (~2400 >> 8) & 255]) + s.tobytes()
    two = R.encode_segment(s, False) + R.encode_segment(s[:5], True)
    assert zlib.decompress(two, -15) == s.tobytes() + s[:5].tobytes()
    # runs are cut at 258 from the start of a stretch; a rest below 3 is literals
    lit, start, clen = R.tokens(np.zeros(1 + 258 + 2, dtype=np.uint8))
    assert list(np.flatnonzero(start)) == [1] and clen[1] == 258 and list(np.flatnonzero(lit)) == [0, 259, 260]
