"""NumPy int64 restatement of the colour fix for restored faces: the oracle of vsp_color_fix_u8 (csrc/color_fix.hip) and of
`python -m vspbfr_amd.restore_photos --color_fix`.  It imports nothing from the package; validity comes from tests/photo_ref.py's tables.

    validity   crop pixel (x, y) is valid iff 0 <= (cx[y] + ax[x]) >> 10 < w and 0 <= (cy[y] + bx[x]) >> 10 < h  (M: crop -> photo)
    wavelet    d = valid ? (c - r) 64 : 0;  per level l, s = 2^l, indices clamped: d = (d[x-s] + 2 d[x] + d[x+s] + 2) >> 2 along x over the
               whole plane, then along y;  out = clamp(r + ((d + 32) >> 6), 0, 255)
    stats      over the N valid pixels, per channel: vc = ((N S2c - S1c^2) 256) // N^2, vr likewise,
               g = clamp(isqrt((vc << 24) // max(vr, 1)), 1024, 16384), mc = (S1c 256 + N // 2) // N, mr likewise,
               out = clamp((g (r 256 - mr) + mc 4096 + 2^19) >> 20, 0, 255);  N = 0: out = r
"""
import math

import numpy as np

import photo_ref as R


def validity(M, S, w, h):
    """bool (S, S): the centre cell of each crop pixel lies inside the (h, w) photo; M (2 x 3 float64) takes crop to photo"""
    ax, bx, cx, cy = R.tables(M, np.arange(S), np.arange(S))
    ix, iy = (cx[:, None] + ax[None, :]) >> 10, (cy[:, None] + bx[None, :]) >> 10
    return (ix >= 0) & (ix < w) & (iy >= 0) & (iy < h)


def validity_from_landmarks(pts5, S, w, h):
    return validity(R.invert(R.similarity(pts5, S)), S, w, h)


def _blur(d, s, axis):
    n = d.shape[axis]
    idx = np.arange(n)
    lo, hi = np.clip(idx - s, 0, n - 1), np.clip(idx + s, 0, n - 1)
    return (np.take(d, lo, axis=axis) + 2 * d + np.take(d, hi, axis=axis) + 2) >> 2


def wavelet_planes(c, r, valid=None, levels=5):
    """the Q6 difference plane after `levels` levels, int64 (S, S, 3)"""
    c, r = np.asarray(c).astype(np.int64), np.asarray(r).astype(np.int64)
    d = (c - r) * 64
    if valid is not None:
        d = np.where(np.asarray(valid, dtype=bool)[..., None], d, 0)
    for l in range(levels):
        d = _blur(d, 1 << l, 1)
        d = _blur(d, 1 << l, 0)
        assert np.abs(d).max(initial=0) <= 16320
    return d


def wavelet(c, r, valid=None, levels=5):
    """uint8 (S, S, 3)"""
    assert 1 <= levels <= 6
    d = wavelet_planes(c, r, valid, levels)
    return np.clip(np.asarray(r).astype(np.int64) + ((d + 32) >> 6), 0, 255).astype(np.uint8)


def stats_constants(c, r, valid=None):
    """[(N, g, mc, mr)] per channel, Python integers"""
    c, r = np.asarray(c).astype(np.int64), np.asarray(r).astype(np.int64)
    m = np.ones(c.shape[:2], dtype=bool) if valid is None else np.asarray(valid, dtype=bool)
    N = int(m.sum())
    out = []
    for ch in range(3):
        if N == 0:
            out.append((0, 4096, 0, 0))
            continue
        cv, rv = c[..., ch][m], r[..., ch][m]
        S1c, S2c, S1r, S2r = int(cv.sum()), int((cv * cv).sum()), int(rv.sum()), int((rv * rv).sum())
        Vc, Vr = N * S2c - S1c * S1c, N * S2r - S1r * S1r
        assert 0 <= Vc * 256 < 1 << 63 and 0 <= Vr * 256 < 1 << 63 and N * max(S2c, S2r) < 1 << 63          # int64 suffices
        vc, vr = (Vc * 256) // (N * N), (Vr * 256) // (N * N)
        g = min(max(math.isqrt((vc << 24) // max(vr, 1)), 1024), 16384)
        out.append((N, g, (S1c * 256 + N // 2) // N, (S1r * 256 + N // 2) // N))
    return out


def stats(c, r, valid=None):
    """uint8 (S, S, 3)"""
    r = np.asarray(r)
    out = np.empty_like(r, dtype=np.uint8)
    for ch, (N, g, mc, mr) in enumerate(stats_constants(c, r, valid)):
        if N == 0:
            out[..., ch] = r[..., ch]
            continue
        v = (g * (r[..., ch].astype(np.int64) * 256 - mr) + mc * 4096 + (1 << 19)) >> 20
        out[..., ch] = np.clip(v, 0, 255).astype(np.uint8)
    return out


def fix(c, r, mode, valid=None, levels=5):
    """one face, uint8 (S, S, 3) crop and restored crop -> the fixed crop"""
    if mode == "wavelet":
        return wavelet(c, r, valid, levels)
    if mode == "stats":
        return stats(c, r, valid)
    raise ValueError(mode)


def fix_batch(crops, restored, mode, valids=None, levels=5):
    """(F, S, S, 3) -> (F, S, S, 3); valids: None or one (S, S) bool array (or None) per face"""
    return np.stack([fix(crops[i], restored[i], mode, None if valids is None else valids[i], levels) for i in range(len(crops))])


def toned_pair(F, S, seed):
    """(crops, restored), uint8 (F, S, S, 3): random bytes, the restored one the crop plus fresh noise and a smooth tone shift that
    differs per face and channel -- so that both fixes move most bytes"""
    rng = np.random.default_rng(seed)
    c = rng.integers(0, 256, (F, S, S, 3)).astype(np.int64)
    yy, xx = np.mgrid[0:S, 0:S].astype(np.float64) / max(S - 1, 1)
    shift = np.stack([[(20 + 9 * ch + 5 * f) * np.cos(2.0 * xx + f) + (15 - 6 * ch) * yy - 10 for ch in range(3)] for f in range(F)])
    gain = 0.6 + 0.15 * np.arange(3)[None, :, None, None] + 0.05 * np.arange(F)[:, None, None, None]
    r = 128 + gain * (c.transpose(0, 3, 1, 2) - 128) + shift + rng.normal(0, 6, (F, 3, S, S))
    return c.astype(np.uint8), np.clip(np.rint(r), 0, 255).astype(np.uint8).transpose(0, 2, 3, 1).copy()
