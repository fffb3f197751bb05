"""NumPy restatement of the whole-photo face path: the float64 Umeyama similarity from five landmarks, the int32 coordinate
tables built with np.rint, the fixed-point bilinear crop and the feathered paste-back, all in int64 arithmetic.  The oracle of
vsp_face_crop_u8 / vsp_face_paste_u8 (csrc/face_warp.hip) and of `python -m vspbfr_amd.restore_photos`; it imports nothing from the package.

    M (2 x 3, destination -> source), destination column x and row y:
        ax[x] = rne(M00 x 1024)   bx[x] = rne(M10 x 1024)   cx[y] = rne((M01 y + M02) 1024) + 16   cy[y] = rne((M11 y + M12) 1024) + 16
        X = (cx[y] + ax[x]) >> 5, Y = (cy[y] + bx[x]) >> 5            Q5 source coordinates, arithmetic shifts
        ix = X >> 5, fx = X & 31, iy = Y >> 5, fy = Y & 31
        v = (sum_{i,j in {0,1}} 32 (i ? fx : 32 - fx)(j ? fy : 32 - fy) p(ix + i, iy + j) + 16384) >> 15
"""
import numpy as np

FFHQ512_TEMPLATE = np.array([[192.98138, 239.94708], [318.90277, 240.1936], [256.63416, 314.01935], [201.26117, 371.41043],
                             [313.08905, 371.15118]], dtype=np.float64)
TABLE_LIMIT = 1 << 30


def umeyama(src, dst):
    """least-squares similarity (rotation, one scale, translation; never a reflection) taking src (n, 2) to dst (n, 2): 2 x 3 float64"""
    src, dst = np.asarray(src, dtype=np.float64), np.asarray(dst, dtype=np.float64)
    n = src.shape[0]
    ms, md = src.mean(axis=0), dst.mean(axis=0)
    sc, dc = src - ms, dst - md
    var = (sc * sc).sum() / n
    if not var >= 1e-12:
        raise ValueError("degenerate landmarks")
    cov = dc.T @ sc / n
    U, D, Vt = np.linalg.svd(cov)
    sgn = np.ones(2)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:
        sgn[1] = -1.0
    R = U @ np.diag(sgn) @ Vt
    scale = (D * sgn).sum() / var
    t = md - scale * (R @ ms)
    return np.concatenate([scale * R, t[:, None]], axis=1)


def similarity(pts5, size=512):
    """A (photo -> crop) for five landmarks and the template scaled to size"""
    return umeyama(pts5, FFHQ512_TEMPLATE * (size / 512.0))


def invert(A):
    """closed-form inverse of a 2 x 3 affine map"""
    a, b, tx, c, d, ty = (float(v) for v in np.asarray(A, dtype=np.float64).reshape(-1))
    det = a * d - b * c
    return np.array([[d / det, -b / det, (b * ty - d * tx) / det], [-c / det, a / det, (c * tx - a * ty) / det]], dtype=np.float64)


def paste_matrix(A, upscale=1):
    """P (output photo -> crop) = A after a division of the output coordinates by the upscale factor"""
    P = np.array(A, dtype=np.float64)
    P[:, :2] = P[:, :2] / float(upscale)
    return P


def tables(M, xs, ys):
    """int64 (ax, bx, cx, cy) for the destination columns xs and rows ys; ValueError at a magnitude of 2^30 or more"""
    M = np.asarray(M, dtype=np.float64)
    xs, ys = np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64)
    ax = np.rint(M[0, 0] * xs * 1024.0)
    bx = np.rint(M[1, 0] * xs * 1024.0)
    cx = np.rint((M[0, 1] * ys + M[0, 2]) * 1024.0) + 16.0
    cy = np.rint((M[1, 1] * ys + M[1, 2]) * 1024.0) + 16.0
    for t in (ax, bx, cx, cy):
        if t.size and not np.all(np.abs(t) < TABLE_LIMIT):
            raise ValueError("table entry of magnitude 2^30 or more")
    return tuple(t.astype(np.int64) for t in (ax, bx, cx, cy))


def _coords(M, xs, ys):
    ax, bx, cx, cy = tables(M, xs, ys)
    return (cx[:, None] + ax[None, :]) >> 5, (cy[:, None] + bx[None, :]) >> 5


def _bilinear(img, X, Y, border=None):
    """the fixed-point bilinear value at Q5 coordinates (X, Y) of a uint8 (h, w, 3) image: taps outside read `border`, or are
    clamped to the last row / column where border is None"""
    h, w = img.shape[:2]
    ix, fx, iy, fy = X >> 5, X & 31, Y >> 5, Y & 31
    acc = np.full(X.shape + (3,), 16384, dtype=np.int64)
    for j in (0, 1):
        for i in (0, 1):
            wgt = 32 * (fx if i else 32 - fx) * (fy if j else 32 - fy)
            xx, yy = ix + i, iy + j
            if border is None:
                p = img[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(np.int64)
            else:
                inside = (xx >= 0) & (xx < w) & (yy >= 0) & (yy < h)
                p = np.where(inside[..., None], img[np.clip(yy, 0, h - 1), np.clip(xx, 0, w - 1)].astype(np.int64),
                             np.asarray(border, dtype=np.int64)[None, None, :])
            acc += wgt[..., None] * p
    return acc >> 15


def crop(photo, M, S, border=(128, 128, 128)):
    """uint8 (S, S, 3): the S x S window of `photo` seen through M (crop -> photo)"""
    photo = np.asarray(photo, dtype=np.uint8)
    X, Y = _coords(M, np.arange(S), np.arange(S))
    return _bilinear(photo, X, Y, border).astype(np.uint8)


def to_f32(u8):
    """(n, S, S, 3) uint8 -> (n, 3, S, S) fp32 (x / 255 - .5) / .5, three separately rounded fp32 operations"""
    v = np.asarray(u8).astype(np.float32)
    return np.ascontiguousarray((((v / np.float32(255.0)) - np.float32(0.5)) / np.float32(0.5)).transpose(0, 3, 1, 2))


def bbox(P, S, H, W):
    """(x0, y0, x1, y1), ends exclusive: the corners of the crop square [0, S - 1]^2 taken back through P into the (H, W) output photo,
    floor / ceil, one pixel of margin, clipped to the photo; x1 <= x0 or y1 <= y0 where nothing is left"""
    Q = invert(P)
    c = np.array([[0.0, 0.0], [S - 1.0, 0.0], [0.0, S - 1.0], [S - 1.0, S - 1.0]])
    px = Q[0, 0] * c[:, 0] + Q[0, 1] * c[:, 1] + Q[0, 2]
    py = Q[1, 0] * c[:, 0] + Q[1, 1] * c[:, 1] + Q[1, 2]
    x0, x1 = int(np.floor(px.min())) - 1, int(np.ceil(px.max())) + 2
    y0, y1 = int(np.floor(py.min())) - 1, int(np.ceil(py.max())) + 2
    return max(x0, 0), max(y0, 0), min(x1, W), min(y1, H)


def default_ramp(inset=8, feather=48):
    """uint16 raised cosine over the distance from the crop border in 1/8 px: 0 up to inset px, 256 from inset + feather px on"""
    L = 8 * (int(inset) + int(feather)) + 1
    px = np.arange(L, dtype=np.float64) / 8.0
    if feather > 0:
        t = np.clip((px - inset) / float(feather), 0.0, 1.0)
    else:
        t = (px > inset).astype(np.float64)
    r = np.rint(128.0 * (1.0 - np.cos(np.pi * t))).astype(np.uint16)
    r[0] = 0
    return r


def paste(photo, faces, S, ramp=None):
    """the output photo after pasting `faces` = [(restored crop uint8 (S, S, 3), P), ...] in list order into a copy of `photo`"""
    out = np.array(photo, dtype=np.uint8)
    H, W = out.shape[:2]
    ramp = default_ramp() if ramp is None else np.asarray(ramp)
    assert ramp[0] == 0 and ramp.max() <= 256
    L = ramp.shape[0]
    lim = (S - 1) * 32
    for restored, P in faces:
        x0, y0, x1, y1 = bbox(P, S, H, W)
        if x1 <= x0 or y1 <= y0:
            continue
        X, Y = _coords(P, np.arange(x0, x1), np.arange(y0, y1))
        d = np.minimum(np.minimum(X, Y), np.minimum(lim - X, lim - Y))
        touch = d >= 0
        w = ramp[np.minimum(np.maximum(d, 0) >> 2, L - 1)].astype(np.int64)
        f = _bilinear(np.asarray(restored, dtype=np.uint8), np.clip(X, 0, lim), np.clip(Y, 0, lim))
        bg = out[y0:y1, x0:x1].astype(np.int64)
        mixed = (w[..., None] * f + (256 - w[..., None]) * bg + 128) >> 8
        out[y0:y1, x0:x1] = np.where(touch[..., None], mixed, bg).astype(np.uint8)
    return out


def test_photo(w, h, seed):
    """uint8 (h, w, 3): a smooth colour field with noise and hard black / white bars (both ends of the byte range next to each other)"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w].astype(np.float64)
    base = np.stack([127 + 120 * np.sin(xx / 7.0 + seed), 127 + 120 * np.cos(yy / 5.0), 127 + 120 * np.sin((xx + yy) / 11.0)], axis=2)
    a = np.clip(base + rng.normal(0, 20, (h, w, 3)), 0, 255).astype(np.uint8)
    a[::7] = 255
    a[3::7] = 0
    if w >= 8:
        a[:, w // 3] = 0
        a[:, w // 3 + 1] = 255
    return a


test_photo.__test__ = False   # a helper, not a test


def landmarks_for(scale, angle_deg, centre, size=512):
    """five landmarks in a photo for a face whose crop is the photo scaled by `scale` (source px -> crop px), turned by angle_deg, with
    the template's centre of mass at `centre`: the template taken back through that similarity"""
    th = np.deg2rad(angle_deg)
    R = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    t = FFHQ512_TEMPLATE * (size / 512.0)
    m = t.mean(axis=0)
    return (t - m) @ R / scale + np.asarray(centre, dtype=np.float64)
