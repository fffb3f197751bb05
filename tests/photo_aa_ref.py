"""NumPy restatement of the anti-aliased face crop and paste-back, int64 throughout; it imports photo_ref and nothing from the
package.  The oracle of vsp_face_crop_aa_u8 / vsp_face_paste_aa_u8 and of `python -m vspbfr_amd.restore_photos --antialias`.

    F (2 x 3 float64, source -> destination; crop: A, paste: P^-1), source lattice point (qx, qy), destination pixel (x, y) absolute:
        U = rne(F00 qx 1024) + rne((F01 qy + F02) 1024)        V = rne(F10 qx 1024) + rne((F11 qy + F12) 1024)
        tu = max(0, 1024 - |U - 1024 x|)   tv = max(0, 1024 - |V - 1024 y|)   w = (tu tv) >> 8
        v_c = (sum w p_c(qx, qy) + (W >> 1)) // W,  W = sum w
    a tent one destination pixel wide, summed over every source lattice point: a point outside the image reads the border colour (crop)
    or the pixel at the clamped index (paste).  `filtered` sums over a window of reach + 2 around the bilinear centre cell -- one wider
    than the kernels', so that a tap the kernels' window dropped would show -- and `filtered_all` over every lattice point that can weigh
    anything at all, one destination pixel at a time (slow: small cases only).  A face with minification m <= 1 keeps photo_ref's four
    bilinear taps (reach 0)."""
import numpy as np

import photo_ref as R

MAX_MINIFY = 16
MAX_REACH = 23


def crop_minify(A):
    """source pixels per crop pixel"""
    return 1.0 / float(np.hypot(A[0, 0], A[1, 0]))


def paste_minify(P):
    """crop pixels per output pixel"""
    return float(np.hypot(P[0, 0], P[1, 0]))


def reach(M, m):
    """M: destination -> source"""
    return 0 if m <= 1.0 else int(np.ceil(abs(float(M[0, 0])) + abs(float(M[0, 1])) + 0.125))


def check_minify(m):
    if m > MAX_MINIFY:
        raise ValueError(f"minification {m} above {MAX_MINIFY}")


def forward(F, qx, qy):
    """(U, V) int64 of the source lattice points (qx, qy) (arrays that broadcast); ValueError at a table magnitude of 2^30 or more"""
    F = np.asarray(F, dtype=np.float64)
    qx, qy = np.asarray(qx, dtype=np.float64), np.asarray(qy, dtype=np.float64)
    parts = (np.rint(F[0, 0] * qx * 1024.0), np.rint((F[0, 1] * qy + F[0, 2]) * 1024.0), np.rint(F[1, 0] * qx * 1024.0),
             np.rint((F[1, 1] * qy + F[1, 2]) * 1024.0))
    for t in parts:
        if t.size and not np.all(np.abs(t) < R.TABLE_LIMIT):
            raise ValueError("forward table entry of magnitude 2^30 or more")
    fu, gu, fv, gv = (t.astype(np.int64) for t in parts)
    return fu + gu, fv + gv


def forward_tables(F, qxs, qys):
    """int64 (fu, fv, gu, gv) over the source columns qxs and rows qys, as the plan lays them out"""
    F = np.asarray(F, dtype=np.float64)
    qxs, qys = np.asarray(qxs, dtype=np.float64), np.asarray(qys, dtype=np.float64)
    return tuple(np.rint(v).astype(np.int64) for v in (F[0, 0] * qxs * 1024.0, F[1, 0] * qxs * 1024.0, (F[0, 1] * qys + F[0, 2]) * 1024.0,
                                                        (F[1, 1] * qys + F[1, 2]) * 1024.0))


def source_range(M, xs, ys, rch):
    """(sx0, sy0, snx, sny) from the extremes of the destination -> source tables of M over columns xs and rows ys"""
    ax, bx, cx, cy = R.tables(M, xs, ys)
    sx0, sx1 = ((int(cx.min()) + int(ax.min())) >> 10) - rch, ((int(cx.max()) + int(ax.max())) >> 10) + rch + 1
    sy0, sy1 = ((int(cy.min()) + int(bx.min())) >> 10) - rch, ((int(cy.max()) + int(bx.max())) >> 10) + rch + 1
    return sx0, sy0, sx1 - sx0 + 1, sy1 - sy0 + 1


def _pixels(img, qx, qy, border):
    """int64 (..., 3): img at the lattice points, the border colour outside, or the clamped index where border is None"""
    h, w = img.shape[:2]
    p = img[np.clip(qy, 0, h - 1), np.clip(qx, 0, w - 1)].astype(np.int64)
    if border is None:
        return p
    inside = (qx >= 0) & (qx < w) & (qy >= 0) & (qy < h)
    return np.where(inside[..., None], p, np.asarray(border, dtype=np.int64))


def _weights(F, qx, qy, x, y):
    U, V = forward(F, qx, qy)
    tu = np.maximum(0, 1024 - np.abs(U - 1024 * x))
    tv = np.maximum(0, 1024 - np.abs(V - 1024 * y))
    return (tu * tv) >> 8


def filtered(img, F, X, Y, xs, ys, rch, border=None, extra=2, stats=None, mask=None):
    """The filter value (int64 (ny, nx, 3)) for the destination pixels (xs, ys) (absolute coordinates) whose Q5 source coordinates are
    X, Y (ny, nx), summed over the window of rch + extra around the centre cell.  stats: a dict that receives the extremes of W and of
    the accumulator.  mask: the pixels whose value is used (paste: those the face touches; the others may have no tap at all)."""
    img = np.asarray(img, dtype=np.uint8)
    ix, iy = X >> 5, Y >> 5
    x, y = np.asarray(xs, dtype=np.int64)[None, :], np.asarray(ys, dtype=np.int64)[:, None]
    acc = np.zeros(X.shape + (3,), dtype=np.int64)
    W = np.zeros(X.shape, dtype=np.int64)
    r = rch + extra
    for dy in range(-r, r + 2):
        for dx in range(-r, r + 2):
            qx, qy = ix + dx, iy + dy
            w = _weights(F, qx, qy, x, y)
            if not w.any():
                continue
            acc += w[..., None] * _pixels(img, qx, qy, border)
            W += w
    used = W if mask is None else W[mask]
    assert (used.size == 0 or used.min() > 0) and acc.max() < 1 << 31
    if stats is not None:
        stats.update(W_min=int(used.min()), W_max=int(used.max()), acc_max=int(acc.max()))
    W = np.maximum(W, 1)
    return (acc + (W >> 1)[..., None]) // W[..., None]


def filtered_all(img, F, X, Y, xs, ys, m, border=None, mask=None):
    """the same value summed over EVERY source lattice point that can weigh anything: one destination pixel at a time over the whole
    lattice rectangle that holds the image and every centre, with a margin of 4 m + 8 (a tent reaches m sqrt(2) source pixels)"""
    img = np.asarray(img, dtype=np.uint8)
    h, w = img.shape[:2]
    ix, iy = X >> 5, Y >> 5
    pad = int(np.ceil(4 * m)) + 8
    qx = np.arange(min(int(ix.min()), 0) - pad, max(int(ix.max()), w) + pad)[None, :]
    qy = np.arange(min(int(iy.min()), 0) - pad, max(int(iy.max()), h) + pad)[:, None]
    qxx, qyy = np.broadcast_arrays(qx, qy)
    px = _pixels(img, qxx, qyy, border)
    out = np.zeros(X.shape + (3,), dtype=np.int64)
    for j, y in enumerate(ys):
        for i, x in enumerate(xs):
            if mask is not None and not mask[j, i]:
                continue
            wt = _weights(F, qx, qy, int(x), int(y))
            W = int(wt.sum())
            assert W > 0
            out[j, i] = ((wt[..., None] * px).sum(axis=(0, 1)) + (W >> 1)) // W
    return out


def crop(photo, A, S, border=(128, 128, 128), every_point=False, stats=None):
    """uint8 (S, S, 3): the anti-aliased crop of `photo` for A (photo -> crop)"""
    A = np.asarray(A, dtype=np.float64)
    M = R.invert(A)
    m = crop_minify(A)
    check_minify(m)
    rch = reach(M, m)
    if rch == 0:
        return R.crop(photo, M, S, border)
    xs = ys = np.arange(S)
    X, Y = R._coords(M, xs, ys)
    if every_point:
        return filtered_all(photo, A, X, Y, xs, ys, m, border).astype(np.uint8)
    return filtered(photo, A, X, Y, xs, ys, rch, border, stats=stats).astype(np.uint8)


def paste(photo, faces, S, ramp=None, every_point=False):
    """photo_ref.paste with the anti-aliased value of every face whose crop is minified into the photo: `faces` = [(restored crop uint8
    (S, S, 3), P), ...] in list order"""
    out = np.array(photo, dtype=np.uint8)
    H, W = out.shape[:2]
    ramp = R.default_ramp() if ramp is None else np.asarray(ramp)
    assert ramp[0] == 0 and ramp.max() <= 256
    L = ramp.shape[0]
    lim = (S - 1) * 32
    for restored, P in faces:
        P = np.asarray(P, dtype=np.float64)
        m = paste_minify(P)
        check_minify(m)
        rch = reach(P, m)
        x0, y0, x1, y1 = R.bbox(P, S, H, W)
        if x1 <= x0 or y1 <= y0:
            continue
        xs, ys = np.arange(x0, x1), np.arange(y0, y1)
        X, Y = R._coords(P, xs, ys)
        d = np.minimum(np.minimum(X, Y), np.minimum(lim - X, lim - Y))
        touch = d >= 0
        w = ramp[np.minimum(np.maximum(d, 0) >> 2, L - 1)].astype(np.int64)
        Xc, Yc = np.clip(X, 0, lim), np.clip(Y, 0, lim)
        restored = np.asarray(restored, dtype=np.uint8)
        if rch == 0:
            f = R._bilinear(restored, Xc, Yc)
        elif every_point:
            f = filtered_all(restored, R.invert(P), Xc, Yc, xs, ys, m, mask=touch)
        else:
            f = filtered(restored, R.invert(P), Xc, Yc, xs, ys, rch, mask=touch)
        bg = out[y0:y1, x0:x1].astype(np.int64)
        mixed = (w[..., None] * f + (256 - w[..., None]) * bg + 128) >> 8
        out[y0:y1, x0:x1] = np.where(touch[..., None], mixed, bg).astype(np.uint8)
    return out
