"""Faces inside whole photos: the host side of csrc/face_warp.hip and the restorer built on it.

    similarity_from_landmarks   five landmarks -> A (2 x 3, photo -> crop): Umeyama's closed-form least-squares similarity onto the
                                FFHQ 512^2 template; float64, NumPy
    FacePlan                    one ragged batch of photos and their faces: the int32 coordinate tables of both kernels, the item and
                                tile tables, the packed photo bytes -- the counterpart of resample.ResamplePlan
    crop_faces / paste_faces    vsp_face_crop_u8 / vsp_face_paste_u8 on a plan (the *_aa entries for a plan built with antialias=True:
                                a face that is minified is resampled by a tent filter one destination pixel wide)
    color_fix                   vsp_color_fix_u8 on the crops and the restored crops: the restored faces take their colours back from the
                                photo before the paste, "stats" or "wavelet"
    PhotoRestorer               photos + landmarks -> photos with their faces restored by a RestorationPipeline

All device arithmetic is integer: the float64 geometry ends in the tables built here (`face_tables`), which tests/photo_ref.py restates.
Integer coordinates are pixel centres; there is no half-pixel shift anywhere.

No torch / HIP import at module level: the geometry and the plan are testable without the library."""
import ctypes as C

import numpy as np

FFHQ512_TEMPLATE = np.array([[192.98138, 239.94708],      # left eye
                             [318.90277, 240.1936],       # right eye
                             [256.63416, 314.01935],      # nose
                             [201.26117, 371.41043],      # left mouth corner
                             [313.08905, 371.15118]],     # right mouth corner
                            dtype=np.float64)
FFHQ512_TEMPLATE.setflags(write=False)

TILE = 32                      # include/vspbfr_hip.h VSP_FACE_TILE
MAX_SIDE = 8192                # VSP_FACE_MAX_SIDE
MAX_ITEMS = 65535              # VSP_FACE_MAX_ITEMS
MAX_RAMP = 65536               # VSP_FACE_MAX_RAMP
TABLE_LIMIT = 1 << 30          # a table entry of this magnitude is refused (cx + ax must not wrap)
DEFAULT_BORDER = (128, 128, 128)
DEFAULT_INSET, DEFAULT_FEATHER = 8, 48     # px; design choices, not measurements
MAX_MINIFY = 16                # the largest minification the filtered kernels serve (int32 accumulator)
MAX_REACH = 23                 # VSP_FACE_AA_MAX_REACH = ceil(16 sqrt(2) + 0.125)


class FaceItem(C.Structure):
    """include/vspbfr_hip.h vsp_face_item"""
    _fields_ = [("src_off", C.c_int64), ("tab_off", C.c_int64)] + [(n, C.c_int32) for n in ("h", "w", "x0", "y0", "nx", "ny")]


class FaceAAItem(C.Structure):
    """include/vspbfr_hip.h vsp_face_aa_item"""
    _fields_ = ([("src_off", C.c_int64), ("tab_off", C.c_int64), ("fwd_off", C.c_int64)]
                + [(n, C.c_int32) for n in ("h", "w", "x0", "y0", "nx", "ny", "sx0", "sy0", "snx", "sny", "reach", "pad_")])


class FaceTile(C.Structure):
    """include/vspbfr_hip.h vsp_face_tile"""
    _fields_ = [("dst_off", C.c_int64)] + [(n, C.c_int32) for n in ("h", "w", "x0", "y0", "face0", "nfaces")]


def _where(photo, face):
    return f"photo {photo!r}, face {face}"


def similarity_from_landmarks(pts5, template=FFHQ512_TEMPLATE, size=512, photo="?", face=0):
    """A (2 x 3 float64, photo -> crop): the least-squares similarity -- rotation, one uniform scale, translation, never a reflection --
    that takes the five landmarks onto `template` scaled by size / 512 (Umeyama 1991, closed form with the determinant check).
    ValueError naming the photo and the face for landmarks that are not (5, 2), not finite, or degenerate (variance below 1e-12)."""
    try:
        src = np.asarray(pts5, dtype=np.float64)
    except (TypeError, ValueError):
        raise ValueError(f"{_where(photo, face)}: landmarks are not numbers") from None
    if src.shape != (5, 2):
        raise ValueError(f"{_where(photo, face)}: landmarks must have shape (5, 2), got {src.shape}")
    if not np.all(np.isfinite(src)):
        raise ValueError(f"{_where(photo, face)}: landmarks are not finite")
    dst = np.asarray(template, dtype=np.float64) * (float(size) / 512.0)
    ms, md = src.mean(axis=0), dst.mean(axis=0)
    sc, dc = src - ms, dst - md
    var = float((sc * sc).sum() / 5.0)
    if not var >= 1e-12:
        raise ValueError(f"{_where(photo, face)}: degenerate landmarks (variance {var:.3g})")
    U, D, Vt = np.linalg.svd(dc.T @ sc / 5.0)
    sgn = np.ones(2)
    if np.linalg.det(U) * np.linalg.det(Vt) < 0:      # the best orthogonal fit would mirror: flip the weaker axis instead
        sgn[1] = -1.0
    R = U @ np.diag(sgn) @ Vt
    scale = float((D * sgn).sum()) / var
    t = md - scale * (R @ ms)
    return np.concatenate([scale * R, t[:, None]], axis=1)


def invert_affine(A):
    """closed-form inverse of a 2 x 3 affine map"""
    a, b, tx, c, d, ty = (float(v) for v in np.asarray(A, dtype=np.float64).reshape(-1))
    det = a * d - b * c
    return np.array([[d / det, -b / det, (b * ty - d * tx) / det], [-c / det, a / det, (c * tx - a * ty) / det]], dtype=np.float64)


def paste_matrix(A, upscale=1):
    """P (output photo -> crop): A after the output coordinates are divided by the upscale factor"""
    P = np.array(A, dtype=np.float64)
    P[:, :2] = P[:, :2] / float(upscale)
    return P


def face_tables(M, xs, ys, photo="?", face=0):
    """The int32 tables of one face for M (2 x 3 float64, destination -> source), destination columns xs and rows ys, concatenated as the
    kernels read them: ax[nx], bx[nx], cx[ny], cy[ny] (include/vspbfr_hip.h).  np.rint rounds half to even."""
    M = np.asarray(M, dtype=np.float64)
    xs, ys = np.asarray(xs, dtype=np.float64), np.asarray(ys, dtype=np.float64)
    parts = (np.rint(M[0, 0] * xs * 1024.0), np.rint(M[1, 0] * xs * 1024.0), np.rint((M[0, 1] * ys + M[0, 2]) * 1024.0) + 16.0,
             np.rint((M[1, 1] * ys + M[1, 2]) * 1024.0) + 16.0)
    t = np.concatenate(parts)
    if t.size and not np.all(np.abs(t) < TABLE_LIMIT):
        raise ValueError(f"{_where(photo, face)}: the face lies too far outside the photo or is too small (a coordinate table entry reaches 2^30)")
    return t.astype(np.int32)


def crop_minify(A):
    """source pixels per crop pixel: 1 / |A|, |A| the similarity's scale"""
    return 1.0 / float(np.hypot(A[0, 0], A[1, 0]))


def paste_minify(P):
    """crop pixels per output pixel: |P| = |A| / upscale"""
    return float(np.hypot(P[0, 0], P[1, 0]))


def filter_reach(M, m):
    """0 for a face that is not minified (m <= 1: four-tap bilinear), else ceil(|M00| + |M01| + 0.125) for M (destination -> source):
    every source lattice point with a non-zero tent weight lies in columns ix - reach .. ix + reach + 1 of the centre cell, rows
    likewise (|M10| + |M11| is the same number for a similarity)"""
    return 0 if m <= 1.0 else int(np.ceil(abs(float(M[0, 0])) + abs(float(M[0, 1])) + 0.125))


def forward_tables(F, qxs, qys, photo="?", face=0):
    """The int32 forward tables of one filtered face for F (2 x 3 float64, source -> destination), source columns qxs and rows qys,
    concatenated as the kernels read them: fu[snx], fv[snx], gu[sny], gv[sny] (include/vspbfr_hip.h).  No rounding offset: U = fu + gu
    is the destination coordinate of a source lattice point in Q10."""
    F = np.asarray(F, dtype=np.float64)
    qxs, qys = np.asarray(qxs, dtype=np.float64), np.asarray(qys, dtype=np.float64)
    t = np.concatenate((np.rint(F[0, 0] * qxs * 1024.0), np.rint(F[1, 0] * qxs * 1024.0), np.rint((F[0, 1] * qys + F[0, 2]) * 1024.0),
                        np.rint((F[1, 1] * qys + F[1, 2]) * 1024.0)))
    if t.size and not np.all(np.abs(t) < TABLE_LIMIT):
        raise ValueError(f"{_where(photo, face)}: the face lies too far outside the photo (a forward table entry reaches 2^30)")
    return t.astype(np.int32)


def source_range(t, nx, ny, reach):
    """(sx0, sy0, snx, sny): the source columns and rows that hold the filter window of every destination pixel of one face, from the
    extremes of its destination -> source tables t = ax[nx], bx[nx], cx[ny], cy[ny] -- what the C entry checks"""
    t = t.astype(np.int64)
    ax, bx, cx, cy = t[:nx], t[nx:2 * nx], t[2 * nx:2 * nx + ny], t[2 * nx + ny:]
    sx0, sx1 = ((int(cx.min()) + int(ax.min())) >> 10) - reach, ((int(cx.max()) + int(ax.max())) >> 10) + reach + 1
    sy0, sy1 = ((int(cy.min()) + int(bx.min())) >> 10) - reach, ((int(cy.max()) + int(bx.max())) >> 10) + reach + 1
    return sx0, sy0, sx1 - sx0 + 1, sy1 - sy0 + 1


def check_minify(A, upscale=1, photo="?", face=0):
    """(crop minification, paste minification) of one face; ValueError naming the photo and the face above MAX_MINIFY"""
    mc, mp = crop_minify(A), paste_minify(paste_matrix(A, upscale))
    if mc > MAX_MINIFY:
        raise ValueError(f"{_where(photo, face)}: the face is {mc:.1f} times larger than the crop; the anti-aliased crop serves at most "
                         f"{MAX_MINIFY} (shrink the photo first)")
    if mp > MAX_MINIFY:
        raise ValueError(f"{_where(photo, face)}: the crop is {mp:.1f} times larger than the face in the output photo; the anti-aliased "
                         f"paste serves at most {MAX_MINIFY}")
    return mc, mp


def face_bbox(P, S, H, W):
    """(x0, y0, x1, y1), ends exclusive: the corners of the crop square [0, S - 1]^2 taken back through P into the (H, W) output photo,
    floor / ceil with one pixel of margin (the tables are rounded), clipped to the photo.  Empty (x1 <= x0 or y1 <= y0) where the face
    lies outside."""
    Q = invert_affine(P)
    c = np.array([[0.0, 0.0], [S - 1.0, 0.0], [0.0, S - 1.0], [S - 1.0, S - 1.0]])
    px = Q[0, 0] * c[:, 0] + Q[0, 1] * c[:, 1] + Q[0, 2]
    py = Q[1, 0] * c[:, 0] + Q[1, 1] * c[:, 1] + Q[1, 2]
    x0, x1 = int(np.floor(px.min())) - 1, int(np.ceil(px.max())) + 2
    y0, y1 = int(np.floor(py.min())) - 1, int(np.ceil(py.max())) + 2
    return max(x0, 0), max(y0, 0), min(x1, W), min(y1, H)


def default_ramp(inset=DEFAULT_INSET, feather=DEFAULT_FEATHER):
    """The blend weight over the distance from the crop border in 1/8 px, uint16 0..256: 0 up to `inset` px, a raised cosine up to 256
    over the next `feather` px; L = 8 (inset + feather) + 1 entries, the last one holds for every larger distance."""
    inset, feather = int(inset), int(feather)
    if inset < 0 or feather < 0 or 8 * (inset + feather) + 1 > MAX_RAMP:
        raise ValueError(f"default_ramp: inset {inset}, feather {feather}")
    px = np.arange(8 * (inset + feather) + 1, dtype=np.float64) / 8.0
    t = np.clip((px - inset) / float(feather), 0.0, 1.0) if feather > 0 else (px > inset).astype(np.float64)
    r = np.rint(128.0 * (1.0 - np.cos(np.pi * t))).astype(np.uint16)
    r[0] = 0
    return r


class FacePlan:
    """One ragged batch: `photos` (uint8 (h, w, 3) arrays) and `faces` = [(photo index, five landmarks), ...] in paste order.
    device_photos: a flat uint8 device tensor that already holds the photos back to back (jpeg.decode_files); `photos` are then
    their (h, w) -- pixels beside the tensor are refused --, upload() sends the tables alone and uses the tensor as its `photos` section.

    For face i: A_i = similarity_from_landmarks; the crop tables of M = A^-1 over the S x S crop; P = paste_matrix(A, upscale), its
    bounding box in the (upscale h, upscale w) output photo and the paste tables over that box.  The paste tiles: every 32 x 32 tile of
    the output photos' tile grids that a box meets, ascending by (photo, row, column), each with its faces in list order.
    `names` (one per photo) appear in error messages.

    antialias=True adds, per face and kernel, the minification m (crop: 1 / |A|, paste: |A| / upscale), reach (0 where m <= 1: that face
    keeps the four bilinear taps), the forward tables over the source range its filter windows touch and a vsp_face_aa_item; a
    minification above MAX_MINIFY is a ValueError.  Without it nothing of this is computed and pack() is unchanged."""

    def __init__(self, photos, faces, size=512, upscale=1, names=None, antialias=False, device_photos=None):
        self.S, self.upscale, self.antialias = int(size), int(upscale), bool(antialias)
        self.device_photos = device_photos
        if not 1 <= self.S <= MAX_SIDE or self.upscale < 1:
            raise ValueError(f"FacePlan: size {size}, upscale {upscale}")
        if len(faces) > MAX_ITEMS:
            raise ValueError(f"FacePlan: at most {MAX_ITEMS} faces")
        names = [str(k) for k in range(len(photos))] if names is None else list(names)
        self.photos, self.shapes, self.src_off, self.out_off, self.out_shape = [], [], [], [], []
        src = out = 0
        for k, a in enumerate(photos):
            if device_photos is not None:                  # the pixels are in device_photos: `a` is the photo's (h, w)
                if hasattr(a, "dtype") or len(tuple(a)) != 2:
                    raise ValueError(f"photo {names[k]!r}: with device_photos the photos are given as (h, w), not as pixels")
                h, w = (int(v) for v in a)
                if h < 1 or w < 1:
                    raise ValueError(f"photo {names[k]!r}: shape {tuple(a)}")
                self.photos.append(None)
            else:
                a = np.asarray(a)
                if a.dtype != np.uint8 or a.ndim != 3 or a.shape[2] != 3 or a.shape[0] < 1 or a.shape[1] < 1:
                    raise ValueError(f"photo {names[k]!r}: must be uint8 (h, w, 3), got {a.dtype} {a.shape}")
                self.photos.append(np.ascontiguousarray(a))
                h, w = a.shape[:2]
            self.shapes.append((h, w))
            self.src_off.append(src)
            self.out_off.append(out)
            self.out_shape.append((h * self.upscale, w * self.upscale))
            src += 3 * h * w
            out += 3 * h * w * self.upscale * self.upscale
        self.src_bytes, self.out_bytes = src, out
        if max(src, out) >= 1 << 31:
            raise ValueError("FacePlan: a batch of photos must stay below 2 GiB")
        if device_photos is not None:
            import torch
            if device_photos.dtype != torch.uint8 or device_photos.dim() != 1 or device_photos.numel() != src or not device_photos.is_contiguous():
                raise ValueError(f"FacePlan: device_photos must be a flat contiguous uint8 tensor of {src} bytes")
        S, n = self.S, len(faces)
        self.n = n
        self.face_photo, self.A, self.P, self.boxes = [], [], [], []
        self.crop_items, self.paste_items = (FaceItem * max(n, 1))(), (FaceItem * max(n, 1))()
        crop_tabs, paste_tabs, ct, pt = [], [], 0, 0
        if self.antialias:
            self.crop_aa_items, self.paste_aa_items = (FaceAAItem * max(n, 1))(), (FaceAAItem * max(n, 1))()
            self.crop_minify, self.paste_minify = [], []
            fwd = {"crop": [], "paste": []}
            fwd_n = {"crop": 0, "paste": 0}

        def aa_item(kind, dst, it, t, M, F, m, where):
            """the vsp_face_aa_item of one face for one kernel: `it` plus reach, source range and forward tables"""
            for name in ("src_off", "tab_off", "h", "w", "x0", "y0", "nx", "ny"):
                setattr(dst, name, getattr(it, name))
            reach = filter_reach(M, m) if it.nx > 0 and it.ny > 0 else 0
            dst.reach, dst.fwd_off = reach, fwd_n[kind]
            if reach:
                dst.sx0, dst.sy0, dst.snx, dst.sny = source_range(t, it.nx, it.ny, reach)
                f = forward_tables(F, np.arange(dst.sx0, dst.sx0 + dst.snx), np.arange(dst.sy0, dst.sy0 + dst.sny), *where)
                fwd[kind].append(f)
                fwd_n[kind] += f.size
        per_photo = {}
        which = {}
        for i, (k, pts) in enumerate(faces):
            k = int(k)
            if not 0 <= k < len(self.photos):
                raise ValueError(f"face {i}: photo index {k}")
            j = which[k] = which.get(k, -1) + 1           # the face's number inside its photo, for messages
            h, w = self.shapes[k]
            A = similarity_from_landmarks(pts, size=S, photo=names[k], face=j)
            P = paste_matrix(A, self.upscale)
            oh, ow = self.out_shape[k]
            x0, y0, x1, y1 = face_bbox(P, S, oh, ow)
            if x1 <= x0 or y1 <= y0:
                x0 = y0 = x1 = y1 = 0
            self.face_photo.append(k)
            self.A.append(A)
            self.P.append(P)
            self.boxes.append((x0, y0, x1, y1))
            if self.antialias:
                mc, mp = check_minify(A, self.upscale, names[k], j)
                self.crop_minify.append(mc)
                self.paste_minify.append(mp)
            Ai = invert_affine(A)
            t = face_tables(Ai, np.arange(S), np.arange(S), names[k], j)
            it = self.crop_items[i]
            it.src_off, it.tab_off, it.h, it.w, it.x0, it.y0, it.nx, it.ny = self.src_off[k], ct, h, w, 0, 0, S, S
            crop_tabs.append(t)
            ct += t.size
            if self.antialias:
                aa_item("crop", self.crop_aa_items[i], it, t, Ai, A, mc, (names[k], j))
            t = face_tables(P, np.arange(x0, x1), np.arange(y0, y1), names[k], j)
            it = self.paste_items[i]
            it.src_off, it.tab_off, it.h, it.w, it.x0, it.y0, it.nx, it.ny = i * 3 * S * S, pt, S, S, x0, y0, x1 - x0, y1 - y0
            paste_tabs.append(t)
            pt += t.size
            if self.antialias:
                aa_item("paste", self.paste_aa_items[i], it, t, P, invert_affine(P), mp, (names[k], j))
            if x1 > x0:
                per_photo.setdefault(k, []).append(i)
        self.crop_tables = np.concatenate(crop_tabs) if crop_tabs else np.zeros(0, dtype=np.int32)
        self.paste_tables = np.concatenate(paste_tabs) if paste_tabs else np.zeros(0, dtype=np.int32)
        if self.antialias:
            self.crop_fwd = np.concatenate(fwd["crop"]) if fwd["crop"] else np.zeros(0, dtype=np.int32)
            self.paste_fwd = np.concatenate(fwd["paste"]) if fwd["paste"] else np.zeros(0, dtype=np.int32)
        tiles, tile_faces = [], []
        for k in sorted(per_photo):
            oh, ow = self.out_shape[k]
            cover = {}
            for i in per_photo[k]:                         # ascending face index: list order
                x0, y0, x1, y1 = self.boxes[i]
                for ty in range(y0 // TILE, (y1 - 1) // TILE + 1):
                    for tx in range(x0 // TILE, (x1 - 1) // TILE + 1):
                        cover.setdefault((ty, tx), []).append(i)
            for (ty, tx) in sorted(cover):
                tiles.append((self.out_off[k], oh, ow, tx * TILE, ty * TILE, len(tile_faces), len(cover[(ty, tx)])))
                tile_faces.extend(cover[(ty, tx)])
        self.ntiles = len(tiles)
        self.tiles = (FaceTile * max(self.ntiles, 1))()
        for t, v in zip(self.tiles, tiles):
            t.dst_off, t.h, t.w, t.x0, t.y0, t.face0, t.nfaces = v
        self.tile_faces = np.asarray(tile_faces, dtype=np.int32)
        self._host = self._dev = None
        self._ramps = {}

    # ---------------------------------------------------------------------------------------------------------------- device side
    def pack(self):
        """every table and the photo bytes in ONE pinned uint8 buffer, 16-byte aligned sections (the photos packed without padding)
        -> (buffer, {section: (offset, bytes)})"""
        import torch
        if self._host is None:
            n, nt = self.n, self.ntiles
            parts = [("crop_items", np.frombuffer(bytes(self.crop_items), dtype=np.uint8)[:n * C.sizeof(FaceItem)]),
                     ("paste_items", np.frombuffer(bytes(self.paste_items), dtype=np.uint8)[:n * C.sizeof(FaceItem)]),
                     ("tiles", np.frombuffer(bytes(self.tiles), dtype=np.uint8)[:nt * C.sizeof(FaceTile)]),
                     ("tile_faces", self.tile_faces.view(np.uint8)), ("crop_tables", self.crop_tables.view(np.uint8)),
                     ("paste_tables", self.paste_tables.view(np.uint8))]
            if self.antialias:                              # extra sections; without them the buffer is what it always was
                parts += [("crop_aa_items", np.frombuffer(bytes(self.crop_aa_items), dtype=np.uint8)[:n * C.sizeof(FaceAAItem)]),
                          ("paste_aa_items", np.frombuffer(bytes(self.paste_aa_items), dtype=np.uint8)[:n * C.sizeof(FaceAAItem)]),
                          ("crop_fwd", self.crop_fwd.view(np.uint8)), ("paste_fwd", self.paste_fwd.view(np.uint8))]
            sections, off = {}, 0
            for name, a in parts:
                sections[name] = (off, a.size)
                off = (off + a.size + 15) // 16 * 16
            held = self.device_photos is not None          # the photos are on the device already: the buffer ends behind the tables
            if not held:
                sections["photos"] = (off, self.src_bytes)
            host = torch.empty(off + (0 if held else self.src_bytes), dtype=torch.uint8, pin_memory=torch.cuda.is_available())
            hv = host.numpy()
            for name, a in parts:
                hv[sections[name][0]:sections[name][0] + a.size] = a
            for o, a in zip(self.src_off, () if held else self.photos):
                hv[off + o:off + o + a.size] = a.reshape(-1)
            self._host = (host, sections)
        return self._host

    def upload(self, device):
        """one copy on the current stream -> {section: device uint8 view}; kept for the later calls on the same device"""
        import torch
        device = torch.device(device)
        if self._dev is None or self._dev[0] != device:
            host, sections = self.pack()
            dev = host.to(device, non_blocking=True)
            self._dev = (device, {name: dev[o:o + nb] for name, (o, nb) in sections.items()})
            if self.device_photos is not None:
                if self.device_photos.device != dev.device:
                    raise ValueError(f"FacePlan: device_photos is on {self.device_photos.device}, the plan goes to {dev.device}")
                self._dev[1]["photos"] = self.device_photos
        return self._dev[1]

    def background(self, device, upscaler=None):
        """The packed output photos before any face is pasted, a fresh device uint8 buffer of out_bytes: the photos themselves at upscale
        1, else each photo resized to exactly (upscale w, upscale h) -- by the device LANCZOS kernel where resample.kernel_serves takes
        it, by PIL otherwise; both are Pillow's bytes.  The group is ONE ragged plan (resample.ResamplePlan with out_sizes) whose
        source is the plan's device `photos` section and whose destinations are the photos' places in the output: one launch pair,
        and no pixel leaves the device but those of a photo the kernel does not serve.

        upscaler (an upscale.SrUpscaler): the photos go through the network instead -- straight to out_off where its scale is
        the plan's, through one ragged LANCZOS resize of its x4 output at upscale 2; upscale 1 or a network below the plan's upscale is
        a ValueError.  `self.background_info` is then upscale()'s info.  None: nothing changes."""
        import torch
        dev = self.upload(device)
        if upscaler is not None:
            if self.upscale not in (2, 4) or upscaler.scale < self.upscale:
                raise ValueError(f"FacePlan.background: a x{upscaler.scale} network cannot fill an upscale of {self.upscale}")
            out = torch.empty(self.out_bytes, dtype=torch.uint8, device=dev["photos"].device)
            out, self.background_info = upscaler.upscale_to(self.upscale, device_photos=(dev["photos"], self.src_off, self.shapes), out=out,
                                                            out_offsets=self.out_off)
            return out
        if self.upscale == 1:
            return dev["photos"].clone()
        from .resample import ResamplePlan
        out = torch.empty(self.out_bytes, dtype=torch.uint8, device=dev["photos"].device)
        plan = ResamplePlan(self.shapes, [(ow, oh) for oh, ow in self.out_shape], [(0, 0)] * len(self.shapes), None,
                            device_sources=(dev["photos"], self.src_off), out_sizes=self.out_shape, out_offsets=self.out_off)
        return plan.run_into(out)

    def split(self, packed):
        """the (upscale h, upscale w, 3) views of a packed output buffer, one per photo"""
        return [packed[o:o + 3 * oh * ow].view(oh, ow, 3) for o, (oh, ow) in zip(self.out_off, self.out_shape)]


def crop_faces(plan, device, u8=True, f32=False, border=DEFAULT_BORDER):
    """The aligned crops of every face of the plan on `device`, current stream -> (u8 (F, S, S, 3) or None, f32 (F, 3, S, S) or None)."""
    from . import hip_ops
    dev = plan.upload(device)
    if plan.antialias:
        return hip_ops.face_crop_aa_u8(plan, dev["crop_aa_items"], dev["crop_tables"], dev["crop_fwd"], dev["photos"], border=border, u8=u8, f32=f32)
    return hip_ops.face_crop_u8(plan, dev["crop_items"], dev["crop_tables"], dev["photos"], border=border, u8=u8, f32=f32)


def paste_faces(plan, restored_u8, device, ramp=None, out=None, mask=None):
    """Paste the restored crops ((F, S, S, 3) uint8 on the device) into the output photos, in place on `out` (a packed device buffer of
    plan.out_bytes; default plan.background(device)) -> out.  ramp: uint16 weights 0..256 over the distance from the crop border in
    1/8 px, ramp[0] = 0; default default_ramp().  plan.split(out) gives the photos.  mask: the (F, S, S) uint16 paste weights
    of parse.FaceParser.mask on the device -- the ramp weight is scaled by the mask sampled where the colour is; None: the unmasked entries."""
    import torch

    from . import hip_ops
    dev = plan.upload(device)
    if out is None:
        out = plan.background(device)
    ramp = default_ramp() if ramp is None else np.ascontiguousarray(np.asarray(ramp))
    if ramp.dtype != np.uint16 or ramp.ndim != 1:
        raise ValueError("paste_faces: ramp must be a one-dimensional uint16 array")
    key = (str(torch.device(device)), ramp.tobytes())
    ramp_dev = plan._ramps.get(key)              # a plan pasted more than once uploads its ramp once
    if ramp_dev is None:
        ramp_dev = plan._ramps[key] = torch.from_numpy(ramp.view(np.int16).copy()).to(device)
    if mask is not None and plan.antialias:
        hip_ops.face_paste_mask_aa_u8(plan, out, restored_u8, dev["paste_aa_items"], dev["paste_tables"], dev["paste_fwd"], dev["tiles"],
                                      dev["tile_faces"], ramp, ramp_dev, mask)
    elif mask is not None:
        hip_ops.face_paste_mask_u8(plan, out, restored_u8, dev["paste_items"], dev["paste_tables"], dev["tiles"], dev["tile_faces"], ramp,
                                   ramp_dev, mask)
    elif plan.antialias:
        hip_ops.face_paste_aa_u8(plan, out, restored_u8, dev["paste_aa_items"], dev["paste_tables"], dev["paste_fwd"], dev["tiles"],
                                 dev["tile_faces"], ramp, ramp_dev)
    else:
        hip_ops.face_paste_u8(plan, out, restored_u8, dev["paste_items"], dev["paste_tables"], dev["tiles"], dev["tile_faces"], ramp, ramp_dev)
    return out


COLOR_FIX_MODES = ("stats", "wavelet")
MAX_COLOR_LEVELS = 6           # VSP_COLOR_FIX_MAX_LEVELS


def check_color_fix(mode, levels=5):
    """(mode or None, levels) of a colour-fix request, ValueError for an unknown mode or levels outside 1..6; None and "none" ask for none"""
    mode = None if mode in (None, "none") else mode
    if mode is not None and mode not in COLOR_FIX_MODES:
        raise ValueError(f"color_fix: mode {mode!r} (None, 'stats' or 'wavelet')")
    if isinstance(levels, bool) or int(levels) != levels or not 1 <= int(levels) <= MAX_COLOR_LEVELS:
        raise ValueError(f"color_fix: levels {levels!r} (1..{MAX_COLOR_LEVELS})")
    return mode, int(levels)


def color_fix(crops_u8, restored_u8, mode, plan=None, device=None, levels=5, out=None):
    """The colour fix of DESIGN 17 on any pair of (F, S, S, 3) uint8 device tensors -> (F, S, S, 3) uint8 (`out`, which may be restored_u8
    itself; default a new tensor).  mode "wavelet": the restored crop keeps its own high frequencies and takes the low ones -- `levels`
    dilated [1 2 1] blurs of the difference -- from the crop; "stats": its per-channel mean and deviation move onto the crop's.  `plan`
    (a FacePlan whose faces these crops are) supplies validity: crop pixels whose centre cell lies outside the photo hold the border
    colour and take no part.  Without a plan every pixel is valid.  device: where the plan's tables go (default: the crops' device)."""
    from . import hip_ops
    mode, levels = check_color_fix(mode, levels)
    if mode is None:
        raise ValueError("color_fix: mode None (nothing to do)")
    if plan is None:
        return hip_ops.color_fix_u8(crops_u8, restored_u8, mode, levels=levels, out=out)
    dev = plan.upload(crops_u8.device if device is None else device)
    return hip_ops.color_fix_u8(crops_u8, restored_u8, mode, plan, dev["crop_items"], dev["crop_tables"], levels=levels, out=out)


class PhotoRestorer:
    """photos + five-point landmarks -> the photos with every face restored.  The photos stay on the device: crop (vsp_face_crop_u8),
    `pipe` (a RestorationPipeline) over the faces of all photos in batches of `batch`, quantisation to uint8 as PngWriter does
    (vsp_quantize_u8_nhwc), paste (vsp_face_paste_u8) onto the photos -- resized first by Pillow's LANCZOS for upscale 2 or 4.
    antialias=True: the anti-aliased entries for crop and paste.  color_fix="stats" or "wavelet": the restored crops take
    their colours back from the crops (vsp_color_fix_u8) and the fixed crops are pasted.  background: an upscale.SrUpscaler
    whose output replaces the LANCZOS resize under the faces (upscale 2 or 4, at most the network's scale).  parser: a
    parse.FaceParser -- the paste goes through the mask it computes from the network's `restored` crops (also when a colour
    fix is on; the crops that are pasted stay what they are); parse_taps / parse_border / parse_keep are handed to its mask().  After a
    call `parse_info` holds {"classes", "mask", "flags"} of the call's faces (None without a parser)."""

    def __init__(self, pipe, batch, upscale=1, size=512, inset=DEFAULT_INSET, feather=DEFAULT_FEATHER, border=DEFAULT_BORDER,
                 antialias=False, color_fix=None, color_levels=5, background=None, parser=None, parse_taps=None, parse_border=None,
                 parse_keep=None):
        if int(upscale) not in (1, 2, 4) or int(batch) < 1:
            raise ValueError(f"PhotoRestorer: batch {batch}, upscale {upscale}")
        if background is not None and (int(upscale) == 1 or background.scale < int(upscale)):
            raise ValueError(f"PhotoRestorer: a x{background.scale} background network cannot fill an upscale of {upscale}")
        self.background = background           # an upscale.SrUpscaler that fills the output photos instead of the LANCZOS resize
        self.pipe, self.batch, self.upscale, self.size, self.border = pipe, int(batch), int(upscale), int(size), tuple(border)
        self.antialias = bool(antialias)       # minified faces through the tent filter of DESIGN 16, crop and paste
        self.ramp = default_ramp(inset, feather)
        self.color_fix, self.color_levels = check_color_fix(color_fix, color_levels)
        if parser is not None:
            from .parse import check_size
            check_size(int(size))
        self.parser, self.parse_taps, self.parse_border, self.parse_keep, self.parse_info = parser, parse_taps, parse_border, parse_keep, None

    def _mask(self, restored):
        """the paste weights of the restored crops, or None without a parser"""
        self.parse_info = None
        if self.parser is None or restored.shape[0] == 0:
            return None
        mask, flags, classes = self.parser.mask(restored, taps=self.parse_taps, border=self.parse_border, keep=self.parse_keep, classes=True)
        self.parse_info = {"classes": classes, "mask": mask, "flags": flags}
        return mask

    def __call__(self, photos, landmarks, device, names=None, device_photos=None):
        """photos: uint8 (h, w, 3) arrays -- or their (h, w) with device_photos, the packed device buffer that holds them back to back
        (jpeg.decode_files) --; landmarks: per photo a list of (5, 2) point sets (None or [] for none) ->
        (output photos: device uint8 (upscale h, upscale w, 3) tensors, crops (F, S, S, 3) uint8, restored (F, S, S, 3) uint8, plan);
        with a colour fix a fifth element, the fixed crops (F, S, S, 3) uint8 that were pasted (`restored` stays the network's output).
        plan.out_packed is the packed buffer the output photos are views of (photo k at byte plan.out_off[k], plan.out_shape[k])"""
        import torch

        from . import hip_ops
        faces = [(k, pts) for k, per in enumerate(landmarks) for pts in (per or [])]
        plan = FacePlan(photos, faces, self.size, self.upscale, names, antialias=self.antialias, device_photos=device_photos)
        S = self.size
        self.parse_info = None
        if plan.n == 0:
            empty = torch.empty((0, S, S, 3), dtype=torch.uint8, device=device)
            plan.out_packed = plan.background(device) if self.background is None else plan.background(device, self.background)
            head = (plan.split(plan.out_packed), empty, empty, plan)
            return head if self.color_fix is None else head + (empty,)
        crops, low = crop_faces(plan, device, u8=True, f32=True, border=self.border)
        restored = []
        with torch.no_grad():
            for i in range(0, plan.n, self.batch):
                out = self.pipe(low[i:i + self.batch])
                restored.append(hip_ops.quantize_u8_nhwc(out["restored"].contiguous(), -1.0, 1.0))
        restored = torch.cat(restored) if len(restored) > 1 else restored[0]
        bg = None if self.background is None else plan.background(device, self.background)
        mask = self._mask(restored)
        if self.color_fix is None:
            out = plan.out_packed = paste_faces(plan, restored, device, self.ramp, out=bg, mask=mask)
            return plan.split(out), crops, restored, plan
        fixed = color_fix(crops, restored, self.color_fix, plan, device, self.color_levels)
        out = plan.out_packed = paste_faces(plan, fixed, device, self.ramp, out=bg, mask=mask)
        return plan.split(out), crops, restored, plan, fixed
