"""Every refusal of the five whole-photo entries (vsp_face_crop_u8, vsp_face_crop_aa_u8, vsp_face_paste_u8, vsp_face_paste_aa_u8,
vsp_color_fix_u8; csrc/face_warp.hip, csrc/color_fix.hip), without a GPU: each of them checks its arguments on the host and returns
before any HIP call, and the library loads without a device.  A case is ONE mutation of otherwise valid arguments, the return code and a
distinctive fragment of vsp_last_error(), which must also begin with the called entry's own prefix.  Device pointers are aligned
non-null dummies; they are never dereferenced on a refusing path, and no case here passes fully valid arguments with work to do (that
would launch).

The table extents check of one face's tables (`table extents %d x %d`) cannot fire through the two crop entries or the colour fix, which
have already required nx == ny == S <= 8192, and a filtered destination beyond 2^20 cannot be reached through the anti-aliased crop
(x0 == y0 == 0 there): both are exercised through the paste entries.

Passed unchanged on the library before the four entries were folded onto one validator pair and on the library after it."""
import ctypes as C

import numpy as np
import pytest

import photo_ref as R
from vspbfr_amd import photo

S = 16
EINVAL, ENOTSUP = -1, -3
DEV = [0x100000 * (k + 1) for k in range(12)]      # 1 MiB apart: aligned, non-null, non-overlapping


def _plan(antialias):
    """two photos (40 x 56 and 33 x 47, rows x columns) at upscale 2 and three faces: a 32 px face (crop minified by 2: filtered in the crop)
    and a 10.7 px one turned by 30 degrees over it (filtered nowhere) in the first photo, a 5.3 px one (paste minified by 1.5: filtered in
    the paste) in the second"""
    photos = [R.test_photo(56, 40, seed=1), R.test_photo(47, 33, seed=2)]
    faces = [(0, R.landmarks_for(0.5, 0.0, (28.0, 20.0), S)), (0, R.landmarks_for(1.5, 30.0, (30.0, 22.0), S)),
             (1, R.landmarks_for(3.0, 17.0, (20.0, 15.0), S))]
    return photo.FacePlan(photos, faces, size=S, upscale=2, antialias=antialias)


@pytest.fixture(scope="module")
def plans():
    plain, aa = _plan(False), _plan(True)
    assert [it.reach > 0 for it in aa.crop_aa_items] == [True, False, False]
    assert [it.reach > 0 for it in aa.paste_aa_items] == [False, False, True]
    tiles = list(aa.tiles)
    assert len({t.dst_off for t in tiles}) == 2 and len({t.y0 for t in tiles if t.dst_off == 0}) > 1 and any(t.nfaces > 1 for t in tiles)
    return {False: plain, True: aa}


class Args(dict):
    """the arguments of one call by name, in the entry's order; host arrays are private copies"""
    __getattr__ = dict.__getitem__
    __setattr__ = dict.__setitem__


def _copy(arr):
    return type(arr).from_buffer_copy(arr)


def _raw(v):
    if isinstance(v, np.ndarray):
        return v.ctypes.data
    if isinstance(v, C.Array):
        return C.addressof(v)
    return v


def crop_args(plan, aa):
    a = Args(out_u8=DEV[0], out_f32=DEV[1], src=DEV[2], src_bytes=plan.src_bytes, tables=plan.crop_tables.copy(), tables_dev=DEV[3],
             table_ints=plan.crop_tables.size)
    if aa:
        a.update(fwd=plan.crop_fwd.copy(), fwd_dev=DEV[4], fwd_ints=plan.crop_fwd.size)
    a.update(items=_copy(plan.crop_aa_items if aa else plan.crop_items), items_dev=DEV[5], n=plan.n, S=plan.S, br=128, bg=128, bb=128, stream=None)
    return a


def paste_args(plan, aa):
    ramp = photo.default_ramp(1, 2)
    a = Args(photos=DEV[0], photo_bytes=plan.out_bytes, crops=DEV[1], crop_bytes=plan.n * 3 * S * S, tables=plan.paste_tables.copy(),
             tables_dev=DEV[3], table_ints=plan.paste_tables.size)
    if aa:
        a.update(fwd=plan.paste_fwd.copy(), fwd_dev=DEV[4], fwd_ints=plan.paste_fwd.size)
    a.update(items=_copy(plan.paste_aa_items if aa else plan.paste_items), items_dev=DEV[5], n=plan.n, S=plan.S, tiles=_copy(plan.tiles),
             tiles_dev=DEV[6], ntiles=plan.ntiles, tile_faces=plan.tile_faces.copy(), tile_faces_dev=DEV[7], tile_face_ints=plan.tile_faces.size,
             ramp=ramp, ramp_dev=DEV[8], ramp_len=int(ramp.size), stream=None)
    return a


def color_args(plan, aa=False):
    return Args(crop=DEV[0], restored=DEV[1], out=DEV[2], F=plan.n, S=plan.S, mode=1, levels=5, items=_copy(plan.crop_items), items_dev=DEV[5],
                tables=plan.crop_tables.copy(), tables_dev=DEV[3], table_ints=plan.crop_tables.size, scratch=DEV[9],
                scratch_bytes=12 * plan.n * S * S, stream=None)


def setter(**kw):
    def f(a):
        for k, v in kw.items():
            a[k] = v(a) if callable(v) else v
    return f


def item(i, **kw):
    """set fields of item i; i = "filtered": the first item with reach > 0; a callable value gets (item, args)"""
    def f(a):
        it = a["items"][next(k for k, x in enumerate(a["items"]) if x.reach > 0) if i == "filtered" else i]
        for k, v in kw.items():
            setattr(it, k, v(it, a) if callable(v) else v)
    return f


def table(name, off_field, value, i=0):
    """one entry of item i's tables (`tables` through tab_off, `fwd` through fwd_off)"""
    def f(a):
        it = a["items"][next(k for k, x in enumerate(a["items"]) if x.reach > 0) if i == "filtered" else i]
        a[name][getattr(it, off_field) + 1] = value
    return f


def tile(k, **kw):
    """set fields of tile k; k = "second photo": the first tile of the second photo; k = "two faces": the first tile with two faces"""
    def f(a):
        ts = a["tiles"]
        j = {"second photo": lambda: next(j for j in range(a["ntiles"]) if ts[j].dst_off != ts[0].dst_off),
             "two faces": lambda: next(j for j in range(a["ntiles"]) if ts[j].nfaces > 1)}.get(k, lambda: k)()
        for name, v in kw.items():
            setattr(ts[j], name, v(ts[j], a) if callable(v) else v)
    return f


def repeat_tile(a):
    C.memmove(C.addressof(a["tiles"][1]), C.addressof(a["tiles"][0]), C.sizeof(photo.FaceTile))


def descending_row(a):
    ts = a["tiles"]
    k = next(k for k in range(1, a["ntiles"]) if ts[k].dst_off == ts[k - 1].dst_off and ts[k].y0 > ts[k - 1].y0)
    keep = _copy(ts)
    C.memmove(C.addressof(ts[k]), C.addressof(keep[k - 1]), C.sizeof(photo.FaceTile))
    C.memmove(C.addressof(ts[k - 1]), C.addressof(keep[k]), C.sizeof(photo.FaceTile))


def tile_face(k, value, second=False):
    """the first (or second) entry of tile k's face list"""
    def f(a):
        ts = a["tiles"]
        j = next(j for j in range(a["ntiles"]) if ts[j].nfaces > 1) if k == "two faces" else k
        a["tile_faces"][ts[j].face0 + (1 if second else 0)] = value(a["tile_faces"][ts[j].face0], a) if callable(value) else value
    return f


def box_leaves(axis):
    def f(a):
        t = a["tiles"][0]
        it = a["items"][a["tile_faces"][t.face0]]
        if axis == "x":
            it.x0 = t.w - it.nx + 1
        else:
            it.y0 = t.h - it.ny + 1
    return f


BIG = 1 << 30


def common_cases(aa):
    """(id, mutation, code, fragment): the checks crop and paste share"""
    cases = [("n below 0", setter(n=-1), EINVAL, "0..65535 faces (got -1)"), ("n above 65535", setter(n=65536), EINVAL, "faces (got 65536)"),
             ("S of 0", setter(S=0), EINVAL, "crop side 1..8192 (got 0)"), ("S of 8193", setter(S=8193), EINVAL, "crop side 1..8192 (got 8193)"),
             ("tables_dev misaligned", setter(tables_dev=DEV[3] + 2), EINVAL, "misaligned"),
             ("items_dev misaligned", setter(items_dev=DEV[5] + 4), EINVAL, "misaligned"),
             ("tab_off past the tables", item(2, tab_off=lambda it, a: a.table_ints - 2 * it.nx - 2 * it.ny + 1), EINVAL, "face 2: tables outside the"),
             ("tab_off negative", item(0, tab_off=-1), EINVAL, "face 0: tables outside the"),
             ("table entry 2^30", table("tables", "tab_off", BIG, 1), EINVAL, "face 1: table overflow (entry 1 = 1073741824"),
             ("table entry -2^30", table("tables", "tab_off", -BIG, 2), EINVAL, "face 2: table overflow (entry 1 = -1073741824")]
    for name in ("tables", "tables_dev", "items", "items_dev"):
        cases.append((f"{name} null", setter(**{name: None}), EINVAL, "null pointer"))
    if aa:
        cases += [("fwd without fwd_dev", setter(fwd_dev=None), EINVAL, "null pointer"), ("fwd_dev without fwd", setter(fwd=None), EINVAL, "null pointer"),
                  ("fwd_dev misaligned", setter(fwd_dev=DEV[4] + 2), EINVAL, "misaligned"),
                  ("fwd of 2 GiB", setter(fwd_ints=1 << 29), EINVAL, "tables must"),
                  ("reach of -1", item(1, reach=-1), EINVAL, "face 1: reach -1"),
                  ("reach of 24", item(2, reach=24), ENOTSUP, "face 2: reach 24 above 23"),
                  ("no forward tables for a filtered face", setter(fwd=None, fwd_dev=None), EINVAL, "null pointer (forward tables of face"),
                  ("source range empty", item("filtered", snx=0), EINVAL, "source range of 0 x"),
                  ("source range too wide", item("filtered", sny=(1 << 18) + 1), EINVAL, "source range of"),
                  ("source range at 2^30", item("filtered", sx0=BIG), EINVAL, "source range at (1073741824"),
                  ("source range at -2^30", item("filtered", sy0=-BIG), EINVAL, "source range at ("),
                  ("fwd_off past the buffer", item("filtered", fwd_off=lambda it, a: it.fwd_off + 1), EINVAL, "forward tables outside the"),
                  ("fwd_off negative", item("filtered", fwd_off=-1), EINVAL, "forward tables outside the"),
                  ("forward entry 2^30", table("fwd", "fwd_off", BIG, "filtered"), EINVAL, "table overflow (forward entry 1 = 1073741824"),
                  ("forward entry -2^30", table("fwd", "fwd_off", -BIG, "filtered"), EINVAL, "table overflow (forward entry 1 = -1073741824"),
                  ("source range short on the left", item("filtered", sx0=lambda it, a: it.sx0 + 1), EINVAL, "source range too small"),
                  ("source range short on the right", item("filtered", snx=lambda it, a: it.snx - 1), EINVAL, "source range too small"),
                  ("source range short at the top", item("filtered", sy0=lambda it, a: it.sy0 + 1), EINVAL, "source range too small"),
                  ("source range short at the bottom", item("filtered", sny=lambda it, a: it.sny - 1), EINVAL, "source range too small")]
    return cases


def crop_cases(aa):
    cases = common_cases(aa) + [
        ("border of 256", setter(bg=256), EINVAL, "border colour outside 0..255"), ("border of -1", setter(bb=-1), EINVAL, "border colour outside 0..255"),
        ("no output", setter(out_u8=None, out_f32=None), EINVAL, "null pointer (no output)"), ("src null", setter(src=None), EINVAL, "null pointer"),
        ("out_f32 misaligned", setter(out_f32=DEV[1] + 2), EINVAL, "misaligned"),
        ("photos of 2 GiB", setter(src_bytes=1 << 31), EINVAL, "must stay below 2 GiB"),
        ("output of 2^31 elements", setter(n=11, S=8192), EINVAL, "(11 faces of 8192 x 8192)"),
        ("photo size 0", item(1, w=0), EINVAL, "face 1: photo size 0 x"),
        ("src_off past the buffer", item(2, src_off=lambda it, a: a.src_bytes - 3 * it.w * it.h + 1), EINVAL, "face 2: photo outside the"),
        ("src_off negative", item(0, src_off=-1), EINVAL, "face 0: photo outside the"),
        ("nx != S", item(1, nx=S - 1), EINVAL, "face 1: tables of 15 x 16"), ("ny != S", item(0, ny=S + 1), EINVAL, "face 0: tables of 16 x 17")]
    if aa:
        cases += [("x0 != 0", item(1, x0=1), EINVAL, "face 1: tables of 16 x 16 at (1, 0) for a crop of side 16"),
                  ("y0 != 0", item(2, y0=-1), EINVAL, "at (0, -1)")]
    return cases


def paste_cases(aa):
    cases = common_cases(aa) + [
        ("ntiles below 0", setter(ntiles=-1), EINVAL, "-1 tiles"),
        ("ramp null", setter(ramp=None), EINVAL, "null pointer (ramp)"), ("ramp_dev null", setter(ramp_dev=None), EINVAL, "null pointer (ramp)"),
        ("ramp of 0", setter(ramp_len=0), EINVAL, "ramp of 1..65536 entries (got 0)"),
        ("ramp of 65537", setter(ramp_len=65537), EINVAL, "ramp of 1..65536 entries (got 65537)"),
        ("ramp[0] != 0", lambda a: a.ramp.__setitem__(0, 1), EINVAL, "ramp[0] != 0"),
        ("ramp entry of 257", lambda a: a.ramp.__setitem__(a.ramp.size - 1, 257), EINVAL, f"ramp[{photo.default_ramp(1, 2).size - 1}] = 257 above 256"),
        ("tiles_dev misaligned", setter(tiles_dev=DEV[6] + 4), EINVAL, "misaligned"),
        ("tile_faces_dev misaligned", setter(tile_faces_dev=DEV[7] + 2), EINVAL, "misaligned"),
        ("ramp_dev misaligned", setter(ramp_dev=DEV[8] + 1), EINVAL, "misaligned"),
        ("photos of 2 GiB", setter(photo_bytes=1 << 31), EINVAL, "stay below 2 GiB"), ("crops of 2 GiB", setter(crop_bytes=1 << 31), EINVAL, "stay below 2 GiB"),
        ("w != S", item(1, w=S + 1), EINVAL, "face 1: its source is the 16 x 16 crop (got 17 x 16)"),
        ("h != S", item(0, h=S - 1), EINVAL, "face 0: its source is the 16 x 16 crop (got 16 x 15)"),
        ("crop outside crop_bytes", item(2, src_off=lambda it, a: it.src_off + 1), EINVAL, "face 2: crop outside the"),
        ("crop before crop_bytes", item(0, src_off=-1), EINVAL, "face 0: crop outside the"),
        ("negative box x", item(1, x0=-1), EINVAL, "face 1: bounding box at (-1,"), ("negative box y", item(2, y0=-2), EINVAL, ", -2)"),
        ("table extents above 8192", item(1, nx=8193), EINVAL, "face 1: table extents 8193 x"),
        ("table extents below 0", item(0, ny=-1), EINVAL, "face 0: table extents"),
        ("tile photo outside photo_bytes", tile("second photo", dst_off=lambda t, a: t.dst_off + 1), EINVAL, "photo outside the"),
        ("tile photo before photo_bytes", tile(0, dst_off=-1), EINVAL, "tile 0: photo outside the"),
        ("tile photo of no size", tile(1, h=0), EINVAL, "tile 1: photo outside the"),
        ("tile origin not a multiple of 32", tile(0, x0=lambda t, a: t.x0 + 16), EINVAL, "tile 0 at ("),
        ("tile origin negative", tile(0, y0=-32), EINVAL, "tile 0 at ("),
        ("tile origin outside the photo", tile(1, x0=lambda t, a: (t.w + 31) // 32 * 32), EINVAL, "tile 1 at ("),
        ("tile origin below the photo", tile(1, y0=lambda t, a: (t.h + 31) // 32 * 32), EINVAL, "tile 1 at ("),
        ("tile repeated", repeat_tile, EINVAL, "tile 1: tiles must ascend"), ("tile rows descend", descending_row, EINVAL, "tiles must ascend"),
        ("photos overlap", tile("second photo", dst_off=lambda t, a: t.dst_off - 3), EINVAL, "tiles must ascend"),
        ("photo changes size between its tiles", tile(1, h=lambda t, a: t.h + 1), EINVAL, "tile 1: tiles must ascend"),
        ("nfaces of 0", tile(2, nfaces=0), EINVAL, "tile 2: face list outside the"),
        ("face list outside its buffer", tile(1, face0=lambda t, a: a.tile_face_ints - t.nfaces + 1), EINVAL, "tile 1: face list outside the"),
        ("face list before its buffer", tile(0, face0=-1), EINVAL, "tile 0: face list outside the"),
        ("face index of n", tile_face(0, 3), EINVAL, "tile 0: faces must be 0..2 in list order"),
        ("face index of -1", tile_face(1, -1), EINVAL, "tile 1: faces must be 0..2 in list order"),
        ("face list not ascending", tile_face("two faces", lambda first, a: first, second=True), EINVAL, "faces must be 0..2 in list order"),
        ("box leaves the photo in x", box_leaves("x"), EINVAL, "tile 0: face 0's bounding box leaves the photo"),
        ("box leaves the photo in y", box_leaves("y"), EINVAL, "tile 0: face 0's bounding box leaves the photo")]
    for name in ("photos", "crops", "tiles", "tiles_dev", "tile_faces", "tile_faces_dev"):
        cases.append((f"{name} null", setter(**{name: None}), EINVAL, "null pointer"))
    if aa:
        cases += [("filtered destination beyond 2^20 in x", item("filtered", x0=lambda it, a: (1 << 20) - it.nx + 1), EINVAL, "must stay below 2^20"),
                  ("filtered destination beyond 2^20 in y", item("filtered", y0=lambda it, a: (1 << 20) - it.ny + 1), EINVAL, "must stay below 2^20")]
    return cases


def color_cases(aa=False):
    nb = 3 * 3 * S * S
    cases = [("unknown mode", setter(mode=2), EINVAL, "unknown mode 2"), ("levels of 0", setter(levels=0), EINVAL, "levels 1..6 (got 0)"),
             ("levels of 7", setter(levels=7), EINVAL, "levels 1..6 (got 7)"), ("F below 0", setter(F=-1), EINVAL, "faces (got -1)"),
             ("F above 65535", setter(F=65536), EINVAL, "faces (got 65536)"), ("S of 0", setter(S=0), EINVAL, "crop side 1..8192 (got 0)"),
             ("S of 8193", setter(S=8193), EINVAL, "crop side 1..8192 (got 8193)"),
             ("stats side above its maximum", setter(mode=0, S=1025), ENOTSUP, "crop side up to 1024 (got 1025)"),
             ("crops of 2 GiB", setter(F=11, S=8192), EINVAL, "below 2 GiB (11 faces of 8192 x 8192)"),
             ("scratch too small", setter(scratch_bytes=lambda a: a.scratch_bytes - 1), EINVAL, "scratch too small (9215 bytes, 9216 needed)"),
             ("stats scratch too small", setter(mode=0, scratch_bytes=383), EINVAL, "scratch too small (383 bytes, 384 needed)"),
             ("scratch misaligned", setter(scratch=DEV[9] + 8), EINVAL, "misaligned scratch"),
             ("out overlaps the crop", setter(out=DEV[0] + nb - 1), EINVAL, "out overlaps an input"),
             ("out overlaps restored in part", setter(out=DEV[1] + 4), EINVAL, "out overlaps an input"),
             ("scratch overlaps out", setter(scratch=DEV[2] + 16), EINVAL, "scratch overlaps a crop buffer"),
             ("scratch overlaps the crop", setter(scratch=DEV[0] - 16), EINVAL, "scratch overlaps a crop buffer"),
             ("scratch overlaps restored", setter(scratch=DEV[1] + nb - 16), EINVAL, "scratch overlaps a crop buffer"),
             ("tables_dev misaligned", setter(tables_dev=DEV[3] + 2), EINVAL, "misaligned tables or items"),
             ("items_dev misaligned", setter(items_dev=DEV[5] + 4), EINVAL, "misaligned tables or items"),
             ("tables of 2 GiB", setter(table_ints=1 << 29), EINVAL, "the tables must stay below 2 GiB"),
             ("photo size 0", item(1, h=0), EINVAL, "face 1: photo size"), ("nx != S", item(2, nx=S - 1), EINVAL, "face 2: tables of 15 x 16 for a crop of side 16"),
             ("ny != S", item(0, ny=S + 1), EINVAL, "face 0: tables of 16 x 17"),
             ("tab_off past the tables", item(2, tab_off=lambda it, a: a.table_ints - 4 * S + 1), EINVAL, "face 2: tables outside the"),
             ("tab_off negative", item(1, tab_off=-1), EINVAL, "face 1: tables outside the"),
             ("table entry 2^30", table("tables", "tab_off", BIG, 1), EINVAL, "face 1: table overflow (entry 1 = 1073741824, magnitude 2^30 or more)"),
             ("table entry -2^30", table("tables", "tab_off", -BIG, 2), EINVAL, "face 2: table overflow (entry 1 = -1073741824")]
    for name in ("crop", "restored", "out", "scratch"):
        cases.append((f"{name} null", setter(**{name: None}), EINVAL, "color_fix: null pointer"))
    for name in ("items", "items_dev", "tables", "tables_dev"):
        cases.append((f"{name} alone missing", setter(**{name: None}), EINVAL, "all four or none"))
    return cases


# entry -> (symbol, prefix, arguments, cases, takes an anti-aliased plan)
ENTRIES = {"face_crop": ("vsp_face_crop_u8", "face_crop: ", crop_args, crop_cases, False),
           "face_crop_aa": ("vsp_face_crop_aa_u8", "face_crop_aa: ", crop_args, crop_cases, True),
           "face_paste": ("vsp_face_paste_u8", "face_paste: ", paste_args, paste_cases, False),
           "face_paste_aa": ("vsp_face_paste_aa_u8", "face_paste_aa: ", paste_args, paste_cases, True),
           "color_fix": ("vsp_color_fix_u8", "color_fix: ", color_args, color_cases, False)}


def _call(symbol, a):
    from vspbfr_amd import _lib
    rc = getattr(_lib.lib, symbol)(*[_raw(v) for v in a.values()])
    return rc, _lib.last_error()


@pytest.mark.parametrize("entry", list(ENTRIES))
def test_every_refusal_names_its_entry_and_its_reason(plans, entry):
    symbol, prefix, make, cases, aa = ENTRIES[entry]
    assert len({c[0] for c in cases(aa)}) == len(cases(aa))
    wrong = []
    for name, mutate, code, fragment in cases(aa):
        a = make(plans[aa], aa)
        mutate(a)
        rc, msg = _call(symbol, a)
        if rc != code or not msg.startswith(prefix) or fragment not in msg:
            wrong.append((name, rc, msg))
    assert not wrong, wrong


def test_nothing_to_do_returns_ok(plans):
    for entry, empty in (("face_crop", dict(n=0)), ("face_crop_aa", dict(n=0)), ("face_paste", dict(n=0)), ("face_paste", dict(ntiles=0)),
                         ("face_paste_aa", dict(n=0)), ("face_paste_aa", dict(ntiles=0)), ("color_fix", dict(F=0))):
        symbol, _, make, _, aa = ENTRIES[entry]
        a = make(plans[aa], aa)
        a.update(empty)
        assert _call(symbol, a)[0] == 0, (entry, empty)
    # the early return comes after the checks of counts, sides and ramp, before the pointers are looked at
    symbol, prefix, make, _, _ = ENTRIES["face_paste_aa"]
    a = make(plans[True], True)
    a.update(ntiles=0, photos=None, tiles=None)
    assert _call(symbol, a)[0] == 0
    a.update(ramp_len=0)
    rc, msg = _call(symbol, a)
    assert rc == EINVAL and msg.startswith(prefix) and "ramp of" in msg
