"""GPU checks of vsp_color_fix_u8 (csrc/color_fix.hip through vspbfr_amd/photo.py): the kernels' bytes equal the NumPy restatement
(tests/color_fix_ref.py) for both modes -- S = 64, 37 (odd: tile and vector tails), 9 (below the largest stride: both clamps at once), 1
and 512; 1, 2, 5 and 6 levels; validity from the plans of test_photo_gpu.py's ragged batch (a face off every edge, one wholly outside),
bilinear and anti-aliased, and without a plan; out aliasing restored; position independence; a second stream; the refusals.  The inputs
are random bytes with a smooth tone shift, so that the fix moves most bytes.  Equality everywhere: no tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

import color_fix_ref as CF
import photo_ref as R
from test_photo_gpu import FACES, SIZES

pytestmark = pytest.mark.gpu
DEV = "cuda"
MODES = ["wavelet", "stats"]
SHAPES = [(3, 64), (2, 37), (1, 9), (1, 1), (2, 512)]


def _dev(a):
    return torch.from_numpy(np.array(a, copy=True)).to(DEV)


def _fix(c, r, mode, **kw):
    from vspbfr_amd import photo as P
    return P.color_fix(_dev(c), _dev(r), mode, **kw).cpu().numpy()


@pytest.mark.parametrize("F,S", SHAPES)
@pytest.mark.parametrize("mode", MODES)
def test_bytes_equal_the_restatement(mode, F, S):
    c, r = CF.toned_pair(F, S, seed=100 + S)
    ref = CF.fix_batch(c, r, mode)
    got = _fix(c, r, mode)
    moved = float((ref != r).mean())
    print(f"{mode} F={F} S={S}: differing bytes {int((got != ref).sum())}, moved by the fix {moved:.3f}")
    assert np.array_equal(got, ref)
    assert S == 1 or moved > 0.5                      # an identity kernel cannot pass


@pytest.mark.parametrize("F,S", [(2, 37), (1, 9), (3, 64), (1, 132)])
@pytest.mark.parametrize("levels", [1, 2, 3, 6])
def test_wavelet_levels(levels, F, S):
    c, r = CF.toned_pair(F, S, seed=200 + S + levels)
    ref = CF.fix_batch(c, r, "wavelet", levels=levels)
    got = _fix(c, r, "wavelet", levels=levels)
    print(f"wavelet levels={levels} F={F} S={S}: differing bytes {int((got != ref).sum())}")
    assert np.array_equal(got, ref)


def test_extremes_and_closed_forms_on_the_device():
    S = 64
    hi, lo = np.full((1, S, S, 3), 255, dtype=np.uint8), np.zeros((1, S, S, 3), dtype=np.uint8)
    for mode in MODES:
        assert np.array_equal(_fix(hi, lo, mode, levels=6), hi) and np.array_equal(_fix(lo, hi, mode, levels=6), lo)
    c, r = CF.toned_pair(1, S, seed=3)
    flat = np.full_like(c, 90)
    for a, b in ((c, flat), (flat, c), (c, c)):       # the gain clamps at both ends; equal inputs
        assert np.array_equal(_fix(a, b, "stats"), CF.fix_batch(a, b, "stats"))
        assert np.array_equal(_fix(a, b, "wavelet"), CF.fix_batch(a, b, "wavelet"))


@pytest.fixture(scope="module")
def ragged():
    """the sixteen faces over the six ragged photos: per plan kind the device crops, a restored batch derived from them, the validity
    masks of the restatement and the reference outputs; computed once and never written to"""
    from vspbfr_amd import photo as P
    S = 64
    photos = [R.test_photo(w, h, seed=11 + k) for k, (w, h) in enumerate(SIZES)]
    faces = [(k, R.landmarks_for(sc, ang, c, S)) for k, sc, ang, c in FACES]
    valid = [CF.validity_from_landmarks(pts, S, SIZES[k][0], SIZES[k][1]) for k, pts in faces]
    rng = np.random.default_rng(5)
    out = dict(S=S, photos=photos, faces=faces, valid=valid)
    for aa in (False, True):
        plan = P.FacePlan(photos, faces, size=S, antialias=aa)
        crops = P.crop_faces(plan, DEV)[0]
        c = crops.cpu().numpy()
        r = np.clip(np.rint(0.7 * c.astype(np.float64) + 40 + rng.normal(0, 8, c.shape)), 0, 255).astype(np.uint8)
        ref = {m: CF.fix_batch(c, r, m, valid) for m in MODES}
        for a in [c, r] + list(ref.values()):
            a.setflags(write=False)
        out[aa] = dict(plan=plan, crops=crops, c=c, r=r, ref=ref)
    return out


@pytest.mark.parametrize("antialias", [False, True])
@pytest.mark.parametrize("mode", MODES)
def test_validity_from_plans_over_the_ragged_batch(ragged, mode, antialias):
    from vspbfr_amd import photo as P
    d, valid = ragged[antialias], ragged["valid"]
    kinds = [("all" if v.all() else "none" if not v.any() else "some") for v in valid]
    assert kinds.count("none") == 1 and kinds[7] == "none" and kinds.count("some") >= 7 and kinds.count("all") >= 1
    got = P.color_fix(d["crops"], _dev(d["r"]), mode, plan=d["plan"], device=DEV).cpu().numpy()
    for i in range(16):
        print(f"{mode} aa={antialias} face {i} ({kinds[i]}, {int(valid[i].sum())} valid): differing bytes {int((got[i] != d['ref'][mode][i]).sum())}")
    assert np.array_equal(got, d["ref"][mode])
    assert np.array_equal(got[7], d["r"][7])          # wholly outside: N = 0, the restored crop
    # The border colour changes no output byte of a face that hangs off the LEFT or the TOP of its photo (2, 4, 14) or lies outside (7):
    # there a valid centre cell has all four taps inside.  Off the right or the bottom the last valid cell's second tap reads the
    # border -- validity is a rule about the centre cell, not about every tap -- so those faces are not part of this claim.
    other = P.crop_faces(d["plan"], DEV, border=(255, 0, 31))[0]
    pick = [2, 4, 7, 14]
    assert all(not torch.equal(other[i], d["crops"][i]) for i in pick) and [kinds[i] for i in pick] == ["some", "some", "none", "some"]
    assert np.array_equal(P.color_fix(other, _dev(d["r"]), mode, plan=d["plan"], device=DEV).cpu().numpy()[pick], got[pick])
    # without the plan the border does tint the face
    assert not np.array_equal(P.color_fix(d["crops"], _dev(d["r"]), mode).cpu().numpy(), got)


@pytest.mark.parametrize("mode", MODES)
def test_without_a_plan_every_pixel_is_valid(ragged, mode):
    d = ragged[False]
    assert np.array_equal(_fix(d["c"], d["r"], mode), CF.fix_batch(d["c"], d["r"], mode))


@pytest.mark.parametrize("levels", [1, 5])
@pytest.mark.parametrize("mode", MODES)
def test_out_may_be_the_restored_tensor(ragged, mode, levels):
    from vspbfr_amd import photo as P
    d = ragged[False]
    ref = d["ref"][mode] if levels == 5 else CF.fix_batch(d["c"], d["r"], mode, ragged["valid"], levels)
    r = _dev(d["r"])
    back = P.color_fix(d["crops"], r, mode, plan=d["plan"], device=DEV, levels=levels, out=r)
    assert back is r and np.array_equal(r.cpu().numpy(), ref)
    c, r2 = CF.toned_pair(2, 132, seed=9)              # several tiles a side, vector path
    t = _dev(r2)
    P.color_fix(_dev(c), t, mode, levels=levels, out=t)
    assert np.array_equal(t.cpu().numpy(), CF.fix_batch(c, r2, mode, levels=levels))


@pytest.mark.parametrize("mode", MODES)
def test_one_face_alone_equals_the_same_face_at_position_eleven(ragged, mode):
    from vspbfr_amd import photo as P
    d = ragged[False]
    plan = P.FacePlan([ragged["photos"][5]], [(0, ragged["faces"][10][1])], size=ragged["S"])
    crops = P.crop_faces(plan, DEV)[0]
    assert np.array_equal(crops.cpu().numpy()[0], d["c"][10])
    got = P.color_fix(crops, _dev(d["r"][10:11]), mode, plan=plan, device=DEV).cpu().numpy()
    assert np.array_equal(got[0], d["ref"][mode][10])


@pytest.mark.parametrize("mode", MODES)
def test_a_repeat_on_a_second_stream_gives_equal_bytes(ragged, mode):
    from vspbfr_amd import photo as P
    d = ragged[True]
    r = _dev(d["r"])
    first = P.color_fix(d["crops"], r, mode, plan=d["plan"], device=DEV)
    torch.cuda.synchronize()
    s = torch.cuda.Stream()
    with torch.cuda.stream(s):
        second = P.color_fix(d["crops"], r, mode, plan=d["plan"], device=DEV)
    s.synchronize()
    assert torch.equal(first, second) and np.array_equal(second.cpu().numpy(), d["ref"][mode])


def test_refusals_return_the_error_code_and_write_nothing(ragged):
    from vspbfr_amd import _lib
    from vspbfr_amd import photo as P
    d, S, F = ragged[False], ragged["S"], 16
    plan = d["plan"]
    dev = plan.upload(DEV)
    crops, r = d["crops"], _dev(d["r"])
    out = torch.full_like(r, 0xA5)
    scratch = torch.empty(12 * F * S * S, dtype=torch.uint8, device=DEV)
    items_h, tabs_h = C.cast(plan.crop_items, C.c_void_p), plan.crop_tables.ctypes.data_as(C.c_void_p)
    items_d, tabs_d = C.c_void_p(dev["crop_items"].data_ptr()), C.c_void_p(dev["crop_tables"].data_ptr())
    p = lambda t: C.c_void_p(t.data_ptr())
    base = dict(crop=p(crops), restored=p(r), out=p(out), F=F, S=S, mode=1, levels=5, items=items_h, items_dev=items_d, tables=tabs_h,
                tables_dev=tabs_d, table_ints=plan.crop_tables.size, scratch=p(scratch), scratch_bytes=scratch.numel())

    def call(**kw):
        a = dict(base, **kw)
        return _lib.lib.vsp_color_fix_u8(a["crop"], a["restored"], a["out"], a["F"], a["S"], a["mode"], a["levels"], a["items"], a["items_dev"],
                                         a["tables"], a["tables_dev"], a["table_ints"], a["scratch"], a["scratch_bytes"], None)

    bad_items = (_lib.FaceItem * F)()
    C.memmove(bad_items, plan.crop_items, C.sizeof(bad_items))
    bad_items[3].tab_off = plan.crop_tables.size - 4 * S + 1
    bad_extent = (_lib.FaceItem * F)()
    C.memmove(bad_extent, plan.crop_items, C.sizeof(bad_extent))
    bad_extent[5].nx = S - 1
    bad_photo = (_lib.FaceItem * F)()
    C.memmove(bad_photo, plan.crop_items, C.sizeof(bad_photo))
    bad_photo[0].w = 0
    big = plan.crop_tables.copy()
    big[2 * S + 1] = 1 << 30
    cases = [(dict(crop=None), -1, "null pointer"), (dict(restored=None), -1, "null pointer"), (dict(out=None), -1, "null pointer"),
             (dict(scratch=None), -1, "null pointer"), (dict(S=0), -1, "crop side"), (dict(S=8193), -1, "crop side"), (dict(F=-1), -1, "faces"),
             (dict(levels=0), -1, "levels"), (dict(levels=7), -1, "levels"), (dict(mode=2), -1, "unknown mode"), (dict(mode=-1), -1, "unknown mode"),
             (dict(F=60000, S=512, items=None, items_dev=None, tables=None, tables_dev=None), -1, "2 GiB"),
             (dict(F=4000, S=256, items=None, items_dev=None, tables=None, tables_dev=None), -1, "2 GiB"),       # the scratch alone
             (dict(scratch_bytes=12 * F * S * S - 1), -1, "scratch too small"), (dict(mode=0, scratch_bytes=128 * F - 1), -1, "scratch too small"),
             (dict(scratch=C.c_void_p(scratch.data_ptr() + 8)), -1, "misaligned scratch"),
             (dict(out=C.c_void_p(r.data_ptr() + 3)), -1, "overlaps"), (dict(out=p(crops)), -1, "overlaps"),
             (dict(scratch=p(r)), -1, "scratch overlaps"), (dict(scratch=C.c_void_p(crops.data_ptr() + 16)), -1, "scratch overlaps"),
             (dict(tables_dev=C.c_void_p(dev["crop_tables"].data_ptr() + 2)), -1, "misaligned tables or items"),
             (dict(items_dev=C.c_void_p(dev["crop_items"].data_ptr() + 4)), -1, "misaligned tables or items"),
             (dict(items=None), -1, "all four or none"), (dict(tables_dev=None), -1, "all four or none"),
             (dict(items=C.cast(bad_items, C.c_void_p)), -1, "tables outside"), (dict(table_ints=plan.crop_tables.size - 1), -1, "tables outside"),
             (dict(items=C.cast(bad_extent, C.c_void_p)), -1, "for a crop of side"), (dict(items=C.cast(bad_photo, C.c_void_p)), -1, "photo size"),
             (dict(tables=big.ctypes.data_as(C.c_void_p)), -1, "table overflow"),
             (dict(mode=0, S=1025, items=None, items_dev=None, tables=None, tables_dev=None), -3, "statistics")]
    for kw, code, text in cases:
        rc = call(**kw)
        print(f"refusal {sorted(kw)}: code {rc}, {_lib.last_error()!r}")
        assert rc == code and text in _lib.last_error(), (kw, rc, _lib.last_error())
    torch.cuda.synchronize()
    assert bool((out == 0xA5).all()) and np.array_equal(r.cpu().numpy(), d["r"])
    assert call(F=0) == 0 and bool((out == 0xA5).all())
    assert call() == 0                                   # and the same arguments unspoilt are served
    assert np.array_equal(out.cpu().numpy(), d["ref"]["wavelet"])
    with pytest.raises(ValueError):
        P.color_fix(crops, r, "adain")
    with pytest.raises(ValueError):
        P.color_fix(crops, r, "wavelet", levels=7)
    with pytest.raises(RuntimeError):
        P.color_fix(crops, r[:, :, :32], "wavelet")
    with pytest.raises(RuntimeError):
        P.color_fix(crops.cpu(), r, "stats")
