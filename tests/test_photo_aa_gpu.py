"""GPU checks of vsp_face_crop_aa_u8 / vsp_face_paste_aa_u8 (csrc/face_warp.hip through vspbfr_amd/photo.py): the kernels' bytes
equal the NumPy restatement tests/photo_aa_ref.py, which sums over a window one wider than the kernels' and derives its own similarity,
tables and reach from the landmarks.  Twelve faces over five ragged photos with minifications 0.37 .. 4 at four turns, over every edge,
two corners and entirely outside, both border colours; the largest minification at S = 16; S = 512; S = 63 (byte stores); pastes at 2 and
3.4; a filtered and a bilinear face overlapping in both orders; upscale 2; the fp32 output; position independence; a second stream; plans
whose every reach is 0 against the old entries; the refusals.  Equality everywhere: no tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

import photo_aa_ref as AA
import photo_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
S = 64

SIZES = [(67, 131), (300, 280), (1, 40), (290, 37), (50, 50)]          # (w, h); the last one has no face
# (photo, crop minification, degrees, centre): 12 faces in paste order.  The paste minification is the inverse: face 8 is filtered there.
FACES = [(1, 4.0, 17.0, (150.0, 140.0)),       # 256 px of a 300 x 280 photo
         (1, 2.9, -163.0, (100.0, 120.0)),
         (1, 1.3, 0.0, (0.0, 140.0)),          # over the left edge
         (1, 1.3, 45.0, (299.0, 100.0)),       # over the right edge
         (1, 2.9, 0.0, (150.0, 2.0)),          # over the top edge
         (1, 1.0, 17.0, (150.0, 278.0)),       # over the bottom edge
         (1, 1.3, 17.0, (298.0, 278.0)),       # over the bottom right corner
         (1, 1.0, 0.0, (-900.0, 30.0)),        # entirely outside
         (0, 0.37, 17.0, (33.0, 65.0)),        # a 24 px face: magnified into the crop, minified 2.7 times on the way back
         (0, 4.0, -163.0, (30.0, 60.0)),       # larger than its photo: over all four edges at once
         (2, 2.9, 0.0, (0.0, 20.0)),           # on the one-pixel-wide photo
         (3, 1.3, 45.0, (3.0, 3.0))]           # over the top left corner


def _photos(sizes=SIZES):
    return [R.test_photo(w, h, seed=31 + k) for k, (w, h) in enumerate(sizes)]


def _faces(which, size=S):
    return [(k, R.landmarks_for(1.0 / m, ang, c, size)) for k, m, ang, c in which]


def _restored(n, size=S):
    return np.stack([R.test_photo(size, size, seed=201 + i) for i in range(n)])


def _ref_crops(photos, faces, size, border=(128, 128, 128)):
    return np.stack([AA.crop(photos[k], R.similarity(pts, size), size, border) for k, pts in faces])


def _ref_paste(base, faces, restored, size, upscale=1, ramp=None):
    out = []
    for k, b in enumerate(base):
        mine = [(restored[i], R.paste_matrix(R.similarity(pts, size), upscale)) for i, (kk, pts) in enumerate(faces) if kk == k]
        out.append(AA.paste(b, mine, size, ramp))
    return out


def _run(photos, faces, size=S, upscale=1, ramp=None, base=None, restored=None, f32=True, border=(128, 128, 128), antialias=True):
    """one crop launch and one paste launch -> (plan, crops u8, crops f32 or None, [output photo], restored)"""
    from vspbfr_amd import photo as P
    plan = P.FacePlan(photos, faces, size=size, upscale=upscale, antialias=antialias)
    u8, f = P.crop_faces(plan, DEV, u8=True, f32=f32, border=border)
    restored = _restored(len(faces), size) if restored is None else restored
    out = None
    if base is not None:
        out = torch.from_numpy(np.concatenate([b.reshape(-1) for b in base])).to(DEV)
    out = P.paste_faces(plan, torch.from_numpy(restored).to(DEV), DEV, ramp=ramp, out=out)
    return plan, u8.cpu().numpy(), (None if f is None else f.cpu().numpy()), [o.cpu().numpy() for o in plan.split(out)], restored


@pytest.fixture(scope="module")
def twelve():
    """the 12-face batch over the five ragged photos, run once; the references computed once and never written to"""
    photos, faces = _photos(), _faces(FACES)
    plan, u8, f32, out, restored = _run(photos, faces)
    ref_c = _ref_crops(photos, faces, S)
    ref_p = _ref_paste(photos, faces, restored, S)
    for a in [ref_c] + ref_p:
        a.setflags(write=False)
    return dict(photos=photos, faces=faces, plan=plan, u8=u8, f32=f32, out=out, restored=restored, ref_c=ref_c, ref_p=ref_p)


def test_twelve_faces_over_ragged_photos_crop(twelve):
    plan, u8, ref = twelve["plan"], twelve["u8"], twelve["ref_c"]
    reach = [plan.crop_aa_items[i].reach for i in range(12)]
    print("crop minify", [round(m, 3) for m in plan.crop_minify], "reach", reach)
    assert plan.n == 12 and sorted({round(m, 2) for m in plan.crop_minify}) == [0.37, 1.0, 1.3, 2.9, 4.0]
    assert reach[8] == 0 and all(reach[i] > 0 for i in (0, 1, 2, 3, 4, 6, 9, 10, 11)) and max(reach) <= 7
    for i in range(12):
        print(f"crop face {i}: differing bytes {int((u8[i] != ref[i]).sum())}, border pixels {int((ref[i] == 128).all(axis=2).sum())}")
    assert np.array_equal(u8, ref)
    assert np.all(u8[7] == 128)                                                   # entirely outside: the border colour
    for i in (2, 3, 4, 5, 6, 9, 11):                                              # over an edge: some border, some photo
        inside = (ref[i] != 128).any(axis=2)
        assert inside.any() and not inside.all(), i
    plain = np.stack([R.crop(twelve["photos"][k], R.invert(R.similarity(pts, S)), S) for k, pts in twelve["faces"]])
    assert np.array_equal(u8[8], plain[8]) and not np.array_equal(u8[0], plain[0])   # the filter changes the minified faces only


def test_second_border_colour(twelve):
    from vspbfr_amd import photo as P
    u8, _ = P.crop_faces(twelve["plan"], DEV, border=(255, 0, 77))
    pick = [0, 3, 7, 9, 10]
    ref = _ref_crops(twelve["photos"], [twelve["faces"][i] for i in pick], S, (255, 0, 77))
    assert np.array_equal(u8.cpu().numpy()[pick], ref)
    assert np.all(ref[2] == np.array([255, 0, 77]))


def test_fp32_output_is_the_normalised_uint8(twelve):
    assert np.array_equal(twelve["f32"].view(np.int32), R.to_f32(twelve["u8"]).view(np.int32))
    from vspbfr_amd import photo as P
    _, only = P.crop_faces(twelve["plan"], DEV, u8=False, f32=True)
    assert np.array_equal(only.cpu().numpy().view(np.int32), twelve["f32"].view(np.int32))


def test_twelve_faces_over_ragged_photos_paste(twelve):
    plan = twelve["plan"]
    reach = [plan.paste_aa_items[i].reach for i in range(12)]
    print("paste minify", [round(m, 3) for m in plan.paste_minify], "reach", reach)
    assert reach[8] > 0 and reach[7] == 0 and reach[0] == 0
    for k, (got, ref) in enumerate(zip(twelve["out"], twelve["ref_p"])):
        print(f"paste photo {k} {got.shape}: differing bytes {int((got != ref).sum())}, changed {int((ref != twelve['photos'][k]).any(axis=2).sum())} px")
        assert np.array_equal(got, ref), k
    assert np.array_equal(twelve["out"][4], twelve["photos"][4])
    for k in (0, 1, 2, 3):
        assert not np.array_equal(twelve["out"][k], twelve["photos"][k]), k


def test_one_face_alone_equals_the_same_face_at_position_nine(twelve):
    photos = [twelve["photos"][0]]
    faces = _faces([(0,) + FACES[9][1:]])
    plan, u8, f32, out, _ = _run(photos, faces, restored=twelve["restored"][9:10])
    assert plan.n == 1 and np.array_equal(u8[0], twelve["u8"][9]) and np.array_equal(f32[0].view(np.int32), twelve["f32"][9].view(np.int32))
    assert np.array_equal(out[0], AA.paste(photos[0], [(twelve["restored"][9], R.similarity(faces[0][1], S))], S))
    # position 8 of 12, the face whose paste is filtered, alone on the photo it shares with face 9
    faces = _faces([(0,) + FACES[8][1:]])
    _, u8, _, out, _ = _run(photos, faces, restored=twelve["restored"][8:9])
    assert np.array_equal(u8[0], twelve["u8"][8])
    assert np.array_equal(out[0], AA.paste(photos[0], [(twelve["restored"][8], R.similarity(faces[0][1], S))], S))


def test_largest_minification_at_side_16():
    photo = R.test_photo(300, 280, seed=41)
    faces = [(0, R.landmarks_for(1.0 / 16.0, 0.0, (150.0, 140.0), 16)), (0, R.landmarks_for(1.0 / 15.99, 45.0, (150.0, 140.0), 16))]
    plan, u8, f32, out, restored = _run([photo], faces, size=16)
    assert [plan.crop_aa_items[i].reach for i in range(2)] == [17, 23] and round(plan.crop_minify[0], 9) == 16.0
    ref = _ref_crops([photo], faces, 16)
    print(f"m 16: differing bytes {int((u8 != ref).sum())}")
    assert np.array_equal(u8, ref) and np.array_equal(f32.view(np.int32), R.to_f32(u8).view(np.int32))
    assert np.array_equal(out[0], _ref_paste([photo], faces, restored, 16)[0])


def test_one_face_at_512():
    photo = R.test_photo(1700, 1600, seed=42)
    faces = [(0, R.landmarks_for(1.0 / 2.9, 17.0, (830.0, 800.0), 512))]
    plan, u8, f32, _, _ = _run([photo], faces, size=512, restored=np.zeros((1, 512, 512, 3), dtype=np.uint8))
    ref = _ref_crops([photo], faces, 512)
    print(f"S = 512, m 2.9, reach {plan.crop_aa_items[0].reach}: differing bytes {int((u8 != ref).sum())}")
    assert np.array_equal(u8, ref) and np.array_equal(f32.view(np.int32), R.to_f32(u8).view(np.int32))


def test_side_63_takes_the_byte_stores():
    photo = R.test_photo(300, 280, seed=43)
    faces = [(0, R.landmarks_for(1.0 / 2.9, 17.0, (150.0, 140.0), 63)), (0, R.landmarks_for(2.0, -163.0, (60.0, 200.0), 63))]
    plan, u8, f32, out, restored = _run([photo], faces, size=63)
    assert np.array_equal(u8, _ref_crops([photo], faces, 63)) and np.array_equal(f32.view(np.int32), R.to_f32(u8).view(np.int32))
    assert plan.paste_aa_items[1].reach > 0 and np.array_equal(out[0], _ref_paste([photo], faces, restored, 63)[0])


def test_paste_into_faces_of_32_and_19_pixels():
    photo = R.test_photo(131, 97, seed=44)
    faces = [(0, R.landmarks_for(2.0, 0.0, (40.0, 40.0), S)), (0, R.landmarks_for(3.4, 17.0, (100.0, 60.0), S))]
    hard = np.array([0, 128, 256], dtype=np.uint16)                               # the default ramp leaves nothing of a 19 px face
    plan, _, _, out, restored = _run([photo], faces, ramp=hard, f32=False)
    assert [round(m, 2) for m in plan.paste_minify] == [2.0, 3.4] and all(plan.paste_aa_items[i].reach > 0 for i in range(2))
    ref = AA.paste(photo, [(restored[i], R.similarity(pts, S)) for i, (_, pts) in enumerate(faces)], S, hard)
    plain = R.paste(photo, [(restored[i], R.similarity(pts, S)) for i, (_, pts) in enumerate(faces)], S, hard)
    print(f"paste at 2 and 3.4: differing bytes {int((out[0] != ref).sum())}; pixels the filter changes {int((ref != plain).any(axis=2).sum())}")
    assert np.array_equal(out[0], ref) and not np.array_equal(ref, plain) and not np.array_equal(ref, photo)


def test_a_filtered_and_a_bilinear_face_overlap_in_both_orders():
    photo = R.test_photo(160, 120, seed=45)
    a, b = (0, 0.5, 17.0, (70.0, 60.0)), (0, 1.25, -10.0, (90.0, 60.0))           # paste of a: minified by 2 (filtered); of b: magnified
    restored = _restored(2)
    hard = np.array([0, 64, 128, 256], dtype=np.uint16)
    outs = []
    for order in ((a, b), (b, a)):
        faces = _faces(order)
        rs = restored if order[0] is a else restored[::-1].copy()
        plan, u8, _, out, _ = _run([photo], faces, restored=rs, ramp=hard, f32=False)
        ia = 0 if order[0] is a else 1
        assert plan.paste_aa_items[ia].reach > 0 and plan.paste_aa_items[1 - ia].reach == 0
        assert plan.crop_aa_items[ia].reach == 0 and plan.crop_aa_items[1 - ia].reach > 0
        assert np.array_equal(u8, _ref_crops([photo], faces, S))
        assert np.array_equal(out[0], _ref_paste([photo], faces, rs, S, ramp=hard)[0])
        outs.append(out[0])
    assert not np.array_equal(outs[0], outs[1])


def test_upscale_two_pastes_into_the_doubled_photo(twelve):
    photos, faces = twelve["photos"], twelve["faces"]
    base = [np.ascontiguousarray(np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)) for p in photos]
    plan, u8, _, out, restored = _run(photos, faces, upscale=2, base=base, restored=twelve["restored"], f32=False)
    assert np.array_equal(u8, twelve["ref_c"])                                    # the crop reads the photo itself
    assert plan.paste_aa_items[8].reach > 0 and round(plan.paste_minify[8], 2) == 1.35
    ref = _ref_paste(base, faces, restored, S, upscale=2)
    for k in range(len(photos)):
        print(f"upscale 2 photo {k}: differing bytes {int((out[k] != ref[k]).sum())}")
        assert np.array_equal(out[k], ref[k]), k


def test_second_launch_and_second_stream_give_the_same_bytes(twelve):
    from vspbfr_amd import photo as P
    plan = twelve["plan"]
    restored = torch.from_numpy(twelve["restored"]).to(DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        runs = []
        for _ in range(2):
            u8, f32 = P.crop_faces(plan, DEV, u8=True, f32=True)
            runs.append((u8, f32, P.paste_faces(plan, restored, DEV)))
    side.synchronize()
    for u8, f32, out in runs:
        assert np.array_equal(u8.cpu().numpy(), twelve["u8"]) and np.array_equal(f32.cpu().numpy().view(np.int32), twelve["f32"].view(np.int32))
        for got, want in zip(plan.split(out), twelve["out"]):
            assert np.array_equal(got.cpu().numpy(), want)


def test_plans_whose_every_reach_is_zero_equal_the_old_entries(twelve):
    from vspbfr_amd import photo as P
    photos, faces, restored = twelve["photos"], twelve["faces"], twelve["restored"]
    _, old_u8, old_f32, old_out, _ = _run(photos, faces, restored=restored, antialias=False)
    plan = P.FacePlan(photos, faces, size=S, antialias=True)
    for i in range(plan.n):                                                       # before pack(): the items travel as they are now
        plan.crop_aa_items[i].reach = plan.paste_aa_items[i].reach = 0
    u8, f32 = P.crop_faces(plan, DEV, u8=True, f32=True)
    out = P.paste_faces(plan, torch.from_numpy(restored).to(DEV), DEV)
    assert np.array_equal(u8.cpu().numpy(), old_u8) and np.array_equal(f32.cpu().numpy().view(np.int32), old_f32.view(np.int32))
    for got, want in zip(plan.split(out), old_out):
        assert np.array_equal(got.cpu().numpy(), want)
    assert not np.array_equal(old_u8, twelve["u8"])
    # a plan that needs no filter at all (every face magnified into the crop, pasted at upscale 4): no forward tables, NULL pointers
    small = [(k, R.landmarks_for(2.0, ang, c, S)) for k, _, ang, c in FACES[:4]]
    base = [np.ascontiguousarray(np.repeat(np.repeat(p, 4, axis=0), 4, axis=1)) for p in photos]
    plan, u8, _, out, rs = _run(photos, small, upscale=4, base=base, f32=False)
    assert plan.crop_fwd.size == 0 and plan.paste_fwd.size == 0
    _, old_u8, _, old_out, _ = _run(photos, small, upscale=4, base=base, restored=rs, f32=False, antialias=False)
    assert np.array_equal(u8, old_u8) and all(np.array_equal(a, b) for a, b in zip(out, old_out))


def test_refusals_return_the_error_code_and_write_nothing(twelve):
    from vspbfr_amd import _lib, hip_ops as H
    from vspbfr_amd import photo as P
    photos, faces = twelve["photos"], twelve["faces"]
    restored = torch.from_numpy(twelve["restored"].copy()).to(DEV)

    def fresh():
        plan = P.FacePlan(photos, faces, size=S, antialias=True)
        return plan, plan.upload(DEV)

    def crop(plan, dev):
        return H.face_crop_aa_u8(plan, dev["crop_aa_items"], dev["crop_tables"], dev["crop_fwd"], dev["photos"])

    before = fresh()[0].background(DEV)
    out = before.clone()
    # reach 24: not served
    plan, dev = fresh()
    plan.crop_aa_items[0].reach = 24
    with pytest.raises(RuntimeError, match="code -3"):
        crop(plan, dev)
    assert "reach 24" in _lib.last_error()
    plan.crop_aa_items[0].reach = -1
    with pytest.raises(RuntimeError, match="code -1"):
        crop(plan, dev)
    plan, dev = fresh()
    plan.paste_aa_items[8].reach = 24
    with pytest.raises(RuntimeError, match="code -3"):
        P.paste_faces(plan, restored, DEV, out=out)
    # a source range that does not hold every window: one column short at either end, one row short, a reach one larger than planned
    for field, delta in (("snx", -1), ("sny", -1), ("sx0", 1), ("sy0", 1), ("reach", 1)):
        plan, dev = fresh()
        setattr(plan.crop_aa_items[1], field, getattr(plan.crop_aa_items[1], field) + delta)
        with pytest.raises(RuntimeError, match="code -1"):
            crop(plan, dev)
        assert "source range too small" in _lib.last_error() or "forward tables outside" in _lib.last_error(), (field, _lib.last_error())
    plan, dev = fresh()
    plan.paste_aa_items[8].sx0 += 1
    with pytest.raises(RuntimeError, match="code -1"):
        P.paste_faces(plan, restored, DEV, out=out)
    assert "source range too small" in _lib.last_error()
    # forward tables outside their buffer, a forward entry of magnitude 2^30, and the old tables' overflow
    plan, dev = fresh()
    plan.crop_aa_items[11].fwd_off += 1
    with pytest.raises(RuntimeError, match="code -1"):
        crop(plan, dev)
    assert "forward tables outside" in _lib.last_error()
    for value in (1 << 30, -(1 << 30)):
        plan, dev = fresh()
        plan.crop_fwd[3] = value
        with pytest.raises(RuntimeError, match="code -1"):
            crop(plan, dev)
        assert "overflow" in _lib.last_error()
    plan, dev = fresh()
    plan.paste_fwd[-1] = 1 << 30
    with pytest.raises(RuntimeError, match="code -1"):
        P.paste_faces(plan, restored, DEV, out=out)
    assert "overflow" in _lib.last_error()
    plan, dev = fresh()
    plan.crop_tables[5] = 1 << 30
    with pytest.raises(RuntimeError, match="code -1"):
        crop(plan, dev)
    assert "overflow" in _lib.last_error()
    torch.cuda.synchronize()
    assert torch.equal(out, before)                                               # nothing was launched
    # null pointers, straight at the C entries
    plan, dev = fresh()
    o8 = torch.full((plan.n, S, S, 3), 7, dtype=torch.uint8, device=DEV)
    args = [o8.data_ptr(), None, dev["photos"].data_ptr(), plan.src_bytes, plan.crop_tables.ctypes.data_as(C.c_void_p), dev["crop_tables"].data_ptr(),
            plan.crop_tables.size, plan.crop_fwd.ctypes.data_as(C.c_void_p), dev["crop_fwd"].data_ptr(), plan.crop_fwd.size,
            C.cast(plan.crop_aa_items, C.c_void_p), dev["crop_aa_items"].data_ptr(), plan.n, S, 128, 128, 128, None]
    for hole in (2, 4, 5, 7, 8, 10, 11):
        bad = list(args)
        bad[hole] = None
        assert _lib.lib.vsp_face_crop_aa_u8(*bad) == -1 and "null pointer" in _lib.last_error(), hole
    bad = list(args)
    bad[7] = bad[8] = None                                                        # no forward tables at all, yet faces with a reach
    assert _lib.lib.vsp_face_crop_aa_u8(*bad) == -1 and "null pointer" in _lib.last_error()
    bad = list(args)
    bad[0] = None
    assert _lib.lib.vsp_face_crop_aa_u8(*bad) == -1 and "no output" in _lib.last_error()
    ramp = P.default_ramp()
    assert _lib.lib.vsp_face_paste_aa_u8(out.data_ptr(), plan.out_bytes, restored.data_ptr(), restored.numel(), None, None, 0, None, None, 0, None,
                                         None, plan.n, S, None, None, plan.ntiles, None, None, 0, ramp.ctypes.data_as(C.c_void_p), None,
                                         ramp.size, None) == -1
    assert "null pointer" in _lib.last_error()
    torch.cuda.synchronize()
    assert torch.equal(out, before) and bool((o8 == 7).all())
    # and the untouched plan still runs
    u8, _ = P.crop_faces(plan, DEV)
    assert np.array_equal(u8.cpu().numpy(), twelve["ref_c"])
