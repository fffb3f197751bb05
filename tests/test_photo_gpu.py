"""GPU checks of vsp_face_crop_u8 / vsp_face_paste_u8 (csrc/face_warp.hip through vspbfr_amd/photo.py): the kernels' bytes equal the
NumPy restatement (tests/photo_ref.py, which derives its own similarity, inverse, tables and bounding boxes from the landmarks) for crop
and paste -- ragged photos whose rows sit off dword alignment, a 1-pixel-wide and a 1100-pixel-wide photo, S = 64 and 512, scales 0.37
and 2.9, rotations 17 and -163 degrees, faces over every edge, over a corner and entirely outside, 1 / 5 / 16 faces, overlaps in both
orders, upscale 2, a one-entry ramp, position independence, repeats, a second stream, the fp32 output, and the refusals.  Equality
everywhere: no tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

import photo_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
S = 64

# (w, h) of the photos of the ragged batch: rows of 3 w bytes off dword alignment, one pixel wide, 1100 wide, one without a face
SIZES = [(67, 131), (130, 65), (1, 40), (1100, 37), (50, 50), (90, 80)]
# (photo, scale source px -> crop px, degrees, centre): 16 faces in paste order
FACES = [(0, 0.37, 17.0, (33.0, 65.0)),        # larger than its photo: over all four edges at once
         (0, 2.9, -163.0, (30.0, 60.0)),       # small, well inside, overlapped by face 0
         (0, 1.0, 17.0, (0.0, 60.0)),          # over the left edge
         (0, 1.0, -163.0, (66.0, 70.0)),       # over the right edge
         (0, 1.3, 0.0, (33.0, 2.0)),           # over the top edge
         (0, 1.3, 5.0, (33.0, 129.0)),         # over the bottom edge
         (1, 1.0, 17.0, (128.0, 63.0)),        # over the bottom right corner
         (1, 1.0, 0.0, (-500.0, 30.0)),        # entirely outside
         (1, 0.8, -10.0, (50.0, 30.0)),
         (1, 0.8, 10.0, (70.0, 34.0)),         # overlaps face 8
         (5, 1.1, 17.0, (45.0, 40.0)),         # position 11 of 16, alone on its photo
         (2, 2.9, 0.0, (0.0, 20.0)),           # on the one-pixel-wide photo
         (3, 0.37, -163.0, (550.0, 18.0)),
         (3, 2.9, 17.0, (1090.0, 30.0)),
         (3, 1.0, 0.0, (5.0, 5.0)),            # over the top left corner
         (1, 0.37, 17.0, (65.0, 32.0))]


def _photos(sizes=SIZES):
    return [R.test_photo(w, h, seed=11 + k) for k, (w, h) in enumerate(sizes)]


def _faces(which, size=S):
    return [(k, R.landmarks_for(sc, ang, c, size)) for k, sc, ang, c in which]


def _restored(n, size=S):
    return np.stack([R.test_photo(size, size, seed=101 + i) for i in range(n)])


def _ref_crops(photos, faces, size, border=(128, 128, 128)):
    return np.stack([R.crop(photos[k], R.invert(R.similarity(pts, size)), size, border) for k, pts in faces])


def _ref_paste(base, faces, restored, size, upscale=1, ramp=None):
    """per photo: photo_ref.paste of its faces in list order onto base[k]"""
    out = []
    for k, b in enumerate(base):
        mine = [(restored[i], R.paste_matrix(R.similarity(pts, size), upscale)) for i, (kk, pts) in enumerate(faces) if kk == k]
        out.append(R.paste(b, mine, size, ramp))
    return out


def _run(photos, faces, size=S, upscale=1, ramp=None, base=None, restored=None, f32=True):
    """one crop launch and one paste launch -> (plan, crops u8, crops f32 or None, [output photo], restored)"""
    from vspbfr_amd import photo as P
    plan = P.FacePlan(photos, faces, size=size, upscale=upscale)
    u8, f = P.crop_faces(plan, DEV, u8=True, f32=f32)
    restored = _restored(len(faces), size) if restored is None else restored
    out = None
    if base is not None:
        out = torch.from_numpy(np.concatenate([b.reshape(-1) for b in base])).to(DEV)
    out = P.paste_faces(plan, torch.from_numpy(restored).to(DEV), DEV, ramp=ramp, out=out)
    return plan, u8.cpu().numpy(), (None if f is None else f.cpu().numpy()), [o.cpu().numpy() for o in plan.split(out)], restored


@pytest.fixture(scope="module")
def sixteen():
    """the 16-face batch over the six ragged photos, run once; reference computed once and never written to"""
    photos, faces = _photos(), _faces(FACES)
    plan, u8, f32, out, restored = _run(photos, faces)
    ref_c = _ref_crops(photos, faces, S)
    ref_p = _ref_paste(photos, faces, restored, S)
    for a in [ref_c] + ref_p:
        a.setflags(write=False)
    return dict(photos=photos, faces=faces, plan=plan, u8=u8, f32=f32, out=out, restored=restored, ref_c=ref_c, ref_p=ref_p)


def test_sixteen_faces_over_ragged_photos_crop(sixteen):
    plan, u8, ref = sixteen["plan"], sixteen["u8"], sixteen["ref_c"]
    assert plan.n == 16 and len({o % 4 for o in plan.src_off}) >= 3              # photos off dword alignment in the packed buffer
    for i in range(16):
        print(f"crop face {i}: differing bytes {int((u8[i] != ref[i]).sum())}, border pixels {int((ref[i] == 128).all(axis=2).sum())}")
    assert np.array_equal(u8, ref)
    assert np.all(u8[7] == 128)                                                   # the face entirely outside: the border colour
    for i in (0, 2, 3, 4, 5, 6, 14):                                              # over an edge: some border, some photo
        inside = (ref[i] != 128).any(axis=2)
        assert inside.any() and not inside.all(), i


def test_fp32_output_is_the_normalised_uint8(sixteen):
    assert np.array_equal(sixteen["f32"].view(np.int32), R.to_f32(sixteen["u8"]).view(np.int32))
    from vspbfr_amd import photo as P
    _, only = P.crop_faces(sixteen["plan"], DEV, u8=False, f32=True)
    assert np.array_equal(only.cpu().numpy().view(np.int32), sixteen["f32"].view(np.int32))


def test_sixteen_faces_over_ragged_photos_paste(sixteen):
    plan = sixteen["plan"]
    sizes = {(plan.boxes[i][2] - plan.boxes[i][0], plan.boxes[i][3] - plan.boxes[i][1]) for i in range(16)}
    assert any(w % 32 and h % 32 for w, h in sizes) and plan.boxes[7] == (0, 0, 0, 0)
    assert any(t.nfaces >= 3 for t in plan.tiles[:plan.ntiles])                   # tiles that walk several faces
    for k, (got, ref) in enumerate(zip(sixteen["out"], sixteen["ref_p"])):
        print(f"paste photo {k} {got.shape}: differing bytes {int((got != ref).sum())}, changed {int((ref != sixteen['photos'][k]).any(axis=2).sum())} px")
        assert np.array_equal(got, ref), k
    assert np.array_equal(sixteen["out"][4], sixteen["photos"][4])                # the photo without a face
    for k in (0, 1, 2, 3, 5):
        assert not np.array_equal(sixteen["out"][k], sixteen["photos"][k]), k


def test_one_face_alone_equals_the_same_face_at_position_eleven(sixteen):
    photos = [sixteen["photos"][5]]
    faces = _faces([(0,) + FACES[10][1:]])
    plan, u8, f32, out, _ = _run(photos, faces, restored=sixteen["restored"][10:11])
    assert plan.n == 1
    assert np.array_equal(u8[0], sixteen["u8"][10]) and np.array_equal(f32[0].view(np.int32), sixteen["f32"][10].view(np.int32))
    assert np.array_equal(out[0], sixteen["out"][5]) and np.array_equal(out[0], sixteen["ref_p"][5])


def test_five_faces_over_three_photos_one_without_a_face(sixteen):
    photos = [sixteen["photos"][0], sixteen["photos"][4], sixteen["photos"][1]]
    pick = [0, 1, 6, 8, 9]
    remap = {0: 0, 1: 2}
    faces = _faces([(remap[FACES[i][0]],) + FACES[i][1:] for i in pick])
    plan, u8, _, out, restored = _run(photos, faces, restored=sixteen["restored"][pick])
    assert plan.n == 5 and np.array_equal(u8, sixteen["ref_c"][pick])
    ref = _ref_paste(photos, faces, restored, S)
    for k in range(3):
        assert np.array_equal(out[k], ref[k]), k
    assert np.array_equal(out[1], photos[1])


def test_overlapping_faces_in_both_orders_at_512():
    photo = R.test_photo(333, 270, seed=5)
    a, b = (0, 2.9, 17.0, (120.0, 130.0)), (0, 2.5, -163.0, (200.0, 140.0))
    restored = _restored(2, 512)
    outs = []
    for order in ((a, b), (b, a)):
        faces = _faces(order, 512)
        rs = restored if order[0] is a else restored[::-1].copy()
        plan, u8, f32, out, _ = _run([photo], faces, size=512, restored=rs)
        ref_c = _ref_crops([photo], faces, 512)
        print(f"S=512 crop: differing bytes {int((u8 != ref_c).sum())}; paste: {int((out[0] != _ref_paste([photo], faces, rs, 512)[0]).sum())}")
        assert np.array_equal(u8, ref_c) and np.array_equal(f32.view(np.int32), R.to_f32(u8).view(np.int32))
        assert np.array_equal(out[0], _ref_paste([photo], faces, rs, 512)[0])
        outs.append(out[0])
    assert not np.array_equal(outs[0], outs[1])


def test_upscale_two_pastes_into_the_doubled_photo(sixteen):
    photos, faces = sixteen["photos"], sixteen["faces"]
    base = [np.ascontiguousarray(np.repeat(np.repeat(p, 2, axis=0), 2, axis=1)) for p in photos]
    plan, u8, _, out, restored = _run(photos, faces, upscale=2, base=base, restored=sixteen["restored"], f32=False)
    assert np.array_equal(u8, sixteen["ref_c"])                                   # the crop reads the photo itself: upscale does not enter
    ref = _ref_paste(base, faces, restored, S, upscale=2)
    for k in range(len(photos)):
        assert out[k].shape == (2 * photos[k].shape[0], 2 * photos[k].shape[1], 3)
        print(f"upscale 2 photo {k}: differing bytes {int((out[k] != ref[k]).sum())}")
        assert np.array_equal(out[k], ref[k]), k


def test_custom_ramps(sixteen):
    photos, faces = sixteen["photos"][:2], [f for f in sixteen["faces"] if f[0] < 2]
    rs = sixteen["restored"][:len(faces)]
    _, _, _, out, _ = _run(photos, faces, ramp=np.zeros(1, dtype=np.uint16), restored=rs, f32=False)      # L = 1: every weight is ramp[0] = 0
    assert np.array_equal(out[0], photos[0]) and np.array_equal(out[1], photos[1])
    hard = np.array([0, 256], dtype=np.uint16)                                                             # L = 2: replace from 1/8 px inside
    _, _, _, out, _ = _run(photos, faces, ramp=hard, restored=rs, f32=False)
    ref = _ref_paste(photos, faces, rs, S, ramp=hard)
    assert np.array_equal(out[0], ref[0]) and np.array_equal(out[1], ref[1])
    steps = (np.arange(37) * 7 % 257).astype(np.uint16)                                                    # not monotonic, every index reached
    steps[0] = 0
    _, _, _, out, _ = _run(photos, faces, ramp=steps, restored=rs, f32=False)
    ref = _ref_paste(photos, faces, rs, S, ramp=steps)
    assert np.array_equal(out[0], ref[0]) and np.array_equal(out[1], ref[1])


def test_second_launch_and_second_stream_give_the_same_bytes(sixteen):
    from vspbfr_amd import photo as P
    plan = sixteen["plan"]
    restored = torch.from_numpy(sixteen["restored"]).to(DEV)
    torch.cuda.synchronize()
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        runs = []
        for _ in range(2):
            u8, f32 = P.crop_faces(plan, DEV, u8=True, f32=True)
            runs.append((u8, f32, P.paste_faces(plan, restored, DEV)))
    side.synchronize()
    for u8, f32, out in runs:
        assert np.array_equal(u8.cpu().numpy(), sixteen["u8"]) and np.array_equal(f32.cpu().numpy().view(np.int32), sixteen["f32"].view(np.int32))
        for got, want in zip(plan.split(out), sixteen["out"]):
            assert np.array_equal(got.cpu().numpy(), want)


def test_refusals_return_the_error_code_and_write_nothing(sixteen):
    from vspbfr_amd import _lib, hip_ops as H
    from vspbfr_amd import photo as P
    photos, faces = sixteen["photos"][:2], [f for f in sixteen["faces"] if f[0] < 2]
    restored = torch.from_numpy(sixteen["restored"][:len(faces)].copy()).to(DEV)
    # a table entry of magnitude 2^30: crop and paste
    plan = P.FacePlan(photos, faces, size=S)
    dev = plan.upload(DEV)
    plan.crop_tables[5] = 1 << 30
    with pytest.raises(RuntimeError, match="code -1"):
        H.face_crop_u8(plan, dev["crop_items"], dev["crop_tables"], dev["photos"])
    assert "overflow" in _lib.last_error()
    plan.crop_tables[5] = -(1 << 30)
    with pytest.raises(RuntimeError, match="code -1"):
        H.face_crop_u8(plan, dev["crop_items"], dev["crop_tables"], dev["photos"])
    plan = P.FacePlan(photos, faces, size=S)
    before = plan.background(DEV)
    out = before.clone()
    plan.paste_tables[-1] = 1 << 30
    with pytest.raises(RuntimeError, match="code -1"):
        P.paste_faces(plan, restored, DEV, out=out)
    assert "overflow" in _lib.last_error()
    # ramp[0] != 0, a ramp value above 256
    plan = P.FacePlan(photos, faces, size=S)
    for ramp, word in ((np.array([1, 256], dtype=np.uint16), r"ramp\[0\]"), (np.array([0, 257], dtype=np.uint16), "above 256")):
        with pytest.raises(RuntimeError, match="code -1"):
            P.paste_faces(plan, restored, DEV, ramp=ramp, out=out)
        import re
        assert re.search(word, _lib.last_error())
    torch.cuda.synchronize()
    assert torch.equal(out, before)                                               # nothing was launched
    # null pointers, straight at the C entries
    dev = plan.upload(DEV)
    tab = plan.crop_tables.ctypes.data_as(C.c_void_p)
    items = C.cast(plan.crop_items, C.c_void_p)
    o8 = torch.empty((plan.n, S, S, 3), dtype=torch.uint8, device=DEV)
    args = [o8.data_ptr(), None, dev["photos"].data_ptr(), plan.src_bytes, tab, dev["crop_tables"].data_ptr(), plan.crop_tables.size, items,
            dev["crop_items"].data_ptr(), plan.n, S, 128, 128, 128, None]
    for hole in (2, 4, 5, 7, 8):
        bad = list(args)
        bad[hole] = None
        assert _lib.lib.vsp_face_crop_u8(*bad) == -1 and "null pointer" in _lib.last_error(), hole
    bad = list(args)
    bad[0] = None
    assert _lib.lib.vsp_face_crop_u8(*bad) == -1 and "no output" in _lib.last_error()
    ramp = P.default_ramp()
    assert _lib.lib.vsp_face_paste_u8(out.data_ptr(), plan.out_bytes, restored.data_ptr(), restored.numel(), None, None, 0, None, None, plan.n, S,
                                      None, None, plan.ntiles, None, None, 0, ramp.ctypes.data_as(C.c_void_p), None, ramp.size, None) == -1
    assert "null pointer" in _lib.last_error()
    torch.cuda.synchronize()
    assert torch.equal(out, before)
    # and the untouched plan still runs
    u8, _ = P.crop_faces(plan, DEV)
    assert np.array_equal(u8.cpu().numpy(), sixteen["ref_c"][[i for i, f in enumerate(sixteen["faces"]) if f[0] < 2]])
