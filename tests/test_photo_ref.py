"""CPU checks of the whole-photo face path's definition (tests/photo_ref.py) in closed form, and of the host side of the product
(vspbfr_amd/photo.py: geometry, tables, plan) against it.  Equality everywhere except the float64 Umeyama fit (1e-9)."""
import ctypes as C

import numpy as np
import pytest

import photo_ref as R


def _M(a=1.0, b=0.0, tx=0.0, c=0.0, d=1.0, ty=0.0):
    return np.array([[a, b, tx], [c, d, ty]], dtype=np.float64)


@pytest.fixture(scope="module")
def photo():
    p = R.test_photo(90, 70, seed=3)
    p.setflags(write=False)
    return p


def test_identity_crops_the_window_byte_for_byte(photo):
    assert np.array_equal(R.crop(photo, _M(), 48), photo[:48, :48])


def test_integer_translation_crops_at_an_offset(photo):
    assert np.array_equal(R.crop(photo, _M(tx=17.0, ty=9.0), 40), photo[9:49, 17:57])


def test_quarter_turn_equals_rot90():
    sq = R.test_photo(33, 33, seed=4)
    # crop (x, y) reads photo (y, 32 - x): out[y, x] = sq[32 - x, y] = rot90(sq, -1)[y, x]
    assert np.array_equal(R.crop(sq, _M(a=0.0, b=1.0, tx=0.0, c=-1.0, d=0.0, ty=32.0), 33), np.rot90(sq, -1))
    assert np.array_equal(R.crop(sq, _M(a=0.0, b=-1.0, tx=32.0, c=1.0, d=0.0, ty=0.0), 33), np.rot90(sq, 1))


def test_half_pixel_shift_is_the_rounded_mean_of_the_neighbours(photo):
    p = photo.astype(np.int64)
    assert np.array_equal(R.crop(photo, _M(tx=0.5), 40), ((p[:40, :40] + p[:40, 1:41] + 1) >> 1).astype(np.uint8))
    assert np.array_equal(R.crop(photo, _M(ty=0.5), 40), ((p[:40, :40] + p[1:41, :40] + 1) >> 1).astype(np.uint8))


def test_taps_outside_the_photo_read_the_border_colour(photo):
    border = (7, 200, 99)
    got = R.crop(photo, _M(tx=-10.0, ty=-6.0), 32, border)
    assert np.array_equal(got[6:, 10:], photo[:26, :22])
    assert np.all(got[:6] == np.array(border, dtype=np.uint8)) and np.all(got[:, :10] == np.array(border, dtype=np.uint8))
    far = R.crop(photo, _M(tx=1000.0, ty=-500.0), 16)
    assert np.all(far == 128)
    # half a pixel over the right edge: the mean of the last column and the border
    edge = R.crop(photo, _M(tx=89.5), 4, (0, 0, 0))
    assert np.array_equal(edge[:, 0], ((photo[:4, 89].astype(np.int64) + 1) >> 1).astype(np.uint8)) and np.all(edge[:, 1:] == 0)


def test_umeyama_recovers_a_known_similarity_and_never_mirrors():
    from vspbfr_amd import photo as P
    rng = np.random.default_rng(0)
    src = rng.uniform(0, 500, (5, 2))
    s, th, t = 1.7, np.deg2rad(-37.0), np.array([31.5, -12.25])
    Rm = np.array([[np.cos(th), -np.sin(th)], [np.sin(th), np.cos(th)]])
    want = np.concatenate([s * Rm, t[:, None]], axis=1)
    assert np.abs(R.umeyama(src, src @ (s * Rm).T + t) - want).max() < 1e-9
    # the product's fit against the template: recover the similarity that was applied to the template
    A = P.similarity_from_landmarks((R.FFHQ512_TEMPLATE - t) @ Rm / s)
    assert np.abs(A - want).max() < 1e-9
    assert np.abs(A - R.similarity((R.FFHQ512_TEMPLATE - t) @ Rm / s)).max() < 1e-12
    # mirrored landmarks: still a proper rotation with one positive scale
    mirrored = R.FFHQ512_TEMPLATE * np.array([-1.0, 1.0]) + np.array([600.0, 0.0])
    for A in (R.similarity(mirrored), P.similarity_from_landmarks(mirrored)):
        L = A[:, :2]
        assert np.linalg.det(L) > 0
        sc = np.sqrt(np.linalg.det(L))
        assert np.abs(L.T @ L - sc * sc * np.eye(2)).max() < 1e-9


def test_template_landmarks_give_the_identity():
    from vspbfr_amd import photo as P
    assert np.array_equal(P.FFHQ512_TEMPLATE, R.FFHQ512_TEMPLATE)
    for size in (512, 64):
        t = R.FFHQ512_TEMPLATE * (size / 512.0)
        for A in (R.similarity(t, size), P.similarity_from_landmarks(t, size=size)):
            assert np.abs(A - _M()).max() < 1e-9


def test_bad_landmarks_are_refused_by_name():
    from vspbfr_amd import photo as P
    t = R.FFHQ512_TEMPLATE
    bad = t.copy()
    bad[2, 1] = np.nan
    for pts, word in ((bad, "finite"), (t[:4], "shape"), (np.zeros((5, 2)) + 3.0, "degenerate")):
        with pytest.raises(ValueError, match=word) as e:
            P.similarity_from_landmarks(pts, photo="dir/a.png", face=2)
        assert "dir/a.png" in str(e.value) and "face 2" in str(e.value)
    with pytest.raises(ValueError, match="b.png.*face 1"):
        P.FacePlan([np.zeros((8, 8, 3), np.uint8)] * 2, [(1, t), (1, bad)], names=["a.png", "b.png"])


def test_paste_with_a_full_ramp_replaces_the_window_and_an_empty_one_keeps_the_photo(photo):
    S = 32
    restored = R.test_photo(S, S, seed=9)
    P = _M(tx=-20.0, ty=-11.0)                     # output (x, y) -> crop (x - 20, y - 11)
    full = np.full(5, 256, dtype=np.uint16)
    full[0] = 0                                    # the interface's rule; d >> 2 == 0 only within 1/8 px of the border: never at integers > 0
    got = R.paste(photo, [(restored, P)], S, full)
    want = np.array(photo)
    want[12:11 + S - 1, 21:20 + S - 1] = restored[1:S - 1, 1:S - 1]       # the border ring has d = 0 -> ramp[0] = 0 -> background
    assert np.array_equal(got, want)
    assert np.array_equal(R.paste(photo, [(restored, P)], S, np.zeros(9, dtype=np.uint16)), photo)
    assert np.array_equal(R.paste(photo, [(restored, P)], S, np.zeros(1, dtype=np.uint16)), photo)


def test_crop_then_paste_at_identity_returns_the_photo(photo):
    S = 40
    A = _M(tx=-13.0, ty=-8.0)
    c = R.crop(photo, R.invert(A), S)
    assert np.array_equal(c, photo[8:48, 13:53])
    assert np.array_equal(R.paste(photo, [(c, R.paste_matrix(A))], S), photo)
    ramp = np.full(3, 256, dtype=np.uint16)
    ramp[0] = 0
    assert np.array_equal(R.paste(photo, [(c, R.paste_matrix(A))], S, ramp), photo)


def test_overlapping_faces_depend_on_their_order(photo):
    S = 32
    a, b = np.full((S, S, 3), 10, dtype=np.uint8), np.full((S, S, 3), 240, dtype=np.uint8)
    Pa, Pb = _M(tx=-10.0, ty=-10.0), _M(tx=-22.0, ty=-16.0)
    ramp = R.default_ramp(2, 6)
    ab, ba = R.paste(photo, [(a, Pa), (b, Pb)], S, ramp), R.paste(photo, [(b, Pb), (a, Pa)], S, ramp)
    assert not np.array_equal(ab, ba)
    # deep inside both faces the later one wins outright
    assert np.all(ab[28, 31] == 240) and np.all(ba[28, 31] == 10)
    # each order equals pasting one face after the other
    assert np.array_equal(ab, R.paste(R.paste(photo, [(a, Pa)], S, ramp), [(b, Pb)], S, ramp))
    # where only one face reaches, the order does not matter
    assert np.array_equal(ab[:16], ba[:16])


def test_default_ramp_shape():
    from vspbfr_amd import photo as P
    r = R.default_ramp()
    assert r.dtype == np.uint16 and r.shape == (8 * 56 + 1,) and r[0] == 0 and np.all(r[:65] == 0) and r[-1] == 256
    assert np.all(np.diff(r.astype(np.int64)) >= 0) and r[64 + 8 * 24] == 128
    assert np.array_equal(P.default_ramp(), r) and np.array_equal(P.default_ramp(3, 0), R.default_ramp(3, 0))
    assert np.array_equal(P.default_ramp(0, 5), R.default_ramp(0, 5)) and P.default_ramp(0, 0).tolist() == [0]


def test_plan_tables_boxes_and_tiles_match_the_reference():
    """the product's host side (tables, inverse, bounding box) restated independently in photo_ref: the same integers"""
    from vspbfr_amd import photo as P
    photos = [R.test_photo(131, 67, seed=1), R.test_photo(37, 1100, seed=2), R.test_photo(64, 64, seed=3)]
    faces = [(0, R.landmarks_for(0.37, 17.0, (60.0, 30.0), 64)), (1, R.landmarks_for(2.9, -163.0, (20.0, 500.0), 64)),
             (0, R.landmarks_for(1.0, 0.0, (-400.0, 30.0), 64)), (0, R.landmarks_for(0.5, 5.0, (120.0, 60.0), 64))]
    for s in (1, 2):
        plan = P.FacePlan(photos, faces, size=64, upscale=s)
        assert plan.n == 4 and C.sizeof(P.FaceItem) == 40 and C.sizeof(P.FaceTile) == 32
        seen = set()
        for i, (k, pts) in enumerate(faces):
            A = R.similarity(pts, 64)
            assert np.array_equal(A, plan.A[i])            # the same float64 operations in the same order: the same bits
            ci, pi = plan.crop_items[i], plan.paste_items[i]
            t = np.concatenate(R.tables(R.invert(A), np.arange(64), np.arange(64)))
            assert np.array_equal(plan.crop_tables[ci.tab_off:ci.tab_off + 256], t)
            oh, ow = photos[k].shape[0] * s, photos[k].shape[1] * s
            box = R.bbox(R.paste_matrix(A, s), 64, oh, ow)
            if box[2] <= box[0] or box[3] <= box[1]:
                assert (pi.nx, pi.ny) == (0, 0) and i == 2
                continue
            assert (pi.x0, pi.y0, pi.x0 + pi.nx, pi.y0 + pi.ny) == box
            t = np.concatenate(R.tables(R.paste_matrix(A, s), np.arange(box[0], box[2]), np.arange(box[1], box[3])))
            assert np.array_equal(plan.paste_tables[pi.tab_off:pi.tab_off + t.size], t)
        order = []
        for t in plan.tiles[:plan.ntiles]:
            key = (t.dst_off, t.y0, t.x0)
            assert key not in seen and t.x0 % 32 == 0 and t.y0 % 32 == 0 and t.x0 < t.w and t.y0 < t.h
            seen.add(key)
            order.append(key)
            fl = plan.tile_faces[t.face0:t.face0 + t.nfaces].tolist()
            assert fl == sorted(set(fl)) and fl
            for f in fl:
                x0, y0, x1, y1 = plan.boxes[f]
                assert x0 < t.x0 + 32 and x1 > t.x0 and y0 < t.y0 + 32 and y1 > t.y0 and plan.out_off[plan.face_photo[f]] == t.dst_off
        assert order == sorted(order)
        # every pixel of every box lies in a tile that lists the face
        for f, (x0, y0, x1, y1) in enumerate(plan.boxes):
            for (xx, yy) in ((x0, y0), (x1 - 1, y1 - 1)):
                if x1 > x0:
                    hit = [t for t in plan.tiles[:plan.ntiles] if t.dst_off == plan.out_off[plan.face_photo[f]] and t.x0 <= xx < t.x0 + 32
                           and t.y0 <= yy < t.y0 + 32]
                    assert len(hit) == 1 and f in plan.tile_faces[hit[0].face0:hit[0].face0 + hit[0].nfaces]


def test_table_overflow_is_refused_on_the_host():
    from vspbfr_amd import photo as P
    with pytest.raises(ValueError, match="2\\^30"):
        R.tables(_M(tx=2.0 ** 20), np.arange(4), np.arange(4))
    with pytest.raises(ValueError, match="x.png.*face 0"):
        P.face_tables(_M(tx=2.0 ** 20), np.arange(4), np.arange(4), "x.png", 0)
    tiny = R.FFHQ512_TEMPLATE * 1e-6 + 5.0            # a face of a thousandth of a pixel: the crop -> photo scale is fine, photo -> crop explodes
    with pytest.raises(ValueError, match="2\\^30"):
        P.FacePlan([np.zeros((16, 16, 3), np.uint8)], [(0, tiny)])
