"""CPU checks of the anti-aliased face path: closed forms of the restatement tests/photo_aa_ref.py -- the window sum equals
the sum over every lattice point, identity and translation, the [1, 2, 1] / 4 filter at a minification of 2, a one-pixel checkerboard
that turns to flat 128, flat stays flat, the accumulator bounds at 16 -- and the product's host side (vspbfr_amd/photo.py: reach, forward
tables, source ranges, items, the unchanged layout without antialias) against it.  Equality everywhere."""
import ctypes as C

import numpy as np
import pytest

import photo_aa_ref as AA
import photo_ref as R

# minification, turn: the six of the prototype run paired in order, and the diamond-shaped worst case of the window at 4
CASES = [(1.0, 0.0), (1.3, 17.0), (2.0, 45.0), (2.9, 90.0), (4.0, -163.0), (7.5, 30.0), (4.0, 45.0)]
S = 24


def _A(m, deg, centre, size=S):
    return R.similarity(R.landmarks_for(1.0 / m, deg, centre, size), size)


def _exact(m=1.0, tx=0.0, ty=0.0):
    """A (photo -> crop) = scale 1 / m, no turn, crop pixel (0, 0) at photo pixel (tx, ty): exact in float64 for dyadic values"""
    return np.array([[1.0 / m, 0.0, -tx / m], [0.0, 1.0 / m, -ty / m]])


@pytest.mark.parametrize("m,deg", CASES)
def test_window_sum_equals_the_sum_over_every_lattice_point(m, deg):
    photo = R.test_photo(150, 170, seed=3)
    A = _A(m, deg, (70.0, 90.0))
    stats = {}
    win = AA.crop(photo, A, S, border=(10, 200, 90), stats=stats)
    assert np.array_equal(win, AA.crop(photo, A, S, border=(10, 200, 90), every_point=True))
    if stats:
        mm = AA.crop_minify(A)
        print(f"m {m} at {deg}: W / (4096 m^2) in {stats['W_min'] / (4096 * mm * mm):.3f} .. {stats['W_max'] / (4096 * mm * mm):.3f}, acc max {stats['acc_max']:.3g}")
        assert stats["W_min"] > 0 and stats["acc_max"] < 1 << 31
    # and the paste of a restored crop into a small face: P = A of the inverse scale
    restored = R.test_photo(S, S, seed=4)
    small = R.test_photo(40, 36, seed=5)
    P = R.similarity(R.landmarks_for(m, deg, (20.0, 18.0), S), S)
    ramp = np.array([0, 100, 256], dtype=np.uint16)
    assert np.array_equal(AA.paste(small, [(restored, P)], S, ramp), AA.paste(small, [(restored, P)], S, ramp, every_point=True))


def test_identity_and_integer_translation_return_the_photo_window():
    photo = R.test_photo(90, 70, seed=6)
    for tx, ty in ((0, 0), (13, 7), (-5, 60)):
        A = _exact(1.0, tx, ty)
        got = AA.crop(photo, A, S)
        assert np.array_equal(got, R.crop(photo, R.invert(A), S))
        if tx >= 0 and ty + S <= 70:
            assert np.array_equal(got, photo[ty:ty + S, tx:tx + S])
    # the filter itself at m = 1 is the identity too (no seam where bilinear hands over): weights 4096 on one lattice point
    A = _exact(1.0, 13, 7)
    xs = np.arange(S)
    X, Y = R._coords(R.invert(A), xs, xs)
    assert np.array_equal(AA.filtered(photo, A, X, Y, xs, xs, 2, (128, 128, 128)), photo[7:7 + S, 13:13 + S])


def test_minification_two_is_the_separable_121_filter():
    photo = R.test_photo(90, 70, seed=7)
    A = _exact(2.0, 6, 4)
    got = AA.crop(photo, A, S).astype(np.int64)
    p = photo.astype(np.int64)
    k = np.array([1, 2, 1])
    want = np.zeros((S, S, 3), dtype=np.int64)
    for j in range(S):
        for i in range(S):
            y, x = 4 + 2 * j, 6 + 2 * i
            want[j, i] = ((p[y - 1:y + 2, x - 1:x + 2] * (k[:, None] * k[None, :])[..., None]).sum(axis=(0, 1)) + 8) // 16
    assert np.array_equal(got, want)


def test_checkerboard_turns_to_flat_grey_where_bilinear_aliases():
    yy, xx = np.mgrid[0:140, 0:140]
    photo = np.repeat((((xx + yy) & 1) * 255).astype(np.uint8)[..., None], 3, axis=2)
    A = _exact(4.0, 8, 12)
    got = AA.crop(photo, A, S)
    assert np.all(got == 128)                                                # every crop pixel is interior here
    plain = R.crop(photo, R.invert(A), S)
    assert set(np.unique(plain)) <= {0, 255} and plain.std() == 0            # four taps on one lattice point: an alias, not an average


@pytest.mark.parametrize("deg", [0.0, 17.0, 45.0, -163.0])
def test_flat_photo_with_its_own_border_colour_stays_flat(deg):
    photo = np.full((50, 60, 3), (31, 200, 77), dtype=np.uint8)
    for m in (1.3, 2.9, 7.5):
        assert np.all(AA.crop(photo, _A(m, deg, (10.0, 45.0)), S, border=(31, 200, 77)) == np.array([31, 200, 77]))


def test_accumulator_and_weight_sum_at_the_largest_minification():
    photo = np.full((300, 300, 3), 255, dtype=np.uint8)
    for m, deg in ((16.0, 0.0), (15.999, 45.0), (15.999, 17.0)):              # (a turned 16 may round to 16 + 4e-15, which is refused)
        stats = {}
        A = _A(m, deg, (150.0, 150.0), 16)
        assert AA.reach(R.invert(A), AA.crop_minify(A)) <= AA.MAX_REACH
        AA.crop(photo, A, 16, border=(255, 255, 255), stats=stats)
        print(f"m {m} at {deg}: reach {AA.reach(R.invert(A), AA.crop_minify(A))}, W {stats['W_min']} .. {stats['W_max']}, acc max {stats['acc_max']} = 2^{np.log2(stats['acc_max']):.2f}")
        assert stats["W_min"] > 0 and stats["acc_max"] < 1 << 31


def test_faces_that_are_not_minified_keep_the_bilinear_bytes():
    photo = R.test_photo(90, 70, seed=8)
    for m in (0.37, 0.8, 1.0):
        A = np.array(_exact(m, 3, 5))
        assert AA.reach(R.invert(A), AA.crop_minify(A)) == 0
        assert np.array_equal(AA.crop(photo, A, S), R.crop(photo, R.invert(A), S))
    restored = R.test_photo(S, S, seed=9)
    P = R.similarity(R.landmarks_for(0.5, 17.0, (40.0, 30.0), S), S)          # the crop is magnified into the photo
    assert np.array_equal(AA.paste(photo, [(restored, P)], S), R.paste(photo, [(restored, P)], S))


def _plan_case():
    photos = [R.test_photo(131, 67, seed=1), R.test_photo(37, 300, seed=2), R.test_photo(64, 64, seed=3)]
    faces = [(0, R.landmarks_for(0.37, 17.0, (60.0, 30.0), 64)), (1, R.landmarks_for(1 / 2.9, -163.0, (20.0, 150.0), 64)),
             (0, R.landmarks_for(1.0, 0.0, (-400.0, 30.0), 64)), (0, R.landmarks_for(0.25, 45.0, (120.0, 60.0), 64)),
             (2, R.landmarks_for(3.4, 17.0, (30.0, 30.0), 64))]
    return photos, faces


@pytest.mark.parametrize("upscale", [1, 2])
def test_plan_integers_equal_the_restatement(upscale):
    from vspbfr_amd import photo as P
    photos, faces = _plan_case()
    plan = P.FacePlan(photos, faces, size=64, upscale=upscale, antialias=True)
    assert C.sizeof(P.FaceAAItem) == 72 and P.MAX_MINIFY == AA.MAX_MINIFY and P.MAX_REACH == AA.MAX_REACH
    seen = set()
    for i, (k, pts) in enumerate(faces):
        A = R.similarity(pts, 64)
        h, w = photos[k].shape[:2]
        for kind in ("crop", "paste"):
            it = (plan.crop_aa_items if kind == "crop" else plan.paste_aa_items)[i]
            old = (plan.crop_items if kind == "crop" else plan.paste_items)[i]
            fwd = (plan.crop_fwd if kind == "crop" else plan.paste_fwd).astype(np.int64)
            assert all(getattr(it, n) == getattr(old, n) for n in ("src_off", "tab_off", "h", "w", "x0", "y0", "nx", "ny"))
            if kind == "crop":
                M, F, m, xs, ys = R.invert(A), A, AA.crop_minify(A), np.arange(64), np.arange(64)
                assert plan.crop_minify[i] == m
            else:
                M = R.paste_matrix(A, upscale)
                F, m = R.invert(M), AA.paste_minify(M)
                x0, y0, x1, y1 = R.bbox(M, 64, h * upscale, w * upscale)
                xs, ys = np.arange(x0, max(x1, x0)), np.arange(y0, max(y1, y0))
                assert plan.paste_minify[i] == m
            rch = AA.reach(M, m) if xs.size and ys.size else 0
            assert it.reach == rch
            seen.add((kind, rch > 0))
            if rch:
                rng = AA.source_range(M, xs, ys, rch)
                assert (it.sx0, it.sy0, it.snx, it.sny) == rng
                want = np.concatenate(AA.forward_tables(F, np.arange(rng[0], rng[0] + rng[2]), np.arange(rng[1], rng[1] + rng[3])))
                assert np.array_equal(fwd[it.fwd_off:it.fwd_off + want.size], want)
            else:
                assert (it.sx0, it.sy0, it.snx, it.sny) == (0, 0, 0, 0)
    assert seen == {("crop", True), ("crop", False), ("paste", True), ("paste", False)}
    assert plan.crop_fwd.dtype == np.int32 and plan.paste_fwd.dtype == np.int32


def test_plan_without_antialias_packs_the_bytes_it_always_did():
    """the layout of the parent commit, restated: six table sections at 16-byte aligned offsets, then the photos; nothing else"""
    from vspbfr_amd import photo as P
    photos, faces = _plan_case()
    plan = P.FacePlan(photos, faces, size=64)
    assert not plan.antialias and not hasattr(plan, "crop_aa_items")
    host, sections = plan.pack()
    assert list(sections) == ["crop_items", "paste_items", "tiles", "tile_faces", "crop_tables", "paste_tables", "photos"]
    n, nt = plan.n, plan.ntiles
    parts = [bytes(plan.crop_items)[:n * C.sizeof(P.FaceItem)], bytes(plan.paste_items)[:n * C.sizeof(P.FaceItem)],
             bytes(plan.tiles)[:nt * C.sizeof(P.FaceTile)], plan.tile_faces.tobytes(), plan.crop_tables.tobytes(), plan.paste_tables.tobytes()]
    want = bytearray()
    for name, b in zip(sections, parts):
        assert sections[name] == (len(want), len(b))
        want += b + bytes(-len(b) % 16)
    assert sections["photos"] == (len(want), sum(p.size for p in photos))
    want += b"".join(p.tobytes() for p in photos)
    got = host.numpy()
    for name, (o, nb) in sections.items():                                  # (the padding between sections is uninitialised)
        assert got[o:o + nb].tobytes() == bytes(want[o:o + nb]), name
    assert got.size == len(want)
    aa, more = P.FacePlan(photos, faces, size=64, antialias=True).pack()
    assert list(more)[:6] == list(sections)[:6] and list(more)[6:] == ["crop_aa_items", "paste_aa_items", "crop_fwd", "paste_fwd", "photos"]
    for name in list(sections)[:6]:
        assert more[name] == sections[name] and aa.numpy()[more[name][0]:more[name][0] + more[name][1]].tobytes() == bytes(want[sections[name][0]:sections[name][0] + sections[name][1]])


def test_minification_above_sixteen_is_refused_by_name():
    from vspbfr_amd import photo as P
    photo = R.test_photo(64, 64, seed=1)
    big = R.landmarks_for(1 / 16.5, 17.0, (30.0, 30.0), 64)                  # a face 16.5 times the crop
    with pytest.raises(ValueError, match="holiday.png.*face 0"):
        P.FacePlan([photo], [(0, big)], size=64, names=["holiday.png"], antialias=True)
    small = R.landmarks_for(16.5, 17.0, (30.0, 30.0), 64)                    # a crop 16.5 times the face
    with pytest.raises(ValueError, match="holiday.png.*face 1"):
        P.FacePlan([photo], [(0, R.landmarks_for(1.0, 0.0, (30.0, 30.0), 64)), (0, small)], size=64, names=["holiday.png"], antialias=True)
    P.FacePlan([photo], [(0, small)], size=64, upscale=2, antialias=True)    # at upscale 2 the paste shrinks by 8.25
    P.FacePlan([photo], [(0, big), (0, small)], size=64, names=["holiday.png"])   # and without the filter nothing is refused
    with pytest.raises(ValueError):
        AA.crop(photo, R.similarity(big, 64), 64)
