"""CPU checks of the colour fix's NumPy restatement (tests/color_fix_ref.py) against closed forms, and of the host side of the
feature: FacePlan's crop tables give the restatement's validity, and the request checks of vspbfr_amd.photo."""
import numpy as np
import pytest

import color_fix_ref as CF
import photo_ref as R

SIDES = (1, 9, 37, 64)


def _rand(S, seed, lo=0, hi=256):
    return np.random.default_rng(seed).integers(lo, hi, (S, S, 3)).astype(np.uint8)


@pytest.mark.parametrize("S", SIDES)
@pytest.mark.parametrize("mode", ["wavelet", "stats"])
def test_equal_inputs_return_the_restored_crop(S, mode):
    r = _rand(S, 1)
    assert np.array_equal(CF.fix(r, r, mode), r)


@pytest.mark.parametrize("S", SIDES)
@pytest.mark.parametrize("mode", ["wavelet", "stats"])
def test_a_constant_offset_without_clipping_returns_the_crop(S, mode):
    c = _rand(S, 2, 0, 239)
    r = (c + 17).astype(np.uint8)
    assert np.array_equal(CF.fix(c, r, mode), c)


def test_a_one_pixel_checkerboard_is_left_alone_away_from_the_border():
    S = 96
    yy, xx = np.mgrid[0:S, 0:S]
    r = _rand(S, 3, 9, 247)
    c = (r.astype(np.int64) + np.where((xx + yy) % 2 == 0, 9, -9)[..., None]).astype(np.uint8)
    out = CF.wavelet(c, r)
    assert np.array_equal(out[31:S - 31, 31:S - 31], r[31:S - 31, 31:S - 31])
    assert not np.array_equal(c, r)


@pytest.mark.parametrize("k", range(-255, 256, 51))
def test_constant_planes_clamp_at_the_rails(k):
    """c - r = k on constant planes, with c or r on a rail of the byte range: both fixes land on c exactly, nothing wraps"""
    S = 37
    pairs = [(k, 0), (255, 255 - k)] if k >= 0 else [(255 + k, 255), (0, -k)]          # (c, r)
    for cv, rv in pairs + [(100 + k, 100)] * (0 <= 100 + k <= 255):
        c, r = np.full((S, S, 3), cv, dtype=np.uint8), np.full((S, S, 3), rv, dtype=np.uint8)
        assert np.all(CF.wavelet(c, r) == cv) and np.all(CF.stats(c, r) == cv), (cv, rv)
    # past the rail the sum is clamped: r on one rail but for a single pixel on the other, c = clip(r + k).  The smoothed difference
    # at that pixel is almost k, so r + d leaves the byte range there and the output stays on the rail; far from it (the five
    # levels reach 31 px) the output is c
    if k == 0:
        return
    S, m = 96, 48
    lo, hi = (0, 255) if k > 0 else (255, 0)
    r = np.full((S, S, 3), lo, dtype=np.uint8)
    r[m, m] = hi
    c = np.clip(r.astype(np.int64) + k, 0, 255).astype(np.uint8)
    assert c[m, m, 0] == hi and c[0, 0, 0] == lo + k
    out = CF.wavelet(c, r)
    raw = r.astype(np.int64) + ((CF.wavelet_planes(c, r) + 32) >> 6)
    assert np.all(raw[m, m] > 255) if k > 0 else np.all(raw[m, m] < 0)
    assert np.array_equal(out, np.clip(raw, 0, 255)) and np.all(out[m, m] == hi)
    far = np.hypot(*np.mgrid[-m:S - m, -m:S - m]) > 45
    assert far.any() and np.all(out[far] == lo + k)


def test_the_extreme_difference_stays_in_int16():
    S = 64
    hi, lo = np.full((S, S, 3), 255, dtype=np.uint8), np.zeros((S, S, 3), dtype=np.uint8)
    for c, r in ((hi, lo), (lo, hi)):
        d = CF.wavelet_planes(c, r, levels=6)
        assert np.abs(d).max() == 16320 and 16320 < 1 << 15
        assert np.array_equal(CF.wavelet(c, r, levels=6), c)
    # the worst alternation: every intermediate stays inside the first plane's range
    yy, xx = np.mgrid[0:S, 0:S]
    c = np.where(((xx + yy) % 2 == 0)[..., None], hi, lo)
    for levels in range(1, 7):
        assert np.abs(CF.wavelet_planes(c, 255 - c, levels=levels)).max() <= 16320


def _hanging_face(S=64):
    """a face over the left and the top edge of a 90 x 80 photo, and one wholly outside"""
    photo = R.test_photo(90, 80, seed=5)
    over = R.landmarks_for(1.0, 17.0, (4.0, 6.0), S)
    outside = R.landmarks_for(1.0, 0.0, (-500.0, 30.0), S)
    return photo, over, outside


@pytest.mark.parametrize("mode", ["wavelet", "stats"])
def test_the_border_colour_changes_no_output_byte(mode):
    S = 64
    photo, over, _ = _hanging_face(S)
    M = R.invert(R.similarity(over, S))
    valid = CF.validity(M, S, 90, 80)
    assert valid.any() and not valid.all()
    r = _rand(S, 7)
    a = CF.fix(R.crop(photo, M, S, (128, 128, 128)), r, mode, valid)
    b = CF.fix(R.crop(photo, M, S, (255, 0, 31)), r, mode, valid)
    assert np.array_equal(a, b) and not np.array_equal(a, r)
    # and it does matter once validity is ignored
    assert not np.array_equal(CF.fix(R.crop(photo, M, S, (128, 128, 128)), r, mode), CF.fix(R.crop(photo, M, S, (255, 0, 31)), r, mode))


@pytest.mark.parametrize("mode", ["wavelet", "stats"])
def test_a_face_wholly_outside_returns_the_restored_crop(mode):
    S = 64
    photo, _, outside = _hanging_face(S)
    M = R.invert(R.similarity(outside, S))
    valid = CF.validity(M, S, 90, 80)
    assert not valid.any()
    r = _rand(S, 8)
    assert np.array_equal(CF.fix(R.crop(photo, M, S), r, mode, valid), r)
    assert CF.stats_constants(R.crop(photo, M, S), r, valid)[0][0] == 0


def test_the_gain_clamps_at_both_ends():
    S = 37
    flat, textured = np.full((S, S, 3), 90, dtype=np.uint8), _rand(S, 9)
    flat[0, 0] = 91                                                  # a deviation far below the textured one, not zero
    assert [k[1] for k in CF.stats_constants(textured, flat)] == [16384] * 3
    assert [k[1] for k in CF.stats_constants(flat, textured)] == [1024] * 3
    flat[0, 0] = 90                                                  # zero deviation on either side
    assert [k[1] for k in CF.stats_constants(textured, flat)] == [16384] * 3
    assert [k[1] for k in CF.stats_constants(flat, textured)] == [1024] * 3
    out = CF.stats(flat, textured)                                   # a quarter of the texture around the flat mean
    assert out.min() >= 90 - 33 and out.max() <= 90 + 33 and out.std() > 10


@pytest.mark.parametrize("levels", [1, 6])
def test_one_and_six_levels(levels):
    S = 37
    c, r = CF.toned_pair(1, S, 11)
    out = CF.wavelet(c[0], r[0], levels=levels)
    assert not np.array_equal(out, r[0]) and not np.array_equal(out, CF.wavelet(c[0], r[0], levels=5))
    if levels == 1:                                                  # one level by hand: [1 2 1] along x, then along y, edge replicated
        d = (c[0].astype(np.int64) - r[0]) * 64
        p = np.pad(d, ((0, 0), (1, 1), (0, 0)), mode="edge")
        d = (p[:, :-2] + 2 * p[:, 1:-1] + p[:, 2:] + 2) >> 2
        p = np.pad(d, ((1, 1), (0, 0), (0, 0)), mode="edge")
        d = (p[:-2] + 2 * p[1:-1] + p[2:] + 2) >> 2
        assert np.array_equal(out, np.clip(r[0].astype(np.int64) + ((d + 32) >> 6), 0, 255).astype(np.uint8))
    with pytest.raises(AssertionError):
        CF.wavelet(c[0], r[0], levels=7)


@pytest.mark.parametrize("antialias", [False, True])
def test_faceplan_tables_give_the_restatements_validity(antialias):
    from vspbfr_amd import photo as P
    S = 64
    photo, over, outside = _hanging_face(S)
    inside = R.landmarks_for(1.1, -10.0, (45.0, 40.0), S)
    faces = [(0, over), (0, outside), (0, inside)]
    plan = P.FacePlan([photo], faces, size=S, antialias=antialias)
    for i, (_, pts) in enumerate(faces):
        it = plan.crop_items[i]
        t = plan.crop_tables[it.tab_off:it.tab_off + 4 * S].astype(np.int64)
        ax, bx, cx, cy = t[:S], t[S:2 * S], t[2 * S:3 * S], t[3 * S:]
        ix, iy = (cx[:, None] + ax[None, :]) >> 10, (cy[:, None] + bx[None, :]) >> 10
        valid = (ix >= 0) & (ix < it.w) & (iy >= 0) & (iy < it.h)
        assert (it.nx, it.ny, it.w, it.h) == (S, S, 90, 80)
        assert np.array_equal(valid, CF.validity_from_landmarks(pts, S, 90, 80)), i
    assert CF.validity_from_landmarks(inside, S, 90, 80).all()


def test_requests_are_checked_on_the_host():
    from vspbfr_amd import photo as P
    assert P.check_color_fix(None) == (None, 5) and P.check_color_fix("none", 3) == (None, 3) and P.check_color_fix("wavelet", 6) == ("wavelet", 6)
    for mode, levels in (("adain", 5), ("wavelet", 0), ("wavelet", 7), ("stats", 2.5), ("stats", True)):
        with pytest.raises(ValueError):
            P.check_color_fix(mode, levels)
    with pytest.raises(ValueError):
        P.PhotoRestorer(None, 4, color_fix="wavelets")
    with pytest.raises(ValueError):
        P.PhotoRestorer(None, 4, color_fix="wavelet", color_levels=9)
    assert P.PhotoRestorer(None, 4).color_fix is None
