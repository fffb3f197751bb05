"""CPU checks of the device ingest's host side: the NumPy restatement of Pillow's 8-bit LANCZOS resize (tests/resample_ref.py, the
kernel's oracle) equals live PIL byte for byte; cover_geometry equals imageio._cover_and_crop; the plan's table is consistent; the C
entry refuses bad arguments before it touches a device; the fp32 normalisation the kernel restates equals imageio._to_tensor bitwise."""
import ctypes as C
import os

import numpy as np
import pytest

import resample_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LOADER_IMAGES = os.path.join(ROOT, "tests", "golden", "loader_images")


def _pil_resize(a, size):
    from PIL import Image
    return np.asarray(Image.fromarray(a).resize(size, Image.Resampling.LANCZOS))


@pytest.mark.parametrize("src,dst", R.SIZE_PAIRS, ids=lambda s: "%dx%d" % s)
def test_restatement_equals_pil(src, dst):
    a = R.test_image(src[0], src[1], seed=src[0] * 7 + src[1])
    want, got = _pil_resize(a, dst), R.resize(a, dst[0], dst[1])
    assert want.shape == got.shape == (dst[1], dst[0], 3)
    assert np.array_equal(want, got), int((want != got).sum())
    if src != dst and min(src) >= 33 and max(src[0] / dst[0], src[1] / dst[1]) <= 2:
        assert want.min() == 0 and want.max() == 255      # both ends of clip8 are reached (a stronger reduction averages the stripes away)


def test_restatement_equals_pil_width_sweep():
    for src, dst in R.SWEEP:
        a = R.test_image(src[0], src[1], seed=src[0])
        assert np.array_equal(_pil_resize(a, dst), R.resize(a, dst[0], dst[1])), src


def test_one_axis_unchanged_equals_pil():
    """Pillow skips the pass of an axis whose size does not change; the restatement runs it with identity taps: the same bytes"""
    for src, dst in (((300, 64), (300, 32)), ((65, 300), (32, 300))):
        a = R.test_image(src[0], src[1], seed=3)
        assert np.array_equal(_pil_resize(a, dst), R.resize(a, dst[0], dst[1])), src


def test_coefficient_table_properties():
    from vspbfr_amd.resample import MAX_TAPS, lanczos_coeffs, lanczos_ksize
    for i, o in ((1024, 512), (513, 512), (40, 64), (1024, 64), (64, 64), (1, 8), (161, 32)):
        xmin, count, taps = lanczos_coeffs(i, o)
        assert taps.shape == (o, lanczos_ksize(i, o)) and xmin.dtype == count.dtype == taps.dtype == np.int32
        assert (xmin >= 0).all() and (count >= 1).all() and (xmin + count <= i).all() and (count <= taps.shape[1]).all()
        assert (np.diff(xmin) >= 0).all() and (np.diff(xmin + count) >= 0).all()      # the crop's source window is xmin[first] .. end[last]
        assert (np.abs(taps.sum(1) - (1 << 22)) <= taps.shape[1]).all()                 # normalised up to the rounding of each tap
        assert int(np.abs(taps.astype(np.int64)).sum(1).max()) * 255 < 2 ** 31          # the 32-bit accumulator cannot overflow
        assert lanczos_coeffs(i, o)[2] is taps                                          # cached
    assert lanczos_ksize(1024, 64) == MAX_TAPS and lanczos_ksize(1088, 64) > MAX_TAPS
    xmin, count, taps = lanczos_coeffs(64, 64)
    assert all(taps[x, x - xmin[x]] == 1 << 22 and np.count_nonzero(taps[x]) == 1 for x in range(64))   # equal size: identity


def _sizes_of_loader_images():
    from PIL import Image
    from vspbfr_amd.imageio import list_images
    return [Image.open(p).size for p in list_images(LOADER_IMAGES)]


def test_cover_geometry_equals_cover_and_crop():
    from PIL import Image
    from vspbfr_amd.imageio import _cover_and_crop
    from vspbfr_amd.resample import cover_geometry

    class Probe:   # records what _cover_and_crop asks of an image
        def __init__(self, size):
            self.size, self.calls = size, []

        def resize(self, size, resample):
            assert resample == Image.Resampling.LANCZOS
            self.calls.append(size)
            return self

        def crop(self, box):
            self.calls.append(box)
            return self

    rng = np.random.default_rng(0)
    sizes = _sizes_of_loader_images()
    assert len(sizes) >= 8
    sizes += [(int(w), int(h)) for w, h in rng.integers(1, 3000, (600, 2))] + [(64, 64), (48, 80), (80, 48), (300, 300), (3, 3)]
    short = 0
    for im_size in ((64, 64), (48, 80), (512, 512), (256, 256)):
        for w, h in sizes:
            p = Probe((w, h))
            got = _cover_and_crop([p], p, im_size)
            nw, nh, box = cover_geometry(w, h, im_size)
            if (h, w) == im_size:
                assert got[0] is p and not p.calls and (nw, nh, box) == (w, h, (0, 0, im_size[1], im_size[0]))
            else:
                assert p.calls == [(nw, nh), box], (w, h, im_size)
            assert box[2] - box[0] == im_size[1] and box[3] - box[1] == im_size[0]
            short += nw < im_size[1] or nh < im_size[0]
    assert short > 0    # int(ratio * w) does fall one short of the target for some sizes: the plan sends those to PIL
    assert cover_geometry(100, 50, (64, 64), origin=(5, 0)) == (128, 64, (5, 0, 69, 64))


def _plan(specs, im_size, flips=None):
    """specs: (sw, sh, nw, nh, x0, y0)"""
    from vspbfr_amd.resample import ResamplePlan
    srcs = [R.test_image(s[0], s[1], seed=i) for i, s in enumerate(specs)]
    return srcs, ResamplePlan(srcs, [s[2:4] for s in specs], [s[4:6] for s in specs], im_size, flips)


def test_plan_offsets_and_fallback():
    from vspbfr_amd import resample as RS
    H, W = 16, 20
    specs = [(41, 33, 25, 20, 2, 1), (41, 33, 25, 20, 5, 4), (20, 16, 20, 16, 0, 0), (23, 301, 23, 301, 1, 100), (340, 16, 20, 16, 0, 0),
             (35, 30, 19, 16, 0, 0)]
    srcs, plan = _plan(specs, (H, W), flips=[False, True, True, False, False, False])
    assert plan.host_items == [4, 5]            # 17x reduction; a resized image narrower than the crop
    it = plan.items
    assert [i.src_off for i in it] == [0, 4059, 8118, 9078, 29847, 30807] and plan.src_bytes == 31767
    assert [i.src_off % 4 for i in it[:4]] == [0, 3, 2, 2]                     # odd widths: sources off dword alignment, kept as packed
    assert (it[0].hco, it[0].vco) == (it[1].hco, it[1].vco) and it[0].hk == RS.lanczos_ksize(41, 25) and it[0].vk == RS.lanczos_ksize(33, 20)
    assert it[3].hk == it[3].vk == 7 and it[3].hco != it[0].hco
    assert [i.flags for i in it] == [0, RS.FLIP, RS.FLIP | RS.COPY, 0, RS.COPY, RS.COPY]
    assert (it[4].sw, it[4].sh, it[5].nw, it[5].nh) == (W, H, W, H)
    stride = RS.work_row_bytes(W)
    assert stride == 60 and RS.work_row_bytes(21) == 64
    off = 0
    for i in (0, 1, 3):
        ymin, ycount, _ = RS.lanczos_coeffs(it[i].sh, it[i].nh)
        assert it[i].row0 == ymin[it[i].y0] and it[i].row1 == ymin[it[i].y0 + H - 1] + ycount[it[i].y0 + H - 1] - 1
        assert it[i].work_off == off and off % 4 == 0
        off += (it[i].row1 - it[i].row0 + 1) * stride
    assert plan.work_bytes == off and it[3].row1 - it[3].row0 + 1 < 40          # only the rows the crop reads, not the 301
    # tables: xmin, count, tap-major taps
    xmin, count, taps = RS.lanczos_coeffs(41, 25)
    o = it[0].hco
    assert np.array_equal(plan.coef[o:o + 25], xmin) and np.array_equal(plan.coef[o + 25:o + 50], count)
    assert np.array_equal(plan.coef[o + 50:o + 50 + 25 * taps.shape[1]].reshape(taps.shape[1], 25), taps.T)
    assert plan.coef_ints == plan.coef.size == sum(o_ * (2 + RS.lanczos_ksize(i_, o_)) for i_, o_ in ((41, 25), (33, 20), (23, 23), (301, 301)))
    # the packed upload
    host, nb, c0, s0 = plan.pack()
    hv = host.numpy()
    assert nb == C.sizeof(RS.ResampleItem) * 6 and c0 % 16 == 0 and s0 % 16 == 0 and hv.size == s0 + plan.src_bytes
    assert bytes(hv[:nb]) == bytes(plan.items) and np.array_equal(hv[c0:c0 + 4 * plan.coef_ints].view(np.int32), plan.coef)
    for i in range(4):
        assert np.array_equal(hv[s0 + it[i].src_off:s0 + it[i].src_off + srcs[i].size], srcs[i].reshape(-1))
    from PIL import Image
    want = np.asarray(Image.fromarray(srcs[4]).resize((20, 16), Image.Resampling.LANCZOS))
    assert np.array_equal(hv[s0 + it[4].src_off:s0 + it[4].src_off + want.size].reshape(want.shape), want)
    # a corrupted table is caught
    it[1].work_off = plan.work_bytes
    with pytest.raises(ValueError, match="work buffer"):
        plan.check()
    with pytest.raises(ValueError):
        RS.ResamplePlan([np.zeros((4, 4), np.uint8)], [(4, 4)], [(0, 0)], (4, 4))


def test_entry_refuses_bad_arguments_without_a_gpu():
    from vspbfr_amd import _lib
    from vspbfr_amd import resample as RS
    lib = _lib.lib
    assert lib.vsp_struct_size(7) == C.sizeof(RS.ResampleItem) == 80
    assert lib.vsp_lanczos_work_bytes(3, 20) == 180 and lib.vsp_lanczos_work_bytes(0, 20) == 0 and lib.vsp_lanczos_work_bytes(1, 8193) == 0
    _, plan = _plan([(41, 33, 25, 20, 2, 1)], (16, 20))
    d = C.c_void_p(256)     # non-null, aligned dummy "device" pointers: every refusal below comes before a launch

    def call(items=plan.items, out=d, src=d, n=1, H=16, W=20, work_bytes=plan.work_bytes, coef_ints=plan.coef_ints, src_bytes=plan.src_bytes):
        return lib.vsp_lanczos_resize_u8(out, None, src, src_bytes, d, coef_ints, d, work_bytes, C.cast(items, C.c_void_p) if items else None,
                                         d, n, H, W, None)

    assert call(out=None) == -1 and "null pointer" in _lib.last_error()
    assert call(src=None) == -1 and "null pointer" in _lib.last_error()
    assert call(items=None) == -1 and "null pointer" in _lib.last_error()
    assert call(H=0) == -1 and call(n=-1) == -1
    assert call(H=8193) == -3
    assert call(H=20) == -1 and "outside the resized" in _lib.last_error()           # y0 + H = 1 + 20 > nh = 20
    assert call(work_bytes=plan.work_bytes - 1) == -1 and "work bytes" in _lib.last_error()
    assert call(coef_ints=plan.coef_ints - 1) == -1 and "coefficient" in _lib.last_error()
    assert call(src_bytes=plan.src_bytes - 1) == -1 and "source" in _lib.last_error()

    def edited(**kw):
        items = (RS.ResampleItem * 1)()
        C.memmove(items, plan.items, C.sizeof(items))
        for k, v in kw.items():
            setattr(items[0], k, v)
        return items

    assert call(items=edited(sw=0)) == -1 and "zero size" in _lib.last_error()
    assert call(items=edited(x0=6)) == -1 and "outside the resized" in _lib.last_error()
    assert call(items=edited(sw=8193)) == -3
    assert call(items=edited(sw=17 * 25), src_bytes=3 * 425 * 33) == -3 and "16x" in _lib.last_error()         # 17x: 103 taps
    assert call(items=edited(sw=16 * 25, hk=97), src_bytes=3 * 400 * 33) == -1 and "coefficient" in _lib.last_error()   # 16x is served: next check
    assert call(items=edited(hk=5)) == -1 and "tap counts" in _lib.last_error()
    assert call(items=edited(row1=33)) == -1 and "source rows" in _lib.last_error()
    assert call(items=edited(work_off=2)) == -1
    assert call(items=edited(flags=RS.COPY)) == -1 and "copy item" in _lib.last_error()
    assert call(n=0) == 0


def test_fp32_normalisation_of_every_byte_value():
    import torch  # noqa: F401
    from vspbfr_amd.imageio import _to_tensor
    v = np.arange(256, dtype=np.uint8).reshape(1, 256, 1).repeat(3, axis=2)
    want = _to_tensor(v).numpy()
    got = R.to_tensor_f32(v).transpose(2, 0, 1)
    assert want.dtype == got.dtype == np.float32 and np.array_equal(want.view(np.int32), got.view(np.int32))
    assert got.shape == (3, 1, 256) and got[0, 0, 0] == -1.0 and got[0, 0, 255] == 1.0
