"""CPU checks of the device-source and ragged-output sides of vspbfr_amd.resample.ResamplePlan and of the refusals of
vsp_lanczos_resize_ragged_u8, which come before any launch (no GPU needed)."""
import ctypes as C

import numpy as np
import pytest
import torch

import resample_ref as R


def _buffer(shapes, lead=0, seed=0):
    """(flat uint8 CPU tensor holding the (h, w, 3) images back to back behind `lead` bytes, offsets, images)"""
    imgs = [R.test_image(w, h, seed=seed + i) for i, (h, w) in enumerate(shapes)]
    offsets, at = [], lead
    for a in imgs:
        offsets.append(at)
        at += a.size
    flat = np.full(at, 0x5A, dtype=np.uint8)
    for o, a in zip(offsets, imgs):
        flat[o:o + a.size] = a.reshape(-1)
    return torch.from_numpy(flat), offsets, imgs


def test_device_sources_take_their_offsets_and_upload_no_pixels():
    from vspbfr_amd import resample as RS
    shapes = [(33, 41), (16, 20), (33, 41)]
    buf, offsets, imgs = _buffer(shapes, lead=1)
    targets, origins = [(25, 20), (20, 16), (25, 20)], [(2, 1), (0, 0), (5, 4)]
    plan = RS.ResamplePlan(shapes, targets, origins, (16, 20), device_sources=(buf, offsets))
    assert [it.src_off for it in plan.items] == offsets == [1, 1 + 3 * 33 * 41, 1 + 3 * 33 * 41 + 3 * 16 * 20]
    assert not plan.host_items and plan.src_bytes == buf.numel()
    nb = 3 * C.sizeof(RS.ResampleItem)
    want = ((nb + 15) // 16 * 16 + plan.coef.nbytes + 15) // 16 * 16
    assert plan.upload_bytes == want == plan.pack()[0].numel()
    # the tables are those of the plan over uploaded arrays, but for where the sources are
    ref = RS.ResamplePlan(imgs, targets, origins, (16, 20))
    assert np.array_equal(plan.coef, ref.coef) and plan.work_bytes == ref.work_bytes
    for a, b in zip(plan.items, ref.items):
        assert all(getattr(a, f) == getattr(b, f) for f, _ in RS.ResampleItem._fields_ if f != "src_off")
    assert ref.pack()[0].numel() == want + ref.src_bytes
    # pixels beside the buffer, and an offset past it
    with pytest.raises(ValueError, match="not as pixels"):
        RS.ResamplePlan(imgs, targets, origins, (16, 20), device_sources=(buf, offsets))
    with pytest.raises(ValueError, match="outside the device buffer"):
        RS.ResamplePlan(shapes, targets, origins, (16, 20), device_sources=(buf, [offsets[0], offsets[1], offsets[2] + 1]))
    with pytest.raises(ValueError, match="outside the device buffer"):
        RS.ResamplePlan(shapes, targets, origins, (16, 20), device_sources=(buf, [-1] + offsets[1:]))
    with pytest.raises(ValueError, match="flat contiguous uint8"):
        RS.ResamplePlan(shapes, targets, origins, (16, 20), device_sources=(buf.to(torch.int32), offsets))
    # a corrupted table is caught against the buffer's size
    plan.items[2].src_off += 1
    with pytest.raises(ValueError, match="device buffer"):
        plan.check()


def test_an_item_the_kernel_does_not_serve_comes_back_alone():
    """a 17x reduction among device sources: that slice is resized by PIL and uploaded behind the tables as a COPY item whose
    source follows the buffer; the other items stay where they are"""
    from PIL import Image
    from vspbfr_amd import resample as RS
    shapes = [(33, 41), (16, 340)]
    buf, offsets, imgs = _buffer(shapes)
    plan = RS.ResamplePlan(shapes, [(25, 20), (20, 16)], [(2, 1), (0, 0)], (16, 20), device_sources=(buf, offsets))
    assert plan.host_items == [1] and plan.items[1].flags == RS.COPY and plan.items[0].src_off == 0
    assert plan.items[1].src_off == buf.numel() and plan.src_bytes == buf.numel() + 3 * 16 * 20
    host, nb, c0, s0 = plan.pack()
    assert plan.upload_bytes == s0 + 3 * 16 * 20
    want = np.asarray(Image.fromarray(imgs[1]).resize((20, 16), Image.Resampling.LANCZOS))
    assert np.array_equal(host.numpy()[s0:].reshape(16, 20, 3), want)


def test_ragged_plan_builds_the_destination_table():
    from vspbfr_amd import _lib
    from vspbfr_amd import resample as RS
    assert _lib.lib.vsp_struct_size(13) == C.sizeof(RS.ResampleDst) == 16
    shapes = [(3, 5), (7, 4), (9, 9)]
    buf, offsets, _ = _buffer(shapes)
    sizes = [(6, 10), (14, 8), (9, 9)]
    targets = [(w, h) for h, w in sizes]
    plan = RS.ResamplePlan(shapes, targets, [(0, 0)] * 3, None, device_sources=(buf, offsets), out_sizes=sizes)
    assert [(d.out_off, d.H, d.W) for d in plan.dst] == [(0, 6, 10), (180, 14, 8), (516, 9, 9)] and plan.out_bytes == 516 + 243
    assert plan.items[2].flags == RS.COPY and plan.nk == 3 and plan.H is None
    # every item's intermediate rows use the stride of its own width
    rows = [it.row1 - it.row0 + 1 for it in plan.items]
    assert plan.items[1].work_off == rows[0] * RS.work_row_bytes(10) and plan.work_bytes == rows[0] * 32 + rows[1] * 24
    gaps = [16, 16 + 180 + 16, 16 + 180 + 16 + 336 + 16]
    plan = RS.ResamplePlan(shapes, targets, [(0, 0)] * 3, None, device_sources=(buf, offsets), out_sizes=sizes, out_offsets=gaps)
    assert [d.out_off for d in plan.dst] == gaps and plan.out_bytes == gaps[2] + 243
    host, nb, c0, s0 = plan.pack()
    assert bytes(host.numpy()[plan.dst_at:plan.dst_at + 48]) == bytes(plan.dst) and s0 == plan.upload_bytes
    for bad, why in (([0, 179, 516], "overlaps"), ([516, 0, 180], "descends"), ([-1, 180, 516], "negative")):
        with pytest.raises(ValueError, match=why):
            RS.ResamplePlan(shapes, targets, [(0, 0)] * 3, None, device_sources=(buf, offsets), out_sizes=sizes, out_offsets=bad)
    with pytest.raises(ValueError):
        RS.ResamplePlan(shapes, targets, [(0, 0)] * 3, (6, 10), device_sources=(buf, offsets), out_sizes=sizes)
    with pytest.raises(ValueError):
        plan.run("cpu")
    # a window above the kernel's largest side is a host item and no item of the launch
    big = RS.ResamplePlan([(2, 2050), (3, 5)], [(8200, 8), (10, 6)], [(0, 0)] * 2, None,
                          device_sources=_buffer([(2, 2050), (3, 5)])[:2], out_sizes=[(8, 8200), (6, 10)])
    assert big.host_items == [0] and big.kernel_items == [1] and big.nk == 1 and big.dst[0].out_off == 3 * 8 * 8200
    assert big.host_pixels[0].shape == (8, 8200, 3)


def test_ragged_entry_refuses_bad_arguments_without_a_gpu():
    from vspbfr_amd import _lib
    from vspbfr_amd import resample as RS
    lib = _lib.lib
    shapes = [(33, 41), (16, 20)]
    buf, offsets, _ = _buffer(shapes)
    plan = RS.ResamplePlan(shapes, [(25, 20), (20, 16)], [(2, 1), (0, 0)], None, device_sources=(buf, offsets), out_sizes=[(16, 20), (16, 20)])
    assert [it.flags for it in plan.items] == [0, RS.COPY]
    d = C.c_void_p(256)     # non-null, aligned dummy "device" pointers: every refusal below comes before a launch
    out_bytes = plan.out_bytes

    def call(items=plan.items, dst=plan.dst, out=d, src=d, n=2, out_bytes=out_bytes, work_bytes=plan.work_bytes, coef_ints=plan.coef_ints,
             src_bytes=plan.src_bytes):
        return lib.vsp_lanczos_resize_ragged_u8(out, out_bytes, src, src_bytes, d, coef_ints, d, work_bytes,
                                                C.cast(items, C.c_void_p) if items else None, d, C.cast(dst, C.c_void_p) if dst else None, d,
                                                n, None)

    def edited(which=0, **kw):
        items = (RS.ResampleItem * 2)()
        C.memmove(items, plan.items, C.sizeof(items))
        for k, v in kw.items():
            setattr(items[which], k, v)
        return items

    def moved(which=0, **kw):
        dst = (RS.ResampleDst * 2)()
        C.memmove(dst, plan.dst, C.sizeof(dst))
        for k, v in kw.items():
            setattr(dst[which], k, v)
        return dst

    assert call(out=None) == -1 and "null pointer" in _lib.last_error()
    assert call(src=None) == -1 and call(items=None) == -1 and call(dst=None) == -1 and "null pointer" in _lib.last_error()
    assert call(n=-1) == -1 and call(n=0) == 0
    assert call(dst=moved(0, out_off=-1)) == -1 and "destination outside" in _lib.last_error()
    assert call(dst=moved(1, out_off=out_bytes - 959)) == -1 and "destination outside" in _lib.last_error()
    assert call(dst=moved(1, out_off=out_bytes + 1)) == -1 and "destination outside" in _lib.last_error()
    assert call(out_bytes=out_bytes - 1) == -1 and "destination outside" in _lib.last_error()
    assert call(dst=moved(1, out_off=959)) == -1 and "overlaps" in _lib.last_error()
    assert call(dst=moved(0, out_off=960), out_bytes=2 * out_bytes) == -1 and "overlaps" in _lib.last_error()      # descending
    assert call(dst=moved(0, H=0)) == -1 and "output size" in _lib.last_error()
    assert call(dst=moved(0, W=8193), out_bytes=1 << 30) == -3
    assert call(items=edited(0, x0=6)) == -1 and "outside the resized" in _lib.last_error()       # 6 + 20 > 25
    assert call(dst=moved(0, H=20), out_bytes=1 << 20) == -1 and "outside the resized" in _lib.last_error()        # 1 + 20 > 20
    assert call(dst=moved(1, W=19)) == -1 and "copy item" in _lib.last_error()
    assert call(items=edited(1, sw=21), src_bytes=1 << 20) == -1 and "copy item" in _lib.last_error()
    assert call(items=edited(0, hk=5)) == -1 and "tap counts" in _lib.last_error()
    assert call(items=edited(0, sw=0)) == -1 and "zero size" in _lib.last_error()
    assert call(items=edited(0, sw=17 * 25), src_bytes=1 << 20) == -3 and "16x" in _lib.last_error()
    assert call(items=edited(0, row1=33)) == -1 and "source rows" in _lib.last_error()
    assert call(items=edited(0, work_off=2)) == -1
    assert call(work_bytes=plan.work_bytes - 1) == -1 and "work bytes" in _lib.last_error()
    assert call(coef_ints=plan.coef_ints - 1) == -1 and "coefficient" in _lib.last_error()
    assert call(src_bytes=plan.src_bytes - 1) == -1 and "source" in _lib.last_error()
    assert call(items=edited(1, src_off=plan.src_bytes - 959), src_bytes=plan.src_bytes) == -1 and "source" in _lib.last_error()


def test_decode_batch_sends_host_files_through_the_pool():
    """jpeg.decode_batch(pool=...) hands the files of the host route to pool.map; the keyword is new and nothing else changes"""
    import inspect

    from vspbfr_amd import jpeg
    assert inspect.signature(jpeg.decode_batch).parameters["pool"].default is None
    assert inspect.signature(jpeg.decode_files).parameters["pool"].default is None
