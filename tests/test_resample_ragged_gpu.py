"""GPU checks of vsp_lanczos_resize_ragged_u8 (csrc/resample.hip) and of ResamplePlan's device sources: every item has a window of its
own and writes it into one packed buffer, from sources that lie in a device buffer at odd byte offsets.  The bytes equal live PIL's
Image.resize(..., LANCZOS) (+ crop) and the NumPy restatement (tests/resample_ref.py); the guard bytes between and behind the images
keep their fill.  Equality everywhere: no tolerance."""
import ctypes as C

import numpy as np
import pytest
import torch

import resample_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"
FILL, GUARD = 0xA5, 16


def _pil(a, nw, nh, box=None):
    from PIL import Image
    img = Image.fromarray(a)
    if img.size != (nw, nh):
        img = img.resize((nw, nh), Image.Resampling.LANCZOS)
    return np.asarray(img.crop(box) if box is not None else img)


class Batch:
    """items: (source uint8 (h, w, 3), (nw, nh), (x0, y0), (H, W)).  The sources lie back to back in a slice, at byte offset 1, of a
    larger device buffer whose other bytes are 0x5A; the destinations lie in one buffer with GUARD bytes between and behind them (and
    `lead` bytes in front, which puts destinations whose sizes are multiples of 4 off dword alignment too)."""

    def __init__(self, items, lead=0):
        self.items, self.lead = items, lead
        self.src_off, at = [], 0
        for a, *_ in items:
            self.src_off.append(at)
            at += a.size
        big = np.full(at + 1 + 7, 0x5A, dtype=np.uint8)
        for o, (a, *_) in zip(self.src_off, items):
            big[1 + o:1 + o + a.size] = a.reshape(-1)
        self.big = torch.from_numpy(big).to(DEV)
        self.buffer = self.big[1:1 + at]
        assert self.buffer.data_ptr() % 4 == 1
        self.out_off, at = [], lead
        for _, _, _, (H, W) in items:
            self.out_off.append(at)
            at += 3 * H * W + GUARD
        self.out_bytes = at

    def plan(self, which=None):
        from vspbfr_amd.resample import ResamplePlan
        which = range(len(self.items)) if which is None else which
        it = [self.items[k] for k in which]
        return ResamplePlan([i[0].shape[:2] for i in it], [i[1] for i in it], [i[2] for i in it], None,
                            device_sources=(self.buffer, [self.src_off[k] for k in which]), out_sizes=[i[3] for i in it],
                            out_offsets=[self.out_off[k] for k in which])

    def fresh(self):
        return torch.full((self.out_bytes,), FILL, dtype=torch.uint8, device=DEV)

    def images(self, out):
        """(the windows, whether every guard byte still holds the fill)"""
        o = out.cpu().numpy()
        mask = np.ones(o.size, dtype=bool)
        got = []
        for off, (_, _, _, (H, W)) in zip(self.out_off, self.items):
            got.append(o[off:off + 3 * H * W].reshape(H, W, 3))
            mask[off:off + 3 * H * W] = False
        assert mask.sum() == GUARD * len(self.items) + self.lead
        return got, bool((o[mask] == FILL).all())

    def check_all_routes(self, want):
        """one launch, one item per launch, a second stream and a repeat into the same buffer: Pillow's bytes and untouched guards"""
        plan = self.plan()
        out = plan.run_into(self.fresh())
        got, guards = self.images(out)
        for k, (g, w) in enumerate(zip(got, want)):
            print(f"item {k}: {self.items[k][0].shape[:2]} -> {g.shape[:2]}: differing bytes vs PIL {int((g != w).sum())}")
        assert guards
        for k, (g, w) in enumerate(zip(got, want)):
            assert np.array_equal(g, w), k
        single = self.fresh()
        for k in range(len(self.items)):
            self.plan([k]).run_into(single)
        assert torch.equal(single, out)
        torch.cuda.synchronize()
        side = torch.cuda.Stream()
        with torch.cuda.stream(side):
            other = plan.run_into(self.fresh())
            again = plan.run_into(other)
        side.synchronize()
        assert again is other and torch.equal(other, out)
        return plan, out


SOURCES = [(1, 1), (3, 5), (7, 4), (9, 9), (2, 171), (2, 345), (16, 33)]      # (h, w)


@pytest.mark.parametrize("factor", [2, 4])
def test_upscaled_group_in_one_ragged_launch(factor):
    """odd byte counts put every later source and destination off dword alignment; (2, 171) x 2 gives an output row of 1026 bytes, past
    one 1024-byte step of the vertical loop; (2, 345) a source row of 1035 bytes, past one step of the staging loop, and an output
    wider than the 256 columns of one step of the horizontal loop"""
    items, want = [], []
    for k, (h, w) in enumerate(SOURCES):
        a = R.test_image(w, h, seed=31 * h + w)
        items.append((a, (w * factor, h * factor), (0, 0), (h * factor, w * factor)))
        ref = _pil(a, w * factor, h * factor)
        assert np.array_equal(ref, R.resize(a, w * factor, h * factor)), (h, w)
        want.append(ref)
    b = Batch(items, lead=factor - 1)          # 3 (f h) (f w) is a multiple of 4: the lead byte(s) take the destinations off alignment
    plan, _ = b.check_all_routes(want)
    assert not plan.host_items and plan.nk == len(SOURCES)
    assert len({o % 4 for o in b.src_off}) >= 3 and all(o % 4 == factor - 1 for o in b.out_off)
    if factor == 2:
        assert 3 * items[4][3][1] == 1026
    assert 3 * SOURCES[5][1] == 1035 and items[5][3][1] > 256
    assert plan.upload_bytes == plan.pack()[3] and plan.src_bytes == b.buffer.numel()          # the tables alone go up: no source byte


def _mixed():
    """(items, Pillow's windows): a reduction, the largest reduction the kernel serves (16x) and the 33 -> 2 columns beside it (16.5x:
    that one is resized on the host and copied into its slot), a factor-1 copy, a non-uniform target, two cropped windows"""
    specs = [((40, 60), (20, 13), (0, 0), (13, 20)),          # (h, w) -> (nw, nh), window origin, window (H, W)
             ((5, 32), (2, 5), (0, 0), (5, 2)),
             ((5, 33), (2, 5), (0, 0), (5, 2)),
             ((11, 23), (23, 11), (0, 0), (11, 23)),
             ((7, 10), (25, 9), (0, 0), (9, 25)),
             ((33, 41), (25, 20), (2, 1), (16, 20)),
             ((61, 97), (64, 64), (37, 50), (14, 27))]
    items, want = [], []
    for (h, w), (nw, nh), (x0, y0), (H, W) in specs:
        a = R.test_image(w, h, seed=17 * h + w)
        items.append((a, (nw, nh), (x0, y0), (H, W)))
        ref = _pil(a, nw, nh, (x0, y0, x0 + W, y0 + H))
        assert np.array_equal(ref, R.resize_crop(a, nw, nh, x0, y0, H, W)), (h, w)
        want.append(ref)
    return items, want


def test_mixed_items_in_one_ragged_launch():
    from vspbfr_amd import resample as RS
    items, want = _mixed()
    b = Batch(items)
    plan, _ = b.check_all_routes(want)
    assert plan.host_items == [2] and plan.kernel_items == [0, 1, 3, 4, 5, 6] and len({o % 4 for o in b.out_off}) >= 2
    assert plan.items[1].hk == RS.MAX_TAPS and plan.items[2].flags == RS.COPY and (plan.items[5].x0, plan.items[5].y0) == (37, 50)


def test_refusals_leave_the_output_alone():
    """the refusals of the CPU test on the device build, with real buffers: the entry's code, and not one byte written"""
    from vspbfr_amd import _lib, hip_ops
    from vspbfr_amd import resample as RS
    items, _ = _mixed()
    b = Batch([items[5], items[3]])            # a resized window and a copy
    plan = b.plan()
    assert [it.flags for it in plan.items] == [0, RS.COPY]
    sections = plan._sections(DEV)
    out = b.fresh()
    keep_items, keep_dst = bytes(plan.items), bytes(plan.dst)

    def refused(code, why, item=None, dst=None, which=0):
        C.memmove(plan.items, keep_items, len(keep_items))
        C.memmove(plan.dst, keep_dst, len(keep_dst))
        for k, v in (item or {}).items():
            setattr(plan.items[which], k, v)
        for k, v in (dst or {}).items():
            setattr(plan.dst[which], k, v)
        with pytest.raises(RuntimeError, match=f"code {code}"):
            hip_ops.lanczos_resize_ragged_u8(plan, sections[0], sections[1], sections[3], sections[2], out)
        assert why in _lib.last_error(), _lib.last_error()

    refused(-1, "destination outside", dst=dict(out_off=-1))
    refused(-1, "destination outside", dst=dict(out_off=b.out_bytes - 3 * 11 * 23 + 1), which=1)
    refused(-1, "destination outside", dst=dict(out_off=b.out_bytes + 1), which=1)
    refused(-1, "overlaps", dst=dict(out_off=3 * 16 * 20 - 1), which=1)
    refused(-1, "outside the resized", item=dict(x0=6))
    refused(-1, "outside the resized", item=dict(y0=5))
    refused(-1, "copy item", dst=dict(W=22), which=1)
    refused(-1, "tap counts", item=dict(hk=5))
    refused(-3, "side above", dst=dict(W=8193))
    C.memmove(plan.items, keep_items, len(keep_items))
    C.memmove(plan.dst, keep_dst, len(keep_dst))
    rc = _lib.lib.vsp_lanczos_resize_ragged_u8(None, out.numel(), b.buffer.data_ptr(), plan.src_bytes, sections[1].data_ptr(), plan.coef_ints,
                                               None, plan.work_bytes, C.cast(plan.items, C.c_void_p), sections[0].data_ptr(),
                                               C.cast(plan.dst, C.c_void_p), sections[2].data_ptr(), 2, None)
    assert rc == -1 and "null pointer" in _lib.last_error()
    torch.cuda.synchronize()
    assert bool((out == FILL).all())
    # and the untouched tables do run
    got, guards = b.images(hip_ops.lanczos_resize_ragged_u8(plan, sections[0], sections[1], sections[3], sections[2], out))
    assert guards and np.array_equal(got[0], _pil(items[5][0], 25, 20, (2, 1, 22, 17))) and np.array_equal(got[1], items[3][0])


# the size pairs of the uniform entry's ragged test (tests/test_resample_gpu.py), restated: ((sw, sh), (nw, nh))
SIZE_PAIRS = [((1, 1), (8, 8)), ((7, 5), (16, 16)), ((40, 33), (64, 77)), ((64, 48), (43, 32)), ((97, 61), (64, 64)),
              ((513, 777), (512, 775)), ((300, 200), (768, 512)), ((1024, 1024), (512, 512)), ((1024, 64), (64, 4)), ((64, 64), (64, 64))]


def test_uniform_entry_with_device_sources_equals_uploaded_sources():
    """every pair with the 4 x 8 crop at the far corner, the seven larger ones with a 32 x 43 crop in the middle: the same call over
    sources that were uploaded with the plan and over sources that lie in a device buffer (at byte offset 1 of a larger one)"""
    from vspbfr_amd.resample import ResamplePlan
    srcs = [R.test_image(s[0], s[1], seed=s[0] * 7 + s[1]) for s, _ in SIZE_PAIRS]
    for (H, W), where in (((4, 8), "corner"), ((32, 43), "middle")):
        sel = [k for k, (_, d) in enumerate(SIZE_PAIRS) if d[0] >= W and d[1] >= H]
        assert len(sel) == (10 if where == "corner" else 7)
        targets = [SIZE_PAIRS[k][1] for k in sel]
        origins = [(nw - W, nh - H) if where == "corner" else ((nw - W) // 2, (nh - H) // 2) for nw, nh in targets]
        up = ResamplePlan([srcs[k] for k in sel], targets, origins, (H, W))
        want8, wantf = up.run(DEV, u8=True, f32=True)
        b = Batch([(srcs[k], None, None, (1, 1)) for k in sel])
        held = ResamplePlan([srcs[k].shape[:2] for k in sel], targets, origins, (H, W), device_sources=(b.buffer, b.src_off))
        assert not held.host_items and held.upload_bytes == up.pack()[0].numel() - up.src_bytes
        got8, gotf = held.run(DEV, u8=True, f32=True)
        assert torch.equal(got8, want8) and torch.equal(gotf.view(torch.int32), wantf.view(torch.int32)), where
        k = sel.index(5)                     # and Pillow itself for one of them
        (nw, nh), (x0, y0) = targets[k], origins[k]
        assert np.array_equal(got8[k].cpu().numpy(), _pil(srcs[5], nw, nh, (x0, y0, x0 + W, y0 + H)))
    with pytest.raises(ValueError, match="is on"):
        ResamplePlan([srcs[1].shape[:2]], [(16, 16)], [(0, 0)], (16, 16), device_sources=(torch.from_numpy(srcs[1].reshape(-1).copy()), [0])).run(DEV)


def test_a_host_item_among_device_sources_of_the_uniform_entry():
    """a 17x reduction among device sources: that slice alone comes back, PIL resizes it and it rides behind the buffer as a copy"""
    from vspbfr_amd.resample import ResamplePlan
    a, c = R.test_image(1088, 68, seed=17), R.test_image(97, 61, seed=5)
    b = Batch([(a, None, None, (1, 1)), (c, None, None, (1, 1))])
    plan = ResamplePlan([a.shape[:2], c.shape[:2]], [(64, 4), (64, 64)], [(0, 0), (0, 30)], (4, 64), device_sources=(b.buffer, b.src_off))
    assert plan.host_items == [0]
    got, _ = plan.run(DEV)
    assert np.array_equal(got[0].cpu().numpy(), _pil(a, 64, 4)) and np.array_equal(got[1].cpu().numpy(), _pil(c, 64, 64, (0, 30, 64, 34)))
