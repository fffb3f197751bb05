"""GPU checks of vsp_lanczos_resize_u8 (csrc/resample.hip through vspbfr_amd/resample.py): the kernel's bytes equal live PIL's
Image.resize(..., LANCZOS) + crop and the NumPy restatement (tests/resample_ref.py), in ragged launches and one item per launch, with
sources off dword alignment, crops at every edge, mirrored reads, non-uniform scaling, both outputs, copies, the 16x limit and the host
fallback above it, a second stream and repeats.  Equality everywhere: no tolerance."""
import numpy as np
import pytest
import torch

import resample_ref as R

pytestmark = pytest.mark.gpu
DEV = "cuda"


def _pil(a, nw, nh, box=None, flip=False):
    from PIL import Image
    img = Image.fromarray(a)
    if flip:
        img = img.transpose(Image.FLIP_LEFT_RIGHT)
    if img.size != (nw, nh):
        img = img.resize((nw, nh), Image.Resampling.LANCZOS)
    return np.asarray(img.crop(box) if box is not None else img)


def _run(items, im_size, u8=True, f32=False):
    """items: (source, (nw, nh), (x0, y0), flip) -> (plan, u8 numpy or None, f32 numpy or None) of ONE launch"""
    from vspbfr_amd.resample import ResamplePlan
    plan = ResamplePlan([i[0] for i in items], [i[1] for i in items], [i[2] for i in items], im_size, [i[3] for i in items])
    o8, of = plan.run(DEV, u8=u8, f32=f32)
    return plan, (None if o8 is None else o8.cpu().numpy()), (None if of is None else of.cpu().numpy())


@pytest.fixture(scope="module")
def cases():
    """the issue's size pairs: source, and PIL's resized image (computed once, never written to)"""
    out = []
    for src, dst in R.SIZE_PAIRS:
        a = R.test_image(src[0], src[1], seed=src[0] * 7 + src[1])
        ref = _pil(a, dst[0], dst[1])
        ref.setflags(write=False)
        out.append((a, dst, ref))
    return out


def test_every_size_pair_one_item_per_launch(cases):
    for a, (nw, nh), ref in cases:
        plan, got, _ = _run([(a, (nw, nh), (0, 0), False)], (nh, nw))
        assert not plan.host_items
        print(f"{a.shape[1]}x{a.shape[0]} -> {nw}x{nh}: differing bytes vs PIL {int((got[0] != ref).sum())}")
        assert np.array_equal(got[0], ref)
        assert np.array_equal(got[0], R.resize(a, nw, nh))


def test_ragged_launch_equals_one_by_one(cases):
    """all ten pairs in one launch with the crop every resized image can hold (4 x 8, at the far corner), and the seven larger ones with
    a 32 x 43 crop in the middle: sources after one of odd size sit off dword alignment in the packed buffer, and the rows of an
    odd-width source start 1, 2 and 3 bytes off"""
    for (H, W), sel, where in (((4, 8), cases, "corner"), ((32, 43), [c for c in cases if c[1][0] >= 43 and c[1][1] >= 32], "middle")):
        items = []
        for a, (nw, nh), ref in sel:
            x0, y0 = (nw - W, nh - H) if where == "corner" else ((nw - W) // 2, (nh - H) // 2)
            items.append((a, (nw, nh), (x0, y0), False))
        plan, got, _ = _run(items, (H, W))
        assert not plan.host_items and len({it.src_off % 4 for it in plan.items}) >= 3
        for k, ((a, (nw, nh), ref), it) in enumerate(zip(sel, items)):
            x0, y0 = it[2]
            assert np.array_equal(got[k], ref[y0:y0 + H, x0:x0 + W]), (where, k)
            _, one, _ = _run([it], (H, W))
            assert np.array_equal(one[0], got[k]), (where, k)


def test_width_sweep_ragged_and_one_by_one():
    """every source width 33..160 -> 32 at height 8: 128 items, rows at every misalignment (3 * w * row bytes), every tap count 9..33"""
    items = [(R.test_image(src[0], src[1], seed=src[0]), dst, (0, 0), False) for src, dst in R.SWEEP]
    plan, got, _ = _run(items, (8, 32))
    assert plan.n == 128 and not plan.host_items
    for k, it in enumerate(items):
        assert np.array_equal(got[k], _pil(it[0], 32, 8)), it[0].shape
        assert np.array_equal(got[k], R.resize(it[0], 32, 8))
        _, one, _ = _run([it], (8, 32))
        assert np.array_equal(one[0], got[k])


def test_crop_origins_and_flip():
    """a wide and a tall source covered to 48 x 40 (H x W): crop at 0, at the maximum and in the middle, mirrored and not"""
    from vspbfr_amd.resample import cover_geometry
    H, W = 48, 40
    items, want = [], []
    for (w, h) in ((203, 64), (80, 190)):
        a = R.test_image(w, h, seed=w)
        nw, nh, _ = cover_geometry(w, h, (H, W))
        assert nw >= W and nh >= H and (nw > W or nh > H)
        for flip in (False, True):
            for x0, y0 in {(0, 0), (nw - W, nh - H), ((nw - W) // 2, (nh - H) // 2)}:
                items.append((a, (nw, nh), (x0, y0), flip))
                want.append(_pil(a, nw, nh, (x0, y0, x0 + W, y0 + H), flip))
    plan, got, _ = _run(items, (H, W))
    assert not plan.host_items and len(items) >= 10
    for k in range(len(items)):
        assert np.array_equal(got[k], want[k]), items[k][1:]
        assert np.array_equal(got[k], R.resize_crop(items[k][0], *items[k][1], *items[k][2], H, W, items[k][3]))


def test_non_uniform_scaling_like_load_pair(tmp_path):
    """load_pair: the HQ image's size decides the resize and the crop of both; the LQ file of another aspect is stretched"""
    from PIL import Image
    from vspbfr_amd.imageio import load_pair
    from vspbfr_amd.resample import cover_geometry
    hq, lq = R.test_image(100, 80, seed=1), R.test_image(70, 90, seed=2)
    Image.fromarray(hq).save(tmp_path / "hq.png")
    Image.fromarray(lq).save(tmp_path / "lq.png")
    im_size = (48, 64)
    want_lq, want_hq = load_pair(str(tmp_path / "lq.png"), str(tmp_path / "hq.png"), im_size)
    nw, nh, box = cover_geometry(100, 80, im_size)
    plan, _, got = _run([(lq, (nw, nh), box[:2], False), (hq, (nw, nh), box[:2], False)], im_size, u8=False, f32=True)
    assert not plan.host_items
    assert np.array_equal(got[0].view(np.int32), want_lq.numpy().view(np.int32))
    assert np.array_equal(got[1].view(np.int32), want_hq.numpy().view(np.int32))


def test_both_outputs_and_every_byte_value():
    """uint8 NHWC and fp32 NCHW from one call; the fp32 equals imageio._to_tensor of the uint8 bitwise, for all 256 byte values (a copy
    item holding each of them) and for a resized item"""
    from vspbfr_amd.imageio import _to_tensor
    H, W = 16, 48
    ramp = np.arange(H * W * 3, dtype=np.int64).reshape(H, W, 3).astype(np.uint8)
    assert len(np.unique(ramp)) == 256
    a = R.test_image(97, 61, seed=5)
    plan, u8, f32 = _run([(ramp, (W, H), (0, 0), False), (a, (64, 40), (9, 13), False), (ramp, (W, H), (0, 0), True)], (H, W), u8=True, f32=True)
    assert [it.flags & 2 for it in plan.items] == [2, 0, 2]
    assert np.array_equal(u8[0], ramp) and np.array_equal(u8[2], ramp[:, ::-1])        # a source of the target size is copied exactly
    assert np.array_equal(u8[1], _pil(a, 64, 40, (9, 13, 9 + W, 13 + H)))
    for k in range(3):
        assert np.array_equal(f32[k].view(np.int32), _to_tensor(u8[k]).numpy().view(np.int32)), k
    _, only8, _ = _run([(a, (64, 40), (9, 13), False)], (H, W), u8=True, f32=False)
    _, _, onlyf = _run([(a, (64, 40), (9, 13), False)], (H, W), u8=False, f32=True)
    assert np.array_equal(only8[0], u8[1]) and np.array_equal(onlyf[0].view(np.int32), f32[1].view(np.int32))


def test_sixteen_fold_is_served_and_seventeen_fold_falls_back():
    a16, a17 = R.test_image(1024, 64, seed=16), R.test_image(1088, 68, seed=17)
    plan, got, _ = _run([(a16, (64, 4), (0, 0), False), (a17, (64, 4), (0, 0), False), (a17, (64, 4), (0, 0), True)], (4, 64))
    assert plan.host_items == [1, 2] and plan.items[0].hk == plan.items[0].vk == 97
    assert np.array_equal(got[0], _pil(a16, 64, 4)) and np.array_equal(got[0], R.resize(a16, 64, 4))
    assert np.array_equal(got[1], _pil(a17, 64, 4)) and np.array_equal(got[2], _pil(a17, 64, 4, flip=True))
    # the entry itself refuses the 17x item
    from vspbfr_amd import _lib, hip_ops as Hh
    from vspbfr_amd import resample as RS
    plan.items[1].sw, plan.items[1].sh, plan.items[1].flags = 1088, 68, 0
    host, nb, c0, s0 = plan.pack()
    dev = host.to(DEV)
    with pytest.raises(RuntimeError, match="code -3"):
        Hh.lanczos_resize_u8(plan, dev[:nb], dev[c0:c0 + plan.coef.nbytes], dev[s0:])
    assert "16x" in _lib.last_error() and RS.MAX_TAPS == 97


def test_second_stream_and_repeats(cases):
    a, (nw, nh), ref = cases[5]     # 513x777 -> 512x775
    b = cases[2][0]
    from vspbfr_amd.resample import ResamplePlan
    H, W = 60, 70
    plan = ResamplePlan([a, b, a], [(nw, nh), (70, 77), (nw, nh)], [(221, 300), (0, 17), (442, 715)], (H, W), [False, True, False])
    first8, firstf = plan.run(DEV, u8=True, f32=True)
    torch.cuda.synchronize()
    assert np.array_equal(first8[0].cpu().numpy(), ref[300:360, 221:291]) and np.array_equal(first8[2].cpu().numpy(), ref[715:775, 442:512])
    side = torch.cuda.Stream()
    with torch.cuda.stream(side):
        outs = [plan.run(DEV, u8=True, f32=True) for _ in range(2)]
    side.synchronize()
    for o8, of in outs:
        assert torch.equal(o8, first8) and torch.equal(of.view(torch.int32), firstf.view(torch.int32))
