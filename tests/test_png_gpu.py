"""GPU: the device PNG encoder (vsp_png_encode_u8, csrc/png.hip) against its host restatement tests/png_ref.py, byte for byte: the deflate
segments, their sizes and the Adler parts; whole files through PIL and the size cap at 512^2; independence of an image's bytes from its
place in the batch, the stream and the launch; the guard bytes behind every image's capacity; refusals and the host path above the
limits."""
import ctypes as C
import io

import numpy as np
import pytest
import torch

import png_ref as R

pytestmark = pytest.mark.gpu

SMALL = [(1, 1), (1, 7), (7, 1), (33, 65), (130, 67), (40, 33), (33, 40)]       # width x height
CASES = [(k, w, h, c) for (w, h) in SMALL for k in R.KINDS for c in (3, 1)]
CASES += [("constant", 64, 300, 3), ("constant", 300, 64, 3), ("constant", 300, 64, 1), ("noise", 1024, 9, 3), ("twolevel", 3072, 8, 1)]


def device_encode(batch, guard=0):
    """(B, H, W, C) uint8 array -> per image (segments [bytes], adler [(a, b)]), and the raw output rows"""
    from vspbfr_amd import hip_ops
    u8 = torch.from_numpy(np.ascontiguousarray(batch)).cuda()
    out, seg_bytes, seg_adler, slot = hip_ops.png_encode(u8, guard=guard)
    torch.cuda.synchronize()
    out, seg_bytes, seg_adler = out.cpu().numpy(), seg_bytes.cpu().numpy(), seg_adler.cpu().numpy().view(np.uint32)
    res = []
    for i in range(batch.shape[0]):
        segs = [out[i, k * slot:k * slot + seg_bytes[i, k]].tobytes() for k in range(seg_bytes.shape[1])]
        res.append((segs, [tuple(int(v) for v in seg_adler[i, k]) for k in range(seg_bytes.shape[1])]))
    return res, out, seg_bytes, slot


@pytest.mark.parametrize("kind,W,H,C", CASES, ids=lambda v: str(v))
def test_device_stream_equals_the_restatement(kind, W, H, C):
    img = R.named_image(kind, H, W, C)
    ref = R.encode_image(img)
    (segs, adler), = device_encode(img[None])[0]
    assert [len(s) for s in segs] == [len(s) for s in ref["segments"]]
    assert segs == ref["segments"]
    assert adler == [(a, b) for a, b, _ in ref["adler"]]


@pytest.fixture(scope="module")
def big():
    """five 512^2 images (smooth and two-level by turns, different seeds), their files from png.encode_batch"""
    from vspbfr_amd import png
    imgs = np.ascontiguousarray(np.stack([R.named_image(("smooth", "twolevel")[i % 2], 512, 512, 3, seed=i) for i in range(5)]))
    files = png.encode_batch(torch.from_numpy(imgs).cuda())
    return imgs, files


def test_files_decode_and_stay_under_the_size_cap(big):
    from PIL import Image
    imgs, files = big
    assert len(files) == 5
    for i, (img, data) in enumerate(zip(imgs, files)):
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), img)
        assert data[:8] == b"\x89PNG\r\n\x1a\n" and data[12:16] == b"IHDR" and data[37:41] == b"IDAT" and data[-8:-4] == b"IEND"
        idat = int.from_bytes(data[33:37], "big")
        filt, _ = R.filter_image(img)
        cap, ref = R.size_cap(filt, 64)
        buf = io.BytesIO()
        Image.fromarray(img).save(buf, format="PNG")
        print(f"image {i} ({('smooth', 'twolevel')[i % 2]}): IDAT {idat} zlib-RLE {ref} cap {cap:.0f} PIL file {len(buf.getvalue())} file {len(data)}")
        assert idat <= cap


def test_one_big_file_equals_the_restatement(big):
    imgs, files = big
    assert files[1] == R.encode_png(imgs[1]) and files[2] == R.encode_png(imgs[2])


def test_bytes_do_not_depend_on_batch_position_stream_or_launch():
    from vspbfr_amd import png
    imgs = np.ascontiguousarray(np.stack([R.named_image(k, 67, 130, 3, seed=s) for s, k in enumerate(("smooth", "noise", "twolevel", "ramp", "smooth"))]))
    want = [R.encode_png(a) for a in imgs]
    dev = torch.from_numpy(imgs).cuda()
    assert png.encode_batch(dev) == want
    assert png.encode_batch(dev) == want                                  # a second launch
    for i in (0, 4):
        assert png.encode_batch(dev[i:i + 1].contiguous()) == [want[i]]     # alone
    swapped = dev[[4, 1, 2, 3, 0]].contiguous()
    assert png.encode_batch(swapped) == [want[k] for k in (4, 1, 2, 3, 0)]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        got = png.encode_batch(dev)
    torch.cuda.current_stream().wait_stream(side)
    assert got == want
    odd = dev.reshape(-1)[3 * 130 * 67:].reshape(4, 67, 130, 3)           # a view that starts one image in: rows off dword alignment
    assert odd.data_ptr() % 4 != 0 and png.encode_batch(odd) == want[1:]


def test_guard_bytes_behind_every_image_are_untouched():
    imgs = np.stack([R.named_image(k, 33, 40, 3, seed=s) for s, k in enumerate(("noise", "smooth", "constant"))])
    res, out, seg_bytes, slot = device_encode(imgs, guard=64)
    cap = R.image_bound(33, 40, 3)
    assert out.shape == (3, cap + 64) and slot == R.segment_bound(R.ROWS, 40, 3)
    assert (out[:, cap:] == 0xA5).all()
    for i in range(3):
        assert res[i][0] == R.encode_image(imgs[i])["segments"]
        for k in range(seg_bytes.shape[1]):
            end = k * slot + (int(seg_bytes[i, k]) + 3) // 4 * 4
            assert int(seg_bytes[i, k]) <= R.segment_bound(min(R.ROWS, 33 - k * R.ROWS), 40, 3)
            assert (out[i, end:(k + 1) * slot] == 0xA5).all()              # the rest of the slot too


def test_refusals_and_limits():
    from PIL import Image
    from vspbfr_amd import _lib, hip_ops, png
    x = torch.zeros(2, 16, 16, 3, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError):
        hip_ops.png_encode(x[:, :, ::2])
    with pytest.raises(RuntimeError):
        hip_ops.png_encode(x.float())
    with pytest.raises(RuntimeError):
        png.encode_batch(x.permute(0, 2, 1, 3))
    with pytest.raises(RuntimeError):
        hip_ops.png_encode(torch.zeros(2, 16, 16, 2, dtype=torch.uint8, device="cuda"))
    # the C entry: above the limits VSP_ENOTSUP, a wrong argument VSP_EINVAL, both before any launch (the pointers are never used)
    lib = _lib.lib
    p = C.c_void_p(x.data_ptr())
    assert lib.vsp_png_bound(16, 1025, 3) == 0 and lib.vsp_png_bound(32769, 16, 3) == 0 and lib.vsp_png_segment_bound(9, 16, 3) == 0
    assert lib.vsp_png_bound(33, 40, 3) == R.image_bound(33, 40, 3) and lib.vsp_png_segment_bound(1, 40, 3) == R.segment_bound(1, 40, 3)
    assert lib.vsp_png_encode_u8(p, 1 << 20, p, p, p, 1, 2, 1025, 3, None) == -3 and "limits" in _lib.last_error()
    assert lib.vsp_png_encode_u8(p, 1 << 20, p, p, p, 1, 32769, 4, 1, None) == -3
    assert lib.vsp_png_encode_u8(p, 1 << 20, p, p, p, 1, 4, 4, 2, None) == -1
    assert lib.vsp_png_encode_u8(p, 8, p, p, p, 1, 4, 4, 3, None) == -1 and "vsp_png_bound" in _lib.last_error()
    assert lib.vsp_png_encode_u8(None, 1 << 20, p, p, p, 1, 4, 4, 3, None) == -1
    with pytest.raises(NotImplementedError):
        hip_ops.png_encode(torch.zeros(1, 2, 1025, 3, dtype=torch.uint8, device="cuda"))
    wide = R.named_image("smooth", 2, 1025, 3)
    files = png.encode_batch(torch.from_numpy(wide[None]).cuda())
    assert len(files) == 1 and np.array_equal(np.asarray(Image.open(io.BytesIO(files[0]))), wide)
    grey = R.named_image("smooth", 20, 31, 1)
    files = png.encode_batch(torch.from_numpy(grey[None]).cuda())
    assert files == [R.encode_png(grey)] and np.array_equal(np.asarray(Image.open(io.BytesIO(files[0]))), grey[:, :, 0])
