"""GPU: the ragged device PNG encoder (vsp_png_encode_ragged_u8, csrc/png.hip) against its host restatement tests/png_ragged_ref.py, byte
for byte: the filter types, the per-segment bytes, sizes and Adler parts in the workspace, the compacted payload and idat_bytes -- every
case of the restatement in ONE ragged batch and again one per call; independence of an image's bytes from its place in the batch, its
buffer offset modulo 4, the stream and the launch; guard bytes between the payloads, behind the last one and in the source buffer;
C = 1; PngWriter(encode="device").submit_photos; and the uniform entry on one 512^2 image as a guard on the shared compress stage."""
import io

import numpy as np
import pytest
import torch

import png_ragged_ref as RR
import png_ref as R

pytestmark = pytest.mark.gpu
GUARD = 64


def pack(imgs, gap=0, lead=0):
    """images back to back with `gap` guard bytes (0xC3) between and behind them and `lead` in front -> (flat array, offsets)"""
    parts, offsets, at = [np.full(lead, 0xC3, np.uint8)], [], lead
    for a in imgs:
        offsets.append(at)
        parts += [a.reshape(-1), np.full(gap, 0xC3, np.uint8)]
        at += a.size + gap
    return np.concatenate(parts), offsets


def device_encode(imgs, C, gap=0, lead=0, guard=GUARD):
    """-> per image dict(payload, segments, adler, types), the raw `out`, out_offsets, idat_bytes, and the source as read back"""
    from vspbfr_amd import hip_ops
    flat, offsets = pack(imgs, gap, lead)
    buf = torch.from_numpy(flat).cuda()
    sizes = [a.shape[:2] for a in imgs]
    out, idat, seg_adler, out_off, work, (rows, _, _, segs) = hip_ops.png_encode_ragged(buf, sizes, offsets, C, guard=guard)
    torch.cuda.synchronize()
    out, idat, work = out.cpu().numpy(), idat.cpu().numpy(), work.cpu().numpy()
    seg_adler = seg_adler.cpu().numpy().view(np.uint32)
    seg_bytes = work[segs * RR.SLOT_BYTES:segs * (RR.SLOT_BYTES + 4)].view(np.int32)
    types = work[segs * (RR.SLOT_BYTES + 4):]
    res = []
    for i, (h, w) in enumerate(sizes):
        s0, r0 = rows[i][4], rows[i][5]
        n = RR.segments(h, w, C)
        res.append({"payload": out[out_off[i]:out_off[i] + idat[i]].tobytes(),
                    "segments": [work[k * RR.SLOT_BYTES:k * RR.SLOT_BYTES + seg_bytes[k]].tobytes() for k in range(s0, s0 + n)],
                    "adler": [tuple(int(v) for v in seg_adler[k]) for k in range(s0, s0 + n)],
                    "types": types[r0:r0 + h].tolist()})
    assert np.array_equal(buf.cpu().numpy(), flat)                       # the source, its guard bytes included, is untouched
    return res, out, out_off, idat


def check_against_ref(got, enc, what):
    assert got["types"] == enc["types"].tolist(), what
    assert [len(s) for s in got["segments"]] == [len(s) for s in enc["segments"]], what
    assert got["segments"] == enc["segments"], what
    assert got["adler"] == [(a, b) for a, b, _ in enc["adler"]], what
    assert got["payload"] == enc["payload"], what


def check_guards(out, out_off, idat, sizes, C):
    """no byte of `out` outside the used ranges is written: behind every payload up to the next one, and behind the last"""
    used = np.zeros(out.size, dtype=bool)
    for o, nb in zip(out_off, idat):
        used[o:o + nb] = True
    assert np.all(out[~used] == 0xA5)
    for o, (h, w) in zip(out_off, sizes):                               # the layout leaves at least GUARD bytes behind every bound
        assert not used[o + RR.image_bound(h, w, C):o + RR.image_bound(h, w, C) + GUARD].any()


CASES3 = [c for c in RR.CASES if c[3] == 3]
CASES1 = [c for c in RR.CASES if c[3] == 1]


@pytest.mark.parametrize("cases", [CASES3, CASES1], ids=["C3", "C1"])
def test_one_ragged_batch_equals_the_restatement(cases):
    """rows wider than a segment (8200, 9000, 30000 px) and narrower than one (130, 341, 1 px) side by side; the images start at odd
    offsets (a guard of 5 bytes between them)"""
    C = cases[0][3]
    imgs = [RR.case_image(c)[0] for c in cases]
    res, out, out_off, idat = device_encode(imgs, C, gap=5, lead=3)
    for c, got in zip(cases, res):
        check_against_ref(got, RR.case_image(c)[1], RR.case_id(c))
    check_guards(out, out_off, idat, [a.shape[:2] for a in imgs], C)


@pytest.mark.parametrize("case", RR.CASES, ids=RR.case_id)
def test_one_image_per_call_equals_the_restatement(case):
    img, enc = RR.case_image(case)
    res, out, out_off, idat = device_encode([img], case[3])
    check_against_ref(res[0], enc, RR.case_id(case))
    assert int(idat[0]) == len(enc["payload"]) <= RR.image_bound(*img.shape)
    check_guards(out, out_off, idat, [img.shape[:2]], case[3])


def test_bytes_do_not_depend_on_place_offset_stream_or_launch():
    from vspbfr_amd import png
    cases = [("smooth", 5, 4099, 3), ("smooth", 25, 341, 3), ("constant", 30, 1000, 3), ("smooth", 67, 130, 3)]
    imgs = [RR.case_image(c)[0] for c in cases]
    want = [RR.encode_png(a) for a in imgs]
    sizes = [a.shape[:2] for a in imgs]
    for lead in range(4):                                                # the first image's offset modulo 4
        flat, offsets = pack(imgs, gap=lead, lead=lead)
        assert png.encode_ragged(torch.from_numpy(flat).cuda(), sizes, offsets) == want, lead
    order = [2, 0, 3, 1]                                                 # another place in the batch
    flat, offsets = pack([imgs[k] for k in order])
    buf = torch.from_numpy(flat).cuda()
    assert png.encode_ragged(buf, [sizes[k] for k in order]) == [want[k] for k in order]
    side = torch.cuda.Stream()
    side.wait_stream(torch.cuda.current_stream())
    with torch.cuda.stream(side):
        first = png.encode_ragged(buf, [sizes[k] for k in order], offsets)
        second = png.encode_ragged(buf, [sizes[k] for k in order], offsets)        # a second launch
    torch.cuda.current_stream().wait_stream(side)
    assert first == second == [want[k] for k in order]
    for k in range(4):                                                   # and alone
        assert png.encode_ragged(torch.from_numpy(imgs[k].reshape(-1).copy()).cuda(), [sizes[k]]) == [want[k]]


def test_files_decode_and_stay_under_the_size_cap():
    from PIL import Image

    from vspbfr_amd import png
    imgs = [R.named_image("smooth", 96, 1537, 3, seed=1), R.named_image("twolevel", 50, 2051, 3, seed=2)]
    flat, offsets = pack(imgs)
    files = png.encode_ragged(torch.from_numpy(flat).cuda(), [a.shape[:2] for a in imgs])
    for img, data in zip(imgs, files):
        H, W, C = img.shape
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), img)
        assert data == RR.encode_png(img)
        idat = int.from_bytes(data[33:37], "big")
        cap, ref = R.size_cap(R.filter_image(img)[0], RR.segments(H, W, C))
        print(f"{W}x{H}: IDAT {idat} zlib-RLE {ref} cap {cap:.0f}")
        assert idat <= cap


def test_grey_files():
    from PIL import Image

    from vspbfr_amd import png
    imgs = [RR.case_image(c)[0] for c in CASES1]
    flat, offsets = pack(imgs, gap=1)
    files = png.encode_ragged(torch.from_numpy(flat).cuda(), [a.shape[:2] for a in imgs], offsets, C=1)
    for img, data in zip(imgs, files):
        assert data == RR.encode_png(img)
        assert np.array_equal(np.asarray(Image.open(io.BytesIO(data))), img[:, :, 0])


def test_the_wrapper_refuses_what_the_entry_refuses():
    from vspbfr_amd import hip_ops
    buf = torch.zeros(4096, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="leaves src"):
        hip_ops.png_encode_ragged(buf, [(40, 40)])
    with pytest.raises(RuntimeError, match="overlaps"):
        hip_ops.png_encode_ragged(buf, [(10, 10), (10, 10)], [0, 299])
    with pytest.raises(RuntimeError):
        hip_ops.png_encode_ragged(buf, [(10, 10)], C=2)
    with pytest.raises(NotImplementedError):
        hip_ops.png_encode_ragged(buf, [(1, (1 << 20) // 3 + 1)])
    assert hip_ops.png_encode_ragged(buf, [])[3] == []


def test_submit_photos_writes_files_pil_decodes(tmp_path):
    from PIL import Image

    from vspbfr_amd.imageio import PngWriter
    imgs = [R.named_image("smooth", 40, 3001, 3, seed=5), R.named_image("smooth", 33, 65, 3, seed=6), R.named_image("noise", 9, 1200, 3, seed=7)]
    flat, offsets = pack(imgs)
    buf = torch.from_numpy(flat).cuda()
    sizes = [a.shape[:2] for a in imgs]
    for encode in ("device", "host"):
        paths = [str(tmp_path / f"{encode}_{k}.png") for k in range(3)]
        w = PngWriter(workers=2, encode=encode)
        w.submit_photos(buf, sizes, offsets, paths)
        w.drain()
        for p, img in zip(paths, imgs):
            assert np.array_equal(np.asarray(Image.open(p)), img)
            assert (open(p, "rb").read() == RR.encode_png(img)) == (encode == "device")     # the device wrote it, not PIL


def test_the_uniform_entry_still_equals_its_restatement():
    """the compress stage is shared with vsp_png_encode_u8: one 512^2 image through it"""
    from vspbfr_amd import png
    img = R.named_image("smooth", 512, 512, 3, seed=3)
    (data,) = png.encode_batch(torch.from_numpy(img[None].copy()).cuda())
    assert data == R.encode_png(img)
