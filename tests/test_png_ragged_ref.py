"""CPU checks of tests/png_ragged_ref.py, the host restatement of the ragged device PNG encoder: zlib inflates its stream to the filtered
bytes, PIL decodes the assembled file to the input, the combined Adler-32 is zlib's, no segment exceeds its bound and the IDAT stays under
png_ref.size_cap with the number of byte segments.  Then the host-side refusals of vsp_png_encode_ragged_u8, which launch nothing, and the
PIL fall-back of png.encode_ragged."""
import ctypes as C
import io

import numpy as np
import pytest

import png_ragged_ref as RR


@pytest.mark.parametrize("case", RR.CASES, ids=RR.case_id)
def test_restatement(case):
    kind, H, W, Cc = case
    img, enc = RR.case_image(case)
    size, cap, ref = RR.check_image(img, enc, RR.assemble(enc["zlib"], H, W, Cc))
    print(f"{RR.case_id(case)}: IDAT {size} zlib-RLE {ref} cap {cap:.0f} raw {enc['filtered'].size} segments {len(enc['segments'])}")
    assert size <= cap


def test_the_boundary_cases_hit_what_they_are_for():
    S = RR.SEG_BYTES
    assert S % (1 + 3 * 341) == 0                                   # segment 1 starts on a filter byte
    assert 25 * (1 + 982) == S - 1                                  # the filter byte of row 25 is segment 0's last byte
    assert 1 + 3 * 8192 == S + 1 and 1 + 3 * 8191 == S - 2
    assert 1 + 24576 == S + 1
    for case, nseg in ((("smooth", 25, 341, 3), 2), (("smooth", 26, 982, 1), 2), (("smooth", 1, 8192, 3), 2), (("smooth", 1, 8191, 3), 1),
                       (("smooth", 2, 24576, 1), 3), (("constant", 30, 1000, 3), 4)):
        assert case in RR.CASES and len(RR.case_image(case)[1]["segments"]) == nseg
    _, enc = RR.case_image(("smooth", 25, 341, 3))
    assert enc["filtered"].reshape(-1)[S] == enc["types"][24]
    _, enc = RR.case_image(("smooth", 26, 982, 1))
    assert enc["filtered"].reshape(-1)[S - 1] == enc["types"][25]
    # the constant image: zeros on both sides of every boundary, so a run is cut there; the pieces still inflate to the stream
    _, enc = RR.case_image(("constant", 30, 1000, 3))
    flat = enc["filtered"].reshape(-1)
    assert all(flat[k * S - 1] == flat[k * S] == 0 for k in (1, 2, 3))
    # the stored form reaches the per-segment bound exactly
    _, enc = RR.case_image(("noise", 4, 5000, 3))
    assert len(enc["segments"][0]) == S + 10


# ---- the entry's host-side checks: dummy non-null pointers that the checks never dereference
def _items(rows):
    from vspbfr_amd import _lib
    return (_lib.PngItem * len(rows))(*(_lib.PngItem(*r) for r in rows))


def _valid():
    """two images, 20 x 30 and 7 x 5000, back to back"""
    from vspbfr_amd import _lib
    lib = _lib.lib
    b0 = lib.vsp_png_ragged_image_bound(20, 30, 3)
    s0 = lib.vsp_png_ragged_segments(20, 30, 3)
    s1 = lib.vsp_png_ragged_segments(7, 5000, 3)
    rows = [(0, 0, 20, 30, 0, 0), (1800, b0, 7, 5000, s0, 20)]
    p = C.c_void_p(4096)
    return dict(out=p, out_bytes=b0 + lib.vsp_png_ragged_image_bound(7, 5000, 3), idat=p, adler=p, work=p,
                work_bytes=lib.vsp_png_ragged_work_bytes(s0 + s1, 27), src=p, src_bytes=1800 + 7 * 5000 * 3, rows=rows, items_dev=p, n=2, C=3)


def _call(a):
    from vspbfr_amd import _lib
    items = None if a["rows"] is None else C.cast(_items(a["rows"]), C.c_void_p)
    rc = _lib.lib.vsp_png_encode_ragged_u8(a["out"], a["out_bytes"], a["idat"], a["adler"], a["work"], a["work_bytes"], a["src"],
                                           a["src_bytes"], items, a["items_dev"], a["n"], a["C"], None)
    return rc, _lib.last_error()


def _edit(which, **kw):
    def make():
        rows = _valid()["rows"]
        names = ("src_off", "out_off", "h", "w", "seg0", "row0")
        f = dict(zip(names, rows[which]))
        f.update(kw)
        rows[which] = tuple(f[k] for k in names)
        return rows
    return make


REFUSALS = [
    (dict(C=2), -1, "channels"), (dict(C=4), -1, "channels"), (dict(n=-1), -1, "images"),
    (dict(out=None), -1, "null pointer"), (dict(idat=None), -1, "null pointer"), (dict(adler=None), -1, "null pointer"),
    (dict(work=None), -1, "null pointer"), (dict(src=None), -1, "null pointer"), (dict(rows=None), -1, "null pointer"),
    (dict(items_dev=None), -1, "null pointer"), (dict(work=C.c_void_p(4098)), -1, "aligned"),
    (dict(rows=_edit(0, h=0)), -1, "0 x 30"), (dict(rows=_edit(1, w=0)), -1, "7 x 0"), (dict(rows=_edit(0, w=-3)), -1, "20 x -3"),
    (dict(rows=_edit(1, src_off=1799)), -1, "overlaps"),            # overlapping images
    (dict(rows=_edit(0, src_off=-1)), -1, "overlaps"),
    (dict(src_bytes=1800 + 7 * 5000 * 3 - 1), -1, "leaves src"),    # image past src_bytes
    (dict(rows=_edit(1, out_off=100)), -1, "output range"),         # overlapping output ranges
    (dict(out_bytes=1000), -1, "output range"),
    (dict(rows=_edit(1, seg0=0)), -1, "seg0"), (dict(rows=_edit(1, row0=19)), -1, "row0"),
    (dict(work_bytes=24588), -1, "work of"),                        # short workspace
    (dict(rows=_edit(1, w=(1 << 20) // 3 + 1)), -3, "rows of"),     # row above the limit
    (dict(n=4097), -3, "images"),
    (dict(src_bytes=1 << 31), -3, "2 GiB"), (dict(out_bytes=1 << 31), -3, "2 GiB"), (dict(work_bytes=1 << 31), -3, "2 GiB"),
]


@pytest.mark.parametrize("change,code,fragment", REFUSALS, ids=lambda v: str(v) if not isinstance(v, dict) else ",".join(v))
def test_the_entry_refuses_on_the_host(change, code, fragment):
    a = _valid()
    a.update({k: (v() if callable(v) else v) for k, v in change.items()})
    rc, msg = _call(a)
    assert rc == code and msg.startswith("png_encode_ragged:") and fragment in msg, (rc, msg)


def test_size_helpers_and_an_empty_call():
    from vspbfr_amd import _lib
    lib = _lib.lib
    assert lib.vsp_abi_version() == 4 and lib.vsp_struct_size(14) == C.sizeof(_lib.PngItem) == 32
    for kind, H, W, Cc in RR.CASES:
        assert lib.vsp_png_ragged_segments(H, W, Cc) == RR.segments(H, W, Cc)
        assert lib.vsp_png_ragged_image_bound(H, W, Cc) == RR.image_bound(H, W, Cc)
    assert lib.vsp_png_ragged_segments(1024, 1536, 3) == 193
    assert lib.vsp_png_ragged_work_bytes(3, 10) == 3 * (RR.SLOT_BYTES + 4) + 12
    for bad in ((0, 5, 3), (5, 0, 3), (5, 5, 2), (5, (1 << 20) + 1, 1), (1 << 16, 1 << 15, 1)):
        assert lib.vsp_png_ragged_segments(*bad) == 0 and lib.vsp_png_ragged_image_bound(*bad) == 0
    assert lib.vsp_png_ragged_segments(5, 1 << 20, 1) == RR.segments(5, 1 << 20, 1)
    a = _valid()
    a.update(n=0, out=None, src=None, rows=None)
    assert _call(a)[0] == 0


def test_ragged_serves():
    from vspbfr_amd import png
    assert png.ragged_serves([(1024, 1536), (4096, 6144), (1, 1)], 3) and png.ragged_serves([(3, 1 << 20)], 1)
    assert not png.ragged_serves([], 3) and not png.ragged_serves([(4, 4)], 2) and not png.ragged_serves([(0, 4)], 3)
    assert not png.ragged_serves([(4, (1 << 20) // 3 + 1)], 3)             # row above the limit
    assert not png.ragged_serves([(1 << 15, 1 << 15)], 3)                  # 3 GiB
    assert not png.ragged_serves([(16384, 16384)] * 3, 3)                  # every image fits, the call does not
    assert not png.ragged_serves([(1, 1)] * 4097, 3)


def test_encode_ragged_falls_back_to_pil(monkeypatch):
    """ragged_serves false -> PIL's files, no kernel: the device route is made to raise, the tensors live on the CPU"""
    import torch
    from PIL import Image

    from vspbfr_amd import png

    def boom(*a, **k):
        raise AssertionError("the device route must not run")
    monkeypatch.setattr(png, "ragged_serves", lambda sizes, C=3: False)
    monkeypatch.setattr(png, "RaggedJob", boom)
    a, b = RR.named_image("smooth", 5, 9, 3), RR.named_image("noise", 3, 4, 3)
    buf = torch.from_numpy(np.concatenate([a.reshape(-1), np.zeros(2, np.uint8), b.reshape(-1)]))
    files = png.encode_ragged(buf, [(5, 9), (3, 4)], [0, a.size + 2])
    assert [np.array_equal(np.asarray(Image.open(io.BytesIO(f))), im) for f, im in zip(files, (a, b))] == [True, True]
    g = RR.named_image("smooth", 4, 6, 1)
    (f,) = png.encode_ragged(torch.from_numpy(g.reshape(-1).copy()), [(4, 6)], C=1)
    assert np.array_equal(np.asarray(Image.open(io.BytesIO(f))), g[:, :, 0])
    assert png.encode_ragged(buf[:0], []) == []
    with pytest.raises(RuntimeError):
        png.encode_ragged(buf, [(5, 9), (3, 4)], [0, a.size + 3])              # the second image leaves the buffer
