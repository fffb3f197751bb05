"""CPU checks of the JPEG encoder's host side: tests/jpeg_ref.py, the NumPy restatement of csrc/jpeg.hip, writes Pillow's bytes for every
case the GPU test runs; vspbfr_amd.jpeg.assemble frames as the restatement does; the C entry refuses bad arguments before any launch;
and the case list reaches what it is meant to reach (asserted from the restatement's counters, so it cannot lapse silently)."""
import ctypes as C

import numpy as np
import pytest

import jpeg_ref as R

CASES = R.thinned_cases()
_cache = {}


def _encoded(case):
    if case not in _cache:
        kind, h, w, quality, sub, restart = case
        _cache[case] = R.encode(R.named_image(kind, h, w), quality, sub, restart)
    return _cache[case]


@pytest.mark.parametrize("case", CASES, ids=lambda v: "-".join(str(x) for x in v))
def test_restatement_equals_pillow(case):
    kind, h, w, quality, sub, restart = case
    enc = _encoded(case)
    ref = R.pillow_file(R.named_image(kind, h, w), quality, sub, restart)
    print(case, len(ref), enc["counters"])
    assert enc["file"] == ref


def test_every_listed_value_appears():
    assert {(h, w) for _, h, w, *_ in CASES} == set(R.SIZES) and sum((h, w) == (512, 512) for _, h, w, *_ in CASES) == 1
    assert {c[3] for c in CASES} == set(R.QUALITIES) and {c[4] for c in CASES} == {"420", "444"} and {c[0] for c in CASES} == set(R.KINDS)
    assert {R.restart_values(h, w, sub).index(r) for _, h, w, _, sub, r in CASES} == {0, 1, 2, 3, 4}
    assert 30 <= len(CASES) <= 60


def test_coverage_of_the_case_list():
    """ZRL, stuffed bytes, the largest categories, a short last interval, RSTm wrapping past 7.  The largest categories of the 8-bit
    path: the DC coefficient of level-shifted samples lies in [-1024, 1016] at a quantiser of 1, so a difference reaches 2040 =
    category 11; an AC coefficient stays below 1024 in magnitude = category 10 (T.81 tables F.1 and F.2 end there for 8 bits)."""
    cnt = [_encoded(c)["counters"] for c in CASES]
    assert any(c["zrl"] > 0 for c in cnt)
    assert any(c["stuffed"] > 0 for c in cnt)
    assert max(c["dc_cat"] for c in cnt) == 11
    assert max(c["ac_cat"] for c in cnt) == 10
    assert any(c["intervals"] > 1 and c["last_interval_mcus"] < r for c, (*_, r) in zip(cnt, CASES))
    assert any(c["intervals"] > 9 for c in cnt)          # more than 8 markers: RST7 is followed by RST0
    assert any(c["intervals"] == 1 for c in cnt)         # restart above the MCU count: no marker at all


def test_assemble_equals_the_restatements_framing():
    from vspbfr_amd import jpeg
    seg = bytes(range(256)) * 3
    for quality in (1, 25, 49, 50, 90, 100):
        for sub in ("420", "444"):
            for restart in (1, 8, 300, 65535):
                assert jpeg.assemble(seg, 37, 1100, quality, sub, restart) == R.frame(seg, 37, 1100, quality, R.SUB[sub], restart)
    head = jpeg.assemble(b"", 5, 7)
    lengths, at = [], 2
    while at < len(head) - 2:
        n = int.from_bytes(head[at + 2:at + 4], "big")
        lengths.append(n)
        at += 2 + n
    assert lengths == [16, 67, 67, 17, 31, 181, 31, 181, 4, 12]
    for bad in (dict(quality=0), dict(quality=101), dict(subsampling="422"), dict(restart=0), dict(restart=65536)):
        with pytest.raises(ValueError):
            jpeg.assemble(b"", 5, 7, **bad)


def _valid():
    """arguments the entry accepts up to its launches: one 20 x 30 image, dummy non-null pointers that the checks never dereference"""
    from vspbfr_amd import _lib
    sub, restart = 2, 8
    items = (_lib.JpegItem * 1)(_lib.JpegItem(0, 0, 20, 30, 0, 0))
    bound = _lib.lib.vsp_jpeg_image_bound(20, 30, restart, sub)
    work = _lib.lib.vsp_jpeg_intervals(20, 30, restart, sub) * _lib.lib.vsp_jpeg_interval_bound(4, sub)
    p = C.c_void_p(4096)
    return dict(out=p, out_bytes=bound, totals=p, work=p, work_bytes=work, ws=p, src=p, src_bytes=20 * 30 * 3, items=items, items_dev=p, n=1,
                quality=90, sub=sub, restart=restart)


def _call(a):
    from vspbfr_amd import _lib
    items = a["items"]
    rc = _lib.lib.vsp_jpeg_encode_u8(a["out"], a["out_bytes"], a["totals"], a["work"], a["work_bytes"], a["ws"], a["src"], a["src_bytes"],
                                     None if items is None else C.cast(items, C.c_void_p), a["items_dev"], a["n"], a["quality"], a["sub"],
                                     a["restart"], None)
    return rc, _lib.last_error()


def _item(**kw):
    from vspbfr_amd import _lib
    f = dict(src_off=0, out_off=0, h=20, w=30, interval0=0, pad_=0)
    f.update(kw)
    return (_lib.JpegItem * 1)(_lib.JpegItem(*(f[k] for k in ("src_off", "out_off", "h", "w", "interval0", "pad_"))))


REFUSALS = [
    (dict(out=None), -1, "null pointer"), (dict(totals=None), -1, "null pointer"), (dict(work=None), -1, "null pointer"),
    (dict(ws=None), -1, "null pointer"), (dict(src=None), -1, "null pointer"), (dict(items=None), -1, "null pointer"),
    (dict(items_dev=None), -1, "null pointer"),
    (dict(quality=0), -1, "quality"), (dict(quality=101), -1, "quality"),
    (dict(sub=1), -1, "subsampling"), (dict(sub=3), -1, "subsampling"),
    (dict(restart=0), -1, "restart"), (dict(restart=65536), -1, "restart"),
    (dict(n=-1), -1, "items"), (dict(n=65536), -1, "items"),
    (dict(items=lambda: _item(h=0)), -1, "1..65535"), (dict(items=lambda: _item(w=65536)), -1, "1..65535"),
    (dict(items=lambda: _item(src_off=1)), -1, "outside src"), (dict(items=lambda: _item(src_off=-1)), -1, "outside src"),
    (dict(src_bytes=20 * 30 * 3 - 1), -1, "outside src"),
    (dict(items=lambda: _item(out_off=1)), -1, "outside out"), (dict(out_bytes=100), -1, "outside out"),
    (dict(items=lambda: _item(interval0=1)), -1, "interval0"),
    (dict(work_bytes=100), -1, "work"),
    (dict(src_bytes=1 << 31), -3, "2 GiB"), (dict(out_bytes=1 << 31), -3, "2 GiB"), (dict(work_bytes=1 << 31), -3, "2 GiB"),
]


@pytest.mark.parametrize("change,code,fragment", REFUSALS, ids=lambda v: str(v) if not isinstance(v, dict) else ",".join(v))
def test_the_entry_refuses_on_the_host(change, code, fragment):
    a = _valid()
    a.update({k: (v() if callable(v) else v) for k, v in change.items()})
    rc, msg = _call(a)
    assert rc == code and msg.startswith("jpeg_encode:") and fragment in msg, (rc, msg)


def test_bounds_and_an_empty_call():
    from vspbfr_amd import _lib
    lib = _lib.lib
    a = _valid()
    a.update(n=0, out=None, items=None)
    assert _call(a)[0] == 0
    assert lib.vsp_jpeg_intervals(20, 30, 8, 2) == 1 and lib.vsp_jpeg_intervals(20, 30, 1, 0) == 12 and lib.vsp_jpeg_intervals(20, 30, 8, 1) == 0
    assert lib.vsp_jpeg_intervals(0, 30, 8, 2) == 0 and lib.vsp_jpeg_intervals(20, 65536, 8, 2) == 0 and lib.vsp_jpeg_intervals(20, 30, 0, 2) == 0
    assert lib.vsp_jpeg_interval_bound(8, 2) == 8 * 6 * 416 + 4 and lib.vsp_jpeg_interval_bound(1, 0) == 3 * 416 + 4
    assert lib.vsp_jpeg_interval_bound(0, 2) == 0 and lib.vsp_jpeg_image_bound(20, 30, 8, 5) == 0
    # no interval of the case list comes near its slot: the bound is (22 + 63 x 26) bits per block with every byte stuffed
    for case in CASES:
        kind, h, w, quality, sub, restart = case
        m = 16 if sub == "420" else 8
        mcus = -(-h // m) * -(-w // m)
        enc = _encoded(case)
        assert max(len(p) for p in enc["pieces"]) <= lib.vsp_jpeg_interval_bound(min(restart, mcus), R.SUB[sub])
        assert len(enc["segment"]) <= lib.vsp_jpeg_image_bound(h, w, restart, R.SUB[sub])


def test_kernel_serves_and_parameters():
    from vspbfr_amd import jpeg
    assert jpeg.kernel_serves([(1024, 1536)] * 8) and jpeg.kernel_serves([(1, 1)], "444", 1)
    assert not jpeg.kernel_serves([(70000, 3)]) and not jpeg.kernel_serves([])
    assert not jpeg.kernel_serves([(20000, 20000)] * 2)            # 2.4 GB of pixels
    assert jpeg.check_params("90", "444", 3) == (90, "444", 3)
    assert np.array_equal(np.array(jpeg.quant_table(37, 1)), R.quant_table(37, 1))
