"""The NumPy restatement of the device JPEG decoder (tests/jpeg_dec_ref.py) against Pillow itself: equal pixels for every case, for a
committed photo and for a file whose padding blocks hold noise; the emulated subsequence / round scheme against the serial decoder; the
coverage the case list is meant to reach; the parser's refusals; corrupt scans.  No GPU."""
import numpy as np
import pytest

import jpeg_dec_ref as D

CASES = D.thinned_cases()
SUBS = (4, 16, 128)


@pytest.mark.parametrize("case", CASES, ids=lambda v: "-".join(str(x) for x in v))
def test_restatement_equals_pillow(case):
    data = D.make_file(*case)
    got = D.decode(data)
    assert got["status"] == 0
    assert np.array_equal(got["pixels"], D.pillow_pixels(data))


def test_committed_photo():
    import os
    with open(os.path.join(os.path.dirname(__file__), "golden", "loader_images", "lq", "c_photo.jpg"), "rb") as f:
        data = f.read()
    got = D.decode(data)
    assert got["status"] == 0 and np.array_equal(got["pixels"], D.pillow_pixels(data))


def test_padding_blocks_that_hold_noise():
    data = D.noisy_padding_file()
    hdr = D.parse(data)
    assert (hdr["h"], hdr["w"], hdr["sub"]) == (33, 17, 2)
    got = D.decode(data)
    assert got["status"] == 0 and np.array_equal(got["pixels"], D.pillow_pixels(data))
    # the padding is not a replica of the edge: the decoded padded planes differ from the edge right of and below the image
    g = D.geometry(33, 17, 2, 0)
    c = got["coef"].reshape(g["mcus"], 6, 64).copy()
    for k, idx in enumerate(([0, 1, 2, 3], [4], [5])):
        c[:, idx, 0] = np.cumsum(c[:, idx, 0].reshape(-1)).reshape(g["mcus"], len(idx))
    comp = np.array([0, 0, 0, 0, 1, 2])
    b = D._idct_pass(D._idct_pass((c * hdr["qt"][comp][None]).reshape(-1, 6, 8, 8).swapaxes(-1, -2), False).swapaxes(-1, -2), True)
    b = b.reshape(g["mh"], g["mw"], 6, 8, 8)
    cb = b[:, :, 4].transpose(0, 2, 1, 3).reshape(g["mh"] * 8, g["mw"] * 8)
    ch, cw = 17, 9
    assert (cb[:ch, cw:] != cb[:ch, cw - 1:cw]).any() and (cb[ch:, :cw] != cb[ch - 1:ch, :cw]).any()


@pytest.mark.parametrize("sub_bytes", SUBS)
def test_parallel_scheme_gives_the_serial_coefficients(sub_bytes):
    for case in CASES:
        data = D.make_file(*case)
        serial, parallel = D.decode(data), D.decode(data, sub_bytes)
        assert parallel["status"] == 0 and np.array_equal(parallel["coef"], serial["coef"]), case
        assert parallel["rounds"] >= 1


def test_case_list_reaches_the_hard_places():
    tot = dict(straddle=0, block_spans3=0, max_blocks_in_sub=0, wrong_round0=0, max_rounds=0, ff_last_byte=0, zrl=0, dc_cat=0, ac_cat=0,
               code16=0, max_subs=0)
    wraps = short = False
    for case in CASES:
        data = D.make_file(*case)
        for sb in SUBS:
            st = D.decode(data, sb)["stats"]
            for k in tot:
                tot[k] = max(tot[k], st[k]) if k.startswith("max_") or k.endswith("_cat") else tot[k] + st[k]
        restart = D.parse(data)["restart"]
        wraps |= st["intervals"] > 9
        short |= restart > 0 and st["intervals"] > 1 and st["last_interval_mcus"] < restart
    print(tot, wraps, short)
    assert tot["straddle"] > 0, "a symbol straddling a subsequence boundary"
    assert tot["block_spans3"] > 0, "a block spanning three or more subsequences"
    assert tot["max_blocks_in_sub"] > 16, "a subsequence holding more than 16 whole blocks"
    assert tot["wrong_round0"] > 0, "a subsequence whose round-0 exit differs from the truth"
    assert tot["max_rounds"] >= 3, "an interval that needed three or more rounds"
    assert tot["ff_last_byte"] > 0, "a stuffed FF as the last byte of a subsequence"
    assert tot["zrl"] > 0 and tot["code16"] > 0
    assert tot["dc_cat"] == 11 and tot["ac_cat"] == 10
    assert wraps, "RSTm wrapping past 7"
    assert short, "a short last interval"
    big = D.decode(D.make_file("noise", 96, 96, 100, "444", 0, False, False), 16)["stats"]
    assert big["max_subs"] > 1024


@pytest.mark.parametrize("name,data,word", D.refused_files(), ids=lambda v: v if isinstance(v, str) else "")
def test_parse_refuses(name, data, word):
    with pytest.raises(D.Refused, match=word):
        D.parse(data)
    from vspbfr_amd import jpeg
    scan, why = jpeg.parse(data)
    assert scan is None and word in why


def test_parse_accepts_the_rest():
    from vspbfr_amd import jpeg
    for case in CASES:
        data = D.make_file(*case)
        ref = D.parse(data)
        scan, why = jpeg.parse(data)
        assert why is None
        assert (scan.h, scan.w, scan.restart, scan.offset, scan.length) == (ref["h"], ref["w"], ref["restart"], ref["off"], ref["length"])
        assert scan.subsampling == ("420" if ref["sub"] == 2 else "444") and np.array_equal(scan.qt, ref["qt"])
        for k in range(3):
            assert (list(scan.huff[2 * k][0]), list(scan.huff[2 * k][1])) == ref["dc"][k]
            assert (list(scan.huff[2 * k + 1][0]), list(scan.huff[2 * k + 1][1])) == ref["ac"][k]


EXPECTED = {"truncated": D.NO_EOI | D.RST_COUNT | D.BLOCK_COUNT, "stray_marker": D.STRAY_MARKER | D.RST_COUNT | D.BLOCK_COUNT,
            "rst_missing": D.RST_ORDER | D.RST_COUNT | D.BLOCK_COUNT}


@pytest.mark.parametrize("name,data", D.corrupt_files(), ids=lambda v: v if isinstance(v, str) else "")
def test_corrupt_scans_set_the_status(name, data):
    hdr = D.corrupt_header()
    for sb in (None, 4, 16):
        coef, status, _, _ = D.decode_coefficients(data, hdr, sb)
        print(name, sb, status)
        assert status != 0
        if name in EXPECTED:
            assert status & EXPECTED[name] == EXPECTED[name]
        D.pixels(coef, hdr)
    assert D.decode_coefficients(data, hdr, 4)[1] == D.decode_coefficients(data, hdr, 16)[1] == D.decode_coefficients(data, hdr, None)[1]
