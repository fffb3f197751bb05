"""The device JPEG decoder (csrc/jpeg_decode.hip, vspbfr_amd/jpeg.py) against Pillow itself, live, and against the NumPy restatement
(tests/jpeg_dec_ref.py): equal pixels, equal round counts, equal status words.  Every comparison is byte equality.  The files are
jpeg_dec_ref.thinned_cases(), written by Pillow at test time; the largest is 260 x 200."""
import ctypes as C

import numpy as np
import pytest
import torch

import jpeg_dec_ref as D

pytestmark = pytest.mark.gpu

CASES = D.thinned_cases()
DEV = "cuda"


def _ids(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


def _unpack(packed, sizes, offsets):
    host = packed.cpu().numpy()
    return [host[o:o + 3 * h * w].reshape(h, w, 3) for (h, w), o in zip(sizes, offsets)]


@pytest.mark.parametrize("case", CASES, ids=_ids)
def test_decode_equals_pillow(case):
    from vspbfr_amd import jpeg
    data = D.make_file(*case)
    packed, sizes, offsets, how = jpeg.decode_batch([data], DEV)
    ref = D.pillow_pixels(data)
    assert how == ["device"] and sizes == [ref.shape[:2]] and offsets == [0]
    got = _unpack(packed, sizes, offsets)[0]
    print(f"{case}: {len(data)} bytes, {int((got != ref).sum())} differing bytes")
    assert np.array_equal(got, ref)


@pytest.mark.parametrize("sub_bytes", [4, 16])
def test_pixels_and_rounds_equal_the_restatement(sub_bytes):
    from vspbfr_amd import jpeg
    datas = [D.make_file(*c) for c in CASES]
    packed, sizes, offsets, how, rounds = jpeg.decode_batch(datas, DEV, sub_bytes=sub_bytes, want_rounds=True)
    assert how == ["device"] * len(datas)
    want = [D.decode(d, sub_bytes) for d in datas]
    print(f"sub_bytes {sub_bytes}: rounds {rounds}, restatement {[r['rounds'] for r in want]}")
    for got, ref in zip(_unpack(packed, sizes, offsets), want):
        assert np.array_equal(got, ref["pixels"])
    assert rounds == [r["rounds"] for r in want]
    assert max(rounds) >= 3


RAGGED = [CASES[i] for i in (2, 4, 6, 12, 24, 27)]


def test_ragged_batch_equals_one_by_one():
    from vspbfr_amd import jpeg
    datas = [D.make_file(*c) for c in RAGGED]
    packed, sizes, offsets, how = jpeg.decode_batch(datas, DEV)
    assert how == ["device"] * 6 and len({s for s in sizes}) > 3
    for d, got in zip(datas, _unpack(packed, sizes, offsets)):
        alone = jpeg.decode_batch([d], DEV)
        assert np.array_equal(got, _unpack(*alone[:3])[0]) and np.array_equal(got, D.pillow_pixels(d))


def test_position_in_the_batch_does_not_matter():
    from vspbfr_amd import jpeg
    datas = [D.make_file(*c) for c in RAGGED]
    order = [3, 5, 0, 2, 4, 1]
    a = _unpack(*jpeg.decode_batch(datas, DEV)[:3])
    b = _unpack(*jpeg.decode_batch([datas[i] for i in order], DEV)[:3])
    for k, i in enumerate(order):
        assert np.array_equal(b[k], a[i])


def _direct(datas, hdrs, guard=0, sub_bytes=16):
    """hip_ops.jpeg_decode over (file, header) pairs, `guard` bytes of 0xA5 before, between and behind the images"""
    from vspbfr_amd import hip_ops
    scans = [d[h["off"]:] for d, h in zip(datas, hdrs)]
    comp = torch.from_numpy(np.frombuffer(b"".join(scans), dtype=np.uint8).copy()).to(DEV)
    specs, tables, offs, at, o = [], [], [], 0, guard
    for s, h in zip(scans, hdrs):
        specs.append((at, len(s), h["h"], h["w"], h["sub"], h["restart"]))
        t = np.zeros(hip_ops.JPEG_DEC_TABLE_BYTES, dtype=np.uint8)
        t[:192] = h["qt"].reshape(-1)
        for k in range(3):
            for j, (bits, vals) in enumerate((h["dc"][k], h["ac"][k])):
                p = 192 + (2 * k + j) * 272
                t[p:p + 16], t[p + 16:p + 16 + len(vals)] = bits, vals
        tables.append(t)
        offs.append(o)
        at, o = at + len(s), o + 3 * h["h"] * h["w"] + guard
    out = torch.full((o,), 0xA5, dtype=torch.uint8, device=DEV)
    _, status, rounds, _ = hip_ops.jpeg_decode(comp, specs, np.concatenate(tables), sub_bytes, out=out, out_offsets=offs, want_rounds=True)
    return out.cpu().numpy(), offs, status.cpu().numpy().tolist(), rounds.cpu().numpy().tolist()


def test_guard_bytes_are_left_alone_and_two_calls_agree():
    datas = [D.make_file(*c) for c in RAGGED]
    hdrs = [D.parse(d) for d in datas]
    out, offs, status, _ = _direct(datas, hdrs, guard=64)
    again = _direct(datas, hdrs, guard=64)[0]
    assert status == [0] * 6 and np.array_equal(out, again)
    mask = np.ones(out.size, dtype=bool)
    for d, h, o in zip(datas, hdrs, offs):
        n = 3 * h["h"] * h["w"]
        assert np.array_equal(out[o:o + n].reshape(h["h"], h["w"], 3), D.pillow_pixels(d))
        mask[o:o + n] = False
    assert mask.sum() == 64 * 7 and (out[mask] == 0xA5).all()


def test_corrupt_scans_report_and_leave_the_others_intact():
    good = [D.make_file(*RAGGED[0]), D.make_file(*RAGGED[3])]
    bad = D.corrupt_files()
    datas = [good[0]] + [d for _, d in bad] + [good[1]]
    hdrs = [D.parse(good[0])] + [D.corrupt_header()] * len(bad) + [D.parse(good[1])]
    out, offs, status, _ = _direct(datas, hdrs, guard=16)
    want = []
    for d, h in zip(datas, hdrs):
        coef, st, _, _ = D.decode_coefficients(d, h, 16)
        want.append(st | D.pixels(coef, h)[1])
    print("status", status, "restatement", want)
    assert status == want and status[0] == 0 and status[-1] == 0 and all(status[1:-1])
    for i in (0, -1):
        h = hdrs[i]
        assert np.array_equal(out[offs[i]:offs[i] + 3 * h["h"] * h["w"]].reshape(h["h"], h["w"], 3), D.pillow_pixels(datas[i]))


def test_decode_batch_hands_flagged_files_to_pillow():
    from vspbfr_amd import jpeg
    good = D.make_file(*RAGGED[0])
    for name, data in D.corrupt_files():
        try:
            ref = D.pillow_pixels(data)
        except Exception as e:                       # the truncated file: Pillow's exception is the caller's
            with pytest.raises(type(e)):
                jpeg.decode_batch([good, data], DEV)
            print(name, "raises", type(e).__name__)
            continue
        packed, sizes, offsets, how = jpeg.decode_batch([good, data, good], DEV)
        got = _unpack(packed, sizes, offsets)
        print(name, how)
        assert how == ["device", "host", "device"]
        assert np.array_equal(got[1], ref) and np.array_equal(got[0], D.pillow_pixels(good)) and np.array_equal(got[2], got[0])
    mixed, raising = [good], []
    for _, d, _ in D.refused_files():
        try:
            D.pillow_pixels(d)
            mixed.append(d)
        except Exception as e:                       # the two-scan file: libjpeg refuses the second scan
            raising.append((d, type(e)))
    packed, sizes, offsets, how = jpeg.decode_batch(mixed, DEV)
    assert len(mixed) >= 6 and how == ["device"] + ["host"] * (len(mixed) - 1)
    for d, got in zip(mixed, _unpack(packed, sizes, offsets)):
        assert np.array_equal(got, D.pillow_pixels(d))
    for d, exc in raising:
        with pytest.raises(exc):
            jpeg.decode_batch([good, d], DEV)


def test_entry_refusals_launch_nothing():
    from vspbfr_amd import _lib
    lib = _lib.lib
    data = D.make_file(*RAGGED[0])
    hdr = D.parse(data)
    scan = data[hdr["off"]:]
    sub_bytes = 16
    need = lib.vsp_jpeg_decode_work_bytes(hdr["h"], hdr["w"], len(scan), hdr["sub"], hdr["restart"], sub_bytes)
    assert need > 0 and need % 16 == 0
    assert lib.vsp_jpeg_decode_work_bytes(hdr["h"], hdr["w"], len(scan), hdr["sub"], hdr["restart"], 6) == 0
    assert lib.vsp_jpeg_decode_work_bytes(0, hdr["w"], len(scan), hdr["sub"], hdr["restart"], sub_bytes) == 0
    npix = 3 * hdr["h"] * hdr["w"]
    tab = np.zeros(1824, dtype=np.uint8)
    tab[:192] = hdr["qt"].reshape(-1)
    for k in range(3):
        for j, (bits, vals) in enumerate((hdr["dc"][k], hdr["ac"][k])):
            p = 192 + (2 * k + j) * 272
            tab[p:p + 16], tab[p + 16:p + 16 + len(vals)] = bits, vals
    comp = torch.from_numpy(np.frombuffer(scan, dtype=np.uint8).copy()).to(DEV)
    out = torch.full((npix,), 0xA5, dtype=torch.uint8, device=DEV)
    status = torch.full((1,), -7, dtype=torch.int32, device=DEV)
    work = torch.empty(need, dtype=torch.uint8, device=DEV)

    def call(item=None, tables=None, n=1, sb=sub_bytes, null=None, out_bytes=npix, work_bytes=need, in_bytes=len(scan)):
        it = _lib.JpegDecItem(0, 0, 0, len(scan), hdr["h"], hdr["w"], hdr["sub"], hdr["restart"], 0)
        for k, v in (item or {}).items():
            setattr(it, k, v)
        t = tab if tables is None else tables
        items_dev = torch.from_numpy(np.frombuffer(bytes(it), dtype=np.uint8).copy()).to(DEV)
        t_dev = torch.from_numpy(t).to(DEV)
        args = dict(out=out.data_ptr(), status=status.data_ptr(), work=work.data_ptr(), comp=comp.data_ptr(), items=C.addressof(it),
                    items_dev=items_dev.data_ptr(), tables=t.ctypes.data, tables_dev=t_dev.data_ptr())
        if null:
            args[null] = None
        return lib.vsp_jpeg_decode_u8(args["out"], out_bytes, args["status"], None, args["work"], work_bytes, args["comp"], in_bytes, args["items"],
                                      args["items_dev"], args["tables"], args["tables_dev"], n, sb, None)

    EINVAL, ENOTSUP = -1, -3
    overfull, many, full = tab.copy(), tab.copy(), tab.copy()
    overfull[192] = 3                                # three codes of one bit
    full[192:192 + 16] = 0
    full[192] = 2                                    # 0 and 1: the all-ones code is in use
    many[192:192 + 16] = 0
    many[192 + 8:192 + 16] = 40                      # 320 codes
    refusals = [(dict(null="out"), EINVAL), (dict(null="status"), EINVAL), (dict(null="work"), EINVAL), (dict(null="comp"), EINVAL),
                (dict(null="items"), EINVAL), (dict(null="items_dev"), EINVAL), (dict(null="tables"), EINVAL), (dict(null="tables_dev"), EINVAL),
                (dict(n=-1), EINVAL), (dict(n=65536), EINVAL), (dict(item=dict(h=0)), EINVAL), (dict(item=dict(w=65536)), EINVAL),
                (dict(item=dict(in_off=1)), EINVAL), (dict(item=dict(in_len=len(scan) + 1)), EINVAL), (dict(item=dict(out_off=1)), EINVAL),
                (dict(item=dict(out_off=-1)), EINVAL), (dict(item=dict(subsampling=1)), EINVAL), (dict(item=dict(restart=-1)), EINVAL),
                (dict(item=dict(interval0=1)), EINVAL), (dict(item=dict(work_off=16)), EINVAL), (dict(sb=0), EINVAL), (dict(sb=6), EINVAL),
                (dict(sb=2), EINVAL), (dict(tables=overfull), EINVAL), (dict(tables=many), EINVAL), (dict(tables=full), EINVAL), (dict(work_bytes=need - 16), EINVAL),
                (dict(out_bytes=1 << 31), ENOTSUP), (dict(work_bytes=1 << 31), ENOTSUP), (dict(in_bytes=1 << 31), ENOTSUP)]
    for kw, rc in refusals:
        assert call(**kw) == rc, kw
        assert _lib.last_error()
    assert call(n=0) == 0
    # two items whose images overlap in out: the second starts inside the first
    two = (_lib.JpegDecItem * 2)(_lib.JpegDecItem(0, 0, 0, len(scan), hdr["h"], hdr["w"], hdr["sub"], hdr["restart"], 0),
                                 _lib.JpegDecItem(0, npix - 3, need, len(scan), hdr["h"], hdr["w"], hdr["sub"], hdr["restart"], 1))
    tab2 = np.concatenate([tab, tab])
    tab2_dev, work2, out2 = torch.from_numpy(tab2).to(DEV), torch.empty(2 * need, dtype=torch.uint8, device=DEV), torch.empty(2 * npix, dtype=torch.uint8, device=DEV)
    status2 = torch.full((2,), -7, dtype=torch.int32, device=DEV)

    def call2():                                     # the device copy of the items is made from the host table as it stands
        two_dev = torch.from_numpy(np.frombuffer(bytes(two), dtype=np.uint8).copy()).to(DEV)
        return lib.vsp_jpeg_decode_u8(out2.data_ptr(), 2 * npix, status2.data_ptr(), None, work2.data_ptr(), 2 * need, comp.data_ptr(), len(scan),
                                      C.addressof(two), two_dev.data_ptr(), tab2.ctypes.data, tab2_dev.data_ptr(), 2, sub_bytes, None)
    assert call2() == EINVAL and "overlaps" in _lib.last_error()
    two[1].out_off = npix
    assert call2() == 0
    torch.cuda.synchronize()
    assert status2.cpu().tolist() == [0, 0] and np.array_equal(out2[:npix].cpu().numpy(), out2[npix:].cpu().numpy())
    torch.cuda.synchronize()
    assert (out.cpu().numpy() == 0xA5).all() and int(status.cpu()[0]) == -7      # nothing was launched
    assert call() == 0
    torch.cuda.synchronize()
    assert int(status.cpu()[0]) == 0 and np.array_equal(out.cpu().numpy().reshape(hdr["h"], hdr["w"], 3), D.pillow_pixels(data))
    from vspbfr_amd import hip_ops
    with pytest.raises(RuntimeError):
        hip_ops.jpeg_decode(comp, [(0, len(scan), hdr["h"], hdr["w"], hdr["sub"], hdr["restart"])], tab, sub_bytes=6)
    with pytest.raises(RuntimeError):
        hip_ops.jpeg_decode(comp, [(0, len(scan), 0, hdr["w"], hdr["sub"], hdr["restart"])], tab)
