"""Which calls the eight convolution entries of csrc/conv_igemm.hip refuse on the host, pinned as a table.

Every argument check ahead of the kernel argument block is pure host code, so the table runs without a GPU: a row changes ONE thing of a call
the entry accepts and names the return code, the message prefix and a fragment of the message.  The pointers are dummies (4096) that no check
dereferences.  A call that passes every host check ends, on a machine without a device, in `-1 conv2d: cannot resolve device constants:
hipGetDevice failed`; those rows (code DEVICE) are the proof that the unchanged call is one the entry accepts.  With a device present they
would go on to launch on the dummy pointers, so they are skipped there -- the refusals themselves run everywhere.

Rules that need a device (the act2 slope, every *_eligible, the tile plans) stay with the GPU tests of tests/test_hip_ops.py and tests/test_wino4f.py.
"""
import ctypes as C

import pytest

ENTRIES = ("f32", "winograd", "winograd4", "winograd4f", "bf16", "bf16x3", "bf16rv", "bf16dg")
SYMBOL = {"f32": "vsp_conv2d_f32", "winograd": "vsp_conv2d_winograd_f32", "winograd4": "vsp_conv2d_winograd4_f32",
          "winograd4f": "vsp_conv2d_winograd4f_f32", "bf16": "vsp_conv2d_bf16", "bf16x3": "vsp_conv2d_bf16x3", "bf16rv": "vsp_conv2d_bf16rv",
          "bf16dg": "vsp_conv2d_bf16dg"}
# the prefix of an entry's own rules (the rules of the shared validator say "conv2d:" whichever entry they are reached through)
OWN = {"f32": "conv2d:", "winograd": "conv2d_winograd:", "winograd4": "conv2d_winograd4:", "winograd4f": "conv2d_winograd4f:",
       "bf16": "conv2d_bf16:", "bf16x3": "conv2d_bf16:", "bf16rv": "conv2d_bf16:", "bf16dg": "conv2d_bf16:"}
BF16 = ("bf16", "bf16x3", "bf16rv", "bf16dg")
P = 4096
DEVICE = "device"          # the call passes every host check: -1 "conv2d: cannot resolve device constants: hipGetDevice failed" without a device
ONES = (1, 1, 1, 1)


def _valid(entry):
    """a call the entry accepts up to the device: 2 x 64 x 32 x 32 -> 64 channels, 3x3, stride 1, padding 1"""
    f = dict(x=P, w=P, y=P, B=2, Cin=64, H=32, W=32, G=1, cout_g=64, OH=32, OW=32, KH=3, KW=3, stride_y=1, stride_x=1, dil=ONES, pad_y=ONES,
             pad_x=ONES, y_ch=64, y_h=32, y_w=32, osy=1, osx=1)
    if entry in ("bf16rv", "bf16dg"):
        f["io_bf16"] = 1
    if entry == "winograd4":
        f.update(work=P, work_floats=None)      # None: what vsp_conv2d_winograd4_work_floats asks for
    return f


def _call(entry, f):
    from vspbfr_amd import _lib
    f = dict(f)
    null_params = f.pop("params", True) is None
    work, work_floats = f.pop("work", None), f.pop("work_floats", None)
    p = _lib.ConvParams()
    for k, v in f.items():
        if k in ("dil", "pad_y", "pad_x"):
            for g in range(4):
                getattr(p, k)[g] = v[g]
        else:
            setattr(p, k, v)
    ref = None if null_params else C.byref(p)
    fn = getattr(_lib.lib, SYMBOL[entry])
    if entry == "winograd4":
        if work_floats is None:
            work_floats = _lib.lib.vsp_conv2d_winograd4_work_floats(C.byref(p))
        rc = fn(ref, work, C.c_size_t(work_floats), None)
    else:
        rc = fn(ref, None)
    return rc, _lib.last_error()


def _rows():
    rows = []

    def add(entries, change, code, prefix, fragment):
        for e in ((entries,) if isinstance(entries, str) else entries):
            rows.append((e, change, code, OWN[e] if prefix == "own" else prefix, fragment))

    # ---- the unchanged call reaches the device
    add(ENTRIES, {}, DEVICE, "conv2d:", "cannot resolve device constants")

    # ---- the shared validator: every rule through vsp_conv2d_f32
    V = "conv2d:"
    for ch in (dict(x=None), dict(w=None), dict(y=None)):
        add("f32", ch, -1, V, "null tensor pointer")
    for ch in (dict(B=-1), dict(Cin=0), dict(H=0), dict(W=0)):
        add("f32", ch, -1, V, "bad input dims")
    for ch in (dict(G=0), dict(G=1025, y_ch=1025 * 64), dict(cout_g=0)):
        add("f32", ch, -1, V, "bad group spec")
    for ch in (dict(x_group_stride=-1), dict(x_ch=-1)):
        add("f32", ch, -1, V, "negative x_ch / x_group_stride")
    add("f32", dict(x_ch=32), -1, V, "group input channels exceed x_ch=32")
    add("f32", dict(G=2, x_group_stride=64, x_ch=127, y_ch=128), -1, V, "group input channels exceed x_ch=127")
    add("f32", dict(G=2, x_group_stride=64, x_ch=128, y_ch=128, in_shift=P), -1, V, "input shift is not supported with grouped input")
    add("f32", dict(G=2, x_group_stride=64, x_ch=128, y_ch=128), DEVICE, V, "cannot resolve device constants")
    for ch in (dict(KH=0), dict(KW=0), dict(KH=8, KW=8), dict(KH=5, KW=10)):
        add("f32", ch, -1, V, "unsupported kernel")
    add("f32", dict(KH=7, KW=7), DEVICE, V, "cannot resolve device constants")
    for ch in (dict(stride_y=0), dict(stride_x=0), dict(stride_y=3), dict(stride_x=3)):
        add("f32", ch, -1, V, "stride must be 1 or 2")
    for ch in (dict(dil_by_input_quarter=2), dict(dil_by_input_quarter=1), dict(dil_by_input_quarter=1, G=4, cout_g=16, Cin=24),
               dict(dil_by_input_quarter=1, G=4, cout_g=16, x_group_stride=64, x_ch=256)):
        add("f32", ch, -1, V, "dil_by_input_quarter needs G = 4")
    for ch in (dict(OH=-1), dict(OW=-1)):
        add("f32", ch, -1, V, "negative output size")
    for ch in (dict(osy=0), dict(osx=0), dict(ooy=-1), dict(oox=-1)):
        add("f32", ch, -1, V, "bad output stride/offset")
    add("f32", dict(noise=P), -1, V, "noise given without noise_w")
    add("f32", dict(act2=2), -1, V, "act2=prelu without slopes")
    for ch in (dict(dil=(0, 1, 1, 1)), dict(G=2, cout_g=32, dil=(1, 0, 1, 1))):
        add("f32", ch, -1, V, "dilation must be >= 1")
    add("f32", dict(y_coff=1), -1, V, "output channel window [1,65) outside 64")
    add("f32", dict(y_coff=-1), -1, V, "output channel window [-1,63) outside 64")
    add("f32", dict(y_ch=63), -1, V, "output channel window [0,64) outside 63")
    add("f32", dict(y_h=31), -1, V, "output positions exceed the 31x32 output tensor")
    add("f32", dict(y_w=31), -1, V, "output positions exceed the 32x31 output tensor")
    add("f32", dict(ooy=1), -1, V, "output positions exceed")
    add("f32", dict(y_ch=1 << 16, y_h=256, y_w=128), -1, V, "fewer than 2^31 elements")
    add(("winograd4", "winograd4f"), dict(x_ch=1 << 21), -1, V, "fewer than 2^31 elements")     # (the other entries have a 2 GiB rule of their own)
    for ch in (dict(res1=P, res_ch=64, res_coff=1), dict(res2=P, res_ch=63), dict(res1=P, res_ch=64, res_coff=-1)):
        add("f32", ch, -1, V, "residual channel window out of range")
    # ---- ... and the null-pointer, channel-window, output-extent and per-image-weight rules through every other entry
    others = ENTRIES[1:]
    for ch in (dict(x=None), dict(w=None), dict(y=None)):
        add(others, ch, -1, V, "null tensor pointer")
    add(others, dict(y_coff=1), -1, V, "output channel window [1,65) outside 64")
    add(others, dict(y_h=31), -1, V, "output positions exceed the 31x32 output tensor")
    add(others, dict(res1=P, res_ch=64, res_coff=1), -1, V, "residual channel window out of range")
    add(others, dict(noise=P), -1, V, "noise given without noise_w")
    add(others, dict(act2=2), -1, V, "act2=prelu without slopes")
    # per-image weights: only vsp_conv2d_bf16 with bf16 activations takes them
    add(("f32", "winograd", "winograd4", "winograd4f"), dict(w_bstride=16), -1, V, "per-image weights (w_bstride)")
    add(("bf16x3", "bf16rv", "bf16dg"), dict(w_bstride=16), -1, "own", "per-image weights need the general bf16 kernel")
    add(("bf16x3", "bf16rv", "bf16dg"), dict(w_bstride=16, io_bf16=1), -1, "own", "per-image weights need the general bf16 kernel")
    add("bf16", dict(w_bstride=16), -1, "own", "per-image weights need the general bf16 kernel with bf16 activations")
    add("bf16", dict(w_bstride=16, io_bf16=1), DEVICE, V, "cannot resolve device constants")
    for ch in (dict(w_bstride=8, io_bf16=1), dict(w_bstride=-16, io_bf16=1)):
        add("bf16", ch, -1, "own", "w_bstride must be a positive multiple of 16 bytes")
    for ch in (dict(w_bstride=16, io_bf16=1, in_scale=P), dict(w_bstride=16, io_bf16=1, in_shift=P)):
        add("bf16", ch, -1, "own", "in_scale / in_shift must be NULL")
    for ch in (dict(w_bstride=16, io_bf16=1, W=30, OW=30, y_w=30, x=P + 2), dict(w_bstride=16, io_bf16=1, W=31, OW=31, y_w=31)):
        add("bf16", ch, -1, "own", "per-image weights need even rows")
    # ---- the empty call is served (nothing to do) by every entry: checked in test_an_empty_call_is_served

    # ---- vsp_conv2d_f32's own rules
    add(ENTRIES, dict(params=None), -1, "own", "null params")
    add("f32", dict(io_bf16=1), -1, "own", "fp32 activations only")
    for ch in (dict(transposed=1, y_h=65, y_w=65), dict(transposed=1, y_h=66, y_w=66)):       # (one row / column wider is allowed here)
        add("f32", ch, DEVICE, V, "cannot resolve device constants")
    for ch in (dict(G=2, y_ch=128), dict(KH=1, KW=1), dict(KH=5)):
        add("f32", dict(transposed=1, y_h=65, y_w=65, **ch), -1, "own", "transposed mode needs a 3x3 kernel and G = 1")
    for ch in (dict(noise=P, noise_w=P), dict(res1=P, res_ch=64), dict(res2=P, res_ch=64)):
        add("f32", dict(transposed=1, y_h=65, y_w=65, **ch), -1, "own", "transposed mode has no noise / residual epilogue")
    for ch in (dict(y_h=64, y_w=65), dict(y_h=65, y_w=64)):
        add("f32", dict(transposed=1, **ch), -1, "own", "(2H+1)x(2W+1)")
    add("f32", dict(x_ch=1 << 19), -1, "own", "smaller than 2 GiB")
    add("f32", dict(Cin=1 << 15, cout_g=1 << 11, y_ch=1 << 11, H=8, W=8, OH=8, OW=8, y_h=8, y_w=8), -1, "own", "smaller than 2 GiB")

    # ---- vsp_conv2d_winograd_f32
    for ch in (dict(transposed=1), dict(G=5, cout_g=8, y_ch=40), dict(G=0), dict(KH=1), dict(KW=5), dict(stride_y=2), dict(stride_x=2),
               dict(G=2, x_group_stride=64, x_ch=128, y_ch=128)):
        add("winograd", ch, -1, "own", "3x3, stride 1, at most four groups over one shared input")
    add("winograd", dict(G=4, cout_g=16, dil=(1, 2, 4, 8), pad_y=(1, 2, 4, 8), pad_x=(1, 2, 4, 8)), DEVICE, V, "cannot resolve device constants")
    for ch in (dict(dil=(3, 1, 1, 1), pad_y=(3, 1, 1, 1), pad_x=(3, 1, 1, 1)), dict(dil=(16, 1, 1, 1), pad_y=(16, 1, 1, 1), pad_x=(16, 1, 1, 1)),
               dict(pad_y=(0, 1, 1, 1)), dict(pad_x=(2, 1, 1, 1)), dict(G=2, cout_g=32, pad_x=(1, 0, 1, 1))):
        add("winograd", ch, -1, "own", "padding = dilation")
    add("winograd", dict(io_bf16=1), -1, "own", "fp32 activations only")
    add("winograd", dict(dil_by_input_quarter=1), -1, "own", "dil_by_input_quarter is served by vsp_conv2d_f32")
    for ch in (dict(osy=2), dict(osx=2), dict(ooy=1), dict(oox=1)):
        add("winograd", ch, -1, "own", "dense")
    for ch in (dict(OH=31), dict(OW=31)):
        add("winograd", ch, -1, "own", "output size must equal the input size")
    add("winograd", dict(w=P + 4), -1, "own", "weights must be 16-byte aligned")
    add("winograd", dict(Cin=1 << 14, cout_g=1 << 13, y_ch=1 << 13, H=4, W=4, OH=4, OW=4, y_h=4, y_w=4), -1, "own", "weight tensor too large")
    add("winograd", dict(x_ch=1 << 19), -1, "own", "smaller than 2 GiB")

    # ---- vsp_conv2d_winograd4_f32
    add("winograd4", dict(work=None), -1, "own", "null params / work buffer")
    for ch in (dict(transposed=1), dict(G=2, cout_g=32), dict(KH=1), dict(KW=1), dict(stride_y=2), dict(stride_x=2), dict(dil=(2, 1, 1, 1)),
               dict(pad_y=(0, 1, 1, 1)), dict(pad_x=(2, 1, 1, 1))):
        add("winograd4", ch, -1, "own", "one group, 3x3, stride 1, dilation 1, padding 1")
    for ch in (dict(io_bf16=1), dict(dil_by_input_quarter=1), dict(in_shift=P)):
        add("winograd4", ch, -1, "own", "fp32, no affine input shift")
    for ch in (dict(osy=2), dict(osx=2), dict(ooy=1), dict(oox=1), dict(OH=31), dict(OW=31)):
        add("winograd4", ch, -1, "own", "dense same-size output")
    for ch in (dict(w=P + 4), dict(work=P + 4)):
        add("winograd4", ch, -1, "own", "16-byte aligned")
    add("winograd4", dict(work_floats=2 * 2 * 16 * 12 * 64 * 6 - 1), -1, "own", "work buffer too small")
    add("winograd4", dict(work_floats=2 * 2 * 16 * 12 * 64 * 6), DEVICE, V, "cannot resolve device constants")
    add("winograd4", dict(Cin=256, H=32768, W=32768, OH=32768, OW=32768, y_h=32768, y_w=32768, work_floats=1 << 62), -1, "own", "image too large")

    # ---- vsp_conv2d_winograd4f_f32
    for ch in (dict(transposed=1), dict(G=5, cout_g=8, y_ch=40), dict(G=0), dict(KH=1), dict(KW=1), dict(stride_y=2), dict(stride_x=2)):
        add("winograd4f", ch, -1, "own", "3x3, stride 1, one group or up to four dilation groups over one shared input")
    add("winograd4f", dict(G=4, cout_g=16, dil=(1, 2, 4, 8), pad_y=(1, 2, 4, 8), pad_x=(1, 2, 4, 8)), DEVICE, V, "cannot resolve device constants")
    for ch in (dict(dil=(3, 1, 1, 1), pad_y=(3, 1, 1, 1), pad_x=(3, 1, 1, 1)), dict(dil=(16, 1, 1, 1), pad_y=(16, 1, 1, 1), pad_x=(16, 1, 1, 1)),
               dict(pad_y=(0, 1, 1, 1)), dict(pad_x=(2, 1, 1, 1)), dict(G=2, cout_g=32, pad_y=(1, 0, 1, 1))):
        add("winograd4f", ch, -1, "own", "padding = dilation")
    for ch in (dict(io_bf16=1), dict(dil_by_input_quarter=1), dict(in_shift=P)):
        add("winograd4f", ch, -1, "own", "fp32, no affine input shift")
    for ch in (dict(osy=2), dict(osx=2), dict(ooy=1), dict(oox=1), dict(OH=31), dict(OW=31)):
        add("winograd4f", ch, -1, "own", "dense same-size output")
    add("winograd4f", dict(w=P + 4), -1, "own", "weights must be 16-byte aligned")

    # ---- the four bf16 entries (one implementation): stride 1, stride 2 and -- except for the two special kernels' eligibility -- transposed
    for ch in (dict(KH=1), dict(KW=5), dict(G=0)):
        add(BF16, ch, -1, "own", "3x3")
    T = dict(transposed=1, y_h=65, y_w=65)
    add(BF16, T, DEVICE, V, "cannot resolve device constants")
    add(BF16, dict(T, G=2, y_ch=128), -1, "own", "G = 1")
    for ch in (dict(noise=P, noise_w=P), dict(res1=P, res_ch=64), dict(res2=P, res_ch=64)):
        add(BF16, dict(T, **ch), -1, "own", "transposed mode has no noise / residual epilogue")
    for ch in (dict(y_h=64), dict(y_w=64), dict(y_h=66, y_w=66)):                               # (exactly (2H+1) x (2W+1) here)
        add(BF16, dict(T, **ch), -1, "own", "(2H+1)x(2W+1)")
    S2 = dict(stride_y=2, stride_x=2, OH=16, OW=16)
    add(BF16, S2, DEVICE, V, "cannot resolve device constants")
    add(BF16, dict(S2, pad_y=(0, 1, 1, 1), pad_x=(0, 1, 1, 1), OH=15, OW=15), DEVICE, V, "cannot resolve device constants")
    for ch in (dict(dil=(2, 1, 1, 1)), dict(pad_y=(2, 1, 1, 1), pad_x=(2, 1, 1, 1)), dict(pad_y=(0, 1, 1, 1))):
        add(BF16, dict(S2, **ch), -1, "own", "stride 2 needs dilation 1 and padding 0 or 1")
    add(BF16, dict(S2, G=2, y_ch=128), -1, "own", "stride-2 groups need their own input slices")
    for ch in (dict(OH=17), dict(OW=17), dict(pad_y=(0, 1, 1, 1), pad_x=(0, 1, 1, 1))):
        add(BF16, dict(S2, **ch), -1, "own", "output larger than the stride-2 convolution of the input")
    for ch in (dict(stride_x=2), dict(stride_y=2), dict(stride_y=3, stride_x=3)):
        add(BF16, ch, -1, "own", "stride must be 1 or 2")
    add(BF16, dict(G=5, cout_g=8, y_ch=40), -1, "own", "more than four groups need their own input slices")
    for ch in (dict(pad_y=(0, 1, 1, 1)), dict(pad_x=(2, 1, 1, 1)), dict(dil=(65, 1, 1, 1), pad_y=(65, 1, 1, 1), pad_x=(65, 1, 1, 1)),
               dict(dil=(0, 1, 1, 1), pad_y=(0, 1, 1, 1), pad_x=(0, 1, 1, 1)), dict(G=2, cout_g=32, pad_x=(1, 0, 1, 1))):
        add(BF16, ch, -1, "own", "padding = dilation")
    add(BF16, dict(dil=(3, 1, 1, 1), pad_y=(3, 1, 1, 1), pad_x=(3, 1, 1, 1)), DEVICE, V, "cannot resolve device constants")   # (any dilation up to 64 here)
    for ch in (dict(OH=31), dict(OW=31)):
        add(BF16, ch, -1, "own", "output size must equal the input size")
    for ch in (dict(osy=2), dict(osx=2), dict(ooy=1), dict(oox=1), dict(S2, osy=2)):
        add(BF16, ch, -1, "own", "dense")
    add(BF16, dict(w=P + 4), -1, "own", "weights must be 16-byte aligned")
    add(BF16, dict(Cin=12), -1, "own", "multiple of 8")
    add(BF16, dict(x_ch=1 << 19), -1, "own", "smaller than 2 GiB")
    for ch in (dict(cout_g=1 << 16, y_ch=1 << 16), dict(B=1 << 16)):
        add(BF16, ch, -1, "own", "grid too large")
    return rows


ROWS = _rows()


def _id(v):
    return ",".join("%s=%s" % kv for kv in v.items()) or "unchanged" if isinstance(v, dict) else None


@pytest.mark.parametrize("entry,change,code,prefix,fragment", ROWS, ids=lambda v: _id(v) if isinstance(v, dict) else str(v))
def test_the_entry_refuses_on_the_host(entry, change, code, prefix, fragment):
    from vspbfr_amd import _lib
    if code == DEVICE:
        if _lib.lib.vsp_device_count() > 0:
            pytest.skip("a call the entry accepts: with a device it would launch on the dummy pointers")
        code = -1
    f = _valid(entry)
    f.update(change)
    rc, msg = _call(entry, f)
    assert rc == code and msg.startswith(prefix) and fragment in msg, (rc, msg)


EMPTY = [(e, dict(B=0)) for e in ENTRIES] + [("f32", dict(OH=0)), ("f32", dict(OW=0))] + [
    (e, dict(stride_y=2, stride_x=2, OH=0, OW=16)) for e in BF16]


@pytest.mark.parametrize("entry,change", EMPTY, ids=lambda v: _id(v) if isinstance(v, dict) else str(v))
def test_an_empty_call_is_served(entry, change):
    """nothing to do is no error and touches no device (the same-size entries have no empty output without an empty input, a bad dimension)"""
    f = _valid(entry)
    f.update(change)
    assert _call(entry, f)[0] == 0


def test_the_table_covers_what_it_promises():
    by = {}
    for e, ch, code, prefix, frag in ROWS:
        by.setdefault(e, []).append((code, frag))
    for e in ENTRIES:
        frags = [f for _, f in by[e]]
        assert (DEVICE, "cannot resolve device constants") in by[e]
        for need in ("null params", "null tensor pointer", "output channel window", "output positions exceed", "per-image weights"):
            assert any(need in f for f in frags), (e, need)
    assert ("bf16", dict(w_bstride=16, io_bf16=1), DEVICE) in [(e, ch, c) for e, ch, c, _, _ in ROWS]
    assert all(c == -1 for e, ch, c, _, _ in ROWS if e != "bf16" and ch in (dict(w_bstride=16), dict(w_bstride=16, io_bf16=1)))
    assert len(ROWS) == len({(e, tuple(sorted((k, str(v)) for k, v in ch.items()))) for e, ch, *_ in ROWS})
