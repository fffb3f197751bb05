"""CPU checks of hip_ops.conv_route: for a layer in a given configuration, which kernel family runs, with which tile / variant hint and
activation dtype.  Pure host logic on PackedConv(None, ...) geometries rebuilt from the tuned tables' shape keys (no GPU needed)."""
import json
import os

import pytest
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FP32 = {"direct", "tconv", "wino", "wino4", "wino4f"}


@pytest.fixture
def H(monkeypatch):
    from vspbfr_amd import hip_ops
    for name, val in (("BF16_CONV", False), ("ACT_BF16", False), ("BF16_FORCE", 0), ("BF16_DG", True), ("BF16_RV", True)):
        monkeypatch.setattr(hip_ops, name, val)
    for name in ("TUNE", "WINO", "BF16_TUNE", "BF16X3_TUNE"):   # (restored after the test: some assign their own)
        monkeypatch.setattr(hip_ops, name, getattr(hip_ops, name))
    return hip_ops


def table(name):
    return json.load(open(os.path.join(ROOT, "vspbfr_amd", name)))


def layer(H, key):
    """(PackedConv, B, H, W, OH, OW, transposed, in_shift) of a shape key B,Cin,H,W,G,cout_g,kh,kw,stride,dil,OH,OW[,gN][,q][,t][,s]:
    dilation groups are 1 / 2 / 4 / 8 with padding = dilation, a stride-2 3x3 layer has the padding (0 or 1) that gives the key's output."""
    parts = key.split(",")
    B, Cin, Hh, Ww, G, cg, kh, kw, stride, d0, OH, OW = (int(v) for v in parts[:12])
    flags = parts[12:]
    xgs = next((int(f[1:]) for f in flags if f.startswith("g")), 0)
    dil = (1, 2, 4, 8)[:G] if 1 < G <= 4 and not xgs else (d0,)
    pad = ((1,) if (Hh - 1) // 2 + 1 == OH else (0,)) if stride == 2 and kh == 3 else dil
    pc = H.PackedConv(None, G, cg, Cin, kh, kw, stride, dil, pad, x_group_stride=xgs, dil_by_input_quarter="q" in flags)
    return pc, B, Hh, Ww, OH, OW, "t" in flags, "s" in flags


def route(H, key, **kw):
    pc, B, Hh, Ww, OH, OW, transposed, shift = layer(H, key)
    r = H.conv_route(pc, B, Hh, Ww, OH, OW, transposed, in_shift=shift, **kw)
    assert r.key == key
    return r


def test_fp32_table_keys_route_to_their_entry(H):
    """fp32: every key of conv_tune.json runs what its entry names -- a Winograd kernel, or vsp_conv2d_f32 with the entry's tile
    configuration as the preference (negative hint)."""
    seen = set()
    for key, val in table("conv_tune.json").items():
        r = route(H, key)
        assert not r.io_bf16 and not r.named, (key, r)
        if val.startswith("winograd"):
            assert (r.family, r.hint) == ({"winograd": "wino", "winograd4": "wino4", "winograd4f": "wino4f"}[val], 0), (key, val, r)
        else:
            assert val in H.CONFIG_IDS, (key, val)
            assert (r.family, r.hint) == ("tconv" if key.endswith(",t") else "direct", -H.CONFIG_IDS[val]), (key, val, r)
        seen.add(r.family)
    assert seen == FP32


def test_bf16_table_keys_route_to_bf16_with_their_variant(H):
    """BF16_CONV = True with bf16 activations: every key of conv_tune_bf16.json runs a bf16 kernel with bf16 I/O, and the table's
    variant is the hint of vsp_conv2d_bf16 (kept by the automatic row-vector / dilation-group launches for their fall-back)."""
    H.BF16_CONV, H.ACT_BF16 = True, True
    for key, variant in table("conv_tune_bf16.json").items():
        r = route(H, key)
        assert r.family in ("bf16", "bf16rv", "bf16dg") and r.hint == variant and r.io_bf16 and not r.named, (key, r)
        assert route(H, key, x_dtype=torch.bfloat16).family == r.family
        assert route(H, key, out_dtype=torch.float32) == r._replace(family="bf16", io_bf16=False)   # an fp32 `out` keeps fp32 I/O
    assert route(H, "16,64,512,512,1,64,3,3,1,1,512,512").family == "bf16rv"


def test_bf16x3_table_keys_and_subset(H):
    """BF16_CONV = "x3": the keys of conv_tune_bf16x3.json run the split-precision kernel with the table's variant and fp32 I/O; a layer
    outside the split form's subset stays on exactly the fp32 route."""
    H.BF16_CONV = "x3"
    for key, variant in table("conv_tune_bf16x3.json").items():
        assert route(H, key) == H.ConvRoute("bf16x3", variant, False, False, key)
    H.ACT_BF16 = True   # (the split form keeps fp32 activations whatever the switch says)
    kinds = {"bf16x3": 0, "fp32": 0}
    for key in table("conv_tune.json"):
        r = route(H, key)
        H.BF16_CONV = True
        r_bf16 = route(H, key)
        H.BF16_CONV = False
        r_fp32 = route(H, key)
        H.BF16_CONV = "x3"
        if r.family == "bf16x3":
            assert r_bf16.family.startswith("bf16") and not r.io_bf16
            kinds["bf16x3"] += 1
        else:
            assert r == r_fp32, (key, r, r_fp32)
            kinds["fp32"] += r_bf16.family.startswith("bf16")   # bf16-served, outside the x3 subset
    assert kinds["bf16x3"] >= 10 and kinds["fp32"] >= 2, kinds


def test_precedence(H):
    key = "8,64,64,64,1,64,3,3,1,1,64,64"
    H.TUNE, H.WINO = {key: 3}, {key: 5}
    assert (route(H, key).family, route(H, key).hint) == ("direct", -3)                    # tuned tile before the Winograd table
    H.TUNE = {}
    assert route(H, key).family == "wino4f"
    assert route(H, "16" + key[1:]).family == "wino4f"                                       # other batches: the batch-8 entry
    assert (route(H, key, tile_hint=2).family, route(H, key, tile_hint=2).hint) == ("direct", 2)
    H.BF16_CONV = True
    assert route(H, key).family == "bf16"                                                    # bf16 before the Winograd table
    assert route(H, key, winograd=True) == H.ConvRoute("wino", 0, False, True, key)          # ... not when a Winograd kernel was asked for
    assert route(H, key, winograd=True, wino_form=2).hint == 2
    dg = "8,64,64,64,4,16,3,3,1,1,64,64"                                                     # dilation groups: dg before rv before bf16
    rv = "8,64,128,128,1,64,3,3,1,1,128,128"
    H.ACT_BF16 = True
    assert route(H, dg).family == "bf16dg" and route(H, rv).family == "bf16rv" and route(H, key).family == "bf16"
    assert route(H, dg, bf16="rv").family == "bf16rv"
    assert route(H, rv, tile_hint=2) == H.ConvRoute("bf16", 2, True, False, rv)               # a caller's variant: the general kernel
    H.BF16_FORCE = 4
    assert route(H, rv) == H.ConvRoute("bf16", 4, True, False, rv)                          # tuner: the forced variant, no rv / dg
    H.BF16_FORCE = 0
    H.BF16_DG, H.BF16_RV = False, False
    assert route(H, dg).family == "bf16" and route(H, rv).family == "bf16"
    assert route(H, rv, bf16="rv", tile_hint=2) == H.ConvRoute("bf16rv", 2, True, True, rv)   # named: the caller's variant


def test_named_requests(H):
    plain = "8,64,64,64,1,64,3,3,1,1,64,64"
    # fused F(4x4): named on a layer it does not serve raises, unnamed (table) falls back to F(2x2)
    odd = "8,64,66,66,1,64,3,3,1,1,66,66"                                                    # H, W not multiples of 4
    with pytest.raises(RuntimeError, match="fused F"):
        route(H, odd, winograd=5)
    H.TUNE, H.WINO = {}, {odd: 5, plain + ",s": 5}
    assert route(H, odd).family == "wino" and route(H, plain + ",s").family == "wino"
    assert route(H, plain, winograd=5) == H.ConvRoute("wino4f", 0, False, True, plain)
    # the F(4x4) pair: where it does not serve the call, F(2x2)
    assert route(H, odd, winograd=4).family == "wino" and route(H, plain + ",s", winograd=4).family == "wino"
    assert route(H, plain, winograd=4).family == "wino4"
    with pytest.raises(RuntimeError, match="Winograd"):
        route(H, "8,64,64,64,1,64,3,3,2,1,32,32", winograd=True)
    # row-vector / dilation-group kernels named on layers they do not serve
    with pytest.raises(RuntimeError, match="row-vector"):
        route(H, "1,32,32,48,1,32,3,3,1,1,32,48", bf16="rv", x_dtype=torch.bfloat16)        # W % 64 != 0
    with pytest.raises(RuntimeError, match="dilation-group"):
        route(H, "8,128,64,64,4,16,3,3,1,1,64,64", bf16="dg", x_dtype=torch.bfloat16)       # Cin > 64
    with pytest.raises(RuntimeError, match="dilation-group"):
        route(H, "8,64,64,64,4,16,3,3,1,1,64,64,s", bf16="dg", x_dtype=torch.bfloat16)      # affine shift
    with pytest.raises(RuntimeError, match="bf16 activations"):
        route(H, "8,64,128,128,1,64,3,3,1,1,128,128", bf16="rv")                            # fp32 input, ACT_BF16 off
    assert route(H, "8,64,64,64,4,16,3,3,1,1,64,64", bf16="dg", x_dtype=torch.bfloat16).family == "bf16dg"
    # the general bf16 kernel named on a layer bf16_eligible refuses
    for key in ("8,8,64,64,1,64,3,3,1,1,64,64", "8,64,64,64,1,64,1,1,1,1,64,64"):           # Cin < 16, 1x1
        with pytest.raises(RuntimeError, match="bf16 kernel"):
            route(H, key, bf16=True)
    # fp32 input without ACT_BF16: bf16 operands, fp32 activations
    assert route(H, plain, bf16=True) == H.ConvRoute("bf16", 0, False, True, plain)
    assert route(H, plain, bf16=True, x_dtype=torch.bfloat16).io_bf16
    assert route(H, plain, bf16=False, winograd=False) == H.ConvRoute("direct", 0, False, False, plain)
