"""GPU checks of every form of the bf16 convolution kernels (csrc/conv_bf16.hip, conv_bf16_rv.hip, conv_bf16_dg.hip) against the float64
restatement of tests/conv_bf16_ref.py.  Every case of that module's table (a shape under an operand chain and an I/O form;
tests/test_conv_bf16_ref.py proves on the CPU that the table reaches every form name, both values of every fact the kernels branch on, and that
wrong variants of the restatement miss this bound on these very inputs) is launched through the C entries vsp_conv2d_bf16, _bf16x3, _bf16rv and
_bf16dg with a parameter block built here, on every tile variant of its mode (tile_hint).  For each launch the library's return code and
message must be the ones conv_bf16_ref.form states; an accepted launch must meet

    max |HIP - float64| <= 4 e_ref + 2e-6 max |float64|   (+ 2^-8 |float64| per element of a bf16 output)

with e_ref the error of the same restatement in float32 on the CPU (the rule of DESIGN sections 28 and 29), leave the sentinel intact in every
element it must not write, and give the same bits when it runs a second time (no atomics).  A bf16-I/O launch must equal the fp32-I/O launch of
the same operands, variant and rounding points rounded once.  No environment switch is set: the one-pixel bf16 tasks are reached through an
odd W or an x one element off its 4-byte boundary.  The references are computed once per (shape, chain, rounding points).

Recorded run (profiles/conv_bf16_forms_gputest.log: 261 passed in 9 s; 824 cases, 6169 launches, 5739 accepted, 430 refused as `form` states).
Worst e_hip / e_ref: general kernel with fp32 I/O 5.00 (stride 1, every PT), 4.61 (stride 2), 1.58 (transposed); split form 4.09 / 3.86 / 2.53;
row-vector 0.17; dilation-group 0.03; the bf16-output forms at most 0.18 beyond their store term -- what holds them is the bit equality with the
fp32-I/O result.  14 launches print more than 4 and pass by the additive term alone: the weight-heavy shapes wh (5.00) and whs2 (4.61), K = 4608
products in one fp32 chain at 7.0e-7 and 7.7e-7 max |float64|, and w32/bn on the split form (4.09).

Found while the table was written (read from the kernel, before the first run): with true groups conv_bf16_kernel scaled every group with the
in_scale entries of group 0 (the header and the fp32 kernels read them from g * x_group_stride on).  On the parent's library tg6, tg6o and s2tg3
under the style, stylefp and bn chains miss the bound with errors of 2.1 to 5.1; fixed in csrc/conv_bf16.hip.  The first run of the table on
the fixed library missed nothing."""
import ctypes as C
from collections import defaultdict

import pytest
import torch

import conv_bf16_ref as R
import conv_tile_ref as T

pytestmark = pytest.mark.gpu
torch.set_grad_enabled(False)
DEV = "cuda"
BF = torch.bfloat16
WORST = {}                  # (entry, mode, staging kind, PT) -> (ratio e_hip / e_ref, launch, e_hip / max |float64|)
COUNT = defaultdict(int)
OVER4 = defaultdict(int)    # shape -> launches that pass through the additive term of the bound alone
ENTRY = {"bf16": "vsp_conv2d_bf16", "x3": "vsp_conv2d_bf16x3", "rv": "vsp_conv2d_bf16rv", "dg": "vsp_conv2d_bf16dg"}


@pytest.fixture(scope="module")
def L():
    from vspbfr_amd import _lib
    return _lib


@pytest.fixture(scope="module")
def H():
    from vspbfr_amd import hip_ops
    return hip_ops


def _aligned(t, elem_off=0):
    """t on the device in a buffer of its own, its first element `elem_off` elements past a 16-byte boundary"""
    t = t.contiguous()
    buf = torch.zeros(t.numel() + 16, dtype=t.dtype, device=DEV)
    assert buf.data_ptr() % 16 == 0
    v = buf[elem_off:elem_off + t.numel()].view(t.shape)
    v.copy_(t)
    return v


class Launch:
    """the operands of a case on the device and its parameter block; run(entry, hint) fills y with the sentinel and calls the entry"""

    def __init__(self, L, H, case):
        base = case.base
        o, g, d = T.operands(base), T.geom(base), R.inputs(base)
        self.L, self.H, self.case, self.d = L, H, case, d
        act = torch.float32 if case.io == "f32" else BF
        es = 4 if case.io == "f32" else 2
        self.x = _aligned(d["x"].to(act), 1 if case.io == "bfoff" else 0)
        x_ptr = self.x.data_ptr() + case.x_coff * case.H * case.W * es
        assert x_ptr % 16 == R.x_align(case)
        self.t = {k: _aligned(v.to(act) if k in ("res1", "res2") else v) for k, v in d.items() if k not in ("x", "w", "wp")}
        self.y = torch.empty(case.B, g.y_ch, g.y_h, g.y_w, device=DEV, dtype=act)
        self.sentinel = float(torch.tensor(R.SENTINEL).to(act))
        self.weights = {}
        t, p = self.t, L.ConvParams()
        ptr = lambda k: t[k].data_ptr() if k in t else None     # noqa: E731
        p.x, p.y = x_ptr, self.y.data_ptr()
        p.B, p.Cin, p.H, p.W, p.G, p.cout_g = case.B, case.Cin, case.H, case.W, case.G, case.cout_g
        p.KH = p.KW = 3
        p.transposed = 1 if case.transposed else 0
        if case.transposed:     # the entry ignores and normalises these
            p.OH = p.OW = p.stride_y = p.stride_x = p.osy = p.osx = 1
        else:
            p.OH, p.OW, p.stride_y, p.stride_x = g.OH, g.OW, case.sy, case.sx
            p.osy = p.osx = 1
        for i in range(4):
            j = i if i < len(case.dil) else 0
            p.dil[i], p.pad_y[i], p.pad_x[i] = case.dil[j], case.pad_y[j], case.pad_x[j]
        p.y_ch, p.y_coff, p.y_h, p.y_w = g.y_ch, g.y_coff, g.y_h, g.y_w
        self.scale_ptr = t["in_scale"].data_ptr() + 4 * case.x_coff if "in_scale" in t else None
        self.scale_bs = g.x_ch if o["in_scale"] == "sample" else 0
        p.in_scale, p.in_scale_bstride, p.in_shift = self.scale_ptr, self.scale_bs, ptr("in_shift")
        p.out_scale, p.ch_scale, p.ch_bias = ptr("out_scale"), ptr("ch_scale"), ptr("ch_bias")
        p.act1, p.bias1, p.slope1, p.gain1 = (1 if o["act1"] else 0), ptr("bias1"), 0.2, T.SQRT2
        p.noise, p.noise_w = ptr("noise"), ptr("noise_w")
        p.act2, p.bias2, p.prelu = o["act2"], ptr("bias2"), ptr("prelu")
        p.slope2, p.gain2 = o["slope2"], o["gain2"]
        p.res1, p.res2, p.res_ch, p.res_coff = ptr("res1"), ptr("res2"), g.res_ch, g.res_coff
        p.x_ch, p.x_group_stride = g.x_ch if (case.x_gs or case.x_coff) else 0, case.x_gs
        p.io_bf16 = 0 if case.io == "f32" else 1
        self.p = p

    def weight(self, entry):
        """the entry's weight image from the library's own packer (and its byte stride between images)"""
        key = "modw" if self.case.io == "modw" else entry      # (per-image weights on an entry that refuses them: the refusal is the test)
        if key not in self.weights:
            H, wp = self.H, self.d["wp"].to(DEV)
            if key == "modw":
                case = self.case
                style = self.d["in_scale"][:, case.x_coff:case.x_coff + case.Cin].contiguous().to(DEV)
                pc = H.PackedConv(wp, case.G, case.cout_g, case.Cin, 3, 3, 1, (1,), (1,))
                w, nbytes = H.bf16_modulated_weight(pc, style)
                assert torch.equal(w.cpu().view(torch.int16), R.modulated_image(self.d["wp"], style.cpu()).view(torch.int16)), "vsp_modulate_weight_bf16"
                self.weights[key] = (w, nbytes)
            else:
                pack = {"bf16": H.bf16_weight, "x3": H.bf16x3_weight, "rv": H.bf16rv_weight, "dg": H.bf16dg_weight}[key]
                self.weights[key] = (pack(wp).contiguous(), 0)
        return self.weights[key]

    def run(self, entry, hint):
        """-> (return code, message, y)"""
        p, L = self.p, self.L
        modw = self.case.io == "modw"
        can_pack = not (entry == "rv" and (self.case.cout_g % 8 or self.case.Cin % 8)) and not (entry == "dg" and (self.case.cout_g > 16 or self.case.Cin > 64))
        w, bs = self.weight(entry if can_pack else "bf16")
        p.w, p.w_bstride = w.data_ptr(), (bs if modw else 0)
        p.in_scale, p.in_scale_bstride = (None, 0) if modw else (self.scale_ptr, self.scale_bs)
        p.tile_hint = hint
        self.y.fill_(R.SENTINEL)
        rc = getattr(L.lib, ENTRY[entry])(C.byref(p), C.c_void_p(torch.cuda.current_stream().cuda_stream))
        return rc, (L.last_error() if rc else ""), self.y


class Checker:
    """the shared references of a (shape, chain, rounding points) on the device"""
    cache = {}

    def __new__(cls, base, how):
        if (base, how) not in cls.cache:
            self = super().__new__(cls)
            self.ref64, _, self.bound, self.e_ref = R.references(base, how)
            self.top = (self.bound - 4.0 * self.e_ref) / 2e-6
            self.ref = self.ref64.to(DEV)
            self.m = T.written(base).to(DEV)
            self.store = self.ref.abs() * 2.0 ** -8
            if len(cls.cache) > 8:
                cls.cache.clear()
            cls.cache[(base, how)] = self
        return cls.cache[(base, how)]

    def errors(self, y, sentinel, bf_out):
        """-> [max error on the written elements beyond the bf16 store term, max change of the other elements]"""
        diff = torch.nan_to_num((y.double() - self.ref).abs(), nan=float("inf"))
        if bf_out:
            diff = (diff - self.store).clamp_min(0.0)
        zero = torch.zeros_like(diff)
        out = torch.nan_to_num((y.double() - sentinel).abs(), nan=float("inf"))
        return torch.stack([torch.where(self.m, diff, zero).max(), torch.where(self.m, zero, out).max()])


def _device_fault(msg):
    return any(s in msg for s in ("HIP error", "illegal memory access", "hipError", "unspecified launch failure", "launch failed"))


def _kind(name):
    if name.startswith(("x3", "rv", "dg")):
        return name.split("/")[0], name.split("/")[-1]
    parts = name.split("/")
    return ("nosc" if name.endswith("nosc") else "pair" if parts[3].startswith("pair") else parts[3]), parts[2]


@pytest.mark.parametrize("name", [b.name for b in R.BASES])
def test_every_form_matches_float64(L, H, name):
    base = R.CASE_BY_NAME[name]
    wrong, bad, lines, ran = [], [], [], 0
    y32 = {}
    try:
        for case in [c for c in R.CASES if c.base == base]:
            launch = Launch(L, H, case)
            bf_out = case.io != "f32"
            cells = defaultdict(list)
            for entry, hint in R.launches(case):
                f = R.form(case, entry, hint)
                rc, msg, y = launch.run(entry, hint)
                tag = f"{case.name} {entry}:{hint}"
                if rc != 0 and _device_fault(msg):
                    raise RuntimeError(msg)
                if rc != f.code or (f.why and f.why not in msg):
                    wrong.append((tag, f"form: {f.code} {f.why!r} {f.name}", f"library: {rc} {msg!r}"))
                    continue
                if rc != 0:
                    if not bool((y == launch.sentinel).all()):
                        bad.append((tag, "a refused launch wrote"))
                    continue
                how = R.rounding(case, entry)
                chk = Checker(base, how)
                first = y.clone()
                e_hip, e_out = chk.errors(first, launch.sentinel, bf_out).cpu().tolist()
                rc2, msg2, y2 = launch.run(entry, hint)
                if rc2 != 0 or not torch.equal(y2.view(torch.int16 if bf_out else torch.int32), first.view(torch.int16 if bf_out else torch.int32)):
                    bad.append((tag, f.name, "second run differs", rc2, msg2))
                ran += 1
                ratio = e_hip / chk.e_ref if chk.e_ref > 0 else float("nan")
                kind, pt = _kind(f.name)
                key = (entry, R.mode_of(case), kind, pt)
                COUNT[key] += 1
                if ratio == ratio and ratio >= WORST.get(key, (-1.0, "", 0.0))[0]:
                    WORST[key] = (ratio, f"{tag} {f.name}", e_hip / chk.top)
                if ratio > 4.0:
                    OVER4[case.shape.name] += 1
                cells[f"{e_hip:.1e}/{ratio:.2f}"].append(f"{entry}:{hint}={f.name}[{f.order}]")
                if not e_hip <= chk.bound:
                    bad.append((tag, f.name, f.order, "error", e_hip, "bound", chk.bound))
                if e_out != 0.0:
                    bad.append((tag, f.name, f.order, "wrote outside its elements", e_out))
                # same operands, both I/O forms: the bf16-I/O result is the fp32-I/O result rounded once
                if entry == "bf16" and how == "pixel":
                    if not bf_out:
                        y32[hint] = first
                    elif hint in y32 and not torch.equal(first, y32[hint].to(BF)):
                        bad.append((tag, f.name, "differs from the fp32-I/O result rounded once", float((first.float() - y32[hint].to(BF).float()).abs().max())))
            lines.append(f"  {case.io}: " + "  ".join(f"{k}@{','.join(v)}" for k, v in cells.items()))
        torch.cuda.synchronize()
    except RuntimeError as e:
        if _device_fault(str(e)):
            pytest.exit(f"{name}: the device reported a fault ({e}); no further case is launched on it", returncode=3)
        raise
    print(f"\nCONV-BF16 {name} launches {ran}\n" + "\n".join(lines))
    assert not wrong, wrong[:6]
    assert not bad, bad[:6]
    assert ran, name


@pytest.mark.parametrize("G,cin,cout", [(1, 8, 8), (1, 24, 36), (2, 40, 12), (3, 16, 72), (4, 8, 20), (1, 64, 160)])
def test_weight_images_equal_the_packers(L, H, G, cin, cout):
    """the restated weight images (tests/test_conv_bf16_ref.py reads them back through the header's index formulas) against the library's
    packers, bit for bit: ragged Cin and cout_g, one to four groups"""
    gen = torch.Generator().manual_seed(G * 1000 + cin + cout)
    wp = torch.randn(G, 9, cin, cout, generator=gen)
    bits = lambda t: t.cpu().contiguous().view(torch.int16)      # noqa: E731
    assert torch.equal(bits(H.bf16_weight(wp.to(DEV))), bits(R.bf16_image(wp)))
    assert torch.equal(bits(H.bf16x3_weight(wp.to(DEV))), bits(R.bf16x3_image(wp)))
    if cout % 8 == 0:
        assert torch.equal(bits(H.bf16rv_weight(wp.to(DEV))), bits(R.bf16rv_image(wp)))
    style = (torch.rand(3, cin, generator=gen) + 0.5)
    pc = H.PackedConv(wp.to(DEV), G, cout, cin, 3, 3, 1, (1,) * G, (1,) * G)
    w, nbytes = H.bf16_modulated_weight(pc, style.to(DEV))
    assert nbytes == 2 * R.bf16_image(wp).numel()
    assert torch.equal(bits(w), bits(R.modulated_image(wp, style)))


def test_zz_worst_ratio_per_form(L):
    """every (entry, mode, staging form, PT) has run; prints the worst e_hip / e_ref of each with that launch's error relative to
    max |float64|, and the count of launches that pass by the additive term of the bound alone"""
    for key in sorted(WORST):
        r, what, rel = WORST[key]
        print(f"CONV-BF16-WORST {key[0]:4s} {key[1]} {key[2]:5s} {key[3]:5s} {r:6.2f}  {what}  (e_hip = {rel:.2e} max|f64|; {COUNT[key]} launches)")
    print(f"CONV-BF16-OVER4 {sum(OVER4.values())} of {sum(COUNT.values())} launches: " + " ".join(f"{k}={v}" for k, v in sorted(OVER4.items())))
    assert COUNT, "this test closes a run of the whole module"
    want = defaultdict(int)
    for c in R.CASES:
        for e, h in R.launches(c):
            f = R.form(c, e, h)
            if f.code == R.OK:
                want[(e, R.mode_of(c)) + _kind(f.name)] += 1
    assert dict(COUNT) == dict(want)      # every accepted launch was measured
