"""Tensor-level wrappers over the C ABI (include/vspbfr_hip.h).

PyTorch is plumbing here: it owns device memory and the current HIP stream; all arithmetic happens in
libvspbfr_hip.so.  Every wrapper requires CUDA(HIP) fp32 contiguous tensors and raises RuntimeError otherwise --
there is no CPU path (the reference's own CPU branch lives in oracle/, test-only).
"""
import ctypes as C
import math
from collections import namedtuple

import os

import torch

from . import _lib
from ._lib import ConvParams, FirEpilogue, GemmParams, check, lib, tune_env

SQRT2 = math.sqrt(2.0)


class ConvProfiler:
    """Optional per-launch timing of vsp_conv2d_f32 with HIP events on the launch stream (bench.py's roofline leg):
    records (algorithmic FLOPs, start event, end event) for every conv launch while installed as `hip_ops.PROFILER`."""

    def __init__(self):
        self.records = []

    def begin(self):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        return ev

    def end(self, start, flops, tag, nbytes=0):
        ev = torch.cuda.Event(enable_timing=True)
        ev.record()
        self.records.append((flops, start, ev, tag, nbytes))

    def summary(self):
        """-> (total algorithmic FLOPs, total ms, launches); call after a device synchronize."""
        fl = sum(r[0] for r in self.records)
        ms = sum(r[1].elapsed_time(r[2]) for r in self.records)
        return fl, ms, len(self.records)

    def executed_flops(self):
        """FLOPs the matrix pipe actually EXECUTED: a Winograd F(2x2,3x3) launch runs 16 multiplies per 2x2 output tile where the
        direct form (the algorithmic count of `summary`) has 36; every other kernel executes its algorithmic count."""
        f = {"wino": 16.0 / 36.0, "wino4": 36.0 / 144.0, "wino4f": 36.0 / 144.0,   # F(4x4,3x3): 36 multiplies per 4x4 tile against 144
             "tconvw": 25.0 / 36.0}   # transposed F(2x2,2x2) phases: 25 multiplies per 2x2 positions against 36
        return sum(r[0] * (f.get(r[3][7], 1.0) if len(r[3]) > 7 else 1.0) for r in self.records)

    def by_kind(self):
        """{kernel family: (algorithmic FLOPs, ms, launches)} -- direct / pipelined / tconv / wino / bf16."""
        out = {}
        for r in self.records:
            k = r[3][7] if len(r[3]) > 7 else "?"
            a = out.setdefault(k, [0.0, 0.0, 0])
            a[0] += r[0]
            a[1] += r[1].elapsed_time(r[2])
            a[2] += 1
        return {k: (v[0], v[1], v[2]) for k, v in out.items()}

    def algorithmic_bytes(self):
        """Sum over the launches of the bytes a convolution must move when every operand crosses HBM exactly once: input image,
        output, weights, noise map and residuals at their element sizes (the unit of the HBM roofline)."""
        return sum(r[4] for r in self.records)


WGRAD_WORKSPACE = True   # False: vsp_conv2d_wgrad_f32 reduces its split-K partial sums with atomics
PROFILER = None
RECORDER = None  # tools/autotune_conv.py: list collecting the shape key of every conv launch


def _load_tune_table():
    import json
    import os
    path = os.environ.get("VSPBFR_CONV_TUNE") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "conv_tune.json")  # (override: tuning runs)
    if not os.path.exists(path):
        return {}
    with open(path) as f:
        return json.load(f)


def _config_ids():
    return {lib.vsp_conv2d_config_name(i).decode(): i + 1 for i in range(lib.vsp_conv2d_num_configs())}


# shape key -> 1-based tile configuration id measured fastest on MI355X (tools/autotune_conv.py stores configuration NAMES,
# resolved here); shapes that are not in the table use the library's cost model (tile_hint = 0)
CONFIG_IDS = _config_ids()
TUNE = {k: CONFIG_IDS[v] for k, v in _load_tune_table().items() if v in CONFIG_IDS}
# shapes where a Winograd kernel won: True = F(2x2,3x3) (vsp_conv2d_winograd_f32), 4 = F(4x4,3x3) (vsp_conv2d_winograd4_f32, deep layers)
#   5 = F(4x4,3x3) fused in registers (vsp_conv2d_winograd4f_f32, shallow wide layers)
#   (also the SMART dilation-group launches of 128 / 256 channels: one launch, a partition of workgroups per group, dilated groups through the
#   kernel's LDS window loader)
WINO = {k: ({"winograd4": 4, "winograd4f": 5}.get(v, True)) for k, v in _load_tune_table().items()
        if v in ("winograd", "winograd4", "winograd4f")}


def _load_bf16_tune(name="conv_tune_bf16.json"):
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), name)
    if not os.path.exists(path):
        return {}
    with open(path) as f:
        return {k: int(v) for k, v in json.load(f).items()}


# shape key -> tile variant of vsp_conv2d_bf16 measured fastest INSIDE the pipeline (tools/autotune_bf16.py); other shapes use the
# library's rule.  BF16_FORCE (tuner only): variant tried on every launch it fits.
BF16_TUNE = _load_bf16_tune()
BF16X3_TUNE = _load_bf16_tune("conv_tune_bf16x3.json")
BF16_FORCE = 0


# the data gradient of the four dilated SMART branches as one convolution (conv_pipe.hip MODE 3) instead of a grouped conv + a sum over
# the branches (tools / A-B runs can switch it off)
SMART_ADJOINT_ONE_PASS = tune_env("VSP_SMART_ADJOINT_ONE_PASS", "1") != "0"
# training: demodulation coefficients and their gradient on the fused kernels (vsp_demod_weight_f32) instead of torch autograd
FUSED_DEMOD_GRAD = tune_env("VSP_FUSED_DEMOD_GRAD", "1") != "0"
# training: a discriminator ResBlock of the first-order passes as one autograd node (discriminator._ResBlockFO)
RESBLOCK_ONE_NODE = tune_env("VSP_RESBLOCK_ONE_NODE", "1") != "0"


def conv_key(B, Cin, H, W, pc, OH, OW):
    return f"{B},{Cin},{H},{W},{pc.G},{pc.cout_g},{pc.kh},{pc.kw},{pc.stride},{pc.dil[0]},{OH},{OW}" + (
        f",g{pc.x_group_stride}" if pc.x_group_stride else "") + (",q" if pc.dil_by_input_quarter else "")


def _tuned(table, key, default=0):
    """The table's entry for this shape key, else that of the same layer at batch 8 (the batch the tables were measured at)."""
    v = table.get(key)
    return v if v is not None else table.get("8" + key[key.index(","):], default)


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def operand_device(args, kwargs=None):
    """Device index shared by every tensor among an operator's arguments (tensors inside lists / tuples included), None when there is
    no tensor; RuntimeError when they lie on different devices.  Pure host logic (CPU-testable): the C ABI takes raw pointers and one
    stream, so operands on two devices cannot be served by one launch -- the reference's extensions would fault on the foreign pointer,
    this refuses."""
    dev = None
    stack = list(args) + (list(kwargs.values()) if kwargs else [])
    while stack:
        a = stack.pop()
        if isinstance(a, torch.Tensor):
            if dev is None:
                dev = a.device
            elif a.device != dev:
                raise RuntimeError(f"operands on different devices: {dev} and {a.device}")
        elif isinstance(a, (list, tuple)):
            stack.extend(a)
    return dev


def device_guarded(fn):
    """The reference's `at::cuda::OptionalCUDAGuard device_guard(device_of(input))` (op/fused_bias_act.cpp:25, op/upfirdn2d.cpp:23) for the
    ctypes path: the launch goes to the TENSORS' device and that device's current stream (`_stream()` is evaluated inside the guard), not
    to whatever device is current in the calling thread; the previous device comes back on return.  One process per GPU never takes the
    slow branch."""
    import functools

    @functools.wraps(fn)
    def guarded(*args, **kwargs):
        dev = operand_device(args, kwargs)
        if dev is None or dev.type != "cuda" or dev.index == torch.cuda.current_device():
            return fn(*args, **kwargs)
        with torch.cuda.device(dev):
            return fn(*args, **kwargs)

    guarded.__wrapped_op__ = fn
    return guarded


def _req(t, name, bf16_ok=False):
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{name} must be a tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")
    if t.dtype != torch.float32 and not (bf16_ok and t.dtype == torch.bfloat16):
        raise RuntimeError(f"{name} must be float32{' or bfloat16' if bf16_ok else ''} (got {t.dtype})")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")
    return t


# bf16 ACTIVATIONS in HBM (BASELINE configs[2]; needs BF16_CONV = True).  Off: every tensor is fp32.  On: a layer that runs on a
# bf16-I/O kernel (vsp_conv2d_bf16 with io_bf16, vsp_upfirdn2d_bf16, vsp_pointwise_bf16) reads and writes bf16 tensors; the dtype
# simply follows the kernel, and a consumer whose kernel wants the other type converts its (small-map) input first -- the
# transitions sit at the 16^2 maps, where the bf16 conv kernel hands over to the fp32 ones.
ACT_BF16 = False
BF = torch.bfloat16


def to_bf16(t):
    """fp32 -> bf16 (round to nearest even) through vsp_convert_f32_to_bf16; bf16 tensors pass through."""
    if t is None or t.dtype == BF:
        return t
    t = _req(t, "tensor")
    out = torch.empty(t.shape, device=t.device, dtype=BF)
    check(lib.vsp_convert_f32_to_bf16(_ptr(out), _ptr(t), t.numel(), _stream()), "convert_f32_to_bf16")
    return out


def to_f32(t):
    """bf16 -> fp32 (exact) through vsp_convert_bf16_to_f32; fp32 tensors pass through."""
    if t is None or t.dtype == torch.float32:
        return t
    t = _req(t, "tensor", bf16_ok=True)
    out = torch.empty(t.shape, device=t.device, dtype=torch.float32)
    check(lib.vsp_convert_bf16_to_f32(_ptr(out), _ptr(t), t.numel(), _stream()), "convert_bf16_to_f32")
    return out


def as_dtype(t, dtype):
    return to_bf16(t) if dtype == BF else to_f32(t)


def _ptr(t):
    return None if t is None else C.c_void_p(t.data_ptr())


def _opt(t, name):
    return None if t is None else _req(t, name)


# ----------------------------------------------------------------------------------------------- fused_bias_act
def fused_bias_act(input, bias, refer, act, grad, alpha, scale):
    """Same signature as the reference's native `fused.fused_bias_act` (op/fused_bias_act.cpp:18-31):
    empty `bias` / `refer` tensors mean "absent"; returns a new tensor."""
    x = _req(input, "input")
    b = _req(bias, "bias") if bias is not None and bias.numel() else None
    r = _req(refer, "refer") if refer is not None and refer.numel() else None
    out = torch.empty_like(x)
    step_b = 1
    for i in range(2, x.dim()):
        step_b *= x.size(i)
    size_b = b.numel() if b is not None else 0
    if r is not None and r.numel() != x.numel():
        raise RuntimeError("refer must have the same number of elements as input")
    check(lib.vsp_fused_bias_act_f32(_ptr(out), _ptr(x), _ptr(b), _ptr(r), x.numel(), step_b, size_b, int(act),
                                     int(grad), float(alpha), float(scale), _stream()), "fused_bias_act")
    return out


# ----------------------------------------------------------------------------------------------- upfirdn2d
def fir_out_size(in_h, in_w, kh, kw, up_x, up_y, down_x, down_y, px0, px1, py0, py1):
    return ((in_h * up_y + py0 + py1 - kh + down_y) // down_y, (in_w * up_x + px0 + px1 - kw + down_x) // down_x)


def upfirdn2d_native_layout(input, kernel, up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1, epilogue=None):
    """Same contract as the reference's native `upfirdn2d_op.upfirdn2d` (op/upfirdn2d.cpp:17-31):
    input [major, in_h, in_w, minor] -> new tensor [major, out_h, out_w, minor]."""
    x = _req(input, "input", bf16_ok=True)
    k = _req(kernel, "kernel")
    if x.dim() != 4 or k.dim() != 2:
        raise RuntimeError("upfirdn2d expects input [major,H,W,minor] and a 2-D kernel")
    major, in_h, in_w, minor = x.shape
    kh, kw = k.shape
    out_h, out_w = fir_out_size(in_h, in_w, kh, kw, up_x, up_y, down_x, down_y, pad_x0, pad_x1, pad_y0, pad_y1)
    if out_h < 0 or out_w < 0:
        raise RuntimeError(f"upfirdn2d: negative output size {out_h}x{out_w}")
    out = torch.empty((major, out_h, out_w, minor), device=x.device, dtype=x.dtype)
    epi = C.byref(epilogue) if epilogue is not None else None
    fn = lib.vsp_upfirdn2d_bf16 if x.dtype == BF else lib.vsp_upfirdn2d_f32
    check(fn(_ptr(out), _ptr(x), _ptr(k), major, in_h, in_w, minor, kh, kw, up_x, up_y, down_x,
             down_y, pad_x0, pad_x1, pad_y0, pad_y1, epi, _stream()), "upfirdn2d")
    return out


def fir_bf16_ok(kh, kw, up, down, minor, out_w, in_w=4, in_h=1):
    """What vsp_upfirdn2d_bf16 serves: the blur form on planes of at least 1 x 4 pixels (narrower ones under wide pads: fp32, generic kernel)."""
    return up == 1 and down == 1 and minor == 1 and out_w >= 16 and in_w >= 4 and in_h >= 1 and (kh, kw) in ((4, 4), (3, 3), (2, 2))


SEPARABLE_BLUR = tune_env("VSP_FIR_SEPARABLE", "1") != "0"   # (A/B runs: the 2-D form)


def taps_separable(kernel):
    """True when the 2-D taps are exactly an outer product k[i][j] == k[i][0] * k[0][j] / k[0][0] in fp32 (make_kernel of a 1-D list: every
    blur of the path) -- decided once per tap tensor on the host (one small device-to-host copy at first use); the answer rides on the
    tensor OBJECT (a module buffer lives as long as its module; a temporary takes its answer with it -- an address is not an identity)."""
    hit = getattr(kernel, "_vsp_separable", None)
    if hit is not None and hit[0] == kernel._version:
        return hit[1]
    k = kernel.detach().float().cpu()
    sep = False
    if k.dim() == 2:
        k = k.flip(0, 1)        # the kernels work on the flipped taps (a true convolution): row factor = first column / corner
        sep = bool(float(k[0, 0]) != 0.0 and torch.equal(k, ((k[:, :1] / k[0, 0]) * k[:1, :]).float()))
    try:
        kernel._vsp_separable = (kernel._version, sep)
    except (AttributeError, RuntimeError):
        pass
    return sep


def blur_fused(x, kernel, pad, plane_scale=None, noise=None, noise_w=None, act_bias=None, act=False, res1=None,
               res2=None, slope=0.2, gain=SQRT2):
    """NCHW blur (up=down=1) with the fused demod/noise/bias/leaky-relu/residual epilogue of the C ABI.  The element type of
    x decides the kernel (fp32 / bf16 activations); residuals are converted to it when they differ (small maps only).  Outer-product
    taps are flagged (VSP_FIR_SEPARABLE): the kernels may then run a row pass and a column pass."""
    x = _req(x, "x", bf16_ok=True)
    B, Cc, H, W = x.shape
    kh, kw = kernel.shape
    if x.dtype == BF and not fir_bf16_ok(kh, kw, 1, 1, 1, fir_out_size(H, W, kh, kw, 1, 1, 1, 1, pad[0], pad[1], pad[0], pad[1])[1], W, H):
        x = to_f32(x)
    res1, res2 = as_dtype(res1, x.dtype), as_dtype(res2, x.dtype)
    epi = FirEpilogue()
    keep = [_opt(plane_scale, "plane_scale"), _opt(noise, "noise"), _opt(noise_w, "noise_w"), _opt(act_bias, "act_bias"),
            _req(res1, "res1", True) if res1 is not None else None, _req(res2, "res2", True) if res2 is not None else None]
    epi.plane_scale, epi.noise, epi.noise_w, epi.act_bias, epi.res1, epi.res2 = [
        (t.data_ptr() if t is not None else None) for t in keep]
    epi.channels, epi.act, epi.slope, epi.gain = Cc, 1 if act else 0, slope, gain
    epi.flags = _lib.FIR_SEPARABLE if (SEPARABLE_BLUR and taps_separable(kernel)) else 0
    out = upfirdn2d_native_layout(x.view(B * Cc, H, W, 1), kernel, 1, 1, 1, 1, pad[0], pad[1], pad[0], pad[1], epi)
    return out.view(B, Cc, out.shape[1], out.shape[2])


# ----------------------------------------------------------------------------------------------- conv2d
class PackedConv:
    """A convolution weight in the kernel's layout Wp[g][tap][ci][co_g] (include/vspbfr_hip.h) plus its geometry.
    Built once per device on first use (pack_weight below; cached on the owning module)."""

    __slots__ = ("w", "G", "cout_g", "cin", "kh", "kw", "stride", "dil", "pad_y", "pad_x", "x_group_stride", "dil_by_input_quarter", "_forms")

    def __init__(self, w, G, cout_g, cin, kh, kw, stride=1, dil=(1,), pad_y=(0,), pad_x=None, x_group_stride=0, dil_by_input_quarter=False):
        self.w, self.G, self.cout_g, self.cin, self.kh, self.kw = w, G, cout_g, cin, kh, kw
        self.stride = stride
        # True: the data gradient of four dilated branches in one pass (include/vspbfr_hip.h: dil_by_input_quarter) -- G = 4 blocks of
        # cout_g output channels over ALL cin input channels, dil / pad belong to the input-channel quarter
        self.dil_by_input_quarter = bool(dil_by_input_quarter)
        self.x_group_stride = x_group_stride  # > 0: true grouped conv, group g reads input channels [g*stride, +cin)
        rep = lambda t, fill: tuple(t) * 4 if len(t) == 1 else tuple(t) + (fill,) * (4 - len(t))  # noqa: E731
        self.dil = rep(dil, 1)          # one value = the same geometry for every group
        self.pad_y = rep(pad_y, 0)
        self.pad_x = rep(pad_y if pad_x is None else pad_x, 0)
        self._forms = {}

    @property
    def cout(self):
        return self.G * self.cout_g

    def form(self, name):
        """The weight in the layout of kernel family `name` (a key of WEIGHT_FORMS), built on first use and kept with the packed weight."""
        f = self._forms.get(name)
        if f is None:
            with torch.no_grad():
                f = self._forms[name] = WEIGHT_FORMS[name](self.w)
        return f


# "bf16 kernels" configuration (BASELINE configs[2]): eligible convolutions run on vsp_conv2d_bf16 (bf16 MFMA, fp32
# accumulate, fp32 activations in HBM).  Off by default: the parity path is fp32 end to end.
BF16_CONV = False   # True: bf16 operands; "x3": split precision (hi + lo bf16 pairs, three MFMAs per product: fp32-grade results)
_env_dtype = os.environ.get("VSPBFR_CONV_DTYPE", "")   # process-wide default of the switch: "bf16" / "bf16x3" (entry points set it explicitly)
if _env_dtype:
    if _env_dtype not in ("f32", "bf16", "bf16x3"):
        raise RuntimeError(f"VSPBFR_CONV_DTYPE must be f32, bf16 or bf16x3 (got {_env_dtype!r})")
    BF16_CONV = {"f32": False, "bf16": True, "bf16x3": "x3"}[_env_dtype]


def bf16_eligible(pc, H, W, OH, OW, transposed=False, out_stride=(1, 1), out_offset=(0, 0)):
    """What vsp_conv2d_bf16 serves: 3x3 kernels with >= 16 input channels as (a) stride 1, padding = dilation, G <= 4 dilation
    groups over one input or true groups; (b) stride 2, dilation 1, padding 0 or 1, G = 1 or true groups; (c) the stride-2
    transposed conv (G = 1); dense output for (a) and (b)."""
    if pc.kh != 3 or pc.kw != 3 or pc.cin < 16 or pc.cin % 8 or pc.dil_by_input_quarter:
        return False
    if transposed:
        return pc.G == 1
    if tuple(out_stride) != (1, 1) or tuple(out_offset) != (0, 0):
        return False
    if pc.stride == 2:
        return (pc.dil[0] == 1 and pc.pad_y[0] == pc.pad_x[0] and pc.pad_y[0] in (0, 1) and (pc.G == 1 or pc.x_group_stride > 0)
                and (OH, OW) == conv2d_out_size(H, W, pc))
    if pc.stride != 1 or (pc.G > 4 and pc.x_group_stride == 0):
        return False
    if any(pc.pad_y[g] != pc.dil[g] or pc.pad_x[g] != pc.dil[g] for g in range(min(pc.G, 4))):
        return False
    return (OH, OW) == (H, W)


def bf16_profitable(pc, H, W, OH, OW, transposed=False):
    """Shapes on which the bf16 kernel beats the fp32 kernels (tools/bench_bf16.py, tools/conv_breakdown.py): 32-pixel row
    segments need maps (polyphase sub-images for dilation groups) at least 8-16 pixels wide."""
    if transposed:
        return W >= 16
    if pc.stride == 2:
        return OW >= 8
    dmax = max(pc.dil[:min(pc.G, 4)])
    return W >= 16 and H // dmax >= 2


def bf16_weight(wp):
    """packed weights (G, 9, Cin, cout_g) fp32 -> bf16 in the LDS-image order of vsp_conv2d_bf16:
    [group][chunk][tap][octet 2][co_pad][8] with ci = 16 chunk + 8 octet + j; Cin zero-padded to 16, cout_g to 32."""
    ng, T, cin, cout = wp.shape
    nch, co_pad = (cin + 15) // 16, (cout + 31) // 32 * 32
    Wz = wp.new_zeros(ng, T, nch * 16, co_pad)
    Wz[:, :, :cin, :cout] = wp
    Wz = Wz.view(ng, T, nch, 2, 8, co_pad).permute(0, 2, 1, 3, 5, 4)
    return Wz.to(torch.bfloat16).contiguous().view(-1)


def bf16rv_weight(wp):
    """packed weights (G, 9, Cin, cout_g) fp32 -> per group [chunk Cin/8][ky 3][quad 2][half 2][co_pad][8] bf16 with element e = channel
    8 chunk + 4 quad + 2 half + (e >> 2), horizontal tap kx = e & 3 (kx = 3: zero), co_pad = cout_g rounded up to 32 (zero rows) --
    the A fragments of vsp_conv2d_bf16rv (G > 1: the dilation groups of one launch, one after the other)."""
    ng, T, cin, cout = wp.shape
    if T != 9 or cin % 8 or cout % 8:
        raise RuntimeError("bf16rv_weight: 3x3, Cin % 8 == 0, channels per group % 8 == 0")
    co_pad = (cout + 31) // 32 * 32
    Wz = wp.new_zeros(ng, 3, 4, cin, co_pad)
    Wz[:, :, :3, :, :cout] = wp.view(ng, 3, 3, cin, cout)
    Wz = Wz.view(ng, 3, 4, cin // 8, 2, 2, 2, co_pad).permute(0, 3, 1, 4, 5, 7, 6, 2)   # group, chunk, ky, quad, half, co, pair, kx
    return Wz.to(torch.bfloat16).contiguous().view(-1)


def bf16rv_eligible(pc, H, W, OH, OW, transposed=False, out_stride=(1, 1), out_offset=(0, 0)):
    """What vsp_conv2d_bf16rv serves (bf16 activations on top; the entry re-checks alignment and returns VSP_ENOTSUP): plain 3x3 layers
    and the 2-4 dilation groups of a SMART branch launch (dilations from 1, 2, 4, 8 over one input)."""
    if (transposed or pc.kh != 3 or pc.kw != 3 or pc.stride != 1 or pc.cin % 8 or pc.cin > 256 or W % 64 or (OH, OW) != (H, W)
            or tuple(out_stride) != (1, 1) or tuple(out_offset) != (0, 0) or pc.dil_by_input_quarter):
        return False
    if pc.G == 1:
        return pc.dil[0] == 1 and pc.pad_y[0] == 1 and pc.pad_x[0] == 1 and pc.cout_g % 32 == 0
    return (2 <= pc.G <= 4 and pc.x_group_stride == 0 and pc.cout_g % 8 == 0
            and all(pc.dil[g] in (1, 2, 4, 8) and pc.pad_y[g] == pc.dil[g] and pc.pad_x[g] == pc.dil[g] for g in range(pc.G)))


def bf16dg_weight(wp):
    """packed weights (G, 9, Cin, cout_g) fp32 -> fp32 [group][stage Cin/32][tap 9][lane 64][8] with lane = 16 kb + co, element e = input
    channel 32 stage + 8 kb + e (zero-padded: Cin to 32 stages, cout_g to 16) -- the A fragments of vsp_conv2d_bf16dg, which multiplies them
    by the image's style scale and rounds to bf16 itself."""
    ng, T, cin, cout = wp.shape
    if T != 9 or cout > 16 or cin > 64:
        raise RuntimeError("bf16dg_weight: 3x3, at most 16 channels per group, at most 64 input channels")
    nst = 1 if cin <= 32 else 2
    Wz = wp.new_zeros(ng, 9, nst * 32, 16)
    Wz[:, :, :cin, :cout] = wp
    return Wz.view(ng, 9, nst, 4, 8, 16).permute(0, 2, 1, 3, 5, 4).contiguous().view(-1)


def bf16dg_eligible(pc, H, W, OH, OW, transposed=False, out_stride=(1, 1), out_offset=(0, 0), in_shift=None):
    """What vsp_conv2d_bf16dg serves (bf16 activations on top): the 2-4 dilation groups of a SMART branch launch with at most 16 channels
    per group over at most 64 input channels."""
    if (transposed or pc.kh != 3 or pc.kw != 3 or pc.stride != 1 or pc.cin % 8 or pc.cin > 64 or pc.cout_g > 16 or W % 8 or (OH, OW) != (H, W)
            or tuple(out_stride) != (1, 1) or tuple(out_offset) != (0, 0) or pc.dil_by_input_quarter or pc.x_group_stride or in_shift is not None):
        return False
    return 1 <= pc.G <= 4 and all(pc.dil[g] in (1, 2, 4, 8) and pc.pad_y[g] == pc.dil[g] and pc.pad_x[g] == pc.dil[g] for g in range(pc.G))


BF16_MODW = tune_env("VSP_BF16_MODW", "1") != "0"   # per-image modulated weights (vsp_modulate_weight_bf16) on the modulated layers of vsp_conv2d_bf16


def bf16_modulated_weight(pc, in_scale):
    """(B sets of bf16(W * style[b]) in the LDS-image order of vsp_conv2d_bf16, byte stride between them): the reference's own fused
    modulated convolution (models/RestoreNet.py:381-383) -- one small launch per layer and batch; the conv kernel then copies its pixels."""
    in_scale = _req(in_scale, "in_scale")
    B = in_scale.shape[0]
    nbytes = lib.vsp_modulate_weight_bf16_bytes(pc.G, pc.cin, pc.cout_g)
    out = torch.empty((B, nbytes // 2), device=in_scale.device, dtype=BF)
    check(lib.vsp_modulate_weight_bf16(_ptr(out), _ptr(pc.w), _ptr(in_scale), B, in_scale.stride(0), pc.G, pc.cin, pc.cout_g, _stream()),
          "modulate_weight")
    return out, nbytes


BF16_DG = tune_env("VSP_BF16_DG", "1") != "0"   # the dilation-group kernel on the launches it serves (G > 1)
BF16_RV = tune_env("VSP_BF16_RV", "1") != "0"   # the row-vector-K kernel on the layers bf16rv_profitable names


def bf16rv_profitable(pc, H, W):
    """Layers where the row-vector-K kernel beats vsp_conv2d_bf16 (tools/bench_bf16rv.py, batch 16: 64 -> 64 at 512^2 x1.53, at 256^2
    x1.51, 64 -> 128 at 128^2 x1.46, 128 -> 128 at 256^2 x1.27, 32 -> 32 at 1024^2 x1.23, 256 -> 256 at 128^2 x1.10; 128 -> 128 at 64^2 x0.83)."""
    if pc.G > 1:   # dilation groups (served, tested, not chosen): every group stages the whole input patch for its few channels -- alone
        return False   # 64 -> 4 x 16 at 512^2 x1.12, 128 -> 4 x 32 at 256^2 x1.03, 256 -> 4 x 64 at 128^2 x0.83; inside configs[2] no gain (400-415 img/s)
    return pc.cin <= 256 and H * W >= 128 * 128


def bf16x3_weight(wp):
    """packed weights (G, 9, Cin, cout_g) fp32 -> [group][chunk][part 2][tap][octet 2][co_pad][8] bf16 with part 0 = bf16(W),
    part 1 = bf16(W - float(bf16(W))) (vsp_conv2d_bf16x3)."""
    ng, T, cin, cout = wp.shape
    nch, co_pad = (cin + 15) // 16, (cout + 31) // 32 * 32
    Wz = wp.new_zeros(ng, T, nch * 16, co_pad)
    Wz[:, :, :cin, :cout] = wp
    hi = Wz.to(torch.bfloat16)
    lo = (Wz - hi.float()).to(torch.bfloat16)
    parts = torch.stack([hi, lo], 0).view(2, ng, T, nch, 2, 8, co_pad).permute(1, 3, 0, 2, 4, 6, 5)
    return parts.contiguous().view(-1)


def pack_weight(weight, groups=1, adjoint=False, flip=False, scale=1.0, out=None):
    """(Cout, Cin, KH, KW) -> [G][KH*KW][Cin][Cout/G] contiguous, times `scale`, taps reversed when `flip`.  `adjoint` (one group):
    the weight of the data gradient, channels exchanged: [KH*KW][i = Cout][o = Cin] (= packing weight.transpose(0, 1)).
    Device weights are packed by vsp_pack_weight_f32 (one launch); the torch expression serves host tensors (layout tests)."""
    cout, cin, kh, kw = weight.shape
    assert cout % groups == 0 and (groups == 1 or not adjoint)
    if weight.is_cuda:
        w = _req(weight.detach().contiguous(), "weight")
        shape = (1, kh * kw, cout, cin) if adjoint else (groups, kh * kw, cin, cout // groups)
        wp = torch.empty(shape, device=w.device, dtype=torch.float32) if out is None else _req(out, "out")   # out: a slice of a group stack
        assert tuple(wp.shape) == shape
        check(lib.vsp_pack_weight_f32(_ptr(wp), _ptr(w), groups, cout // groups, cin, kh, kw, int(adjoint), int(flip), float(scale),
                                      _stream()), "pack_weight")
        return wp
    w = weight * scale if scale != 1.0 else weight
    if flip:
        w = w.flip(2, 3)
    if adjoint:
        w = w.transpose(0, 1)
        cout, cin = cin, cout
    wp = w.reshape(groups, cout // groups, cin, kh * kw).permute(0, 3, 2, 1).contiguous()
    return wp if out is None else out.copy_(wp)


def pack_weight_stack(weights, adjoint=False, flip=False, scale=1.0):
    """One packed weight with a group per entry of `weights` (equal shapes): the dilated branches of one layer."""
    cout, cin, kh, kw = weights[0].shape
    shape = (len(weights), kh * kw, cout, cin) if adjoint else (len(weights), kh * kw, cin, cout)
    wp = torch.empty(shape, device=weights[0].device, dtype=torch.float32)
    for i, w in enumerate(weights):
        pack_weight(w, 1, adjoint, flip, scale, out=wp[i:i + 1])
    return wp


def winograd_eligible(pc, H, W, OH, OW, transposed=False, out_stride=(1, 1), out_offset=(0, 0)):
    """3x3, stride 1, padding = dilation, G = 1 or up to four dilation groups over one shared input, dense output."""
    if transposed or pc.kh != 3 or pc.kw != 3 or pc.stride != 1 or pc.x_group_stride != 0 or not 1 <= pc.G <= 4 or pc.dil_by_input_quarter:
        return False
    if any(pc.pad_y[g] != pc.dil[g] or pc.pad_x[g] != pc.dil[g] or pc.dil[g] not in (1, 2, 4, 8) for g in range(pc.G)):
        return False
    return (OH, OW) == (H, W) and tuple(out_stride) == (1, 1) and tuple(out_offset) == (0, 0)


def winograd_weight(wp):
    """packed weights (G, 9, Cin, cout_g) -> U = G g G^T in the FRAGMENT order of vsp_conv2d_winograd_f32:
    [group][co tile][chunk][wave 8][lane 64][pp 2][mb MB] with position = 2 wave + pp, ci = CK chunk + (lane >> 4),
    co = 16 MB tile + 16 mb + (lane & 15); Cin / cout_g zero-padded to multiples of CK / 16 MB.  Sums in float64, rounded once
    (vsp_winograd_weight_f32: one launch -- a trained weight is transformed again every iteration)."""
    wp = _req(wp, "packed weight")
    ng, cin, cout = wp.shape[0], wp.shape[2], wp.shape[3]
    U = torch.empty(lib.vsp_winograd_weight_floats(ng, cin, cout), device=wp.device, dtype=torch.float32)
    check(lib.vsp_winograd_weight_f32(_ptr(U), _ptr(wp), ng, cin, cout, _stream()), "winograd_weight")
    return U


def winograd4_weight(wp):
    """packed weights (1, 9, Cin, Cout) -> U = G g G^T of F(4x4,3x3) (points 0, +-3/4, +-3/2, inf; fp64 sums rounded once) in the
    fragment order of vsp_conv2d_winograd4_f32 (vsp_winograd4_weight_f32)."""
    wp = _req(wp, "packed weight")
    ng, taps, cin, cout = wp.shape
    if ng != 1 or taps != 9:
        raise RuntimeError("winograd4_weight: one group of 3x3 taps")
    U = torch.empty(lib.vsp_winograd4_weight_floats(cin, cout), device=wp.device, dtype=torch.float32)
    check(lib.vsp_winograd4_weight_f32(_ptr(U), _ptr(wp), cin, cout, _stream()), "winograd4_weight")
    return U


def winograd4f_weight(wp):
    """packed weights (G, 9, Cin, cout_g) -> U = G g G^T of F(4x4,3x3) in the order of vsp_conv2d_winograd4f_f32
    ([group][co / 32][ci / 4][position pair][lane][4], include/vspbfr_hip.h)."""
    wp = _req(wp, "packed weight")
    ng, taps, cin, cout = wp.shape
    if taps != 9:
        raise RuntimeError("winograd4f_weight: 3x3 taps")
    n = lib.vsp_winograd4f_weight_floats(cin, cout)
    U = torch.empty(ng * n, device=wp.device, dtype=torch.float32)
    for g in range(ng):
        check(lib.vsp_winograd4f_weight_f32(_ptr(U[g * n:]), _ptr(wp[g]), cin, cout, _stream()), "winograd4f_weight")
    return U


def _load_tconvw_allow():
    import json
    import os
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "tconv_wino_allow.json")
    if not os.path.exists(path):
        return {}
    with open(path) as f:
        return {k: True for k in json.load(f)}


# the up-convs on the fused Winograd phase kernel: True = the shapes of TCONVW_ALLOW (tconv_wino_allow.json: shape keys where it measured
# >= 5 % faster than the direct launch in the same process, tools/bench_tconv_wino.py; looked up by the exact key -- another batch size
# was not measured and keeps the direct kernel and its bits), "all" = every launch it serves (tests, A/B runs), False = never
TCONV_WINO = True
TCONVW_ALLOW = _load_tconvw_allow()


def tconvw_eligible(pc, transposed=True, in_shift=False, io_bf16=False):
    """What vsp_conv_transpose2d_s2_wino_f32 serves (the entry re-checks, alignment included, and returns VSP_ENOTSUP): the stride-2
    transposed 3x3 conv of one group, fp32, no affine shift, Cin a multiple of 4."""
    return bool(transposed and pc.kh == 3 and pc.kw == 3 and pc.G == 1 and pc.x_group_stride == 0 and not pc.dil_by_input_quarter
                and not in_shift and not io_bf16 and pc.cin % 4 == 0)


def tconvw_weight_host(wp, scale=1.0):
    """Host restatement of vsp_tconvw_weight_f32 on a packed weight (1, 9, Cin, Cout) -> (16, Cin, Cout): the 16 distinct transformed weights of
    the 25 products (g_0 = tap 2, g_1 = tap 2 + tap 0, g_2 = tap 0 on a 2-tap axis), fp64 sums rounded once."""
    w = wp[0].double().reshape(3, 3, wp.shape[2], wp.shape[3]) * torch.tensor(scale, dtype=torch.float32).double()   # (the entry takes a float)
    g = torch.tensor([[0., 0., 1.], [1., 0., 1.], [1., 0., 0.]], dtype=torch.float64)
    u00 = torch.einsum("ik,jl,klco->ijco", g, g, w).reshape(9, *w.shape[2:])
    u01 = torch.einsum("ik,kco->ico", g, w[:, 1])
    u10 = torch.einsum("jl,lco->jco", g, w[1])
    return torch.cat([u00, u01, u10, w[1, 1][None]], 0).float()


def tconvw_weight(wp, scale=1.0):
    """packed weights (1, 9, Cin, Cout) -> the U image of vsp_conv_transpose2d_s2_wino_f32 ([co / 16][ci / 4][quad 4][lane 64][4],
    include/vspbfr_hip.h)."""
    wp = _req(wp, "packed weight")
    ng, taps, cin, cout = wp.shape
    if ng != 1 or taps != 9:
        raise RuntimeError("tconvw_weight: one group of 3x3 taps")
    U = torch.empty(lib.vsp_tconvw_weight_floats(cin, cout), device=wp.device, dtype=torch.float32)
    check(lib.vsp_tconvw_weight_f32(_ptr(U), _ptr(wp), cin, cout, float(scale), _stream()), "tconvw_weight")
    return U


def tconvw_unpack(U, cin, cout):
    """The U image back as (16, Cin, Cout) (tests: the inverse of the fragment order)."""
    ncb, nks = (cout + 15) // 16, (cin + 3) // 4
    u = U.view(ncb, nks, 4, 4, 16, 4).permute(2, 5, 1, 3, 0, 4).reshape(16, nks * 4, ncb * 16)   # [q][e][ks][kq][cb][lr]
    return u[:, :cin, :cout]


def winograd4f_eligible(pc, H, W, OH, OW, transposed=False, out_stride=(1, 1), out_offset=(0, 0), in_shift=None):
    """fused F(4x4,3x3): one group or up to four dilation groups over one shared input, 3x3 / stride 1 / padding = dilation in (1, 2, 4, 8)
    -- dilated groups run on their polyphase sub-images: whole 4x4 tiles in each (H, W multiples of 4 x dilation) --, no affine shift, Cin a
    multiple of 8 up to 512, rows of at least 16 pixels"""
    return (winograd_eligible(pc, H, W, OH, OW, transposed, out_stride, out_offset) and in_shift is None
            and pc.cin % 8 == 0 and pc.cin <= 512 and W >= 16 and all(H % (4 * pc.dil[g]) == 0 and W % (4 * pc.dil[g]) == 0 for g in range(pc.G)))


def winograd4_eligible(pc, H, W, OH, OW, transposed=False, out_stride=(1, 1), out_offset=(0, 0), in_shift=None):
    """F(4x4,3x3) pair of kernels: one group, 3x3 / stride 1 / dilation 1 / padding 1, no affine shift, whole 4x4 tiles"""
    return (winograd_eligible(pc, H, W, OH, OW, transposed, out_stride, out_offset) and pc.G == 1 and pc.dil[0] == 1 and in_shift is None
            and pc.cin % 4 == 0 and H % 4 == 0 and W % 4 == 0)


def conv2d_out_size(H, W, pc):
    d, py, px = pc.dil[0], pc.pad_y[0], pc.pad_x[0]
    oh = (H + 2 * py - d * (pc.kh - 1) - 1) // pc.stride + 1
    ow = (W + 2 * px - d * (pc.kw - 1) - 1) // pc.stride + 1
    return oh, ow


ConvRoute = namedtuple("ConvRoute", "family hint io_bf16 named key")


def conv_route(pc, B, H, W, OH, OW, transposed=False, out_stride=(1, 1), out_offset=(0, 0), in_shift=False, x_dtype=torch.float32,
               out_dtype=None, winograd=None, bf16=None, tile_hint=0, wino_form=0):
    """Which kernel family serves a conv2d_packed launch: pure host logic on plain values (no library call, no device memory), reading the
    tuned tables and module switches at call time.  `in_shift`: whether the launch has one; `out_dtype`: that of the caller's `out`, None
    without one; `winograd` / `bf16` / `tile_hint` / `wino_form`: the caller's (see conv2d_packed).  A family named by the caller on a layer
    its eligibility rule refuses raises.  -> ConvRoute(family, hint, io_bf16, named, key): `family` the launcher and profiler label,
    `hint` the tile_hint it starts with, `io_bf16` bf16 activations, `named` the caller's `winograd` / `bf16` named the family, `key` the
    shape key of the tables.  In order:
    1. tile_hint 0 takes the TUNE entry as a preference (negative hint: the cost model decides where that tile cannot serve the call).
    2. bf16: the caller's `bf16`; None = BF16_CONV on a bf16_eligible, bf16_profitable layer when no Winograd kernel was asked for
       (BF16_CONV "x3": the subset where the split form wins).  "rv" / "dg" -> bf16rv / bf16dg (bf16 activations required, hint = the
       caller's); "x3" -> bf16x3; with bf16 activations and neither a caller's variant nor BF16_FORCE: bf16dg on the dilation-group
       launches it serves (BF16_DG), else bf16rv where eligible and profitable (BF16_RV); else bf16.  hint = the caller's variant, else
       BF16_FORCE, else BF16_TUNE / BF16X3_TUNE (the automatic bf16rv / bf16dg pick their own and keep it for their fall-back to bf16).
    3. Winograd: the caller's `winograd`; None = the WINO table on a winograd_eligible layer without a tile preference.  5 -> wino4f where
       winograd4f_eligible (else a named 5 raises, an unnamed one takes wino), 4 -> wino4 where winograd4_eligible (else wino).
       hint = `wino_form`, the F(2x2) form.
    4. direct, tconv when transposed, with the hint of step 1."""
    key = conv_key(B, pc.cin, H, W, pc, OH, OW) + (",t" if transposed else "") + (",s" if in_shift else "")
    geo = (pc, H, W, OH, OW, transposed, out_stride, out_offset)
    shift = True if in_shift else None
    pref = tile_hint or -_tuned(TUNE, key)
    named = bf16 is not None
    x3 = bf16 == "x3" or (not named and BF16_CONV == "x3")
    if not named:
        bf16 = (bool(BF16_CONV) and not winograd and bf16_eligible(*geo) and bf16_profitable(pc, H, W, OH, OW, transposed) and (
            # split precision: doubled LDS images -- the layers where it beats the tuned fp32 kernels (tools/conv_breakdown.py)
            not x3 or (W >= 32 if transposed else pc.stride == 1 or (pc.stride == 2 and pc.G == 1 and OW >= 32))))
    elif bf16 and not bf16_eligible(*geo):
        raise RuntimeError("conv2d: this layer is not eligible for the bf16 kernel (see bf16_eligible)")
    if bf16:
        io = not x3 and (x_dtype == BF or (ACT_BF16 and out_dtype is None)) and out_dtype in (None, BF)
        if bf16 in ("rv", "dg"):
            if bf16 == "rv" and not bf16rv_eligible(*geo):
                raise RuntimeError("conv2d: this layer is not eligible for the row-vector bf16 kernel (see bf16rv_eligible)")
            if bf16 == "dg" and not bf16dg_eligible(*geo, shift):
                raise RuntimeError("conv2d: this layer is not eligible for the dilation-group bf16 kernel (see bf16dg_eligible)")
            if not io:
                raise RuntimeError("conv2d: bf16='rv' names the row-vector kernel, which reads and writes bf16 activations: pass a bf16 input "
                                   "(and output) or switch ACT_BF16 on")
            return ConvRoute("bf16" + bf16, max(tile_hint, 0), True, True, key)
        own = max(tile_hint, 0)
        hint = own or BF16_FORCE or _tuned(BF16X3_TUNE if x3 else BF16_TUNE, key)
        if x3:
            return ConvRoute("bf16x3", hint, False, named, key)
        if io and not own and not BF16_FORCE:
            if BF16_DG and pc.G > 1 and bf16dg_eligible(*geo, shift):
                return ConvRoute("bf16dg", hint, True, False, key)
            if BF16_RV and bf16rv_eligible(*geo) and bf16rv_profitable(pc, H, W):
                return ConvRoute("bf16rv", hint, True, False, key)
        return ConvRoute("bf16", hint, io, named, key)
    named = winograd is not None
    if not named:
        winograd = not pref and winograd_eligible(*geo) and _tuned(WINO, key, False)
    elif winograd and not winograd_eligible(*geo):
        raise RuntimeError("conv2d: this layer is not eligible for the Winograd kernel (3x3, stride 1, dilation 1, pad 1, G = 1)")
    if winograd == 5:
        if winograd4f_eligible(*geo, shift):
            return ConvRoute("wino4f", wino_form, False, named, key)
        if named:
            raise RuntimeError("conv2d: this launch is not eligible for the fused F(4x4,3x3) kernel (winograd4f_eligible: one group or up to four "
                               "dilation groups over one shared input, 3x3 / stride 1 / padding = dilation in {1, 2, 4, 8}, H and W multiples of "
                               "4 x dilation, no affine shift, Cin % 8 == 0 up to 512, W >= 16)")
    elif winograd == 4 and winograd4_eligible(*geo, shift):
        return ConvRoute("wino4", wino_form, False, named, key)
    if winograd:
        return ConvRoute("wino", wino_form, False, named, key)
    return ConvRoute("tconv" if transposed else "direct", pref, False, False, key)


# ---- one launcher per kernel family: (filled ConvParams, PackedConv, keep-alive list, named, in_scale) -> the family that ran.  Each owns its
# VSP_ENOTSUP (-3) fall-back; a named fused F(4x4), row-vector or dilation-group launch raises instead (the pair and bf16x3 fall back either way).
def _set_weight(p, keep, w):
    keep.append(w)
    p.w = w.data_ptr()


def _force_retry(entry, p):
    """One launch of `entry`; when the variant BF16_FORCE imposes (tuner) does not serve it, another with the library's own choice."""
    rc = entry(p)
    if rc != 0 and BF16_FORCE and p.tile_hint == BF16_FORCE:
        p.tile_hint = 0
        rc = entry(p)
    return rc


def _launch_f32(p, pc, keep, named, in_scale):
    check(lib.vsp_conv2d_f32(C.byref(p), _stream()), "conv2d")
    return "tconv" if p.transposed else "direct"


def _launch_tconv(p, pc, keep, named, in_scale):
    """The up-convs: the fused Winograd phase kernel (vsp_conv_transpose2d_s2_wino_f32, 25 of the 36 products) where TCONV_WINO asks for it --
    True: on the shapes of TCONVW_ALLOW, "all": on every launch it serves -- and the caller named no tile of the direct kernel; else, and on
    VSP_ENOTSUP, the transposed mode of vsp_conv2d_f32."""
    want = TCONV_WINO and p.tile_hint <= 0 and tconvw_eligible(pc, p.transposed, p.in_shift is not None, p.io_bf16) and (
        TCONV_WINO == "all" or (conv_key(p.B, pc.cin, p.H, p.W, pc, p.OH, p.OW) + ",t") in TCONVW_ALLOW)   # (the measured key itself: no batch-8 stand-in)
    if want:
        hint = p.tile_hint
        _set_weight(p, keep, pc.form("tconvw"))
        p.tile_hint = 0
        rc = lib.vsp_conv_transpose2d_s2_wino_f32(C.byref(p), _stream())
        if rc != -3:
            check(rc, "conv_transpose2d_s2_wino")
            return "tconvw"
        p.w, p.tile_hint = pc.w.data_ptr(), hint   # VSP_ENOTSUP (alignment of an operand plane): nothing was written
    return _launch_f32(p, pc, keep, named, in_scale)


def _launch_wino(p, pc, keep, named, in_scale):
    _set_weight(p, keep, pc.form("wino"))
    check(lib.vsp_conv2d_winograd_f32(C.byref(p), _stream()), "conv2d_winograd")
    return "wino"


def _launch_wino4(p, pc, keep, named, in_scale):
    _set_weight(p, keep, pc.form("wino4"))
    nfl = lib.vsp_conv2d_winograd4_work_floats(C.byref(p))
    work = torch.empty(nfl, device=pc.w.device, dtype=torch.float32)   # V = B^T d B in fragment order (2.25 x the input)
    keep.append(work)
    rc = lib.vsp_conv2d_winograd4_f32(C.byref(p), _ptr(work), nfl, _stream())
    if rc == -3:   # VSP_ENOTSUP: alignment of an operand plane -> F(2x2,3x3)
        return _launch_wino(p, pc, keep, named, in_scale)
    check(rc, "conv2d_winograd4")
    return "wino4"


def _launch_wino4f(p, pc, keep, named, in_scale):
    _set_weight(p, keep, pc.form("wino4f"))
    rc = lib.vsp_conv2d_winograd4f_f32(C.byref(p), _stream())
    if rc == -3 and not named:   # VSP_ENOTSUP: alignment of an operand plane -> F(2x2,3x3)
        return _launch_wino(p, pc, keep, named, in_scale)
    check(rc, "conv2d_winograd4f")
    return "wino4f"


def _launch_bf16x3(p, pc, keep, named, in_scale):
    _set_weight(p, keep, pc.form("bf16x3"))
    rc = _force_retry(lambda q: lib.vsp_conv2d_bf16x3(C.byref(q), _stream()), p)
    if rc == -3:   # VSP_ENOTSUP: the doubled LDS images of this shape do not fit (small stride-2 maps) -> the fp32 kernel
        p.w = pc.w.data_ptr()
        return _launch_f32(p, pc, keep, named, in_scale)
    check(rc, "conv2d_bf16x3")
    return "bf16x3"


def _launch_bf16(p, pc, keep, named, in_scale):
    # a modulated layer with bf16 activations (per-sample style, no shift, even rows): the style goes into per-image weights (the
    # reference's fused form) and the kernel's staging becomes a copy (conv_bf16.hip NOSC)
    if (BF16_MODW and p.io_bf16 and p.in_scale_bstride and p.in_shift is None and p.x_group_stride == 0 and p.W % 2 == 0
            and in_scale.dim() == 2 and in_scale.shape == (p.B, p.Cin) and p.x % 4 == 0):
        bw, wbytes = bf16_modulated_weight(pc, in_scale)
        p.in_scale, p.in_scale_bstride, p.w_bstride = None, 0, wbytes
    else:
        bw = pc.form("bf16")
    _set_weight(p, keep, bw)

    def entry(q):
        rc = lib.vsp_conv2d_bf16(C.byref(q), _stream())
        if rc == -3 and q.w_bstride:   # VSP_ENOTSUP: this tile's patch plane is too large for the copy-only staging -> shared weights + style scale
            _set_weight(q, keep, pc.form("bf16"))
            q.w_bstride, q.in_scale, q.in_scale_bstride = 0, in_scale.data_ptr(), q.Cin
            rc = lib.vsp_conv2d_bf16(C.byref(q), _stream())
        return rc
    check(_force_retry(entry, p), "conv2d_bf16")
    return "bf16"


def _launch_bf16rv(p, pc, keep, named, in_scale):
    hint = p.tile_hint
    if not named:   # automatic: the kernel's own variant; `hint` is the one of vsp_conv2d_bf16
        p.tile_hint = 0
    _set_weight(p, keep, pc.form("bf16rv"))
    rc = lib.vsp_conv2d_bf16rv(C.byref(p), _stream())
    if rc == -3 and not named:   # VSP_ENOTSUP: alignment -> vsp_conv2d_bf16
        p.tile_hint = hint
        return _launch_bf16(p, pc, keep, named, in_scale)
    check(rc, "conv2d_bf16rv")
    return "bf16rv"


def _launch_bf16dg(p, pc, keep, named, in_scale):
    _set_weight(p, keep, pc.form("bf16dg"))
    rc = lib.vsp_conv2d_bf16dg(C.byref(p), _stream())   # (no variants: tile_hint is not read)
    if rc == -3 and not named:   # VSP_ENOTSUP: alignment -> vsp_conv2d_bf16
        return _launch_bf16(p, pc, keep, named, in_scale)
    check(rc, "conv2d_bf16dg")
    return "bf16dg"


_LAUNCH = {"direct": _launch_f32, "tconv": _launch_tconv, "wino": _launch_wino, "wino4": _launch_wino4, "wino4f": _launch_wino4f,
           "bf16": _launch_bf16, "bf16x3": _launch_bf16x3, "bf16rv": _launch_bf16rv, "bf16dg": _launch_bf16dg}


def conv2d_packed(x, pc, out=None, out_hw=None, y_coff=0, out_stride=(1, 1), out_offset=(0, 0), in_scale=None,
                  in_scale_per_sample=True, in_shift=None, out_scale=None, ch_scale=None, ch_bias=None, act1=False,
                  bias1=None, noise=None, noise_w=None, act2=0, bias2=None, prelu=None, slope2=0.2, gain2=SQRT2, res1=None,
                  res2=None, res_coff=0, n_out=None, tile_hint=0, transposed=False, winograd=None, bf16=None, wino_form=0):
    """One convolution on the kernel family conv_route picks.  `out` (B, y_ch, y_h, y_w) is allocated when None.  `n_out` = (OH, OW) positions
    to compute (defaults to the standard conv output size).  `winograd`: True / False forces / forbids the F(2x2,3x3) kernel
    (vsp_conv2d_winograd_f32) on an eligible layer, 4 / 5 name the F(4x4,3x3) pair / fused kernel; None = what the tuned table says for this
    shape; `wino_form` names the F(2x2) kernel form (0 automatic, 1 task list, 2 row owner, 3 register-resident U: include/vspbfr_hip.h,
    tests / tuning).  `bf16`: True runs the layer on vsp_conv2d_bf16 (tile_hint = its variant), "x3" / "rv" / "dg" on its split-precision /
    row-vector / dilation-group forms, None = the module switch BF16_CONV on eligible layers."""
    x = _req(x, "x", bf16_ok=True)
    B, x_ch, H, W = x.shape
    Cin = pc.cin
    if (pc.G - 1) * pc.x_group_stride + Cin != x_ch:
        raise RuntimeError(f"conv2d: input has {x_ch} channels, weight expects {(pc.G - 1) * pc.x_group_stride + Cin}")
    OH, OW = n_out if n_out is not None else ((H + 1, W + 1) if transposed else conv2d_out_size(H, W, pc))
    # decided before anything is allocated: the family fixes the activation dtype
    r = conv_route(pc, B, H, W, OH, OW, transposed, out_stride, out_offset, in_shift is not None, x.dtype, None if out is None else out.dtype,
                   winograd, bf16, tile_hint, wino_form)
    act_dt = BF if r.io_bf16 else torch.float32
    x = as_dtype(x, act_dt)
    res1, res2 = as_dtype(res1, act_dt), as_dtype(res2, act_dt)
    if out is None:
        yh, yw = (2 * H + 1, 2 * W + 1) if transposed else (out_hw if out_hw is not None else (OH, OW))
        out = torch.empty((B, pc.cout, yh, yw), device=x.device, dtype=act_dt)
    _req(out, "out", bf16_ok=r.io_bf16)
    if out.dtype != act_dt:
        raise RuntimeError(f"conv2d: `out` is {out.dtype} but this launch writes {act_dt}")
    if B == 0:  # empty batch: nothing to enqueue (an empty tensor has no device pointer to hand to the C ABI)
        return out
    p = ConvParams()
    keep = [x, pc.w, out, _opt(in_scale, "in_scale"), _opt(in_shift, "in_shift"), _opt(out_scale, "out_scale"),
            _opt(ch_scale, "ch_scale"), _opt(ch_bias, "ch_bias"), _opt(bias1, "bias1"), _opt(noise, "noise"),
            _opt(noise_w, "noise_w"), _opt(bias2, "bias2"), _opt(prelu, "prelu"),
            _req(res1, "res1", r.io_bf16) if res1 is not None else None, _req(res2, "res2", r.io_bf16) if res2 is not None else None]
    dp = [(t.data_ptr() if t is not None else None) for t in keep]
    (p.x, p.w, p.y, p.in_scale, p.in_shift, p.out_scale, p.ch_scale, p.ch_bias, p.bias1, p.noise, p.noise_w, p.bias2,
     p.prelu, p.res1, p.res2) = dp
    p.io_bf16 = 1 if r.io_bf16 else 0
    p.B, p.Cin, p.H, p.W = B, Cin, H, W
    p.G, p.cout_g, p.OH, p.OW, p.KH, p.KW = pc.G, pc.cout_g, OH, OW, pc.kh, pc.kw
    p.stride_y = p.stride_x = pc.stride
    for g in range(4):
        p.dil[g], p.pad_y[g], p.pad_x[g] = pc.dil[g], pc.pad_y[g], pc.pad_x[g]
    p.y_ch, p.y_coff, p.y_h, p.y_w = out.shape[1], y_coff, out.shape[2], out.shape[3]
    p.osy, p.osx = out_stride
    p.ooy, p.oox = out_offset
    p.in_scale_bstride = (in_scale.shape[-1] if pc.x_group_stride else Cin) if (in_scale is not None and in_scale_per_sample) else 0
    p.act1, p.slope1, p.gain1 = (1 if act1 else 0), 0.2, SQRT2
    p.act2, p.slope2, p.gain2 = int(act2), float(slope2), float(gain2)
    rt = res1 if res1 is not None else res2
    p.res_ch = rt.shape[1] if rt is not None else 0
    p.res_coff = res_coff
    p.tile_hint = r.hint
    p.x_ch, p.x_group_stride = x_ch, pc.x_group_stride
    p.transposed = 1 if transposed else 0
    p.dil_by_input_quarter = 1 if pc.dil_by_input_quarter else 0
    if RECORDER is not None:
        RECORDER.append((r.key, (B, Cin, H, W, OH, OW), pc, transposed))
    if rt is not None and (rt.shape[0] != B or rt.shape[2] != out.shape[2] or rt.shape[3] != out.shape[3]):
        raise RuntimeError("conv2d: residual must match the output tensor's batch and spatial size")
    prof = PROFILER
    if prof is not None:
        start = prof.begin()
    ran = _LAUNCH[r.family](p, pc, keep, r.named, in_scale)
    if prof is not None:
        es = 2 if r.io_bf16 else 4
        n_out_el = B * pc.cout * ((2 * H + 1) * (2 * W + 1) if transposed else OH * OW)
        nbytes = (x.numel() + n_out_el * (1 + (res1 is not None) + (res2 is not None))) * es + pc.cout * Cin * pc.kh * pc.kw * (
            2 if ran.startswith("bf16") else 4) + (B * OH * OW * 4 if noise is not None else 0)
        prof.end(start, 2.0 * B * pc.cout * (H * W if transposed else OH * OW) * Cin * pc.kh * pc.kw,
                 (Cin, pc.cout, OH, OW, pc.kh, pc.stride, pc.G, ran, r.key), nbytes)
    return out


CONV1X1_SMALL_MAX_P = 1024   # maps up to 32 x 32 (measured to 28 x 28, batch 8: tools/bench_1x1_gemm.py); larger maps amortise the tiled kernel's weight slabs


def conv1x1_small(x, w2d, bias=None, act=False, slope=0.2, gain=SQRT2):
    """y[b, co, p] = act(w2d @ x[b] + bias) for a 1x1 stride-1 conv on a small map (vsp_conv1x1_small_f32); w2d = (Cout, Cin)."""
    x, w2d = _req(x, "x"), _req(w2d, "weight")
    B, cin, Hh, Ww = x.shape
    cout = w2d.shape[0]
    if w2d.shape[1] != cin:
        raise RuntimeError(f"conv1x1_small: input has {cin} channels, weight expects {w2d.shape[1]}")
    y = torch.empty((B, cout, Hh, Ww), device=x.device, dtype=torch.float32)
    check(lib.vsp_conv1x1_small_f32(_ptr(y), _ptr(w2d), _ptr(x), _ptr(_opt(bias, "bias")), B, cout, cin, Hh * Ww, int(bool(act)),
                                    float(slope), float(gain), _stream()), "conv1x1_small")
    return y


def conv2d(x, weight, bias=None, stride=1, padding=0, dilation=1, **epi):
    """F.conv2d-shaped convenience entry (groups=1): packs the weight on the fly (tests, generic callers)."""
    weight = _req(weight, "weight")
    cout, cin, kh, kw = weight.shape
    if (kh == 1 and kw == 1 and stride == 1 and padding == 0 and cin % 16 == 0 and x.dtype == torch.float32 and x.dim() == 4
            and x.shape[2] * x.shape[3] <= CONV1X1_SMALL_MAX_P and not (set(epi) - {"act2", "bias2", "slope2", "gain2"})
            and not (bias is not None and epi.get("bias2") is not None)):
        act = epi.get("act2", 0)
        if act in (0, 1):   # GEMM-shaped: K = Cin against a few hundred columns
            return conv1x1_small(x, weight.view(cout, cin), bias if bias is not None else epi.get("bias2"), act == 1,
                                 epi.get("slope2", 0.2), epi.get("gain2", SQRT2))
    # The packed (and, on a Winograd layer, transformed) weight rides on the tensor object it was built from: a long-lived weight
    # (frozen loss networks, folded BatchNorm weights) is packed once per version, a temporary dies with its packing.
    key = (weight._version, weight.data_ptr(), stride, dilation, padding)
    cached = getattr(weight, "_vsp_packed", None)
    if cached is not None and cached[0] == key:
        pc = cached[1]
    else:
        pc = PackedConv(pack_weight(weight), 1, cout, cin, kh, kw, stride, (dilation,), (padding,))
        try:
            weight._vsp_packed = (key, pc)
        except (AttributeError, RuntimeError):
            pass
    return conv2d_packed(x, pc, ch_bias=bias, **epi)


# transposed conv, stride 2, pad 0, as four sub-pixel phases (include/vspbfr_hip.h, osy/osx/ooy/oox)
def pack_transposed_s2(weight_oihw):
    """weight (Cout, Cin, 3, 3) as stored by ModulatedConv2d (reference models/RestoreNet.py:463-465; the reference
    transposes it to (Cin, Cout, 3, 3) for conv_transpose2d, :527-529).  out[2m+py, 2n+px] only sees taps with
    ky = py (mod 2): phase 0 is a 2-tap correlation [W[2], W[0]] with pad 1 over m = 0..H, phase 1 the single tap W[1]
    over m = 0..H-1.  Returns {(py, px): PackedConv}."""
    cout, cin, kh, kw = weight_oihw.shape
    assert kh == 3 and kw == 3
    sel = {0: [2, 0], 1: [1]}
    phases = {}
    for py in (0, 1):
        for px in (0, 1):
            sub = weight_oihw[:, :, sel[py], :][:, :, :, sel[px]]
            phases[(py, px)] = PackedConv(pack_weight(sub), 1, cout, cin, len(sel[py]), len(sel[px]), 1, (1,),
                                          (1 if py == 0 else 0,), (1 if px == 0 else 0,))
    return phases


def conv_transpose2d_s2_fused(x, pc, **kw):
    """(B, Cin, H, W) -> (B, Cout, 2H+1, 2W+1): conv_transpose2d(stride=2, padding=0), 3x3, in ONE launch (`pc` is the
    ordinary packed 3x3 weight).  Supports in_scale / out_scale / per-channel epilogue terms."""
    return conv2d_packed(x, pc, transposed=True, **kw)


def conv_transpose2d_s2_into(x, pc, out_hw, **kw):
    """The same launch writing into a (B, Cout, OH, OW) tensor with OH in {2H+1, 2H+2} (the data gradient of a stride-2 conv over an
    even-sized input has one zero row / column more): the margin is zeroed here, no padded copy is made."""
    B, _, H, W = x.shape
    OH, OW = out_hw
    if not (0 <= OH - (2 * H + 1) <= 1 and 0 <= OW - (2 * W + 1) <= 1):
        raise RuntimeError("conv_transpose2d_s2_into: out_hw must be (2H+1 or 2H+2, 2W+1 or 2W+2)")
    out = torch.empty((B, pc.cout, OH, OW), device=x.device, dtype=torch.float32)
    if OH > 2 * H + 1:
        out[:, :, -1].zero_()
    if OW > 2 * W + 1:
        out[:, :, :, -1].zero_()
    return conv2d_packed(x, pc, transposed=True, out=out, bf16=False, **kw)


def conv_transpose2d_s2(x, phases, **kw):
    """(B, Cin, H, W) -> (B, Cout, 2H+1, 2W+1): conv_transpose2d(stride=2, padding=0) with a 3x3 kernel, as four
    sub-pixel phase launches (kept as the cross-check of the fused kernel)."""
    B, _, H, W = x.shape
    cout = phases[(0, 0)].cout
    out = torch.empty((B, cout, 2 * H + 1, 2 * W + 1), device=x.device, dtype=x.dtype)
    for (py, px), pc in phases.items():
        conv2d_packed(x, pc, out=out, out_stride=(2, 2), out_offset=(py, px),
                      n_out=(H + 1 if py == 0 else H, W + 1 if px == 0 else W), **kw)
    return out


# ----------------------------------------------------------------------------------------------- gemm / linear
def gemm_nt(a, b, out=None, alpha=1.0, bias=None, bias_scale=1.0, act=0, slope=0.2, gain=SQRT2, a_strides=None,
            b_strides=None, dims=None, bias_zs=0):
    """C[z,m,n] = epi(alpha * sum_k A[z,m,k] B[z,n,k]).  Default: a [Z?,M,K], b [Z?,N,K] contiguous.
    `a_strides` = (zs, ms, ks), `b_strides` = (zs, ns, ks) and dims = (Z, M, N, K) describe arbitrary views of the
    storage starting at a.data_ptr()/b.data_ptr()."""
    if dims is None:
        if a.dim() == 2:
            a3, b3 = a.unsqueeze(0), b.unsqueeze(0)
        else:
            a3, b3 = a, b
        Z, M, K = a3.shape
        N = b3.shape[1]
        if b3.shape[0] not in (1, Z) or b3.shape[2] != K:
            raise RuntimeError("gemm_nt: shape mismatch")
        a_strides = (a3.stride(0), a3.stride(1), a3.stride(2))
        b_strides = ((b3.stride(0) if b3.shape[0] == Z and Z > 1 else 0), b3.stride(1), b3.stride(2))
        if Z == 1:
            a_strides = (0,) + a_strides[1:]
        out_shape = (M, N) if a.dim() == 2 else (Z, M, N)
    else:
        Z, M, N, K = dims
        out_shape = (Z, M, N)
    for t, nm in ((a, "a"), (b, "b")):
        if not (t.is_cuda and t.dtype == torch.float32):
            raise RuntimeError(f"gemm_nt: {nm} must be a CUDA float32 tensor")
    if out is None:
        out = torch.empty(out_shape, device=a.device, dtype=a.dtype)
    _req(out, "out")
    p = GemmParams()
    p.A, p.Bm, p.C = a.data_ptr(), b.data_ptr(), out.data_ptr()
    p.Z, p.M, p.N, p.K = Z, M, N, K
    p.a_zs, p.a_ms, p.a_ks = a_strides
    p.b_zs, p.b_ns, p.b_ks = b_strides
    p.c_zs, p.c_ms = M * N, N
    p.alpha = alpha
    p.bias = _opt(bias, "bias").data_ptr() if bias is not None else None
    p.bias_scale, p.act, p.slope, p.gain = bias_scale, act, slope, gain
    p.bias_zs = bias_zs
    check(lib.vsp_gemm_f32(C.byref(p), _stream()), "gemm")
    return out


def linear(x, weight, bias=None, alpha=1.0, bias_scale=1.0, act=0):
    """F.linear(x, weight*alpha, bias*bias_scale) (+ fused leaky-relu*sqrt2 when act=1, sigmoid when act=2)."""
    lead = x.shape[:-1]
    if x.dim() == 2 and x.stride(1) == 1 and x.is_cuda and x.dtype == torch.float32:
        x2 = x  # rows may be strided (a slice latent[:, i] of a (B, 18, D) tensor): the GEMM takes the row pitch, no copy
    else:
        x2 = _req(x, "x").reshape(-1, x.shape[-1])
    out = gemm_nt(x2, _req(weight, "weight"), alpha=alpha, bias=bias, bias_scale=bias_scale, act=act)
    return out.view(*lead, weight.shape[0])


# ----------------------------------------------------------------------------------------------- row helpers
def pixelnorm_dim1(x, eps=1e-8):
    x = _req(x, "x")
    if x.dim() == 2:
        Z, R, Cc = 1, x.shape[0], x.shape[1]
        # PixelNorm on (B, D) normalises over dim 1 = D: that is a [B, D, 1] problem
        Z, R, Cc = x.shape[0], x.shape[1], 1
    else:
        Z, R = x.shape[0], x.shape[1]
        Cc = x.numel() // (Z * R) if Z * R else 0
    out = torch.empty_like(x)
    check(lib.vsp_pixelnorm_dim1_f32(_ptr(out), _ptr(x), Z, R, Cc, eps, _stream()), "pixelnorm_dim1")
    return out


def layernorm(x, add=None, gamma=None, beta=None, eps=1e-5, post_lrelu=False):
    x = _req(x, "x")
    cols = x.shape[-1]
    rows = x.numel() // cols
    out = torch.empty_like(x)
    check(lib.vsp_layernorm_f32(_ptr(out), _ptr(x), _ptr(_opt(add, "add")), _ptr(_opt(gamma, "gamma")),
                                _ptr(_opt(beta, "beta")), rows, cols, eps, 1 if post_lrelu else 0, 0.2, SQRT2,
                                _stream()), "layernorm")
    return out


def softmax_lastdim(x):
    x = _req(x, "x")
    cols = x.shape[-1]
    out = torch.empty_like(x)
    check(lib.vsp_softmax_lastdim_f32(_ptr(out), _ptr(x), x.numel() // cols, cols, _stream()), "softmax_lastdim")
    return out


def softmax_dim1(x):
    x = _req(x, "x")
    Z, R = x.shape[0], x.shape[1]
    Cc = x.numel() // (Z * R)
    out = torch.empty_like(x)
    check(lib.vsp_softmax_dim1_f32(_ptr(out), _ptr(x), Z, R, Cc, _stream()), "softmax_dim1")
    return out


def film(h, gamma, beta):
    out = torch.empty_like(_req(h, "h"))
    check(lib.vsp_film_f32(_ptr(out), _ptr(h), _ptr(_req(gamma, "gamma")), _ptr(_req(beta, "beta")), h.numel(),
                           _stream()), "film")
    return out


def axpby_idx(x, y, a, b, idx):
    out = torch.empty_like(_req(x, "x"))
    check(lib.vsp_axpby_idx_f32(_ptr(out), _ptr(x), _ptr(_req(y, "y")), _ptr(_req(a, "a")), _ptr(_req(b, "b")), int(idx),
                                x.numel(), _stream()), "axpby_idx")
    return out


def demod_coefs(style, wsq, wscale, eps=1e-8):
    style, wsq = _req(style, "style"), _req(wsq, "wsq")
    B, Cin = style.shape
    Cout = wsq.shape[0]
    out = torch.empty((B, Cout), device=style.device, dtype=style.dtype)
    check(lib.vsp_demod_f32(_ptr(out), _ptr(style), _ptr(wsq), B, Cin, Cout, wscale, eps, _stream()), "demod")
    return out


def demod_weight(style, weight, wscale, eps=1e-8):
    """(demod (B, Cout), wsq (Cout, Cin)) straight from the weight (..., Cout, Cin, kh, kw): the training form of demod_coefs."""
    style, weight = _req(style, "style"), _req(weight, "weight")
    B, Cin = style.shape
    Cout, K = weight.shape[-4], weight.shape[-1] * weight.shape[-2]
    if weight.shape[-3] != Cin or weight.numel() != Cout * Cin * K:
        raise RuntimeError(f"demod_weight: style {tuple(style.shape)} does not match weight {tuple(weight.shape)}")
    out = torch.empty((B, Cout), device=style.device, dtype=torch.float32)
    wsq = torch.empty((Cout, Cin), device=style.device, dtype=torch.float32)
    check(lib.vsp_demod_weight_f32(_ptr(out), _ptr(wsq), _ptr(style), _ptr(weight), B, Cin, Cout, K, float(wscale), float(eps), _stream()),
          "demod_weight")
    return out, wsq


def demod_weight_bwd(g, out, style, wsq, weight, wscale, need_style=True, need_weight=True, ds_out=None, dw_out=None, accumulate=False):
    """Gradient of a loss through demod_weight's `out`: (dstyle (B, Cin) or None, dweight shaped like weight or None).  `g` and `out` may be
    column windows of wider row-major tensors with the SAME row pitch (slices [:, a:b]).  `ds_out` / `dw_out` + `accumulate`: add the
    result to existing contiguous buffers (the convolution's own style / weight gradient) instead of allocating."""
    style, wsq, weight = _req(style, "style"), _req(wsq, "wsq"), _req(weight, "weight")
    B, Cin = style.shape
    Cout, K = wsq.shape[0], weight.numel() // wsq.numel()
    for t, nm in ((g, "g"), (out, "out")):
        if not (t.is_cuda and t.dtype == torch.float32 and t.dim() == 2 and t.shape == (B, Cout) and t.stride(1) == 1):
            raise RuntimeError(f"demod_weight_bwd: {nm} must be a float32 device (B, Cout) row-major window")
    if g.stride(0) != out.stride(0) and B > 1:
        raise RuntimeError("demod_weight_bwd: g and out must share their row pitch")
    gs = int(g.stride(0)) if B > 1 else Cout
    ds = (ds_out if ds_out is not None else torch.empty_like(style)) if need_style else None
    dw = (dw_out if dw_out is not None else torch.empty_like(weight)) if need_weight else None
    for t, nm, ref in ((ds, "ds_out", style), (dw, "dw_out", weight)):
        if t is not None and not (t.is_contiguous() and t.numel() == ref.numel() and t.dtype == torch.float32 and t.is_cuda):
            raise RuntimeError(f"demod_weight_bwd: {nm} must be a contiguous float32 device tensor with the operand's element count")
    if accumulate and ((need_style and ds_out is None) or (need_weight and dw_out is None)):
        raise RuntimeError("demod_weight_bwd: accumulate needs the buffers to add to")
    check(lib.vsp_demod_weight_bwd_acc_f32(_ptr(ds), _ptr(dw), C.c_void_p(g.data_ptr()), gs, C.c_void_p(out.data_ptr()), _ptr(style), _ptr(wsq),
                                           _ptr(weight), B, Cin, Cout, K, float(wscale), int(bool(accumulate)), _stream()), "demod_weight_bwd")
    return ds, dw


def avgpool2x2(x):
    x = _req(x, "x")
    H, W = x.shape[-2:]
    if H % 2 or W % 2:
        raise RuntimeError("avgpool2x2 needs even spatial dims")
    out = torch.empty(x.shape[:-2] + (H // 2, W // 2), device=x.device, dtype=x.dtype)
    check(lib.vsp_avgpool2x2_f32(_ptr(out), _ptr(x), x.numel() // (H * W), H // 2, W // 2, _stream()), "avgpool2x2")
    return out


def upsample_add(x, y):
    x, y = _req(x, "x"), _req(y, "y")
    IH, IW = x.shape[-2:]
    OH, OW = y.shape[-2:]
    out = torch.empty_like(y)
    check(lib.vsp_upsample_add_f32(_ptr(out), _ptr(x), _ptr(y), y.numel() // (OH * OW), IH, IW, OH, OW, _stream()),
          "upsample_add")
    return out


def e4e_codes(heads, latent_avg=None):
    """(T, B, D) map2style outputs -> (B, T, D) W+ codes: w0 + delta_i (+ latent_avg), one launch."""
    heads = _req(heads, "heads")
    T, B, D = heads.shape
    out = torch.empty((B, T, D), device=heads.device, dtype=torch.float32)
    check(lib.vsp_e4e_codes_f32(_ptr(out), _ptr(heads), _ptr(_opt(latent_avg, "latent_avg")), B, T, D, _stream()), "e4e_codes")
    return out


def rows_concat(B, T, segments):
    """out (B, T, sum widths) from up to three segments (tensor, width, per_token, flip): per_token=True reads tensor[b, t (or T-1-t),
    :width] of a (B, >= T, >= width) contiguous tensor, per_token=False broadcasts tensor[b, :width] over the tokens."""
    n = len(segments)
    keep = [_req(t, "segment") for t, _, _, _ in segments]
    src = (C.c_void_p * n)(*[t.data_ptr() for t in keep])
    bs = (C.c_int * n)(*[t.stride(0) for t in keep])
    ts = (C.c_int * n)(*[(t.stride(1) if per_tok else 0) for (t, _, per_tok, _) in segments])
    wd = (C.c_int * n)(*[int(w) for _, w, _, _ in segments])
    fl = (C.c_int * n)(*[1 if f else 0 for _, _, _, f in segments])
    out = torch.empty((B, T, sum(int(w) for _, w, _, _ in segments)), device=keep[0].device, dtype=torch.float32)
    check(lib.vsp_rows_concat_f32(_ptr(out), B, T, n, src, bs, ts, wd, fl, _stream()), "rows_concat")
    return out


def resize_bilinear(x, size):
    """F.interpolate(x, size, mode="bilinear", align_corners=False) for NCHW fp32."""
    x = _req(x, "x")
    B, Cc, IH, IW = x.shape
    OH, OW = size
    out = torch.empty((B, Cc, OH, OW), device=x.device, dtype=x.dtype)
    check(lib.vsp_resize_bilinear_f32(_ptr(out), _ptr(x), B * Cc, IH, IW, OH, OW, _stream()), "resize_bilinear")
    return out


def resize_bilinear_bwd(dy, in_size):
    """Adjoint of resize_bilinear: gradient w.r.t. the (IH, IW) input."""
    dy = _req(dy, "dy")
    B, Cc, OH, OW = dy.shape
    IH, IW = in_size
    dx = torch.empty((B, Cc, IH, IW), device=dy.device, dtype=dy.dtype)
    check(lib.vsp_resize_bilinear_bwd_f32(_ptr(dx), _ptr(dy), B * Cc, IH, IW, OH, OW, _stream()), "resize_bilinear_bwd")
    return dx


def maxpool2d(x, k, s, p=0):
    """F.max_pool2d(x, k, s, p) (floor mode) for NCHW fp32."""
    x = _req(x, "x")
    B, Cc, H, W = x.shape
    OH, OW = (H + 2 * p - k) // s + 1, (W + 2 * p - k) // s + 1
    out = torch.empty((B, Cc, OH, OW), device=x.device, dtype=x.dtype)
    check(lib.vsp_maxpool2d_f32(_ptr(out), _ptr(x), B * Cc, H, W, OH, OW, k, s, p, _stream()), "maxpool2d")
    return out


def maxpool2d_bwd(dy, x, k, s, p=0):
    x, dy = _req(x, "x"), _req(dy, "dy")
    B, Cc, H, W = x.shape
    OH, OW = dy.shape[-2:]
    dx = torch.empty_like(x)
    check(lib.vsp_maxpool2d_bwd_f32(_ptr(dx), _ptr(dy), _ptr(x), B * Cc, H, W, OH, OW, k, s, p, _stream()), "maxpool2d_bwd")
    return dx


LPIPS_WORK_BLOCKS = 2048                     # include/vspbfr_hip.h VSP_LPIPS_WORK_BLOCKS


def lpips_layer(f0, f1, w):
    """One LPIPS level: (B,) = spatial mean of sum_c w_c (unit(f0) - unit(f1))^2 over NCHW fp32 features."""
    f0, f1, w = _req(f0, "f0"), _req(f1, "f1"), _req(w, "w")
    B, Cc, H, W = f0.shape
    if f1.shape != f0.shape or w.numel() != Cc:
        raise RuntimeError("lpips_layer: f0 / f1 / w shapes do not match")
    out = torch.empty((B,), device=f0.device, dtype=torch.float32)
    work = torch.empty((B * LPIPS_WORK_BLOCKS,), device=f0.device, dtype=torch.float32)   # block sums, added in a fixed order (no atomics)
    check(lib.vsp_lpips_layer_ws_f32(_ptr(out), _ptr(work), work.numel(), _ptr(f0), _ptr(f1), _ptr(w), B, Cc, H * W, _stream()), "lpips_layer")
    return out


def lpips_layer_bwd(gout, f0, f1, w):
    f0, f1, w, gout = _req(f0, "f0"), _req(f1, "f1"), _req(w, "w"), _req(gout, "gout")
    B, Cc, H, W = f0.shape
    df1 = torch.empty_like(f1)
    check(lib.vsp_lpips_layer_bwd_f32(_ptr(df1), _ptr(f0), _ptr(f1), _ptr(w), _ptr(gout), B, Cc, H * W, _stream()), "lpips_layer_bwd")
    return df1


def plane_mean(x):
    x = _req(x, "x")
    B, Cc, H, W = x.shape
    out = torch.empty((B, Cc), device=x.device, dtype=x.dtype)
    check(lib.vsp_plane_mean_f32(_ptr(out), _ptr(x), B * Cc, H * W, _stream()), "plane_mean")
    return out


def scale_add(x, gate, y=None):
    x = _req(x, "x")
    B, Cc, H, W = x.shape
    out = torch.empty_like(x)
    check(lib.vsp_scale_add_f32(_ptr(out), _ptr(x), _ptr(_req(gate, "gate")), _ptr(_opt(y, "y")), B * Cc, H * W,
                                _stream()), "scale_add")
    return out


def subsample(x, s):
    x = _req(x, "x")
    B, Cc, H, W = x.shape
    out = torch.empty((B, Cc, (H - 1) // s + 1, (W - 1) // s + 1), device=x.device, dtype=x.dtype)
    check(lib.vsp_subsample_f32(_ptr(out), _ptr(x), B * Cc, H, W, s, _stream()), "subsample")
    return out


def add3(a, b, c=None):
    out = torch.empty_like(_req(a, "a"))
    check(lib.vsp_add3_f32(_ptr(out), _ptr(a), _ptr(_req(b, "b")), _ptr(_opt(c, "c")), a.numel(), _stream()), "add3")
    return out


# ----------------------------------------------------------------------------------------------- fused TACC step
def tacc_scores(P, eQ, wq_col, tfrac, B, k_off=0):
    score = torch.empty((B, 18, 18), device=P.device, dtype=P.dtype)
    check(lib.vsp_tacc_scores_f32(_ptr(score), _ptr(_req(P, "P")), P.shape[1], k_off, _ptr(_req(eQ, "eQ")),
                                  C.c_void_p(wq_col.data_ptr()), wq_col.stride(0), float(tfrac), B, 18, 512, _stream()),
          "tacc_scores")
    return score


def tacc_chan_attn(P, ek, wk_col, tfrac, B, q2_off=1024, v2_off=1536):
    t = torch.empty((B, 18, 512), device=P.device, dtype=P.dtype)
    check(lib.vsp_tacc_chan_attn_f32(_ptr(t), _ptr(_req(P, "P")), P.shape[1], q2_off, v2_off, _ptr(_req(ek, "ek")),
                                     C.c_void_p(wk_col.data_ptr()), wk_col.stride(0), float(tfrac), B, 18, 512, _stream()),
          "tacc_chan_attn")
    return t


def tacc_tail(P, eQ, wq, tfrac, t, gamma, beta, B, xold=None, c1=None, c2=None, idx=0, k_off=0, v_off=512, want_pn=True):
    """`wq`: the CONTIGUOUS last weight column of the block's q_matrix (512 floats)."""
    y = torch.empty((B, 18, 512), device=P.device, dtype=P.dtype)
    pn = torch.empty_like(y) if want_pn else None
    check(lib.vsp_tacc_tail_f32(_ptr(y), _ptr(pn), _ptr(_req(P, "P")), P.shape[1], k_off, v_off, _ptr(_req(eQ, "eQ")),
                                _ptr(_req(wq, "wq")), float(tfrac), _ptr(_req(t, "t")), _ptr(_req(gamma, "gamma")),
                                _ptr(_req(beta, "beta")), _ptr(_opt(xold, "xold")), _ptr(_opt(c1, "c1")), _ptr(_opt(c2, "c2")),
                                int(idx), B, 18, 512, _stream()), "tacc_tail")
    return y, pn


def tacc_head_pre(e, wcol, ln_w, ln_b, steps, t_div):
    M = e.shape[0]
    out = torch.empty((steps * M, 512), device=e.device, dtype=e.dtype)
    check(lib.vsp_tacc_head_pre_f32(_ptr(out), _ptr(_req(e, "e")), C.c_void_p(wcol.data_ptr()), wcol.stride(0),
                                    _ptr(_req(ln_w, "ln_w")), _ptr(_req(ln_b, "ln_b")), steps, M, 512, float(t_div), _stream()),
          "tacc_head_pre")
    return out


def pointwise(x, w, in_scale=None, ch_bias=None, bias1=None, bias2=None, res=None, up_src=None, up_kernel=None):
    """1x1 convolution with <= 4 channels on one side as an HBM stream (see vsp_pointwise_f32): x (B,Cin,H,W), w (Cout,Cin);
    bias1 / bias2 switch on the two FusedLeakyReLU stages (few-input form), res is added last (few-output form);
    up_src (B,Cout,H/2,W/2) + up_kernel (4,4): the 2x FIR-upsampled skip is evaluated inside the kernel and added."""
    x = _req(x, "x", bf16_ok=True)
    B, Cin, Hh, Ww = x.shape
    Cout = w.shape[0]
    # bf16 on the WIDE side only: few outputs (ToRGB) read bf16 features and write the fp32 image; few inputs (the 3 -> 64 input
    # layer) read the fp32 image and, in the bf16-activation configuration, write bf16 features
    if Cout > 4 and x.dtype == BF:
        x = to_f32(x)
    wide_bf = (x.dtype == BF) if Cout <= 4 else bool(ACT_BF16 and BF16_CONV is True and min(Hh, Ww) >= 32)
    y = torch.empty((B, Cout, Hh, Ww), device=x.device, dtype=BF if (wide_bf and Cout > 4) else torch.float32)
    fn = lib.vsp_pointwise_bf16 if wide_bf else lib.vsp_pointwise_f32
    check(fn(_ptr(y), _ptr(x), _ptr(_req(w, "w")), _ptr(_opt(in_scale, "in_scale")), _ptr(_opt(ch_bias, "ch_bias")),
             _ptr(_opt(bias1, "bias1")), 1 if bias1 is not None else 0, _ptr(_opt(bias2, "bias2")),
             1 if bias2 is not None else 0, _ptr(_opt(res, "res")), _ptr(_opt(up_src, "up_src")),
             _ptr(_opt(up_kernel, "up_kernel")), Ww, B, Cin, Cout, Hh * Ww, _stream()), "pointwise")
    return y


def tacc_chain(x, blocks, steps, coef_idx=None, c1=None, c2=None, t_div=1.0, head_steps=None):
    """Run the whole sampler chain in place on x (B,18,512): for each t in `steps` (host ints, execution order) x <- c1[k] *
    denoiser(x, t) + c2[k] * x with k = coef_idx[s] (default t); c1 = c2 = None: x <- denoiser(x, t).  `blocks`: one dict per
    TACC block with device tensors wcat, eQ, ek, wq, wk, gamma, beta (gamma/beta: (head_steps, B, 18, 512))."""
    from ._lib import TaccBlock, TaccChainParams
    x = _req(x, "x")
    B = x.shape[0]
    n = len(blocks)
    arr = (TaccBlock * n)()
    keep = []
    for i, blk in enumerate(blocks):
        for name in ("wcat", "eQ", "ek", "wq", "wk", "gamma", "beta"):
            t = _req(blk[name], name)
            keep.append(t)
            setattr(arr[i], name, t.data_ptr())
        if blk.get("wcat_frag") is not None:   # optional: the projection matrix in MFMA fragment order (coalesced loads)
            t = _req(blk["wcat_frag"], "wcat_frag")
            if t.numel() != blk["wcat"].numel():
                raise RuntimeError("tacc_chain: wcat_frag must hold the same elements as wcat")
            keep.append(t)
            arr[i].wcat_frag = t.data_ptr()
    if head_steps is None:
        head_steps = blocks[0]["gamma"].shape[0] if n else 0
    nfl = lib.vsp_tacc_chain_work_floats(B)
    work = torch.empty(nfl, device=x.device, dtype=torch.float32)
    steps = [int(s) for s in steps]
    st = (C.c_int * len(steps))(*steps)
    # the C entry checks step[s] as it reaches it, after the earlier steps have been enqueued on x: every step is checked here first, so
    # that a refused call has launched nothing
    for t in (steps if B and n else ()):
        if not 0 <= t < int(head_steps):
            raise RuntimeError(f"tacc_chain: step {t} outside the prepared heads [0, {int(head_steps)})")
    if coef_idx is not None and len(coef_idx) != len(steps):
        raise RuntimeError(f"tacc_chain: coef_idx has {len(coef_idx)} entries for {len(steps)} steps")
    ci = (C.c_int * len(steps))(*[int(k) for k in coef_idx]) if coef_idx is not None else None
    if c1 is not None and c2 is not None:
        # the C entry range-checks `step` against the prepared heads but has no length for the coefficient tables: the kernels read
        # c1[k] / c2[k] wherever k points, so the tables' own length is checked here
        ntab = min(c1.numel(), c2.numel())
        for k in (steps if coef_idx is None else [int(k) for k in coef_idx]):
            if not 0 <= k < ntab:
                raise RuntimeError(f"tacc_chain: coefficient index {k} outside the c1 / c2 tables [0, {ntab})")
    p = TaccChainParams()
    p.B, p.n_tok, p.dim, p.n_blocks = B, 18, 512, n
    p.blocks = arr
    p.x, p.work, p.work_floats = x.data_ptr(), work.data_ptr(), nfl
    p.n_steps, p.step = len(steps), st
    p.coef_idx = ci
    p.c1 = _opt(c1, "c1").data_ptr() if c1 is not None else None
    p.c2 = _opt(c2, "c2").data_ptr() if c2 is not None else None
    p.t_div, p.head_steps = float(t_div), int(head_steps)
    check(lib.vsp_tacc_chain_f32(C.byref(p), _stream()), "tacc_chain")
    return x


def quantize_u8_nhwc(x, lo=-1.0, hi=1.0):
    """(B, C, H, W) fp32 -> (B, H, W, C) uint8 with torchvision's save_image(normalize=True, value_range=(lo, hi)) rounding."""
    x = _req(x, "x")
    B, Cc, Hh, Ww = x.shape
    out = torch.empty((B, Hh, Ww, Cc), device=x.device, dtype=torch.uint8)
    check(lib.vsp_quantize_u8_nhwc(C.c_void_p(out.data_ptr()), _ptr(x), B, Cc, Hh, Ww, float(lo), float(hi), _stream()),
          "quantize_u8_nhwc")
    return out


PAIR_WINDOWS = {"uniform7": 7, "gauss11": 11}      # include/vspbfr_hip.h VSP_WIN_UNIFORM7 / VSP_WIN_GAUSS11


def _req_u8(t, name):
    if not isinstance(t, torch.Tensor):
        raise RuntimeError(f"{name} must be a tensor")
    if not t.is_cuda:
        raise RuntimeError(f"{name} must be a CUDA tensor")
    if t.dtype != torch.uint8:
        raise RuntimeError(f"{name} must be uint8 (got {t.dtype})")
    if not t.is_contiguous():
        raise RuntimeError(f"{name} must be contiguous")
    return t


def pair_stats_u8(a, b, window="gauss11"):
    """a, b: (B, H, W, C) uint8 on one device, C = 1 or 3 -> (sse int64 (B,), ssim float64 (B,)) on that device, on the current
    stream, without synchronising (vsp_pair_stats_u8: exact sum of squared differences; mean SSIM over the valid positions of the
    `uniform7` or `gauss11` window).  The workspace (16 bytes per 32 x 32 tile) comes from torch's caching allocator per call, which
    reuses the block on the stream that used it: calls on different streams never share partial sums."""
    a, b = _req_u8(a, "a"), _req_u8(b, "b")
    if a.device != b.device:
        raise RuntimeError(f"operands on different devices: {a.device} and {b.device}")
    if a.dim() != 4 or a.shape != b.shape:
        raise RuntimeError(f"pair_stats_u8: a and b must be (B, H, W, C) of one shape (got {tuple(a.shape)} and {tuple(b.shape)})")
    if window not in PAIR_WINDOWS:
        raise RuntimeError(f"pair_stats_u8: window must be one of {sorted(PAIR_WINDOWS)} (got {window!r})")
    win = PAIR_WINDOWS[window]
    B, Hh, Ww, Cc = (int(v) for v in a.shape)
    sse = torch.empty(B, device=a.device, dtype=torch.int64)
    ssim = torch.empty(B, device=a.device, dtype=torch.float64)
    work = torch.empty(max(int(lib.vsp_pair_stats_work_bytes(B, Hh, Ww, Cc, win)) // 8, 1), device=a.device, dtype=torch.float64)
    check(lib.vsp_pair_stats_u8(C.c_void_p(sse.data_ptr()), C.c_void_p(ssim.data_ptr()), C.c_void_p(a.data_ptr()), C.c_void_p(b.data_ptr()),
                                B, Hh, Ww, Cc, win, C.c_void_p(work.data_ptr()), _stream()), "pair_stats_u8")
    return sse, ssim


NIQE_BLOCK, NIQE_FEATURES, NIQE_GAMMAS = 96, 36, 9801   # include/vspbfr_hip.h VSP_NIQE_*
_niqe_tables = {}


def niqe_gamma_table():
    """(4, 9801) float64 on the host, rows gamma_k = 0.2 + 0.001 k, r(gamma) = G(2/g)^2 / (G(1/g) G(3/g)), sqrt(G(1/g) / G(3/g)) and
    G(2/g) / G(1/g): what the feature kernel looks its shape parameter up in (vsp_niqe_features_u8 rgam_table).  Pure host code."""
    import math
    rows = ([], [], [], [])
    for k in range(NIQE_GAMMAS):
        g = 0.2 + 0.001 * k
        g1, g2, g3 = math.gamma(1.0 / g), math.gamma(2.0 / g), math.gamma(3.0 / g)
        for row, v in zip(rows, (g, g2 * g2 / (g1 * g3), math.sqrt(g1 / g3), g2 / g1)):
            row.append(v)
    return torch.tensor(rows, dtype=torch.float64)


def niqe_blocks(H, W, crop_border=0):
    """(rows, columns) of 96 x 96 blocks of an H x W image after `crop_border` -- pure host code"""
    return max(H - 2 * crop_border, 0) // NIQE_BLOCK, max(W - 2 * crop_border, 0) // NIQE_BLOCK


def niqe_features_u8(img, crop_border=0, with_moments=False):
    """img: (B, H, W, 3) uint8 -> (features float64 (B, nblk, 36), sharpness float32 (B, nblk)[, moments float64 (B, nblk, 2, 5, 6)])
    on the image's device and the current stream, one launch, without synchronising (vsp_niqe_features_u8; the gamma table is
    built once per device)."""
    img = _req_u8(img, "img")
    if img.dim() != 4 or img.shape[3] != 3:
        raise RuntimeError(f"niqe_features_u8: img must be (B, H, W, 3) uint8 RGB (got {tuple(img.shape)})")
    B, Hh, Ww = (int(v) for v in img.shape[:3])
    crop_border = int(crop_border)
    nby, nbx = niqe_blocks(Hh, Ww, crop_border)
    if crop_border < 0 or nby * nbx < 2:
        raise RuntimeError(f"niqe_features_u8: a {Hh} x {Ww} image with crop_border {crop_border} has fewer than two 96 x 96 blocks")
    table = _niqe_tables.get(img.device)
    if table is None:
        table = _niqe_tables[img.device] = niqe_gamma_table().to(img.device)
    nblk = nby * nbx
    feats = torch.empty(B, nblk, NIQE_FEATURES, device=img.device, dtype=torch.float64)
    sharp = torch.empty(B, nblk, device=img.device, dtype=torch.float32)
    mom = torch.empty(B, nblk, 2, 5, 6, device=img.device, dtype=torch.float64) if with_moments else None
    nwork = int(lib.vsp_niqe_work_bytes(B, Hh, Ww, crop_border))
    work = torch.empty((nwork + 7) // 8, device=img.device, dtype=torch.float64) if nwork else None
    check(lib.vsp_niqe_features_u8(C.c_void_p(feats.data_ptr()), C.c_void_p(mom.data_ptr()) if with_moments else None,
                                   C.c_void_p(sharp.data_ptr()), C.c_void_p(img.data_ptr()), B, Hh, Ww, crop_border,
                                   C.c_void_p(table.data_ptr()), C.c_void_p(work.data_ptr()) if nwork else None, _stream()),
          "niqe_features_u8")
    return (feats, sharp, mom) if with_moments else (feats, sharp)


# ----------------------------------------------------------------------------------------------- keyed random tensors
# segment ids of the path's draws (they enter the Philox counter: a tensor keeps its values whatever else is drawn with it)
SEG_LQ, SEG_XT, SEG_Z = 1, 2, 3           # synthetic LQ batch (bench), x_T (ldm/ddpm.py:423), z (restoration_test.py:77-82; +1: second mixing code)
SEG_GEN, SEG_ENC, SEG_DEC = 16, 48, 80    # + layer index: prior decoder / Restoration_net encoder / decoder NoiseInjection maps


def keyed_fill(shapes, ids, seed, image_index0, dist="normal", device=None, index_tensor=None):
    """[tensor of shape s for s in shapes], every shape = (B, ...) with the same B, all drawn by ONE launch of
    vsp_keyed_fill_f32 into one allocation: value = f(seed, image_index0 + b, id, element).  dist: "normal" | "uniform"
    (-1, 1).  index_tensor: optional device int64 scalar added to image_index0 at run time (graph replays)."""
    shapes = [tuple(int(d) for d in s) for s in shapes]
    if not shapes:
        return []
    B = shapes[0][0]
    if any(s[0] != B for s in shapes) or len(ids) != len(shapes):
        raise RuntimeError("keyed_fill: every tensor needs the same leading batch dimension and one id")
    elems = [math.prod(s[1:]) for s in shapes]
    dev = torch.device(device) if device is not None else torch.device("cuda", torch.cuda.current_device())
    if dev.type != "cuda":
        raise RuntimeError("keyed_fill: CUDA(HIP) device required")
    if index_tensor is not None and (index_tensor.dtype != torch.int64 or not index_tensor.is_cuda or index_tensor.numel() != 1):
        raise RuntimeError("keyed_fill: index_tensor must be a device int64 scalar")
    flat = torch.empty(B * sum(elems), device=dev, dtype=torch.float32)
    n = len(shapes)
    check(lib.vsp_keyed_fill_f32(_ptr(flat), B, (C.c_int64 * n)(*elems), (C.c_int32 * n)(*[int(i) for i in ids]), n,
                                 C.c_uint64(int(seed) & (2 ** 64 - 1)), int(image_index0),
                                 None if index_tensor is None else C.c_void_p(index_tensor.data_ptr()), {"normal": 0, "uniform": 1}[dist],
                                 _stream()), "keyed_fill")
    out, off = [], 0
    for s, e in zip(shapes, elems):
        out.append(flat[off:off + B * e].view(s))
        off += B * e
    return out


# ----------------------------------------------------------------------------------------------- convolution backward
def conv2d_wgrad(x, dy, weight_shape, stride=1, padding=0, dilation=1, groups=1, x_scale=None, dy_scale=None, x_shared=False,
                 dy_coff=0, out=None, accumulate=False, scale=1.0, x_coff=0):
    """dL/dW of y = conv2d(x * x_scale, W, stride, padding, dilation, groups) * dy_scale given dL/dy (vsp_conv2d_wgrad_f32):
    x (B, G*Cin_g, H, W), dy (B, G*Cout_g, OH, OW) -> (G*Cout_g, Cin_g, KH, KW); the scales are optional (B, channels).
    `x_shared`: every group reads the same Cin_g channels of x; `dilation` / `padding` may then be per-group tuples (<= 4 groups: the
    dilated SMART branches in one launch).  `dy_coff` / `x_coff`: first channel of dy / x used (either tensor may hold more channels
    than the layer reads: G*Cout_g of dy, G*Cin_g -- shared: Cin_g -- of x; the scales are indexed by the channels of the whole tensor).
    `scale` multiplies the result (the layer's equalized-lr factor: the gradient of the parameter, not of the scaled weight)."""
    from ._lib import ConvWgradParams
    x, dy = _req(x, "x"), _req(dy, "dy")
    cout, cin_g, kh, kw = (int(v) for v in weight_shape)
    B, xc, H, W = x.shape
    if dy.shape[0] != B or dy.shape[1] < dy_coff + cout or x_coff < 0 or xc < x_coff + (cin_g if x_shared else cin_g * groups) or cout % groups:
        raise RuntimeError(f"conv2d_wgrad: x {tuple(x.shape)} / dy {tuple(dy.shape)} do not match weight {tuple(weight_shape)} with {groups} groups")
    dw = out if out is not None else torch.empty((cout, cin_g, kh, kw), device=x.device, dtype=torch.float32)
    if out is not None and (_req(out, "out").shape != (cout, cin_g, kh, kw)):
        raise RuntimeError("conv2d_wgrad: `out` must be (Cout, Cin_g, KH, KW)")
    p = ConvWgradParams()
    keep = [x, dy, dw, _opt(x_scale, "x_scale"), _opt(dy_scale, "dy_scale")]
    p.x, p.dy, p.dw, p.x_scale, p.dy_scale = [(t.data_ptr() if t is not None else None) for t in keep]
    p.B, p.Cin_g, p.H, p.W, p.G, p.Cout_g = B, cin_g, H, W, groups, cout // groups
    p.OH, p.OW, p.KH, p.KW, p.stride = dy.shape[2], dy.shape[3], kh, kw, int(stride)
    per_group = isinstance(dilation, (tuple, list)) or isinstance(padding, (tuple, list))
    if per_group:
        dl = tuple(dilation) if isinstance(dilation, (tuple, list)) else (dilation,) * groups
        pd = tuple(padding) if isinstance(padding, (tuple, list)) else (padding,) * groups
        if len(dl) != groups or len(pd) != groups or groups > 4:
            raise RuntimeError("conv2d_wgrad: per-group dilation / padding need one value per group, at most 4 groups")
        p.per_group_geometry = 1
        for i in range(groups):
            p.dil_g[i], p.pad_g[i] = int(dl[i]), int(pd[i])
        p.dil, p.pad = int(dl[0]), int(pd[0])
        dilation = dl[0]
    else:
        p.dil, p.pad = int(dilation), int(padding)
    p.x_shared, p.dy_ch, p.dy_coff, p.accumulate = int(bool(x_shared)), dy.shape[1], int(dy_coff), int(bool(accumulate))
    p.x_ch, p.x_coff = xc, int(x_coff)
    p.dw_scale = float(scale)
    # split-K partial sums in private copies of dw (torch's caching allocator: stream-ordered) instead of fp32 atomics
    wf = int(lib.vsp_conv2d_wgrad_work_floats(C.byref(p))) if WGRAD_WORKSPACE else 0
    if wf > 0:
        work = torch.empty((wf,), device=x.device, dtype=torch.float32)
        keep.append(work)
        p.work, p.work_floats = work.data_ptr(), wf
    prof = PROFILER
    start = prof.begin() if prof is not None else None
    check(lib.vsp_conv2d_wgrad_f32(C.byref(p), _stream()), "conv2d_wgrad")
    if prof is not None:
        prof.end(start, 2.0 * B * cout * dy.shape[2] * dy.shape[3] * cin_g * kh * kw,
                 (cin_g, cout // groups, dy.shape[2], dy.shape[3], kh, int(stride), groups, "wgrad", f"d{int(dilation)}"))
    return dw


def plane_dot_scale_(a, b, scale):
    """-> (B, C) = sum over the plane of a * b; `a` (B, C, H, W) is multiplied IN PLACE by scale (B, C)."""
    a, b, scale = _req(a, "a"), _req(b, "b"), _req(scale, "scale")
    if a.shape != b.shape or a.dim() < 3 or scale.numel() != a.shape[0] * a.shape[1]:
        raise RuntimeError("plane_dot_scale_: a, b of the same (B, C, ...) shape and scale (B, C)")
    out = torch.empty(a.shape[:2], device=a.device, dtype=torch.float32)
    planes = a.shape[0] * a.shape[1]
    check(lib.vsp_plane_dot_scale_f32(_ptr(out), _ptr(a), _ptr(b), _ptr(scale), planes, a.numel() // max(planes, 1), _stream()),
          "plane_dot_scale")
    return out


def noise_bias_act(x, noise, noise_w, bias, slope=0.2, gain=SQRT2):
    """lrelu(x + noise_w * noise + bias[c], slope) * gain for x (B, C, H, W), noise (B, 1, H, W), noise_w (1,), bias (C,) or None."""
    x, noise, noise_w = _req(x, "x"), _req(noise, "noise"), _req(noise_w, "noise_w")
    B, Cc, Hh, Ww = x.shape
    if noise.numel() != B * Hh * Ww or noise_w.numel() != 1 or (bias is not None and bias.numel() != Cc):
        raise RuntimeError("noise_bias_act: noise (B, 1, H, W), noise_w (1,), bias (C,)")
    y = torch.empty_like(x)
    check(lib.vsp_noise_bias_act_f32(_ptr(y), _ptr(x), _ptr(noise), _ptr(noise_w), _ptr(_opt(bias, "bias")), B, Cc, Hh * Ww, float(slope),
                                     float(gain), _stream()), "noise_bias_act")
    return y


def noise_dot(gx, noise):
    """(1,) = sum over everything of gx (B, C, H, W) * noise (B, 1, H, W)."""
    gx, noise = _req(gx, "gx"), _req(noise, "noise")
    B, Cc, Hh, Ww = gx.shape
    out = torch.empty((1,), device=gx.device, dtype=torch.float32)
    check(lib.vsp_noise_dot_f32(_ptr(out), _ptr(gx), _ptr(noise), B, Cc, Hh * Ww, _stream()), "noise_dot")
    return out


def smart_tail_bwd(g, y, noise, noise_w, bias2, slope=0.2, gain=SQRT2):
    """Backward of FusedLeakyReLU(bias1) -> NoiseInjection -> FusedLeakyReLU(bias2) from the final output y (vsp_smart_tail_bwd_f32):
    returns (g1 = gradient entering the conv, d bias1 (C,), d bias2 (C,), d noise_weight (1,))."""
    g, y, noise = _req(g, "g"), _req(y, "y"), _req(noise, "noise")
    B, Cc, Hh, Ww = g.shape
    g1 = torch.empty_like(g)
    sums = torch.empty(2 * Cc + 1, device=g.device, dtype=torch.float32)
    check(lib.vsp_smart_tail_bwd_f32(_ptr(g1), _ptr(sums), C.c_void_p(sums.data_ptr() + 4 * Cc), C.c_void_p(sums.data_ptr() + 8 * Cc),
                                     _ptr(g), _ptr(y), _ptr(noise), _ptr(_req(noise_w, "noise_w")), _ptr(_req(bias2, "bias2")), B, Cc,
                                     Hh * Ww, float(slope), float(gain), _stream()), "smart_tail_bwd")
    return g1, sums[:Cc], sums[Cc:2 * Cc], sums[2 * Cc:]


def channel_sum(x):
    """(B, C, ...) -> (C,): sum over the batch and everything behind the channel dimension (bias gradients)."""
    x = _req(x, "x")
    if x.dim() < 2:
        raise RuntimeError("channel_sum: (B, C, ...) tensor")
    B, Cc = x.shape[0], x.shape[1]
    out = torch.empty((Cc,), device=x.device, dtype=torch.float32)
    check(lib.vsp_channel_sum_f32(_ptr(out), _ptr(x), B, Cc, x.numel() // max(B * Cc, 1), _stream()), "channel_sum")
    return out


def plane_dot(a, b):
    """(B, C, H, W) x (B, C, H, W) -> (B, C): sum over the plane of a * b."""
    a, b = _req(a, "a"), _req(b, "b")
    if a.shape != b.shape or a.dim() < 3:
        raise RuntimeError("plane_dot: two tensors of the same (B, C, ...) shape")
    out = torch.empty(a.shape[:2], device=a.device, dtype=torch.float32)
    planes = a.shape[0] * a.shape[1]
    check(lib.vsp_plane_dot_f32(_ptr(out), _ptr(a), _ptr(b), planes, a.numel() // max(planes, 1), _stream()), "plane_dot")
    return out

# ----------------------------------------------------------------------------------------------- training degradations
# Thin wrappers of the vsp_degrade_* stages (csrc/degrade.hip).  `items` is a device uint8 tensor holding n vsp_degrade_item structs and
# `taps` a device fp32 tensor, both uploaded by vspbfr_amd.degrade.DegradePlan, which also sizes the ragged buffers passed here.
def _u8(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.uint8 or not t.is_contiguous():
        raise RuntimeError(f"{name} must be a contiguous CUDA uint8 tensor")
    return t


def degrade_gt(hwc=None, src=None, grey=None, out=None):
    """(B, H, W, 3) uint8 -> (B, 3, H, W) fp32 / 255, or (B, 3, H, W) fp32 -> out (may be src itself); grey: device int32 (B,) flags of
    the images to turn grey (cv2 BGR2GRAY weights)."""
    if (hwc is None) == (src is None):
        raise RuntimeError("degrade_gt: exactly one of hwc / src")
    if hwc is not None:
        _u8(hwc, "hwc")
        if hwc.dim() != 4 or hwc.shape[3] != 3:
            raise RuntimeError("degrade_gt: hwc must be (B, H, W, 3)")
        B, Hh, Ww = hwc.shape[:3]
    else:
        _req(src, "src")
        if src.dim() != 4 or src.shape[1] != 3:
            raise RuntimeError("degrade_gt: src must be (B, 3, H, W)")
        B, Hh, Ww = src.shape[0], src.shape[2], src.shape[3]
    if out is None:
        out = torch.empty((B, 3, Hh, Ww), device=(hwc if hwc is not None else src).device, dtype=torch.float32)
    elif tuple(_req(out, "out").shape) != (B, 3, Hh, Ww):
        raise RuntimeError("degrade_gt: out shape")
    if grey is not None and (not grey.is_cuda or grey.dtype != torch.int32 or grey.numel() != B):
        raise RuntimeError("degrade_gt: grey must be a CUDA int32 tensor of B flags")
    check(lib.vsp_degrade_gt_f32(_ptr(out), _ptr(hwc), _ptr(src), _ptr(grey), B, Hh, Ww, _stream()), "degrade_gt")
    return out


def degrade_blur(gt, taps, items, n):
    """(B, 3, H, W) -> (n, 3, H, W): item i = gt[src_i] correlated with its taps (reflect-101), haze where flagged."""
    gt, taps = _req(gt, "gt"), _req(taps, "taps")
    B, _, Hh, Ww = gt.shape
    out = torch.empty((n, 3, Hh, Ww), device=gt.device, dtype=torch.float32)
    check(lib.vsp_degrade_blur_f32(_ptr(out), _ptr(gt), _ptr(taps), _ptr(_u8(items, "items")), n, B, Hh, Ww, _stream()), "degrade_blur")
    return out


def degrade_down(blurred, items, n, lq_elems, max_pixels, seed, step, noise=None, pre=False):
    """(n, 3, H, W) -> ragged uint8 (lq_elems,) of resized + noisy + rounded images; with pre=True also the fp32 resized values before
    the noise (ragged (dh, dw, 3) per item).  noise: injected ragged fp32 (lq_elems,) or None for the keyed Philox draw."""
    blurred = _req(blurred, "blurred")
    lq = torch.empty(lq_elems, device=blurred.device, dtype=torch.uint8)
    pre_t = torch.empty(lq_elems, device=blurred.device, dtype=torch.float32) if pre else None
    if noise is not None and (_req(noise, "noise").numel() != lq_elems):
        raise RuntimeError("degrade_down: noise must hold lq_elems values")
    check(lib.vsp_degrade_down_u8(_ptr(lq), _ptr(pre_t), _ptr(blurred), _ptr(noise), _ptr(_u8(items, "items")), n, blurred.shape[2],
                                  blurred.shape[3], max_pixels, C.c_uint64(int(seed) & (2 ** 64 - 1)), int(step), _stream()),
          "degrade_down")
    return (lq, pre_t) if pre else lq


def degrade_jpeg(lq, items, n, total_mcus, work_bytes, max_pixels):
    """In place: the JPEG round trip of every item of the ragged uint8 image buffer."""
    work = torch.empty(max(int(work_bytes), 1), device=lq.device, dtype=torch.uint8)
    check(lib.vsp_degrade_jpeg_u8(_ptr(_u8(lq, "lq")), _ptr(work), _ptr(_u8(items, "items")), n, total_mcus, max_pixels, _stream()),
          "degrade_jpeg")
    return lq


def degrade_up(lq, items, n, Hh, Ww):
    """ragged uint8 -> (n, 3, H, W) fp32 multiples of 1/255 (grey where flagged)."""
    out = torch.empty((n, 3, Hh, Ww), device=lq.device, dtype=torch.float32)
    check(lib.vsp_degrade_up_f32(_ptr(out), _ptr(_u8(lq, "lq")), _ptr(_u8(items, "items")), n, Hh, Ww, _stream()), "degrade_up")
    return out

# ----------------------------------------------------------------------------------------------- device-side ingest
def lanczos_resize_u8(plan, items, coef, src, u8=True, f32=False):
    """Pillow-exact LANCZOS resize + crop of one ragged batch (vsp_lanczos_resize_u8, csrc/resample.hip).  plan: the
    vspbfr_amd.resample.ResamplePlan whose sections `items`, `coef`, `src` (device uint8 tensors, ResamplePlan.pack's layout) were
    uploaded.  Returns (u8 (n, H, W, 3) uint8 or None, f32 (n, 3, H, W) fp32 or None) on the current stream."""
    import ctypes as Ct
    _u8(items, "items"), _u8(coef, "coef"), _u8(src, "src")
    if not (u8 or f32):
        raise RuntimeError("lanczos_resize_u8: no output asked for")
    if plan.ragged:
        raise RuntimeError("lanczos_resize_u8: a plan with out_sizes goes through lanczos_resize_ragged_u8")
    if items.numel() != Ct.sizeof(plan.items) or coef.numel() != 4 * plan.coef_ints or src.numel() != plan.src_bytes:
        raise RuntimeError("lanczos_resize_u8: the device sections do not have the plan's sizes")
    n, Hh, Ww = plan.n, plan.H, plan.W
    out8 = torch.empty((n, Hh, Ww, 3), device=src.device, dtype=torch.uint8) if u8 else None
    outf = torch.empty((n, 3, Hh, Ww), device=src.device, dtype=torch.float32) if f32 else None
    work = torch.empty(max(plan.work_bytes // 4, 1), device=src.device, dtype=torch.int32)
    check(lib.vsp_lanczos_resize_u8(_ptr(out8), _ptr(outf), _ptr(src), plan.src_bytes, _ptr(coef), plan.coef_ints, _ptr(work),
                                    plan.work_bytes, Ct.cast(plan.items, Ct.c_void_p), _ptr(items), n, Hh, Ww, _stream()),
          "lanczos_resize_u8")
    return out8, outf


def lanczos_resize_ragged_u8(plan, items, coef, src, dst, out):
    """Pillow-exact LANCZOS resize of a batch whose items each have a window of their own (vsp_lanczos_resize_ragged_u8,
    csrc/resample.hip).  plan: a vspbfr_amd.resample.ResamplePlan built with out_sizes, whose sections `items`, `coef`, `dst` (device
    uint8 tensors, ResamplePlan.pack's layout) were uploaded; src: the source bytes on the device; out: a flat uint8 device tensor.
    Item i's (H_i, W_i, 3) window is written at its out_off of `out`, on the current stream; the other bytes of `out` are left alone.
    Returns out."""
    import ctypes as Ct
    from .resample import ResampleDst, ResampleItem
    _u8(items, "items"), _u8(coef, "coef"), _u8(src, "src"), _u8(dst, "dst"), _u8(out, "out")
    if not plan.ragged:
        raise RuntimeError("lanczos_resize_ragged_u8: the plan has no out_sizes")
    n = plan.nk
    if (items.numel() != n * Ct.sizeof(ResampleItem) or dst.numel() != n * Ct.sizeof(ResampleDst) or coef.numel() != 4 * plan.coef_ints
            or src.numel() != plan.src_bytes or out.dim() != 1):
        raise RuntimeError("lanczos_resize_ragged_u8: the device sections do not have the plan's sizes")
    if len({t.device for t in (items, coef, src, dst, out)}) != 1:
        raise RuntimeError("lanczos_resize_ragged_u8: the sections, the source and the output must be on one device")
    work = torch.empty(max(plan.work_bytes // 4, 1), device=src.device, dtype=torch.int32)
    check(lib.vsp_lanczos_resize_ragged_u8(_ptr(out), out.numel(), _ptr(src), plan.src_bytes, _ptr(coef), plan.coef_ints, _ptr(work),
                                           plan.work_bytes, Ct.cast(plan.items, Ct.c_void_p), _ptr(items), Ct.cast(plan.dst, Ct.c_void_p),
                                           _ptr(dst), n, _stream()), "lanczos_resize_ragged_u8")
    return out


def png_encode(u8, guard=0):
    """Row filters + deflate of a (B, H, W, C) uint8 batch on the current stream (vsp_png_encode_u8, csrc/png.hip; C = 3 or 1).  Returns
    (out (B, capacity + guard) uint8, seg_bytes (B, nseg) int32, seg_adler (B, nseg, 2) int32 bit patterns of uint32, slot): image i's
    segment k is out[i, k * slot : k * slot + seg_bytes[i, k]]; vspbfr_amd.png.assemble turns them into files.  guard: extra bytes behind
    every image's capacity that the kernel must leave alone (tests).  A shape above the header's limits raises NotImplementedError."""
    _u8(u8, "u8")
    if u8.dim() != 4:
        raise RuntimeError("png_encode: u8 must be (B, H, W, C)")
    B, Hh, Ww, Cc = u8.shape
    if Cc not in (1, 3) or B < 1 or Hh < 1 or Ww < 1:
        raise RuntimeError(f"png_encode: shape {tuple(u8.shape)}")
    cap, slot = lib.vsp_png_bound(Hh, Ww, Cc), lib.vsp_png_segment_bound(8, Ww, Cc)
    if cap == 0 or B > 65535:
        raise NotImplementedError(f"png_encode: shape {tuple(u8.shape)} above the limits of vsp_png_encode_u8")
    if guard % 4:
        raise RuntimeError("png_encode: guard must be a multiple of 4")
    nseg = (Hh + 7) // 8
    out = torch.full((B, cap + guard), 0xA5, device=u8.device, dtype=torch.uint8) if guard else torch.empty((B, cap), device=u8.device,
                                                                                                       dtype=torch.uint8)
    seg_bytes = torch.empty((B, nseg), device=u8.device, dtype=torch.int32)
    seg_adler = torch.empty((B, nseg, 2), device=u8.device, dtype=torch.int32)
    check(lib.vsp_png_encode_u8(_ptr(out), cap + guard, _ptr(seg_bytes), _ptr(seg_adler), _ptr(u8), B, Hh, Ww, Cc, _stream()), "png_encode")
    return out, seg_bytes, seg_adler, slot


PNG_RAGGED_SEG_BYTES = 24576                  # include/vspbfr_hip.h VSP_PNG_RAGGED_SEG_BYTES
PNG_RAGGED_SLOT_BYTES = 24588                 # VSP_PNG_RAGGED_SLOT_BYTES
PNG_RAGGED_MAX_ROW_BYTES = 1 << 20            # VSP_PNG_RAGGED_MAX_ROW_BYTES
PNG_RAGGED_MAX_IMAGES = 4096
PNG_RAGGED_MAX_SEGMENTS = 65535
PNG_LIMIT_BYTES = 1 << 31                     # a buffer of this size or more: VSP_ENOTSUP


def png_ragged_layout(sizes, offsets=None, C=3):
    """What one vsp_png_encode_ragged_u8 call over packed (h, w, C) images of `sizes` = [(h, w), ...] at the byte `offsets` of the source
    buffer (default: back to back) needs: (rows, out_bytes, work_bytes, segments) -- per image the vsp_png_item fields (src_off, out_off,
    h, w, seg0, row0) with the payloads at 16-byte boundaries of `out`.  None when a size helper refuses a size.  The one place the Python
    side works this out: png_encode_ragged and png.ragged_serves both ask here."""
    rows, src, out, segs, nrows = [], 0, 0, 0, 0
    for i, (h, w) in enumerate(sizes):
        h, w = int(h), int(w)
        nseg = lib.vsp_png_ragged_segments(h, w, C)
        if nseg == 0:
            return None
        off = src if offsets is None else int(offsets[i])
        rows.append((off, out, h, w, segs, nrows))
        src, out = off + C * h * w, out + (lib.vsp_png_ragged_image_bound(h, w, C) + 15) // 16 * 16
        segs, nrows = segs + nseg, nrows + h
    return rows, out, lib.vsp_png_ragged_work_bytes(segs, nrows), segs


def png_encode_ragged(buffer, sizes, offsets=None, C=3, guard=0):
    """Row filters + deflate of packed (h, w, C) uint8 images of any width on the current stream (vsp_png_encode_ragged_u8,
    csrc/png.hip).  buffer: 1-D uint8 device tensor; image i lies at byte offsets[i] (default: back to back), any alignment.  Returns
    (out uint8, idat_bytes (n,) int32, seg_adler (segments, 2) int32 bit patterns of uint32, out_offsets, work, layout): image i's zlib
    payload is out[out_offsets[i] : out_offsets[i] + idat_bytes[i]]; vspbfr_amd.png.assemble_ragged frames it.  work holds the slots, the
    segment sizes and the filter types as the header lays them out (tests read them); layout = (rows, out_bytes, work_bytes, segments).
    guard: every payload's range is lengthened by this many bytes the kernels must leave alone, and `out` is pre-filled with 0xA5
    (tests).  Nothing is synchronised: the item table goes up from pinned memory on the current stream.  Wrong arguments raise
    RuntimeError (the entry's message); a call above the header's limits raises NotImplementedError."""
    import ctypes as Ct
    from ._lib import PngItem
    _u8(buffer, "buffer")
    n = len(sizes)
    if buffer.dim() != 1 or (offsets is not None and len(offsets) != n):
        raise RuntimeError("png_encode_ragged: a flat buffer, and one offset per size")
    dev = buffer.device
    if n == 0:
        return (torch.empty(0, device=dev, dtype=torch.uint8), torch.empty(0, device=dev, dtype=torch.int32),
                torch.empty((0, 2), device=dev, dtype=torch.int32), [], torch.empty(0, device=dev, dtype=torch.uint8), ([], 0, 0, 0))
    if any(int(h) < 1 or int(w) < 1 for h, w in sizes) or C not in (1, 3):
        raise RuntimeError(f"png_encode_ragged: sizes {list(sizes)}, {C} channels")
    layout = png_ragged_layout(sizes, offsets, C)
    if layout is None:
        raise NotImplementedError(f"png_encode_ragged: sizes {list(sizes)} above the limits of vsp_png_encode_ragged_u8")
    rows, out_bytes, work_bytes, segs = layout
    if guard:
        rows = [(r[0], r[1] + i * guard) + r[2:] for i, r in enumerate(rows)]
        out_bytes += n * guard
        layout = (rows, out_bytes, work_bytes, segs)
    if max(buffer.numel(), out_bytes, work_bytes) >= PNG_LIMIT_BYTES or n > PNG_RAGGED_MAX_IMAGES or segs > PNG_RAGGED_MAX_SEGMENTS:
        raise NotImplementedError(f"png_encode_ragged: {n} images, {segs} segments, buffers of {buffer.numel()}, {out_bytes} and {work_bytes} "
                                  "bytes reach the limits of vsp_png_encode_ragged_u8")
    table = torch.empty(n * Ct.sizeof(PngItem), dtype=torch.uint8, pin_memory=True)
    items = (PngItem * n).from_address(table.data_ptr())
    for i, row in enumerate(rows):
        items[i] = PngItem(*row)
    out = torch.full((out_bytes,), 0xA5, device=dev, dtype=torch.uint8) if guard else torch.empty(out_bytes, device=dev, dtype=torch.uint8)
    work = torch.empty(work_bytes, device=dev, dtype=torch.uint8)
    idat = torch.empty(n, device=dev, dtype=torch.int32)
    seg_adler = torch.empty((segs, 2), device=dev, dtype=torch.int32)
    items_dev = table.to(dev, non_blocking=True)
    rc = lib.vsp_png_encode_ragged_u8(_ptr(out), out_bytes, _ptr(idat), _ptr(seg_adler), _ptr(work), work_bytes, _ptr(buffer), buffer.numel(),
                                      Ct.c_void_p(table.data_ptr()), _ptr(items_dev), n, C, _stream())
    if rc == -3:
        raise NotImplementedError(_lib.last_error())
    check(rc, "png_encode_ragged")
    return out, idat, seg_adler, [r[1] for r in rows], work, layout


JPEG_SUBSAMPLING = {"444": 0, "420": 2}      # include/vspbfr_hip.h VSP_JPEG_444 / VSP_JPEG_420 (Pillow's numbers)
JPEG_LIMIT_BYTES = 1 << 31                    # a buffer of this size or more: VSP_ENOTSUP


def jpeg_layout(sizes, subsampling="420", restart=8):
    """What one vsp_jpeg_encode_u8 call over packed images of `sizes` = [(h, w), ...] needs: (rows, src_bytes, out_bytes, work_bytes,
    intervals) -- per image the vsp_jpeg_item fields (src_off, out_off, h, w, interval0), the images back to back in `src` and every
    segment at a 16-byte boundary of `out`; the three buffer sizes; the number of restart intervals.  None when the entry refuses a size
    (h or w outside 1..65535).  The one place the Python side works this out: jpeg_encode and jpeg.kernel_serves both ask here."""
    sub, restart = JPEG_SUBSAMPLING[subsampling], int(restart)
    mcu = 16 if sub == JPEG_SUBSAMPLING["420"] else 8
    rows, src, out, total, max_mcus = [], 0, 0, 0, 0
    for h, w in sizes:
        h, w = int(h), int(w)
        nint = lib.vsp_jpeg_intervals(h, w, restart, sub)
        if nint == 0:
            return None
        max_mcus = max(max_mcus, -(-h // mcu) * -(-w // mcu))
        rows.append((src, out, h, w, total))
        src, out, total = src + 3 * h * w, out + (lib.vsp_jpeg_image_bound(h, w, restart, sub) + 15) // 16 * 16, total + nint
    work = total * lib.vsp_jpeg_interval_bound(min(restart, max_mcus), sub) if rows else 0
    return rows, src, out, work, total


def jpeg_encode(buffer, sizes, quality=90, subsampling="420", restart=8):
    """Entropy-coded JPEG segments of packed RGB images on the current stream (vsp_jpeg_encode_u8, csrc/jpeg.hip).  buffer: 1-D uint8
    device tensor holding the (h, w, 3) images of `sizes` = [(h, w), ...] back to back.  Returns (out uint8, totals (n,) int32, offsets):
    image i's segment is out[offsets[i] : offsets[i] + totals[i]]; vspbfr_amd.jpeg.assemble frames it.  Nothing is synchronised: the
    item table goes up from pinned memory on the current stream, as degrade.py and resample.py send theirs.  Wrong arguments raise
    RuntimeError (the entry's message); a call that needs a buffer of 2 GiB or more raises NotImplementedError."""
    import ctypes as Ct
    from ._lib import JpegItem
    _u8(buffer, "buffer")
    if subsampling not in JPEG_SUBSAMPLING:
        raise RuntimeError(f"jpeg_encode: subsampling {subsampling!r} ('444' or '420')")
    sub, quality, restart, n = JPEG_SUBSAMPLING[subsampling], int(quality), int(restart), len(sizes)
    layout = jpeg_layout(sizes, subsampling, restart)
    if layout is None:
        raise RuntimeError(f"jpeg_encode: sizes {list(sizes)}, quality {quality}, subsampling {subsampling!r}, restart {restart}")
    rows, src_bytes, out_bytes, work_bytes, total = layout
    if buffer.dim() != 1 or buffer.numel() != src_bytes:
        raise RuntimeError(f"jpeg_encode: a flat buffer of {src_bytes} bytes for these sizes, got {tuple(buffer.shape)}")
    if n == 0:
        return torch.empty(0, device=buffer.device, dtype=torch.uint8), torch.empty(0, device=buffer.device, dtype=torch.int32), []
    if max(src_bytes, out_bytes, work_bytes) >= JPEG_LIMIT_BYTES:
        raise NotImplementedError(f"jpeg_encode: buffers of {src_bytes}, {out_bytes} and {work_bytes} bytes reach the limit of "
                                  "vsp_jpeg_encode_u8")
    dev = buffer.device
    table = torch.empty(n * Ct.sizeof(JpegItem), dtype=torch.uint8, pin_memory=True)
    items = (JpegItem * n).from_address(table.data_ptr())
    for i, row in enumerate(rows):
        items[i] = JpegItem(*row, 0)
    out = torch.empty(out_bytes, device=dev, dtype=torch.uint8)
    work = torch.empty(work_bytes, device=dev, dtype=torch.uint8)
    ws = torch.empty(2 * total, device=dev, dtype=torch.int32)
    totals = torch.empty(n, device=dev, dtype=torch.int32)
    items_dev = table.to(dev, non_blocking=True)
    rc = lib.vsp_jpeg_encode_u8(_ptr(out), out_bytes, _ptr(totals), _ptr(work), work_bytes, _ptr(ws), _ptr(buffer), src_bytes,
                                Ct.c_void_p(table.data_ptr()), _ptr(items_dev), n, quality, sub, restart, _stream())
    if rc == -3:
        raise NotImplementedError(_lib.last_error())
    check(rc, "jpeg_encode")
    return out, totals, [row[1] for row in rows]


JPEG_DEC_TABLE_BYTES = 1824                  # include/vspbfr_hip.h VSP_JPEG_DEC_TABLE_BYTES: 3 x 64 quantisers + 6 x (16 BITS + 256 HUFFVAL)
JPEG_DEC_SUB_BYTES = 256                     # default subsequence length, from the sweep of tools/bench_jpeg_decode.py
JPEG_DEC_MAX_SCAN_BYTES = 0x0FFFFFFF


def jpeg_decode_layout(specs, sub_bytes=JPEG_DEC_SUB_BYTES):
    """What one vsp_jpeg_decode_u8 call over `specs` = [(in_off, in_len, h, w, subsampling number, restart), ...] needs: (rows, out_bytes,
    work_bytes) -- per image the vsp_jpeg_dec_item fields with the images back to back in `out`.  None when the entry refuses a spec."""
    rows, out, work, intervals = [], 0, 0, 0
    for in_off, in_len, h, w, sub, restart in specs:
        need = lib.vsp_jpeg_decode_work_bytes(h, w, in_len, sub, restart, sub_bytes)
        if need == 0:
            return None
        rows.append((in_off, out, work, in_len, h, w, sub, restart, intervals))
        m = 16 if sub == JPEG_SUBSAMPLING["420"] else 8
        mcus = -(-h // m) * -(-w // m)
        out, work, intervals = out + 3 * h * w, work + need, intervals + (-(-mcus // restart) if restart else 1)
    return rows, out, work


def jpeg_decode(comp, specs, tables, sub_bytes=None, out=None, out_offsets=None, want_rounds=False):
    """Baseline JPEG scans -> packed RGB images on the current stream (vsp_jpeg_decode_u8, csrc/jpeg_decode.hip).  comp: 1-D uint8 device
    tensor of entropy-coded bytes; specs: [(in_off, in_len, h, w, subsampling number, restart), ...]; tables: n x JPEG_DEC_TABLE_BYTES
    uint8 on the host.  Returns (out uint8, status (n,) int32, rounds (n,) int32 or None, offsets): image i is out[offsets[i] :
    offsets[i] + 3 h w] when status[i] == 0.  out / out_offsets: write into a caller's buffer at the caller's offsets.  Nothing is
    synchronised: items and tables go up as one pinned block.  Wrong arguments raise RuntimeError (the entry's message); a call that
    needs a buffer of 2 GiB or more raises NotImplementedError."""
    import ctypes as Ct
    import numpy as np
    from ._lib import JpegDecItem
    _u8(comp, "comp")
    sub_bytes = JPEG_DEC_SUB_BYTES if sub_bytes is None else int(sub_bytes)
    n, dev = len(specs), comp.device
    tables = np.ascontiguousarray(tables, dtype=np.uint8).reshape(-1)
    if comp.dim() != 1 or tables.size != n * JPEG_DEC_TABLE_BYTES:
        raise RuntimeError(f"jpeg_decode: a flat buffer and {n} x {JPEG_DEC_TABLE_BYTES} table bytes, got {tuple(comp.shape)} and {tables.size}")
    if sub_bytes < 4 or sub_bytes % 4:
        raise RuntimeError(f"jpeg_decode: sub_bytes {sub_bytes} (a multiple of 4, at least 4)")
    layout = jpeg_decode_layout(specs, sub_bytes)
    if layout is None:
        raise RuntimeError(f"jpeg_decode: specs {list(specs)}, sub_bytes {sub_bytes}")
    rows, out_bytes, work_bytes = layout
    if out is None:
        out = torch.empty(out_bytes, device=dev, dtype=torch.uint8)
    else:
        _u8(out, "out")
        rows = [(r[0], int(o)) + r[2:] for r, o in zip(rows, out_offsets)]
        out_bytes = out.numel()
    if n == 0:
        return out, torch.empty(0, device=dev, dtype=torch.int32), torch.empty(0, device=dev, dtype=torch.int32) if want_rounds else None, []
    if max(comp.numel(), out_bytes, work_bytes) >= JPEG_LIMIT_BYTES:
        raise NotImplementedError(f"jpeg_decode: buffers of {comp.numel()}, {out_bytes} and {work_bytes} bytes reach the limit of "
                                  "vsp_jpeg_decode_u8")
    isz = Ct.sizeof(JpegDecItem)
    block = torch.empty(n * (isz + JPEG_DEC_TABLE_BYTES), dtype=torch.uint8, pin_memory=True)
    items = (JpegDecItem * n).from_address(block.data_ptr())
    for i, row in enumerate(rows):
        items[i] = JpegDecItem(*row)
    block[n * isz:].copy_(torch.from_numpy(tables))
    block_dev = block.to(dev, non_blocking=True)
    work = torch.empty(work_bytes, device=dev, dtype=torch.uint8)
    status = torch.empty(n, device=dev, dtype=torch.int32)
    rounds = torch.empty(n, device=dev, dtype=torch.int32) if want_rounds else None
    rc = lib.vsp_jpeg_decode_u8(_ptr(out), out_bytes, _ptr(status), _ptr(rounds) if want_rounds else None, _ptr(work), work_bytes, _ptr(comp),
                                comp.numel(), Ct.c_void_p(block.data_ptr()), _ptr(block_dev), Ct.c_void_p(block.data_ptr() + n * isz),
                                Ct.c_void_p(block_dev.data_ptr() + n * isz), n, sub_bytes, _stream())
    if rc == -3:
        raise NotImplementedError(_lib.last_error())
    check(rc, "jpeg_decode")
    return out, status, rounds, [row[1] for row in rows]


# ----------------------------------------------------------------------------------------------- faces inside whole photos
def _fwd_args(fwd_host, fwd):
    """the forward tables of a *_aa entry: host pointer, device pointer (both NULL when no face is filtered), entries; () for a plain entry"""
    import ctypes as Ct
    if fwd is None:
        return ()
    has = fwd_host.size > 0
    return (fwd_host.ctypes.data_as(Ct.c_void_p) if has else None, _ptr(fwd) if has else None, fwd_host.size)


def _face_crop(name, plan, items, tables, fwd, src, border, u8, f32):
    """face_crop_u8 (fwd None: vsp_face_crop_u8 on the plan's crop_items) and face_crop_aa_u8 (vsp_face_crop_aa_u8 on its crop_aa_items)"""
    import ctypes as Ct
    aa = fwd is not None
    for t, tname in ((items, "items"), (tables, "tables")) + (((fwd, "fwd"),) if aa else ()) + ((src, "src"),):
        _u8(t, tname)
    if not (u8 or f32):
        raise RuntimeError(f"{name}: no output asked for")
    n, S = plan.n, plan.S
    entry, host_items = (lib.vsp_face_crop_aa_u8, plan.crop_aa_items) if aa else (lib.vsp_face_crop_u8, plan.crop_items)
    if (items.numel() != Ct.sizeof(host_items._type_) * n or tables.numel() != plan.crop_tables.nbytes
            or (aa and fwd.numel() != plan.crop_fwd.nbytes) or src.numel() != plan.src_bytes):
        raise RuntimeError(f"{name}: the device sections do not have the plan's sizes")
    out8 = torch.empty((n, S, S, 3), device=src.device, dtype=torch.uint8) if u8 else None
    outf = torch.empty((n, 3, S, S), device=src.device, dtype=torch.float32) if f32 else None
    check(entry(_ptr(out8), _ptr(outf), _ptr(src), plan.src_bytes, plan.crop_tables.ctypes.data_as(Ct.c_void_p), _ptr(tables),
                plan.crop_tables.size, *_fwd_args(plan.crop_fwd if aa else None, fwd), Ct.cast(host_items, Ct.c_void_p), _ptr(items), n, S,
                int(border[0]), int(border[1]), int(border[2]), _stream()), name)
    return out8, outf


def _face_paste(name, plan, photos, crops, items, tables, fwd, tiles, tile_faces, ramp, ramp_dev, mask=None):
    """face_paste_u8 (fwd None: vsp_face_paste_u8 on the plan's paste_items) and face_paste_aa_u8 (vsp_face_paste_aa_u8 on its paste_aa_items);
    with `mask`, the (F, S, S) paste weights of parse_blur_u16, the *_mask_* entries of DESIGN 24"""
    import ctypes as Ct
    aa = fwd is not None
    for t, tname in ((photos, "photos"), (crops, "crops"), (items, "items"), (tables, "tables")) + (((fwd, "fwd"),) if aa else ()) + (
            (tiles, "tiles"), (tile_faces, "tile_faces")):
        _u8(t, tname)
    n, S = plan.n, plan.S
    if not isinstance(ramp_dev, torch.Tensor) or not ramp_dev.is_cuda or ramp_dev.dtype != torch.int16 or ramp_dev.numel() != ramp.size:
        raise RuntimeError(f"{name}: ramp_dev must be the ramp as a CUDA int16 tensor")
    entry, host_items = (lib.vsp_face_paste_aa_u8, plan.paste_aa_items) if aa else (lib.vsp_face_paste_u8, plan.paste_items)
    mask_args = ()
    if mask is not None:
        if (not isinstance(mask, torch.Tensor) or not mask.is_cuda or mask.dtype not in (torch.int16, torch.uint16) or not mask.is_contiguous()
                or mask.numel() != n * S * S):
            raise RuntimeError(f"{name}: mask must be the ({n}, {S}, {S}) paste weights as a contiguous CUDA 16-bit tensor")
        entry = lib.vsp_face_paste_mask_aa_u8 if aa else lib.vsp_face_paste_mask_u8
        mask_args = (_ptr(mask), mask.numel())
    if (photos.numel() != plan.out_bytes or crops.numel() != n * S * S * 3 or items.numel() != Ct.sizeof(host_items._type_) * n
            or tables.numel() != plan.paste_tables.nbytes or (aa and fwd.numel() != plan.paste_fwd.nbytes)
            or tiles.numel() != plan.ntiles * Ct.sizeof(_lib.FaceTile) or tile_faces.numel() != plan.tile_faces.nbytes):
        raise RuntimeError(f"{name}: the device buffers do not have the plan's sizes")
    check(entry(_ptr(photos), plan.out_bytes, _ptr(crops), crops.numel(), plan.paste_tables.ctypes.data_as(Ct.c_void_p), _ptr(tables),
                plan.paste_tables.size, *_fwd_args(plan.paste_fwd if aa else None, fwd), Ct.cast(host_items, Ct.c_void_p), _ptr(items), n, S,
                Ct.cast(plan.tiles, Ct.c_void_p), _ptr(tiles), plan.ntiles, plan.tile_faces.ctypes.data_as(Ct.c_void_p), _ptr(tile_faces),
                plan.tile_faces.size, ramp.ctypes.data_as(Ct.c_void_p), _ptr(ramp_dev), int(ramp.size), *mask_args, _stream()), name)
    return photos


def face_crop_u8(plan, items, tables, src, border=(128, 128, 128), u8=True, f32=False):
    """The aligned S x S crop of every face of a vspbfr_amd.photo.FacePlan (vsp_face_crop_u8, csrc/face_warp.hip).  `items`, `tables`, `src`:
    the plan's crop_items / crop_tables / photos sections on the device (FacePlan.upload).  The library checks the plan's HOST tables
    before it launches.  Returns (u8 (F, S, S, 3) uint8 or None, f32 (F, 3, S, S) fp32 or None) on the current stream."""
    return _face_crop("face_crop_u8", plan, items, tables, None, src, border, u8, f32)


def face_paste_u8(plan, photos, crops, items, tables, tiles, tile_faces, ramp, ramp_dev):
    """Paste the restored crops ((F, S, S, 3) uint8) into the packed output photos, in place (vsp_face_paste_u8, csrc/face_warp.hip).
    `items`, `tables`, `tiles`, `tile_faces`: the plan's paste sections on the device; ramp: host uint16 array, ramp_dev: the same
    values on the device (int16 storage).  Returns photos."""
    return _face_paste("face_paste_u8", plan, photos, crops, items, tables, None, tiles, tile_faces, ramp, ramp_dev)


def face_crop_aa_u8(plan, items, tables, fwd, src, border=(128, 128, 128), u8=True, f32=False):
    """face_crop_u8 for a FacePlan built with antialias=True (vsp_face_crop_aa_u8): `items` is the plan's crop_aa_items section and `fwd`
    its crop_fwd section; a face with reach > 0 is resampled by the tent filter of DESIGN 16, the others exactly as face_crop_u8 does."""
    return _face_crop("face_crop_aa_u8", plan, items, tables, fwd, src, border, u8, f32)


def face_paste_aa_u8(plan, photos, crops, items, tables, fwd, tiles, tile_faces, ramp, ramp_dev):
    """face_paste_u8 for a FacePlan built with antialias=True (vsp_face_paste_aa_u8): `items` is the plan's paste_aa_items section and
    `fwd` its paste_fwd section.  Returns photos."""
    return _face_paste("face_paste_aa_u8", plan, photos, crops, items, tables, fwd, tiles, tile_faces, ramp, ramp_dev)


def face_paste_mask_u8(plan, photos, crops, items, tables, tiles, tile_faces, ramp, ramp_dev, mask):
    """face_paste_u8 through a face-parsing mask (vsp_face_paste_mask_u8): mask is the (F, S, S) tensor of parse_blur_u16, paste
    weights 0 .. 256 sampled with the colour's four taps; the blend weight is (ramp * wm + 128) >> 8.  Returns photos."""
    return _face_paste("face_paste_mask_u8", plan, photos, crops, items, tables, None, tiles, tile_faces, ramp, ramp_dev, mask)


def face_paste_mask_aa_u8(plan, photos, crops, items, tables, fwd, tiles, tile_faces, ramp, ramp_dev, mask):
    """face_paste_aa_u8 through a face-parsing mask (vsp_face_paste_mask_aa_u8): the colour keeps its tent filter, the mask its four taps"""
    return _face_paste("face_paste_mask_aa_u8", plan, photos, crops, items, tables, fwd, tiles, tile_faces, ramp, ramp_dev, mask)


COLOR_FIX_MODES = {"stats": 0, "wavelet": 1}      # include/vspbfr_hip.h VSP_COLOR_FIX_STATS / VSP_COLOR_FIX_WAVELET


def color_fix_u8(crops, restored, mode, plan=None, items=None, tables=None, levels=5, out=None):
    """The colour fix of DESIGN 17 (vsp_color_fix_u8, csrc/color_fix.hip) on two (F, S, S, 3) uint8 device tensors: mode "wavelet" keeps the
    restored high frequencies and takes the low ones (`levels` dilated [1 2 1] blurs) from the crop, "stats" moves the restored crop's
    per-channel mean and deviation onto the crop's.  plan / items / tables: a FacePlan and its crop_items / crop_tables sections on the
    device -- pixels whose centre cell lies outside the photo take no part; all None: every pixel is valid.  out: None (a new tensor)
    or a contiguous tensor like `restored`, which may be `restored` itself.  The scratch is allocated here.  Returns out."""
    import ctypes as Ct
    _u8(crops, "crops"), _u8(restored, "restored")
    if mode not in COLOR_FIX_MODES:
        raise ValueError(f"color_fix_u8: mode {mode!r} (one of {sorted(COLOR_FIX_MODES)})")
    if crops.dim() != 4 or crops.shape[3] != 3 or crops.shape[1] != crops.shape[2] or crops.shape != restored.shape:
        raise RuntimeError(f"color_fix_u8: crops {tuple(crops.shape)} and restored {tuple(restored.shape)} must both be (F, S, S, 3)")
    F, S = int(crops.shape[0]), int(crops.shape[1])
    if out is None:
        out = torch.empty_like(restored)
    _u8(out, "out")
    if out.shape != restored.shape:
        raise RuntimeError("color_fix_u8: out must have the shape of restored")
    if (plan is None) != (items is None) or (plan is None) != (tables is None):
        raise RuntimeError("color_fix_u8: plan, items and tables go together")
    host_items = host_tables = dev_items = dev_tables = None
    table_ints = 0
    if plan is not None:
        _u8(items, "items"), _u8(tables, "tables")
        if plan.n != F or plan.S != S or items.numel() != F * Ct.sizeof(_lib.FaceItem) or tables.numel() != plan.crop_tables.nbytes:
            raise RuntimeError("color_fix_u8: the plan or its device sections do not match the crops")
        host_items, host_tables = Ct.cast(plan.crop_items, Ct.c_void_p), plan.crop_tables.ctypes.data_as(Ct.c_void_p)
        dev_items, dev_tables, table_ints = _ptr(items), _ptr(tables), plan.crop_tables.size
    nbytes = 12 * F * S * S if mode == "wavelet" else 128 * F
    scratch = torch.empty(max(nbytes, 16), device=restored.device, dtype=torch.uint8)
    check(lib.vsp_color_fix_u8(_ptr(crops), _ptr(restored), _ptr(out), F, S, COLOR_FIX_MODES[mode], int(levels), host_items, dev_items,
                               host_tables, dev_tables, table_ints, _ptr(scratch), nbytes, _stream()), "color_fix_u8")
    return out


# ----------------------------------------------------------------------------------------------- face detection
DET_MAX_CANDIDATES = 2048                    # include/vspbfr_hip.h VSP_DET_MAX_CANDIDATES
DET_CAND_CAPPED, DET_FACES_CAPPED, DET_NONFINITE = 1, 2, 4      # VSP_DET_* status bits


def det_priors(Hc, Wc):
    """priors of an (Hc, Wc) canvas: 2 sum over steps 8, 16, 32 of ceil(Hc / s) ceil(Wc / s) (vsp_det_priors)"""
    n = lib.vsp_det_priors(int(Hc), int(Wc))
    if n <= 0:
        raise RuntimeError(f"det_priors: canvas {(Hc, Wc)}")
    return n


def det_entry_u8(y, src, items, items_dev, n, w, b, Hc, Wc, slope=0.1):
    """The detector's first layer on n u8 photos inside `src` (vsp_det_entry_u8): writes y[slot] (y is (B, 8, ceil(Hc/2), ceil(Wc/2)))
    for the slots of `items` (a _lib.DetSrc array; items_dev the same bytes on the device).  w (3, 9, 8), b (8).  Returns y."""
    _req(y, "y"), _u8(src, "src"), _u8(items_dev, "items_dev"), _req(w, "w"), _req(b, "b")
    B = int(y.shape[0])
    if y.dim() != 4 or tuple(y.shape[1:]) != (8, (Hc + 1) // 2, (Wc + 1) // 2) or w.numel() != 216 or b.numel() != 8:
        raise RuntimeError(f"det_entry_u8: y {tuple(y.shape)} for a {(Hc, Wc)} canvas, w {tuple(w.shape)}, b {tuple(b.shape)}")
    if items_dev.numel() < n * C.sizeof(_lib.DetSrc):
        raise RuntimeError("det_entry_u8: items_dev is shorter than the item table")
    check(lib.vsp_det_entry_u8(_ptr(y), _ptr(src), src.numel(), C.cast(items, C.c_void_p), _ptr(items_dev), int(n), _ptr(w), _ptr(b), B,
                               int(Hc), int(Wc), 1, float(slope), _stream()), "det_entry_u8")
    return y


def det_sep(x, wd, bd, wp, bp, stride=1, slope=0.1):
    """One depthwise-separable block (vsp_det_sep_f32): x (B, Cin, H, W), wd (Cin, 9), bd (Cin), wp (Cin, Cout), bp (Cout) ->
    (B, Cout, OH, OW), LeakyReLU(slope) behind both convolutions."""
    for t, nm in ((x, "x"), (wd, "wd"), (bd, "bd"), (wp, "wp"), (bp, "bp")):
        _req(t, nm)
    B, Cin, H, W = (int(v) for v in x.shape)
    Cout = int(wp.shape[1]) if wp.dim() == 2 else -1
    if tuple(wd.shape) != (Cin, 9) or tuple(bd.shape) != (Cin,) or tuple(wp.shape) != (Cin, Cout) or tuple(bp.shape) != (Cout,):
        raise RuntimeError(f"det_sep: x {tuple(x.shape)}, wd {tuple(wd.shape)}, bd {tuple(bd.shape)}, wp {tuple(wp.shape)}, bp {tuple(bp.shape)}")
    if stride not in (1, 2):
        raise RuntimeError(f"det_sep: stride {stride}")
    y = torch.empty((B, Cout, (H - 1) // stride + 1, (W - 1) // stride + 1), device=x.device, dtype=torch.float32)
    check(lib.vsp_det_sep_f32(_ptr(y), _ptr(x), _ptr(wd), _ptr(bd), _ptr(wp), _ptr(bp), B, Cin, Cout, H, W, int(stride), float(slope),
                              _stream()), "det_sep")
    return y


def det_conv3x3(x, w, b, slope=None, out=None, y_coff=0):
    """Dense 3x3, stride 1, pad 1 (vsp_det_conv3x3_f32): x (B, Cin, H, W), w (Cin, 9, Cout), b (Cout).  slope None: no activation,
    else LeakyReLU(slope) (0: ReLU).  out: None (a new (B, Cout, H, W)) or a (B, C, H, W) tensor whose channels y_coff.. take the result."""
    _req(x, "x"), _req(w, "w"), _req(b, "b")
    B, Cin, H, W = (int(v) for v in x.shape)
    if w.dim() != 3 or tuple(w.shape[:2]) != (Cin, 9) or tuple(b.shape) != (int(w.shape[2]),):
        raise RuntimeError(f"det_conv3x3: x {tuple(x.shape)}, w {tuple(w.shape)}, b {tuple(b.shape)}")
    Cout = int(w.shape[2])
    if out is None:
        out = torch.empty((B, Cout, H, W), device=x.device, dtype=torch.float32)
    _req(out, "out")
    if out.dim() != 4 or (int(out.shape[0]), int(out.shape[2]), int(out.shape[3])) != (B, H, W):
        raise RuntimeError(f"det_conv3x3: out {tuple(out.shape)} for x {tuple(x.shape)}")
    check(lib.vsp_det_conv3x3_f32(_ptr(out), _ptr(x), _ptr(w), _ptr(b), B, Cin, Cout, H, W, int(out.shape[1]), int(y_coff),
                                  0 if slope is None else 1, 0.0 if slope is None else float(slope), _stream()), "det_conv3x3")
    return out


def det_lateral(x, w, b, up=None, slope=0.1):
    """1x1 to 64 channels, LeakyReLU(slope), plus the nearest upsampling (source index floor(i in / out)) of `up` (B, 64, h2, w2)
    (vsp_det_lateral_f32): x (B, Cin, H, W), w (Cin, 64), b (64) -> (B, 64, H, W)."""
    _req(x, "x"), _req(w, "w"), _req(b, "b"), _opt(up, "up")
    B, Cin, H, W = (int(v) for v in x.shape)
    if tuple(w.shape) != (Cin, 64) or tuple(b.shape) != (64,):
        raise RuntimeError(f"det_lateral: x {tuple(x.shape)}, w {tuple(w.shape)}, b {tuple(b.shape)}")
    h2 = w2 = 0
    if up is not None:
        if up.dim() != 4 or tuple(up.shape[:2]) != (B, 64):
            raise RuntimeError(f"det_lateral: up {tuple(up.shape)}")
        h2, w2 = int(up.shape[2]), int(up.shape[3])
    y = torch.empty((B, 64, H, W), device=x.device, dtype=torch.float32)
    check(lib.vsp_det_lateral_f32(_ptr(y), _ptr(x), _ptr(w), _ptr(b), _ptr(up), B, Cin, H, W, h2, w2, 1, float(slope), _stream()),
          "det_lateral")
    return y


def det_heads(x, w, b, conf, loc, lm, p0):
    """The class, box and landmark heads of one level (vsp_det_heads_f32): x (B, 64, H, W), w (64, 32), b (32) -> priors p0 .. p0 + 2 H W
    - 1 of conf (B, P, 2), loc (B, P, 4), lm (B, P, 10)."""
    for t, nm in ((x, "x"), (w, "w"), (b, "b"), (conf, "conf"), (loc, "loc"), (lm, "lm")):
        _req(t, nm)
    B, Cin, H, W = (int(v) for v in x.shape)
    P = int(conf.shape[1]) if conf.dim() == 3 else -1
    if Cin != 64 or tuple(w.shape) != (64, 32) or tuple(b.shape) != (32,) or tuple(conf.shape) != (B, P, 2) or tuple(loc.shape) != (B, P, 4) \
            or tuple(lm.shape) != (B, P, 10):
        raise RuntimeError(f"det_heads: x {tuple(x.shape)}, w {tuple(w.shape)}, conf {tuple(conf.shape)}, loc {tuple(loc.shape)}, lm {tuple(lm.shape)}")
    check(lib.vsp_det_heads_f32(_ptr(conf), _ptr(loc), _ptr(lm), _ptr(x), _ptr(w), _ptr(b), B, H, W, P, int(p0), _stream()), "det_heads")


def det_decode_nms(conf, loc, lm, Hc, Wc, threshold=0.8, nms=0.4, max_candidates=1024, max_faces=256):
    """Decode, candidate selection and greedy NMS per image on the device (vsp_det_decode_nms_f32): conf (B, P, 2), loc (B, P, 4), lm
    (B, P, 10) for the P priors of an (Hc, Wc) canvas -> (faces: uint8 (B, max_faces, 64) holding _lib.DetFace records, zero past the
    count; info: int32 (B, 4) = faces written, status bits DET_*, candidates before the cap, non-finite candidates dropped)."""
    _req(conf, "conf"), _req(loc, "loc"), _req(lm, "lm")
    P = det_priors(Hc, Wc)
    B = int(conf.shape[0])
    if tuple(conf.shape) != (B, P, 2) or tuple(loc.shape) != (B, P, 4) or tuple(lm.shape) != (B, P, 10):
        raise RuntimeError(f"det_decode_nms: conf {tuple(conf.shape)}, loc {tuple(loc.shape)}, lm {tuple(lm.shape)} for {P} priors")
    max_candidates, max_faces = int(max_candidates), int(max_faces)
    faces = torch.zeros((B, max(max_faces, 1), 64), device=conf.device, dtype=torch.uint8)
    info = torch.zeros((B, 4), device=conf.device, dtype=torch.int32)
    nbytes = lib.vsp_det_work_bytes(max(B, 1), int(Hc), int(Wc), max_candidates)
    work = torch.empty(max(nbytes, 16), device=conf.device, dtype=torch.uint8)
    check(lib.vsp_det_decode_nms_f32(_ptr(faces), _ptr(info), _ptr(work), work.numel(), _ptr(conf), _ptr(loc), _ptr(lm), B, int(Hc), int(Wc),
                                     float(threshold), float(nms), max_candidates, max_faces, _stream()), "det_decode_nms")
    return faces, info


SR_TILE_H, SR_TILE_W, SR_NONFINITE = 8, 32, 1      # include/vspbfr_hip.h VSP_SR_TILE_*, VSP_SR_NONFINITE
_TWO_GIB = 1 << 31


def _sr_act(t, name):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float16 or t.dim() != 1 or not t.is_contiguous():
        raise RuntimeError(f"{name} must be a flat contiguous CUDA float16 tensor")
    return t


def sr_head_u8(y, src, items, items_dev, n, w, b, slope):
    """The upscaler's first layer on the u8 photos of a group where they lie in `src` (vsp_sr_head_u8): y, a flat float16 buffer, takes
    PReLU(conv3x3(src / 255) + b) as (h, w, 64) per item at items[i].act_off pixels.  items: a _lib.SrItem array, items_dev the same
    bytes on the device.  w (27, 64), b (64), slope (64) float32.  Returns y."""
    _sr_act(y, "y"), _u8(src, "src"), _u8(items_dev, "items_dev"), _req(w, "w"), _req(b, "b"), _req(slope, "slope")
    if w.numel() != 27 * 64 or b.numel() != 64 or slope.numel() != 64 or items_dev.numel() < n * C.sizeof(_lib.SrItem):
        raise RuntimeError(f"sr_head_u8: w {tuple(w.shape)}, b {tuple(b.shape)}, slope {tuple(slope.shape)}, items_dev of {items_dev.numel()} bytes")
    check(lib.vsp_sr_head_u8(_ptr(y), y.numel() * 2, _ptr(src), src.numel(), C.cast(items, C.c_void_p), _ptr(items_dev), int(n), _ptr(w),
                             _ptr(b), _ptr(slope), _stream()), "sr_head_u8")
    return y


def sr_body_f16(y, x, items, items_dev, n, w_img, b, slope):
    """One body layer of the upscaler over a group (vsp_sr_body_f16): y = PReLU(conv3x3(x) + b), x and y flat float16 buffers of one size
    holding (h, w, 64) per item; w_img the float16 image of upscale.pack_body_weight (18, 4, 64, 8), b and slope float32 (64)."""
    _sr_act(y, "y"), _sr_act(x, "x"), _u8(items_dev, "items_dev"), _req(b, "b"), _req(slope, "slope")
    if y.numel() != x.numel() or not isinstance(w_img, torch.Tensor) or w_img.dtype != torch.float16 or not w_img.is_contiguous() \
            or w_img.numel() != 18 * 4 * 64 * 8 or b.numel() != 64 or slope.numel() != 64 or items_dev.numel() < n * C.sizeof(_lib.SrItem):
        raise RuntimeError("sr_body_f16: x and y of one size, w_img a float16 image of 18 x 4 x 64 x 8, b and slope of 64")
    check(lib.vsp_sr_body_f16(_ptr(y), _ptr(x), x.numel() * 2, C.cast(items, C.c_void_p), _ptr(items_dev), int(n), _ptr(w_img), _ptr(b),
                              _ptr(slope), _stream()), "sr_body_f16")
    return y


def sr_tail_u8(out, info, x, src, items, items_dev, n, w_img, b, scale, out_f32=None):
    """The upscaler's last layer over a group (vsp_sr_tail_u8): conv3x3 64 -> 3 scale^2, + b, pixel shuffle, + src / 255, clamp, u8 into
    the flat uint8 `out` at items[i].out_off; info (int32, zeroed by the caller) takes SR_NONFINITE at items[i].slot.  w_img: float16
    (18, NB, 64, 8) with NB = 1 (scale 2) or 3 (scale 4), b float32 (16 NB).  out_f32: a flat float32 tensor of out's size or None."""
    _u8(out, "out"), _sr_act(x, "x"), _u8(src, "src"), _u8(items_dev, "items_dev"), _req(b, "b"), _opt(out_f32, "out_f32")
    nb = {2: 1, 4: 3}.get(int(scale), 0)
    if not isinstance(info, torch.Tensor) or info.dtype != torch.int32 or not info.is_cuda or not info.is_contiguous():
        raise RuntimeError("sr_tail_u8: info must be a contiguous CUDA int32 tensor")
    if nb and (not isinstance(w_img, torch.Tensor) or w_img.dtype != torch.float16 or not w_img.is_contiguous()
               or w_img.numel() != 18 * nb * 64 * 8 or b.numel() != 16 * nb):
        raise RuntimeError(f"sr_tail_u8: scale {scale} takes a float16 image of 18 x {nb} x 64 x 8 and {16 * nb} biases")
    if out_f32 is not None and out_f32.numel() != out.numel():
        raise RuntimeError("sr_tail_u8: out_f32 must have one float per byte of out")
    if items_dev.numel() < n * C.sizeof(_lib.SrItem):
        raise RuntimeError("sr_tail_u8: items_dev is shorter than the item table")
    check(lib.vsp_sr_tail_u8(_ptr(out), out.numel(), _ptr(out_f32), _ptr(info), info.numel(), _ptr(x), x.numel() * 2, _ptr(src), src.numel(),
                             C.cast(items, C.c_void_p), _ptr(items_dev), int(n), _ptr(w_img), _ptr(b), int(scale), _stream()), "sr_tail_u8")
    return out


# ------------------------------------------------------------------------------------------------- face parsing
PARSE_CLASSES, PARSE_MAX_RADIUS, PARSE_NONFINITE = 19, 64, 1      # include/vspbfr_hip.h VSP_PARSE_*
PARSE_ACT, PARSE_UP = 1, 2
PARSE_KEEP = tuple(0 if c in (0, 14, 16, 17, 18) else 1 for c in range(19))     # the common MASK_COLORMAP: background, neck, clothes, hair, hat go


def _parse_t(t, name, dtype, numel=None):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != dtype or not t.is_contiguous() or (numel is not None and t.numel() != numel):
        raise RuntimeError(f"{name} must be a contiguous CUDA {dtype} tensor" + (f" of {numel} elements" if numel is not None else ""))
    return t


def parse_conv_out(H, W, stride=1, up=False):
    """the output map of parse_conv_f16 for an (H, W) input"""
    hd, wd = (2 * H, 2 * W) if up else (H, W)
    return ((hd - 1) // 2 + 1, (wd - 1) // 2 + 1) if stride == 2 else (hd, wd)


def parse_head_u8(y, crops, w, b):
    """ParseNet's first layer (vsp_parse_head_u8): crops (F, H, W, 3) uint8 -> y, a float16 tensor of F H W 64 elements, = conv3x3 of
    (crops / 255 - 0.5) / 0.5 behind a reflection padding, + b, without an activation.  w (27, 64), b (64) float32.  Returns y."""
    _u8(crops, "crops"), _req(w, "w"), _req(b, "b")
    if crops.dim() != 4 or crops.shape[3] != 3 or w.numel() != 27 * 64 or b.numel() != 64:
        raise RuntimeError(f"parse_head_u8: crops {tuple(crops.shape)}, w {tuple(w.shape)}, b {tuple(b.shape)}")
    F, H, W = (int(v) for v in crops.shape[:3])
    _parse_t(y, "y", torch.float16, F * H * W * 64)
    check(lib.vsp_parse_head_u8(_ptr(y), _ptr(crops), F, H, W, _ptr(w), _ptr(b), _stream()), "parse_head_u8")
    return y


def parse_conv_f16(y, x, F, H, W, w_img, b, stride=1, act=False, up=False, res1=None, res2=None):
    """One 3x3 convolution of ParseNet (vsp_parse_conv_f16): x holds (F, H, W, Cin) float16, y takes (F, OH, OW, Cout) with (OH, OW) =
    parse_conv_out(H, W, stride, up); reflection padding, optional fused nearest x2 (`up`), LeakyReLU(0.2) (`act`) and up to two float16
    residuals of y's shape, either of which may be y itself.  w_img: parse.pack_conv_weight's image (Cout / 64, Cin / 64, 18, 4, 64, 8)
    float16; b float32 (Cout).  Returns y."""
    _parse_t(w_img, "w_img", torch.float16), _req(b, "b")
    if w_img.dim() != 6 or tuple(w_img.shape[2:]) != (18, 4, 64, 8):
        raise RuntimeError(f"parse_conv_f16: w_img {tuple(w_img.shape)}, expected (Cout / 64, Cin / 64, 18, 4, 64, 8)")
    cout, cin = 64 * int(w_img.shape[0]), 64 * int(w_img.shape[1])
    F, H, W = int(F), int(H), int(W)
    oh, ow = parse_conv_out(H, W, stride, up)
    if b.numel() != cout:
        raise RuntimeError(f"parse_conv_f16: {b.numel()} biases for {cout} channels")
    _parse_t(x, "x", torch.float16, F * H * W * cin), _parse_t(y, "y", torch.float16, F * oh * ow * cout)
    for r, name in ((res1, "res1"), (res2, "res2")):
        if r is not None:
            _parse_t(r, name, torch.float16, y.numel())
    check(lib.vsp_parse_conv_f16(_ptr(y), _ptr(x), F, H, W, cin, cout, int(stride), (PARSE_ACT if act else 0) | (PARSE_UP if up else 0),
                                 _ptr(w_img), _ptr(b), _ptr(res1), _ptr(res2), _stream()), "parse_conv_f16")
    return y


def parse_mask_u8(x, F, H, W, w_img, b, keep=PARSE_KEEP, info=None, logits=False, out=None):
    """ParseNet's out_mask_conv and what follows it (vsp_parse_mask_u8): x (F, H, W, 64) float16 -> (classes (F, H, W) uint8 = argmax of the
    19 fp32 logits, a tie to the lowest class; keep map (F, H, W) uint8 = keep[class]; info (F) int32 with PARSE_NONFINITE for a face
    that had a non-finite logit -- its pixel gets class 0; the (F, H, W, 19) fp32 logits or None).  w_img (1, 1, 18, 2, 64, 8) float16,
    b float32 (32, the last 13 zero); keep: 19 values 0 / 1 on the host.  logits: False, True (a new tensor) or a contiguous float32
    tensor of F H W 19 elements to write into; out: None or (classes, keep map), contiguous uint8 tensors of F H W elements to write into."""
    import ctypes as Ct
    F, H, W = int(F), int(H), int(W)
    _parse_t(x, "x", torch.float16, F * H * W * 64), _parse_t(w_img, "w_img", torch.float16, 18 * 2 * 64 * 8), _req(b, "b")
    keep = [int(v) for v in keep]
    if b.numel() != 32 or len(keep) != PARSE_CLASSES or any(v not in (0, 1) for v in keep):
        raise RuntimeError("parse_mask_u8: b of 32 values (19 and padding), keep of 19 values 0 / 1")
    if info is None:
        info = torch.zeros(F, dtype=torch.int32, device=x.device)
    _parse_t(info, "info", torch.int32, F)
    if out is None:
        out = (torch.empty((F, H, W), dtype=torch.uint8, device=x.device), torch.empty((F, H, W), dtype=torch.uint8, device=x.device))
    cls, kmap = out
    _parse_t(cls, "classes", torch.uint8, F * H * W), _parse_t(kmap, "keep map", torch.uint8, F * H * W)
    if isinstance(logits, torch.Tensor):
        lg = _parse_t(logits, "logits", torch.float32, F * H * W * PARSE_CLASSES)
    else:
        lg = torch.empty((F, H, W, PARSE_CLASSES), dtype=torch.float32, device=x.device) if logits else None
    table = (Ct.c_uint8 * PARSE_CLASSES)(*keep)
    check(lib.vsp_parse_mask_u8(_ptr(cls), _ptr(kmap), _ptr(lg), _ptr(info), _ptr(x), F, H, W, _ptr(w_img), _ptr(b),
                                Ct.cast(table, Ct.c_void_p), _stream()), "parse_mask_u8")
    return cls, kmap, info, lg


def parse_blur_u16(keep, taps, border, out=None, work=None):
    """The paste weights of a keep map (vsp_parse_blur_u16): keep (F, S, S) uint8 -> (F, S, S) torch.uint16 in 0 .. 256 -- m0 = 16384 keep,
    four 1-D integer passes with reflect-101 borders (x, y, x, y), (m + 32) >> 6, the outermost `border` rows and columns 0.  taps: R + 1 non-negative ints on the host, g[0] + 2 sum g[k >= 1]
    = 65536.  work: a uint16 tensor of 2 F S S elements or None (allocated here)."""
    import ctypes as Ct
    _u8(keep, "keep")
    if keep.dim() != 3 or keep.shape[1] != keep.shape[2]:
        raise RuntimeError(f"parse_blur_u16: keep {tuple(keep.shape)}, expected (F, S, S)")
    F, S = int(keep.shape[0]), int(keep.shape[1])
    taps = [int(v) for v in taps]
    if not taps or len(taps) > PARSE_MAX_RADIUS + 1:
        raise RuntimeError(f"parse_blur_u16: {len(taps)} taps (1..{PARSE_MAX_RADIUS + 1})")
    if out is None:
        out = torch.empty((F, S, S), dtype=torch.uint16, device=keep.device)
    if work is None:
        work = torch.empty(2 * F * S * S, dtype=torch.uint16, device=keep.device)
    _parse_t(out, "out", torch.uint16, F * S * S), _parse_t(work, "work", torch.uint16)
    table = (Ct.c_int32 * len(taps))(*taps)
    check(lib.vsp_parse_blur_u16(_ptr(out), _ptr(keep), _ptr(work), work.numel() * 2, F, S, Ct.cast(table, Ct.c_void_p), len(taps) - 1, int(border),
                                 _stream()), "parse_blur_u16")
    return out


# ------------------------------------------------------------------------------------------------------------ FID
FID_POOL_MAX_S2, FID_POOL_AVG_S1, FID_POOL_MAX_S1, FID_POOL_GLOBAL_AVG = 0, 1, 2, 3      # include/vspbfr_hip.h VSP_FID_POOL_*
FID_FILTERS = ((1, 1), (3, 3), (5, 5), (1, 7), (7, 1), (1, 3), (3, 1))


def fid_conv_out(H, W, kh, kw, ph, pw, stride):
    """the output map of fid_conv_f32"""
    return (H + 2 * ph - kh) // stride + 1, (W + 2 * pw - kw) // stride + 1


def fid_pool_out(H, W, mode):
    """the output map of fid_pool_f32"""
    return ((H - 3) // 2 + 1, (W - 3) // 2 + 1) if mode == FID_POOL_MAX_S2 else (1, 1) if mode == FID_POOL_GLOBAL_AVG else (H, W)


def _fid_view(t, name, B, H, W, C):
    """(tensor, channel offset, pitch) -> the pointer of channel `offset` and the pitch, after checking that the tensor holds the
    (B, H, W, pitch) image"""
    buf, off, pitch = t
    _req(buf, name)
    off, pitch = int(off), int(pitch)
    if off < 0 or off % 4 or pitch % 4 or off + C > pitch or buf.numel() < B * H * W * pitch:
        raise RuntimeError(f"{name}: channels {off}..{off + C} of a pitch of {pitch}, {B} x {H} x {W} pixels in a tensor of {buf.numel()} floats")
    return buf.data_ptr() + 4 * off, off, pitch


def fid_stem_u8(y, src, items, items_dev, n, B, TH, TW, w, b):
    """The first layer of the FID Inception on n u8 RGB images inside `src` (vsp_fid_stem_u8): bilinear resize to (TH, TW) without
    anti-aliasing, x / 127.5 - 1, Conv2d_1a 3 -> 32 (3x3, stride 2) + b, ReLU.  y: a float32 tensor of B OH OW 32 elements, written at
    the slots of `items` (a _lib.DetSrc array; items_dev the same bytes on the device).  w (27, 32), b (32).  Returns y."""
    _req(y, "y"), _u8(src, "src"), _u8(items_dev, "items_dev"), _req(w, "w"), _req(b, "b")
    oh, ow = (int(TH) - 3) // 2 + 1, (int(TW) - 3) // 2 + 1
    if y.numel() != B * oh * ow * 32 or w.numel() != 27 * 32 or b.numel() != 32:
        raise RuntimeError(f"fid_stem_u8: y of {y.numel()} floats for {B} x {oh} x {ow} x 32, w {tuple(w.shape)}, b {tuple(b.shape)}")
    if items_dev.numel() < n * C.sizeof(_lib.DetSrc):
        raise RuntimeError("fid_stem_u8: items_dev is shorter than the item table")
    check(lib.vsp_fid_stem_u8(_ptr(y), _ptr(src), src.numel(), C.cast(items, C.c_void_p), _ptr(items_dev), int(n), int(B), int(TH), int(TW),
                              _ptr(w), _ptr(b), _stream()), "fid_stem_u8")
    return y


def fid_conv_f32(out, x, w, bias, B, H, W, stride=1, pad=(0, 0)):
    """One convolution of the FID Inception (vsp_fid_conv_f32): ReLU(conv(x) + bias) on the fp32-input MFMA.  x and out are (tensor,
    channel offset, pitch) triples over float32 tensors holding (B, H, W, pitch) and (B, OH, OW, pitch): the convolution reads Cin
    channels from x's offset on and writes Cout channels from out's offset on.  w (KH, KW, Cin, Cout) float32, bias (Cout).  Returns
    (OH, OW)."""
    _req(w, "w"), _req(bias, "bias")
    if w.dim() != 4 or bias.numel() != w.shape[3]:
        raise RuntimeError(f"fid_conv_f32: w {tuple(w.shape)}, expected (KH, KW, Cin, Cout), and {bias.numel()} biases")
    kh, kw, cin, cout = (int(v) for v in w.shape)
    B, H, W, ph, pw = int(B), int(H), int(W), int(pad[0]), int(pad[1])
    oh, ow = fid_conv_out(H, W, kh, kw, ph, pw, int(stride))
    xp, _, x_pitch = _fid_view(x, "fid_conv_f32: x", B, H, W, cin)
    _, c_off, c_pitch = _fid_view(out, "fid_conv_f32: out", B, max(oh, 0), max(ow, 0), cout)
    check(lib.vsp_fid_conv_f32(_ptr(out[0]), C.c_void_p(xp), _ptr(w), _ptr(bias), B, H, W, cin, x_pitch, cout, kh, kw, ph, pw, int(stride), c_off,
                               c_pitch, _stream()), "fid_conv_f32")
    return oh, ow


def fid_pool_f32(out, x, B, H, W, C_, mode):
    """A pool of the FID Inception (vsp_fid_pool_f32) over C_ channels: FID_POOL_MAX_S2 (3x3 / 2), FID_POOL_AVG_S1 (3x3 / 1 / pad 1, the
    mean of the in-bounds taps), FID_POOL_MAX_S1 (3x3 / 1 / pad 1) or FID_POOL_GLOBAL_AVG ((B, H, W, C) -> (B, C)).  x and out as in
    fid_conv_f32.  Returns (OH, OW)."""
    B, H, W, C_, mode = int(B), int(H), int(W), int(C_), int(mode)
    oh, ow = fid_pool_out(H, W, mode)
    xp, _, x_pitch = _fid_view(x, "fid_pool_f32: x", B, H, W, C_)
    _, c_off, c_pitch = _fid_view(out, "fid_pool_f32: out", B, max(oh, 0), max(ow, 0), C_)
    check(lib.vsp_fid_pool_f32(_ptr(out[0]), C.c_void_p(xp), B, H, W, C_, x_pitch, mode, c_off, c_pitch, _stream()), "fid_pool_f32")
    return oh, ow


# ------------------------------------------------------------------------------------------------- RRDBNet upscaling
RRDB_NONFINITE, RRDB_ACT, RRDB_UP = 1, 1, 2      # include/vspbfr_hip.h VSP_RRDB_*


def _rrdb_act(t, name, need):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float16 or t.dim() != 1 or not t.is_contiguous() or t.numel() < need:
        raise RuntimeError(f"{name} must be a flat contiguous CUDA float16 tensor of at least {need} elements")
    return t


def rrdb_head_u8(y, y_pitch, src, src_off, h, w, scale, w_pack, b, row0=0, rows=None):
    """RRDBNet's conv_first on the u8 photo (h, w, 3) at byte src_off of the flat uint8 `src` (vsp_rrdb_head_u8): rows row0 .. row0 + rows
    - 1 of the network's input map -- (h, w) at scale 4, (ceil(h / 2), ceil(w / 2)) behind the pixel unshuffle at scale 2 -- go to y, a flat
    float16 buffer with y_pitch halves per pixel, channels 0 .. 63.  w_pack (27 | 108, 64), b (64) float32.  Returns (rows, map width)."""
    h, w, scale, y_pitch = int(h), int(w), int(scale), int(y_pitch)
    nh, nw = (h, w) if scale == 4 else ((h + 1) // 2, (w + 1) // 2)
    rows = nh - int(row0) if rows is None else int(rows)
    _u8(src, "src"), _req(w_pack, "w_pack"), _req(b, "b")
    if w_pack.numel() != (27 if scale == 4 else 108) * 64 or b.numel() != 64:
        raise RuntimeError(f"rrdb_head_u8: scale {scale}: w_pack {tuple(w_pack.shape)}, b {tuple(b.shape)}")
    _rrdb_act(y, "y", max(rows, 0) * nw * y_pitch)
    check(lib.vsp_rrdb_head_u8(_ptr(y), y_pitch, _ptr(src), src.numel(), int(src_off), h, w, scale, int(row0), rows, _ptr(w_pack), _ptr(b),
                               _stream()), "rrdb_head_u8")
    return rows, nw


def rrdb_conv_f16(y, y_pitch, y_off, x, x_pitch, H, W, w_img, b, act=False, up=False, res1=None, res2=None):
    """One 3x3 convolution of RRDBNet (vsp_rrdb_conv_f16): x, a flat float16 buffer holding (H, W, x_pitch), is read in its channels
    0 .. Cin - 1; channels y_off .. y_off + Cout - 1 of y, (OH, OW, y_pitch) with (OH, OW) = (2 H, 2 W) under `up` (nearest x2 of the
    input) and (H, W) otherwise, take f16(s2 (s1 v + r1) + r2) with v = [LeakyReLU 0.2] (conv(x) + b).  res1, res2: None or (flat float16
    tensor, pitch, scale).  y may be x when y_off >= Cin.  w_img: rrdb.pack_conv_weight's image (Cin / 32, 9, Cout / 16, 64, 8); b float32
    (Cout).  Returns y."""
    H, W, y_pitch, y_off, x_pitch = int(H), int(W), int(y_pitch), int(y_off), int(x_pitch)
    if not isinstance(w_img, torch.Tensor) or not w_img.is_cuda or w_img.dtype != torch.float16 or not w_img.is_contiguous() or w_img.dim() != 5 \
            or tuple(w_img.shape[3:]) != (64, 8) or w_img.shape[1] != 9:
        raise RuntimeError("rrdb_conv_f16: w_img must be a contiguous CUDA float16 image (Cin / 32, 9, Cout / 16, 64, 8)")
    cin, cout = 32 * int(w_img.shape[0]), 16 * int(w_img.shape[2])
    _req(b, "b")
    if b.numel() != cout:
        raise RuntimeError(f"rrdb_conv_f16: {b.numel()} biases for {cout} channels")
    oh, ow = (2 * H, 2 * W) if up else (H, W)
    _rrdb_act(x, "x", H * W * x_pitch), _rrdb_act(y, "y", oh * ow * y_pitch)
    r = []
    for res, name in ((res1, "res1"), (res2, "res2")):
        if res is None:
            r += [None, 0, 0.0]
        else:
            r += [_ptr(_rrdb_act(res[0], name, oh * ow * int(res[1]))), int(res[1]), float(res[2])]
    check(lib.vsp_rrdb_conv_f16(_ptr(y), y_pitch, y_off, _ptr(x), x_pitch, H, W, cin, cout, (RRDB_ACT if act else 0) | (RRDB_UP if up else 0),
                                _ptr(w_img), _ptr(b), r[0], r[1], r[2], r[3], r[4], r[5], _stream()), "rrdb_conv_f16")
    return y


def rrdb_tail_u8(out, out_off, out_pitch, out_w, info, x, x_pitch, H, W, keep0, keepn, w_img, b, out_f32=None):
    """RRDBNet's conv_last and the quantisation (vsp_rrdb_tail_u8): x holds (H, W, x_pitch) float16; rows keep0 .. keep0 + keepn - 1 and
    columns 0 .. out_w - 1 of clamp(conv(x) + b) go as rintf(255 v) bytes to the flat uint8 `out`, row keep0 at byte out_off, rows
    out_pitch bytes apart.  info: a CUDA int32 tensor of one word, zeroed by the caller, takes RRDB_NONFINITE.  w_img (2, 9, 1, 64, 8)
    float16, b float32 (16, the last 13 zero).  out_f32: a flat float32 tensor of out's size or None.  Returns out."""
    H, W, x_pitch = int(H), int(W), int(x_pitch)
    _u8(out, "out"), _rrdb_act(x, "x", H * W * x_pitch), _req(b, "b"), _opt(out_f32, "out_f32")
    if not isinstance(info, torch.Tensor) or info.dtype != torch.int32 or not info.is_cuda or not info.is_contiguous() or info.numel() < 1:
        raise RuntimeError("rrdb_tail_u8: info must be a contiguous CUDA int32 tensor")
    if not isinstance(w_img, torch.Tensor) or not w_img.is_cuda or w_img.dtype != torch.float16 or not w_img.is_contiguous() \
            or w_img.numel() != 2 * 9 * 64 * 8 or b.numel() != 16:
        raise RuntimeError("rrdb_tail_u8: w_img must be a contiguous CUDA float16 image of 2 x 9 x 1 x 64 x 8, b of 16 values")
    if out_f32 is not None and out_f32.numel() != out.numel():
        raise RuntimeError("rrdb_tail_u8: out_f32 must have one float per byte of out")
    check(lib.vsp_rrdb_tail_u8(_ptr(out), out.numel(), int(out_off), int(out_pitch), int(out_w), _ptr(out_f32), _ptr(info), _ptr(x), x_pitch,
                               H, W, int(keep0), int(keepn), _ptr(w_img), _ptr(b), _stream()), "rrdb_tail_u8")
    return out


# --------------------------------------------------------------------------------- face detection, ResNet-50
DET50_RELU = 1      # include/vspbfr_hip.h VSP_DET50_RELU


def _det50_act(t, name, need):
    if not isinstance(t, torch.Tensor) or not t.is_cuda or t.dtype != torch.float16 or t.dim() != 1 or not t.is_contiguous() or t.numel() < need:
        raise RuntimeError(f"{name} must be a flat contiguous CUDA float16 tensor of at least {need} elements")
    return t


def det50_out_size(H, W, stride):
    """(OH, OW) of a convolution of vsp_det50_conv_f16 (1x1 without, 3x3 with padding 1) and of the stem and the pool at stride 2"""
    return (int(H) - 1) // int(stride) + 1, (int(W) - 1) // int(stride) + 1


def det50_stem_u8(y, src, items, items_dev, n, w, b, B, Hc, Wc):
    """The ResNet-50 detector's stem on n u8 photos inside `src` (vsp_det50_stem_u8): writes images `slot` of y, a flat float16 buffer
    holding (B, ceil(Hc/2), ceil(Wc/2), 64), for the items of `items` (a _lib.DetSrc array; items_dev the same bytes on the device).
    w (147, 64), b (64) float32.  Returns y."""
    _u8(src, "src"), _u8(items_dev, "items_dev"), _req(w, "w"), _req(b, "b")
    B, Hc, Wc = int(B), int(Hc), int(Wc)
    oh, ow = det50_out_size(Hc, Wc, 2)
    _det50_act(y, "y", B * oh * ow * 64)
    if w.numel() != 147 * 64 or b.numel() != 64:
        raise RuntimeError(f"det50_stem_u8: w {tuple(w.shape)}, b {tuple(b.shape)}")
    if items_dev.numel() < n * C.sizeof(_lib.DetSrc):
        raise RuntimeError("det50_stem_u8: items_dev is shorter than the item table")
    check(lib.vsp_det50_stem_u8(_ptr(y), _ptr(src), src.numel(), C.cast(items, C.c_void_p), _ptr(items_dev), int(n), _ptr(w), _ptr(b), B, Hc,
                                Wc, _stream()), "det50_stem_u8")
    return y


def det50_pool_f16(y, x, B, H, W, C_):
    """3x3 / 2 / pad 1 max pool (vsp_det50_pool_f16): x holds (B, H, W, C_) float16, y takes (B, ceil(H/2), ceil(W/2), C_).  Returns y."""
    B, H, W, C_ = int(B), int(H), int(W), int(C_)
    oh, ow = det50_out_size(H, W, 2)
    _det50_act(x, "x", B * H * W * C_), _det50_act(y, "y", B * oh * ow * C_)
    check(lib.vsp_det50_pool_f16(_ptr(y), _ptr(x), B, H, W, C_, _stream()), "det50_pool_f16")
    return y


def det50_conv_f16(y, y_pitch, y_off, x, x_pitch, x_off, B, H, W, w_img, b, stride=1, relu=False, res=None, up=None):
    """One convolution of the ResNet-50 detector (vsp_det50_conv_f16): channels x_off .. x_off + Cin - 1 of x, a flat float16 buffer
    holding (B, H, W, x_pitch), -> channels y_off .. y_off + Cout - 1 of y, (B, OH, OW, y_pitch), as f16([relu](conv + b [+ res]) [+ up]).
    The filter (1x1, or 3x3 with padding 1) and the channel counts come from w_img, detect_r50.pack_conv_weight's image
    (taps, Cin / 32, Cout / 16, 64, 8); b float32 (Cout).  res: None or (flat float16 tensor, pitch, offset) at the output's size, which may
    be y's own window; up: None or (tensor, pitch, offset) of an (OH / 2, OW / 2) map read at (oy >> 1, ox >> 1).  Returns y."""
    B, H, W, y_pitch, y_off, x_pitch, x_off, stride = (int(v) for v in (B, H, W, y_pitch, y_off, x_pitch, x_off, stride))
    if not isinstance(w_img, torch.Tensor) or not w_img.is_cuda or w_img.dtype != torch.float16 or not w_img.is_contiguous() or w_img.dim() != 5 \
            or tuple(w_img.shape[3:]) != (64, 8) or int(w_img.shape[0]) not in (1, 9):
        raise RuntimeError("det50_conv_f16: w_img must be a contiguous CUDA float16 image (1 | 9, Cin / 32, Cout / 16, 64, 8)")
    ks, cin, cout = (1 if int(w_img.shape[0]) == 1 else 3), 32 * int(w_img.shape[1]), 16 * int(w_img.shape[2])
    _req(b, "b")
    if b.numel() != cout:
        raise RuntimeError(f"det50_conv_f16: {b.numel()} biases for {cout} channels")
    oh, ow = det50_out_size(H, W, stride) if stride in (1, 2) else (H, W)
    _det50_act(x, "x", B * H * W * x_pitch), _det50_act(y, "y", B * oh * ow * y_pitch)
    r = [None, 0, 0] if res is None else [_ptr(_det50_act(res[0], "res", B * oh * ow * int(res[1]))), int(res[1]), int(res[2])]
    u = [None, 0, 0] if up is None else [_ptr(_det50_act(up[0], "up", B * (oh // 2) * (ow // 2) * int(up[1]))), int(up[1]), int(up[2])]
    check(lib.vsp_det50_conv_f16(_ptr(y), y_pitch, y_off, _ptr(x), x_pitch, x_off, B, H, W, cin, cout, ks, stride, DET50_RELU if relu else 0,
                                 _ptr(w_img), _ptr(b), r[0], r[1], r[2], u[0], u[1], u[2], _stream()), "det50_conv_f16")
    return y


def det50_heads(x, x_pitch, B, H, W, w, b, conf, loc, lm, p0):
    """The class, box and landmark heads of one level (vsp_det50_heads_f32): channels 0 .. 255 of x, a flat float16 buffer holding
    (B, H, W, x_pitch); w (256, 32), b (32) float32 -> priors p0 .. p0 + 2 H W - 1 of conf (B, P, 2), loc (B, P, 4), lm (B, P, 10)."""
    for t, nm in ((w, "w"), (b, "b"), (conf, "conf"), (loc, "loc"), (lm, "lm")):
        _req(t, nm)
    B, H, W, x_pitch = int(B), int(H), int(W), int(x_pitch)
    _det50_act(x, "x", B * H * W * x_pitch)
    P = int(conf.shape[1]) if conf.dim() == 3 else -1
    if tuple(w.shape) != (256, 32) or tuple(b.shape) != (32,) or tuple(conf.shape) != (B, P, 2) or tuple(loc.shape) != (B, P, 4) \
            or tuple(lm.shape) != (B, P, 10):
        raise RuntimeError(f"det50_heads: w {tuple(w.shape)}, conf {tuple(conf.shape)}, loc {tuple(loc.shape)}, lm {tuple(lm.shape)} for a batch of {B}")
    check(lib.vsp_det50_heads_f32(_ptr(conf), _ptr(loc), _ptr(lm), _ptr(x), x_pitch, _ptr(w), _ptr(b), B, H, W, P, int(p0), _stream()), "det50_heads")


# --------------------------------------------------------------------------------- facial landmarks, 2D-FAN
FAN_RELU, FAN_OUT_F32 = 1, 2      # include/vspbfr_hip.h VSP_FAN_*


def _fan_win(t, name, n_pix, what="float16"):
    """(tensor, pitch, offset) -> [pointer, pitch, offset] of a channel window of a flat activation buffer; None -> [None, 0, 0]"""
    if t is None:
        return [None, 0, 0]
    buf, pitch, off = t[0], int(t[1]), int(t[2])
    dt = torch.float16 if what == "float16" else torch.float32
    if not isinstance(buf, torch.Tensor) or not buf.is_cuda or buf.dtype != dt or buf.dim() != 1 or not buf.is_contiguous() or buf.numel() < n_pix * pitch:
        raise RuntimeError(f"{name} must be a flat contiguous CUDA {what} tensor of at least {n_pix * pitch} elements")
    return [_ptr(buf), pitch, off]


def fan_stem_u8(y, src, box, w, b, side):
    """2D-FAN's stem on the boxes of B u8 photos (vsp_fan_stem_u8): src (B, H, W, 3) uint8, box (B, 3) float32 (x0, y0, s) ->
    y, a flat float16 buffer holding (B, side / 2, side / 2, 64).  w (147, 64), b (64) float32.  Returns y."""
    _u8(src, "src"), _req(box, "box"), _req(w, "w"), _req(b, "b")
    if src.dim() != 4 or src.shape[3] != 3 or not src.is_contiguous():
        raise RuntimeError(f"fan_stem_u8: src must be a contiguous (B, H, W, 3) uint8 tensor (got {tuple(src.shape)})")
    B, Hh, Ww, side = int(src.shape[0]), int(src.shape[1]), int(src.shape[2]), int(side)
    if tuple(box.shape) != (B, 3) or w.numel() != 147 * 64 or b.numel() != 64:
        raise RuntimeError(f"fan_stem_u8: box {tuple(box.shape)} for a batch of {B}, w {tuple(w.shape)}, b {tuple(b.shape)}")
    _det50_act(y, "y", B * (side // 2) * (side // 2) * 64)
    check(lib.vsp_fan_stem_u8(_ptr(y), _ptr(src), _ptr(box), _ptr(w), _ptr(b), B, Hh, Ww, side, _stream()), "fan_stem_u8")
    return y


def fan_pool_f16(y, x, B, H, W, C_):
    """2 x 2 mean (vsp_fan_pool_f16): channels of x = (flat float16 tensor, pitch, offset) holding (B, H, W, pitch) -> the window y of a
    (B, H / 2, W / 2, pitch) buffer, C_ channels.  Returns y's tensor."""
    B, H, W, C_ = int(B), int(H), int(W), int(C_)
    xs, ys = _fan_win(x, "x", B * H * W), _fan_win(y, "y", B * (H // 2) * (W // 2))
    check(lib.vsp_fan_pool_f16(ys[0], ys[1], ys[2], xs[0], xs[1], xs[2], B, H, W, C_, _stream()), "fan_pool_f16")
    return y[0]


def fan_conv_f16(y, x, B, H, W, w_img, cout, b=None, affine=None, relu=False, raw=None, res1=None, res2=None, up=None, out_f32=False):
    """One convolution of 2D-FAN (vsp_fan_conv_f16).  x, y, raw, res1, res2, up: (flat tensor, pitch, offset) channel windows of
    (B, H, W, pitch) buffers (up: (B, H / 2, W / 2, pitch)); all float16 except y with out_f32.  v = conv(x') [+ b] [relu], raw = f16(v),
    y = v [+ res1] [+ res2] [+ up]; x' = f16(relu(a x + b')) with affine = (a, b') float32 (Cin each).  w_img: fan.pack_conv_weight's float16
    image (1 | 9, Cin / 32, Cp / 16, 64, 8), Cp = cout rounded up to 32; b float32 (cout) or None.  Returns y's tensor."""
    B, H, W, cout = int(B), int(H), int(W), int(cout)
    if not isinstance(w_img, torch.Tensor) or not w_img.is_cuda or w_img.dtype != torch.float16 or not w_img.is_contiguous() or w_img.dim() != 5 \
            or tuple(w_img.shape[3:]) != (64, 8) or int(w_img.shape[0]) not in (1, 9) or int(w_img.shape[2]) != 2 * ((cout + 31) // 32):
        raise RuntimeError("fan_conv_f16: w_img must be a contiguous CUDA float16 image (1 | 9, Cin / 32, Cp / 16, 64, 8) for the channels stored")
    ks, cin = (1 if int(w_img.shape[0]) == 1 else 3), 32 * int(w_img.shape[1])
    if b is not None:
        _req(b, "b")
        if b.numel() != cout:
            raise RuntimeError(f"fan_conv_f16: {b.numel()} biases for {cout} channels")
    ia = ib = None
    if affine is not None:
        ia, ib = affine
        _req(ia, "affine a"), _req(ib, "affine b")
        if ia.numel() != cin or ib.numel() != cin:
            raise RuntimeError(f"fan_conv_f16: an affine of {ia.numel()} / {ib.numel()} values for {cin} input channels")
    n = B * H * W
    ys, xs = _fan_win(y, "y", n, "float32" if out_f32 else "float16"), _fan_win(x, "x", n)
    rw, r1, r2, u = _fan_win(raw, "raw", n), _fan_win(res1, "res1", n), _fan_win(res2, "res2", n), _fan_win(up, "up", B * (H // 2) * (W // 2))
    flags = (FAN_RELU if relu else 0) | (FAN_OUT_F32 if out_f32 else 0)
    check(lib.vsp_fan_conv_f16(ys[0], ys[1], ys[2], rw[0], rw[1], rw[2], xs[0], xs[1], xs[2], B, H, W, cin, cout, ks, flags, _ptr(w_img), _ptr(b),
                               _ptr(ia), _ptr(ib), r1[0], r1[1], r1[2], r2[0], r2[1], r2[2], u[0], u[1], u[2], _stream()), "fan_conv_f16")
    return y[0]


def fan_decode(hm, pitch, box, B, n, K=68):
    """Heatmaps -> landmarks (vsp_fan_decode_f32): hm a flat float32 buffer holding (B, n, n, pitch) with landmark k at channel k, box
    (B, 3) float32 -> (lm (B, K, 2) float32 in image pixels, peak (B, K) float32, flag (B, K) int32: the map held a non-finite value)"""
    _req(hm, "hm"), _req(box, "box")
    B, n, K, pitch = int(B), int(n), int(K), int(pitch)
    if hm.numel() < B * n * n * pitch or tuple(box.shape) != (B, 3):
        raise RuntimeError(f"fan_decode: hm of {hm.numel()} floats, box {tuple(box.shape)} for ({B}, {n}, {n}, {pitch})")
    lm = torch.empty((B, K, 2), device=hm.device, dtype=torch.float32)
    peak = torch.empty((B, K), device=hm.device, dtype=torch.float32)
    flag = torch.empty((B, K), device=hm.device, dtype=torch.int32)
    check(lib.vsp_fan_decode_f32(_ptr(lm), _ptr(peak), _ptr(flag), _ptr(hm), pitch, _ptr(box), B, n, K, _stream()), "fan_decode")
    return lm, peak, flag


def _guard_public_ops():
    """every public operator of this module runs under `device_guarded` (helpers without tensor arguments pass straight through)"""
    import types
    skip = {"conv_key", "conv_route", "fir_out_size", "fir_bf16_ok", "conv2d_out_size", "operand_device", "device_guarded", "check", "parse_conv_out",
            "fid_conv_out", "fid_pool_out", "det50_out_size"}
    g = globals()
    for name, obj in list(g.items()):
        if isinstance(obj, types.FunctionType) and not name.startswith("_") and name not in skip and obj.__module__ == __name__:
            g[name] = device_guarded(obj)


_guard_public_ops()
# PackedConv.form: kernel family -> its weight layout (the device-guarded builders)
WEIGHT_FORMS = {"wino": winograd_weight, "wino4": winograd4_weight, "wino4f": winograd4f_weight, "tconvw": tconvw_weight, "bf16": bf16_weight, "bf16x3": bf16x3_weight,
                "bf16rv": bf16rv_weight, "bf16dg": bf16dg_weight}
