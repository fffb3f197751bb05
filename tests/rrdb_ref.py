"""Real-ESRGAN's RRDBNet in plain torch on the CPU with exactly the rounding points of csrc/rrdb.hip: the reference of
tests/test_rrdb_ref.py, tests/test_rrdb_gpu.py and tests/test_rrdb_cli_gpu.py.  Written from the public model definition; the pixel
unshuffle, the reflection, the nearest x2, the crop and the quantisation are written out by index.

dtype = float64 is the reference, dtype = float32 its restatement: the bound of a device result is 4 e_ref + 2e-6 max|ref64| with e_ref
= max |float32 - float64| of the same case (the project's rule), plus half an f16 ulp for an f16 tensor, and 0.5 + 255 x that for a byte."""
import numpy as np
import torch
import torch.nn.functional as F

from vspbfr_amd import rrdb as R
from vspbfr_amd.upscale import plan_bands

SLOPE = 0.2


DEPTH_GAIN = 0.5


def make_state(num_block, scale, seed=0, gain=1.6):
    """a random checkpoint in the public layout: trunk and up convolutions N(0, gain / fan_in), biases N(0, 0.05^2), conv_last
    N(0, 0.05 / fan_in) with bias N(0.5, 0.05^2) -- with gain = 1.6 most outputs of a net of 1 .. 3 blocks lie strictly inside (0, 1).
    Over 23 blocks that gain lets the features grow to a standard deviation of 47 behind conv_up1 and only 6 % of the outputs stay
    unclamped (gain 1.2: 13 %, 1.0: 21 %, 0.8: 37 %, 0.5: 87 %, all on the CPU in float64), so the depth case takes DEPTH_GAIN = 0.5: the
    condition that at least half of a case's outputs are unclamped is what makes its comparison mean something."""
    g = torch.Generator().manual_seed(seed)
    sd = {}
    for key, shape in R.expected_state(num_block, scale).items():
        name, kind = key.rsplit(".", 1)
        if kind == "weight":
            var = (0.05 if name == "conv_last" else gain) / (9 * shape[1])
            sd[key] = torch.randn(shape, generator=g, dtype=torch.float64).mul(var ** 0.5).to(torch.float32)
        else:
            sd[key] = (torch.randn(shape, generator=g, dtype=torch.float64) * 0.05 + (0.5 if name == "conv_last" else 0.0)).to(torch.float32)
    return sd


def make_photo(h, w, seed=0):
    return np.random.default_rng(seed).integers(0, 256, (h, w, 3), dtype=np.uint8)


def q16(t, f16=True):
    """one rounding to f16"""
    return t.to(torch.float16).to(t.dtype) if f16 else t


def lrelu(v):
    return torch.where(v >= 0, v, SLOPE * v)


def unshuffle_by_index(x):
    """(h, w, C) -> (ceil(h / 2), ceil(w / 2), 4 C): the reflection of an odd last row / column (index h -> h - 2) and
    pixel_unshuffle(2), channel 4 c + 2 dy + dx"""
    h, w, C = x.shape
    nh, nw = (h + 1) // 2, (w + 1) // 2
    ys, xs = torch.arange(2 * nh), torch.arange(2 * nw)
    ys[ys >= h] = h - 2
    xs[xs >= w] = w - 2
    out = x.new_empty((nh, nw, 4 * C))
    for c in range(C):
        for dy in (0, 1):
            for dx in (0, 1):
                out[:, :, 4 * c + 2 * dy + dx] = x[ys[dy::2]][:, xs[dx::2], c]
    return out


def nearest2(x):
    """(1, C, H, W) -> (1, C, 2 H, 2 W) by index >> 1"""
    iy, ix = torch.arange(2 * x.shape[2]) >> 1, torch.arange(2 * x.shape[3]) >> 1
    return x[:, :, iy][:, :, :, ix]


class Net:
    """the network of a state dict at one dtype: f16 = True rounds weights (all but conv_first's) and activations as the kernels do"""

    def __init__(self, sd, dtype=torch.float64, f16=True):
        st = R.check_state_dict(sd)
        self.nb, self.scale, self.dtype, self.f16 = st.num_block, st.scale, dtype, f16
        self.w = {}
        for name in R.conv_names(self.nb):
            w, b = st.tensors[name + ".weight"], st.tensors[name + ".bias"]
            if f16 and name != "conv_first":
                w = w.to(torch.float16)
            self.w[name] = (w.to(dtype), b.to(dtype))

    def conv(self, name, x):
        return F.conv2d(x, *self.w[name], padding=1)

    def net_input(self, photo):
        x = torch.from_numpy(np.ascontiguousarray(photo)).to(self.dtype) / 255
        if self.scale == 2:
            x = unshuffle_by_index(x)
        return x.permute(2, 0, 1)[None]

    def trunk(self, photo):
        """u8 (h, w, 3) -> the 2x map behind conv_up1, (1, 64, 2 nh, 2 nw)"""
        q = lambda t: q16(t, self.f16)
        feat = q(self.conv("conv_first", self.net_input(photo)))
        f = feat
        for i in range(self.nb):
            d = f
            for j in (1, 2, 3):
                cat = d
                for k in (1, 2, 3, 4):
                    cat = torch.cat([cat, q(lrelu(self.conv(f"body.{i}.rdb{j}.conv{k}", cat)))], 1)
                v = SLOPE * self.conv(f"body.{i}.rdb{j}.conv5", cat) + d
                d = q(SLOPE * v + f) if j == 3 else q(v)
            f = d
        f = q(self.conv("conv_body", f) + feat)
        return q(lrelu(self.conv("conv_up1", nearest2(f))))

    def tail(self, u1):
        """the 2x map -> the unclamped output (4 rows per row pair ..., 3) as (H4, W4, 3)"""
        q = lambda t: q16(t, self.f16)
        f = q(lrelu(self.conv("conv_up2", nearest2(u1))))
        f = q(lrelu(self.conv("conv_hr", f)))
        return self.conv("conv_last", f)[0].permute(1, 2, 0)

    def tail_banded(self, u1, band_rows, halo):
        """tail() in bands of band_rows rows of the 2x map with `halo` rows on each inner side"""
        rows = []
        for r0, r1, a0, a1 in plan_bands(u1.shape[2], band_rows, halo):
            v = self.tail(u1[:, :, a0:a1])
            rows.append(v[2 * (r0 - a0):2 * (r1 - a0)])
        return torch.cat(rows, 0)

    def forward(self, photo, tail_band=None):
        """u8 (h, w, 3) -> the unclamped output (s h, s w, 3), s the scale, cropped for x2"""
        h, w = photo.shape[:2]
        u1 = self.trunk(photo)
        v = self.tail(u1) if tail_band is None else self.tail_banded(u1, *tail_band)
        return v[:self.scale * h, :self.scale * w]

    def forward_banded(self, photo, band_rows, halo):
        """forward() in bands of band_rows photo rows (even), each run on the photo rows of the band and `halo` more on each inner side"""
        s = self.scale
        rows = []
        for r0, r1, a0, a1 in plan_bands(photo.shape[0], band_rows, halo):
            v = self.forward(photo[a0:a1])
            rows.append(v[s * (r0 - a0):s * (r1 - a0)])
        return torch.cat(rows, 0)


def to_bytes(v):
    """clamp to [0, 1], rintf(255 v); a non-finite value is 0"""
    fin = torch.isfinite(v)
    b = torch.round(255 * torch.where(fin, v, torch.zeros_like(v)).clamp(0, 1))
    return b.to(torch.uint8).numpy()


_CASES = {}


def case(num_block, scale, h, w, seed=0):
    """(state dict, photo, float64 output, e_ref, byte bound) of a whole-net case, computed once and shared"""
    key = (num_block, scale, h, w, seed)
    if key not in _CASES:
        sd, photo = make_state(num_block, scale, seed, gain=1.6 if num_block <= 3 else DEPTH_GAIN), make_photo(h, w, seed + 100)
        ref = Net(sd, torch.float64).forward(photo)
        r32 = Net(sd, torch.float32).forward(photo)
        e_ref = float((r32.double() - ref).abs().max())
        bound = 4 * e_ref + 2e-6 * float(ref.abs().max())
        _CASES[key] = (sd, photo, ref, e_ref, 0.5 + 255 * bound)
    return _CASES[key]


def inside_share(ref):
    """the share of values strictly inside (0, 1)"""
    return float(((ref > 0) & (ref < 1)).double().mean())


def f16_half_ulp(ref):
    """half an f16 ulp at the magnitude of each value (normal range: 2^-11 of the power of two below; subnormal: 2^-25)"""
    a = ref.abs().double().clamp_min(2.0 ** -14)
    return torch.pow(2.0, torch.floor(torch.log2(a))) * 2.0 ** -11
