"""GPU: vsp_pair_stats_u8 (vspbfr_amd/csrc/metrics.hip) against the float64 oracle tests/metrics_ref.py -- never against another
device computation.

Bounds (from the arithmetic, not from the kernel's results):
  sse       equal as integers.
  uniform7  |ssim - ref| <= 1e-6: the window sums are exact integers, the ratio at one position is ~10 fp32 roundings of 6e-8 on
            a value <= 1, the mean over positions cannot be worse and is accumulated in float64.
  gauss11   relative to plain arithmetic, as tests/test_tacc_kernels.py does: e_ref = |fp32 five-F.conv2d form on the CPU - ref|,
            e_hip = |kernel - ref| on the same pair; e_hip <= max(e_ref, 1e-6).  The kernel is asked to be at least as accurate as
            the form a user would write; centring the moments makes that easy.
Run with -s to see e_ref / e_hip / ratio per case (profiles/metrics_pr_gputest.log)."""
import ctypes as C

import numpy as np
import pytest
import torch

import metrics_ref as R

pytestmark = pytest.mark.gpu

KINDS = ("smooth", "bright_flat", "noise", "identical", "negative")
CASES = [(k, 512, 512, 3) for k in KINDS] + [
    ("smooth", 11, 11, 3), ("noise", 11, 11, 3), ("smooth", 67, 131, 3), ("noise", 67, 131, 3), ("bright_flat", 130, 65, 3),
    ("negative", 130, 65, 3), ("smooth", 1024, 1024, 3), ("bright_flat", 1024, 1024, 3),
    ("smooth", 512, 512, 1), ("bright_flat", 67, 131, 1), ("noise", 130, 65, 1), ("noise", 11, 11, 1)]
UNIFORM_ONLY = [("smooth", 7, 7, 3), ("noise", 7, 7, 1), ("bright_flat", 7, 10, 3)]


def _device(pairs):
    a = torch.from_numpy(np.stack([p[0] for p in pairs])).cuda()
    b = torch.from_numpy(np.stack([p[1] for p in pairs])).cuda()
    return a, b


def _stats(pairs, window):
    from vspbfr_amd import hip_ops as H
    a, b = _device(pairs)
    sse, ssim = H.pair_stats_u8(a, b, window)
    assert sse.dtype == torch.int64 and ssim.dtype == torch.float64 and sse.shape == ssim.shape == (len(pairs),)
    return sse.cpu().numpy(), ssim.cpu().numpy()


def _check(tag, pairs, window, sse, ssim):
    for i, (a, b) in enumerate(pairs):
        ref = R.ssim(a, b, window)
        e_hip = abs(float(ssim[i]) - ref)
        if window == "uniform7":
            print(f"{tag}[{i}] uniform7 ref {ref:+.9f} e_hip {e_hip:.2e} (bound 1e-6)")
            bound = 1e-6
        else:
            e_ref = abs(R.ssim_fp32_naive(a, b, window) - ref)
            bound = max(e_ref, 1e-6)
            print(f"{tag}[{i}] gauss11 ref {ref:+.9f} e_ref {e_ref:.2e} e_hip {e_hip:.2e} ratio {e_hip / max(e_ref, 1e-300):.3g}")
        assert int(sse[i]) == R.sse(a, b), (tag, i, int(sse[i]), R.sse(a, b))
        assert e_hip <= bound, (tag, i, window, float(ssim[i]), ref, e_hip, bound)


@pytest.mark.parametrize("window", ["uniform7", "gauss11"])
@pytest.mark.parametrize("kind,h,w,c", CASES, ids=lambda v: str(v))
def test_pair_stats_against_float64(kind, h, w, c, window):
    pairs = [R.pair(kind, h, w, c, seed=3)]
    sse, ssim = _stats(pairs, window)
    _check(f"{kind}-{h}x{w}x{c}", pairs, window, sse, ssim)


@pytest.mark.parametrize("kind,h,w,c", UNIFORM_ONLY, ids=lambda v: str(v))
def test_pair_stats_single_window(kind, h, w, c):
    pairs = [R.pair(kind, h, w, c, seed=4)]
    sse, ssim = _stats(pairs, "uniform7")
    _check(f"{kind}-{h}x{w}x{c}", pairs, "uniform7", sse, ssim)


@pytest.mark.parametrize("window", ["uniform7", "gauss11"])
@pytest.mark.parametrize("B,h,w", [(1, 512, 512), (5, 512, 512), (16, 512, 512), (5, 67, 131), (16, 130, 65)])
def test_pair_stats_batches(B, h, w, window):
    pairs = [R.pair(KINDS[i % len(KINDS)], h, w, 3, seed=10 + i) for i in range(B)]
    sse, ssim = _stats(pairs, window)
    _check(f"batch{B}-{h}x{w}", pairs, window, sse, ssim)


@pytest.mark.parametrize("window", ["uniform7", "gauss11"])
@pytest.mark.parametrize("h,w", [(512, 512), (67, 131)])
def test_bits_do_not_depend_on_batch_or_launch(h, w, window):
    """Image i alone, inside a batch of 16 at position 0 and at position 11, and on a second launch: identical bit patterns."""
    from vspbfr_amd import hip_ops as H
    me = R.pair("smooth", h, w, 3, seed=77)
    others = [R.pair(KINDS[i % len(KINDS)], h, w, 3, seed=200 + i) for i in range(16)]
    a1, b1 = _device([me])
    s1, q1 = H.pair_stats_u8(a1, b1, window)
    bits = (int(s1[0]), int(q1.view(torch.int64)[0]))
    for pos in (0, 11):
        batch = list(others)
        batch[pos] = me
        a, b = _device(batch)
        for launch in range(2):
            s, q = H.pair_stats_u8(a, b, window)
            assert (int(s[pos]), int(q.view(torch.int64)[pos])) == bits, (pos, launch)
    s2, q2 = H.pair_stats_u8(a1, b1, window)
    assert (int(s2[0]), int(q2.view(torch.int64)[0])) == bits
    assert int(s1[0]) == R.sse(*me)


@pytest.mark.parametrize("window", ["uniform7", "gauss11"])
def test_unaligned_base_pointers(window):
    """Odd row length (W * C = 393 bytes) and operands that start 1 and 3 bytes into their allocations: the first and the last dword of the
    byte stream straddle the tensors' ends."""
    from vspbfr_amd import hip_ops as H
    pairs = [R.pair("smooth", 67, 131, 3, seed=5), R.pair("noise", 67, 131, 3, seed=6)]
    n = 2 * 67 * 131 * 3
    bufa = torch.full((n + 1,), 255, dtype=torch.uint8, device="cuda")
    bufb = torch.full((n + 3,), 255, dtype=torch.uint8, device="cuda")
    a, b = bufa[1:].view(2, 67, 131, 3), bufb[3:].view(2, 67, 131, 3)
    a.copy_(torch.from_numpy(np.stack([p[0] for p in pairs])))
    b.copy_(torch.from_numpy(np.stack([p[1] for p in pairs])))
    assert a.data_ptr() % 4 == 1 and b.data_ptr() % 4 == 3 and a.is_contiguous()
    sse, ssim = H.pair_stats_u8(a, b, window)
    _check("unaligned", pairs, window, sse.cpu().numpy(), ssim.cpu().numpy())


def test_non_default_stream():
    from vspbfr_amd import hip_ops as H
    pairs = [R.pair("smooth", 130, 65, 3, seed=8)]
    a, b = _device(pairs)
    torch.cuda.synchronize()
    st = torch.cuda.Stream()
    with torch.cuda.stream(st):
        sse, ssim = H.pair_stats_u8(a, b, "gauss11")
    st.synchronize()
    _check("stream", pairs, "gauss11", sse.cpu().numpy(), ssim.cpu().numpy())


def test_refusals():
    from vspbfr_amd import _lib
    from vspbfr_amd import hip_ops as H
    a = torch.zeros(1, 16, 16, 3, dtype=torch.uint8, device="cuda")
    out = torch.zeros(4, dtype=torch.float64, device="cuda")
    p = lambda t: C.c_void_p(t.data_ptr())
    f = _lib.lib.vsp_pair_stats_u8
    assert f(p(out), p(out), p(a), p(a), 1, 6, 16, 3, _lib.WIN_UNIFORM7, p(out), None) == -1          # VSP_EINVAL: below the window
    assert f(p(out), p(out), p(a), p(a), 1, 16, 10, 3, _lib.WIN_GAUSS11, p(out), None) == -1
    assert f(p(out), p(out), p(a), p(a), 1, 16, 24, 2, _lib.WIN_GAUSS11, p(out), None) == -1          # C = 2
    with pytest.raises(RuntimeError, match="smaller than"):
        H.pair_stats_u8(a[:, :6].contiguous(), a[:, :6].contiguous(), "uniform7")
    with pytest.raises(RuntimeError, match="C must be 1 or 3"):
        H.pair_stats_u8(a[..., :2].contiguous(), a[..., :2].contiguous(), "gauss11")
    with pytest.raises(RuntimeError, match="one shape"):
        H.pair_stats_u8(a, a[:, :12].contiguous(), "gauss11")
    with pytest.raises(RuntimeError, match="contiguous"):
        H.pair_stats_u8(a[:, :, ::2], a[:, :, ::2], "gauss11")
    with pytest.raises(RuntimeError, match="uint8"):
        H.pair_stats_u8(a.float(), a.float(), "gauss11")
    with pytest.raises(RuntimeError, match="window"):
        H.pair_stats_u8(a, a, "box3")
    torch.cuda.synchronize()
    assert float(out.abs().sum()) == 0.0                                                             # a refused call writes nothing


def test_psnr_ssim_public_function():
    """Float images in [-1, 1] are scored as the uint8 images the PNG writer makes of them; uint8 input is taken as it is."""
    from vspbfr_amd import hip_ops as H
    from vspbfr_amd import metrics as M
    g = torch.Generator().manual_seed(3)
    x = (torch.rand(3, 3, 96, 80, generator=g) * 2.4 - 1.2).cuda()
    y = (x + 0.1 * torch.randn(3, 3, 96, 80, generator=g).cuda()).contiguous()
    y[2] = x[2]
    xa, ya = H.quantize_u8_nhwc(x).cpu().numpy(), H.quantize_u8_nhwc(y).cpu().numpy()
    for window in ("gauss11", "uniform7"):
        psnr, ssim = M.psnr_ssim(x, y, window)
        psnr8, ssim8 = M.psnr_ssim(torch.from_numpy(xa).cuda(), torch.from_numpy(ya).cuda(), window)
        assert torch.equal(psnr, psnr8) and torch.equal(ssim, ssim8)
        for i in range(3):
            ref, sref = R.psnr(xa[i], ya[i]), R.ssim(xa[i], ya[i], window)
            bound = 1e-6 if window == "uniform7" else max(abs(R.ssim_fp32_naive(xa[i], ya[i], window) - sref), 1e-6)
            assert abs(float(ssim[i]) - sref) <= bound
            if ref is None:
                assert torch.isinf(psnr[i]) and psnr[i] > 0 and abs(float(ssim[i]) - 1.0) < 1e-12
            else:
                assert abs(float(psnr[i]) - ref) < 1e-9
