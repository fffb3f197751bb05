"""GPU checks of the training degradation chain (csrc/degrade.hip through vspbfr_amd/degrade.py and vspbfr_amd/trainset.py): every stage
against its oracle on the same inputs (tests/degrade_ref.py restates the OpenCV operations in float64; PIL's libjpeg-turbo and the
committed PIL fixtures stand in for cv2's JPEG codec), the whole chain end to end, ragged batches against one-by-one runs, repeat
launches, and the dataset iterator feeding one training step."""
import os

import numpy as np
import pytest
import torch

from degrade_ref import bgr2gray, degrade_chain, filter2d, jpeg_cv2, philox_normals, resize_linear, round_u8

pytestmark = pytest.mark.gpu
DEV = "cuda"
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HQ = os.path.join(ROOT, "tests", "golden", "loader_images", "hq")


def _lq(size, quality=75, sigma=0.0, taps=None, ksize=None, haze=False, alpha=1.0, scale=1.0):
    from vspbfr_amd.degrade import LQParams
    taps = np.ones((1, 1), np.float32) if taps is None and ksize is None else taps
    k = ksize if taps is None else taps.shape[0]
    return LQParams(k, True, 2.0, 2.0, 0.0, scale, tuple(size), sigma, quality, haze, alpha, taps)


def _smooth(rng, B, H, W):
    """face-like inputs: a smooth field + texture, in [0, 1], float32"""
    y, x = np.mgrid[0:H, 0:W]
    base = np.stack([0.5 + 0.3 * np.sin(x / (5.0 + c) + rng.random() * 6) * np.cos(y / (7.0 + c)) for c in range(3)])
    return np.clip(base[None] + 0.08 * rng.standard_normal((B, 3, H, W)), 0, 1).astype(np.float32)


def _plan(lqs, src, im_size, B, **kw):
    from vspbfr_amd.degrade import DegradePlan
    plan = DegradePlan(lqs, src, im_size, B, **kw)
    return plan, plan.upload(DEV)


def test_blur_matches_float64_correlation():
    """K in {3, 39, 41} with different (non-symmetric) taps per item in one launch, odd map sizes, a map smaller than the kernel
    (reflect-101 more than once), the haze epilogue: <= 2e-6 of float64 correlation with the same fp32 taps."""
    from vspbfr_amd import hip_ops as H
    from vspbfr_amd.degrade import bivariate_gaussian
    rng = np.random.default_rng(1)
    for (Hh, Ww) in ((77, 133), (17, 23)):
        gt = _smooth(rng, 2, Hh, Ww)
        t3 = rng.random((3, 3)).astype(np.float32)
        t3 /= t3.sum()
        t39 = bivariate_gaussian(39, 6.0, 1.5, 0.7, False).astype(np.float32)
        t41 = (rng.random((41, 41)) * bivariate_gaussian(41, 4.0, 4.0, 0, True)).astype(np.float32)
        t41 /= t41.sum()
        lqs = [_lq((8, 8), taps=t3), _lq((8, 8), taps=t39), _lq((8, 8), taps=t41), _lq((8, 8), taps=t41, haze=True, alpha=0.8)]
        src = [0, 1, 1, 0]
        plan, (items, taps) = _plan(lqs, src, (Hh, Ww), 2)
        out = H.degrade_blur(torch.from_numpy(gt).to(DEV), taps, items, plan.n).cpu().numpy()
        for i, (p, s) in enumerate(zip(lqs, src)):
            ref = np.stack([filter2d(gt[s, c], p.taps) for c in range(3)])
            if p.haze:
                ref = ref * 0.8 + 0.2
            err = np.abs(out[i] - ref).max()
            assert err <= 2e-6, (Hh, Ww, p.ksize, err)


def test_downsample_noise_and_u8():
    """INTER_LINEAR down at scales 0.8, 1, 2, 3.7, 8 (non-square): <= 1e-6 before the noise; the uint8 image equals
    round-half-even(clip(pre + z sigma / 255) * 255) for injected noise and for the kernel's own Philox draw restated on the host
    (away from rounding ties, where float32 and float64 may round apart)."""
    from vspbfr_amd import hip_ops as H
    rng = np.random.default_rng(2)
    Hh, Ww = 96, 160
    gt = _smooth(rng, 1, Hh, Ww)
    scales = [0.8, 1.0, 2.0, 3.7, 8.0]
    sizes = [(int(Hh // s), int(Ww // s)) for s in scales]
    lqs = [_lq(sz, sigma=12.5, scale=s) for sz, s in zip(sizes, scales)]
    plan, (items, taps) = _plan(lqs, [0] * 5, (Hh, Ww), 1, samples=[11, 12, 13, 14, 15], slots=[1, 2, 1, 2, 1])
    g = torch.from_numpy(gt).to(DEV)
    blurred = H.degrade_blur(g, taps, items, plan.n)
    assert torch.equal(blurred[0], g[0])                                            # 1 x 1 unit taps
    z = [rng.standard_normal((dh, dw, 3)).astype(np.float32) for dh, dw in sizes]
    from vspbfr_amd.degrade import pack_noise
    lq_inj, pre = H.degrade_down(blurred, items, plan.n, plan.lq_elems, plan.max_pixels, 0, 0, noise=pack_noise(plan, z, DEV), pre=True)
    lq_key = H.degrade_down(blurred, items, plan.n, plan.lq_elems, plan.max_pixels, 1234, 5)
    pre_l, inj_l, key_l = plan.split(pre.cpu()), plan.split(lq_inj.cpu()), plan.split(lq_key.cpu())
    for i, (dh, dw) in enumerate(sizes):
        ref = resize_linear(gt[0], dh, dw)
        p = pre_l[i].numpy().transpose(2, 0, 1)
        assert np.abs(p - ref).max() <= 1e-6, (scales[i], np.abs(p - ref).max())
        for got, zz in ((inj_l[i], z[i]),
                        (key_l[i], philox_normals(1234, 5, plan.items[i].slot, plan.items[i].sample, dh * dw * 3)[0].reshape(dh, dw, 3))):
            x = np.clip(p.astype(np.float64) + zz.transpose(2, 0, 1).astype(np.float64) * (np.float32(12.5) / np.float32(255)), 0, 1) * 255
            want = round_u8(x)
            tie = np.abs(x - np.floor(x) - 0.5) < 1e-3
            bad = (got.numpy() != want) & ~tie
            assert not bad.any(), (scales[i], int(bad.sum()))
            assert (got.numpy() != want).mean() < 1e-3


def test_jpeg_bit_identical_to_pil_goldens(golden):
    """The committed PIL round trips (all sizes and qualities in ONE ragged launch), bit for bit."""
    from vspbfr_amd import hip_ops as H
    g = golden("degrade")
    cases = []
    for k in g:
        if k.startswith("jpeg_out_"):
            size, q = k[len("jpeg_out_"):].split("_q")
            cases.append((size, int(q), g["jpeg_in_" + size], g[k]))
    assert len(cases) >= 17
    lqs = [_lq(img.shape[:2], quality=q) for _, q, img, _ in cases]
    plan, (items, _) = _plan(lqs, [0] * len(lqs), (8, 8), 1)
    flat = torch.cat([torch.from_numpy(np.ascontiguousarray(img.transpose(2, 0, 1))).reshape(-1) for _, _, img, _ in cases]).to(DEV)
    H.degrade_jpeg(flat, items, plan.n, plan.total_mcus, plan.work_bytes, plan.max_pixels)
    for (size, q, _, want), got in zip(cases, plan.split(flat.cpu())):
        got = got.numpy().transpose(1, 2, 0)
        assert np.array_equal(got, want), (size, q, int((got != want).sum()))


def test_jpeg_bit_identical_to_live_pil():
    from vspbfr_amd import hip_ops as H
    pytest.importorskip("PIL")
    rng = np.random.default_rng(3)
    shapes = [(37, 300), (129, 64), (64, 65), (203, 131), (640, 512), (1, 7), (2, 2)]
    quals = [60, 77, 99, 61, 90, 75, 60]
    imgs = [np.clip(_smooth(rng, 1, h, w)[0] * 255, 0, 255).round().astype(np.uint8) for h, w in shapes]
    plan, (items, _) = _plan([_lq(s, quality=q) for s, q in zip(shapes, quals)], [0] * len(shapes), (8, 8), 1)
    flat = torch.cat([torch.from_numpy(im).reshape(-1) for im in imgs]).to(DEV)
    H.degrade_jpeg(flat, items, plan.n, plan.total_mcus, plan.work_bytes, plan.max_pixels)
    for im, q, got in zip(imgs, quals, plan.split(flat.cpu())):
        want = jpeg_cv2(im, q)
        assert np.array_equal(got.numpy(), want), (im.shape, q, int((got.numpy() != want).sum()))


def test_upsample_and_final_rounding():
    """uint8 -> INTER_LINEAR up -> round: exact multiples of 1/255; at most 0.1 % of the pixels one step off the restatement in cv2's
    float32 operation order and none more (an exact 2x enlargement puts x * 255 on .5 ties, which only the float32 order decides), within
    one step of the float64 restatement everywhere; grey items equal BGR2GRAY of the colour result."""
    from vspbfr_amd import hip_ops as H
    rng = np.random.default_rng(4)
    Hh, Ww = 128, 96
    sizes = [(int(Hh // s), int(Ww // s)) for s in (0.8, 1.0, 2.0, 3.7, 8.0)]
    imgs = [np.clip(_smooth(rng, 1, h, w)[0] * 255, 0, 255).round().astype(np.uint8) for h, w in sizes]
    lqs = [_lq(s) for s in sizes] + [_lq(sizes[3])]
    imgs.append(imgs[3])
    plan, (items, _) = _plan(lqs, [0] * len(lqs), (Hh, Ww), 1, grey=[False] * 5 + [True])
    flat = torch.cat([torch.from_numpy(im).reshape(-1) for im in imgs]).to(DEV)
    out = H.degrade_up(flat, items, plan.n, Hh, Ww).cpu().numpy()
    k = out[:5] * 255
    assert np.array_equal(out[:5], (np.rint(k) / np.float32(255)).astype(np.float32))
    for i in range(5):
        src = imgs[i].astype(np.float32) / np.float32(255)
        ref32 = round_u8(resize_linear(src, Hh, Ww, f32=True) * np.float32(255))
        d = np.abs(np.rint(k[i]) - ref32)
        assert d.max() <= 1 and (d > 0).mean() <= 1e-3, (sizes[i], d.max(), (d > 0).mean())
        assert np.abs(np.rint(k[i]) - round_u8(resize_linear(src, Hh, Ww) * 255)).max() <= 1
    assert np.abs(out[5] - bgr2gray(out[3])[None]).max() <= 1e-6
    assert np.array_equal(out[5][0], out[5][1]) and np.array_equal(out[5][0], out[5][2])


def test_end_to_end_with_injected_parameters_and_noise():
    """The whole chain with reference-distributed parameters and injected normals against the float64 restatement + PIL: <= 1 LSB on
    >= 99.9 % of the pixels (a pre-JPEG pixel that rounds the other way moves its 8 x 8 block, hence the tail)."""
    from vspbfr_amd.degrade import DegradeParams, degrade, sample_lq, sample_rng
    rng = np.random.default_rng(5)
    Hh = Ww = 128
    gt = _smooth(rng, 2, Hh, Ww)
    p = DegradeParams.free_form()
    lqs = [sample_lq(p, (Hh, Ww), sample_rng(9, 0, i, 1)) for i in range(6)]
    lqs[2].haze, lqs[2].alpha = True, 0.85
    z = [rng.standard_normal((q.size[0], q.size[1], 3)).astype(np.float32) for q in lqs]
    src = [0, 1, 0, 1, 0, 1]
    out = degrade(torch.from_numpy(gt).to(DEV), lqs, src=src, noise=z).cpu().numpy()
    worst = []
    for i, q in enumerate(lqs):
        ref = degrade_chain(gt[src[i]], q, z[i])
        d = np.abs(np.rint(out[i] * 255) - np.rint(ref * 255))
        frac = (d > 1).mean()
        worst.append((frac, float(d.mean())))
        assert frac <= 1e-3, (i, q, frac, d.max())
    print("end-to-end mean |delta| per image (LSB):", [round(m, 5) for _, m in worst])


def test_ragged_batch_equals_one_by_one_and_repeats():
    """8 images at 8 scales and qualities in one call equal the same images degraded one call each (Philox noise keyed per item),
    bit for bit; 20 repeats of a B = 4 free-form batch at 512^2 are bit-identical, blur stage included."""
    from vspbfr_amd.degrade import DegradeParams, DegradePlan, degrade, run_plan, sample_lq, sample_rng
    rng = np.random.default_rng(6)
    Hh = Ww = 128
    gt = torch.from_numpy(_smooth(rng, 4, Hh, Ww)).to(DEV)
    p = DegradeParams.free_form()
    lqs = [sample_lq(p, (Hh, Ww), sample_rng(3, 1, i, 1)) for i in range(8)]
    for i, (s, q) in enumerate(zip((0.8, 1.0, 1.7, 2.0, 3.3, 4.5, 6.1, 8.0), (60, 65, 70, 75, 80, 88, 93, 99))):
        lqs[i].scale, lqs[i].size, lqs[i].quality = s, (int(Hh // s), int(Ww // s)), q
    src, samples, slots = [i % 4 for i in range(8)], [100 + i % 4 for i in range(8)], [1 + i // 4 for i in range(8)]
    both = degrade(gt, lqs, src=src, seed=77, step=3, samples=samples, slots=slots)
    for i in range(8):
        one = degrade(gt[src[i]:src[i] + 1], [lqs[i]], src=[0], seed=77, step=3, samples=[samples[i]], slots=[slots[i]])
        assert torch.equal(one[0], both[i]), i
    # repeats at the production shape
    g512 = torch.from_numpy(_smooth(rng, 4, 512, 512)).to(DEV)
    lqs = [sample_lq(p, (512, 512), sample_rng(3, 2, i % 4, 1 + i // 4)) for i in range(8)]
    plan = DegradePlan(lqs, [i % 4 for i in range(8)], (512, 512), 4, samples=list(range(8)), slots=[1 + i // 4 for i in range(8)])
    first, st0 = run_plan(plan, g512, seed=1, step=2, stages=True)
    for _ in range(20):
        again, st = run_plan(plan, g512, seed=1, step=2, stages=True)
        assert torch.equal(again, first) and torch.equal(st["blurred"], st0["blurred"])


def test_free_form_iterator_feeds_a_training_step():
    """ImageFolder_restore_free_form over the loader fixtures at 64^2: (lq1, lq2, gt) on the device with the reference's shapes and
    ranges, gt = the decoded crop / 255, and one RestorationTrainer.step on (lq1 * 2 - 1, gt * 2 - 1) gives finite losses;
    ImageFolder_restore yields (lq float, gt uint8)."""
    import copy

    from oracle import cases, weights
    from vspbfr_amd.discriminator import Discriminator
    from vspbfr_amd.restorenet import Restoration_net
    from vspbfr_amd.train_step import RestorationTrainer
    from vspbfr_amd.trainset import DegradeLoader, ImageFolder_restore, ImageFolder_restore_free_form
    size, B = 64, 4
    ds = ImageFolder_restore_free_form(HQ, im_size=(size, size))
    loader = DegradeLoader(ds, B, device=DEV, seed=4)
    idx = loader.indices(0)[:B]
    lq1, lq2, gt = next(iter(loader))
    for t in (lq1, lq2, gt):
        assert t.shape == (B, 3, size, size) and t.dtype == torch.float32 and t.is_cuda
        assert float(t.min()) >= 0 and float(t.max()) <= 1
    for b, i in enumerate(idx):
        grey, _, rng = ds.draws(0, int(i), 4)
        img = ds.load(int(i), rng)
        if not grey:
            assert torch.equal(gt[b].cpu(), torch.from_numpy(img.astype(np.float32) / np.float32(255)).permute(2, 0, 1))
            assert torch.equal(lq1[b] * 255, torch.round(lq1[b] * 255))
    assert not torch.equal(lq1, lq2)
    rs = DegradeLoader(ImageFolder_restore(HQ, im_size=(size, size)), 2, device=DEV)
    lq, gtu = next(iter(rs))
    assert lq.shape == (2, 3, size, size) and lq.dtype == torch.float32 and gtu.shape == (2, 3, size, size) and gtu.dtype == torch.uint8
    sd = weights.synth_state_dict("restorenet", weights.load_specs()["restorenet64"], cases.SEED)
    G = Restoration_net(size, 512, 8)
    G.load_state_dict(sd, strict=True)
    G = G.to(DEV).eval()
    D = Discriminator(size)
    D.load_state_dict(weights.synth_state_dict("discriminator", weights.load_specs()["discriminator64"], cases.SEED), strict=True)
    D = D.to(DEV).eval()
    tr = RestorationTrainer(G, copy.deepcopy(G), D, mixing=0.0)
    de = [cases.tensor("train", f"de_feat{k}", (B, 512, 2 ** (k + 2), 2 ** (k + 2)), 0.5).to(DEV) for k in range(5)]
    lat = cases.tensor("train", "latent", (B, 18, 512)).to(DEV)
    with torch.enable_grad():
        losses = tr.step(0, lq1 * 2.0 - 1, gt * 2.0 - 1, de_feats=de, latent=lat)
    assert all(torch.isfinite(torch.as_tensor(v)).all() for v in losses.values()), losses
