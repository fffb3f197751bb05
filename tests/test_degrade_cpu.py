"""CPU checks of the training degradation front end (vspbfr_amd/degrade.py, vspbfr_amd/trainset.py): the host kernel builder against
the reference's kernels, the parameter sampler against the reference's ranges, rank / world-size invariance of the draws, the dataset
listing, the C ABI's argument checks.  No GPU."""
import ctypes as C
import math
import os
import random

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HQ = os.path.join(ROOT, "tests", "golden", "loader_images", "hq")


def _crop(k41, K):
    o = (41 - K) // 2
    return k41[o:o + K, o:o + K]


def test_kernel_builder_bit_identical_to_reference(golden):
    from vspbfr_amd.degrade import bivariate_gaussian
    g = golden("degrade")
    for (K, sx, sy, th, iso), ref in zip(g["kernel_params"], g["kernels"]):
        K = int(K)
        k = bivariate_gaussian(K, sx, sy, th, bool(iso))
        assert k.dtype == np.float64 and k.shape == (K, K)
        assert np.array_equal(k, _crop(ref, K)), (K, sx, sy, th, iso)
        assert np.array_equal(np.pad(k, (41 - K) // 2), ref)     # nothing outside the window


def test_random_mixed_kernels_sequence(golden):
    """The reference's draw order (random.choices for the type, then np.random.uniform for sigma_x [, sigma_y, theta]) fed to the host
    builder reproduces `random_mixed_kernels` bit for bit."""
    from vspbfr_amd.degrade import bivariate_gaussian
    g = golden("degrade")
    for s, K, ref in zip(g["mixed_seeds"], g["mixed_ksize"], g["mixed_kernels"]):
        random.seed(int(s))
        np.random.seed(int(s))
        assert random.randint(19, 20) * 2 + 1 == K
        kind = random.choices(("iso", "aniso"), [0.5, 0.5])[0]
        sx = np.random.uniform(0.1, 10)
        if kind == "aniso":
            sy, th = np.random.uniform(0.1, 10), np.random.uniform(-math.pi, math.pi)
        else:
            sy, th = sx, 0
        k = bivariate_gaussian(int(K), sx, sy, th, kind == "iso")
        assert np.array_equal(k / np.sum(k), _crop(ref, int(K)))


def test_sampler_ranges_and_types():
    from vspbfr_amd.degrade import DegradeParams, sample_lq, sample_rng
    p = DegradeParams.free_form()
    n = 20000
    lqs = [sample_lq(p, (512, 512), sample_rng(7, 0, i, 1)) for i in range(n)]
    ks = np.array([q.ksize for q in lqs])
    assert set(ks) == {39, 41} and abs((ks == 41).mean() - 0.5) < 0.03
    qual = [q.quality for q in lqs]
    assert all(isinstance(v, int) for v in qual) and min(qual) == 60 and max(qual) == 99
    sc = np.array([q.scale for q in lqs])
    assert sc.min() >= 0.8 and sc.max() < 8.0
    assert all(q.size == (int(512 // q.scale), int(512 // q.scale)) for q in lqs)
    assert min(q.size[0] for q in lqs) == 64 and 630 <= max(q.size[0] for q in lqs) <= 640      # 512 // 8 .. 512 // 0.8
    iso = np.array([q.iso for q in lqs])
    assert abs(iso.mean() - 0.5) < 0.03
    assert all(q.sig_y == q.sig_x and q.theta == 0 for q in lqs if q.iso)
    sx = np.array([q.sig_x for q in lqs])
    th = np.array([q.theta for q in lqs if not q.iso])
    assert sx.min() >= 0.1 and sx.max() < 10 and th.min() >= -math.pi and th.max() < math.pi
    sig = np.array([q.sigma for q in lqs])
    assert sig.min() >= 0 and sig.max() < 20
    haze = np.array([q.haze for q in lqs])
    assert abs(haze.mean() - 0.008) < 4 * math.sqrt(0.008 * 0.992 / n)
    al = np.array([q.alpha for q in lqs if q.haze])
    assert al.min() >= 0.75 and al.max() < 0.95
    # ImageFolder_restore: no haze step
    r = DegradeParams.restore()
    assert not any(sample_lq(r, (256, 256), sample_rng(7, 0, i, 1)).haze for i in range(3000))
    # grey (slot 0 of a free-form sample) at 0.008
    from vspbfr_amd.trainset import ImageFolder_restore_free_form
    ds = ImageFolder_restore_free_form(HQ, im_size=(64, 64))
    grey = np.array([ds.draws(0, i, 3)[0] for i in range(n)])
    assert abs(grey.mean() - 0.008) < 4 * math.sqrt(0.008 * 0.992 / n)


def test_draws_are_pure_functions_of_the_key():
    from vspbfr_amd.degrade import DegradeParams, sample_lq, sample_rng
    p = DegradeParams.free_form()
    a = sample_lq(p, (512, 512), sample_rng(1, 2, 3, 1))
    np.random.seed(0)
    random.seed(0)
    b = sample_lq(p, (512, 512), sample_rng(1, 2, 3, 1))
    assert a == b
    assert sample_lq(p, (512, 512), sample_rng(1, 2, 3, 2)) != a
    assert sample_lq(p, (512, 512), sample_rng(1, 2, 4, 1)) != a
    assert sample_lq(p, (512, 512), sample_rng(1, 3, 3, 1)) != a


@pytest.mark.parametrize("world", [2, 4])
def test_draws_identical_at_every_world_size(world):
    """A sample gets the same crop / flip / grey / degradation whichever rank serves it: the ranks' shards cover the epoch
    (DistributedSampler's padding repeats the first indices), and every sample's draws and decoded crop through each rank's loader
    equal those of the single-rank loader."""
    from vspbfr_amd.trainset import DegradeLoader, ImageFolder_restore_free_form
    ds = ImageFolder_restore_free_form(HQ, im_size=(64, 64))
    one = DegradeLoader(ds, 2, device="cpu", seed=5)
    ranks = [DegradeLoader(ds, 2, device="cpu", seed=5, rank=r, world_size=world) for r in range(world)]
    for epoch in (0, 1):
        order = one.indices(epoch)
        assert sorted(order) == list(range(len(ds)))
        parts = [ld.indices(epoch) for ld in ranks]
        assert all(len(p) == math.ceil(len(ds) / world) for p in parts)
        assert set(np.concatenate(parts)) == set(order)
        for ld, part in zip(ranks, parts):
            for idx in part:
                g1, l1, img1 = ld._decode(epoch, int(idx))
                g0, l0, img0 = one._decode(epoch, int(idx))
                assert g1 == g0 and l1 == l0 and np.array_equal(img1, img0)
    assert not np.array_equal(one.indices(0), one.indices(1)) or len(ds) < 3


def test_dataset_listing_and_layout():
    from vspbfr_amd.degrade import DegradeParams, sample_rng
    from vspbfr_amd.imageio import list_images
    from vspbfr_amd.trainset import ImageFolder_restore, ImageFolder_restore_free_form
    for cls, n_lq in ((ImageFolder_restore_free_form, 2), (ImageFolder_restore, 1)):
        ds = cls(HQ, transform=None, im_size=(64, 48))
        assert ds.frame == list_images(HQ) and len(ds) == 4 and ds.im_size == (64, 48)
        grey, lqs, rng = ds.draws(0, 1)
        assert len(lqs) == n_lq
        img = ds.load(1, rng)
        assert img.shape == (64, 48, 3) and img.dtype == np.uint8
    assert ImageFolder_restore_free_form.params == DegradeParams.free_form()
    assert ImageFolder_restore.params == DegradeParams.restore() and ImageFolder_restore.params.gray_prob == 0
    # ImageFolder_restore does not flip: the same crop draw gives the same pixels as a plain PIL cover-resize + crop
    from PIL import Image
    ds = ImageFolder_restore(HQ, im_size=(64, 64))
    for i in range(len(ds)):
        img = Image.open(ds.frame[i]).convert("RGB")
        w, h = img.size
        if (h, w) == (64, 64):
            assert np.array_equal(ds.load(i, sample_rng(0, 0, i, 0)), np.asarray(img))


def test_degrade_entry_points_refuse_bad_arguments_without_a_gpu():
    from vspbfr_amd import _lib
    lib = _lib.lib
    assert lib.vsp_struct_size(6) == C.sizeof(_lib.DegradeItem) == 72
    p = C.c_void_p(256)   # non-null dummy: never dereferenced on these paths
    assert lib.vsp_degrade_gt_f32(p, p, p, None, 1, 8, 8, None) == -1 and "exactly one" in _lib.last_error()
    assert lib.vsp_degrade_gt_f32(p, p, None, None, 1, 0, 8, None) == -1 and "bad shape" in _lib.last_error()
    assert lib.vsp_degrade_blur_f32(None, p, p, p, 2, 1, 8, 8, None) == -1 and "null" in _lib.last_error()
    assert lib.vsp_degrade_blur_f32(p, p, p, p, _lib.DEGRADE_MAX_ITEMS + 1, 1, 8, 8, None) == -1 and "items" in _lib.last_error()
    assert lib.vsp_degrade_blur_f32(p, p, p, p, 1, 1, 8, _lib.DEGRADE_MAX_SIZE + 1, None) == -1
    assert lib.vsp_degrade_down_u8(p, None, p, None, p, 1, 8, 8, 0, 0, 0, None) == -1 and "max_pixels" in _lib.last_error()
    assert lib.vsp_degrade_down_u8(p, None, p, None, p, 1, 8, 8, 16, 0, -1, None) == -1 and "step" in _lib.last_error()
    assert lib.vsp_degrade_down_u8(p, None, None, None, p, 1, 8, 8, 16, 0, 0, None) == -1 and "null" in _lib.last_error()
    assert lib.vsp_degrade_jpeg_u8(p, None, p, 1, 4, 64, None) == -1 and "null" in _lib.last_error()
    assert lib.vsp_degrade_jpeg_u8(p, p, p, 1, -1, 64, None) == -1
    assert lib.vsp_degrade_up_f32(p, p, p, -1, 8, 8, None) == -1
    assert lib.vsp_degrade_up_f32(None, p, p, 1, 8, 8, None) == -1 and "null" in _lib.last_error()
    # empty batches are no-ops
    assert lib.vsp_degrade_up_f32(None, None, None, 0, 8, 8, None) == 0


def test_plan_checks_and_layout():
    from vspbfr_amd.degrade import DegradePlan, LQParams
    a = LQParams(41, True, 2.0, 2.0, 0.0, 2.0, (32, 24), 5.0, 75)
    b = LQParams(3, False, 1.0, 2.0, 0.5, 1.0, (64, 64), 0.0, 60, haze=True, alpha=0.8)
    plan = DegradePlan([a, b], [0, 0], (64, 64), 1, samples=[5, 5], slots=[1, 2], grey=[False, True])
    assert plan.n == 2 and plan.lq_elems == 3 * (32 * 24 + 64 * 64) and plan.max_pixels == 64 * 64
    assert plan.total_mcus == 2 * 2 + 4 * 4 and plan.work_bytes == 32 * 32 * 3 // 2 + 64 * 64 * 3 // 2
    it = plan.items
    assert (it[0].tap_off, it[1].tap_off, it[1].pix_off, it[1].mcu0, it[1].jpg_off) == (0, 41 * 41, 3 * 32 * 24, 4, 32 * 32 * 3 // 2)
    assert it[1].flags == 3 and it[0].flags == 0 and it[1].slot == 2 and it[0].sample == 5
    assert plan.taps.dtype == np.float32 and plan.taps.size == 41 * 41 + 9 and abs(plan.taps[:41 * 41].sum() - 1) < 1e-5
    for bad in (LQParams(40, True, 1, 1, 0, 1, (8, 8), 0, 75), LQParams(43, True, 1, 1, 0, 1, (8, 8), 0, 75),
                LQParams(3, True, 1, 1, 0, 1, (0, 8), 0, 75), LQParams(3, True, 1, 1, 0, 1, (8, 8), 0, 0)):
        with pytest.raises(ValueError):
            DegradePlan([bad], [0], (64, 64), 1)
    with pytest.raises(ValueError):
        DegradePlan([a], [1], (64, 64), 1)
