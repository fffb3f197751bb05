"""CPU: the float64 NIQE oracle (tests/niqe_ref.py) checked against independent statements of its parts."""
import numpy as np
from scipy import ndimage

import niqe_ref as R


def test_half_size_taps_come_from_the_cubic_kernel():
    t = R.half_taps_from_cubic()
    assert abs(t.sum() - 1.0) < 1e-15
    assert np.array_equal(t * 256.0, [-3, -9, 29, 111, 111, 29, -9, -3]) and np.array_equal(t, R.HALF_TAPS)


def test_half_size_image_boundary_and_order():
    rng = np.random.default_rng(0)
    x = rng.integers(0, 256, (12, 10)).astype(np.float64)
    got = R.imresize_half(x)
    assert got.shape == (6, 5)
    refl = lambda i, n: -1 - i if i < 0 else (2 * n - 1 - i if i >= n else i)   # noqa: E731  symmetric: -1 -> 0, n -> n - 1
    want = np.zeros((6, 5))
    for i in range(6):
        for j in range(5):
            want[i, j] = sum(R.HALF_TAPS[a] * R.HALF_TAPS[b] * x[refl(2 * i - 3 + a, 12), refl(2 * j - 3 + b, 10)] for a in range(8) for b in range(8))
    assert np.abs(got - want).max() < 1e-12
    assert np.abs(R.imresize_half(np.full((8, 8), 7.0)) - 7.0).max() < 1e-14


def test_window_sums_to_one_and_filter_is_scipys_nearest_correlation():
    w = R.gauss_window()
    assert abs(w.sum() - 1.0) < 1e-15 and np.abs(w - np.outer(R.gauss_taps(), R.gauss_taps())).max() < 1e-16
    x = np.random.default_rng(1).normal(100, 30, (40, 33))
    assert np.abs(R.gauss_filter(x) - ndimage.correlate(x, w, mode="nearest")).max() < 1e-12


def test_luma_is_exact_and_rounds_half_to_even():
    grey = np.arange(256, dtype=np.uint8)[:, None, None].repeat(3, 2)       # R = G = B = v: 16 + 219 v / 255
    y = R.luma(grey)[:, 0]
    for v in range(256):
        q, rem = divmod(219 * v, 255)
        assert y[v] == 16 + q + (1 if 2 * rem > 255 else 0)
    assert y[0] == 16 and y[255] == 235


def test_aggd_estimator_recovers_alpha_within_its_own_spread():
    """Samples of a generalised Gaussian of known shape: |v| = Gamma(1/alpha, 1)^(1/alpha) with a random sign.  The estimates over 20
    draws of 96^2 samples scatter around the truth; the mean must lie within 3 standard errors of it (plus the grid step)."""
    rng = np.random.default_rng(2)
    for alpha in (0.8, 2.0, 3.5):
        est = []
        for _ in range(20):
            v = rng.gamma(1.0 / alpha, 1.0, 96 * 96) ** (1.0 / alpha) * rng.choice([-1.0, 1.0], 96 * 96)
            _, a, bl, br = R.aggd_from(*R.smooth_of(v))
            est.append(a)
            assert abs(bl / br - 1.0) < 0.1
        est = np.array(est)
        assert abs(est.mean() - alpha) <= 3.0 * est.std(ddof=1) / np.sqrt(len(est)) + 0.001, (alpha, est.mean(), est.std())


def test_lookup_takes_the_first_minimum_of_a_monotone_table():
    assert (np.diff(R.R_GAM) > 0).all() and len(R.GAM) == 9801 and abs(R.GAM[-1] - 10.0) < 1e-12
    assert R.lookup(R.R_GAM[1234]) == 1234 and R.lookup(0.0) == 0 and R.lookup(1.0) == 9800
    mid = 0.5 * (R.R_GAM[500] + R.R_GAM[501])
    assert R.lookup(mid * (1 - 1e-9)) == 500 and R.lookup(mid * (1 + 1e-9)) == 501


def test_score_of_a_hand_computed_two_block_case():
    """Two blocks that differ in feature 0 only (1 and 3), model mean 0 and covariance 2 I - C, C = the blocks' own covariance: the pooled
    matrix is the identity, d = -(2, 1, ..., 1), the score sqrt(4 + 35)."""
    f = np.ones((2, 36))
    f[1, 0] = 3.0
    c = np.zeros((36, 36))
    c[0, 0] = 2.0                                                  # np.cov of (1, 3): ((1)^2 + (1)^2) / (2 - 1)
    assert np.array_equal(np.cov(f, rowvar=False), c)
    assert abs(R.score(f, np.zeros(36), 2.0 * np.eye(36) - c) - np.sqrt(39.0)) < 1e-12
    withnan = np.vstack([f, np.full((1, 36), np.nan)])
    assert R.score(withnan, np.zeros(36), 2.0 * np.eye(36) - c) == R.score(f, np.zeros(36), 2.0 * np.eye(36) - c)


def test_the_gpu_cases_keep_the_oracle_well_conditioned():
    """no MSCN or product sample of the GPU tests' inputs is within 1e-9 of zero, except in the half-constant case"""
    for kind, h, w in (("white", 96, 192), ("smooth", 192, 192), ("bright", 200, 301)):
        assert R.analyse(R.case_image(kind, h, w, 3))["tiny"] == 0
    half = R.analyse(R.case_image("half", 192, 384, 21))
    assert half["tiny"] > 0 and np.isnan(half["features"][[0, 4]]).any(axis=1).all() and np.isfinite(half["features"][[2, 3, 6, 7]]).all()
    img = R.case_image("bright", 192, 192, 17)
    ref = R.analyse(img)["smooth"]
    assert (np.abs(R.plain_fp32(img) - ref) / np.abs(ref)).max() > 1e-4      # the case that needs the shifted accumulation
