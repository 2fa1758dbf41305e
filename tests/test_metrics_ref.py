"""The CPU statements the csrc/metrics.hip tests rest on (tests/_metrics_ref.py), each pinned on the host before the device is asked.

* numpy's float32 summation, written out, equals np.add.reduce bit for bit at every pixel count tests/test_gpu_metrics.py uses, for
  one- and two-dimensional arrays.  If a numpy upgrade changes the summation, this is the test that fails.
* ssim_exact (exact integer window sums, correctly rounded per-pixel quotients, math.fsum) against the scipy restatement
  oracle.metrics_ref.ssim on every image maker: measured maximum difference 6.7e-13 (the diagonal ramp against its mirror image at
  7x200, where scipy's running float64 window sums cancel; 2.0e-13 at 45x71, at most 2.7e-14 on the other contents); bound 1e-12.
* the degenerate normalize_preds inputs: on x86-64 the reference's NaN -> uint8 cast gives byte 0 on exactly the sides the device
  contract names, and every non-degenerate input of the GPU tests runs through the oracle without a warning.
* the device's raw-byte float64 covariance for a prediction of another size, restated, stays inside the project's cap (<= 1 grey level
  on <= 0.5 % of the pixels) against the oracle on each shape the GPU test adds: measured 0 differing pixels on all four.
"""
import numpy as np
import pytest

import _metrics_ref as R


def _pixel_counts():
    shapes = [s[1:] for s in R.NORM_SHAPES] + [R.EDGE_SHAPE[1:], R.DEGENERATE_SHAPE[1:]]
    for hr_shape, hat_shape in R.RESIZED_SHAPES:
        shapes += [hr_shape[1:], hat_shape[1:]]
    return sorted(set(shapes), key=lambda s: (s[0] * s[1], s))


def test_chunked_pairwise_sum_is_numpys_float32_reduction():
    rng = np.random.default_rng(0)
    unchunked_differs = 0
    for shape in _pixel_counts():
        for scale in (1.0, 1e22):                                          # 1e22: the magnitudes pmin == pmax puts into the sums
            x = ((rng.random(shape) * 255 - 20) * scale).astype(np.float32)
            for arr in (x, x.ravel(), x.ravel()[None, :], x.ravel()[:, None]):
                got, want = R.chunked_pairwise_sum_f32(arr), np.add.reduce(arr, axis=None)
                assert got.dtype == want.dtype == np.float32
                assert got.view(np.uint32) == want.view(np.uint32), (shape, scale, arr.shape, got, want)
                assert np.mean(arr).view(np.uint32) == np.float32(got / np.float32(arr.size)).view(np.uint32)      # np.mean is this sum / n
            unchunked_differs += int(R._pairwise_f32(x.ravel()).view(np.uint32) != want.view(np.uint32))
    assert unchunked_differs > 0          # the pieces matter: one pairwise sum over the whole array is a different number somewhere


def test_tail_pieces_cover_every_branch():
    """The pixel counts hold: a tail shorter than 8 after full pieces, one of 8..128, one above 128 that is no multiple of 8, and
    single pieces of fewer than 8, exactly 128, 129 and 8191 / 8192 elements."""
    tails = {n: R.tail_of(n) for n in (s[1] * s[2] for s in R.NORM_SHAPES)}
    assert tails[8193] == (1, True) and tails[8199] == (7, True) and tails[8281] == (89, True) and tails[8320] == (128, True)
    assert tails[8327] == (135, True) and tails[10000] == (1808, True) and tails[16383] == (8191, True) and tails[32761] == (8185, True)
    assert tails[63300] == (5956, True) and tails[8192] == (8192, False) and tails[8191] == (8191, False)
    assert {2, 7, 9, 128, 129, 130, 136} <= set(tails)


@pytest.fixture(scope="module")
def ssim_errors():
    from oracle import metrics_ref as M
    errs = {}
    for shape in R.METRIC_SHAPES:
        for content in R.METRIC_CONTENTS:
            a, b = R.metric_pair(shape, content)
            errs[shape, content] = max(abs(R.ssim_exact(a[i], b[i]) - M.ssim(a[i], b[i])) for i in range(shape[0]))
    return errs


def test_ssim_exact_agrees_with_the_scipy_oracle(ssim_errors):
    worst = max(ssim_errors, key=ssim_errors.get)
    print(f"ssim_exact vs oracle.metrics_ref.ssim: max {ssim_errors[worst]:.3e} at {worst}")
    for key, err in ssim_errors.items():
        assert err <= 1e-12, (key, err)


def test_ssim_exact_against_fractions_and_known_values():
    from fractions import Fraction
    a, b = R.metric_pair((1, 12, 13), "saturated")
    num, den = R.ssim_terms_exact(a[0], b[0])
    mean = sum(Fraction(p, q) for p, q in zip(num.ravel().tolist(), den.ravel().tolist())) / num.size
    assert abs(Fraction(R.ssim_exact(a[0], b[0])) - mean) <= Fraction(1, 2 ** 52)
    x = R.random_image((9, 30), 1)
    assert R.ssim_exact(x, x) == 1.0 and R.ssd_exact(x, x) == 0
    # zeros against 255: means 0 and 255, no variance -> C1 / (255^2 + C1)
    assert R.ssim_exact(R.flat((7, 9), 0), R.flat((7, 9), 255)) == pytest.approx(6.5025 / (65025 + 6.5025), rel=1e-15)
    assert R.ssd_exact(R.flat((7, 9), 0), R.flat((7, 9), 255)) == 63 * 65025 and type(R.ssd_exact(x, x)) is int


def test_image_makers_are_seeded_and_shaped():
    s = (2, 40, 45)
    for make in (lambda: R.random_image(s, 3), lambda: R.sparse(s, 6, 255, 3), lambda: R.two_level(s, 3, 4, 3), lambda: R.saturated(s, 3),
                 lambda: R.saturated(s, 3, noise=20.0), lambda: R.gradient(s), lambda: R.blocks(s), lambda: R.flat(s, 9)):
        x = make()
        assert x.dtype == np.uint8 and x.shape == s and np.array_equal(x, make())
    assert [(img == 255).sum() for img in R.sparse(s, 6, 255, 3)] == [6, 6] and not np.array_equal(*R.random_image(s, 3))
    sat = R.saturated(s, 3)
    assert ((sat == 0) | (sat == 255)).mean() > 0.5 and 0 < (sat == 0).mean() < 1          # large clipped regions, both ends
    assert set(np.unique(R.two_level(s, 3, 4, 3))) == {3, 4} and set(np.unique(R.blocks(s, 250))) == {0, 250}
    g = R.gradient(s)
    assert g[0, 0, 0] == 0 and g[0, -1, -1] == 255 and (np.diff(g.astype(int), axis=-1) >= 0).all()


def test_non_degenerate_normalize_cases_run_through_the_oracle_without_a_warning():
    for shape in R.NORM_SHAPES:
        for content in R.NORM_CONTENTS:
            hr, hat = R.norm_pair(shape, content)
            assert len({img.tobytes() for img in hr}) == shape[0]                            # a different image per batch item
            for pcts in R.NORM_PERCENTILES:
                assert R.oracle_normalize(hr, hat, *pcts)[2] == [], (shape, content, pcts)
    hr, hat = R.edge_pair()
    for pcts in R.EDGE_PERCENTILES:
        a, b, caught = R.oracle_normalize(hr, hat, *pcts)
        assert caught == [] and a.std() > 10 and b.std() > 10, pcts
    for name, (hr, hat, percentiles) in R.distribution_pairs().items():
        for pcts in percentiles:
            a, b, caught = R.oracle_normalize(hr, hat, *pcts)
            assert caught == [] and a.max() > a.min() and b.max() > b.min(), (name, pcts)


def test_degenerate_normalize_cases_give_zero_bytes_on_this_host():
    """What the reference does on x86-64 for the inputs whose value is NaN: `invalid value` warnings and byte 0 on the sides that
    tests/test_gpu_metrics.py asserts to be 0 on the device; the other sides are ordinary images."""
    for name, (hr, hat, zero_hr, zero_hat) in R.degenerate_cases().items():
        a, b, caught = R.oracle_normalize(hr, hat)
        assert any("invalid value" in m for m in caught), name
        for i in range(R.DEGENERATE_SHAPE[0]):
            assert (not a[i].any()) == zero_hr[i] and (not b[i].any()) == zero_hat[i], (name, i)
            assert zero_hr[i] or a[i].std() > 10
            assert zero_hat[i] or b[i].std() > 10
    hr, hat, _ = R.distribution_pairs()["sparse50"]
    a, b, caught = R.oracle_normalize(hr, hat, 2.0, 98.0)                                     # the sparse image at the narrower percentiles
    assert caught and not a.any() and not b.any()


@pytest.mark.parametrize("hr_shape,hat_shape", R.RESIZED_SHAPES)
def test_raw_byte_covariance_restatement_stays_inside_the_cap(hr_shape, hat_shape):
    hr, hat = R.resized_pair(hr_shape, hat_shape)
    want_a, want_b, caught = R.oracle_normalize(hr, hat)
    assert caught == [] and want_b.std() > 10
    a, b = R.normalize_preds_raw_cov(hr, hat)
    np.testing.assert_array_equal(a, want_a)
    ok, figures = R.within_resized_cap(b, want_b)
    print(f"raw-byte covariance vs oracle {hr_shape} / {hat_shape}: max diff {figures[0]}, fraction {figures[1]:.2e}")
    assert ok, figures
