"""normalize_preds on the device (csrc/metrics.hip) vs the reference's own outputs (tests/golden/metrics.npz) and,
at sizes the fixtures do not hold, vs the pinned numpy restatement (oracle/metrics_ref.py): bit-exact uint8.  The image metrics
against exact values (tests/_metrics_ref.py, whose statements tests/test_metrics_ref.py pins on the host).

Pixel counts of the chunk-tail test (numpy sums float32 in pieces of 8192 elements; "tail" is the last piece, "+" means full pieces
come before it), each with three contents (correlated, anti-correlated = 255 - hr, saturated) at percentiles (0.1, 99.9) and (2, 98):
    one piece     2, 7 (left to right, n < 8); 9 (8 accumulators + 1); 128 (one full leaf); 129 = 64 + 65, 130 = 64 + 66, 136 = 64 + 72
                  (first split); 8191 (uneven splits all the way down); 8192 (exactly one piece)
    tail < 8      8193 = 8192 + 1, 8199 = 8192 + 7
    tail 8..128   8281 = 8192 + 89 (89 % 8 = 1), 8320 = 8192 + 128
    tail > 128    8327 = 8192 + 135 (135 % 8 = 7), 10000 = 8192 + 1808, 16383 = 8192 + 8191, 32761 = 3 * 8192 + 8185 (8185 % 8 = 1),
                  63300 = 7 * 8192 + 5956 (5956 % 8 = 4)
The prediction of another size adds 3600 / 9000, 4500 / 7200 (single pieces) and 8281 / 32761 both ways (a tail on either reduction).

Degenerate contract (header of csrc/metrics.hip, ops.normalize_preds_u8): a side whose reference value is NaN -- 0/0 from a constant
ground truth (both sides), a constant prediction (prediction side only) or a ground truth so sparse that its upper percentile is 0
(both sides) -- is byte 0, asserted literally; the other sides, and the other images of the same call, stay bit-exact.  Every
non-degenerate case asserts that the oracle ran without a warning.

SSIM errors against the exact value, measured on an MI355X over the 8 shapes x 7 contents of test_image_metrics_vs_exact_values:
    kernel        max 1.6e-14 (200x7, the diagonal ramp against its mirror image); at most 2.0e-15 off the ramp
    scipy oracle  max 6.7e-13 (7x200, the same content); 2.0e-13 at 45x71, 2.7e-14 on the saturated field
The kernel's maximum is 40 times below the oracle's, and inside what its arithmetic allows (the cancellation in uxx - ux * ux is at
most about 65025 * 2^-52 = 1.4e-11 against c2 = 58.5: a few 1e-13).  Its window sums are exact, so its error does not depend on the
image size; scipy's running float64 sums drift along a row, hence 6.7e-13 over 200 columns.  On single cases the oracle is the closer
one (200x7 ramp: 4.4e-16 against the kernel's 1.6e-14; zeros against 255: 0 against 1.6e-17): scipy's first pass then runs over
integers and is exact too, while the kernel still rounds s / 49 (as s * (1 / 49)) and the products in the SSIM expression.  That is
the rounding the kernel's header names, not a loss in the sums.

test_metrics' `psnr = inf` for a prediction equal to its ground truth is not asserted here: reaching that guard needs a model whose
output equals the ground truth, i.e. a fake model."""
import numpy as np
import pytest
import torch

import _metrics_ref as R

pytestmark = pytest.mark.gpu


def _dev(x):
    return torch.tensor(x).cuda()


def _normalize(hr, hat, pmin=0.1, pmax=99.9):
    from pssr2_amd import ops
    a, b = ops.normalize_preds_u8(_dev(hr), _dev(hat), pmin=pmin, pmax=pmax)
    return a.cpu().numpy(), b.cpu().numpy()


def _assert_bit_exact_vs_clean_oracle(hr, hat, pcts, what):
    want_a, want_b, caught = R.oracle_normalize(hr, hat, *pcts)
    assert caught == [], (what, pcts, caught)                 # a degenerate input must not slip into the bit-exact set
    a, b = _normalize(hr, hat, *pcts)
    np.testing.assert_array_equal(a, want_a, err_msg=f"{what} {pcts} hr side")
    np.testing.assert_array_equal(b, want_b, err_msg=f"{what} {pcts} prediction side")


@pytest.mark.parametrize("shape", R.NORM_SHAPES)
def test_normalize_preds_bit_exact_on_chunk_tails(shape):
    for content in R.NORM_CONTENTS:
        hr, hat = R.norm_pair(shape, content)
        for pcts in R.NORM_PERCENTILES:
            _assert_bit_exact_vs_clean_oracle(hr, hat, pcts, (shape, content))


@pytest.mark.parametrize("pcts", R.EDGE_PERCENTILES)
def test_normalize_preds_bit_exact_on_percentile_edges(pcts):
    hr, hat = R.edge_pair()
    _assert_bit_exact_vs_clean_oracle(hr, hat, pcts, "edge")


@pytest.mark.parametrize("name", ["two_level", "narrow", "sparse50"])
def test_normalize_preds_bit_exact_on_narrow_distributions(name):
    hr, hat, percentiles = R.distribution_pairs()[name]
    for pcts in percentiles:
        _assert_bit_exact_vs_clean_oracle(hr, hat, pcts, name)


@pytest.mark.parametrize("name", ["constant_hr", "constant_hat", "both_zero", "sparse4", "mixed"])
def test_normalize_preds_degenerate_sides_are_zero_bytes(name):
    """The contract of csrc/metrics.hip's header: a side whose reference value is NaN is byte 0, literally; every other side is still
    bit-exact with the oracle (tests/test_metrics_ref.py documents that the oracle's own cast gives 0 on the same sides on x86-64)."""
    hr, hat, zero_hr, zero_hat = R.degenerate_cases()[name]
    want_a, want_b, _ = R.oracle_normalize(hr, hat)
    a, b = _normalize(hr, hat)
    for i in range(hr.shape[0]):
        np.testing.assert_array_equal(a[i], np.zeros_like(a[i]) if zero_hr[i] else want_a[i], err_msg=f"{name} image {i} hr side")
        np.testing.assert_array_equal(b[i], np.zeros_like(b[i]) if zero_hat[i] else want_b[i], err_msg=f"{name} image {i} prediction side")
        assert zero_hr[i] or a[i].std() > 10
    if name == "sparse4":                                      # the sparse image of the distribution test, at the percentiles that empty it
        hr, hat, _ = R.distribution_pairs()["sparse50"]
        a, b = _normalize(hr, hat, 2.0, 98.0)
        assert not a.any() and not b.any()


def test_normalize_preds_bit_exact_vs_reference_fixture(golden):
    from pssr2_amd import ops
    g = golden("metrics.npz")
    for n in "abc":
        a, b = ops.normalize_preds_u8(torch.tensor(g[f"{n}_hr"]).cuda(), torch.tensor(g[f"{n}_hat"]).cuda())
        np.testing.assert_array_equal(a.cpu().numpy(), g[f"{n}_hr_norm"])
        np.testing.assert_array_equal(b.cpu().numpy(), g[f"{n}_hat_norm"])
    a, b = ops.normalize_preds_u8(torch.tensor(g["a_hr"]).cuda(), torch.tensor(g["a_hat"]).cuda(), pmin=2.0, pmax=98.0)
    np.testing.assert_array_equal(a.cpu().numpy(), g["a_p2_hr_norm"])
    np.testing.assert_array_equal(b.cpu().numpy(), g["a_p2_hat_norm"])


@pytest.mark.parametrize("shape", [(2, 512, 512), (3, 100, 37), (1, 9, 13), (2, 1, 256, 320)])
def test_normalize_preds_bit_exact_vs_oracle(shape):
    from oracle import metrics_ref as M
    from pssr2_amd import ops
    rng = np.random.default_rng(sum(shape))
    base = rng.normal(120, 40, size=shape)
    hr = np.clip(base + rng.normal(0, 5, size=shape), 0, 255).astype(np.uint8)
    hat = np.clip(0.7 * base + 30 + rng.normal(0, 9, size=shape), 0, 255).astype(np.uint8)
    want_a, want_b = M.normalize_preds(hr, hat)
    a, b = ops.normalize_preds_u8(torch.tensor(hr).cuda(), torch.tensor(hat).cuda())
    np.testing.assert_array_equal(a.cpu().numpy(), want_a)
    np.testing.assert_array_equal(b.cpu().numpy(), want_b)


def test_normalize_preds_argument_checks():
    from pssr2_amd import ops
    x = torch.zeros(1, 8, 8, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError):
        ops.normalize_preds_u8(x, x.float())
    with pytest.raises(RuntimeError, match="percentiles"):
        ops.normalize_preds_u8(x, x, pmin=60.0, pmax=40.0)


def test_normalize_preds_api_and_drivers():
    """pssr2_amd.util.normalize_preds (numpy in / numpy out like the reference), predict_images(norm=True) on a paired dataset and
    test_metrics (pssr/predict.py:144-211: the reference's own smoke tests check only that these run and the result sizes)."""
    from oracle import metrics_ref as M
    from pssr2_amd.crappifiers import AdditiveGaussian
    from pssr2_amd.data import ArrayDataset
    from pssr2_amd.models import ResUNet
    from pssr2_amd.predict import predict_images, test_metrics
    from pssr2_amd.util import normalize_preds
    rng = np.random.default_rng(4)
    hr = rng.integers(0, 256, size=(2, 1, 64, 64), dtype=np.uint8)
    hat = np.clip(hr.astype(np.int32) // 2 + 40 + rng.integers(-9, 10, size=hr.shape), 0, 255).astype(np.uint8)
    a, b = normalize_preds(hr, hat)
    wa, wb = M.normalize_preds(hr, hat)
    assert a.dtype == np.uint8 and a.shape == hr.shape
    np.testing.assert_array_equal(a, wa)
    np.testing.assert_array_equal(b, wb)
    with pytest.raises(ValueError):
        normalize_preds(hr, hat[0])
    a4, b4 = normalize_preds(hr, np.ascontiguousarray(hat[..., :32, :32]))       # a prediction of another size keeps its size (pssr/util.py:176-179)
    assert a4.shape == hr.shape and b4.shape == (2, 1, 32, 32) and np.array_equal(a4, wa)
    torch.manual_seed(0)
    model = ResUNet(hidden=[16, 32])
    images = rng.integers(0, 256, size=(6, 1, 64, 64), dtype=np.uint8)
    ds = ArrayDataset(images, hr_res=64, lr_scale=4, crappifier=AdditiveGaussian(5), val_split=0.5, rotation=False)
    plain = predict_images(model, ds, device="cuda", batch_size=2, out_dir=None)
    normed = predict_images(model, ds, device="cuda", batch_size=2, out_dir=None, norm=True)
    assert plain.keys() == normed.keys() and len(plain) == len(ds.val_idx)
    assert all(v.dtype == np.uint8 and v.shape == (1, 64, 64) for v in normed.values())
    assert any(not np.array_equal(plain[k], normed[k]) for k in plain)          # an untrained net is far from the ground truth's intensities
    res = test_metrics(model, ds, device="cuda")
    assert set(res) == {"mse", "pixel", "psnr", "ssim"} and all(np.isfinite(v) for v in res.values())
    per = test_metrics(model, ds, device="cuda", metrics=["psnr", "ssim"], avg=False, norm=False)
    assert len(per["psnr"]) == len(ds.val_idx) and -1.0 <= per["ssim"][0] <= 1.0


@pytest.mark.parametrize("shape", [(1, 7, 7), (3, 64, 64), (2, 100, 37), (1, 38, 39), (1, 512, 512)])
def test_image_metrics_vs_oracle(shape):
    """Sum of squared differences exact; SSIM vs the scipy restatement of skimage's structural_similarity (float64, 1e-10)."""
    from oracle import metrics_ref as M
    from pssr2_amd import ops
    rng = np.random.default_rng(sum(shape))
    hr = rng.integers(0, 256, size=shape, dtype=np.uint8)
    hat = np.clip(hr.astype(np.int32) + rng.integers(-40, 41, size=shape), 0, 255).astype(np.uint8)
    hat[0, :3] = 255 - hat[0, :3]                                                  # some strongly anti-correlated windows
    got = ops.image_metrics_u8(torch.tensor(hr).cuda(), torch.tensor(hat).cuda()).cpu().numpy()
    again = ops.image_metrics_u8(torch.tensor(hr).cuda(), torch.tensor(hat).cuda()).cpu().numpy()
    assert np.array_equal(got, again)                                              # fixed summation order
    for i in range(shape[0]):
        ssd = int(((hr[i].astype(np.int64) - hat[i].astype(np.int64)) ** 2).sum())
        assert got[i, 0] == ssd
        assert abs(10 * np.log10(255.0 ** 2 * hr[i].size / got[i, 0]) - M.psnr(hr[i], hat[i])) < 1e-9      # bar: 1e-3 dB
        assert abs(got[i, 1] - M.ssim(hr[i], hat[i])) < 1e-10


def test_image_metrics_identical_and_argument_checks():
    from pssr2_amd import ops
    x = torch.randint(0, 256, (2, 1, 48, 48), dtype=torch.uint8, device="cuda")
    got = ops.image_metrics_u8(x, x).cpu().numpy()
    assert np.array_equal(got[:, 0], [0.0, 0.0]) and np.allclose(got[:, 1], 1.0, atol=1e-15)
    with pytest.raises(ValueError):
        ops.image_metrics_u8(x[..., :6, :], x[..., :6, :])                          # the 7x7 window does not fit (skimage raises too)
    with pytest.raises(ValueError):
        ops.image_metrics_u8(x, x.float())
    with pytest.raises(ValueError):
        ops.image_metrics_u8(x, x[:1])


def test_test_metrics_values_match_oracle_on_the_arrays_it_evaluated():
    """test_metrics' numbers against the oracle evaluated on the very uint8 arrays a reference-style callback receives
    (pssr/predict.py:193-203: mse of the /255 images, pixel_metric, skimage psnr / ssim)."""
    from oracle import metrics_ref as M
    from pssr2_amd.crappifiers import AdditiveGaussian
    from pssr2_amd.data import ArrayDataset
    from pssr2_amd.models import ResUNet
    from pssr2_amd.predict import test_metrics
    from pssr2_amd.util import pixel_metric
    rng = np.random.default_rng(5)
    torch.manual_seed(1)
    model = ResUNet(hidden=[16, 32])
    images = rng.integers(0, 256, size=(4, 1, 64, 64), dtype=np.uint8)
    ds = ArrayDataset(images, hr_res=64, lr_scale=4, crappifier=AdditiveGaussian(5), val_split=0.5, rotation=False)
    seen = []
    per = test_metrics(model, ds, device="cuda", avg=False, callbacks=[lambda loc: seen.append((loc["hr"].copy(), loc["hr_hat"].copy()))])
    assert len(seen) == len(ds.val_idx)
    for k, (hr, hat) in enumerate(seen):
        mse = np.mean((hr[0] / 255 - hat[0] / 255) ** 2)
        assert abs(per["mse"][k] - mse) <= 1e-12 * mse
        assert abs(per["pixel"][k] - pixel_metric(mse, 255)) <= 1e-9
        assert abs(per["psnr"][k] - M.psnr(hr[0], hat[0])) < 1e-9
        assert abs(per["ssim"][k] - M.ssim(hr[0].squeeze(), hat[0].squeeze())) < 1e-10


@pytest.mark.parametrize("hr_shape,hat_shape", [((2, 128, 128), (2, 32, 32)), ((1, 64, 96), (1, 256, 384)), ((3, 100, 37), (3, 41, 90)),
                                                  ((1, 512, 512), (1, 128, 128)), ((2, 40, 40), (2, 40, 56))])
def test_normalize_preds_with_a_prediction_of_another_size_vs_oracle(hr_shape, hat_shape):
    """pssr/util.py:176-179 on the device (pssr_normalize_preds_resized_u8) against the numpy / scipy restatement: the ground-truth
    side is bit-exact (it does not depend on the resize); the prediction side is a 256-entry table scaled by the covariance amplitude,
    whose resize the device evaluates from the raw bytes in float64 instead of from mean-removed float32 values -- equal up to the last
    bits of `amp`, so a byte may land on the other side of a truncation: <= 1 grey level on <= 0.5 % of the pixels."""
    from oracle import metrics_ref as M
    from pssr2_amd import ops
    from pssr2_amd.util import normalize_preds
    rng = np.random.default_rng(sum(hr_shape) + sum(hat_shape))
    base = rng.normal(120, 40, size=hr_shape)
    from scipy import ndimage as ndi
    base = ndi.gaussian_filter(base, (0, 2, 2)) * 2.5 - 180            # spatial structure, so that the covariance is not noise
    hr = np.clip(base + rng.normal(0, 5, size=hr_shape), 0, 255).astype(np.uint8)
    zoom = (1, hat_shape[1] / hr_shape[1], hat_shape[2] / hr_shape[2])
    hat = np.clip(0.7 * ndi.zoom(base, zoom, order=1, grid_mode=True, mode="mirror") + 30 + rng.normal(0, 6, size=hat_shape), 0, 255).astype(np.uint8)
    want_a, want_b = M.normalize_preds(hr, hat)
    a, b = ops.normalize_preds_resized_u8(torch.tensor(hr).cuda(), torch.tensor(hat).cuda())
    a, b = a.cpu().numpy(), b.cpu().numpy()
    np.testing.assert_array_equal(a, want_a)
    d = np.abs(b.astype(int) - want_b.astype(int))
    assert d.max() <= 1 and (d > 0).mean() <= 5e-3, (d.max(), (d > 0).mean())
    assert want_b.std() > 10                                           # a real image came out, not a constant
    a3, b3 = normalize_preds(hr, hat)                                  # the reference-shaped entry point routes here
    assert np.array_equal(a3, a) and np.array_equal(b3, b) and b3.shape == hat_shape


@pytest.mark.parametrize("hr_shape,hat_shape", R.RESIZED_SHAPES)
def test_normalize_preds_of_another_size_on_the_remaining_branches(hr_shape, hat_shape):
    """Shrinking along y only (the Gaussian pre-filter on axis 0 alone), shrinking y while enlarging x, and both ways between 91x91
    and 181x181, where the n and n_hat reductions both end in a tail piece.  The bound is the one of the test above;
    tests/test_metrics_ref.py shows that the device's covariance formula, restated on the host, stays inside it on these inputs."""
    from pssr2_amd import ops
    hr, hat = R.resized_pair(hr_shape, hat_shape)
    want_a, want_b, caught = R.oracle_normalize(hr, hat)
    assert caught == [] and want_b.std() > 10
    a, b = ops.normalize_preds_resized_u8(_dev(hr), _dev(hat))
    a, b = a.cpu().numpy(), b.cpu().numpy()
    np.testing.assert_array_equal(a, want_a)
    ok, figures = R.within_resized_cap(b, want_b)
    print(f"resized {hr_shape} / {hat_shape}: max diff {figures[0]}, fraction {figures[1]:.2e}")
    assert ok and b.shape == hat_shape, figures


def _image_metrics(a, b):
    from pssr2_amd import ops
    return ops.image_metrics_u8(_dev(a), _dev(b)).cpu().numpy()


@pytest.mark.parametrize("shape", R.METRIC_SHAPES)
def test_image_metrics_vs_exact_values(shape):
    """Squared-difference sum equal to the Python-int sum; SSIM within 1e-10 of the exact value (tests/_metrics_ref.py:ssim_exact);
    two calls bit-identical; a batch row equal, bit for bit, to the same image evaluated alone (the img * tiles + tile indexing)."""
    from oracle import metrics_ref as M
    for content in R.METRIC_CONTENTS:
        a, b = R.metric_pair(shape, content)
        got = _image_metrics(a, b)
        assert got.shape == (shape[0], 2) and np.array_equal(got, _image_metrics(a, b))
        exact = [R.ssim_exact(a[i], b[i]) for i in range(shape[0])]
        err_kernel = max(abs(got[i, 1] - exact[i]) for i in range(shape[0]))
        err_oracle = max(abs(M.ssim(a[i], b[i]) - exact[i]) for i in range(shape[0]))
        print(f"ssim {shape} {content}: kernel error {err_kernel:.3e}, scipy oracle error {err_oracle:.3e}")
        for i in range(shape[0]):
            assert got[i, 0] == R.ssd_exact(a[i], b[i]), (content, i)
            assert abs(got[i, 1] - exact[i]) <= 1e-10, (content, i, got[i, 1], exact[i])
        if shape[0] > 1:
            for i in range(shape[0]):
                assert np.array_equal(_image_metrics(a[i:i + 1], b[i:i + 1])[0], got[i]), (content, i)
    x = R.flat(shape, 200)                                                         # identical constant images: every variance cancels
    got = _image_metrics(x, x)
    assert np.array_equal(got[:, 0], np.zeros(shape[0])) and np.abs(got[:, 1] - 1.0).max() <= 1e-15, got
