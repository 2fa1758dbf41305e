"""Consistency maps without a GPU: the numpy restatement of tests/_consistency_ref.py against PIL.Image.resize and against its own
properties, the keyword and argument checks of the Python entry points (raised before any device work), and the argument checks of the
two C entry points."""
import ctypes
import math
from pathlib import Path

import numpy as np
import pytest
import torch

import _consistency_ref as R

ROOT = Path(__file__).resolve().parent.parent
SCALES = (1, 2, 3, 4, 8, 16)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("s", SCALES)
@pytest.mark.parametrize("h,w", [(5, 7), (9, 33), (2, 3), (1, 1), (33, 40)])
def test_restated_reduction_is_pillow(h, w, s):
    from PIL import Image
    rng = np.random.default_rng(100 * s + h)
    for y in (rng.integers(0, 256, size=(h * s, w * s), dtype=np.uint8), np.full((h * s, w * s), 255, dtype=np.uint8),
              (rng.integers(0, 2, size=(h * s, w * s)) * 255).astype(np.uint8)):
        want = np.asarray(Image.fromarray(y).resize((w, h), Image.BILINEAR))
        np.testing.assert_array_equal(R.reduce_ref(y, h, w), want)


def test_taps_of_an_integer_ratio_stay_inside_the_block_halo():
    """What the fused kernel's LDS arrays are sized by: at most 2 s taps, starting at i s - s // 2 (clipped), so that 32 outputs read at
    most 33 s inputs."""
    for s in range(1, 17):
        for n in (1, 2, 31, 32, 33, 70):
            t = R.taps(n, n * s)
            assert all(len(k) <= 2 * s and xmin == max(i * s - s // 2, 0) for i, (xmin, k) in enumerate(t))
            assert all(xmin + len(k) <= n * s for xmin, k in t)
            for i0 in range(0, n, 32):
                last = t[min(i0 + 31, n - 1)]
                assert last[0] + len(last[1]) - t[i0][0] <= 33 * s


def test_scale_one_is_the_identity():
    y = np.random.default_rng(1).integers(0, 256, size=(2, 7, 5), dtype=np.uint8)
    np.testing.assert_array_equal(R.reduce_ref(y, 7, 5), y)


@pytest.mark.parametrize("s", [1, 4])
def test_identity_fit_of_the_reduction_itself_is_a_zero_map(s):
    y = np.random.default_rng(2).integers(0, 256, size=(1, 1, 9 * s, 11 * s), dtype=np.uint8)
    d = R.reduce_ref(y, 9, 11)
    cmap, alpha, beta, rse, rsp = R.consistency_ref(d, y, "identity")
    assert not cmap.any() and alpha[0, 0] == 1.0 and beta[0, 0] == 0.0 and rse[0, 0] == 0.0
    assert rsp[0, 0] == 1.0
    # ... and the affine fit finds the identity, up to the rounding of the division
    cmap, alpha, beta, rse, rsp = R.consistency_ref(d, y, "affine")
    assert not cmap.any() and abs(alpha[0, 0] - 1.0) < 1e-12 and abs(beta[0, 0]) < 1e-9 and rse[0, 0] < 1e-2


def test_constant_prediction_takes_the_degenerate_branch():
    l = np.random.default_rng(3).integers(0, 256, size=(1, 1, 6, 6), dtype=np.uint8)
    y = np.full((1, 1, 12, 12), 77, dtype=np.uint8)
    cmap, alpha, beta, rse, rsp = R.consistency_ref(l, y)
    assert alpha[0, 0] == 0.0 and beta[0, 0] == int(l.astype(np.int64).sum()) / 36 and rsp[0, 0] == 0.0
    sse = sum((256 * int(v) - round(256.0 * beta[0, 0])) ** 2 for v in l.reshape(-1))
    assert rse[0, 0] == math.sqrt(sse / 36) / 256
    # a constant LR image: den > 0 but denl == 0
    cmap, alpha, beta, rse, rsp = R.consistency_ref(np.full((1, 1, 6, 6), 9, dtype=np.uint8), np.random.default_rng(4).integers(
        0, 256, size=(1, 1, 12, 12), dtype=np.uint8))
    assert rsp[0, 0] == 0.0 and alpha[0, 0] == 0.0 and beta[0, 0] == 9.0 and not cmap.any()


def test_planted_affine_data_is_recovered_and_a_hallucination_shows():
    rng = np.random.default_rng(5)
    yy, xx = np.mgrid[0:64, 0:64]
    d = np.clip(120 + 90 * np.sin(yy / 9.0) * np.cos(xx / 7.0), 0, 255).astype(np.uint8)
    l = np.clip(np.round(0.5 * d + 10 + rng.normal(0, 3, size=d.shape)), 0, 255).astype(np.uint8)
    cmap, alpha, beta, rse, rsp = R.consistency_ref(l[None, None], d[None, None])          # s = 1: D = Y
    assert abs(alpha[0, 0] - 0.5) < 0.02 and abs(beta[0, 0] - 10) < 2 and 0.98 < rsp[0, 0] < 1 and 2.5 < rse[0, 0] < 3.5
    assert cmap.max() < 20
    l[20:24, 30:34] = 255                                                                  # what the microscope saw and the network lost
    cmap2 = R.consistency_ref(l[None, None], d[None, None])[0]
    assert cmap2[0, 0, 20:24, 30:34].min() >= 150 and np.delete(cmap2[0, 0], np.s_[20:24], 0).max() < 25


def test_table_clamps_and_rounds_half_to_even():
    assert R.table_ref(0.0, 0.5 / 256)[0] == 0 and R.table_ref(0.0, 1.5 / 256)[0] == 2          # half to even
    t = R.table_ref(1e9, -1e9)
    assert t[0] == -65536 and t[1] == 0 and t[2] == 131071 and t.dtype == np.int32
    cmap, sse = R.map_ref(np.array([[0, 2]], dtype=np.uint8), np.array([[255, 0]], dtype=np.uint8), t)
    assert cmap.tolist() == [[255, 255]] and sse == (65280 + 65536) ** 2 + 131071 ** 2


def test_centre_frames():
    lr = np.arange(5, dtype=np.uint8).reshape(1, 5, 1, 1)
    assert R.slice_center(lr, 1).reshape(-1).tolist() == [2] and R.slice_center(lr, 3).reshape(-1).tolist() == [1, 2, 3]
    assert R.slice_center(lr, 2).reshape(-1).tolist() == [1, 2] and R.slice_center(lr, 5).reshape(-1).tolist() == [0, 1, 2, 3, 4]
    from pssr2_amd.data import _slice_center
    for n in range(1, 6):
        np.testing.assert_array_equal(R.slice_center(lr, n), _slice_center(lr, n))


def test_package_fit_is_the_restated_fit():
    """util._consistency_fit (host Python) against the restatement, on sums from real planes and on the degenerate ones."""
    from pssr2_amd.util import _consistency_fit
    rng = np.random.default_rng(6)
    cases = [R.moments_ref(rng.integers(0, 256, size=50), rng.integers(0, 256, size=50)) for _ in range(20)]
    cases += [R.moments_ref(np.full(50, 7), rng.integers(0, 256, size=50)), R.moments_ref(rng.integers(0, 256, size=50), np.full(50, 7)),
              R.moments_ref(np.zeros(50), np.zeros(50)), R.moments_ref(np.full(50, 255), np.full(50, 255))]
    for sums in cases:
        for fit in R.FITS:
            alpha, beta, rsp, table = _consistency_fit(50, sums, fit)
            assert (alpha, beta, rsp) == R.fit_ref(50, sums, fit)
            assert table == R.table_ref(alpha, beta).tolist()


# ------------------------------------------------------------------------------------------------ keyword and argument checks
class _Never(torch.nn.Module):
    def forward(self, x):                                  # pragma: no cover
        raise AssertionError("the checks come before the model runs")

    def to(self, *a, **k):                                 # pragma: no cover
        raise AssertionError("the checks come before the model is moved")


class _NoData:
    def __getattr__(self, name):                           # pragma: no cover
        raise AssertionError(f"the keyword checks come before the dataset is touched ({name})")


def test_fits():
    from pssr2_amd import ops
    assert ops.FITS == ("affine", "identity") == R.FITS


U8 = np.zeros((2, 3, 4, 5), dtype=np.uint8)


@pytest.mark.parametrize("lr,hat,kw,error,word", [
    (U8, np.zeros((2, 1, 8, 10), dtype=np.uint8), dict(fit="linear"), ValueError, "fit"),
    (U8, np.zeros((2, 1, 8, 10), dtype=np.uint8), dict(fit=None), ValueError, "fit"),
    (U8.astype(np.float32), np.zeros((2, 1, 8, 10), dtype=np.uint8), {}, TypeError, "uint8"),
    (U8, np.zeros((2, 1, 8, 10), dtype=np.int16), {}, TypeError, "uint8"),
    (torch.zeros(2, 3, 4, 5, dtype=torch.uint8), torch.zeros(2, 1, 8, 10, dtype=torch.uint8), {}, RuntimeError, "no CPU fallback"),
    (U8, np.zeros((2, 4, 8, 10), dtype=np.uint8), {}, ValueError, "4 planes"),                 # C_out > m
    (U8, np.zeros((3, 1, 8, 10), dtype=np.uint8), {}, ValueError, "same number of images"),
    (U8, np.zeros((2, 1, 8, 11), dtype=np.uint8), {}, ValueError, "integer multiple"),
    (U8, np.zeros((2, 1, 8, 15), dtype=np.uint8), {}, ValueError, "integer multiple"),        # two ratios
    (U8, np.zeros((2, 1, 3, 4), dtype=np.uint8), {}, ValueError, "integer multiple"),         # smaller than the input
    (U8, np.zeros((2, 1, 68, 85), dtype=np.uint8), {}, ValueError, "integer multiple"),       # s = 17
    (U8, np.zeros((1, 8, 10), dtype=np.uint8), {}, ValueError, "3-D"),
    (U8[0, 0], np.zeros((8, 10), dtype=np.uint8), {}, ValueError, "3-D"),
    (np.zeros((1, 1, 0, 5), dtype=np.uint8), np.zeros((1, 1, 0, 10), dtype=np.uint8), {}, ValueError, "integer multiple"),
])
def test_consistency_map_checks_its_arguments_before_the_device(lr, hat, kw, error, word):
    from pssr2_amd.util import consistency_map
    with pytest.raises(error, match=word):
        consistency_map(lr, hat, **kw)


def test_ops_refuse_host_tensors_and_wrong_shapes():
    from pssr2_amd import ops
    y, l = torch.zeros(1, 8, 8, dtype=torch.uint8), torch.zeros(1, 4, 4, dtype=torch.uint8)
    with pytest.raises(ValueError, match="uint8 device tensors"):
        ops.reduce_moments_u8(y, l)
    with pytest.raises(ValueError, match="uint8 device tensors"):
        ops.consistency_map_u8(l, l, torch.zeros(1, 256, dtype=torch.int32))


@pytest.mark.parametrize("kw,error,word", [(dict(consistency=True, fit="poly"), ValueError, "fit"), (dict(fit="poly"), ValueError, "fit"),
                                           (dict(consistency=True, device="cpu"), RuntimeError, "no CPU fallback")])
def test_predict_images_checks_its_keywords_first(kw, error, word):
    from pssr2_amd.predict import predict_images
    kw = {"device": "cuda", **kw}
    with pytest.raises(error, match=word):
        predict_images(_Never(), _NoData(), out_dir=None, **kw)


def test_test_metrics_and_predict_sheet_check_fit_first():
    from pssr2_amd.predict import predict_sheet, test_metrics
    with pytest.raises(ValueError, match="fit"):
        test_metrics(_Never(), _NoData(), device="cuda", metrics=("rse",), fit="cubic")
    with pytest.raises(ValueError, match="fit"):
        predict_sheet(_Never(), np.zeros((1, 40, 40), dtype=np.uint8), tile_res=16, overlap=4, device="cuda", consistency=True, fit="cubic")


def test_new_arguments_are_keyword_only_and_off_by_default():
    import inspect
    from pssr2_amd import predict as P
    from pssr2_amd import util as U
    for fn, names in ((P.predict_images, ("consistency", "fit")), (P.predict_sheet, ("consistency", "fit")), (P.test_metrics, ("fit",)),
                      (U.consistency_map, ("fit", "to_numpy"))):
        params = inspect.signature(fn).parameters
        for name in names:
            assert params[name].kind is inspect.Parameter.KEYWORD_ONLY
            assert params[name].default == {"consistency": False, "fit": "affine", "to_numpy": True}[name]
    assert inspect.signature(P.test_metrics).parameters["metrics"].default == ("mse", "pixel", "psnr", "ssim")
    assert U.Consistency._fields == ("map", "alpha", "beta", "rse", "rsp")


# ------------------------------------------------------------------------------------------------ argument checks of the entry points
def _lib():
    path = ROOT / "pssr2_amd" / "libpssr_mi355.so"
    if not path.exists():
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(str(path))
    lib.pssr_last_error.restype = ctypes.c_char_p
    return lib


def test_consistency_entry_points_validate_without_gpu():
    """Every check happens before the launch: an error code and a message, no crash, no device needed."""
    lib = _lib()
    assert lib.pssr_abi_version() == 5
    i, i64, p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    reduce, cmap = lib.pssr_reduce_moments_u8, lib.pssr_consistency_map_u8
    reduce.argtypes = [p] * 4 + [i] * 4 + [p, p]
    cmap.argtypes = [p] * 5 + [i, i64, p, p]
    lib.pssr_reduce_moments_workspace_bytes.restype = lib.pssr_consistency_map_workspace_bytes.restype = i64
    lib.pssr_reduce_moments_workspace_bytes.argtypes = [i] * 4
    lib.pssr_consistency_map_workspace_bytes.argtypes = [i, i64]
    fake = 0x1000          # never dereferenced: every call below fails its checks

    def err(status, word):
        return status == -1 and word in lib.pssr_last_error()

    # y, l, d, sums, planes, h, w, s, workspace
    for hole in range(4):
        ptrs = [None if k == hole else fake for k in range(4)]
        assert err(reduce(*ptrs, 2, 8, 8, 4, fake, None), b"null")
    assert err(reduce(fake, fake, fake, fake, 2, 8, 8, 4, None, None), b"null")
    for bad in (0, 17, -1, 32):
        assert err(reduce(fake, fake, fake, fake, 2, 8, 8, bad, fake, None), b"scale")
    for bad in ((0, 8, 8), (2, 0, 8), (2, 8, 0), (-1, 8, 8), (2, -8, 8)):
        assert err(reduce(fake, fake, fake, fake, *bad, 4, fake, None), b"positive")
    assert err(reduce(fake, fake, fake, fake, 1, 16385, 16384, 1, fake, None), b"2^28")            # one row over 2^28 pixels
    assert err(reduce(fake, fake, fake, fake, 1, 1 << 27, 1, 16, fake, None), b"2^30")             # an axis of y of 2^31
    assert lib.pssr_reduce_moments_workspace_bytes(1, 16385, 16384, 1) == 0
    assert lib.pssr_reduce_moments_workspace_bytes(1, 8, 8, 17) == 0
    assert lib.pssr_reduce_moments_workspace_bytes(3, 64, 64, 4) >= 3 * 5 * 8                      # a row of five 64-bit sums per plane at least

    # d, l, lut, map, sse, planes, pixels, workspace
    for hole in range(5):
        ptrs = [None if k == hole else fake for k in range(5)]
        assert err(cmap(*ptrs, 2, 64, fake, None), b"null")
    assert err(cmap(fake, fake, fake, fake, fake, 2, 64, None, None), b"null")
    for bad in ((0, 64), (2, 0), (-3, 64), (2, -1)):
        assert err(cmap(fake, fake, fake, fake, fake, *bad, fake, None), b"positive")
    assert err(cmap(fake, fake, fake, fake, fake, 1, (1 << 28) + 1, fake, None), b"2^28")
    assert lib.pssr_consistency_map_workspace_bytes(0, 64) == 0
    assert lib.pssr_consistency_map_workspace_bytes(2, 64) >= 2 * 8
