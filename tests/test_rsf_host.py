"""The resolution-scaling-function search without a GPU: the tap table and its properties, the numpy restatement of tests/_rsf_ref.py
against PIL.Image.resize and the registration restatement, planted candidates, the tie rule, constant pairs, pooling, the argument checks
of the Python entry points (raised before any device work) and those of the four C entry points.

One property is weaker than "every row sums to 2^22": the row of sigma = 0 must be Pillow's interior taps bit for bit, and Pillow rounds
each tap on its own, so at s = 3 that row sums to 2^22 + 1 (at s = 1, 2, 4, 8, 16 to 2^22).  Every row of a sigma > 0 sums to exactly 2^22.
Likewise a row at an even s is symmetric only up to the rounding's remainder: the definition gives it to the first of the two equal
largest taps, so those two taps differ by it and every other tap equals its mirror image."""
import ctypes
import inspect
import math
from pathlib import Path

import numpy as np
import pytest
import torch

import _consistency_ref as C
import _register_ref as R
import _rsf_ref as F

ROOT = Path(__file__).resolve().parent.parent
SCALES = (1, 2, 3, 4, 8, 16)
HALVES = [0.5 * i for i in range(17)]         # 0, 0.5, .. 8: every candidate gives another D on white noise (the 0.25 grid does not at s = 1)


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("s", SCALES)
def test_table_properties(s):
    from pssr2_amd import ops
    interior = R.interior_taps(s)
    for sigmas, radius in ((F.DEFAULT_SIGMAS, None), (HALVES, None), ([0.0], None), ([0.0], 3), ([0.3, 0.0, 10.6, 1.0], None), ([1.0, 2.5], 24),
                           ([0.0, 0.1], 32)):
        rows, rad = F.table(s, sigmas, radius)
        assert rad == (max(F.rad(v) for v in sigmas) if radius is None else radius) and len(rows) == len(sigmas)
        for sigma, row in zip(sigmas, rows):
            assert len(row) == 2 * s + 2 * rad and min(row) >= 0
            r = F.rad(sigma)
            assert not any(row[:rad - r]) and not any(row[rad + r + 2 * s:])
            if sigma == 0:
                assert row[rad:rad + 2 * s] == interior and sum(row) == sum(interior)
            else:
                assert sum(row) == F.ONE
            if s % 2 == 0:                       # symmetric but for the rounding's remainder, which the first of the two largest taps takes
                top = row.index(max(row))
                odd = [j for j in range(len(row)) if row[j] != row[len(row) - 1 - j]]
                assert set(odd) <= {top, len(row) - 1 - top} and 0 <= row[top] - row[len(row) - 1 - top] <= len(row) // 2
                assert sigma != 0 or not odd
        got, got_rad = ops.rsf_taps(s, sigmas, radius)
        assert got_rad == rad and got.dtype == np.int32 and got.shape == (len(sigmas), 2 * s + 2 * rad) and got.tolist() == rows
    assert sum(interior) == F.ONE + (1 if s == 3 else 0)


def test_default_grid():
    from pssr2_amd import ops, util
    assert list(util.RSF_SIGMAS) == F.DEFAULT_SIGMAS and len(util.RSF_SIGMAS) == 33
    taps, rad = ops.rsf_taps(4, util.RSF_SIGMAS)
    assert rad == 24 and taps.shape == (33, 56) and ops.register_margin(4, rad) == 7
    # a wide Gaussian is a smooth bump: it rises to its centre
    row = taps[32].tolist()
    assert all(a <= b for a, b in zip(row[:28], row[1:28]))


@pytest.mark.parametrize("bad,word", [
    (dict(s=0, sigmas=[1.0]), "scale"), (dict(s=17, sigmas=[1.0]), "scale"), (dict(s=2.0, sigmas=[1.0]), "scale"), (dict(s=True, sigmas=[1.0]), "scale"),
    (dict(s=4, sigmas=[]), "candidate"), (dict(s=4, sigmas=[0.1] * 65), "candidate"), (dict(s=4, sigmas=[-0.5]), "finite"),
    (dict(s=4, sigmas=[float("nan")]), "finite"), (dict(s=4, sigmas=[float("inf")]), "finite"), (dict(s=4, sigmas=[10.7]), "ceil"),
    (dict(s=4, sigmas=["a"]), "numbers"), (dict(s=4, sigmas=3.0), "numbers"),
    (dict(s=4, sigmas=[2.0], radius=5), "radius"), (dict(s=4, sigmas=[2.0], radius=33), "radius"), (dict(s=4, sigmas=[2.0], radius=6.0), "radius"),
])
def test_rsf_taps_checks_its_arguments(bad, word):
    from pssr2_amd import ops
    with pytest.raises(ValueError, match=word):
        ops.rsf_taps(**bad)


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("s", SCALES)
def test_the_sigma_zero_row_is_the_plain_reduction(s):
    """D of the sigma = 0 row is D_(0,0) of the registration restatement at the same radius -- which tests/test_register_host.py pins to
    PIL.Image.resize -- and PIL.Image.resize itself, whatever R."""
    from PIL import Image
    rng = np.random.default_rng(30 + s)
    for radius in (0, 3, 24):
        m = F.margin(s, radius)
        h, w = 4 + 2 * m, 6 + 2 * m
        y = rng.integers(0, 256, size=(2, s * h, s * w), dtype=np.uint8)
        rows, rad = F.table(s, [0.0], radius)
        assert rad == radius
        d = F.reduce_k(y, rows[0], s, radius)
        np.testing.assert_array_equal(d, R.dense(y, s)[..., s * m - s // 2:s * (h - m) - s // 2:s, s * m - s // 2:s * (w - m) - s // 2:s])
        if radius <= 3:
            np.testing.assert_array_equal(d, R.reduced_windows(y, h, w, radius)[(0, 0)])
        for p in range(2):
            want = np.asarray(Image.fromarray(y[p]).resize((w, h), Image.BILINEAR))[m:h - m, m:w - m]
            np.testing.assert_array_equal(d[p], want)
        np.testing.assert_array_equal(d, C.reduce_ref(y, h, w)[:, m:h - m, m:w - m])


def test_a_blurred_reduction_is_the_reduction_of_the_blur_up_to_rounding():
    """The rows are what the text says they are: D_sigma stays within two grey levels of the float Gaussian blur followed by the float
    triangle reduction (one rounding per pass, and the table's own rounding)."""
    rng = np.random.default_rng(40)
    s, sigma = 4, 1.5
    rows, radius = F.table(s, [sigma])
    m = F.margin(s, radius)
    h = w = 6 + 2 * m
    y = rng.integers(0, 256, size=(s * h, s * w), dtype=np.uint8)
    g = np.exp(-np.arange(-radius, radius + 1) ** 2 / (2 * sigma * sigma))
    g /= g.sum()
    t = np.array(R.interior_taps(s)) / F.ONE
    blur = np.apply_along_axis(lambda v: np.convolve(v, g, mode="same"), 1, y.astype(np.float64))
    blur = np.apply_along_axis(lambda v: np.convolve(v, g, mode="same"), 0, blur)
    want = np.empty((h - 2 * m, w - 2 * m))
    for yy in range(h - 2 * m):
        for xx in range(w - 2 * m):
            y0, x0 = s * (yy + m) - s // 2, s * (xx + m) - s // 2
            want[yy, xx] = t @ blur[y0:y0 + 2 * s, x0:x0 + 2 * s] @ t
    assert np.abs(F.reduce_k(y, rows[0], s, radius).astype(np.float64) - want).max() <= 2.0


def test_sums_layout():
    rng = np.random.default_rng(41)
    rows, radius = F.table(2, [0.0, 1.0, 0.4])
    m = F.margin(2, radius)
    y = rng.integers(0, 256, size=(2, 2 * (3 + 2 * m), 2 * (5 + 2 * m)), dtype=np.uint8)
    l = rng.integers(0, 256, size=(2, 3 + 2 * m, 5 + 2 * m), dtype=np.uint8)
    sums = F.sums_ref(y, l, rows, radius)
    assert len(sums) == 2 and all(len(r) == 3 * 3 + 2 for r in sums)
    lc = l[1, m:-m, m:-m].astype(np.int64)
    d = F.reduce_k(y[1], rows[2], 2, radius).astype(np.int64)
    assert sums[1][6:9] == [d.sum(), (d * d).sum(), (d * lc).sum()] and sums[1][-2:] == [lc.sum(), (lc * lc).sum()]


# ------------------------------------------------------------------------------------------------ the choice
@pytest.mark.parametrize("s", SCALES)
def test_every_planted_candidate_is_found_with_score_one(s):
    from pssr2_amd.util import _rsf_choose
    rng = np.random.default_rng(50 + s)
    rows, radius = F.table(s, HALVES)
    assert radius == 24
    m = F.margin(s, radius)
    h, w = 5 + 2 * m, 9 + 2 * m
    y = rng.integers(0, 256, size=(1, s * h, s * w), dtype=np.uint8)
    ds = [F.reduce_k(y, row, s, radius) for row in rows]
    assert len({d.tobytes() for d in ds}) == len(HALVES)
    for k_true in range(len(HALVES)):
        sums = F.sums_of(ds, ds[k_true])
        k, curve = F.choose_ref(45, sums, len(HALVES))
        assert (k, curve[k]) == (k_true, 1.0)
        got = _rsf_choose(45, sums, len(HALVES))
        assert got == (k, curve)
    # the same through planted_pair and sums_ref, two planes pooled
    hat, lr = F.planted_pair(rng, 1, 2, 3, h, w, s, rows, radius, [5])
    sums = F.sums_ref(hat[0], C.slice_center(lr, 2)[0], rows, radius)
    assert F.choose_ref(90, sums, len(HALVES))[0] == _rsf_choose(90, sums, len(HALVES))[0] == 5


def test_ties_go_to_the_smaller_index():
    from pssr2_amd.util import _rsf_choose
    rng = np.random.default_rng(60)
    rows, radius = F.table(2, [0.0, 1.0, 1.0, 2.0])            # two identical rows
    assert rows[1] == rows[2]
    m = F.margin(2, radius)
    hat, lr = F.planted_pair(rng, 1, 1, 1, 6 + 2 * m, 7 + 2 * m, 2, rows, radius, [2])
    sums = F.sums_ref(hat[0], lr[0], rows, radius)
    assert sums[0][3:6] == sums[0][6:9]
    assert _rsf_choose(42, sums, 4)[0] == F.choose_ref(42, sums, 4)[0] == 1
    # synthetic rows: the same triple everywhere is a K-way tie; a better triple further on wins; an equal one does not
    row = [10, 60, 70] * 3 + [12, 80]
    assert _rsf_choose(2, [row], 3) == F.choose_ref(2, [row], 3) and _rsf_choose(2, [row], 3)[0] == 0
    row = [10, 50, 60, 10, 60, 70, 10, 60, 70, 12, 80]           # scores 0, 1.25, 1.25
    assert _rsf_choose(2, [row], 3)[0] == F.choose_ref(2, [row], 3)[0] == 1


def test_constant_pairs_choose_the_first_candidate():
    from pssr2_amd.util import _rsf_choose
    rows, radius = F.table(2, [0.0, 0.5, 1.0])
    m = F.margin(2, radius)
    h = w = 4 + 2 * m
    rng = np.random.default_rng(61)
    for hat_v, lr_v in ((7, 7), (0, 255), (255, 255), (None, 9), (100, None)):
        hat = np.full((1, 2 * h, 2 * w), hat_v, dtype=np.uint8) if hat_v is not None else rng.integers(0, 256, size=(1, 2 * h, 2 * w), dtype=np.uint8)
        lr = np.full((1, h, w), lr_v, dtype=np.uint8) if lr_v is not None else rng.integers(0, 256, size=(1, h, w), dtype=np.uint8)
        sums = F.sums_ref(hat, lr, rows, radius)
        k, curve = _rsf_choose(16, sums, 3)
        assert (k, curve) == F.choose_ref(16, sums, 3) and k == 0 and curve == [0.0] * 3


def test_pooling_adds_the_sums():
    """pool="all": one choice from the sums of every plane of every item.  Two items planted at different candidates with very different
    contrast: the pooled choice follows the sums, not a vote."""
    from pssr2_amd.util import _rsf_choose
    rng = np.random.default_rng(62)
    rows, radius = F.table(2, HALVES[:7])
    m = F.margin(2, radius)
    h, w = 8 + 2 * m, 9 + 2 * m
    hat, lr = F.planted_pair(rng, 3, 1, 1, h, w, 2, rows, radius, [1, 4, 4])
    hat[0] //= 2
    lr[0, 0, m:h - m, m:w - m] = F.reduce_k(hat[0], rows[1], 2, radius)
    per_plane = [F.sums_ref(hat[i], lr[i], rows, radius)[0] for i in range(3)]
    assert [_rsf_choose(72, [r], 7)[0] for r in per_plane] == [1, 4, 4]
    pooled = _rsf_choose(3 * 72, per_plane, 7)
    assert pooled == F.choose_ref(3 * 72, per_plane, 7) and 0 < pooled[1][pooled[0]] < 1.0
    want = F.estimate_ref(lr, hat, HALVES[:7], pool="all")
    assert want[4].tolist() == [pooled[0]] * 3 and want[3].tolist() == [pooled[1]] * 3
    assert F.estimate_ref(lr, hat, HALVES[:7])[4].tolist() == [1, 4, 4]


# ------------------------------------------------------------------------------------------------ argument checks in Python
HAT, LR = np.zeros((2, 1, 64, 80), dtype=np.uint8), np.zeros((2, 3, 16, 20), dtype=np.uint8)


@pytest.mark.parametrize("lr,hat,kw,error,word", [
    (LR, HAT, dict(pool="image"), ValueError, "pool"),
    (LR, HAT, dict(pixel_size=0), ValueError, "pixel_size"),
    (LR, HAT, dict(pixel_size=-1.0), ValueError, "pixel_size"),
    (LR, HAT, dict(pixel_size=True), ValueError, "pixel_size"),
    (LR, HAT, dict(pixel_size="1"), ValueError, "pixel_size"),
    (LR, HAT, dict(sigmas=[]), ValueError, "candidates"),
    (LR, HAT, dict(sigmas=[0.5] * 65), ValueError, "candidates"),
    (LR, HAT, dict(sigmas=[1.0, -1.0]), ValueError, "finite"),
    (LR, HAT, dict(sigmas=[float("nan")]), ValueError, "finite"),
    (LR, HAT, dict(sigmas=[10.7]), ValueError, "ceil"),
    (LR, HAT, dict(sigmas="fit"), ValueError, "numbers"),
    (LR, HAT, dict(sigmas=1.0), ValueError, "numbers"),
    (LR[..., :14, :], HAT[..., :56, :], {}, ValueError, "margin"),                                  # R = 24 at s = 4: m = 7, h' = 0
    (LR[..., :14], HAT[..., :56], dict(sigmas=[0.0, 8.0]), ValueError, "margin"),                   # w' = 0
    (LR, HAT.astype(np.float32), dict(sigmas=[1.0]), TypeError, "uint8"),
    (LR.astype(np.int16), HAT, dict(sigmas=[1.0]), TypeError, "uint8"),
    (torch.zeros(2, 3, 16, 20, dtype=torch.uint8), torch.zeros(2, 1, 64, 80, dtype=torch.uint8), dict(sigmas=[1.0]), RuntimeError, "no CPU fallback"),
    (LR, np.zeros((2, 4, 64, 80), dtype=np.uint8), dict(sigmas=[1.0]), ValueError, "4 planes"),
    (LR, HAT[:1], dict(sigmas=[1.0]), ValueError, "same number of images"),
    (LR, np.zeros((2, 1, 64, 81), dtype=np.uint8), dict(sigmas=[1.0]), ValueError, "integer multiple"),
    (LR, np.zeros((2, 1, 16 * 17, 20 * 17), dtype=np.uint8), dict(sigmas=[1.0]), ValueError, "integer multiple"),
    (LR, HAT[0], dict(sigmas=[1.0]), ValueError, "3-D"),
])
def test_estimate_rsf_checks_its_arguments_before_the_device(lr, hat, kw, error, word):
    from pssr2_amd.util import estimate_rsf
    with pytest.raises(error, match=word):
        estimate_rsf(lr, hat, **kw)


@pytest.mark.parametrize("kw,error,word", [
    (dict(rsf="search"), ValueError, "rsf"),
    (dict(rsf=-1.0), ValueError, "finite"),
    (dict(rsf=11.0), ValueError, "ceil"),
    (dict(rsf=[1.0]), ValueError, "one sigma per item"),
    (dict(rsf=[1.0, 2.0, 3.0]), ValueError, "one sigma per item"),
    (dict(rsf=[1.0, float("nan")]), ValueError, "finite"),
    (dict(rsf=True), ValueError, "numbers"),
    (dict(rsf=1.0, fit="linear"), ValueError, "fit"),
    (dict(rsf=8.0), ValueError, "margin"),
])
def test_consistency_map_checks_rsf_before_the_device(kw, error, word):
    from pssr2_amd.util import consistency_map
    with pytest.raises(error, match=word):
        consistency_map(LR[..., :14, :], HAT[..., :56, :], **kw)                                     # 14 LR rows: m = 7 leaves nothing
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        consistency_map(torch.zeros(2, 3, 16, 20, dtype=torch.uint8), torch.zeros(2, 1, 64, 80, dtype=torch.uint8), rsf=1.0)


def test_without_a_device_the_reason_is_given(monkeypatch):
    from pssr2_amd.util import consistency_map, estimate_rsf
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="HIP"):
        estimate_rsf(LR, HAT, sigmas=[0.0, 1.0])
    with pytest.raises(RuntimeError, match="HIP"):
        consistency_map(LR, HAT, rsf=1.0)


def test_test_metrics_checks_the_device_before_model_and_dataset():
    from pssr2_amd.predict import test_metrics as metrics_driver

    class Unread:
        def __getattr__(self, name):                           # pragma: no cover
            raise AssertionError(f"the device check comes before model and dataset are touched ({name})")

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        metrics_driver(Unread(), Unread(), device="cpu", metrics=("rsf",))


def test_ops_refuse_host_tensors_and_bad_tables():
    from pssr2_amd import ops
    y, l = torch.zeros(1, 48, 48, dtype=torch.uint8), torch.zeros(1, 12, 12, dtype=torch.uint8)
    taps, rad = ops.rsf_taps(4, [0.0, 1.0])
    assert rad == 3
    with pytest.raises(ValueError, match="uint8 device tensors"):
        ops.rsf_moments_u8(y, l, taps, rad)
    with pytest.raises(ValueError, match="uint8 device tensor"):
        ops.rsf_reduce_u8(y, taps, rad, [0])
    with pytest.raises(ValueError, match="uint8 device tensor"):
        ops.rsf_reduce_u8(y.float(), taps, rad, [0])
    # the table's own checks need no device: shape, sign, row sums, radius
    check = ops._rsf_table
    assert check("t", taps, rad, 4)[1:] == (2, 4) and check("t", taps.tolist(), rad)[1:] == (2, 4)
    neg = taps.copy()
    neg[1, 0], neg[1, 1] = -1, neg[1, 1] + 1
    off = taps.copy()
    off[1, 5] += 1
    for bad, radius, s in ((neg, rad, 4), (off, rad, 4), (taps, rad, 2), (taps, 7, None),(taps[:, :-1], rad, None), (taps[0], rad, None),
                           (taps.astype(np.float64), rad, None), (np.zeros((0, 14), dtype=np.int32), rad, None),
                           (np.tile(taps[:1], (65, 1)), rad, None), (taps, -1, None), (taps, 33, None), (taps, 3.0, None)):
        with pytest.raises(ValueError):
            check("t", bad, radius, s)
    # Pillow's own row at s = 3 sums to 2^22 + 1 and is taken; a row that is off by one at s = 4 is not (above)
    t3, r3 = ops.rsf_taps(3, [0.0, 1.0])
    assert t3.sum(axis=1).tolist() == [F.ONE + 1, F.ONE] and check("t", t3, r3, 3)[1:] == (2, 3)
    assert ops.MAX_RSF_CANDIDATES == 64 and ops.rsf_radius(0) == 0 and ops.rsf_radius(0.25) == 1 and ops.rsf_radius(8.0) == 24


def test_new_arguments_are_keyword_only_and_off_by_default():
    import pssr2_amd
    from pssr2_amd import util as U
    params = inspect.signature(U.estimate_rsf).parameters
    assert [params[k].default for k in ("sigmas", "pool", "pixel_size", "to_numpy")] == [None, "item", 1.0, True]
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("sigmas", "pool", "pixel_size", "to_numpy"))
    p = inspect.signature(U.consistency_map).parameters["rsf"]
    assert p.kind is inspect.Parameter.KEYWORD_ONLY and p.default is None
    assert U.Consistency._fields == ("map", "alpha", "beta", "rse", "rsp")
    assert U.RSFConsistency._fields == ("map", "alpha", "beta", "rse", "rsp", "sigma", "margin")
    assert U.RSF._fields == ("sigma", "fwhm", "score", "curve", "index", "margin")
    assert pssr2_amd.estimate_rsf is U.estimate_rsf
    assert math.isclose(U._FWHM, 2.3548200450309493)


# ------------------------------------------------------------------------------------------------ argument checks of the entry points
def _lib():
    path = ROOT / "pssr2_amd" / "libpssr_mi355.so"
    if not path.exists():
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(str(path))
    lib.pssr_last_error.restype = ctypes.c_char_p
    return lib


def test_rsf_entry_points_validate_without_gpu():
    """Every check happens before the launch: an error code and a message, no crash, no device needed."""
    lib = _lib()
    assert lib.pssr_abi_version() == 5
    i, i64, p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    moments, reduce_, ws, block = lib.pssr_rsf_moments_u8, lib.pssr_rsf_reduce_u8, lib.pssr_rsf_moments_workspace_bytes, lib.pssr_rsf_block
    moments.argtypes = [p] * 4 + [i] * 6 + [p, p]
    reduce_.argtypes = [p] * 4 + [i] * 6 + [p]
    ws.restype, ws.argtypes = i64, [i] * 6
    block.argtypes = [i, i]
    fake = 0x1000          # never dereferenced: every call below fails its checks

    def err(status, word):
        return status == -1 and word in lib.pssr_last_error()

    # y, l, taps, sums, planes, h, w, s, K, radius, workspace / y, taps, sel, d, planes, h, w, s, K, radius
    for hole in range(4):
        ptrs = [None if k == hole else fake for k in range(4)]
        assert err(moments(*ptrs, 2, 32, 32, 4, 3, 2, fake, None), b"null")
        assert err(reduce_(*ptrs, 2, 32, 32, 4, 3, 2, None), b"null")
    assert err(moments(fake, fake, fake, fake, 2, 32, 32, 4, 3, 2, None, None), b"null")
    for call in (lambda *a: moments(fake, fake, fake, fake, *a, fake, None), lambda *a: reduce_(fake, fake, fake, fake, *a, None)):
        for bad in (0, 17, -1, 32):
            assert err(call(2, 32, 32, bad, 3, 2), b"scale")
        for bad in (0, 65, -1):
            assert err(call(2, 32, 32, 4, bad, 2), b"candidates")
        for bad in (-1, 33, 100):
            assert err(call(2, 64, 64, 4, 3, bad), b"radius")
        for bad in ((0, 16, 16), (2, 0, 16), (2, 16, 0), (-1, 16, 16), (2, -16, 16)):
            assert err(call(*bad, 4, 3, 2), b"positive")
        for hw in ((6, 16), (16, 6), (2, 2)):                                                    # radius 8 at scale 4 has m = 3
            assert err(call(1, *hw, 4, 3, 8), b"margin")
        assert err(call(1, 16385, 16384, 1, 1, 0), b"2^28")                                      # one row over 2^28 pixels
        assert err(call(1, 1 << 27, 2, 16, 1, 0), b"2^30")                                       # an axis of y of 2^31
    for bad in ((2, 32, 32, 0, 3, 2), (2, 32, 32, 4, 0, 2), (2, 32, 32, 4, 65, 2), (2, 64, 64, 4, 3, 33), (0, 16, 16, 4, 3, 2), (1, 6, 16, 4, 3, 8),
                (1, 16385, 16384, 1, 1, 0)):
        assert ws(*bad) == 0
    assert ws(1, 7, 7, 4, 3, 8) >= (3 * 3 + 2) * 8 and ws(3, 64, 64, 4, 33, 24) >= 3 * (3 * 33 + 2) * 8       # a row of sums per plane at least
    # the block side: the largest that fits the LDS budget, never 0 for arguments in range
    assert block(1, 0) == 32 and block(4, 24) == 32 and 1 <= block(16, 32) <= 8 and block(0, 0) == 0 and block(17, 0) == 0 and block(4, 33) == 0
    assert all(block(s, r) >= 1 for s in range(1, 17) for r in range(33))
