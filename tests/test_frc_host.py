"""Fourier ring correlation without a GPU: the numpy restatement of tests/_frc_ref.py against the definitions and against its own
properties, util._frc_resolve on hand-built curves, the argument checks of the Python entry points (raised before any device work), the
argument checks of the two C entry points, and the fitness of the planted inputs that the GPU tests rely on."""
import ctypes
import inspect
import math
from pathlib import Path

import numpy as np
import pytest
import torch

import _frc_ref as F

ROOT = Path(__file__).resolve().parent.parent


# ------------------------------------------------------------------------------------------------ the restatement
@pytest.mark.parametrize("name", F.WINDOWS)
@pytest.mark.parametrize("n", (16, 18, 30))
def test_tables_are_the_definition(n, name):
    """ops.frc_tables and the restatement against a scalar evaluation of step 1 with math.cos / math.sin: float32 [n][n], within half a
    float32 ulp of 1 plus the libm / numpy difference of a float64 cosine."""
    from pssr2_amd import ops
    want_c, want_s = np.zeros((n, n)), np.zeros((n, n))
    for x in range(n):
        w = math.sin(math.pi * (x + 0.5) / n) ** 2 if name == "hann" else 1.0
        for k in range(n):
            angle = 2.0 * math.pi * ((x * k) % n) / n
            want_c[x, k], want_s[x, k] = w * math.cos(angle), -w * math.sin(angle)
    for ct, st in (ops.frc_tables(n, name), F.tables(n, name)):
        assert ct.dtype == np.float32 and st.dtype == np.float32 and ct.shape == st.shape == (n, n)
        np.testing.assert_allclose(ct, want_c, rtol=0, atol=6.1e-8)
        np.testing.assert_allclose(st, want_s, rtol=0, atol=6.1e-8)
    assert all(np.array_equal(p, q) for p, q in zip(ops.frc_tables(n, name), F.tables(n, name)))
    assert ops.frc_tables(n, name)[0] is ops.frc_tables(n, name)[0]          # made once
    assert ops.FRC_WINDOWS == F.WINDOWS == ("hann", "none")


@pytest.mark.parametrize("name", F.WINDOWS)
def test_fft_of_the_windowed_block_is_the_table_form(name):
    """rings_ref's transform (numpy fft2 of block x w (x) w) is W^T a W with W = Ct + i St, in float64."""
    rng = np.random.default_rng(1)
    for n in (16, 18, 30):
        block = rng.integers(0, 256, size=(n, n), dtype=np.uint8)
        w = F.window(n, name)
        want = np.fft.fft2(block * (w[:, None] * w[None, :]))
        got = F.transform_tables64(block, n, name)
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-9 * np.abs(want).max())


@pytest.mark.parametrize("n", (16, 18, 30, 64, 100))
def test_the_two_ring_index_forms_agree(n):
    rmap = F.ring_map(n)
    for ky in range(n):
        fy = ky if ky <= n // 2 else ky - n
        for kx in range(n):
            fx = kx if kx <= n // 2 else kx - n
            assert F.ring_isqrt(fy, fx) == F.ring_floor(fy, fx) == rmap[ky, kx] == F.ring_isqrt(fy, kx if kx <= n // 2 else n - kx)


@pytest.mark.parametrize("n", (16, 18, 30, 64, 100))
def test_kept_rings_count_every_coefficient_once(n):
    """With |F|^2 = 1 everywhere the sums are the ring populations: they add up to the number of full-spectrum coefficients with r <= R,
    in rings_ref's full-spectrum form and in the half-spectrum form with doubled interior columns alike."""
    R = n // 2
    ones = np.ones((1, 1, n, n), dtype=np.complex128)
    counts = F._ring_sums(ones, ones, n)[0, 0]
    kept = int((F.ring_map(n) <= R).sum())
    assert counts.shape == (R + 1, 3) and np.array_equal(counts[:, 0], counts[:, 1]) and counts[:, 1].sum() == kept
    assert counts[0, 1] == 1 and kept < n * n
    half = np.zeros(R + 1)
    for ky in range(n):
        for kx in range(R + 1):
            r = F.ring_map(n)[ky, kx]
            if r <= R:
                half[r] += 2 if 0 < kx < R else 1
    assert np.array_equal(half, counts[:, 1])


def test_f32_yardstick_is_the_reference_to_round_off():
    """rings_f32 (two float32 matrix products, half spectrum) against rings_ref (float64 fft2, full spectrum) on the GPU tests' inputs: the
    recorded errors are what this machine's numpy gives again, to the factor that another BLAS's blocking may move them by."""
    for n in F.SUMS_SIZES:
        got = F.f32_error(n)
        print(f"n={n}: max |rings_f32 - rings_ref| / sqrt(Saa Sbb) = {got:.3e} (recorded {F.F32_ERROR[n]:.3e})")
        assert F.F32_ERROR[n] / 4 <= got <= 4 * F.F32_ERROR[n]
        assert F.TOL[n] == 8 * F.F32_ERROR[n]
    assert set(F.TOL) == set(F.SUMS_SIZES + F.BIG_SIZES)


def test_blocks_are_the_centred_grid():
    rng = np.random.default_rng(2)
    img = rng.integers(0, 256, size=(2, 40, 70), dtype=np.uint8)
    assert F.grid(40, 70, 16) == (2, 4, 4, 3) and F.grid(37, 53, 18) == (2, 2, 0, 8)
    b = F.blocks(img, 16)
    assert b.shape == (2, 8, 16, 16)
    np.testing.assert_array_equal(b[1, 5], img[1, 4 + 16:4 + 32, 3 + 16:3 + 32])


# ------------------------------------------------------------------------------------------------ curve and crossing
def _sums_of(curve, n):
    """Ring sums whose correlation is `curve`: Saa = Sbb = 1, Sab = curve."""
    s = np.ones((n // 2 + 1, 3))
    s[:, 0] = curve
    return s


def test_resolve_a_crossing_between_rings():
    from pssr2_amd.util import _frc_resolve
    n = 16
    curve = [1.0, 0.9, 0.8, 0.5, 0.1, 0.0, 0.0, 0.0, 0.0]
    got, res, crossed = _frc_resolve(_sums_of(curve, n), n, 0.3, 0, 1.0)
    r_star = 3 + (0.5 - 0.3) / (0.5 - 0.1)
    np.testing.assert_allclose(got, curve, rtol=1e-15)
    assert crossed and res == pytest.approx(n / r_star, rel=1e-15)
    ref = F.curve_ref(_sums_of(curve, n), n, 0.3)
    assert ref[1] == pytest.approx(r_star, rel=1e-15) and ref[2] == pytest.approx(res, rel=1e-15) and ref[3]
    # pixel_size scales the resolution only
    assert _frc_resolve(_sums_of(curve, n), n, 0.3, 0, 2.5)[1] == pytest.approx(2.5 * n / r_star, rel=1e-15)
    # planes and blocks pool their sums, not their curves
    a, b = _sums_of(curve, n), _sums_of([1.0] * 9, n) * 3
    pooled = _frc_resolve(np.stack([a, b]), n, 0.3, 0, 1.0)[0]
    np.testing.assert_allclose(pooled, (np.array(curve) + 3) / 4, rtol=1e-15)


def test_resolve_the_first_ring_below_the_threshold():
    from pssr2_amd.util import _frc_resolve
    n = 16
    curve = [1.0, 0.05] + [0.0] * 7
    _, res, crossed = _frc_resolve(_sums_of(curve, n), n, 1 / 7, 0, 1.0)
    r_star = (1.0 - 1 / 7) / (1.0 - 0.05)
    assert crossed and res == pytest.approx(n / r_star, rel=1e-15) and F.curve_ref(_sums_of(curve, n), n)[1] == pytest.approx(r_star, rel=1e-15)
    # ring 0 below the threshold as well (an all-zero pair): r* = 1, no division by zero
    _, res, crossed = _frc_resolve(_sums_of([0.0] * 9, n), n, 1 / 7, 0, 1.0)
    assert crossed and res == n and F.curve_ref(_sums_of([0.0] * 9, n), n)[1:] == (1.0, n, True)


def test_resolve_no_crossing_is_the_sampling_limit():
    from pssr2_amd.util import _frc_resolve
    n = 18
    curve, res, crossed = _frc_resolve(_sums_of([1.0] * 10, n), n, 1 / 7, 0, 3.0)
    assert not crossed and res == 6.0 and np.array_equal(curve, np.ones(10))
    assert F.curve_ref(_sums_of([1.0] * 10, n), n, pixel_size=3.0)[1:] == (None, 6.0, False)


def test_smooth_never_pulls_ring_zero_in():
    from pssr2_amd.util import _frc_resolve
    n = 16
    sums = np.ones((9, 3))
    sums[:, 0] = [-1.0, 0.8, 0.6, 0.4, 0.2, 0.0, 0.0, 0.0, 0.0]
    sums[0] = [-100.0, 100.0, 100.0]                            # a ring 0 that would ruin rings 1 and 2 if pooled
    for k in (1, 2, 20):
        curve = _frc_resolve(sums, n, 1 / 7, k, 1.0)[0]
        want = [-1.0] + [sums[max(1, r - k):min(8, r + k) + 1, 0].sum() / len(sums[max(1, r - k):min(8, r + k) + 1]) for r in range(1, 9)]
        np.testing.assert_allclose(curve, want, rtol=1e-14)
        np.testing.assert_allclose(F.curve_ref(sums, n, smooth=k)[0], want, rtol=1e-14)
    np.testing.assert_allclose(_frc_resolve(sums, n, 1 / 7, 0, 1.0)[0], sums[:, 0] / sums[:, 1], rtol=1e-15)


def test_zero_denominators_give_zero():
    from pssr2_amd.util import _frc_resolve
    n = 16
    sums = np.ones((9, 3))
    sums[2] = [0.5, 0.0, 1.0]
    sums[3] = [0.0, 0.0, 0.0]
    curve, res, crossed = _frc_resolve(sums, n, 1 / 7, 0, 1.0)
    assert curve[2] == 0.0 and curve[3] == 0.0 and curve[1] == 1.0 and crossed
    assert res == pytest.approx(n / (1 + (1 - 1 / 7)), rel=1e-15)
    assert np.array_equal(F.curve_ref(sums, n)[0], curve)
    curve, res, crossed = _frc_resolve(np.zeros((2, 3, 9, 3)), n, 1 / 7, 0, 1.0)
    assert np.array_equal(curve, np.zeros(9)) and crossed and res == n


# ------------------------------------------------------------------------------------------------ the planted inputs are fit for purpose
@pytest.mark.parametrize("n,r0", ((64, 12), (128, 24), (250, 40)))
def test_planted_pairs_cross_just_above_their_cutoff(n, r0):
    """What the GPU tests' bound of 1e-3 rings on r* rests on: the reference curve alone is near 1 up to r0 and falls through 1/7 within
    five rings above it (the Hann window widens the edge by about two rings), steeply."""
    for seed in range(3):
        a, b = F.planted_pair(n, r0, seed)
        assert a.dtype == np.uint8 and a.shape == (n, n) and not np.array_equal(a, b)
        curve, r_star, res, crossed = F.curve_ref(F.rings_ref(a[None], b[None], n), n)
        print(f"n={n} r0={r0} seed={seed}: min frc[1..r0] = {curve[1:r0 + 1].min():.4f}, r* = {r_star:.3f}")
        assert curve[1:r0 + 1].min() >= 0.95
        assert crossed and r0 < r_star <= r0 + 5 and res == pytest.approx(n / r_star)
        r = int(math.floor(r_star)) + 1                         # the ring of the crossing
        assert curve[r - 1] - curve[r] > 0.1                    # the slope the bound on r* assumes


# ------------------------------------------------------------------------------------------------ argument checks in Python
A = np.zeros((2, 1, 32, 48), dtype=np.uint8)


@pytest.mark.parametrize("a,b,kw,error,word", [
    (A, A, dict(window="hamming"), ValueError, "window"),
    (A, A, dict(threshold=0), ValueError, "threshold"),
    (A, A, dict(threshold=1), ValueError, "threshold"),
    (A, A, dict(threshold=1.5), ValueError, "threshold"),
    (A, A, dict(threshold="0.5"), ValueError, "threshold"),
    (A, A, dict(smooth=-1), ValueError, "smooth"),
    (A, A, dict(smooth=1.0), ValueError, "smooth"),
    (A, A, dict(smooth=True), ValueError, "smooth"),
    (A, A, dict(pixel_size=0), ValueError, "pixel_size"),
    (A, A, dict(block=17), ValueError, "block"),
    (A, A, dict(block=14), ValueError, "block"),
    (A, A, dict(block=34), ValueError, "block"),                                                      # larger than the smaller side
    (A, A, dict(block=16.0), ValueError, "block"),
    (A, A, dict(block=True), ValueError, "block"),
    (np.zeros((1, 1, 2048, 2048), dtype=np.uint8), np.zeros((1, 1, 2048, 2048), dtype=np.uint8), dict(block=1026), ValueError, "block"),
    (A.astype(np.float32), A, {}, TypeError, "uint8"),
    (A, A.astype(np.int16), {}, TypeError, "uint8"),
    (torch.zeros(2, 1, 32, 48, dtype=torch.uint8), torch.zeros(2, 1, 32, 48, dtype=torch.uint8), {}, RuntimeError, "no CPU fallback"),
    (torch.zeros(2, 1, 32, 48), torch.zeros(2, 1, 32, 48), {}, TypeError, "uint8"),                       # a host tensor of another dtype: the dtype first
    (A, A[:1], {}, ValueError, "same shape"),
    (A, A[..., :32], {}, ValueError, "same shape"),
    (A[0, 0, 0], A[0, 0, 0], {}, ValueError, "same shape"),
    (A[None], A[None], {}, ValueError, "same shape"),
    (A[..., :15, :], A[..., :15, :], {}, ValueError, "16x16"),
    (A[:0], A[:0], {}, ValueError, "at least one plane"),
])
def test_frc_checks_its_arguments_before_the_device(a, b, kw, error, word):
    from pssr2_amd.util import frc
    with pytest.raises(error, match=word):
        frc(a, b, **kw)


def test_without_a_device_the_reason_is_given(monkeypatch):
    from pssr2_amd.util import frc
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="HIP"):
        frc(A, A)


def test_numpy_scalars_are_numbers_too(monkeypatch):
    """np.float32 / np.int64 keywords pass the checks (the call then stops at the missing device), their bad values do not."""
    from pssr2_amd.util import frc
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="HIP"):
        frc(A, A, threshold=np.float32(0.25), pixel_size=np.float32(2.0), smooth=np.int64(1), block=np.int64(16))
    with pytest.raises(ValueError, match="threshold"):
        frc(A, A, threshold=np.float32(1.5))
    with pytest.raises(ValueError, match="pixel_size"):
        frc(A, A, pixel_size=np.float64(-1.0))


def test_test_metrics_refuses_frc_without_a_device_before_the_model_runs():
    from pssr2_amd import predict

    class Untouched:
        def __getattr__(self, name):                           # pragma: no cover
            raise AssertionError(f"the device check comes before model and dataset are touched ({name})")

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        predict.test_metrics(Untouched(), Untouched(), device="cpu", metrics=("psnr", "frc"))


def test_ops_refuse_host_tensors_and_wrong_arguments():
    from pssr2_amd import ops
    t = torch.zeros(1, 32, 32, dtype=torch.uint8)
    with pytest.raises(ValueError, match="uint8 device tensors"):
        ops.frc_rings_u8(t, t, 16)
    with pytest.raises(ValueError, match="uint8 device tensors"):
        ops.frc_rings_u8(t.float(), t.float(), 16)
    for bad in (15, 14, 1026, 16.0, True):
        with pytest.raises(ValueError, match="block"):
            ops.frc_tables(bad)
    with pytest.raises(ValueError, match="window"):
        ops.frc_tables(16, "hamming")


def test_new_names_and_defaults():
    import pssr2_amd
    from pssr2_amd import util as U
    params = inspect.signature(U.frc).parameters
    assert [params[k].default for k in ("block", "window", "threshold", "smooth", "pixel_size", "to_numpy")] == [None, "hann", 1 / 7, 0, 1.0, True]
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in ("block", "window", "threshold", "smooth", "pixel_size", "to_numpy"))
    assert U.FRC._fields == ("curve", "freq", "resolution", "crossed", "block")
    assert pssr2_amd.frc is U.frc
    from pssr2_amd import predict
    assert "frc" not in inspect.signature(predict.test_metrics).parameters["metrics"].default


# ------------------------------------------------------------------------------------------------ argument checks of the entry points
def _lib():
    path = ROOT / "pssr2_amd" / "libpssr_mi355.so"
    if not path.exists():
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(str(path))
    lib.pssr_last_error.restype = ctypes.c_char_p
    return lib


def test_frc_entry_points_validate_without_gpu():
    """Every check happens before the launch: an error code and a message, no crash, no device needed."""
    lib = _lib()
    assert lib.pssr_abi_version() == 5
    i, i64, p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    rings, ws = lib.pssr_frc_rings_u8, lib.pssr_frc_workspace_bytes
    rings.argtypes = [p] * 5 + [i] * 4 + [p, p]
    ws.restype, ws.argtypes = i64, [i] * 4
    fake = 0x1000          # never dereferenced: every call below fails its checks

    def err(status, word):
        return status == -1 and word in lib.pssr_last_error()

    # a, b, ct, st, sums, planes, H, W, n, workspace
    for hole in range(5):
        ptrs = [None if k == hole else fake for k in range(5)]
        assert err(rings(*ptrs, 2, 64, 64, 32, fake, None), b"null")
    assert err(rings(*[fake] * 5, 2, 64, 64, 32, None, None), b"null")
    for bad in ((0, 64, 64), (2, 0, 64), (2, 64, 0), (-1, 64, 64), (2, -64, 64)):
        assert err(rings(*[fake] * 5, *bad, 32, fake, None), b"positive")
        assert ws(*bad, 32) == 0
    for bad in (0, 14, 17, 33, 1026, 2048, -16):
        assert err(rings(*[fake] * 5, 1, 4096, 4096, bad, fake, None), b"block side")
        assert ws(1, 4096, 4096, bad) == 0
    for hw in ((31, 64), (64, 31), (16, 16)):
        assert err(rings(*[fake] * 5, 1, *hw, 32, fake, None), b"does not fit")
        assert ws(1, *hw, 32) == 0
    assert err(rings(*[fake] * 5, (1 << 20) + 1, 64, 64, 16, fake, None), b"2^24")             # 16 blocks a plane: 2^24 + 16 in all
    assert ws((1 << 20) + 1, 64, 64, 16) == 0
    # T of both images (four [n][n/2+1] float planes) and one row of partial sums per block at least, and never much above 256 MB
    assert ws(1, 16, 16, 16) >= 4 * 16 * 9 * 4 + 9 * 3 * 8
    assert ws(3, 500, 500, 500) >= 3 * (4 * 500 * 251 * 4 + 251 * 3 * 8)
    assert 0 < ws(1, 8192, 8192, 512) <= 260 << 20
