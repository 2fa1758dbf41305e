"""Decorrelation analysis without a GPU: the numpy restatement of tests/_decorr_ref.py against the definitions and against its own
properties, the algebra that lets two ring sums stand for every filtered curve, util._decorr_resolve on hand-built curves and on the
reference sums of planted, white, constant and blurred images, the argument checks of the Python entry points (raised before any device
work) and of the two C entry points."""
import ctypes
import inspect
import math
from pathlib import Path

import numpy as np
import pytest
import torch

import _decorr_ref as D
import _frc_ref as F

ROOT = Path(__file__).resolve().parent.parent


# ------------------------------------------------------------------------------------------------ the restatement
def test_means_are_rounded_once_and_constant_blocks_vanish():
    one = np.zeros((1, 18, 18), dtype=np.uint8)
    one[0, 3, 5] = 1
    assert D.means(one)[0] == np.float32(1 / 324) and D.means(one).dtype == np.float32
    c = D.centred(one)
    assert c[0, 3, 5] == np.float32(1) - np.float32(1 / 324) and c[0, 0, 0] == -np.float32(1 / 324)
    for v in (0, 200, 255):
        assert not D.centred(np.full((2, 30, 30), v, dtype=np.uint8)).any()
        assert not D.rings_ref(np.full((2, 30, 30), v, dtype=np.uint8), 30).any()
        assert not D.rings_f32(np.full((2, 30, 30), v, dtype=np.uint8), 30, "none").any()


@pytest.mark.parametrize("name", F.WINDOWS)
def test_fft_of_the_centred_windowed_block_is_the_table_form(name):
    rng = np.random.default_rng(1)
    for n in (16, 18, 30):
        a = rng.integers(0, 256, size=(1, n, n), dtype=np.uint8)
        want = D.spectrum_ref(a, n, name)[0, 0]
        got = F.transform_tables64(D.centred(a)[0], n, name)
        np.testing.assert_allclose(got, want, rtol=0, atol=1e-9 * np.abs(want).max())


@pytest.mark.parametrize("n", (16, 18, 30, 64, 100))
def test_ring_populations(n):
    from pssr2_amd.util import _decorr_pop
    R = n // 2
    want = [0] * (R + 1)
    for ky in range(n):
        for kx in range(n):
            r = F.ring_isqrt(ky if ky <= R else ky - n, kx if kx <= R else kx - n)
            if r <= R:
                want[r] += 1
    assert D.pop(n).tolist() == want and _decorr_pop(n).tolist() == want and want[0] == 1


def test_f32_yardstick_is_the_reference_to_round_off():
    """rings_f32 against rings_ref on the GPU tests' inputs: the recorded errors are what this machine's numpy gives again, to the factor
    that another BLAS's blocking may move them by."""
    for n in D.SUMS_SIZES:
        ea, ep = D.f32_error(n)
        print(f"n={n}: rings_f32 against rings_ref: A {ea:.3e} (recorded {D.F32_ERROR[n][0]:.3e}), P {ep:.3e} (recorded {D.F32_ERROR[n][1]:.3e})")
        assert D.F32_ERROR[n][0] / 4 <= ea <= 4 * D.F32_ERROR[n][0] and D.F32_ERROR[n][1] / 4 <= ep <= 4 * D.F32_ERROR[n][1]
        assert D.tol(n) == (8 * D.F32_ERROR[n][0], 8 * D.F32_ERROR[n][1])
    assert set(D.F32_ERROR) == set(D.SUMS_SIZES + D.BIG_SIZES)


def test_sums_inputs_have_an_unrepresentable_mean_somewhere():
    """What makes ring 0 a rounding residue: at n = 18 the mean S / 324 of white noise is no float32."""
    a = D.sums_inputs(18)[0][0]
    S = int(a.astype(np.int64).sum())
    assert float(np.float32(S / 324)) != S / 324


# ------------------------------------------------------------------------------------------------ two ring sums carry every curve
@pytest.mark.parametrize("n,name", [(18, "hann"), (30, "none")])
def test_filtered_curves_from_two_ring_sums_are_the_definition(n, name):
    """d_g(r) is the correlation of the weighted spectrum G = g F (rings 1 .. R) with the normalised spectrum N_r = F / |F| inside rings
    1 .. r: sum Re(G conj N_r) / sqrt(sum |G|^2 sum |N_r|^2), evaluated here on the full spectrum coefficient by coefficient."""
    R = n // 2
    a = F.sums_inputs(n)[0][0]
    spec = D.spectrum_ref(a, n, name)[0, 0]
    rmap = F.ring_map(n)
    sums = D.rings_ref(a, n, name)[0, 0]
    A, P = sums[:, 0].tolist(), sums[:, 1].tolist()
    M = np.concatenate([[0.0], np.cumsum(D.pop(n)[1:])]).tolist()
    assert (np.abs(spec[(rmap >= 1) & (rmap <= R)]) > 0).all()
    for s in (0.15, 1.7, float(R)):
        g = [1.0 - math.exp(-2.0 * s * s * (r / R) ** 2) for r in range(R + 1)]
        got = D.curve_ref(A, P, M, g)
        weight = np.where((rmap >= 1) & (rmap <= R), np.array(g + [0.0] * (2 * n))[np.minimum(rmap, R + 1)], 0.0)
        G = weight * spec
        for r in range(1, R + 1):
            inside = (rmap >= 1) & (rmap <= r)
            N = np.where(inside, spec / np.abs(spec), 0.0)
            want = (G * np.conj(N)).real.sum() / math.sqrt((np.abs(G) ** 2).sum() * (np.abs(N) ** 2).sum())
            assert abs(got[r] - want) <= 1e-12


# ------------------------------------------------------------------------------------------------ the peak rule
def _peak(d):
    from pssr2_amd.util import _decorr_peak
    got, want = _decorr_peak(np.array(d, dtype=np.float64)), D.peak_ref(list(d))
    assert (got is None) == (want is None)
    if got is not None:
        assert got[0] == want[0] and got[1] == pytest.approx(want[1], rel=1e-15) and got[2] == want[2]
    return got


def test_peak_rule_on_hand_built_curves():
    assert _peak([0.0, 0.1, 0.2, 0.3, 0.4, 0.5, 0.6, 0.7, 0.8]) is None                                  # a monotone rise
    assert _peak([0.0, 0.1, 0.2, 0.3, 0.3 - 4e-4, 0.3 - 4e-4, 0.3 - 4e-4, 0.3 - 4e-4, 0.3 - 4e-4]) is None    # a drop of 4e-4
    got = _peak([0.0, 0.1, 0.2, 0.3, 0.3 - 6e-4, 0.3 - 6e-4, 0.3 - 6e-4, 0.3 - 6e-4, 0.3 - 6e-4])            # a drop of 6e-4
    assert got[0] == 3 and got[2] == 0.3
    assert got[1] == pytest.approx(3 + 0.5 * (0.2 - (0.3 - 6e-4)) / (0.2 - 0.6 + 0.3 - 6e-4), rel=1e-14)
    got = _peak([0.0, 0.1, 0.5, 0.5, 0.2, 0.1, 0.0, 0.0, 0.0])                                             # the first of equal maxima
    assert got[0] == 2 and got[1] == pytest.approx(2 + 0.5 * (0.1 - 0.5) / (0.1 - 1.0 + 0.5), rel=1e-14)
    # the maximum sits at the end for e = 8, 7, 6; at e = 5 the peak is ring 4 = e - 1
    got = _peak([0.0, 0.1, 0.2, 0.3, 0.6, 0.5, 0.7, 0.8, 0.9])
    assert got[0] == 4 and got[2] == 0.6
    # a flat top still bends downwards at the first of its maxima
    got = _peak([0.0, 0.5, 0.5, 0.5, 0.2, 0.1, 0.0, 0.0, 0.0])
    assert got[0] == 1 and got[1] == 1.5
    # the second difference at a first maximum is negative unless the curve lies below d[0] = 0 (no curve of sums does; the rule holds
    # anyway): zero, then positive, and the parabola is not used
    got = _peak([0.0, -0.1, -0.2, -0.3, -0.4, -0.5, -0.6, -0.7, -0.8])
    assert got[0] == 1 and got[1] == 1.0 and got[2] == -0.1
    got = _peak([0.0, -0.3, -0.4, -0.5, -0.6, -0.7, -0.8, -0.9, -1.0])
    assert got[0] == 1 and got[1] == 1.0
    # a peak at ring 1 refines against d[0] = 0
    got = _peak([0.0, 0.6, 0.5, 0.1, 0.0, 0.0, 0.0, 0.0, 0.0])
    assert got[0] == 1 and got[1] == pytest.approx(1 + 0.5 * (0.0 - 0.5) / (0.0 - 1.2 + 0.5), rel=1e-14)


def _sums_for(curve_A, n):
    """Ring sums [R + 1][2] with A as given and P = pop: sum_{1..R} P = M(R)."""
    s = np.zeros((n // 2 + 1, 2))
    s[:, 0], s[:, 1] = curve_A, D.pop(n)
    return s


def test_filters_zero_and_one():
    from pssr2_amd.util import _decorr_resolve
    n = 64
    sums = D.rings_ref(D.planted(n, 12, 1)[None], n)
    ref0, ref1, ref10 = (D.resolve_ref(sums, n, k) for k in (0, 1, 10))
    got0, got1 = _decorr_resolve(sums, n, 0, 1.0), _decorr_resolve(sums, n, 1, 1.0)
    assert got0[4].shape == (1, 33) and got1[4].shape == (2, 33) and ref0["curves"].shape == (1, 33)
    assert got0[5] == 0 and got0[2] == pytest.approx(ref0["peak"], rel=1e-12) and ref0["peak"] == ref10["peaks"][0][1]
    # one filter: s_0 = min(2 R / i0, R) alone
    i0 = ref0["peaks"][0][0]
    assert D.family_ref(32, i0, 1) == [min(64 / i0, 32)] and D.family_ref(32, None, 3)[0] == 32.0
    assert D.family_ref(32, i0, 10)[-1] == pytest.approx(0.15, rel=1e-12) and D.family_ref(32, i0, 0) == []
    g = 1.0 - np.exp(-2.0 * (64 / i0) ** 2 * (np.arange(33) / 32) ** 2)
    pooled = sums[0, 0]
    want = np.cumsum((g * pooled[:, 0])[1:]) / np.sqrt((g[1:] ** 2 * pooled[1:, 1]).sum() * np.cumsum(D.pop(n)[1:]))
    np.testing.assert_allclose(got1[4][1, 1:], want, rtol=1e-12)
    np.testing.assert_allclose(got1[4], ref1["curves"], rtol=0, atol=1e-12)
    assert got1[5] == ref1["chosen"] and got1[2] == pytest.approx(ref1["peak"], rel=1e-12)


@pytest.mark.parametrize("n,r0", D.PLANTED)
def test_planted_cutoffs_are_found_just_above_them(n, r0):
    from pssr2_amd.util import _decorr_resolve
    for seed in (1, 2):
        sums = D.rings_ref(D.planted(n, r0, seed)[None], n)
        ref = D.resolve_ref(sums, n)
        res, found, peak, amplitude, curves, chosen = _decorr_resolve(sums, n, 10, 1.0)
        print(f"n={n} r0={r0} seed={seed}: unfiltered peak {ref['peaks'][0][1]:.3f} ({ref['peaks'][0][2]:.3f}), p* = {peak:.3f} on curve {chosen}")
        assert found and ref["found"] and r0 <= peak <= r0 + 1.5 and r0 <= ref["peak"] <= r0 + 1.5
        assert r0 <= ref["peaks"][0][1] <= r0 + 0.5 and 0.8 <= ref["peaks"][0][2] <= 0.9
        assert chosen == ref["chosen"] and abs(peak - ref["peak"]) <= 1e-9 and res == pytest.approx(n / peak, rel=1e-15)
        assert amplitude == pytest.approx(ref["amplitude"], rel=1e-9) and curves.shape == (11, n // 2 + 1)
        np.testing.assert_allclose(curves, ref["curves"], rtol=0, atol=1e-12)
        assert _decorr_resolve(sums, n, 10, 32.5)[0] == pytest.approx(32.5 * res, rel=1e-15)


def test_white_zero_and_constant_images_have_no_peak():
    from pssr2_amd.util import _decorr_resolve
    rng = np.random.default_rng(5)
    for n in (16, 64, 128):
        for name in F.WINDOWS:
            white = rng.integers(0, 256, size=(1, n, n), dtype=np.uint8)
            for a in (white, np.zeros((1, n, n), dtype=np.uint8), np.full((1, n, n), 200, dtype=np.uint8)):
                sums = D.rings_ref(a, n, name)
                res, found, peak, amplitude, curves, chosen = _decorr_resolve(sums, n, 10, 3.0)
                assert not found and res == 6.0 and math.isnan(peak) and amplitude == 0.0 and chosen is None and curves.shape == (11, n // 2 + 1)
                ref = D.resolve_ref(sums, n, pixel_size=3.0)
                assert not ref["found"] and ref["resolution"] == 6.0
    assert not _decorr_resolve(np.zeros((3, 9, 2)), 16, 10, 1.0)[4].any()                                  # zero denominators give zero curves


def test_a_blurred_series_resolves_less_and_less():
    from pssr2_amd.util import _decorr_resolve
    n = 256
    for seed in (3, 4):
        res = []
        for sigma in (1, 1.5, 2, 3, 4):
            r = _decorr_resolve(D.rings_ref(D.blurred(n, sigma, seed)[None], n), n, 10, 1.0)
            assert r[1]
            res.append(r[0])
        print(f"seed={seed}: resolutions {[round(v, 2) for v in res]} pixels for sigma = 1, 1.5, 2, 3, 4")
        assert all(a < b for a, b in zip(res, res[1:])) and 2.0 < res[0] < 3.0 and 8.0 < res[-1] < 12.0


def test_pooling_adds_sums_and_counts_spectra():
    from pssr2_amd.util import _decorr_resolve
    n = 16
    rng = np.random.default_rng(6)
    two = rng.uniform(1, 2, size=(2, 9, 2))
    d = _decorr_resolve(two, n, 0, 1.0)[4][0]
    A, P, pop = two[0, :, 0] + two[1, :, 0], two[0, :, 1] + two[1, :, 1], D.pop(n)
    for r in range(1, 9):
        assert d[r] == pytest.approx(A[1:r + 1].sum() / math.sqrt(P[1:].sum() * 2 * pop[1:r + 1].sum()), rel=1e-14)
    assert d[0] == 0.0
    np.testing.assert_allclose(D.resolve_ref(two, n, 0)["curves"][0], d, rtol=1e-14)
    # leading axes of any shape pool alike; ring 0 never enters
    again = two.reshape(2, 1, 9, 2).copy()
    again[:, :, 0] = 1e9
    np.testing.assert_array_equal(_decorr_resolve(again, n, 0, 1.0)[4][0], d)


def test_block_pooling_returns_maps():
    from pssr2_amd.util import _decorr_assemble
    n = 32
    imgs = np.stack([np.stack([np.block([[D.planted(n, 5 + 2 * (2 * i + j), 20 + c) for j in range(2)] for i in range(2)]) for c in range(3)])
                     for _ in range(2)])
    assert imgs.shape == (2, 3, 64, 64)
    sums = D.rings_ref(imgs.reshape(6, 64, 64), n)
    res, found, peak, amp, curves = _decorr_assemble(sums, 2, 3, 2, 2, n, 4, "block", 1.0, True)
    assert res.shape == found.shape == peak.shape == amp.shape == (2, 2, 2) and curves.shape == (2, 2, 2, 5, 17) and found.dtype == bool
    for i in range(2):
        for k in range(4):
            ref = D.resolve_ref(sums.reshape(2, 3, 4, 17, 2)[i, :, k], n, 4)
            assert found[i, k // 2, k % 2] == ref["found"] and res[i, k // 2, k % 2] == pytest.approx(ref["resolution"], rel=1e-9)
    one = _decorr_assemble(sums[:3], 1, 3, 2, 2, n, 4, "block", 1.0, False)
    assert one[0].shape == (2, 2) and one[4].shape == (2, 2, 5, 17) and np.array_equal(one[0], res[0])
    item = _decorr_assemble(sums, 2, 3, 2, 2, n, 4, "item", 1.0, True)
    assert item[0].shape == (2,) and item[4].shape == (2, 5, 17)
    item = _decorr_assemble(sums[:3], 1, 3, 2, 2, n, 4, "item", 1.0, False)
    assert isinstance(item[0], float) and isinstance(item[1], bool) and item[4].shape == (5, 17)


# ------------------------------------------------------------------------------------------------ argument checks in Python
A = np.zeros((2, 1, 32, 48), dtype=np.uint8)


@pytest.mark.parametrize("a,kw,error,word", [
    (A, dict(window="hamming"), ValueError, "window"),
    (A, dict(filters=-1), ValueError, "filters"),
    (A, dict(filters=65), ValueError, "filters"),
    (A, dict(filters=2.0), ValueError, "filters"),
    (A, dict(filters=True), ValueError, "filters"),
    (A, dict(pool="all"), ValueError, "pool"),
    (A, dict(pixel_size=0), ValueError, "pixel_size"),
    (A, dict(pixel_size="1"), ValueError, "pixel_size"),
    (A, dict(block=17), ValueError, "block"),
    (A, dict(block=14), ValueError, "block"),
    (A, dict(block=34), ValueError, "block"),                                                        # larger than the smaller side
    (A, dict(block=16.0), ValueError, "block"),
    (A, dict(block=True), ValueError, "block"),
    (np.zeros((1, 1, 2048, 2048), dtype=np.uint8), dict(block=1026), ValueError, "block"),
    (A.astype(np.float32), {}, TypeError, "uint8"),
    (torch.zeros(2, 1, 32, 48, dtype=torch.uint8), {}, RuntimeError, "no CPU fallback"),
    (torch.zeros(2, 1, 32, 48), {}, TypeError, "uint8"),                                             # a host tensor of another dtype: the dtype first
    (A[0, 0, 0], {}, ValueError, "shape"),
    (A[None], {}, ValueError, "shape"),
    (A[..., :15, :], {}, ValueError, "16x16"),
    (A[:0], {}, ValueError, "at least one plane"),
    (A.astype(np.float32), dict(window="hamming"), ValueError, "window"),                              # keywords before the image
])
def test_decorr_checks_its_arguments_before_the_device(a, kw, error, word):
    from pssr2_amd.util import decorr
    with pytest.raises(error, match=word):
        decorr(a, **kw)


def test_without_a_device_the_reason_is_given(monkeypatch):
    from pssr2_amd.util import decorr
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    with pytest.raises(RuntimeError, match="HIP"):
        decorr(A)
    with pytest.raises(RuntimeError, match="HIP"):               # numpy scalars are numbers too
        decorr(A, filters=np.int64(3), pixel_size=np.float32(2.0), block=np.int64(16), pool="block")
    with pytest.raises(ValueError, match="pixel_size"):
        decorr(A, pixel_size=np.float64(-1.0))


def test_test_metrics_refuses_decorr_without_a_device_before_the_model_runs():
    from pssr2_amd import predict

    class Untouched:
        def __getattr__(self, name):                           # pragma: no cover
            raise AssertionError(f"the device check comes before model and dataset are touched ({name})")

    with pytest.raises(RuntimeError, match="no CPU fallback"):
        predict.test_metrics(Untouched(), Untouched(), device="cpu", metrics=("psnr", "decorr"))


def test_ops_refuse_host_tensors():
    from pssr2_amd import ops
    t = torch.zeros(1, 32, 32, dtype=torch.uint8)
    with pytest.raises(ValueError, match="uint8 device tensor"):
        ops.decorr_rings_u8(t, 16)
    with pytest.raises(ValueError, match="uint8 device tensor"):
        ops.decorr_rings_u8(t.float(), 16)
    with pytest.raises(ValueError, match="uint8 device tensor"):
        ops.decorr_rings_u8(np.zeros((32, 32), dtype=np.uint8), 16)


def test_new_names_and_defaults():
    import pssr2_amd
    from pssr2_amd import predict, util as U
    params = inspect.signature(U.decorr).parameters
    names = ("block", "window", "filters", "pool", "pixel_size", "to_numpy")
    assert [params[k].default for k in names] == [None, "hann", 10, "item", 1.0, True]
    assert all(params[k].kind is inspect.Parameter.KEYWORD_ONLY for k in names) and list(params) == ["img"] + list(names)
    assert U.Decorr._fields == ("resolution", "found", "peak", "amplitude", "curves", "freq", "block")
    assert pssr2_amd.decorr is U.decorr and U.DECORR_POOLS == ("item", "block")
    assert "decorr" not in inspect.signature(predict.test_metrics).parameters["metrics"].default


# ------------------------------------------------------------------------------------------------ argument checks of the entry points
def _lib():
    path = ROOT / "pssr2_amd" / "libpssr_mi355.so"
    if not path.exists():
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(str(path))
    lib.pssr_last_error.restype = ctypes.c_char_p
    return lib


def test_decorr_entry_points_validate_without_gpu():
    """Every check happens before the launch: an error code and a message, no crash, no device needed."""
    lib = _lib()
    assert lib.pssr_abi_version() == 5
    i, i64, p = ctypes.c_int, ctypes.c_int64, ctypes.c_void_p
    rings, ws = lib.pssr_decorr_rings_u8, lib.pssr_decorr_workspace_bytes
    rings.argtypes = [p] * 4 + [i] * 4 + [p, i64, p]
    ws.restype, ws.argtypes = i64, [i] * 4
    fake, big = 0x1000, 1 << 40          # never dereferenced: every call below fails its checks

    def err(status, word):
        return status == -1 and word in lib.pssr_last_error()

    # a, ct, st, sums, planes, H, W, n, workspace, workspace_bytes
    for hole in range(4):
        ptrs = [None if k == hole else fake for k in range(4)]
        assert err(rings(*ptrs, 2, 64, 64, 32, fake, big, None), b"null")
    assert err(rings(*[fake] * 4, 2, 64, 64, 32, None, big, None), b"null")
    for bad in ((0, 64, 64), (2, 0, 64), (2, 64, 0), (-1, 64, 64), (2, -64, 64)):
        assert err(rings(*[fake] * 4, *bad, 32, fake, big, None), b"positive")
        assert ws(*bad, 32) == 0
    for bad in (0, 14, 17, 33, 1026, 2048, -16):
        assert err(rings(*[fake] * 4, 1, 4096, 4096, bad, fake, big, None), b"block side")
        assert ws(1, 4096, 4096, bad) == 0
    for hw in ((31, 64), (64, 31), (16, 16)):
        assert err(rings(*[fake] * 4, 1, *hw, 32, fake, big, None), b"does not fit")
        assert ws(1, *hw, 32) == 0
    assert err(rings(*[fake] * 4, (1 << 20) + 1, 64, 64, 16, fake, big, None), b"2^24")
    assert ws((1 << 20) + 1, 64, 64, 16) == 0
    need = ws(2, 64, 64, 32)
    for short in (0, -1, need - 1):
        assert err(rings(*[fake] * 4, 2, 64, 64, 32, fake, short, None), b"short")
    # T of one image (two [n][n/2+1] float planes), one row of partial sums and a mean per block at least, never much above 256 MB,
    # and less than the pair needs
    frc_ws = lib.pssr_frc_workspace_bytes
    frc_ws.restype, frc_ws.argtypes = i64, [i] * 4
    assert ws(1, 16, 16, 16) >= 2 * 16 * 9 * 4 + 9 * 2 * 8 + 4
    assert ws(3, 500, 500, 500) >= 3 * (2 * 500 * 251 * 4 + 251 * 2 * 8 + 4)
    assert ws(3, 500, 500, 500) < frc_ws(3, 500, 500, 500)
    assert 0 < ws(1, 8192, 8192, 512) <= 260 << 20
