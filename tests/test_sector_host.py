"""Directional resolution without a device: the restatement of tests/_sector_ref.py against scalar loops and against the text of
include/pssr_mi355.h ("Directional resolution"), the host halves of util.frc_sectors / decorr_sectors against the restatement, every new
argument check, and the recovery of a planted anisotropy by the restatement alone."""
import ctypes
import math

import numpy as np
import pytest

import _decorr_ref as D
import _frc_ref as F
import _sector_ref as Q

SECTORS = (1, 2, 3, 4, 8, 16)


# ------------------------------------------------------------------------------------------------ the sector of a coefficient
def _sector_scalar(n, S, ky, kx):
    """Step S2 in Python ints, one coefficient of the full spectrum."""
    if kx > n // 2:
        ky, kx = (n - ky) % n, n - kx
    fy = ky if ky <= n // 2 else ky - n
    gx, gy = (kx, fy) if fy >= 0 else (-kx, -fy)
    count = 0
    for j in range(S):
        beta = (j + 0.5) * math.pi / S
        bx, by = round(2 ** 20 * math.cos(beta)), round(2 ** 20 * math.sin(beta))
        assert abs(bx * gy) < 2 ** 30 and abs(by * gx) < 2 ** 30
        count += bx * gy - by * gx >= 0
    return count % S


@pytest.mark.parametrize("n", (16, 18, 30))
def test_sector_map_against_a_scalar_loop(n):
    from pssr2_amd import ops
    for S in SECTORS:
        got = Q.sector_map(n, S)
        want = np.array([[_sector_scalar(n, S, ky, kx) for kx in range(n)] for ky in range(n)])
        np.testing.assert_array_equal(got, want)
        assert got.min() == 0 and got.max() == S - 1
        bx, by = ops.frc_sector_bounds(S)
        assert bx.dtype == np.int32 and by.dtype == np.int32 and bx.shape == (S,)
        np.testing.assert_array_equal(bx, Q.bounds(S)[0])
        np.testing.assert_array_equal(by, Q.bounds(S)[1])
        assert (by > 0).all() and (np.diff(np.arctan2(by, bx)) > 0).all()        # strictly inside the upper half plane, ascending
    assert not Q.sector_map(n, 1).any()


def test_sectors_are_centred_on_their_directions_and_ties_fall_as_stated():
    n = 16
    two = Q.sector_map(n, 2)
    assert two[0, 0] == 0                                       # the origin
    assert two[0, 1] == 0 and two[0, 5] == 0                    # along x
    assert two[1, 0] == 1 and two[n - 1, 0] == 1                # along y, either sign
    assert two[3, 3] == 1 and two[n - 3, n - 3] == 1            # gy = gx (and its mirror): sector 1
    assert two[n - 3, 3] == 0 and two[3, n - 3] == 0            # gy = -gx (and its mirror): sector 0
    four = Q.sector_map(n, 4)
    assert four[0, 4] == 0 and four[4, 4] == 1 and four[4, 0] == 2 and four[n - 4, 4] == 3
    # a coefficient and its Hermitian mirror share a sector, for every S: what doubling the columns 0 < kx < n / 2 rests on (the Nyquist
    # column kx = n / 2 is its own mirror column, visited once, and its rows fy and -fy are told apart as kept coefficients)
    ky, kx = np.meshgrid(np.arange(n), np.arange(n), indexing="ij")
    for S in SECTORS:
        m = Q.sector_map(n, S)
        off = kx != n // 2
        np.testing.assert_array_equal(m[off], m[(n - ky) % n, (n - kx) % n][off])


# ------------------------------------------------------------------------------------------------ populations
@pytest.mark.parametrize("n,totals", [(16, (108, 107)), (18, (140, 139)), (64, (1646, 1645))])
def test_populations(n, totals):
    from pssr2_amd import ops
    for S in SECTORS:
        p = Q.pop(n, S)
        assert p.shape == (n // 2 + 1, S) and p.dtype == np.int64
        np.testing.assert_array_equal(p.sum(axis=1), D.pop(n))
        got = ops.frc_sector_pop(n, S)
        assert got.dtype == np.int64
        np.testing.assert_array_equal(got, p)
    assert tuple(Q.pop(n, 2).sum(axis=0)) == totals
    assert (Q.pop(n, 8)[1:] == 0).sum() == 6 and (Q.pop(n, 16)[1:] == 0).sum() in (32, 33)


# ------------------------------------------------------------------------------------------------ sums
@pytest.mark.parametrize("n", (16, 18, 30, 64))
def test_sector_sums_add_up_to_the_ring_sums(n):
    """Regrouping a ring's fewer than 3300 terms costs at most 3300 eps = 3.6e-13 of sum |terms|, and sum |Re(Fa conj Fb)| <= sqrt(Saa Sbb)
    (Cauchy-Schwarz): 1e-12 sqrt(Saa Sbb) per ring."""
    for a, b, name in Q.sums_inputs(n):
        ref = F.rings_ref(a, b, n, name)
        dref = D.rings_ref(a, n, name)
        for S in SECTORS:
            got = Q.sectors_ref(a, b, n, S, name)
            assert got.shape == (1, 1, n // 2 + 1, S, 3)
            assert (np.abs(got.sum(axis=-2) - ref) <= 1e-12 * F.scale_of(ref)[..., None]).all()
            assert not got[0, 0][Q.pop(n, S) == 0].any()        # an empty cell holds exactly nothing
            dgot = Q.decorr_sectors_ref(a, n, S, name)
            assert (np.abs(dgot.sum(axis=-2) - dref) <= 1e-12 * np.maximum(dref, dref[..., 1:].sum())).all()
        np.testing.assert_array_equal(Q.sectors_ref(a, b, n, 1, name)[..., 0, :], ref)


def test_f32_yardstick_is_the_reference_to_round_off():
    """sectors_f32 against sectors_ref on the GPU tests' inputs: the recorded errors are what this machine's numpy gives again, to the
    factor that another BLAS's blocking may move them by."""
    for n in Q.SUMS_SIZES:
        e, (ea, ep) = Q.f32_error(n)
        print(f"n={n}: sectors_f32 against sectors_ref {e:.3e} (recorded {Q.F32_ERROR[n]:.3e}); decorrelation A {ea:.3e} "
              f"(recorded {Q.DECORR_F32_ERROR[n][0]:.3e}), P {ep:.3e} (recorded {Q.DECORR_F32_ERROR[n][1]:.3e})")
        assert Q.F32_ERROR[n] / 4 <= e <= 4 * Q.F32_ERROR[n]
        assert Q.DECORR_F32_ERROR[n][0] / 4 <= ea <= 4 * Q.DECORR_F32_ERROR[n][0] and Q.DECORR_F32_ERROR[n][1] / 4 <= ep <= 4 * Q.DECORR_F32_ERROR[n][1]
        assert Q.tol(n) == 8 * Q.F32_ERROR[n] and Q.decorr_tol(n) == (8 * Q.DECORR_F32_ERROR[n][0], 8 * Q.DECORR_F32_ERROR[n][1])
    sizes = set(Q.SUMS_SIZES) | {n for n, _ in Q.BIG}
    assert set(Q.F32_ERROR) == sizes and set(Q.DECORR_F32_ERROR) == sizes


# ------------------------------------------------------------------------------------------------ the curve and its empty cells
def _sums_of(curve):
    """Ring sums [R + 1][3] whose correlation is ``curve`` (Saa = Sbb = 1)."""
    return np.array([[c, 1.0, 1.0] for c in curve])


def _both(sums, counts, n, **kw):
    """The restatement and util._frc_resolve_sector on the same sums: equal curves, flags and resolutions."""
    from pssr2_amd.util import _frc_resolve_sector
    curve, r_star, resolution, crossed = Q.curve_ref(sums, counts, n, **kw)
    got = _frc_resolve_sector(sums, counts, n, kw.get("threshold", 1 / 7), kw.get("smooth", 0), kw.get("pixel_size", 1.0))
    np.testing.assert_array_equal(got[0], curve)
    assert got[2] is crossed and got[1] == pytest.approx(resolution, rel=1e-14)
    return curve, r_star, resolution, crossed


def test_empty_cells_are_skipped_by_the_crossing_search():
    n = 16
    full = [1.0, 0.9, 0.8, 0.1, 0.05, 0.0, 0.0, 0.0, 0.0]
    ones = np.ones(9, dtype=np.int64)
    # no empty cell: step 5 of FRC
    curve, r_star, resolution, crossed = _both(_sums_of(full), ones, n, threshold=0.5)
    assert crossed and r_star == pytest.approx(2 + 0.3 / 0.7) and resolution == pytest.approx(n / r_star)
    assert r_star == pytest.approx(F.curve_ref(_sums_of(full), n, threshold=0.5)[1], rel=1e-15)
    # a crossing right after a skipped ring: interpolated from ring 1 to ring 3
    counts = ones.copy()
    counts[2] = 0
    curve, r_star, _, crossed = _both(_sums_of(full), counts, n, threshold=0.5)
    assert crossed and math.isnan(curve[2]) and not np.isnan(np.delete(curve, 2)).any()
    assert r_star == pytest.approx(1 + (0.9 - 0.5) / (0.9 - 0.1) * 2)
    # a skipped ring that lies below the threshold does not cross
    low = list(full)
    low[2] = 0.0
    assert _both(_sums_of(low), counts, n, threshold=0.5)[1] == pytest.approx(2.0)
    # a skipped ring 1: from ring 0 to ring 2
    counts = ones.copy()
    counts[1] = 0
    curve, r_star, _, _ = _both(_sums_of([1.0, 0.0, 0.25, 0, 0, 0, 0, 0, 0]), counts, n, threshold=0.5)
    assert math.isnan(curve[1]) and r_star == pytest.approx(0 + (1.0 - 0.5) / (1.0 - 0.25) * 2)
    # ring 0 below the threshold too, or unpopulated (every sector but 0): r* = 1
    assert _both(_sums_of([0.2, 0.1, 0, 0, 0, 0, 0, 0, 0]), ones, n, threshold=0.5)[1] == 1.0
    counts = ones.copy()
    counts[0] = counts[1] = 0
    curve, r_star, resolution, crossed = _both(_sums_of([1.0, 0.9, 0.3, 0, 0, 0, 0, 0, 0]), counts, n, threshold=0.5)
    assert math.isnan(curve[0]) and crossed and r_star == 1.0 and resolution == float(n)
    # smooth fills a cell: ring 2 pools rings 1 .. 3 of sums and of populations
    counts = ones.copy()
    counts[2] = 0
    sums = _sums_of(full)
    sums[2] = 0
    curve, r_star, _, _ = _both(sums, counts, n, threshold=0.5, smooth=1)
    assert not np.isnan(curve).any() and curve[2] == pytest.approx((0.9 + 0.1) / 2) and curve[1] == pytest.approx(0.9)
    # no crossing
    curve, r_star, resolution, crossed = _both(_sums_of([1.0] * 9), counts, n, pixel_size=3.0)
    assert r_star is None and not crossed and resolution == 6.0


def test_the_curve_of_one_sector_is_the_ring_curve():
    n = 64
    a, b = F.planted_pair(n, 12, 0)
    sums = F.rings_ref(a[None], b[None], n)
    for smooth in (0, 2):
        want = F.curve_ref(sums, n, smooth=smooth)
        got = _both(Q.sectors_ref(a[None], b[None], n, 1)[..., 0, :], Q.pop(n, 1)[:, 0], n, smooth=smooth)
        np.testing.assert_array_equal(got[0], want[0])
        assert got[1:] == want[1:]


def test_decorr_resolve_default_population_is_todays():
    from pssr2_amd import ops
    from pssr2_amd.util import _decorr_pop, _decorr_resolve
    n = 64
    sums = D.rings_ref(np.stack([D.blurred(n, 1.5, s) for s in range(2)]), n)
    for filters in (0, 10):
        old = _decorr_resolve(sums, n, filters, 1.5)
        for new in (_decorr_resolve(sums, n, filters, 1.5, None), _decorr_resolve(sums, n, filters, 1.5, _decorr_pop(n)),
                    _decorr_resolve(sums, n, filters, 1.5, ops.frc_sector_pop(n, 1)[:, 0])):
            assert new[:4] == old[:4] and new[5] == old[5]
            assert np.array_equal(new[4], old[4])
    # a sector's populations: the restatement
    S = 4
    cells = Q.decorr_sectors_ref(D.blurred(n, 1.5, 0)[None], n, S)
    for s in range(S):
        got = _decorr_resolve(cells[..., s, :], n, 10, 1.0, Q.pop(n, S)[:, s])
        want = Q.decorr_resolve_ref(cells[..., s, :], Q.pop(n, S)[:, s], n)
        assert got[1] == want["found"] and got[0] == pytest.approx(want["resolution"], rel=1e-9)
        assert np.abs(got[4] - want["curves"]).max() <= 1e-12


# ------------------------------------------------------------------------------------------------ checks
def test_python_argument_checks():
    from pssr2_amd import ops
    from pssr2_amd.predict import test_metrics
    from pssr2_amd.util import decorr_sectors, frc_sectors
    import pssr2_amd
    assert pssr2_amd.frc_sectors is frc_sectors and pssr2_amd.decorr_sectors is decorr_sectors
    img = np.zeros((32, 32), dtype=np.uint8)
    for bad in (0, 17, -1, 2.0, True, None, "2"):
        with pytest.raises(ValueError, match="sectors must be"):
            frc_sectors(img, img, sectors=bad)                  # before any device work: this machine may have none
        with pytest.raises(ValueError, match="sectors must be"):
            decorr_sectors(img, sectors=bad)
        with pytest.raises(ValueError, match="sectors must be"):
            ops.frc_sector_bounds(bad)
        with pytest.raises(ValueError, match="sectors must be"):
            ops.frc_sector_pop(16, bad)
    for bad in (14, 17, 1026, True):
        with pytest.raises(ValueError, match="block must be"):
            ops.frc_sector_pop(bad, 2)
    # the checks of frc and decorr, under the new names
    with pytest.raises(ValueError, match="window"):
        frc_sectors(img, img, window="hamming")
    with pytest.raises(ValueError, match="threshold"):
        frc_sectors(img, img, threshold=1.5)
    with pytest.raises(ValueError, match="smooth"):
        frc_sectors(img, img, smooth=-1)
    with pytest.raises(ValueError, match="pixel_size"):
        decorr_sectors(img, pixel_size=0)
    with pytest.raises(ValueError, match="filters"):
        decorr_sectors(img, filters=65)
    with pytest.raises(ValueError, match="pool"):
        decorr_sectors(img, pool="plane")
    with pytest.raises(TypeError, match="frc_sectors takes uint8 images; b is"):
        frc_sectors(img, img.astype(np.float32))
    with pytest.raises(TypeError, match="decorr_sectors takes uint8"):
        decorr_sectors(img.astype(np.int16))
    with pytest.raises(ValueError, match="same shape"):
        frc_sectors(img, img[:, :16])
    with pytest.raises(ValueError, match="at least one plane"):
        decorr_sectors(img[:8, :8])
    with pytest.raises(ValueError, match="block must be"):
        frc_sectors(img, img, block=34)
    import torch
    with pytest.raises(RuntimeError, match="frc_sectors runs on an MI355X"):
        frc_sectors(torch.zeros(32, 32, dtype=torch.uint8), torch.zeros(32, 32, dtype=torch.uint8))
    with pytest.raises(RuntimeError, match="decorr_sectors runs on an MI355X"):
        decorr_sectors(torch.zeros(32, 32, dtype=torch.uint8))
    for name in ("frc_x", "frc_y", "decorr_x", "decorr_y"):
        with pytest.raises(RuntimeError, match="MI355X"):
            test_metrics(None, None, device="cpu", metrics=("psnr", name))           # before model or dataset are touched


def test_entry_points_refuse_bad_arguments():
    """PSSR_ERR_ARG from the four entry points; nothing is launched, so no device is needed."""
    from pssr2_amd import _lib
    lib = _lib.lib()
    assert lib.pssr_abi_version() == 5
    buf = ctypes.create_string_buffer(64)
    p = ctypes.c_void_p(ctypes.addressof(buf))
    for ws_bytes in (lib.pssr_frc_sectors_workspace_bytes, lib.pssr_decorr_sectors_workspace_bytes):
        assert ws_bytes(1, 64, 64, 64, 0) == 0 and ws_bytes(1, 64, 64, 64, 17) == 0 and ws_bytes(1, 64, 64, 63, 2) == 0
        assert ws_bytes(1, 64, 64, 128, 2) == 0 and ws_bytes(0, 64, 64, 64, 2) == 0
        sizes = [ws_bytes(3, 64, 64, 64, S) for S in (1, 2, 16)]
        assert 0 < sizes[0] < sizes[1] < sizes[2]
        # S times the partial rows: the chunk of blocks shrinks and stays inside 256 MB (plus a block)
        assert ws_bytes(200, 512, 512, 512, 16) <= (256 << 20) and ws_bytes(200, 512, 512, 512, 16) < 200 * ws_bytes(1, 512, 512, 512, 16)
    assert lib.pssr_frc_sectors_workspace_bytes(3, 64, 64, 64, 1) == lib.pssr_frc_workspace_bytes(3, 64, 64, 64)
    assert lib.pssr_decorr_sectors_workspace_bytes(3, 64, 64, 64, 1) == lib.pssr_decorr_workspace_bytes(3, 64, 64, 64)
    big = 1 << 40

    def frc_call(bx=p, by=p, n=64, S=2, ws=big, a=p):
        return lib.pssr_frc_sectors_u8(a, p, p, p, bx, by, p, 1, 64, 64, n, S, p, ws, None)

    def decorr_call(bx=p, by=p, n=64, S=2, ws=big, a=p):
        return lib.pssr_decorr_sectors_u8(a, p, p, bx, by, p, 1, 64, 64, n, S, p, ws, None)

    for call in (frc_call, decorr_call):
        for S in (0, -1, 17):
            assert call(S=S) == -1 and b"sector count" in lib.pssr_last_error()
        assert call(bx=None) == -1 and b"boundary" in lib.pssr_last_error()
        assert call(by=None) == -1 and b"boundary" in lib.pssr_last_error()
        assert call(a=None) == -1 and b"null pointer" in lib.pssr_last_error()
        assert call(n=62 + 1) == -1 and b"even" in lib.pssr_last_error()
        assert call(n=128) == -1 and b"does not fit" in lib.pssr_last_error()
        assert call(ws=1024) == -1 and b"short" in lib.pssr_last_error()


# ------------------------------------------------------------------------------------------------ recovery, by the restatement alone
@pytest.mark.parametrize("n,rx,ry", Q.ANISO)
def test_the_restatement_recovers_a_planted_anisotropy(n, rx, ry):
    """Measured: r*_x 21.6 - 21.9, 41.7 - 41.9, 61.2 - 61.7; r*_y 11.4 - 11.7, 21.7 - 24.6, 33.8 - 34.2; the smallest ratio is 1.70."""
    for seed in range(3):
        a, b = Q.planted_aniso(n, rx, ry, seed)
        two, four = Q.sectors_ref(a[None], b[None], n, 2), Q.sectors_ref(a[None], b[None], n, 4)
        x, y = (Q.curve_ref(two[..., s, :], Q.pop(n, 2)[:, s], n)[1] for s in range(2))
        print(f"n={n} seed {seed}: r*_x = {x:.2f}, r*_y = {y:.2f}, ratio {x / y:.2f}")
        assert rx <= x <= rx + 4 and x / y >= 1.5
        r4 = [Q.curve_ref(four[..., s, :], Q.pop(n, 4)[:, s], n)[1] for s in range(4)]
        assert r4[2] < r4[1] and r4[2] < r4[3]                  # the 90 degree sector crosses below both 45 degree sectors


def test_the_restatement_orders_the_decorrelation_peaks_of_an_anisotropic_blur():
    """blurred_aniso(128, 1.0, 3.0, 3): peak_x = 49.15, peak_y = 19.24 rings."""
    n = Q.DECORR_SCENE[0]
    cells = Q.decorr_sectors_ref(Q.blurred_aniso(*Q.DECORR_SCENE)[None], n, 2)
    x, y = (Q.decorr_resolve_ref(cells[..., s, :], Q.pop(n, 2)[:, s], n) for s in range(2))
    print(f"peak_x = {x['peak']:.2f}, peak_y = {y['peak']:.2f}")
    assert x["found"] and y["found"] and x["peak"] > 1.5 * y["peak"]
