"""Directional resolution on the device (the sectorial column pass of csrc/frc.hip through ops.frc_sectors_u8 / decorr_sectors_u8,
util.frc_sectors / decorr_sectors and test_metrics) against the numpy restatement of tests/_sector_ref.py.  The bound on a cell's sums is
|S - S_ref| <= tol(n) sqrt(Saa_ref Sbb_ref) of the whole ring, tol(n) = 8 x the error of the float32 numpy restatement on the same inputs
(measured on the CPU, recorded in _sector_ref.py); sectors = 1 and the sum over the sectors are pinned to the unsectored kernels."""
import functools
import math

import numpy as np
import pytest
import torch

import _decorr_ref as D
import _frc_ref as F
import _sector_ref as Q

pytestmark = pytest.mark.gpu


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _frc_cells(a, b, n, S, name="hann"):
    from pssr2_amd import ops
    got = ops.frc_sectors_u8(_dev(a), _dev(b), n, S, name)
    assert got.dtype == torch.float64 and got.is_cuda
    return got.cpu().numpy()


def _decorr_cells(a, n, S, name="hann"):
    from pssr2_amd import ops
    got = ops.decorr_sectors_u8(_dev(a), n, S, name)
    assert got.dtype == torch.float64 and got.is_cuda
    return got.cpu().numpy()


@functools.lru_cache(maxsize=None)
def _case(n):
    """[(a, b, window, {S: sectors_ref}, {S: decorr_sectors_ref})] of the accuracy tests at block side n, computed once."""
    return [(a, b, name, {S: Q.sectors_ref(a, b, n, S, name) for S in Q.sectors_of(n)}, {S: Q.decorr_sectors_ref(a, n, S, name) for S in Q.sectors_of(n)})
            for a, b, name in Q.sums_inputs(n)]


# ------------------------------------------------------------------------------------------------ pinned to the unsectored kernels
@pytest.mark.parametrize("n", F.SUMS_SIZES)
def test_one_sector_is_the_unsectored_call_bit_for_bit(n):
    from pssr2_amd import ops
    for a, b, name in F.sums_inputs(n):
        a, b = _dev(a), _dev(b)
        got = ops.frc_sectors_u8(a, b, n, 1, name)
        assert got.shape == (1, 1, n // 2 + 1, 1, 3) and torch.equal(got[..., 0, :], ops.frc_rings_u8(a, b, n, name))
        got = ops.decorr_sectors_u8(a, n, 1, name)
        assert got.shape == (1, 1, n // 2 + 1, 1, 2) and torch.equal(got[..., 0, :], ops.decorr_rings_u8(a, n, name))


@pytest.mark.parametrize("n", (18, 66))
def test_two_calls_give_the_same_bits_for_every_sector_count(n):
    from pssr2_amd import ops
    a, b, name = F.sums_inputs(n)[1]
    a, b = _dev(np.tile(a, (3, 2, 2))), _dev(np.tile(b, (3, 2, 2)))
    for S in range(1, Q.MAX_SECTORS + 1):
        first, dfirst = ops.frc_sectors_u8(a, b, n, S, name), ops.decorr_sectors_u8(a, n, S, name)
        assert first.shape == (3, 4, n // 2 + 1, S, 3) and dfirst.shape == (3, 4, n // 2 + 1, S, 2)
        for _ in range(2):
            assert torch.equal(ops.frc_sectors_u8(a, b, n, S, name), first) and torch.equal(ops.decorr_sectors_u8(a, n, S, name), dfirst)


@pytest.mark.parametrize("n", (16, 34, 66, 130))
def test_the_sectors_add_up_to_the_device_ring_sums(n):
    """Regrouping a ring's fewer than 3300 terms: 1e-12 sqrt(Saa Sbb) (tests/test_sector_host.py derives it); for the two sums of
    decorrelation analysis sum |F| <= sqrt(pop P), so 1e-12 sqrt(pop P) and 1e-12 P."""
    from pssr2_amd import ops
    for a, b, name in Q.sums_inputs(n):
        whole = ops.frc_rings_u8(_dev(a), _dev(b), n, name).cpu().numpy()
        dwhole = ops.decorr_rings_u8(_dev(a), n, name).cpu().numpy()
        for S in Q.SUMS_SECTORS:
            got = _frc_cells(a, b, n, S, name).sum(axis=-2)
            assert (np.abs(got - whole) <= 1e-12 * F.scale_of(whole)[..., None]).all()
            dgot = _decorr_cells(a, n, S, name).sum(axis=-2)
            assert (np.abs(dgot[..., 0] - dwhole[..., 0]) <= 1e-12 * np.sqrt(D.pop(n) * dwhole[..., 1])).all()
            assert (np.abs(dgot[..., 1] - dwhole[..., 1]) <= 1e-12 * dwhole[..., 1]).all()


# ------------------------------------------------------------------------------------------------ accuracy
@pytest.mark.parametrize("n", Q.SUMS_SIZES + tuple(m for m, _ in Q.BIG))
def test_cell_sums_against_the_float64_fft(n):
    """The sizes of tests/test_gpu_frc.py (16 the minimum; 18, 30, 34 no multiples of a tile; 64, 66 one tile and just over; 130 several
    stages and tiles), S = 2, 3, 4, 8, 16, on white noise, an isotropic and an anisotropic planted pair, both windows; 500 at S = 2 and
    1024 at S = 4 once each.  Empty cells are exactly zero."""
    worst, worst_a, worst_p = 0.0, 0.0, 0.0
    for a, b, name, refs, drefs in _case(n):
        for S in Q.sectors_of(n):
            got = _frc_cells(a, b, n, S, name)
            assert got.shape == (1, 1, n // 2 + 1, S, 3) and not got[0, 0][Q.pop(n, S) == 0].any()
            worst = max(worst, Q.frc_error(got, refs[S]))
            dgot = _decorr_cells(a, n, S, name)
            assert dgot.shape == (1, 1, n // 2 + 1, S, 2) and not dgot[0, 0][Q.pop(n, S) == 0].any()
            ea, ep = Q.decorr_error(dgot, drefs[S], n)
            worst_a, worst_p = max(worst_a, ea), max(worst_p, ep)
    print(f"n={n}: FRC cells {worst:.3e}, bound {Q.tol(n):.3e} (float32 numpy {Q.F32_ERROR[n]:.3e}); decorrelation A {worst_a:.3e}, "
          f"P {worst_p:.3e}, bounds {Q.decorr_tol(n)[0]:.3e}, {Q.decorr_tol(n)[1]:.3e}")
    assert worst <= Q.tol(n)
    assert worst_a <= Q.decorr_tol(n)[0] and worst_p <= Q.decorr_tol(n)[1]


# ------------------------------------------------------------------------------------------------ geometry
@pytest.mark.parametrize("H,W,n,planes", [(40, 70, 16, 1), (40, 70, 16, 3), (37, 53, 18, 1), (37, 53, 18, 3)])
def test_blocks_of_the_centred_grid(H, W, n, planes):
    """The grids of tests/test_gpu_frc.py, the planes at every start address modulo 16 in turn, S = 3."""
    from pssr2_amd import ops
    rng = np.random.default_rng(H + planes)
    a, b = (rng.integers(0, 256, size=(planes, H, W), dtype=np.uint8) for _ in range(2))
    nby, nbx, _, _ = F.grid(H, W, n)
    ref, dref = Q.sectors_ref(a, b, n, 3), Q.decorr_sectors_ref(a, n, 3)
    assert ref.shape == (planes, nby * nbx, n // 2 + 1, 3, 3)
    first = dfirst = None
    for off in range(16):
        bufs = []
        for img in (a, b):
            flat = torch.zeros(off + img.size + 16, dtype=torch.uint8, device="cuda")
            flat[off:off + img.size] = _dev(img).reshape(-1)
            bufs.append(flat[off:off + img.size].view(planes, H, W))
        assert bufs[0].data_ptr() % 16 == off and bufs[0].is_contiguous()
        got, dgot = ops.frc_sectors_u8(bufs[0], bufs[1], n, 3).cpu().numpy(), ops.decorr_sectors_u8(bufs[0], n, 3).cpu().numpy()
        first, dfirst = (got, dgot) if first is None else (first, dfirst)
        np.testing.assert_array_equal(got, first)               # where the bytes lie changes nothing
        np.testing.assert_array_equal(dgot, dfirst)
    assert Q.frc_error(first, ref) <= Q.tol(n)
    ea, ep = Q.decorr_error(dfirst, dref, n)
    assert ea <= Q.decorr_tol(n)[0] and ep <= Q.decorr_tol(n)[1]


def test_non_contiguous_inputs_and_leading_dimensions():
    from pssr2_amd import ops
    rng = np.random.default_rng(12)
    wide = _dev(rng.integers(0, 256, size=(2, 3, 36, 80), dtype=np.uint8))
    a, b = wide[..., ::2], wide[..., 1::2]
    assert not a.is_contiguous() and not b.is_contiguous()
    got = ops.frc_sectors_u8(a, b, 18, 4)
    assert got.shape == (6, 4, 10, 4, 3)
    assert torch.equal(got, ops.frc_sectors_u8(a.contiguous().reshape(6, 36, 40), b.contiguous().reshape(6, 36, 40), 18, 4))
    assert Q.frc_error(got.cpu().numpy(), Q.sectors_ref(a.cpu().numpy().reshape(6, 36, 40), b.cpu().numpy().reshape(6, 36, 40), 18, 4)) <= Q.tol(18)
    dgot = ops.decorr_sectors_u8(a, 18, 4)
    assert dgot.shape == (6, 4, 10, 4, 2) and torch.equal(dgot, ops.decorr_sectors_u8(a.contiguous().reshape(6, 36, 40), 18, 4))


def test_more_planes_than_a_grid_axis_of_the_plane_kernels():
    """1100 planes of 16 x 16 at S = 16, every one with its own content."""
    rng = np.random.default_rng(11)
    a, b = (rng.integers(0, 256, size=(1100, 16, 16), dtype=np.uint8) for _ in range(2))
    got = _frc_cells(a, b, 16, 16)
    assert got.shape == (1100, 1, 9, 16, 3)
    assert Q.frc_error(got, Q.sectors_ref(a, b, 16, 16)) <= Q.tol(16)
    ea, ep = Q.decorr_error(_decorr_cells(a, 16, 16), Q.decorr_sectors_ref(a, 16, 16), 16)
    assert ea <= Q.decorr_tol(16)[0] and ep <= Q.decorr_tol(16)[1]


def test_a_call_that_works_its_blocks_off_in_chunks():
    """At n = 512 and S = 16 a block takes 6.05 MB of workspace (3.95 MB of partial rows, 16 times the unsectored call's): 44 blocks fit
    the 256 MB of a chunk, so 46 launch twice; with one image per block 3.68 MB, 72 fit, 74 launch twice.  Every block's sums are what a
    call of its own gives, bit for bit."""
    from pssr2_amd import _lib, ops
    gen = torch.Generator(device="cuda").manual_seed(5)
    a = torch.randint(0, 256, (74, 512, 512), dtype=torch.uint8, device="cuda", generator=gen)
    b = torch.randint(0, 256, (46, 512, 512), dtype=torch.uint8, device="cuda", generator=gen)
    lib = _lib.lib()
    assert lib.pssr_frc_sectors_workspace_bytes(46, 512, 512, 512, 16) < 46 * lib.pssr_frc_sectors_workspace_bytes(1, 512, 512, 512, 16)
    assert lib.pssr_frc_sectors_workspace_bytes(44, 512, 512, 512, 16) == 44 * lib.pssr_frc_sectors_workspace_bytes(1, 512, 512, 512, 16)
    assert lib.pssr_decorr_sectors_workspace_bytes(74, 512, 512, 512, 16) < 74 * lib.pssr_decorr_sectors_workspace_bytes(1, 512, 512, 512, 16)
    whole = ops.frc_sectors_u8(a[:46], b, 512, 16)
    assert whole.shape == (46, 1, 257, 16, 3)
    for lo, hi in ((0, 1), (43, 45), (45, 46)):
        assert torch.equal(whole[lo:hi], ops.frc_sectors_u8(a[lo:hi], b[lo:hi], 512, 16))
    whole = ops.decorr_sectors_u8(a, 512, 16)
    assert whole.shape == (74, 1, 257, 16, 2)
    for lo, hi in ((0, 1), (71, 73), (73, 74)):
        assert torch.equal(whole[lo:hi], ops.decorr_sectors_u8(a[lo:hi], 512, 16))


def test_an_all_zero_pair_is_exactly_zero():
    from pssr2_amd.util import decorr_sectors, frc_sectors
    z = np.zeros((2, 34, 50), dtype=np.uint8)
    for S in (1, 2, 5, 16):
        got = _frc_cells(z, z, 18, S, "none")
        assert got.shape == (2, 2, 10, S, 3) and not got.any() and not np.signbit(got).any()
        dgot = _decorr_cells(z, 18, S)
        assert dgot.shape == (2, 2, 10, S, 2) and not dgot.any() and not np.signbit(dgot).any()
    res = frc_sectors(z, z, block=18)
    assert res.curve.shape == (2, 10) and res.crossed.all() and (res.resolution == 18.0).all() and res.anisotropy == 1.0
    assert np.array_equal(res.curve[0], np.zeros(10)) and math.isnan(res.curve[1, 0]) and not res.curve[1, 1:].any()
    res = decorr_sectors(z, block=18, pixel_size=3.0)
    assert not res.found.any() and (res.resolution == 6.0).all() and np.isnan(res.peak).all() and not res.curves.any()


def test_arguments_are_checked_on_device_tensors_too():
    from pssr2_amd import _lib, ops
    t = torch.zeros(2, 32, 48, dtype=torch.uint8, device="cuda")
    for a, b in ((t, t[:1]), (t, t.float()), (t[0, 0], t[0, 0]), (t, t.cpu())):
        with pytest.raises(ValueError, match="frc_sectors_u8 needs two uint8 device tensors"):
            ops.frc_sectors_u8(a, b, 16, 2)
    for a in (t.float(), t[0, 0], t.cpu()):
        with pytest.raises(ValueError, match="decorr_sectors_u8 needs a uint8 device tensor"):
            ops.decorr_sectors_u8(a, 16, 2)
    for bad in (14, 17, 1026, 16.0, True):
        with pytest.raises(ValueError, match="block must be"):
            ops.frc_sectors_u8(t, t, bad, 2)
    for bad in (0, 17, 2.0, True):
        with pytest.raises(ValueError, match="sectors must be"):
            ops.frc_sectors_u8(t, t, 16, bad)
        with pytest.raises(ValueError, match="sectors must be"):
            ops.decorr_sectors_u8(t, 16, bad)
    with pytest.raises(ValueError, match="does not fit"):
        ops.decorr_sectors_u8(t, 34, 2)
    with pytest.raises(ValueError, match="window"):
        ops.frc_sectors_u8(t, t, 16, 2, "hamming")
    # the boundary vectors are cached per (S, device)
    ops.frc_sectors_u8(t, t, 16, 5)
    assert ops._frc_device_bounds(5, t.device) is ops._frc_device_bounds(5, t.device)
    np.testing.assert_array_equal(ops._frc_device_bounds(5, t.device)[0].cpu().numpy(), ops.frc_sector_bounds(5)[0])
    # a short workspace is refused before anything is launched
    lib = _lib.lib()
    ct, st = ops._frc_device_tables(16, "hann", t.device)
    bx, by = ops._frc_device_bounds(2, t.device)
    need = lib.pssr_frc_sectors_workspace_bytes(2, 32, 48, 16, 2)
    ws = torch.empty(need, dtype=torch.uint8, device="cuda")
    sums = torch.full((2, 6, 9, 2, 3), -1.0, dtype=torch.float64, device="cuda")
    p = _lib.ptr
    assert lib.pssr_frc_sectors_u8(p(t), p(t), p(ct), p(st), p(bx), p(by), p(sums), 2, 32, 48, 16, 2, p(ws), need - 1, _lib.stream_ptr()) == -1
    assert b"short" in lib.pssr_last_error()
    need = lib.pssr_decorr_sectors_workspace_bytes(2, 32, 48, 16, 2)
    assert lib.pssr_decorr_sectors_u8(p(t), p(ct), p(st), p(bx), p(by), p(sums), 2, 32, 48, 16, 2, p(ws), need - 1, _lib.stream_ptr()) == -1
    assert b"short" in lib.pssr_last_error()
    torch.cuda.synchronize()
    assert (sums == -1).all()


# ------------------------------------------------------------------------------------------------ util.frc_sectors
TOL_500 = max(Q.tol(n) for n in Q.F32_ERROR if n <= 500)       # every block side used below is at most 500


def _curve_bound(cells, s, n, smooth=0):
    """Each of a cell's three sums lies within TOL sqrt(Saa Sbb) of the whole ring, so the sector's Sab / sqrt(Saa Sbb) moves by about
    2 TOL times the ring's scale over the cell's own; pooling adds bounds and scales alike.  [R + 1], from the reference cells."""
    R = n // 2
    pooled = cells.reshape(-1, R + 1, cells.shape[-2], 3).sum(axis=0)
    ring, cell = F.scale_of(pooled.sum(axis=1)), pooled[:, s]
    out = np.zeros(R + 1)
    for r in range(R + 1):
        lo, hi = (r, r) if r == 0 else (max(1, r - smooth), min(R, r + smooth))
        own = math.sqrt(cell[lo:hi + 1, 1].sum() * cell[lo:hi + 1, 2].sum())
        out[r] = 2 * TOL_500 * ring[lo:hi + 1].sum() / own if own > 0 else math.inf
    return out


def _check_frc_item(got_curve, got_resolution, got_crossed, cells, n, S, **kw):
    """One item of a frc_sectors result against the restatement on the reference cells; -> the reference crossings."""
    stars = []
    for s in range(S):
        curve, r_star, _, crossed = Q.curve_ref(cells[..., s, :], Q.pop(n, S)[:, s], n, **kw)
        assert np.array_equal(np.isnan(got_curve[s]), np.isnan(curve)) and bool(got_crossed[s]) == crossed
        ok = ~np.isnan(curve)
        assert (np.abs(got_curve[s] - curve)[ok] <= _curve_bound(cells, s, n, kw.get("smooth", 0))[ok]).all()
        if crossed:
            assert abs(n / got_resolution[s] - r_star) <= 1e-3
        else:
            assert got_resolution[s] == 2.0
        stars.append(r_star)
    return stars


@pytest.mark.parametrize("n,rx,ry", Q.ANISO)
def test_frc_sectors_finds_the_planted_anisotropy(n, rx, ry):
    """|r*_device - r*_ref| <= 1e-3 rings per sector (the bound of tests/test_gpu_frc.py), flags equal, and the recovery inequalities of
    tests/test_sector_host.py on the device's own figures."""
    from pssr2_amd.util import SectorFRC, frc_sectors
    for seed in range(3):
        a, b = Q.planted_aniso(n, rx, ry, seed)
        two, four = Q.sectors_ref(a[None], b[None], n, 2), Q.sectors_ref(a[None], b[None], n, 4)
        got = frc_sectors(a, b)
        assert isinstance(got, SectorFRC) and got.block == n and got.curve.shape == (2, n // 2 + 1) and got.resolution.shape == (2,)
        assert got.crossed.dtype == bool and got.crossed.shape == (2,) and np.array_equal(got.angles, [0.0, 90.0])
        np.testing.assert_array_equal(got.freq, np.arange(n // 2 + 1) / n)
        _check_frc_item(got.curve, got.resolution, got.crossed, two, n, 2)
        x, y = n / got.resolution
        print(f"n={n} seed {seed}: r*_x = {x:.3f}, r*_y = {y:.3f}, anisotropy {got.anisotropy:.3f}")
        assert rx <= x <= rx + 4 and x / y >= 1.5
        assert isinstance(got.anisotropy, float) and got.anisotropy == pytest.approx(x / y, rel=1e-14)
        got4 = frc_sectors(a, b, sectors=4)
        _check_frc_item(got4.curve, got4.resolution, got4.crossed, four, n, 4)
        assert np.array_equal(got4.angles, [0.0, 45.0, 90.0, 135.0])
        assert got4.resolution[2] > got4.resolution[1] and got4.resolution[2] > got4.resolution[3]     # the 90 degree sector crosses lowest
    # device tensors, the curve left on the device, smooth, another threshold, the pixel size (the last seed's pair)
    for make in (lambda v: v, _dev):
        for to_numpy in (True, False):
            again = frc_sectors(make(a), make(b), to_numpy=to_numpy)
            curve = again.curve if to_numpy else again.curve.cpu().numpy()
            assert (isinstance(again.curve, np.ndarray) if to_numpy else again.curve.is_cuda)
            assert np.array_equal(curve, got.curve, equal_nan=True) and np.array_equal(again.resolution, got.resolution)      # NaN: sector 1's ring 0
    for kw in (dict(smooth=2), dict(threshold=0.5)):
        other = frc_sectors(a, b, **kw)
        _check_frc_item(other.curve, other.resolution, other.crossed, two, n, 2, **kw)
    scaled = frc_sectors(a, b, pixel_size=32.5)
    assert scaled.resolution == pytest.approx(32.5 * got.resolution, rel=1e-15) and np.array_equal(scaled.curve, got.curve, equal_nan=True)
    # one sector is frc
    from pssr2_amd.util import frc
    one, ring = frc_sectors(a, b, sectors=1), frc(a, b)
    assert np.array_equal(one.curve[0], ring.curve) and one.resolution[0] == ring.resolution and one.anisotropy == 1.0 and one.angles.tolist() == [0.0]


@pytest.mark.parametrize("c", (1, 3))
def test_frc_sectors_pools_planes_and_keeps_empty_cells_apart(c):
    """(N, C) = (2, 1) and (2, 3) at S = 2 and at S = 8, whose six empty cells are NaN in the curve and skipped by the search."""
    from pssr2_amd.util import frc_sectors
    n = 64
    pairs = [[Q.planted_aniso(n, rx, ry, 10 * i + j) for j in range(c)] for i, (rx, ry) in enumerate(((20, 8), (12, 24)))]
    a = np.stack([np.stack([p[0] for p in item]) for item in pairs])
    b = np.stack([np.stack([p[1] for p in item]) for item in pairs])
    assert a.shape == (2, c, n, n)
    for S in (2, 8):
        got = frc_sectors(a, b, sectors=S)
        assert got.curve.shape == (2, S, n // 2 + 1) and got.resolution.shape == got.crossed.shape == (2, S) and got.anisotropy.shape == (2,)
        assert np.array_equal(np.isnan(got.curve[0]), Q.pop(n, S).T == 0) and np.isnan(got.curve).sum() == 2 * ((Q.pop(n, S) == 0).sum())
        for i in range(2):
            _check_frc_item(got.curve[i], got.resolution[i], got.crossed[i], Q.sectors_ref(a[i], b[i], n, S), n, S)
        np.testing.assert_array_equal(got.anisotropy, got.resolution.max(axis=1) / got.resolution.min(axis=1))
        # sharper along x in the first item, along y in the second
        assert got.resolution[0, 0] < got.resolution[0, S // 2] and got.resolution[1, 0] > got.resolution[1, S // 2]
    smooth = frc_sectors(a, b, sectors=8, smooth=2)
    assert np.isnan(smooth.curve[:, 1:, 0]).all() and not np.isnan(smooth.curve[:, :, 1:]).any()        # pooled populations fill the cells
    for i in range(2):
        _check_frc_item(smooth.curve[i], smooth.resolution[i], smooth.crossed[i], Q.sectors_ref(a[i], b[i], n, 8), n, 8, smooth=2)
    one = frc_sectors(_dev(a[1]), _dev(b[1]))                   # a [C, H, W] pair is the item without the batch axis
    two = frc_sectors(a, b)
    assert np.array_equal(one.resolution, two.resolution[1]) and np.array_equal(one.curve, two.curve[1], equal_nan=True) and one.anisotropy == two.anisotropy[1]


# ------------------------------------------------------------------------------------------------ util.decorr_sectors
DECORR_TOL_500 = tuple(max(Q.decorr_tol(n)[k] for n in Q.DECORR_F32_ERROR if n <= 500) for k in range(2))


def _check_decorr_item(got, index, cells, n, S, filters=10):
    """One item (or block) of a decorr_sectors result against the restatement on the reference cells: flags equal, peaks within 1e-3
    rings (the bound of tests/test_gpu_decorr.py), and the unfiltered curve within the bound that follows from the cells': the numerator
    up to ring r moves by at most tol_A sqrt(M(r) sum P) of the whole rings and the sector's denominator is sqrt(M_s(r) sum P_s); the
    denominator itself moves by tol_P / 2 sum P / sum P_s of itself, and d <= 1.  -> the reference peaks."""
    pooled = cells.reshape(-1, n // 2 + 1, S, 2).sum(axis=0)
    peaks = []
    for s in range(S):
        want = Q.decorr_resolve_ref(cells[..., s, :], Q.pop(n, S)[:, s], n, filters)
        at = index + (s,)
        assert bool(got.found[at]) == want["found"]
        if want["found"]:
            assert abs(got.peak[at] - want["peak"]) <= 1e-3 and got.resolution[at] == pytest.approx(n / got.peak[at], rel=1e-15)
        else:
            assert math.isnan(got.peak[at]) and got.resolution[at] == 2.0
        share = pooled[1:, :, 1].sum() / pooled[1:, s, 1].sum()
        m_all, m_own = np.cumsum(D.pop(n)[1:]), np.cumsum(Q.pop(n, S)[1:, s])
        ok = m_own > 0
        bound = DECORR_TOL_500[0] * np.sqrt(m_all[ok] / m_own[ok] * share) + DECORR_TOL_500[1] / 2 * share
        assert (np.abs(got.curves[at][0, 1:] - want["curves"][0, 1:])[ok] <= bound).all()
        peaks.append(want["peak"])
    return peaks


def test_decorr_sectors_orders_the_peaks_of_an_anisotropic_blur():
    """blurred_aniso(128, 1.0, 3.0, 3), sharper along x: the restatement alone gives peak_x = 49.15 and peak_y = 19.24 rings
    (tests/test_sector_host.py); the device is held to the ordering and to the restatement."""
    from pssr2_amd.util import SectorDecorr, decorr, decorr_sectors
    n = Q.DECORR_SCENE[0]
    img = Q.blurred_aniso(*Q.DECORR_SCENE)
    cells = Q.decorr_sectors_ref(img[None], n, 2)
    for make in (lambda v: v, _dev):
        for to_numpy in (True, False):
            raw = decorr_sectors(make(img), to_numpy=to_numpy)
            assert isinstance(raw, SectorDecorr) and raw.block == n and (isinstance(raw.curves, np.ndarray) if to_numpy else raw.curves.is_cuda)
            got = raw if to_numpy else raw._replace(curves=raw.curves.cpu().numpy())
            assert got.resolution.shape == got.found.shape == got.peak.shape == got.amplitude.shape == (2,) and got.curves.shape == (2, 11, n // 2 + 1)
            assert np.array_equal(got.angles, [0.0, 90.0]) and isinstance(got.anisotropy, float)
            peaks = _check_decorr_item(got, (), cells, n, 2)
            print(f"peak_x = {got.peak[0]:.3f} (reference {peaks[0]:.3f}), peak_y = {got.peak[1]:.3f} (reference {peaks[1]:.3f})")
            assert got.found.all() and got.peak[0] > 1.5 * got.peak[1]
            assert got.anisotropy == pytest.approx(got.peak[0] / got.peak[1], rel=1e-14)
    np.testing.assert_allclose(decorr_sectors(img, pixel_size=2.5).freq, got.freq / 2.5, rtol=1e-15)
    assert decorr_sectors(img, pixel_size=2.5).resolution == pytest.approx(2.5 * got.resolution, rel=1e-15)
    # one sector is decorr; no filters: the unfiltered curve alone
    one, ring = decorr_sectors(img, sectors=1), decorr(img)
    assert one.resolution[0] == ring.resolution and np.array_equal(one.curves[0], ring.curves) and one.anisotropy == 1.0
    got0 = decorr_sectors(img, filters=0)
    assert got0.curves.shape == (2, 1, n // 2 + 1) and np.array_equal(got0.curves[:, 0], got.curves[:, 0])
    _check_decorr_item(got0, (), cells, n, 2, filters=0)


@pytest.mark.parametrize("c", (1, 3))
def test_decorr_sectors_on_the_planted_anisotropy_items_and_blocks(c):
    """(N, C) = (2, 1) and (2, 3) of planted_aniso images at S = 2 and S = 8 against the restatement, pooled per item; and pool="block" on a
    2 x 2 grid of 64-blocks, a directional local-resolution map."""
    from pssr2_amd.util import decorr_sectors
    n = 64
    a = np.stack([np.stack([Q.planted_aniso(n, rx, ry, 10 * i + j)[0] for j in range(c)]) for i, (rx, ry) in enumerate(((20, 8), (12, 24)))])
    for S in (2, 8):
        got = decorr_sectors(a, sectors=S)
        assert got.resolution.shape == got.found.shape == (2, S) and got.curves.shape == (2, S, 11, n // 2 + 1) and got.anisotropy.shape == (2,)
        for i in range(2):
            _check_decorr_item(got, (i,), Q.decorr_sectors_ref(a[i], n, S), n, S)
        np.testing.assert_array_equal(got.anisotropy, got.resolution.max(axis=-1) / got.resolution.min(axis=-1))
    grid = np.block([[a[0, 0], a[1, 0]], [a[1, 0], a[0, 0]]])
    got = decorr_sectors(grid, block=n, pool="block")
    assert got.resolution.shape == got.peak.shape == (2, 2, 2) and got.curves.shape == (2, 2, 2, 11, n // 2 + 1) and got.anisotropy.shape == (2, 2)
    cells = Q.decorr_sectors_ref(grid[None], n, 2)
    for i in range(2):
        for j in range(2):
            _check_decorr_item(got, (i, j), cells[0, 2 * i + j], n, 2)
    assert np.array_equal(got.resolution[0, 0], got.resolution[1, 1]) and np.array_equal(got.resolution[0, 1], got.resolution[1, 0])
    batch = decorr_sectors(np.stack([grid, grid[::-1].copy()])[:, None], block=n, pool="block")
    assert batch.resolution.shape == (2, 2, 2, 2) and np.array_equal(batch.resolution[0], got.resolution) and batch.anisotropy.shape == (2, 2, 2)
    pooled = decorr_sectors(_dev(grid), block=n)
    assert pooled.resolution.shape == (2,) and pooled.curves.shape == (2, 11, n // 2 + 1)
    _check_decorr_item(pooled, (), cells, n, 2)


# ------------------------------------------------------------------------------------------------ test_metrics
class _Positional(torch.nn.Module):
    """0.5 x + 3.25 enlarged 2 x 2, plus 3 col - 2 row of the output coordinate: every ensemble member predicts something else."""

    def forward(self, x):
        y = (0.5 * x[:, x.shape[1] // 2:x.shape[1] // 2 + 1] + 3.25).repeat_interleave(2, dim=-2).repeat_interleave(2, dim=-1)
        i = torch.arange(y.shape[-1], dtype=y.dtype, device=y.device)
        j = torch.arange(y.shape[-2], dtype=y.dtype, device=y.device)
        return y + 3 * i.view(1, 1, 1, -1) - 2 * j.view(1, 1, -1, 1)


class _Pairs(torch.utils.data.Dataset):
    """A paired dataset in memory: LR [1, 32, 32] random, HR [1, 64, 64] its enlargement plus noise, handed over as float32."""
    is_lr, extra_hr_files, lr_scale = False, None, 2

    def __init__(self, n=2, crop_res=48):
        rng = np.random.default_rng(14)
        self.lrs = rng.integers(0, 128, size=(n, 1, 32, 32), dtype=np.uint8)
        self.hrs = (self.lrs.repeat(2, axis=-2).repeat(2, axis=-1) + rng.integers(0, 64, size=(n, 1, 64, 64))).astype(np.uint8)
        self.val_idx, self.crop_res = list(range(n)), crop_res

    def __len__(self):
        return len(self.lrs)

    def _get_name(self, i):
        return f"img{i}"

    def __getitem__(self, i):
        return torch.tensor(self.hrs[i]).float(), torch.tensor(self.lrs[i]).float()


NAMES = ("frc_x", "frc_y", "decorr_x", "decorr_y")


@pytest.mark.parametrize("norm", [False, True])
def test_test_metrics_directional_names(norm, monkeypatch):
    from pssr2_amd import ops
    from pssr2_amd.predict import predict_images, test_metrics
    from pssr2_amd.util import decorr_sectors, frc_sectors
    ds = _Pairs()
    before = test_metrics(_Positional(), ds, device="cuda", metrics=("psnr", "frc"), norm=norm, avg=False)
    got = test_metrics(_Positional(), ds, device="cuda", metrics=("psnr", "frc") + NAMES, norm=norm, avg=False)
    pred = predict_images(_Positional(), ds, device="cuda", batch_size=1, out_dir=None)["img0"]
    f, d = frc_sectors(pred, ds.hrs[0][:, :48, :48]), decorr_sectors(pred)
    assert f.block == d.block == 48 and np.isfinite(f.resolution).all() and (f.resolution >= 2.0).all() and (d.resolution >= 2.0).all()
    want = {"frc_x": f.resolution[0], "frc_y": f.resolution[1], "decorr_x": d.resolution[0], "decorr_y": d.resolution[1]}
    assert got == dict(before, **{k: [v] * 2 for k, v in want.items()})             # every iteration: dataset[0]; before norm
    assert test_metrics(_Positional(), ds, device="cuda", metrics="frc_y", norm=norm) == {"frc_y": want["frc_y"]}
    assert test_metrics(_Positional(), ds, device="cuda", metrics=("decorr_x",), norm=norm) == {"decorr_x": want["decorr_x"]}
    got8 = test_metrics(_Positional(), ds, device="cuda", metrics=NAMES, norm=norm, avg=False, ensemble=8)
    pred8 = predict_images(_Positional(), ds, device="cuda", batch_size=1, out_dir=None, ensemble=8)["img0"]
    f8, d8 = frc_sectors(pred8, ds.hrs[0][:, :48, :48]), decorr_sectors(pred8)
    assert got8 == {"frc_x": [f8.resolution[0]] * 2, "frc_y": [f8.resolution[1]] * 2, "decorr_x": [d8.resolution[0]] * 2, "decorr_y": [d8.resolution[1]] * 2}
    # one sums call per method and item however many names are given, none where none is
    calls = []
    for name in ("frc_sectors_u8", "decorr_sectors_u8"):
        monkeypatch.setattr(ops, name, lambda *args, _f=getattr(ops, name), _n=name: (calls.append(_n), _f(*args))[1])
    test_metrics(_Positional(), ds, device="cuda", metrics=NAMES, norm=norm)
    assert sorted(calls) == ["decorr_sectors_u8"] * 2 + ["frc_sectors_u8"] * 2
    del calls[:]
    assert test_metrics(_Positional(), ds, device="cuda", metrics=("psnr", "frc"), norm=norm, avg=False) == before and not calls
