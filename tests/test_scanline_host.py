"""Scan phase without a device: the restatement of tests/_scanline_ref.py against scalar loops, the choice and the sub-pixel step on
hand-built sums, the recovery of a planted phase by the restatement alone, the Python checks of the entry points of pssr2_amd.util, the
argument checks of the C ABI (nothing is launched), and ScanPhase.crappify against the restatement under a seeded global stream."""
import ctypes
from pathlib import Path

import numpy as np
import pytest
import torch

import _scanline_ref as S

ROOT = Path(__file__).resolve().parent.parent
PHASES = (0, 1, -1, 2, -3, 0.5, 1.30, -2.25, 0.25, -0.156, 2.73)


# ------------------------------------------------------------------------------------------------ the restatement against scalar loops
@pytest.mark.parametrize("H, W, R", [(3, 1, 0)] + [(H, W, R) for H, W in ((3, 7), (4, 9), (5, 13)) for R in (0, 1, 3)])
def test_row_sums_ref_against_scalar_loops(H, W, R):
    T = 2 * R + 1
    x = np.random.default_rng(H * 100 + W).integers(0, 256, size=(2, H, W), dtype=np.uint8)
    got = S.row_sums_ref(x, R)
    assert got.shape == (2, H - 2, 3 * T + 2) and got.dtype == np.int64
    for pl in range(2):
        for y in range(1, H - 1):
            want = [0] * (3 * T + 2)
            for c in range(R, W - R):
                e = int(x[pl, y - 1, c]) + int(x[pl, y + 1, c])
                for k in range(-R, R + 1):
                    o = int(x[pl, y, c + k])
                    want[3 * (k + R)] += o
                    want[3 * (k + R) + 1] += o * o
                    want[3 * (k + R) + 2] += o * e
                want[3 * T] += e
                want[3 * T + 1] += e * e
            assert got[pl, y - 1].tolist() == want


@pytest.mark.parametrize("k", range(-3, 4))
def test_shift_rows_ref_integer_shift_is_slicing_with_edge_replication(k):
    x = np.random.default_rng(5).integers(0, 256, size=(2, 4, 9), dtype=np.uint8)
    want = x[..., np.clip(np.arange(9) - k, 0, 8)]
    assert np.array_equal(S.shift_rows_ref(x, np.full((2, 4), 256 * k)), want)
    out, fragile = S.shift_rows_ref(x.astype(np.float32), np.full((2, 4), 256 * k))
    assert np.array_equal(out, want.astype(np.float32)) and not fragile.any()


def test_shift_rows_ref_half_pixel_rounds_up():
    x = np.array([[0, 255]], dtype=np.uint8)
    assert S.shift_rows_ref(x, [128]).tolist() == [[0, 128]]                    # (128 * 0 + 128 * 255 + 128) >> 8
    assert S.shift_rows_ref(x, [-128]).tolist() == [[128, 255]]
    out, _ = S.shift_rows_ref(x.astype(np.float32), [-128], gain=1.0)
    assert out.tolist() == [[128.5, 256.0]]
    out, _ = S.shift_rows_ref(x.astype(np.float32), [-128], gain=1.0, flags=2)
    assert out.tolist() == [[128.0, 255.0]]                                     # half to even, then the clip


def _sums(T, triples, sl, sll):
    out = []
    for tr in triples:
        out += list(tr)
    assert len(triples) == T
    return out + [sl, sll]


def test_tie_goes_to_the_smaller_magnitude_then_the_smaller_shift():
    # n = 4, L = (0, 0, 2, 2): sl = 4, sll = 8.  D equal to L (sd 4, sdd 8, sdl 8) scores 1 at every k that has it
    hit, miss = (4, 8, 8), (4, 8, 4)
    assert S.scan_choose_ref(4, _sums(5, [hit, miss, miss, miss, hit], 4, 8), 2)[0] == -2        # |k| equal: the smaller k
    assert S.scan_choose_ref(4, _sums(5, [hit, miss, miss, hit, miss], 4, 8), 2)[0] == 1         # the smaller |k|
    assert S.scan_choose_ref(4, _sums(5, [hit, hit, hit, hit, hit], 4, 8), 2)[:2] == (0, 0.0)
    from pssr2_amd import util
    for triples in ([hit, miss, miss, miss, hit], [hit, miss, miss, hit, miss], [hit] * 5):
        sums = _sums(5, triples, 4, 8)
        assert util._scan_choose(4, sums, 2) == S.scan_choose_ref(4, sums, 2)


def test_constant_image_gives_phase_zero_and_score_zero():
    x = np.full((1, 6, 12), 77, dtype=np.uint8)
    k, phase, score, curve = S.estimate_ref(x, 3)
    assert (k, phase, score) == (0, 0.0, 0.0) and not any(curve)


def _curve_sums(rs, n=1000):
    """Sums whose correlations are about `rs`: L and D_k unit-variance-like integers built from sd = sl = 0."""
    scale = 10 ** 6
    return _sums(len(rs), [(0, scale, int(round(r * scale))) for r in rs], 0, scale), n


def test_subpixel_step_is_clipped_and_zero_on_the_window_edge():
    from pssr2_amd import util
    sums, n = _curve_sums([0.1, 0.5, 0.9, 0.8999, 0.2])          # peak at k = 0 (index 2) with a shoulder on the right
    for choose in (S.scan_choose_ref, util._scan_choose):
        k, phase, score, curve = choose(n, sums, 2)
        assert k == 0 and 0.0 < phase - k <= 0.5 and score == curve[2]
        rm, r0, rp = curve[1:4]
        assert phase == min(max(0.5 * (rm - rp) / (rm - 2 * r0 + rp), -0.5), 0.5)
    sums, n = _curve_sums([0.1, 0.2, 0.5, 0.5, 0.9])             # the best on the edge: no step
    for choose in (S.scan_choose_ref, util._scan_choose):
        assert choose(n, sums, 2)[:2] == (2, 2.0)
    sums, n = _curve_sums([0.0, 0.9, 0.9, 0.0, 0.0])             # two equal neighbours: the tie goes to k = 0, delta = -0.5 exactly
    for choose in (S.scan_choose_ref, util._scan_choose):
        assert choose(n, sums, 2)[:2] == (0, -0.5)
    sums, n = _curve_sums([0.5, 0.2, 0.3, 0.25, 0.5])            # both edges tie: the smaller k, and no step on the edge
    for choose in (S.scan_choose_ref, util._scan_choose):
        k, phase = choose(n, sums, 2)[:2]
        assert k == -2 and phase == -2.0


# ------------------------------------------------------------------------------------------------ recovery by the restatement alone
@pytest.mark.parametrize("res", [64, 128])
def test_planted_phase_is_recovered_by_the_restatement(res):
    """The integer k equals round(phi) for every integer phi, and |phase - phi| <= 0.1 px.  Measured with this restatement, worst case over
    the four tiles and the eleven phases: 0.025 px at res = 64, 0.026 px at res = 128."""
    from pssr2_amd.data import synthetic_em_tile
    worst = 0.0
    for i in range(4):
        tile = synthetic_em_tile(i, res)
        for phi in PHASES:
            k, phase, score, _ = S.estimate_ref(S.plant_ref(tile, phi), 8)
            if float(phi).is_integer():
                assert k == round(phi), (i, phi, k)
            worst = max(worst, abs(phase - phi))
            assert abs(phase - phi) <= 0.1, (i, phi, phase)
    print(f"res={res}: worst |phase - phi| = {worst:.4f} px")


def test_correction_undoes_an_integer_plant():
    x = np.random.default_rng(9).integers(0, 256, size=(1, 8, 20), dtype=np.uint8)
    for k in (-3, -1, 0, 2):
        back = S.correct_ref(S.plant_ref(x, k), k)
        a = abs(k)
        assert np.array_equal(back[..., a:20 - a], x[..., a:20 - a])


# ------------------------------------------------------------------------------------------------ the Python checks
def test_python_checks_come_before_any_device_work():
    from pssr2_amd import util
    img = np.zeros((2, 1, 16, 32), dtype=np.uint8)
    for fn in (util.estimate_scan_phase, util.correct_scan_phase):
        for bad in (-1, 17, 1.5, True, None):
            with pytest.raises(ValueError, match="radius"):
                fn(img, radius=bad)
        with pytest.raises(ValueError, match="pool"):
            fn(img, pool="batch")
        with pytest.raises(RuntimeError, match="MI355X"):
            fn(torch.zeros(2, 1, 16, 32, dtype=torch.uint8))
        with pytest.raises(TypeError, match="uint8"):
            fn(img.astype(np.float32))
        for shape in ((16, 32), (1, 2, 1, 16, 32), (2, 1, 2, 32), (0, 1, 16, 32)):
            with pytest.raises(ValueError, match="lr"):
                fn(np.zeros(shape, dtype=np.uint8))
    with pytest.raises(ValueError, match="columns"):
        util.estimate_scan_phase(np.zeros((1, 1, 16, 16), dtype=np.uint8), radius=8)
    for bad in (float("nan"), 65.0, [0.5, 0.5], np.zeros((2, 2))):
        with pytest.raises(ValueError, match="phase"):
            util.correct_scan_phase(img, bad, pool="all")
    with pytest.raises(ValueError, match="phase"):
        util.correct_scan_phase(img, [0.5, 0.5, 0.5], pool="item")
    with pytest.raises(ValueError, match="phase"):
        util.correct_scan_phase(img, np.zeros(2), pool="plane")


def test_scan_phase_fit_builds_a_crappifier():
    from pssr2_amd import util
    from pssr2_amd.crappifiers import ScanPhase
    fit = util.ScanPhaseFit(1.25, 1, 0.9, np.zeros(17), 8)
    cr = fit.crappifier(spread=0.1, jitter=0.05)
    assert isinstance(cr, ScanPhase) and cr.device_spec() == ("scanphase", 1.25, 0.0, 0.1, 0.05)
    assert util.ScanPhaseFit(np.array([1.0, 2.0]), None, None, None, 8).crappifier().intensity == 1.5
    with pytest.raises(ValueError):
        ScanPhase(1.0, jitter=-1.0)
    with pytest.raises(TypeError):
        ScanPhase(1.0, 0, 0, 0.5)            # jitter is keyword-only


# ------------------------------------------------------------------------------------------------ argument checks of the entry points
def _lib():
    path = ROOT / "pssr2_amd" / "libpssr_mi355.so"
    if not path.exists():
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(str(path))
    lib.pssr_last_error.restype = ctypes.c_char_p
    return lib


def test_scanline_entry_points_validate_without_gpu():
    """PSSR_ERR_ARG from the four entry points; nothing is launched, so no device is needed."""
    lib = _lib()
    i, p, f, u64 = ctypes.c_int, ctypes.c_void_p, ctypes.c_float, ctypes.c_uint64
    moments, su8, sf32, table = lib.pssr_line_moments_u8, lib.pssr_shift_rows_u8, lib.pssr_shift_rows_f32, lib.pssr_scan_rows_table
    moments.argtypes = [p] * 2 + [i] * 4 + [p]
    su8.argtypes = [p] * 3 + [i] * 3 + [p]
    sf32.argtypes = [p] * 3 + [i] * 3 + [f, i, p]
    table.argtypes = [p] + [i] * 3 + [f] * 3 + [u64] * 2 + [p] * 2
    fake, other = 0x1000, 0x2000          # never dereferenced: every call below fails its checks

    def err(status, word):
        return status == -1 and word in lib.pssr_last_error()

    # x, sums, planes, H, W, radius
    assert err(moments(None, fake, 1, 8, 8, 1, None), b"null") and err(moments(fake, None, 1, 8, 8, 1, None), b"null")
    for bad in ((0, 8, 8), (-1, 8, 8), (1, 0, 8), (1, 8, -2)):
        assert err(moments(fake, fake, *bad, 1, None), b"positive")
    for bad in (-1, 17, 100):
        assert err(moments(fake, fake, 1, 8, 64, bad, None), b"radius")
    for bad in (1, 2):
        assert err(moments(fake, fake, 1, bad, 64, 1, None), b"rows")
    assert err(moments(fake, fake, 1, 8, 32, 16, None), b"shorter") and err(moments(fake, fake, 1, 8, 2, 1, None), b"shorter")
    assert err(moments(fake, fake, 1, 16385, 16384, 0, None), b"2^28")
    # in, out, table, planes, H, W (, gain, flags)
    for fn, tail in ((su8, ()), (sf32, (0.0, 0))):
        for hole in range(3):
            ptrs = [None if k == hole else (fake, other, fake)[k] for k in range(3)]
            assert err(fn(*ptrs, 1, 8, 8, *tail, None), b"null")
        assert err(fn(fake, fake, fake, 1, 8, 8, *tail, None), b"in place")
        for bad in ((0, 8, 8), (1, 0, 8), (1, 8, 0), (-3, 8, 8)):
            assert err(fn(fake, other, fake, *bad, *tail, None), b"positive")
        assert err(fn(fake, other, fake, 1, 16385, 16384, *tail, None), b"2^28")
    for bad in (-1, 4):
        assert err(sf32(fake, other, fake, 1, 8, 8, 0.0, bad, None), b"flags")
    # table, tiles, frames, h, intensity, spread, jitter, seed, tile_offset, tile_counter
    assert err(table(None, 1, 1, 8, 1.0, 0.0, 0.0, 0, 0, None, None), b"null")
    for bad in ((0, 1, 8), (1, 0, 8), (1, 1, 0), (1, -1, 8)):
        assert err(table(fake, *bad, 1.0, 0.0, 0.0, 0, 0, None, None), b"positive")
    assert err(table(fake, 1, 1, 8, 1.0, -0.5, 0.0, 0, 0, None, None), b"negative")
    assert err(table(fake, 1, 1, 8, 1.0, 0.0, -0.5, 0, 0, None, None), b"negative")


# ------------------------------------------------------------------------------------------------ the host crappifier
@pytest.mark.parametrize("spread, jitter", [(0, 0.0), (0.5, 0.0), (0, 0.3), (0.5, 0.3)])
def test_scanphase_crappify_equals_the_restatement_of_the_same_draws(spread, jitter):
    from pssr2_amd.crappifiers import MultiCrappifier, ScanPhase
    img = np.random.default_rng(3).integers(0, 256, size=(2, 9, 21), dtype=np.uint8)
    np.random.seed(11)
    got = ScanPhase(-1.5, gain=2, spread=spread, jitter=jitter).crappify(img)
    np.random.seed(11)
    phase = np.random.normal(-1.5, spread) if spread > 0 else -1.5
    j = np.random.normal(0, jitter, (2, 9)) if jitter > 0 else np.zeros((2, 9))
    d = np.clip(np.rint(256.0 * (phase * (np.arange(9) & 1) + j)), -S.MAX_D, S.MAX_D).astype(np.int64)
    want, _ = S.shift_rows_ref(img.astype(np.float32), d, gain=2.0)
    assert got.shape == img.shape and np.array_equal(got.astype(np.float32), want)
    if not jitter:
        assert np.array_equal(got[:, 0::2], img[:, 0::2] + 2.0)                  # even rows only get the gain
    fed = ScanPhase(9.0).crappify(img, table=d)                                  # a table in place of the draws
    assert np.array_equal(fed.astype(np.float32), S.shift_rows_ref(img.astype(np.float32), d)[0])
    multi = MultiCrappifier(ScanPhase(1.0), ScanPhase(-1.0))
    assert np.array_equal(multi.crappify(img)[..., 1:-1], img[..., 1:-1])


def test_scan_table_ref_has_few_fragile_rows():
    """The restatement alone: 0 - 2 fragile rows among the 4 x 1 x 64 rows that tests/test_gpu_scanline.py uses."""
    for spread, jitter in ((0.0, 0.0), (0.25, 0.0), (0.0, 0.25), (0.25, 0.25)):
        for off in (0, 1 << 40):
            d, fragile = S.scan_table_ref(4, 1, 64, 1.5, spread, jitter, 1234, off)
            assert d.shape == (4, 1, 64) and int(fragile.sum()) <= 2
            if not jitter:
                assert not d[:, :, 0::2].any() and (d[:, :, 1::2] == d[:, :, 1:2]).all()
            if not spread and not jitter:
                assert (d[:, :, 1::2] == 384).all()
