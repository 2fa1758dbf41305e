"""The scan-phase kernels (csrc/scanline.hip, the ScanPhase kernels of csrc/crappify.hip) and their drivers against the restatement of
tests/_scanline_ref.py.  Everything is compared for equality: the sums, the resampled bytes and the estimate are integers or come from
the device's own integers; the float32 resampling and the row table are float64 arithmetic, equal outside the restatement's fragile mask
(an element within a relative 1e-9 of a rounding decision, where a contracted multiply-add may decide the other way)."""
import re
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch

import _noise_ref as N
import _scanline_ref as S

pytestmark = pytest.mark.gpu

ROOT = Path(__file__).resolve().parent.parent
PLANES_CAP = int(re.search(r"U8_PLANES_CAP\s*=\s*(\d+)", (ROOT / "pssr2_amd" / "csrc" / "u8_planes.h").read_text()).group(1))
D_VALUES = (0, 1, -1, 128, -128, 255, -255, 256, -256, 700, -700, 16384, -16384)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


def _moments(x, R):
    from pssr2_amd import ops
    return ops.line_moments_u8(_dev(x), R).cpu().numpy()


# ------------------------------------------------------------------------------------------------ line_moments_u8
@pytest.mark.parametrize("R", [0, 1, 3, 8, 16])
def test_line_moments_sizes_and_planes(R):
    T = 2 * R + 1
    rng = np.random.default_rng(R)
    for H, W in ((3, T), (4, 65), (5, 130), (33, 40), (64, 64)):
        for planes in (1, 3):
            x = rng.integers(0, 256, size=(planes, H, W), dtype=np.uint8)
            got = _moments(x, R)
            assert got.dtype == np.int64 and got.shape == (planes, H - 2, 3 * T + 2)
            assert np.array_equal(got, S.row_sums_ref(x, R)), (H, W, planes)
    for value in (0, 255):
        x = np.full((2, 5, 130), value, dtype=np.uint8)
        assert np.array_equal(_moments(x, R), S.row_sums_ref(x, R))


def test_line_moments_more_planes_than_the_grid_cap():
    x = np.random.default_rng(1).integers(0, 256, size=(PLANES_CAP + 6, 5, 20), dtype=np.uint8)
    assert np.array_equal(_moments(x, 1), S.row_sums_ref(x, 1))


def test_line_moments_long_rows_pass_32_bits_and_several_chunks():
    x = np.full((1, 3, 40000), 255, dtype=np.uint8)
    got = _moments(x, 8)
    assert np.array_equal(got, S.row_sums_ref(x, 8))
    assert got[0, 0, 2] == 255 * 510 * (40000 - 16) > 1 << 32
    x = np.random.default_rng(2).integers(0, 256, size=(2, 4, 9001), dtype=np.uint8)         # three chunks, the last one short, odd row length
    assert np.array_equal(_moments(x, 16), S.row_sums_ref(x, 16))


def test_line_moments_a_workgroup_walks_many_rows():
    x = np.random.default_rng(3).integers(0, 256, size=(1, 300, 20), dtype=np.uint8)
    assert np.array_equal(_moments(x, 3), S.row_sums_ref(x, 3))
    x = np.random.default_rng(4).integers(0, 256, size=(2, 1500, 33), dtype=np.uint8)        # runs of more rows than the ring holds
    assert np.array_equal(_moments(x, 16), S.row_sums_ref(x, 16))


def test_line_moments_copies_a_non_contiguous_input_and_repeats_itself():
    from pssr2_amd import ops
    base = _dev(np.random.default_rng(5).integers(0, 256, size=(2, 40, 70), dtype=np.uint8))
    view = base[:, 3:30, 5:61]                                    # a non-contiguous view is copied, not refused
    assert not view.is_contiguous()
    got = ops.line_moments_u8(view, 3)
    assert np.array_equal(got.cpu().numpy(), S.row_sums_ref(view.cpu().numpy(), 3))
    assert torch.equal(got, ops.line_moments_u8(view, 3))
    off = base.flatten()[1:1 + 2 * 13 * 70].view(2, 13, 70)       # contiguous, but not 16-byte aligned
    assert np.array_equal(ops.line_moments_u8(off, 8).cpu().numpy(), S.row_sums_ref(off.cpu().numpy(), 8))
    for bad, exc in ((base.cpu(), ValueError), (base.float(), ValueError), (base[:, :2], ValueError), (base[..., :5], ValueError)):
        with pytest.raises(exc):
            ops.line_moments_u8(bad, 3)
    with pytest.raises(ValueError):
        ops.line_moments_u8(base, ops.MAX_SCAN_RADIUS + 1)


# ------------------------------------------------------------------------------------------------ shift_rows_u8
@pytest.mark.parametrize("W", [1, 15, 16, 17, 130])
def test_shift_rows_u8_against_the_restatement(W):
    from pssr2_amd import ops
    rng = np.random.default_rng(W)
    x = rng.integers(0, 256, size=(3, 5, W), dtype=np.uint8)
    tables = [np.resize(np.array(D_VALUES, dtype=np.int32), 15).reshape(3, 5), np.resize(np.array(D_VALUES[::-1], dtype=np.int32), 15).reshape(3, 5),
              rng.integers(-16384, 16385, size=(3, 5)).astype(np.int32), rng.integers(-600, 601, size=(3, 5)).astype(np.int32),
              np.array([40000, -40000, 2 ** 31 - 1, -2 ** 31, 0] * 3, dtype=np.int32).reshape(3, 5)]          # beyond +-16384: clamped
    for table in tables:
        got = ops.shift_rows_u8(_dev(x), _dev(table))
        assert got.dtype == torch.uint8 and np.array_equal(got.cpu().numpy(), S.shift_rows_ref(x, table)), table
    with pytest.raises(ValueError):
        ops.shift_rows_u8(_dev(x), _dev(tables[0][:2]))
    with pytest.raises(ValueError):
        ops.shift_rows_u8(_dev(x), _dev(tables[0].astype(np.int64)))


def test_shift_rows_u8_several_pieces_per_row():
    from pssr2_amd import ops
    x = np.random.default_rng(8).integers(0, 256, size=(2, 7, 48), dtype=np.uint8)
    table = np.random.default_rng(9).integers(-3000, 3001, size=(2, 7)).astype(np.int32)
    assert np.array_equal(ops.shift_rows_u8(_dev(x), _dev(table)).cpu().numpy(), S.shift_rows_ref(x, table))


@pytest.mark.parametrize("k", [-3, -1, 0, 1, 2])
def test_correction_undoes_an_integer_plant(k):
    from pssr2_amd import ops, util
    x = np.random.default_rng(10).integers(0, 256, size=(2, 1, 9, 40), dtype=np.uint8)
    planted = ops.shift_rows_u8(_dev(x), _dev(S.odd_rows_table(x.shape, 256 * k).astype(np.int32)))
    assert np.array_equal(planted.cpu().numpy(), S.plant_ref(x, k))
    back, phase = util.correct_scan_phase(planted, k)
    a = abs(k)
    assert phase == k and back.dtype == np.uint8 and np.array_equal(back[..., a:40 - a], x[..., a:40 - a])
    assert np.array_equal(back, S.correct_ref(S.plant_ref(x, k), k))


# ------------------------------------------------------------------------------------------------ shift_rows_f32, scan_rows_table
@pytest.mark.parametrize("flags", [0, 1, 2])
def test_shift_rows_f32_against_the_restatement(flags):
    from pssr2_amd import ops
    rng = np.random.default_rng(20 + flags)
    for W in (1, 15, 16, 130):
        table = np.resize(np.array(D_VALUES, dtype=np.int32), 15).reshape(3, 5) if W != 130 else rng.integers(-16384, 16385, size=(3, 5)).astype(np.int32)
        whole = rng.integers(0, 256, size=(3, 5, W)).astype(np.float32)
        broken = (rng.random((3, 5, W)) * 300.0 - 20.0).astype(np.float32)
        for x, gain in ((whole, 0.0), (whole, 0.5), (whole, -3.25), (broken, 0.0), (broken, 1.7)):
            got = ops.shift_rows_f32(_dev(x), _dev(table), gain, flags).cpu().numpy()
            want, fragile = S.shift_rows_ref(x, table, gain, flags)
            assert got.dtype == np.float32 and np.array_equal(got[~fragile], want[~fragile]), (W, gain)
            assert fragile.mean() <= 0.01


@pytest.mark.parametrize("spread", [0.0, 0.25])
@pytest.mark.parametrize("jitter", [0.0, 0.25])
def test_scan_rows_table_against_the_restatement(spread, jitter):
    from pssr2_amd import ops
    for off in (0, 1 << 40):
        got = ops.scan_rows_table(4, 1, 64, 1.5, spread, jitter, 1234, off).cpu().numpy()
        want, fragile = S.scan_table_ref(4, 1, 64, 1.5, spread, jitter, 1234, off)
        assert got.dtype == np.int32 and got.shape == (4, 1, 64)
        assert fragile.sum() <= 2 and fragile.mean() <= 0.01
        assert np.array_equal(got[~fragile], want[~fragile])
    counter = torch.tensor([5], dtype=torch.int64, device="cuda")
    assert torch.equal(ops.scan_rows_table(4, 2, 9, -0.75, spread, jitter, 77, 100, tile_counter=counter), ops.scan_rows_table(4, 2, 9, -0.75, spread, jitter, 77, 105))
    got = ops.scan_rows_table(3, 2, 9, -0.75, spread, jitter, 77, 100).cpu().numpy()          # frames: the jitter counter is c h + y
    want, fragile = S.scan_table_ref(3, 2, 9, -0.75, spread, jitter, 77, 100)
    assert np.array_equal(got[~fragile], want[~fragile])
    big = ops.scan_rows_table(2, 1, 8, 100.0, 0.0, jitter, 1, 0).cpu().numpy()                 # beyond 64 pixels: clamped
    assert (big[:, :, 1::2] == S.MAX_D).all()


# ------------------------------------------------------------------------------------------------ the pair generator
@pytest.fixture(scope="module")
def hr_batch():
    from pssr2_amd.data import synthetic_em_tile
    return np.stack([synthetic_em_tile(i, 256) for i in range(4)])          # [4, 1, 256, 256] -> LR [4, 1, 64, 64]


def test_pair_generator_scanphase_equals_the_restatements(hr_batch):
    from pssr2_amd import ops
    from pssr2_amd.crappifiers import ScanPhase
    from pssr2_amd.data import DevicePairGenerator
    cr = ScanPhase(1.5, jitter=0.25)
    hr = _dev(hr_batch)
    lr_u8 = ops.bilinear_down_u8(hr, 64, 64).cpu().numpy().astype(np.float32)
    for off in (0, 3):
        hr_f, lr = DevicePairGenerator(4, cr, seed=42)(hr, tile_offset=off)
        assert torch.equal(hr_f, hr.float()) and lr.shape == (4, 1, 64, 64) and lr.dtype == torch.float32
        d, row_fragile = S.scan_table_ref(4, 1, 64, 1.5, 0.0, 0.25, 42, off)
        want, fragile = S.shift_rows_ref(lr_u8, d, 0.0, N.ROUND_CLIP)
        fragile |= row_fragile[..., None]
        assert fragile.mean() <= 0.02
        got = lr.cpu().numpy()
        assert np.array_equal(got[~fragile], want[~fragile])
        host = np.stack([np.clip(np.rint(cr.crappify(lr_u8[i], table=d[i])), 0, 255) for i in range(4)]).astype(np.float32)
        assert np.array_equal(got[~fragile], host[~fragile])
    assert (got[:, :, 1::2] != lr_u8[:, :, 1::2]).mean() > 0.5           # the odd rows really moved


def test_pair_generator_scanphase_inside_a_multicrappifier(hr_batch):
    from pssr2_amd import ops
    from pssr2_amd.crappifiers import MultiCrappifier, Poisson, ScanPhase
    from pssr2_amd.data import DevicePairGenerator
    hr = _dev(hr_batch)
    lr_u8 = ops.bilinear_down_u8(hr, 64, 64).cpu().numpy().astype(np.float32)
    _, lr = DevicePairGenerator(4, MultiCrappifier(ScanPhase(1.0), Poisson()), seed=42)(hr, tile_offset=7)
    d, row_fragile = S.scan_table_ref(4, 1, 64, 1.0, 0.0, 0.0, 42, 7)
    assert not row_fragile.any() and (d[:, :, 1::2] == 256).all()
    moved, fragile = S.shift_rows_ref(lr_u8, d, 0.0, N.CLIP)
    assert not fragile.any()
    want, fragile, _ = N.poisson(moved, 1.0, 0.0, 0.0, 42 + 7919, 7, N.ROUND_CLIP)          # the second stage sees seed + 7919
    got = lr.cpu().numpy()
    assert fragile.mean() <= 0.01 and np.array_equal(got[~fragile], want[~fragile])


def test_from_stacks_applies_the_phase_after_the_geometry(hr_batch):
    from pssr2_amd import ops
    from pssr2_amd.crappifiers import ScanPhase
    from pssr2_amd.data import DevicePairGenerator
    gen = DevicePairGenerator(4, ScanPhase(2.0), seed=1)
    stacks = [_dev(hr_batch[i]) for i in range(2)]
    rotations = [[True, 2], False]
    _, lr = gen.from_stacks(stacks, 256, rotations)
    turned = ops.bilinear_down_u8(ops.gen_pair_geometry_u8(stacks, rotations, 256), 64, 64).cpu().numpy().astype(np.float32)
    want, _ = S.shift_rows_ref(turned, S.odd_rows_table(turned.shape, 512), 0.0, N.ROUND_CLIP)
    assert np.array_equal(lr.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ estimate_scan_phase / correct_scan_phase
def _planted(c, res=64):
    from pssr2_amd.data import synthetic_em_tile
    phases = (1.30, -2.25)
    return np.stack([S.plant_ref(np.concatenate([synthetic_em_tile(2 * i + j, res) for j in range(c)]), phi) for i, phi in enumerate(phases)]), phases


@pytest.mark.parametrize("c", [1, 3])
def test_estimate_scan_phase_equals_the_restatement(c):
    from pssr2_amd import util
    x, phases = _planted(c)                                      # [2, c, 64, 64]
    want = {"all": S.estimate_ref(x, 8), "item": [S.estimate_ref(x[i], 8) for i in range(2)],
            "plane": [[S.estimate_ref(x[i, j], 8) for j in range(c)] for i in range(2)]}
    for given in (x, _dev(x)):
        fit = util.estimate_scan_phase(given, radius=8, pool="all")
        assert isinstance(fit.phase, float) and isinstance(fit.shift, int) and fit.radius == 8 and fit.curve.shape == (17,)
        assert (fit.shift, fit.phase, fit.score, fit.curve.tolist()) == want["all"]
        fit = util.estimate_scan_phase(given, radius=8, pool="item")
        assert fit.phase.shape == (2,) and fit.shift.dtype == np.int64 and fit.curve.shape == (2, 17)
        for i in range(2):
            assert (int(fit.shift[i]), float(fit.phase[i]), float(fit.score[i]), fit.curve[i].tolist()) == want["item"][i]
            assert abs(fit.phase[i] - phases[i]) <= 0.1
        fit = util.estimate_scan_phase(given, radius=8, pool="plane")
        assert fit.phase.shape == (2, c) and fit.curve.shape == (2, c, 17)
        for i in range(2):
            for j in range(c):
                assert (int(fit.shift[i, j]), float(fit.phase[i, j]), float(fit.score[i, j]), fit.curve[i, j].tolist()) == want["plane"][i][j]
    # a 3-D input has no item axis
    fit = util.estimate_scan_phase(x[0], radius=8, pool="item")
    assert isinstance(fit.phase, float) and (fit.shift, fit.phase, fit.score, fit.curve.tolist()) == want["item"][0]
    fit = util.estimate_scan_phase(x[0], radius=8, pool="plane")
    assert fit.phase.shape == (c,) and float(fit.phase[c - 1]) == want["plane"][0][c - 1][1]
    fit = util.estimate_scan_phase(_dev(x), radius=8, pool="item", to_numpy=False)
    assert torch.is_tensor(fit.phase) and fit.phase.dtype == torch.float64 and fit.shift.dtype == torch.int64
    assert fit.phase.tolist() == [w[1] for w in want["item"]] and fit.curve.shape == (2, 17)
    assert fit.crappifier(jitter=0.1).device_spec() == ("scanphase", float(np.mean([w[1] for w in want["item"]])), 0.0, 0.0, 0.1)


def test_correct_scan_phase_equals_the_restatement():
    from pssr2_amd import util
    x, phases = _planted(3)
    want = [S.estimate_ref(x[i], 8)[1] for i in range(2)]
    out, phase = util.correct_scan_phase(x, radius=8, pool="item")
    assert phase.tolist() == want and out.dtype == np.uint8
    assert np.array_equal(out, np.stack([S.correct_ref(x[i], want[i]) for i in range(2)]))
    dev, phase = util.correct_scan_phase(_dev(x), want, pool="item", to_numpy=False)
    assert torch.is_tensor(dev) and dev.is_cuda and np.array_equal(dev.cpu().numpy(), out) and phase == want
    out, phase = util.correct_scan_phase(x, 0.5)                                               # one number for everything
    assert phase == 0.5 and np.array_equal(out, S.correct_ref(x, 0.5)) and np.array_equal(out[:, :, 0::2], x[:, :, 0::2])
    per_plane = np.array([[0.5, -1.0, 2.25], [0.0, 3.0, -0.126]])
    out, _ = util.correct_scan_phase(x, per_plane, pool="plane")
    assert np.array_equal(out, np.stack([np.stack([S.correct_ref(x[i, j], per_plane[i, j]) for j in range(3)]) for i in range(2)]))
    out, _ = util.correct_scan_phase(x[1], per_plane[1], pool="plane")                          # 3-D: one value per frame
    assert out.shape == x[1].shape and np.array_equal(out, np.stack([S.correct_ref(x[1, j], per_plane[1, j]) for j in range(3)]))
    all_out, all_phase = util.correct_scan_phase(x[0])                                          # estimate first, pool="all"
    assert all_phase == S.estimate_ref(x[0], 8)[1] and np.array_equal(all_out, S.correct_ref(x[0], all_phase))


def test_estimate_scan_phase_warns_on_the_window_edge_and_on_a_constant_image():
    from pssr2_amd import util
    from pssr2_amd.data import synthetic_em_tile
    x = S.plant_ref(synthetic_em_tile(0, 64), 3)
    with pytest.warns(UserWarning, match="edge of the search window"):
        fit = util.estimate_scan_phase(x, radius=3)
    assert fit.shift == 3 and fit.phase == 3.0
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        assert util.estimate_scan_phase(x, radius=4).shift == 3
        assert util.estimate_scan_phase(x, radius=0).shift == 0
    with pytest.warns(UserWarning, match="constant"):
        fit = util.estimate_scan_phase(np.full((1, 8, 40), 9, dtype=np.uint8), radius=2)
    assert fit.phase == 0.0 and fit.score == 0.0 and fit.shift == 0


def test_correction_does_not_lower_the_frc_along_the_scan_lines():
    """frc_sectors(sectors=2) of (clean, planted-then-corrected) against (clean, planted): sector 0 holds the detail along a scan line."""
    from pssr2_amd import util
    from pssr2_amd.data import synthetic_em_tile
    clean = synthetic_em_tile(1, 128)
    planted = S.plant_ref(clean, 1.5)
    corrected, phase = util.correct_scan_phase(planted)
    assert abs(phase - 1.5) <= 0.1
    before = util.frc_sectors(clean, planted, sectors=2)
    after = util.frc_sectors(clean, corrected, sectors=2)
    print("FRC along x, mean of the curve: planted", np.nanmean(before.curve[0]), "corrected", np.nanmean(after.curve[0]),
          "resolution", before.resolution[0], after.resolution[0])
    assert np.nanmean(after.curve[0]) >= np.nanmean(before.curve[0])
