"""tests/_noise_ref.py, the host restatement of the device noise streams, is itself right: published Philox known answers, the 64-bit
key arithmetic against Python integers, the quality of the streams, the restated Poisson sampler against numpy's, and -- for every
input and seed of tests/test_gpu_noise_streams.py -- the premises under which that file compares for equality.  No GPU."""
import numpy as np
import pytest

import _noise_cases as K
import _noise_ref as R

N = 1 << 18
SEED = 0x123456789ABCDEF0


def _words(*w):
    return tuple(int(v) for v in w)


@pytest.mark.parametrize("counter,key,answer", [
    ((0, 0, 0, 0), (0, 0), (0x6627E8D5, 0xE169C58D, 0xBC57AC4C, 0x9B00DBD8)),
    ((0xFFFFFFFF,) * 4, (0xFFFFFFFF,) * 2, (0x408F276D, 0x41C83B0E, 0xA20BC7C6, 0x6D5451FD)),
    ((0x243F6A88, 0x85A308D3, 0x13198A2E, 0x03707344), (0xA4093822, 0x299F31D0), (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)),
])
def test_philox_known_answers(counter, key, answer):
    """The three Random123 known-answer vectors of Philox4x32-10."""
    assert _words(*R.philox4x32_10(*counter, *key)) == answer


def test_draw_lays_the_counter_out_as_the_kernel_does():
    """draw() = Philox of (low32(counter), high32(counter), sub, 0x1BD11BDA) under both words of the key: with the stream key undone
    (seed = key ^ constant at tile 0) it reproduces the third known answer only if neither the high counter word nor the high key
    word is dropped."""
    key = 0x299F31D0A4093822
    seed = key ^ 0xD1B54A32D192ED03
    assert _words(*R.stream_key(seed, 0)) == (0xA4093822, 0x299F31D0)
    counter = (0x85A308D3 << 32) | 0x243F6A88
    k0, k1 = R.stream_key(seed, 0)
    assert _words(*R.philox4x32_10(counter & 0xFFFFFFFF, counter >> 32, 0x13198A2E, 0x03707344, k0, k1)) == \
        (0xD16CFE09, 0x94FDCCEB, 0x5001E420, 0x24126EA1)
    # the same through draw(): c3 is fixed there, so compare with the plain function at draw's own layout
    got = R.draw(seed, 0, counter, 0x13198A2E)
    assert _words(*got) == _words(*R.philox4x32_10(0x243F6A88, 0x85A308D3, 0x13198A2E, 0x1BD11BDA, 0xA4093822, 0x299F31D0))
    assert _words(*got) != _words(*R.draw(seed, 0, counter & 0xFFFFFFFF, 0x13198A2E))          # the high counter word counts
    assert _words(*got) != _words(*R.draw(seed & 0xFFFFFFFF, 0, counter, 0x13198A2E))          # and the high seed word


def test_stream_key_wraps_like_64_bit_integers_and_is_injective():
    for seed, tile in ((0xFEDCBA9800000001, (1 << 40) + 3), (SEED, (1 << 40) - 1), (0, 0), ((1 << 64) - 1, (1 << 64) - 1)):
        k = (seed ^ ((tile * 0x9E3779B97F4A7C15 + 0xD1B54A32D192ED03) % (1 << 64)))
        assert _words(*R.stream_key(seed, tile)) == (k & 0xFFFFFFFF, k >> 32)
    lo, hi = R.stream_key(SEED, np.arange(4096))
    assert np.unique((hi << np.uint64(32)) | lo).size == 4096


def test_u01_is_strictly_inside_the_unit_interval():
    u = R.u01(np.array([0, 0xFFFFFFFF, 0x80000000, 0xFFFFFFFF]), np.array([0, 0xFFFFFFFF, 0, 0xFFFFF7FF]))
    assert np.all(u > 0.0) and np.all(u < 1.0)
    assert u[0] == 2.0 ** -54 and u[2] == 0.5 and u[1] == 1.0 - 2.0 ** -53   # 2^52 + 0.5 is a tie and rounds to even; so would 2^53 - 0.5


def test_finish_rounds_half_to_even_and_clips():
    v = np.array([-0.5, 0.5, 1.5, 2.5, 254.5, 255.5, -3.2, -0.49, 0.49, 100.5, 101.5, 255.49, 300.0, -1e9, 12.0])
    assert np.array_equal(R.finish(v, R.ROUND_CLIP), np.clip(np.round(v), 0, 255))
    assert np.array_equal(R.finish(v, 3), np.clip(np.round(v), 0, 255))
    assert np.array_equal(R.finish(v, R.CLIP), np.clip(v, 0, 255))
    assert np.array_equal(R.finish(v, 0), v)
    assert R.finish(np.array([0.5, 1.5, 2.5, 254.5]), R.ROUND_CLIP).tolist() == [0.0, 2.0, 2.0, 254.0]


def test_fragile_marks_near_ties_and_keeps_exact_ones():
    up = float(np.nextafter(np.float32(100.0), np.float32(200.0)))
    mid = 0.5 * (100.0 + up)                                     # a float32 rounding midpoint, exactly representable in float64
    v = np.array([7.5, 7.5 + 1e-12, 7.5 - 1e-12, 7.4, mid, mid * (1 + 1e-14), mid * (1 + 1e-11), 1e-12, 255.0 + 1e-10, 0.0, 255.0])
    T, F = True, False
    assert R.to_f32(v, R.ROUND_CLIP)[1].tolist() == [F, T, T, F, F, F, F, F, F, F, F]
    assert R.to_f32(v, 0)[1].tolist() == [F, F, F, F, F, T, F, F, F, F, F]
    assert R.to_f32(v, R.CLIP)[1].tolist() == [F, F, F, F, F, T, F, T, T, F, F]
    # the midpoint window is relative to the terms of the sum, where the caller knows them: 100 = 1e5 - 99900 has lost three digits
    assert R.to_f32(np.array([mid * (1 + 1e-11)]), 0, np.array([1e5]))[1].tolist() == [T]


def _corr(a, b):
    return float(np.corrcoef(a, b)[0, 1])


def test_stream_quality():
    """Mean, deviation and the correlations a counter mix-up would raise: along pixels, between neighbouring tiles, between subs."""
    pix = np.arange(N, dtype=np.uint64)
    z = R.normal(R.draw(SEED, 5, pix, 0))
    assert abs(z.mean()) < 4 / np.sqrt(N) and abs(z.std() - 1.0) < 4 / np.sqrt(2 * N)
    bound = 4 / np.sqrt(N)
    assert abs(_corr(z[:-1], z[1:])) < bound
    assert abs(_corr(z, R.normal(R.draw(SEED, 6, pix, 0)))) < bound
    assert abs(_corr(z, R.normal(R.draw(SEED, 5, pix, 1)))) < bound
    u = R.u01(*R.draw(SEED, 5, pix, 0)[:2])
    assert abs(u.mean() - 0.5) < 4 / np.sqrt(12 * N)


@pytest.mark.parametrize("lam", [0.5, 3.0, 9.999, 10.0, 40.0, 200.0])
def test_restated_poisson_is_poisson(lam):
    from scipy import stats
    k, margin = R.poisson_draw(SEED, 5, np.arange(N, dtype=np.uint64), np.full(N, lam))
    assert np.array_equal(k, np.floor(k)) and k.min() >= 0
    assert abs(k.mean() - lam) < 4 * np.sqrt(lam / N)
    # var of the sample variance of a Poisson: (mu4 - sigma^4) / n with mu4 = lam + 3 lam^2
    assert abs(k.var() - lam) < 4 * np.sqrt((lam + 2 * lam * lam) / N)
    assert stats.ks_2samp(k, np.random.default_rng(0).poisson(lam, N)).pvalue > 1e-3
    assert margin > 0


def test_restated_poisson_edges():
    lam = np.array([0.0, -1.0, -0.0, 5.0, 50.0])
    k, _ = R.poisson_draw(SEED, 0, np.arange(5, dtype=np.uint64), lam)
    assert k[:3].tolist() == [0.0, 0.0, 0.0]
    # one pixel's draw does not depend on what it is batched with, nor on the shape it is asked in
    k2, _ = R.poisson_draw(SEED, 0, np.array([[3], [4]], dtype=np.uint64), np.array([[5.0], [50.0]]))
    assert k2.shape == (2, 1) and k2.ravel().tolist() == k[3:].tolist()


def test_tile_intensity_and_blur_sigma():
    t = np.arange(5, 9, dtype=np.uint64)
    assert R.tile_intensity(SEED, t, 0.1, 0.0).tolist() == [float(np.float32(0.1))] * 4
    z = R.normal(R.draw(SEED, t, (1 << 64) - 1, 7))
    assert np.array_equal(R.tile_intensity(SEED, t, 2.0, 0.5), np.maximum(2.0 + 0.5 * z, 0.0))
    assert np.array_equal(R.blur_sigma(SEED, 4, 5, 2.0, 0.5), R.tile_intensity(SEED, t, 2.0, 0.5))
    many = R.tile_intensity(SEED, np.arange(4096, dtype=np.uint64), 0.3, 1.0)
    assert many.min() == 0.0 and abs((many == 0).mean() - 0.382) < 0.04        # P(N(0.3, 1) <= 0) = 0.382


def test_blur_restatement_states_what_the_oracle_states():
    """blur_tiles divides the sum by the sum of the weights where oracle.pairs_ref.gaussian_blur_nearest normalises the weights first:
    the same blur to float32 rounding.  Sigma 0 is the identity plus gain."""
    from oracle import pairs_ref as P
    x = K.blur_input()[:3]
    out, _ = R.blur_tiles(x, [2.0, 0.7, 0.0], 1.5, 0)
    for t, s in enumerate((2.0, 0.7)):
        np.testing.assert_allclose(out[t], P.gaussian_blur_nearest(x[t], s) + 1.5, rtol=0, atol=1e-4)
    assert np.array_equal(out[2], x[2] + np.float32(1.5))


@pytest.mark.parametrize("case", K.CASES, ids=lambda c: c.id)
def test_premises_of_the_gpu_comparison(case):
    """What tests/test_gpu_noise_streams.py relies on, per input set: no comparison of the samplers closer than a relative 1e-10 to
    tipping, and at most 1e-4 of the elements next to a rounding decision."""
    ref = K.reference(case)
    share = ref.fragile.mean()
    print(f"{case.id}: {ref.out.size} elements, margin {ref.margin:.3g}, fragile {int(ref.fragile.sum())} ({share:.2g})")
    assert ref.margin >= 1e-10
    assert share <= 1e-4
    assert ref.out.dtype == np.float32 and ref.out.shape == K.case_input(case).shape
    if case.id.startswith("stride-"):
        assert ref.out.size > K.GRID_CAP_BLOCKS * K.BLOCK_THREADS


def test_premises_of_the_chain_and_blur_cases():
    lr, ref = K.chain_reference()
    print(f"chain: {ref.out.size} elements, margin {ref.margin:.3g}, fragile {int(ref.fragile.sum())}")
    assert ref.margin >= 1e-10 and ref.fragile.mean() <= 1e-4
    assert np.abs(ref.out - lr).mean() > 1.0 and np.array_equal(ref.out, np.round(ref.out)) and ref.out.min() >= 0 and ref.out.max() <= 255
    # case B of the per-tile blur needs tiles on both sides of sigma = 0
    sig = R.blur_sigma(K.SEED_B, 16, K.BLUR_OFFSET, *K.BLUR_CASES["B"])
    print(f"blur B: sigmas {np.round(sig, 3).tolist()}")
    assert (sig == 0).any() and (sig > 0).any()
    assert (R.blur_sigma(K.SEED_B, 16, K.BLUR_OFFSET, *K.BLUR_CASES["A"]) > 0.5).all()
    for name in "AB":            # no radius int(4 * float32(sigma) + 0.5) within 1e-6 of taking another tap
        r = 4.0 * R.blur_sigma(K.SEED_B, 16, K.BLUR_OFFSET, *K.BLUR_CASES[name]).astype(np.float32).astype(np.float64) + 0.5
        assert np.abs(r - np.rint(r))[r > 0.5].min() > 1e-6


def test_a_tile_index_off_by_one_would_show():
    """What tests/test_gpu_noise_streams.py compares against changes in (nearly) every element when the tile index is read as
    tile_offset + tile + 1, for each kernel: such a device would fail every comparison there."""
    # the restatement's own tile index, written out from draw(): tile 2 at offset 5 is stream 7
    case = next(c for c in K.SMALL_CASES if c.id == "gaussian-f0-s0")
    x = K.case_input(case)[2].ravel().astype(np.float64)
    z = R.normal(R.draw(case.seed, 7, np.arange(x.size, dtype=np.uint64), 0))
    assert np.array_equal(K.reference(case).out[2].ravel(), (x + (2.0 + float(np.float32(13.0)) * z)).astype(np.float32))
    for case in (c for c in K.SMALL_CASES if c.flags == 0 and c.spread > 0):
        x = K.case_input(case)
        shifted = getattr(R, case.kind)(x, case.p0, case.gain, case.spread, case.seed, case.tile_offset + 1, case.flags)[0]
        differ = (shifted != K.reference(case).out).mean()
        assert differ > (0.05 if case.kind == "saltpepper" else 0.9), (case.id, differ)
        if case.kind == "saltpepper":        # every tile has the same input there: tile t at offset + 1 is tile t + 1 at offset
            assert np.array_equal(shifted[:-1], K.reference(case).out[1:])
