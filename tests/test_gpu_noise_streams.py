"""The Philox-driven kernels of csrc/crappify.hip -- additive Gaussian, Poisson, salt and pepper, per-tile blur -- value for value
against their host restatement (tests/_noise_ref.py, itself pinned by tests/test_noise_ref.py), with the device's OWN draws: the
streams are counter based, so an output is a pure function of (seed, tile, pixel).  Also what surrounds them in a training batch: the
grid-stride loops, the device tile counter, the seeds of a crappifier chain, the Pillow reduction at its ratio and plane limits, the
untested branches of the geometry kernel, and the launchers' argument checks.

Comparison rule: float32 outputs are compared with np.array_equal after dropping the restatement's `fragile` elements (values next
to a rounding decision, where the last bit of log / cos may differ between host and device); the dropped share must be <= 1e-4 and is
printed.  tests/test_noise_ref.py measures it, and the margins of the Poisson sampler's comparisons, for these same inputs on the CPU."""
import ctypes as C

import numpy as np
import pytest
import torch

import _noise_cases as K
import _noise_ref as R

pytestmark = pytest.mark.gpu

ERR_ARG, ERR_UNSUPPORTED = -1, -3          # include/pssr_mi355.h
BLUR_ATOL = 3e-4                           # test_gpu_pairs.test_blur_vs_oracle's bound for the same two-pass arithmetic on 0..255 data


def _dev(x):
    return torch.tensor(np.ascontiguousarray(x)).cuda()


def _run(kind, x, p0, gain, spread, seed, tile_offset, flags, counter=None):
    from pssr2_amd import ops
    fn = {"gaussian": ops.crappify_gaussian, "poisson": ops.crappify_poisson, "saltpepper": ops.crappify_saltpepper}[kind]
    return fn(x, p0, gain, spread, seed, tile_offset, flags, tile_counter=counter)


def _run_case(case, **kw):
    return _run(case.kind, _dev(K.case_input(case)), case.p0, case.gain, case.spread, case.seed, case.tile_offset, case.flags, **kw)


def _assert_equal(got, ref, what):
    got = got.cpu().numpy()
    dropped = int(ref.fragile.sum())
    print(f"{what}: {got.size} elements, {dropped} dropped as fragile")
    assert got.shape == ref.out.shape and got.dtype == np.float32
    assert dropped <= 1e-4 * got.size
    keep = ~ref.fragile
    if not np.array_equal(got[keep], ref.out[keep]):
        bad = np.flatnonzero((got != ref.out) & keep)
        first = [(int(i), float(got.flat[i]), float(ref.out.flat[i])) for i in bad[:6]]
        pytest.fail(f"{what}: {bad.size} of {got.size} elements differ from the restatement; (index, device, host): {first}")


@pytest.mark.parametrize("case", K.SMALL_CASES, ids=lambda c: c.id)
def test_noise_kernel_equals_restatement(case):
    """3 tiles of 1961 pixels: tile boundaries fall inside workgroups.  Gaussian: every flag with and without a per-tile sigma, a tile
    offset beyond 2^40, seed 0.  Poisson: both samplers, their switch at 10, lambda <= 0, values past 255; plain, mixed, and mixed
    with a per-tile mix.  Salt and pepper: both amounts, with and without a per-tile amount."""
    _assert_equal(_run_case(case), K.reference(case), case.id)


def test_noise_kernels_touch_what_they_should():
    """The cases mean something: the clip acts on both sides, both Poisson samplers ran, untouched salt-and-pepper pixels are exact."""
    by_id = {c.id: c for c in K.CASES}
    raw, clipped = K.reference(by_id["gaussian-f0-s0"]).out, K.reference(by_id["gaussian-f1-s0"]).out
    assert (raw < 0).any() and (raw > 255).any() and clipped.min() == 0.0 and clipped.max() == 255.0
    x = K.case_input(by_id["poisson-i1-g0-s0-f0"])
    y = K.reference(by_id["poisson-i1-g0-s0-f0"]).out
    assert ((x > 0) & (x < 10)).sum() > 500 and (x >= 10).sum() > 500 and np.all(y[x <= 0] == 0) and np.array_equal(y, np.round(y))
    sp = K.reference(by_id["saltpepper-a0.05-s0-f0"]).out
    assert np.all((sp == 0) | (sp == 255) | (sp == np.float32(103.25))) and 0.03 < (sp != np.float32(103.25)).mean() < 0.07


def test_tile_index_is_offset_plus_tile():
    """The comparison bites on the tile index: the device's tile t at offset 5 is the restatement's at offset 5, not at offset 6 -- but
    its tile 1 is the restatement's tile 0 at offset 6."""
    case = next(c for c in K.CASES if c.id == "gaussian-f0-s3")
    got = _run_case(case).cpu().numpy()
    shifted = R.gaussian(K.case_input(case), case.p0, case.gain, case.spread, case.seed, case.tile_offset + 1, case.flags)[0]
    assert (got != shifted).mean() > 0.99
    one = R.gaussian(K.case_input(case)[1:2], case.p0, case.gain, case.spread, case.seed, case.tile_offset + 1, case.flags)[0]
    assert np.array_equal(got[1:2], one)


@pytest.mark.parametrize("case", K.STRIDE_CASES, ids=lambda c: c.id)
def test_grid_stride(case):
    """More elements than one sweep of the grid covers: the launchers start at most 8192 workgroups (grid1d's cap) of 256 threads,
    2,097,152 elements, and the kernels stride over the rest -- the last 8,848 of these 2,106,000."""
    x = K.case_input(case)
    assert x.size > K.GRID_CAP_BLOCKS * K.BLOCK_THREADS
    _assert_equal(_run_case(case), K.reference(case), case.id)


def _blur(x, sigma, spread, tile_offset, counter=None):
    from pssr2_amd import ops
    return ops.gaussian_blur_tiles(x, sigma, spread, K.BLUR_GAIN, K.SEED_B, tile_offset, 0, tile_counter=counter)


@pytest.mark.parametrize("name", ["A", "B"])
def test_per_tile_blur_draws_the_stated_sigma(name):
    """16 tiles, each blurred with the sigma the restatement says its stream draws (A: N(2, 0.5); B: max(N(0.3, 1), 0), where about
    four tiles in ten draw 0 and must come out as the input plus the gain, exactly)."""
    sigma, spread = K.BLUR_CASES[name]
    x = K.blur_input()
    sig = R.blur_sigma(K.SEED_B, x.shape[0], K.BLUR_OFFSET, sigma, spread)
    print(f"blur {name}: sigmas {np.round(sig, 4).tolist()}")
    if name == "B":
        assert (sig == 0).any() and (sig > 0).any()
    ref, _ = R.blur_tiles(x, sig, K.BLUR_GAIN, 0)
    got = _blur(_dev(x), sigma, spread, K.BLUR_OFFSET).cpu().numpy()
    for t in range(x.shape[0]):
        if sig[t] == 0:
            assert np.array_equal(got[t], x[t] + np.float32(K.BLUR_GAIN)), t
        else:
            np.testing.assert_allclose(got[t], ref[t], rtol=0, atol=BLUR_ATOL, err_msg=f"tile {t}, sigma {sig[t]}")
    assert np.abs(got - (x + np.float32(K.BLUR_GAIN))).max() > 1.0           # and something was blurred


def test_fixed_sigma_blur_wider_than_the_image():
    """sigma 2 on 5 x 7 planes: the radius, 8, exceeds both sides, so every tap row runs into the replicated edge."""
    from scipy import ndimage
    from pssr2_amd import ops
    img = np.random.default_rng(7).uniform(0, 255, (3, 5, 7)).astype(np.float32)
    got = ops.gaussian_blur(_dev(img), 2.0, 1.5, 0).cpu().numpy()
    ref = np.stack([ndimage.gaussian_filter(p, 2.0, mode="nearest", truncate=4.0) for p in img])
    np.testing.assert_allclose(got, ref + np.float32(1.5), rtol=0, atol=BLUR_ATOL)


@pytest.mark.parametrize("kind", ["gaussian", "poisson", "saltpepper", "blur"])
def test_tile_counter_adds_to_the_offset(kind):
    """What a captured training step replays with: offset 3 plus a device counter holding 4 draws what offset 7 draws, and after
    counter_add(counter, 2) what offset 9 draws."""
    from pssr2_amd import ops
    if kind == "blur":
        x = _dev(K.blur_input()[:4])

        def run(offset, counter=None):
            return _blur(x, 2.0, 0.5, offset, counter)
    else:
        case = next(c for c in K.SMALL_CASES if c.kind == kind and c.spread > 0)
        x = _dev(K.case_input(case))

        def run(offset, counter=None):
            return _run(kind, x, case.p0, case.gain, case.spread, case.seed, offset, case.flags, counter)
    counter = torch.tensor([4], dtype=torch.int64, device="cuda")
    at7, at9 = run(7), run(9)
    assert not torch.equal(at7, run(3)) and not torch.equal(at7, at9)
    assert torch.equal(run(3, counter), at7)
    ops.counter_add(counter, 2)
    assert counter.item() == 6
    assert torch.equal(run(3, counter), at9)


def test_chain_seeds_and_clip_between_stages():
    """DevicePairGenerator over MultiCrappifier(AdditiveGaussian(13, spread=2), Poisson(0.5, spread=0.1)): stage i runs with
    seed + 7919 * i, the first stage clips, the last rounds and clips.  4 HR tiles of 256 x 256, i.e. LR tiles of 64 x 64."""
    from pssr2_amd.crappifiers import AdditiveGaussian, MultiCrappifier, Poisson
    from pssr2_amd.data import DevicePairGenerator
    hr = K.chain_input()
    gen = DevicePairGenerator(4, MultiCrappifier(AdditiveGaussian(13, spread=2), Poisson(0.5, spread=0.1)), seed=K.SEED_CHAIN)
    hr_d, lr_d = gen(_dev(hr))
    assert np.array_equal(hr_d.cpu().numpy(), hr.astype(np.float32))
    _, ref = K.chain_reference()
    _assert_equal(lr_d, ref, "chain")


@pytest.mark.parametrize("shape,out", [((1030, 1, 8, 12), (2, 3)), ((2, 1, 38, 57), (2, 3)), ((2, 1, 16, 16), (16, 16))],
                         ids=["1030-planes", "ratio-19", "ratio-1"])
def test_pillow_reduction_limits(shape, out):
    """More planes than the vertical pass has workgroups for (1024), the largest ratio it supports, and no reduction at all."""
    from oracle import pairs_ref as P
    from pssr2_amd import ops
    hr = np.random.default_rng(8).integers(0, 256, shape, dtype=np.uint8)
    assert np.array_equal(ops.bilinear_down_u8(_dev(hr), *out).cpu().numpy(), P.pil_bilinear_u8(hr, *out))


def _stream():
    from pssr2_amd import _lib as L
    return L.stream_ptr()


def test_pillow_reduction_refuses_ratio_20():
    from pssr2_amd import _lib as L
    hr = torch.zeros(40 * 40, dtype=torch.uint8, device="cuda")
    tmp, lr = torch.full((40 * 2,), 7, dtype=torch.uint8, device="cuda"), torch.full((4,), 7, dtype=torch.uint8, device="cuda")
    assert L.lib().pssr_bilinear_down_u8(L.ptr(hr), L.ptr(tmp), L.ptr(lr), 1, 40, 40, 2, 2, _stream()) == ERR_UNSUPPORTED
    torch.cuda.synchronize()
    assert bool((lr == 7).all()) and bool((tmp == 7).all())                  # nothing was launched


@pytest.mark.parametrize("sources,rotations,res", [
    ([(3, 12, 12)], [[False, 0]], 8),
    ([(3, 12, 12), (3, 9, 14)], [[True, 0], [True, 0]], 8),
    ([(2, 1, 9), (2, 9, 1)], [False, [True, 2]], 6),
    ([(3, 7, 5), (3, 7, 5), (3, 5, 6)], [False, [True, (1, 2)], [True, 0]], 16),
], ids=["frame-flip", "frame-flip-rot90", "side-of-1", "reflect-periods-3-frames"])
def test_geometry_branches(sources, rotations, res):
    """gen_pair_geometry_u8 against the oracle's crop, reflect pad, rot90 and flip: the flip along the frame axis alone and after a
    rot90, a source with a side of 1 (its crop is one pixel, repeated), and reflect padding over more than one period with 3 frames."""
    from oracle import pairs_ref as P
    from pssr2_amd import ops
    rng = np.random.default_rng(9)
    stacks = [rng.integers(0, 256, s, dtype=np.uint8) for s in sources]
    got = ops.gen_pair_geometry_u8([_dev(s) for s in stacks], rotations, res).cpu().numpy()
    for i, (s, rot) in enumerate(zip(stacks, rotations)):
        ref = P.augment(P.pad_image(P.square_crop(s, res), res), rot)
        assert ref.shape == got[i].shape and np.array_equal(got[i], ref), (i, s.shape, rot)
    if rotations[0] and rotations[0][1] == 0:
        plain = ops.gen_pair_geometry_u8([_dev(stacks[0])], [False], res).cpu().numpy()
        assert not np.array_equal(plain[0], got[0])                          # the frames differ, so the flip shows


def test_argument_checks_return_without_launching():
    from pssr2_amd import _lib as L
    lib = L.lib()
    x = torch.zeros(2, 64, device="cuda")
    out = torch.full_like(x, 7.0)
    f, u64 = C.c_float, C.c_uint64
    assert lib.pssr_crappify_gaussian(L.ptr(x), L.ptr(out), 2, C.c_int64(64), f(13), f(0), f(0), u64(1), u64(0), None, 4, None,
                                      _stream()) == ERR_ARG
    assert lib.pssr_crappify_poisson(L.ptr(x), L.ptr(out), 2, C.c_int64(64), f(1), f(0), f(0), u64(1), u64(0), 4, None, _stream()) == ERR_ARG
    assert lib.pssr_crappify_saltpepper(L.ptr(x), L.ptr(out), 2, C.c_int64(64), f(-0.01), f(0), f(0), u64(1), u64(0), 0, None,
                                        _stream()) == ERR_ARG
    assert lib.pssr_counter_add(None, u64(1), _stream()) == ERR_ARG
    torch.cuda.synchronize()
    assert bool((out == 7.0).all())
