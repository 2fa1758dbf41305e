"""Decorrelation analysis on the device (csrc/frc.hip with one image per block, through ops.decorr_rings_u8, util.decorr and test_metrics)
against the numpy restatement of tests/_decorr_ref.py.  The bounds on the ring sums are, per ring r >= 1,
|A - A_ref| <= tol_A(n) sqrt(pop[r] P_ref[r]) and |P - P_ref| <= tol_P(n) P_ref[r], with tol = 8 x the error of the float32 numpy
restatement on the same inputs in the same units (measured on the CPU, recorded in _decorr_ref.py); ring 0, which the mean removal
cancels and which enters no curve, is held to the same figures in the units of the whole block (_decorr_ref.errors says why)."""
import functools
import math

import numpy as np
import pytest
import torch

import _decorr_ref as D
import _frc_ref as F

pytestmark = pytest.mark.gpu


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _rings(a, n, name="hann"):
    from pssr2_amd import ops
    got = ops.decorr_rings_u8(_dev(a), n, name)
    assert got.dtype == torch.float64 and got.is_cuda
    return got.cpu().numpy()


def _within(got, ref, n):
    ea, ep = D.errors(got, ref, n)
    return ea <= D.tol(n)[0] and ep <= D.tol(n)[1]


@functools.lru_cache(maxsize=None)
def _case(n):
    return [(a, name, D.rings_ref(a, n, name)) for a, name in D.sums_inputs(n)]


# ------------------------------------------------------------------------------------------------ ring sums
@pytest.mark.parametrize("n", D.SUMS_SIZES + D.BIG_SIZES)
def test_ring_sums_against_the_float64_fft(n):
    """The sizes of test_gpu_frc.py, for its reasons: 16 the minimum; 18, 30, 34 no multiples of an MFMA tile or of the K step; 64, 66 two
    32-tiles exactly and just over; 130 several LDS stages; 500 and 1024 once.  White noise and a planted image, both windows."""
    for a, name, ref in _case(n):
        assert (ref[..., 1:, 1] > 0).all()
        got = _rings(a, n, name)
        ea, ep = D.errors(got, ref, n)
        print(f"n={n} {name}: A {ea:.3e} (bound {D.tol(n)[0]:.3e}, float32 numpy {D.F32_ERROR[n][0]:.3e}), "
              f"P {ep:.3e} (bound {D.tol(n)[1]:.3e}, float32 numpy {D.F32_ERROR[n][1]:.3e})")
        assert ea <= D.tol(n)[0] and ep <= D.tol(n)[1]


def test_the_mean_is_the_blocks_own_and_is_taken_off():
    """What frc_rings_u8(a, a) cannot give: with the mean left in, the Hann window leaks it into rings 1 and 2, far outside the bound."""
    from pssr2_amd import ops
    a = np.concatenate([D.sums_inputs(18)[0][0] // 2, D.sums_inputs(18)[0][0] // 2 + 120], axis=2)      # two blocks, means 120 apart
    assert a.shape == (1, 18, 36)
    got, ref = _rings(a, 18), D.rings_ref(a, 18)
    assert got.shape == (1, 2, 10, 2) and _within(got, ref, 18)
    pair = ops.frc_rings_u8(_dev(a), _dev(a), 18).cpu().numpy()
    assert (pair[..., 1, 1] > 10 * ref[..., 1, 1]).all()


@pytest.mark.parametrize("H,W,n,planes", [(40, 70, 16, 1), (40, 70, 16, 3), (37, 53, 18, 1), (37, 53, 18, 3)])
def test_blocks_of_the_centred_grid(H, W, n, planes):
    """40 x 70 at 16: 2 x 4 blocks from (4, 3); 37 x 53 at 18: 2 x 2 blocks from (0, 8), odd row pitch.  The planes start at every
    address modulo 16 in turn."""
    from pssr2_amd import ops
    rng = np.random.default_rng(H + planes)
    a = rng.integers(0, 256, size=(planes, H, W), dtype=np.uint8)
    nby, nbx, _, _ = F.grid(H, W, n)
    ref = D.rings_ref(a, n)
    assert ref.shape == (planes, nby * nbx, n // 2 + 1, 2)
    first = None
    for off in range(16):
        flat = torch.zeros(off + a.size + 16, dtype=torch.uint8, device="cuda")
        flat[off:off + a.size] = _dev(a).reshape(-1)
        buf = flat[off:off + a.size].view(planes, H, W)
        assert buf.data_ptr() % 16 == off and buf.is_contiguous()
        got = ops.decorr_rings_u8(buf, n).cpu().numpy()
        assert _within(got, ref, n)
        first = got if first is None else first
        np.testing.assert_array_equal(got, first)               # where the bytes lie changes nothing


def test_more_planes_than_a_grid_axis_of_the_plane_kernels():
    """1100 planes of 16 x 16, every one with its own content and its own mean."""
    rng = np.random.default_rng(11)
    a = (rng.integers(0, 128, size=(1100, 16, 16)) + rng.integers(0, 128, size=(1100, 1, 1))).astype(np.uint8)
    got = _rings(a, 16)
    assert got.shape == (1100, 1, 9, 2) and _within(got, D.rings_ref(a, 16), 16)


def test_a_call_that_works_its_blocks_off_in_chunks():
    """224 blocks of 512 x 512 need more than the 256 MB of workspace that a chunk of blocks may take (1.22 MB a block: 220 fit): the
    call works them off in two chunks, and every block's sums are what a call of its own gives, bit for bit."""
    from pssr2_amd import _lib, ops
    gen = torch.Generator(device="cuda").manual_seed(5)
    a = torch.randint(0, 256, (224, 512, 512), dtype=torch.uint8, device="cuda", generator=gen)
    lib = _lib.lib()
    assert lib.pssr_decorr_workspace_bytes(224, 512, 512, 512) < 224 * lib.pssr_decorr_workspace_bytes(1, 512, 512, 512)
    assert lib.pssr_decorr_workspace_bytes(224, 512, 512, 512) == lib.pssr_decorr_workspace_bytes(220, 512, 512, 512)
    whole = ops.decorr_rings_u8(a, 512)
    assert whole.shape == (224, 1, 257, 2)
    for lo, hi in ((0, 1), (110, 113), (219, 221), (223, 224)):
        assert torch.equal(whole[lo:hi], ops.decorr_rings_u8(a[lo:hi], 512))


def test_non_contiguous_inputs_and_leading_dimensions():
    from pssr2_amd import ops
    rng = np.random.default_rng(12)
    wide = _dev(rng.integers(0, 256, size=(2, 3, 36, 80), dtype=np.uint8))
    a = wide[..., ::2]
    assert not a.is_contiguous()
    got = ops.decorr_rings_u8(a, 18)
    assert got.shape == (6, 4, 10, 2)
    assert torch.equal(got, ops.decorr_rings_u8(a.contiguous().reshape(6, 36, 40), 18))
    assert _within(got.cpu().numpy(), D.rings_ref(a.cpu().numpy().reshape(6, 36, 40), 18), 18)


def test_ops_check_device_tensors_too():
    """The checks of ops.decorr_rings_u8 that a host tensor never reaches."""
    from pssr2_amd import ops
    t = torch.zeros(2, 32, 48, dtype=torch.uint8, device="cuda")
    for a in (t.float(), t.short(), t[0, 0]):
        with pytest.raises(ValueError, match="uint8 device tensor"):
            ops.decorr_rings_u8(a, 16)
    for bad in (14, 17, 31, 1026, 16.0, True):
        with pytest.raises(ValueError, match="block must be"):
            ops.decorr_rings_u8(t, bad)
    for bad in (34, 48):                                        # even and in range, larger than the smaller side
        with pytest.raises(ValueError, match="does not fit"):
            ops.decorr_rings_u8(t, bad)
    with pytest.raises(ValueError, match="window"):
        ops.decorr_rings_u8(t, 16, "hamming")
    with pytest.raises(ValueError, match="at least one plane"):
        ops.decorr_rings_u8(t[:0], 16)
    assert ops.decorr_rings_u8(t, 32).shape == (2, 1, 17, 2)


# ------------------------------------------------------------------------------------------------ properties without a measured tolerance
@pytest.mark.parametrize("n", (18, 64, 130))
def test_two_calls_give_the_same_bits(n):
    from pssr2_amd import ops
    a, name, _ = _case(n)[0]
    a = _dev(np.tile(a, (3, 2, 2)))
    first = ops.decorr_rings_u8(a, n, name)
    for _ in range(3):
        assert torch.equal(ops.decorr_rings_u8(a, n, name), first)


@pytest.mark.parametrize("name", F.WINDOWS)
def test_zero_and_constant_stacks_are_exactly_zero(name):
    from pssr2_amd.util import decorr
    for v in (0, 200):
        c = np.full((2, 34, 50), v, dtype=np.uint8)
        for n in (16, 18, 34):
            got = _rings(c, n, name)
            assert got.shape == (2, (34 // n) * (50 // n), n // 2 + 1, 2) and not got.any() and not np.signbit(got).any()
        res = decorr(c, block=18, window=name, pixel_size=3.0)
        assert res.found is False and res.resolution == 6.0 and not res.curves.any() and math.isnan(res.peak) and res.amplitude == 0.0


def test_a_mean_that_is_no_float32():
    """One pixel of 1 in zeros at n = 18: m = float32(1 / 324), every other pixel is -m."""
    a = np.zeros((1, 18, 18), dtype=np.uint8)
    a[0, 7, 11] = 1
    for name in F.WINDOWS:
        assert _within(_rings(a, 18, name), D.rings_ref(a, 18, name), 18)


# ------------------------------------------------------------------------------------------------ util.decorr
# A curve is a running sum of A over sqrt(sum P . M(r)).  With every A[rho] within tol_A sqrt(pop[rho] P[rho]) the numerator moves by at most
# tol_A sum sqrt(pop P) <= tol_A sqrt(sum pop . sum P) (Cauchy-Schwarz), that is by tol_A of the denominator; with every P[rho] within
# tol_P P[rho] the denominator moves by tol_P / 2 of itself, and d <= 1.  The largest figures of the table up to n = 500 bound the block
# sides used below (64, 128, 250, 500); the filters' weights lie in [0, 1] and change neither argument.
CURVE_TOL = max(D.tol(n)[0] for n in D.F32_ERROR if n <= 500) + max(D.tol(n)[1] for n in D.F32_ERROR if n <= 500) / 2


def _device_resolve(a, n, filters=10):
    from pssr2_amd import ops
    from pssr2_amd.util import _decorr_resolve
    return _decorr_resolve(ops.decorr_rings_u8(_dev(a), n).cpu().numpy(), n, filters, 1.0)


@pytest.mark.parametrize("n,r0", D.PLANTED)
def test_decorr_finds_the_planted_cutoff(n, r0):
    """|p*_device - p*_ref| <= 1e-3 rings, the same curve chosen (tests/test_decorr_host.py holds the reference itself to
    r0 <= p* <= r0 + 1.5)."""
    from pssr2_amd.util import Decorr, decorr
    a = D.planted(n, r0, 1)
    ref = D.resolve_ref(D.rings_ref(a[None], n), n)
    assert ref["found"] and r0 <= ref["peak"] <= r0 + 1.5
    assert _device_resolve(a[None], n)[5] == ref["chosen"]
    for make in (lambda x: x, _dev):
        for to_numpy in (True, False):
            got = decorr(make(a), to_numpy=to_numpy)
            assert isinstance(got, Decorr) and got.block == n and got.found is True
            curves = got.curves if to_numpy else got.curves.cpu().numpy()
            assert (isinstance(got.curves, np.ndarray) if to_numpy else got.curves.is_cuda) and curves.shape == (11, n // 2 + 1)
            print(f"n={n} r0={r0}: p* = {got.peak:.6f} (reference {ref['peak']:.6f}), curves off by {np.abs(curves - ref['curves']).max():.2e}")
            assert abs(got.peak - ref["peak"]) <= 1e-3 and got.resolution == pytest.approx(n / got.peak, rel=1e-15)
            assert got.amplitude == pytest.approx(ref["amplitude"], abs=CURVE_TOL) and np.abs(curves - ref["curves"]).max() <= CURVE_TOL
            np.testing.assert_array_equal(got.freq, np.arange(n // 2 + 1) / n)
    # the pixel size scales the answer and the frequencies, nothing else
    plain, scaled = decorr(a), decorr(a, pixel_size=32.5)
    assert scaled.resolution == pytest.approx(32.5 * plain.resolution, rel=1e-15) and np.array_equal(scaled.curves, plain.curves)
    np.testing.assert_allclose(scaled.freq, plain.freq / 32.5, rtol=1e-15)
    # no filters: the unfiltered peak alone
    ref0 = D.resolve_ref(D.rings_ref(a[None], n), n, 0)
    got0 = decorr(a, filters=0)
    assert got0.curves.shape == (1, n // 2 + 1) and abs(got0.peak - ref0["peak"]) <= 1e-3 and np.array_equal(got0.curves[0], plain.curves[0])


@pytest.mark.parametrize("c", (1, 3))
def test_decorr_pools_the_planes_of_an_item(c):
    from pssr2_amd.util import decorr
    n, r0s = 64, (12, 20)
    a = np.stack([np.stack([D.planted(n, r0, 10 * i + j) for j in range(c)]) for i, r0 in enumerate(r0s)])
    assert a.shape == (2, c, n, n)
    got = decorr(a)
    assert got.curves.shape == (2, 11, n // 2 + 1) and got.resolution.shape == (2,) and got.found.dtype == bool and got.found.all()
    for i in range(2):
        ref = D.resolve_ref(D.rings_ref(a[i], n), n)
        assert abs(got.peak[i] - ref["peak"]) <= 1e-3 and r0s[i] <= got.peak[i] <= r0s[i] + 1.5
        assert _device_resolve(a[i], n)[5] == ref["chosen"]
    assert got.resolution[0] > got.resolution[1]                # the lower cutoff resolves less
    # a [C, H, W] image is the item without the batch axis; device tensors take the same way
    one = decorr(_dev(a[1]))
    assert one.resolution == got.resolution[1] and np.array_equal(one.curves, got.curves[1])


def test_decorr_maps_the_blocks_of_a_grid():
    """Two plantings on the checkerboard of a 2 x 2 grid of 64-blocks: pool="block" recovers each where it lies."""
    from pssr2_amd.util import decorr
    n, r0 = 64, ((10, 20), (20, 10))
    a = np.block([[D.planted(n, r0[i][j], 30 + 2 * i + j) for j in range(2)] for i in range(2)])
    assert a.shape == (128, 128)
    got = decorr(a, block=n, pool="block")
    assert got.resolution.shape == got.peak.shape == (2, 2) and got.found.all() and got.curves.shape == (2, 2, 11, 33)
    ref = D.rings_ref(a[None], n)
    for i in range(2):
        for j in range(2):
            want = D.resolve_ref(ref[0, 2 * i + j], n)
            assert abs(got.peak[i, j] - want["peak"]) <= 1e-3 and r0[i][j] <= got.peak[i, j] <= r0[i][j] + 1.5
            assert got.resolution[i, j] == pytest.approx(n / got.peak[i, j], rel=1e-15)
    batch = decorr(np.stack([a, a[::-1].copy()])[:, None], block=n, pool="block")
    assert batch.resolution.shape == (2, 2, 2) and np.array_equal(batch.resolution[0], got.resolution)
    whole = decorr(a, block=n)                                   # pooled: one figure
    assert isinstance(whole.resolution, float) and whole.curves.shape == (11, 33)


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


@pytest.mark.parametrize("norm", [False, True])
def test_test_metrics_decorr(norm):
    from pssr2_amd.predict import predict_images, test_metrics
    from pssr2_amd.util import decorr
    ds = _Pairs()
    default = test_metrics(_Positional(), ds, device="cuda", metrics=("psnr",), norm=norm, avg=False)
    got = test_metrics(_Positional(), ds, device="cuda", metrics=("psnr", "decorr"), norm=norm, avg=False)
    pred = predict_images(_Positional(), ds, device="cuda", batch_size=1, out_dir=None)["img0"]
    want = decorr(pred)
    assert want.block == 48 and math.isfinite(want.resolution) and want.resolution >= 2.0
    assert got == {"psnr": default["psnr"], "decorr": [want.resolution] * 2}          # every iteration: dataset[0]; before norm
    assert test_metrics(_Positional(), ds, device="cuda", metrics="decorr", norm=norm) == {"decorr": want.resolution}
    got8 = test_metrics(_Positional(), ds, device="cuda", metrics=("decorr",), norm=norm, avg=False, ensemble=8)
    pred8 = predict_images(_Positional(), ds, device="cuda", batch_size=1, out_dir=None, ensemble=8)["img0"]
    assert got8 == {"decorr": [decorr(pred8).resolution] * 2}
