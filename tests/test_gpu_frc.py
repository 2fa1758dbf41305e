"""Fourier ring correlation on the device (csrc/frc.hip through ops.frc_rings_u8, util.frc and test_metrics) against the numpy restatement
of tests/_frc_ref.py.  The bound on the ring sums is |S - S_ref| <= TOL[n] sqrt(Saa_ref Sbb_ref) per ring, TOL[n] = 8 x the error of the
float32 numpy restatement on the same inputs (measured on the CPU, recorded in _frc_ref.py)."""
import functools
import math

import numpy as np
import pytest
import torch

import _frc_ref as F

pytestmark = pytest.mark.gpu


def _dev(x):
    return torch.from_numpy(np.ascontiguousarray(x)).cuda()


def _rings(a, b, n, name="hann"):
    from pssr2_amd import ops
    got = ops.frc_rings_u8(_dev(a), _dev(b), n, name)
    assert got.dtype == torch.float64 and got.is_cuda
    return got.cpu().numpy()


def _worst(got, ref):
    """max over rings and the three sums of |S - S_ref| / sqrt(Saa_ref Sbb_ref)."""
    assert got.shape == ref.shape
    return float((np.abs(got - ref) / F.scale_of(ref)[..., None]).max())


@functools.lru_cache(maxsize=None)
def _case(n):
    return [(a, b, name, F.rings_ref(a, b, n, name)) for a, b, name in F.sums_inputs(n)]


# ------------------------------------------------------------------------------------------------ ring sums
@pytest.mark.parametrize("n", F.SUMS_SIZES + F.BIG_SIZES)
def test_ring_sums_against_the_float64_fft(n):
    """16: the minimum; 18, 30, 34: no multiples of an MFMA tile or of the K step, n/2 + 1 = 10, 16, 18; 64, 66: two 32-tiles exactly and just
    over; 130: several LDS stages; 500 (the reference tests' CROP_RES) and 1024 once, one plane.  White noise and a planted pair, both
    windows: power in every ring."""
    for a, b, name, ref in _case(n):
        assert (F.scale_of(ref) > 0).all()
        got = _rings(a, b, n, name)
        worst = _worst(got, ref)
        print(f"n={n} {name}: max |S - S_ref| / sqrt(Saa Sbb) = {worst:.3e}, bound {F.TOL[n]:.3e} (float32 numpy: {F.F32_ERROR[n]:.3e})")
        assert worst <= F.TOL[n]


@pytest.mark.parametrize("H,W,n,planes", [(40, 70, 16, 1), (40, 70, 16, 3), (37, 53, 18, 1), (37, 53, 18, 3)])
def test_blocks_of_the_centred_grid(H, W, n, planes):
    """40 x 70 at 16: 2 x 4 blocks from (4, 3); 37 x 53 at 18: 2 x 2 blocks from (0, 8), odd row pitch.  The planes start at every
    address modulo 16 in turn."""
    from pssr2_amd import ops
    rng = np.random.default_rng(H + planes)
    a, b = (rng.integers(0, 256, size=(planes, H, W), dtype=np.uint8) for _ in range(2))
    nby, nbx, _, _ = F.grid(H, W, n)
    ref = F.rings_ref(a, b, n)
    assert ref.shape == (planes, nby * nbx, n // 2 + 1, 3)
    first = None
    for off in range(16):
        bufs = []
        for img in (a, b):
            flat = torch.zeros(off + img.size + 16, dtype=torch.uint8, device="cuda")
            flat[off:off + img.size] = _dev(img).reshape(-1)
            bufs.append(flat[off:off + img.size].view(planes, H, W))
        assert bufs[0].data_ptr() % 16 == off and bufs[0].is_contiguous()
        got = ops.frc_rings_u8(bufs[0], bufs[1], n).cpu().numpy()
        assert _worst(got, ref) <= F.TOL[n]
        first = got if first is None else first
        np.testing.assert_array_equal(got, first)               # where the bytes lie changes nothing


def test_more_planes_than_a_grid_axis_of_the_plane_kernels():
    """1100 planes of 16 x 16 (more than U8_PLANES_CAP = 1024), every one with its own content."""
    rng = np.random.default_rng(11)
    a, b = (rng.integers(0, 256, size=(1100, 16, 16), dtype=np.uint8) for _ in range(2))
    got = _rings(a, b, 16)
    assert got.shape == (1100, 1, 9, 3)
    assert _worst(got, F.rings_ref(a, b, 16)) <= F.TOL[16]


def test_a_call_that_works_its_blocks_off_in_chunks():
    """116 blocks of 512 x 512 need more than the 256 MB of workspace that a chunk of blocks may take (2.35 MB a block: 114 fit): the
    call launches twice, and every block's sums are what a call of its own gives, bit for bit."""
    from pssr2_amd import _lib, ops
    gen = torch.Generator(device="cuda").manual_seed(5)
    a = torch.randint(0, 256, (116, 512, 512), dtype=torch.uint8, device="cuda", generator=gen)
    b = torch.randint(0, 256, (116, 512, 512), dtype=torch.uint8, device="cuda", generator=gen)
    lib = _lib.lib()
    assert lib.pssr_frc_workspace_bytes(116, 512, 512, 512) < 116 * (lib.pssr_frc_workspace_bytes(1, 512, 512, 512))
    whole = ops.frc_rings_u8(a, b, 512)
    assert whole.shape == (116, 1, 257, 3)
    for lo, hi in ((0, 1), (57, 60), (113, 116)):
        assert torch.equal(whole[lo:hi], ops.frc_rings_u8(a[lo:hi], b[lo:hi], 512))


def test_non_contiguous_inputs_and_leading_dimensions():
    from pssr2_amd import ops
    rng = np.random.default_rng(12)
    wide = _dev(rng.integers(0, 256, size=(2, 3, 36, 80), dtype=np.uint8))
    a, b = wide[..., ::2], wide[..., 1::2]
    assert not a.is_contiguous() and not b.is_contiguous()
    got = ops.frc_rings_u8(a, b, 18)
    assert got.shape == (6, 4, 10, 3)
    assert torch.equal(got, ops.frc_rings_u8(a.contiguous().reshape(6, 36, 40), b.contiguous().reshape(6, 36, 40), 18))
    assert _worst(got.cpu().numpy(), F.rings_ref(a.cpu().numpy().reshape(6, 36, 40), b.cpu().numpy().reshape(6, 36, 40), 18)) <= F.TOL[18]


def test_ops_check_device_tensors_too():
    """The checks of ops.frc_rings_u8 that a host tensor never reaches."""
    from pssr2_amd import ops
    t = torch.zeros(2, 32, 48, dtype=torch.uint8, device="cuda")
    for a, b in ((t, t[:1]), (t, t[..., :32]), (t, t.float()), (t.short(), t.short()), (t[0, 0], t[0, 0]), (t, t.cpu())):
        with pytest.raises(ValueError, match="uint8 device tensors"):
            ops.frc_rings_u8(a, b, 16)
    for bad in (14, 17, 31, 1026, 16.0, True):
        with pytest.raises(ValueError, match="block must be"):
            ops.frc_rings_u8(t, t, bad)
    for bad in (34, 48):                                        # even and in range, larger than the smaller side
        with pytest.raises(ValueError, match="does not fit"):
            ops.frc_rings_u8(t, t, bad)
    with pytest.raises(ValueError, match="window"):
        ops.frc_rings_u8(t, t, 16, "hamming")
    with pytest.raises(ValueError, match="at least one plane"):
        ops.frc_rings_u8(t[:0], t[:0], 16)
    assert ops.frc_rings_u8(t, t, 32).shape == (2, 1, 17, 3)


# ------------------------------------------------------------------------------------------------ properties without a measured tolerance
@pytest.mark.parametrize("n", (18, 64, 130))
def test_two_calls_give_the_same_bits(n):
    from pssr2_amd import ops
    a, b, name, _ = _case(n)[0]
    a, b = _dev(np.tile(a, (3, 2, 2))), _dev(np.tile(b, (3, 2, 2)))
    first = ops.frc_rings_u8(a, b, n, name)
    for _ in range(3):
        assert torch.equal(ops.frc_rings_u8(a, b, n, name), first)


def test_an_all_zero_pair_is_exactly_zero():
    from pssr2_amd.util import frc
    z = np.zeros((2, 34, 50), dtype=np.uint8)
    got = _rings(z, z, 18, "none")
    assert got.shape == (2, 2, 10, 3) and not got.any() and not np.signbit(got).any()
    res = frc(z, z, block=18)
    assert np.array_equal(res.curve, np.zeros(10)) and res.crossed is True and res.resolution == 18.0


@pytest.mark.parametrize("n", (18, 64))
def test_a_constant_image_has_its_power_in_ring_zero(n):
    """Under "none" the transform of a constant is its sum at the origin and nothing elsewhere."""
    c = np.full((1, n, n), 255, dtype=np.uint8)
    got = _rings(c, c, n, "none")[0, 0]
    assert got[0, 1] == pytest.approx((255.0 * n * n) ** 2, rel=1e-5)
    assert (np.abs(got[1:]) <= F.TOL[n] * got[0, 1]).all()


@pytest.mark.parametrize("n", (16, 34, 130))
def test_an_image_against_itself_correlates_fully(n):
    from pssr2_amd.util import frc
    a = _case(n)[0][0]
    res = frc(a, a, block=n)
    assert res.curve.shape == (n // 2 + 1,) and np.abs(res.curve - 1).max() <= 1e-6
    assert res.crossed is False and res.resolution == 2.0 and res.block == n
    np.testing.assert_array_equal(res.freq, np.arange(n // 2 + 1) / n)


@pytest.mark.parametrize("n", (18, 66))
def test_swapping_the_images_swaps_their_power(n):
    for a, b, name, ref in _case(n):
        ab, ba = _rings(a, b, n, name), _rings(b, a, n, name)
        bound = F.TOL[n] * F.scale_of(ref)
        assert (np.abs(ab[..., 1] - ba[..., 2]) <= bound).all() and (np.abs(ab[..., 2] - ba[..., 1]) <= bound).all()
        assert (np.abs(ab[..., 0] - ba[..., 0]) <= bound).all()


# ------------------------------------------------------------------------------------------------ util.frc
PLANTED = ((64, 12), (128, 24), (250, 40))
# Each of the three sums of a ring lies within TOL[n] sqrt(Saa Sbb) of the reference, so Sab / sqrt(Saa Sbb) moves by at most about
# (1 + |frc|) TOL[n] <= 2 TOL[n]; pooling planes, blocks or rings adds bounds and scales alike.  Every block side used below is at most 500.
CURVE_TOL = 2 * F.TOL[500]


@pytest.mark.parametrize("n,r0", PLANTED)
def test_frc_finds_the_planted_cutoff(n, r0):
    """|r*_device - r*_ref| <= 1e-3 rings: the curve is off by about 1e-6 and falls by more than 0.1 per ring at the crossing
    (tests/test_frc_host.py guards that premise)."""
    from pssr2_amd.util import FRC, frc
    a, b = F.planted_pair(n, r0, 0)
    curve, r_star, resolution, crossed = F.curve_ref(F.rings_ref(a[None], b[None], n), n)
    assert crossed and r0 < r_star <= r0 + 5
    for make in (lambda x: x, _dev):
        for to_numpy in (True, False):
            got = frc(make(a), make(b), to_numpy=to_numpy)
            assert isinstance(got, FRC) and got.block == n and got.crossed is True
            got_curve = got.curve if to_numpy else got.curve.cpu().numpy()
            assert (isinstance(got.curve, np.ndarray) if to_numpy else got.curve.is_cuda) and got_curve.shape == (n // 2 + 1,)
            assert abs(n / got.resolution - r_star) <= 1e-3
            assert np.abs(got_curve - curve).max() <= CURVE_TOL
    # the pixel size scales the answer, nothing else
    scaled = frc(a, b, pixel_size=32.5)
    assert scaled.resolution == pytest.approx(32.5 * frc(a, b).resolution, rel=1e-15) and np.array_equal(scaled.curve, frc(a, b).curve)
    # pooled rings: the restatement on the reference sums
    curve2, r_star2, _, _ = F.curve_ref(F.rings_ref(a[None], b[None], n), n, smooth=2)
    got = frc(a, b, smooth=2)
    assert np.abs(got.curve - curve2).max() <= CURVE_TOL and abs(n / got.resolution - r_star2) <= 1e-3
    # another threshold
    _, r_half, _, _ = F.curve_ref(F.rings_ref(a[None], b[None], n), n, threshold=0.5)
    assert abs(n / frc(a, b, threshold=0.5).resolution - r_half) <= 1e-3


@pytest.mark.parametrize("c", (1, 3))
def test_frc_pools_the_planes_of_an_item(c):
    from pssr2_amd.util import frc
    n, r0s = 64, (12, 20)
    pairs = [[F.planted_pair(n, r0, 10 * i + j) for j in range(c)] for i, r0 in enumerate(r0s)]
    a = np.stack([np.stack([p[0] for p in item]) for item in pairs])
    b = np.stack([np.stack([p[1] for p in item]) for item in pairs])
    assert a.shape == (2, c, n, n)
    got = frc(a, b)
    assert got.curve.shape == (2, n // 2 + 1) and got.resolution.shape == (2,) and got.crossed.dtype == bool and got.crossed.all()
    for i in range(2):
        curve, r_star, _, _ = F.curve_ref(F.rings_ref(a[i], b[i], n), n)
        assert np.abs(got.curve[i] - curve).max() <= CURVE_TOL and abs(n / got.resolution[i] - r_star) <= 1e-3
    assert got.resolution[0] > got.resolution[1]                # the lower cutoff resolves less
    # a [C, H, W] pair is the item without the batch axis; device tensors take the same way
    one = frc(_dev(a[1]), _dev(b[1]))
    assert one.resolution == got.resolution[1] and np.array_equal(one.curve, got.curve[1])


def test_frc_pools_the_blocks_of_a_plane():
    from pssr2_amd.util import frc
    rng = np.random.default_rng(13)
    low = rng.integers(0, 256, size=(10, 18), dtype=np.uint8).repeat(4, axis=0).repeat(4, axis=1)          # 40 x 72, blocky: low-pass
    a = np.clip(low[:, :70] + rng.integers(0, 9, size=(40, 70)), 0, 255).astype(np.uint8)
    b = np.clip(low[:, :70] + rng.integers(0, 9, size=(40, 70)), 0, 255).astype(np.uint8)
    got = frc(a, b, block=16)
    curve, r_star, resolution, crossed = F.curve_ref(F.rings_ref(a[None], b[None], 16), 16)
    assert got.block == 16 and got.crossed == crossed and np.abs(got.curve - curve).max() <= CURVE_TOL
    assert got.resolution == pytest.approx(resolution, rel=1e-3)
    assert frc(a, b).block == 40                                # the default: the largest even side that fits


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
def test_test_metrics_frc(norm):
    from pssr2_amd.predict import predict_images, test_metrics
    from pssr2_amd.util import frc
    ds = _Pairs()
    default = test_metrics(_Positional(), ds, device="cuda", metrics=("psnr",), norm=norm, avg=False)
    got = test_metrics(_Positional(), ds, device="cuda", metrics=("psnr", "frc"), norm=norm, avg=False)
    pred = predict_images(_Positional(), ds, device="cuda", batch_size=1, out_dir=None)["img0"]
    want = frc(pred, ds.hrs[0][:, :48, :48])
    assert want.block == 48 and math.isfinite(want.resolution) and want.resolution >= 2.0
    assert got == {"psnr": default["psnr"], "frc": [want.resolution] * 2}           # every iteration: dataset[0]; before norm
    assert test_metrics(_Positional(), ds, device="cuda", metrics="frc", norm=norm) == {"frc": want.resolution}
    got8 = test_metrics(_Positional(), ds, device="cuda", metrics=("frc",), norm=norm, avg=False, ensemble=8)
    pred8 = predict_images(_Positional(), ds, device="cuda", batch_size=1, out_dir=None, ensemble=8)["img0"]
    assert got8 == {"frc": [frc(pred8, ds.hrs[0][:, :48, :48]).resolution] * 2}
