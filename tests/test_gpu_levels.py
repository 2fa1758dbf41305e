"""The noise measurement on the device: ops.level_moments_u8 against the numpy restatement of tests/_levels_ref.py (integers: every
comparison of a table is ==), util.estimate_noise against the restatement of the whole (integers equal, floats within 1e-12), its
warnings, and one statistical check on the device's own noise generator."""
import warnings

import numpy as np
import pytest
import torch

import _levels_ref as R
import _rsf_ref as F

pytestmark = pytest.mark.gpu

PLANES_CAP = 1024                             # grid.y of the kernel: planes beyond it take the stride loop


def _case(d, l, want=None):
    from pssr2_amd import ops
    got = ops.level_moments_u8(torch.tensor(d).cuda(), torch.tensor(l).cuda())
    assert got.dtype == torch.int64 and got.shape == (d.shape[0], 256, 5) and got.is_cuda
    if want is None:
        want = R.table_ref(d, l)
    assert torch.equal(got.cpu(), torch.as_tensor(np.asarray(want, dtype=np.int64)))
    return got


def _constant(planes, n, v, x):
    """The table of constant planes in closed form."""
    want = np.zeros((planes, 256, 5), dtype=np.int64)
    want[:, v] = [n, n * x, n * x * x, n * (x == 0), n * (x == 255)]
    return want


# ------------------------------------------------------------------------------------------------ the table
@pytest.mark.parametrize("per_plane", [1, 15, 16, 17, 63, 65, 4097])
def test_table_at_every_start_address(per_plane):
    """Three planes of an odd size: the later ones start at every address modulo 16 as the sizes go by."""
    rng = np.random.default_rng(per_plane)
    _case(rng.integers(0, 256, size=(3, per_plane), dtype=np.uint8), rng.integers(0, 256, size=(3, per_plane), dtype=np.uint8))


def test_table_of_offset_views():
    """Both stacks at every byte offset of a buffer (pieces that straddle the buffer's ends, the shift inside), and the two at different
    offsets, where no 16-byte piece is aligned in both."""
    from pssr2_amd import ops
    rng = np.random.default_rng(1)
    planes, n = 3, 1237
    d, l = rng.integers(0, 256, size=(planes, n), dtype=np.uint8), rng.integers(0, 256, size=(planes, n), dtype=np.uint8)
    want = torch.as_tensor(R.table_ref(d, l))

    def view(a, off, pad):
        buf = torch.full((a.size + 16 + pad,), 255, dtype=torch.uint8, device="cuda")
        buf[off:off + a.size] = torch.tensor(a.reshape(-1)).cuda()
        v = buf[off:off + a.size].view(planes, n)
        assert v.data_ptr() % 16 == off and v.is_contiguous()
        return v

    for od, ol in [(o, o) for o in range(16)] + [(0, 1), (3, 11), (15, 0), (8, 9)]:
        for pad in (0, 5):                                     # the last piece ends with the buffer, or inside it
            assert torch.equal(ops.level_moments_u8(view(d, od, pad), view(l, ol, pad)).cpu(), want), (od, ol, pad)


def test_table_with_every_level_present():
    rng = np.random.default_rng(2)
    d = np.tile(np.arange(256, dtype=np.uint8), (2, 40))
    for l in (rng.integers(0, 256, size=d.shape, dtype=np.uint8), np.zeros_like(d), np.full_like(d, 255)):
        got = _case(d, l)
        assert got[..., 0].eq(40).all()


def test_table_of_constant_planes():
    """A constant plane puts every lane of every wave on one level; 300 x 300 pixels of 255 pass 2^32 in sum L^2 of a plane."""
    n = 300 * 300
    assert n * 255 * 255 > 1 << 32
    _case(np.full((1, 300, 300), 255, dtype=np.uint8), np.full((1, 300, 300), 255, dtype=np.uint8), _constant(1, n, 255, 255))
    _case(np.zeros((2, 300, 300), dtype=np.uint8), np.zeros((2, 300, 300), dtype=np.uint8), _constant(2, n, 0, 0))
    _case(np.full((1, 300, 300), 7, dtype=np.uint8), np.full((1, 300, 300), 255, dtype=np.uint8), _constant(1, n, 7, 255))
    flat = np.full((1, 5, 5), 7, dtype=np.uint8)               # ... which the restatement says too
    assert R.table_ref(flat, np.full_like(flat, 255)).tolist() == _constant(1, 25, 7, 255).tolist()


def test_table_over_many_workgroups():
    from pssr2_amd import _lib
    assert _lib.lib().pssr_level_moments_workspace_bytes(1, 512 * 512) > 8 * 256 * 5 * 8         # more than eight partial rows to fold
    rng = np.random.default_rng(3)
    _case(rng.integers(0, 256, size=(1, 512, 512), dtype=np.uint8), rng.integers(0, 256, size=(1, 512, 512), dtype=np.uint8))
    _case(rng.integers(0, 256, size=(2, 301, 317), dtype=np.uint8), rng.integers(0, 256, size=(2, 301, 317), dtype=np.uint8))


def test_table_of_more_planes_than_the_grid():
    rng = np.random.default_rng(4)
    planes = PLANES_CAP + 1
    _case(rng.integers(0, 256, size=(planes, 16, 16), dtype=np.uint8), rng.integers(0, 256, size=(planes, 16, 16), dtype=np.uint8))


def test_table_of_non_contiguous_inputs_and_the_same_bits_on_every_run():
    from pssr2_amd import ops
    rng = np.random.default_rng(5)
    d, l = rng.integers(0, 256, size=(3, 128, 130), dtype=np.uint8), rng.integers(0, 256, size=(3, 128, 130), dtype=np.uint8)
    td, tl = torch.tensor(d).cuda(), torch.tensor(l).cuda()
    first = ops.level_moments_u8(td, tl)
    assert all(torch.equal(ops.level_moments_u8(td, tl), first) for _ in range(3))
    got = ops.level_moments_u8(td[:, ::2, 1:], tl[:, ::2, 1:])                                   # made contiguous, as the neighbouring ops do
    assert torch.equal(got.cpu(), torch.as_tensor(R.table_ref(np.ascontiguousarray(d[:, ::2, 1:]), np.ascontiguousarray(l[:, ::2, 1:]))))
    got = ops.level_moments_u8(td.transpose(1, 2), tl.transpose(1, 2))
    assert torch.equal(got, first)
    for bad in ((td, tl[:, :-1]), (td.float(), tl), (td.cpu(), tl), (td[:0], tl[:0]), (td[:, :0], tl[:, :0])):
        with pytest.raises(ValueError):
            ops.level_moments_u8(*bad)


# ------------------------------------------------------------------------------------------------ estimate_noise
def _same_noise(got, want, on_device=False):
    from pssr2_amd.util import Noise
    assert type(got) is Noise
    table = got.table.cpu().numpy() if on_device else got.table
    assert torch.is_tensor(got.table) == on_device and table.dtype == np.int64
    np.testing.assert_array_equal(table, want["table"])
    for name in R.FIELDS[:8] + ("sigma",):
        a, b = np.asarray(getattr(got, name)), np.asarray(want[name])
        assert a.dtype == np.float64 and a.shape == b.shape and np.abs(a - b).max(initial=0.0) <= 1e-12, (name, a, b)
    assert np.asarray(got.levels).tolist() == np.asarray(want["levels"]).tolist() and np.asarray(got.found).tolist() == np.asarray(want["found"]).tolist()
    assert got.margin == want["margin"]


def _scale_one_pair(n_img, c_hr, c_lr, planting, seed):
    """HR items of the scene and LR items whose centre frames are the planted noise model of them (the other frames are random)."""
    rng = np.random.default_rng(seed)
    hr = R.scene(n_img * c_hr, 64, 64, seed).reshape(n_img, c_hr, 64, 64)
    lr = rng.integers(0, 256, size=(n_img, c_lr, 64, 64), dtype=np.uint8)
    first = c_lr // 2 - c_hr // 2
    lr[:, first:first + c_hr] = R.plant(hr, *planting, seed)
    return lr, hr


@pytest.mark.parametrize("c_hr,c_lr", [(1, 1), (3, 3), (1, 3)])
def test_estimate_noise_at_scale_one(c_hr, c_lr):
    from pssr2_amd.util import estimate_noise
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        for k, planting in enumerate(R.PLANTINGS):
            lr, hr = _scale_one_pair(2, c_hr, c_lr, planting, 10 + k)
            np.testing.assert_array_equal(R.pair_ref(lr, hr)[0], hr)                             # at scale 1 the reduction is the identity
            want = R.estimate_ref(lr, hr)
            got = estimate_noise(lr, hr)
            _same_noise(got, want)
            assert got.found is True and type(got.poisson) is float and type(got.levels) is int and got.sigma == 0.0 and got.margin == 0
            _same_noise(estimate_noise(torch.tensor(lr).cuda(), torch.tensor(hr).cuda(), to_numpy=False), want, on_device=True)
            per_item = R.estimate_ref(lr, hr, pool="item", min_count=8, guard=3.0)
            got = estimate_noise(lr, torch.tensor(hr).cuda(), pool="item", min_count=8, guard=3.0)
            _same_noise(got, per_item)
            assert got.poisson.shape == (2,) and got.table.shape == (2, 256, 5) and got.found.dtype == bool and got.levels.dtype == np.int64
            _same_noise(estimate_noise(lr, hr, pool="item", min_count=8, guard=3.0, to_numpy=False), per_item, on_device=True)
            one = estimate_noise(lr[1], hr[1], pool="item", min_count=8, guard=3.0)                 # one pair without the batch axis
            assert one.table.shape == (256, 5) and type(one.gain) is float and abs(one.gain - per_item["gain"][1]) <= 1e-12
            assert one.table.tolist() == per_item["table"][1].tolist()


@pytest.mark.parametrize("rsf", [None, 1.0, "fit"])
def test_estimate_noise_at_scale_four(rsf):
    from pssr2_amd.util import estimate_noise, estimate_rsf
    rng = np.random.default_rng(20)
    rows, radius = F.table(4, F.DEFAULT_SIGMAS)
    planted = [8, 20] if rsf == "fit" else ([4, 4] if rsf else [0, 0])                            # sigma 2 and 5; 1; none
    hat, lr = F.planted_pair(rng, 2, 1, 3, 30, 32, 4, rows, radius, planted)
    hat = np.repeat(np.repeat(hat[..., ::8, ::8], 8, axis=-2), 8, axis=-1)                        # coarse texture: the widths differ visibly
    for i, k in enumerate(planted):
        lr[i, 1:2, 7:-7, 7:-7] = F.reduce_k(hat[i], rows[k], 4, radius)
    lr = R.plant(lr, 0.3, 1, 2, 0, 21)
    want = R.estimate_ref(lr, hat, rsf, min_count=4)
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = estimate_noise(lr, hat, rsf=rsf, min_count=4)
        _same_noise(got, want)
        _same_noise(estimate_noise(lr, hat, rsf=rsf, pool="item", min_count=4), R.estimate_ref(lr, hat, rsf, pool="item", min_count=4))
        if rsf is None:
            assert (got.sigma, got.margin) == (0.0, 0) and got.table[:, 0].sum() == 2 * 30 * 32
            return
        found = estimate_rsf(lr, hat, sigmas=None if rsf == "fit" else [rsf])
    assert got.margin == found.margin == (7 if rsf == "fit" else 2) and got.sigma == found.sigma.mean()
    assert found.sigma.tolist() == ([2.0, 5.0] if rsf == "fit" else [1.0, 1.0])
    assert got.table[:, 0].sum() == 2 * (30 - 2 * got.margin) * (32 - 2 * got.margin)
    if rsf == "fit":                                           # one width per item, as consistency_map(rsf=...) takes them: R = 15, m = 5
        given = estimate_noise(lr, hat, rsf=[2.0, 5.0], min_count=4)
        _same_noise(given, R.estimate_ref(lr, hat, [2.0, 5.0], min_count=4))
        assert (given.sigma, given.margin) == (3.5, 5)


def test_estimate_noise_warns():
    from pssr2_amd.util import estimate_noise
    flat = np.zeros((2, 1, 8, 8), dtype=np.uint8)
    with pytest.warns(UserWarning, match="the pooled batch"):
        got = estimate_noise(flat, flat)
    assert got.found is False and got.levels == 0 and (got.poisson, got.gaussian, got.gain, got.saltpepper, got.alpha) == (0.0,) * 5
    assert got.table[0].tolist() == [128, 0, 0, 128, 0] and got.crappifier().crappifiers == ()
    lr, hr = _scale_one_pair(2, 1, 1, (0, 0, 2, 0), 30)
    lr[1], hr[1] = 255, 255
    with pytest.warns(UserWarning, match=r"item\(s\) \[1\]"):
        got = estimate_noise(lr, hr, pool="item")
    assert got.found.tolist() == [True, False]
    _same_noise(got, R.estimate_ref(lr, hr, pool="item"))
    with pytest.warns(UserWarning, match="intensity scale"):
        got = estimate_noise(hr // 2, hr, pool="item")
    assert abs(got.alpha[0] - 0.5) < 0.01 and got.found.tolist() == [True, True]                # item 1: the one level 255 at a constant 127
    assert (got.levels[1], got.alpha[1], got.gain[1]) == (1, 1.0, -128.0)


def test_estimate_noise_of_the_device_generator():
    """The one statistical check on the GPU: the scene through the device crappifier path (Philox, not numpy's generator), rounded to
    uint8, is recovered within the bounds that tests/test_levels_host.py measured for this planting."""
    from pssr2_amd import AdditiveGaussian, MultiCrappifier, Poisson
    from pssr2_amd.data import DevicePairGenerator
    from pssr2_amd.util import estimate_noise
    from test_levels_host import WORST
    hr = torch.tensor(R.scene(8, 64, 64, 1)).cuda().view(8, 1, 64, 64)
    _, lr = DevicePairGenerator(lr_scale=1, crappifier=MultiCrappifier(Poisson(0.5, 3), AdditiveGaussian(4)), seed=5)(hr)
    lr8 = lr.to(torch.uint8)
    assert torch.equal(lr8.float(), lr)                        # the generator's last stage rounds and clips
    got = estimate_noise(lr8, hr)
    bound = WORST[(0.5, 3, 4, 0)]
    print(got[:10])
    assert got.found and got.levels >= 150
    assert abs(got.poisson - 0.5) <= 2 * bound["poisson"] and abs(got.gain - 3) <= 2 * bound["gain"] and abs(got.gaussian - 4) <= 2 * bound["gaussian"]
    c = got.crappifier().crappifiers
    assert [type(s).__name__ for s in c] == ["Poisson", "AdditiveGaussian"] and (c[0].intensity, c[0].gain, c[1].intensity) == (got.poisson, got.gain, got.gaussian)
