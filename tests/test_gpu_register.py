"""Registration of real pairs on the device: the fused shift-search kernel and the crop kernel against the numpy restatement of
tests/_register_ref.py, util.register_pairs on planted shifts, and the ``register=`` keyword of the three tile-pair datasets.  Everything is
integer arithmetic on the same bytes, and the choice is made from the same integers, so every comparison is with ==."""
import random
import warnings

import numpy as np
import pytest
import torch

import _register_ref as R

pytestmark = pytest.mark.gpu

SCALES = (1, 2, 3, 4, 8, 16)
INNER = ((1, 1), (5, 65), (33, 40))           # h' x w': one output, a wide strip over several blocks, blocks with remainders on both axes
PLANES_CAP = 1024                             # grid.y of the kernels: planes beyond it take the stride loop


def _sums_case(hr, lr, radius):
    from pssr2_amd import ops
    got = ops.register_shifts_u8(torch.tensor(hr).cuda(), torch.tensor(lr).cuda(), radius)
    planes = lr.size // (lr.shape[-1] * lr.shape[-2])
    assert got.dtype == torch.int64 and got.shape == (planes, 3 * (2 * radius + 1) ** 2 + 2)
    want = R.sums_ref(hr.reshape(-1, *hr.shape[-2:]), lr.reshape(-1, *lr.shape[-2:]), radius)
    assert got.cpu().tolist() == want
    return want


def _sizes_case(s, radius, rng):
    m = R.margin(s, radius)
    for hc, wc in INNER:
        h, w = hc + 2 * m, wc + 2 * m
        for planes in (1, 3):
            _sums_case(rng.integers(0, 256, size=(planes, s * h, s * w), dtype=np.uint8), rng.integers(0, 256, size=(planes, h, w), dtype=np.uint8),
                       radius)
        for v in (0, 255):
            want = _sums_case(np.full((1, s * h, s * w), v, dtype=np.uint8), np.full((1, h, w), v, dtype=np.uint8), radius)
            n = hc * wc
            assert want[0] == [v * n, v * v * n, v * v * n] * (2 * radius + 1) ** 2 + [v * n, v * v * n]


# ------------------------------------------------------------------------------------------------ the sums table
@pytest.mark.parametrize("radius", [0, 1, 3, 8])
@pytest.mark.parametrize("s", SCALES)
def test_sums_match_the_restatement(s, radius):
    _sizes_case(s, radius, np.random.default_rng(100 * s + radius))


def test_sums_at_the_largest_radius():
    _sizes_case(4, 32, np.random.default_rng(32))


def test_sums_when_a_workgroup_walks_several_blocks():
    """128 planes leave 32 workgroups to a plane, and a 163 x 163 window has 36 blocks of 32 x 32 outputs: every workgroup takes two, and
    adds the second into the slots the first one wrote."""
    rng = np.random.default_rng(1)
    s, radius, planes = 2, 1, 128
    h = w = 163 + 2 * R.margin(s, radius)
    _sums_case(rng.integers(0, 256, size=(planes, s * h, s * w), dtype=np.uint8), rng.integers(0, 256, size=(planes, h, w), dtype=np.uint8), radius)
    # ... and shifts that outnumber the threads (R = 32: 4226 work items, 17 per thread): the partial rows are large, which leaves 20
    # workgroups to each of 32 planes, and a 33 x 120 window has 24 blocks of 16 x 16 outputs
    s, radius, planes = 4, 32, 32
    h, w = 33 + 2 * R.margin(s, radius), 120 + 2 * R.margin(s, radius)
    _sums_case(rng.integers(0, 256, size=(planes, s * h, s * w), dtype=np.uint8), rng.integers(0, 256, size=(planes, h, w), dtype=np.uint8), radius)


def test_sums_with_more_partial_rows_than_the_fold_has_threads():
    """One plane, s = 1, radius 0 (m = 1): a 544 x 544 window is 17 x 17 blocks of 32 x 32 outputs, one per workgroup, so the fold adds
    289 partial rows of 3 T + 2 = 5 sums.  The workspace is the tap table (128 bytes) and one such row per workgroup and plane."""
    from pssr2_amd import _lib
    rows = (_lib.lib().pssr_register_shifts_workspace_bytes(1, 546, 546, 1, 0) - 128) // (8 * 5)
    assert rows > 256
    rng = np.random.default_rng(5)
    _sums_case(rng.integers(0, 256, size=(1, 546, 546), dtype=np.uint8), rng.integers(0, 256, size=(1, 546, 546), dtype=np.uint8), 0)


def test_sums_leading_dimensions_and_odd_addresses():
    """[N, C, ...] inputs, and an HR buffer that starts at every address modulo 4 (the 16-byte staging must fall back to bytes at the
    buffer's ends and shift inside it)."""
    from pssr2_amd import ops
    rng = np.random.default_rng(2)
    hr, lr = rng.integers(0, 256, size=(2, 3, 27, 39), dtype=np.uint8), rng.integers(0, 256, size=(2, 3, 9, 13), dtype=np.uint8)
    want = _sums_case(hr, lr, 3)
    for off in range(1, 5):
        buf = torch.full((hr.size + 8,), 255, dtype=torch.uint8, device="cuda")
        buf[off:off + hr.size] = torch.tensor(hr.reshape(-1)).cuda()                        # hr at byte offset `off` of the buffer
        view = buf[off:off + hr.size].view(2, 3, 27, 39)
        assert view.data_ptr() % 4 == off % 4 and view.is_contiguous()
        assert ops.register_shifts_u8(view, torch.tensor(lr).cuda(), 3).cpu().tolist() == want
    # a plane that is the whole buffer: the first and the last piece of every block's rows are the buffer's ends
    for s, radius in ((1, 0), (2, 2)):
        m = R.margin(s, radius)
        _sums_case(rng.integers(0, 256, size=(1, s * (3 + 2 * m), s * (3 + 2 * m)), dtype=np.uint8),
                   rng.integers(0, 256, size=(1, 3 + 2 * m, 3 + 2 * m), dtype=np.uint8), radius)


def test_sums_more_planes_than_the_grid():
    rng = np.random.default_rng(3)
    planes = PLANES_CAP + 1
    _sums_case(rng.integers(0, 256, size=(planes, 6, 6), dtype=np.uint8), rng.integers(0, 256, size=(planes, 3, 3), dtype=np.uint8), 0)
    _sums_case(rng.integers(0, 256, size=(planes, 10, 12), dtype=np.uint8), rng.integers(0, 256, size=(planes, 5, 6), dtype=np.uint8), 1)


def test_sums_pass_32_bits():
    want = _sums_case(np.full((1, 302, 302), 255, dtype=np.uint8), np.full((1, 302, 302), 255, dtype=np.uint8), 0)
    assert want[0] == [90000 * 255, 90000 * 255 * 255, 90000 * 255 * 255, 90000 * 255, 90000 * 255 * 255] and want[0][1] > 1 << 32


def test_sums_are_the_same_bits_on_every_run():
    from pssr2_amd import ops
    rng = np.random.default_rng(4)
    hr = torch.tensor(rng.integers(0, 256, size=(5, 4 * 50, 4 * 61), dtype=np.uint8)).cuda()
    lr = torch.tensor(rng.integers(0, 256, size=(5, 50, 61), dtype=np.uint8)).cuda()
    first = ops.register_shifts_u8(hr, lr, 8)
    assert all(torch.equal(ops.register_shifts_u8(hr, lr, 8), first) for _ in range(3))


# ------------------------------------------------------------------------------------------------ the crop
@pytest.mark.parametrize("H,W,ho,wo", [(37, 53, 7, 16), (37, 53, 37, 53), (37, 53, 5, 13), (40, 64, 8, 32), (40, 64, 40, 48), (9, 300, 3, 272),
                                       (6, 7, 1, 1)])
def test_crop_shift_is_slicing(H, W, ho, wo):
    from pssr2_amd import ops
    rng = np.random.default_rng(H + W + ho)
    x = rng.integers(0, 256, size=(2, 3, H, W), dtype=np.uint8)
    ys, xs = [0, H - ho, (H - ho) // 2, 0, H - ho, min(1, H - ho)], [0, W - wo, (W - wo) // 2, W - wo, 0, min(16, W - wo)]
    origins = list(zip(ys, xs))                                           # both extremes on both axes, and origins of every alignment
    got = ops.crop_shift_u8(torch.tensor(x).cuda(), origins, ho, wo)
    assert got.dtype == torch.uint8 and got.shape == (2, 3, ho, wo)
    want = np.stack([p[y0:y0 + ho, x0:x0 + wo] for p, (y0, x0) in zip(x.reshape(6, H, W), origins)]).reshape(2, 3, ho, wo)
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    table = torch.tensor([(0, 0)] + origins, dtype=torch.int32).cuda()    # rows of a larger table, as register_pairs passes them
    assert torch.equal(ops.crop_shift_u8(torch.tensor(x).cuda(), np.array(origins), ho, wo, table=table[1:]), got)
    for bad in (origins[:-1], [(-1, 0)] + origins[1:], [(H - ho + 1, 0)] + origins[1:], [(0, W - wo + 1)] + origins[1:]):
        with pytest.raises(ValueError, match="origins"):
            ops.crop_shift_u8(torch.tensor(x).cuda(), bad, ho, wo)


def test_crop_shift_more_planes_than_the_grid():
    from pssr2_amd import ops
    rng = np.random.default_rng(5)
    planes = PLANES_CAP + 3
    x = rng.integers(0, 256, size=(planes, 5, 20), dtype=np.uint8)
    origins = [(int(a), int(b)) for a, b in zip(rng.integers(0, 3, size=planes), rng.integers(0, 5, size=planes))]
    got = ops.crop_shift_u8(torch.tensor(x).cuda(), origins, 3, 16).cpu().numpy()
    np.testing.assert_array_equal(got, np.stack([p[a:a + 3, b:b + 16] for p, (a, b) in zip(x, origins)]))


# ------------------------------------------------------------------------------------------------ register_pairs
def _same_registration(got, want, to_numpy=True):
    hr, lr = (got.hr, got.lr) if to_numpy else (got.hr.cpu().numpy(), got.lr.cpu().numpy())
    assert (type(got.hr) is np.ndarray) == to_numpy and hr.dtype == np.uint8 and lr.dtype == np.uint8
    np.testing.assert_array_equal(hr, want[0])
    np.testing.assert_array_equal(lr, want[1])
    assert got.shift.tolist() == want[2].tolist() and got.score.dtype == np.float64 and got.score.tolist() == want[3].tolist()
    assert got.margin == want[4]


@pytest.mark.parametrize("c_lr,c_hr", [(3, 1), (3, 3), (4, 2)])
def test_register_pairs_finds_planted_shifts(c_lr, c_hr):
    from pssr2_amd.util import register_pairs
    rng = np.random.default_rng(10 * c_lr + c_hr)
    s, radius, h, w = 2, 3, 17, 20
    planted = [(2, -1), (0, 0), (-2, 2), (1, 1)]
    hr, lr = R.planted_pair(rng, 4, c_hr, c_lr, h, w, s, radius, planted)
    want = R.register_ref(hr, lr, radius)
    assert want[2].tolist() == [list(t) for t in planted] and want[3].tolist() == [1.0] * 4
    with warnings.catch_warnings():
        warnings.simplefilter("error")                     # no shift lies on the edge of the window
        _same_registration(register_pairs(hr, lr, radius=radius), want)
        _same_registration(register_pairs(torch.tensor(hr).cuda(), torch.tensor(lr).cuda(), radius=radius, to_numpy=False), want, to_numpy=False)
        _same_registration(register_pairs(torch.tensor(hr).cuda(), lr, radius=radius), want)
        one = register_pairs(hr[2], lr[2], radius=radius)                   # one pair without the batch axis
    np.testing.assert_array_equal(one.hr, want[0][2])
    np.testing.assert_array_equal(one.lr, want[1][2])
    assert one.shift.tolist() == [-2, 2] and float(one.score) == 1.0 and one.shift.shape == (2,)
    # the aligned pair needs no shift any more
    again = register_pairs(want[0], want[1], radius=1)
    assert again.shift.tolist() == [[0, 0]] * 4


def test_register_pairs_with_noise_and_at_scale_one():
    """The LR side carries noise (scores below 1), and s = 1: a prediction against its ground truth."""
    from pssr2_amd.util import register_pairs
    rng = np.random.default_rng(7)
    for s, radius in ((4, 5), (1, 4)):
        h = w = 30
        planted = [(-5, 3), (4, 0), (1, -2)] if s == 4 else [(3, 3), (-1, 2), (0, -3)]
        hr, lr = R.planted_pair(rng, 3, 1, 1, h, w, s, radius, planted)
        lr = np.clip(lr.astype(np.int64) + rng.integers(-20, 21, size=lr.shape), 0, 255).astype(np.uint8)
        want = R.register_ref(hr, lr, radius)
        assert want[2].tolist() == [list(t) for t in planted] and all(0.0 < v < 1.0 for v in want[3])
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            _same_registration(register_pairs(hr, lr, radius=radius), want)


def test_register_pairs_warns_at_the_edge_of_the_window():
    from pssr2_amd.util import register_pairs
    rng = np.random.default_rng(8)
    hr, lr = R.planted_pair(rng, 3, 1, 1, 14, 14, 2, 2, [(0, 1), (2, 0), (-1, -2)])
    with pytest.warns(UserWarning, match=r"item\(s\) \[1, 2\]"):
        reg = register_pairs(hr, lr, radius=2)
    assert reg.shift.tolist() == [[0, 1], [2, 0], [-1, -2]]
    with warnings.catch_warnings():
        warnings.simplefilter("error")                     # radius 0 has no edge to warn about
        assert register_pairs(hr, lr, radius=0).shift.tolist() == [[0, 0]] * 3


# ------------------------------------------------------------------------------------------------ the dataset keyword
S, RADIUS, SIDE = 2, 3, 22                    # LR 22 x 22, margin 3: aligned items are 16 x 16 and 32 x 32


def _planted_stack(seed, n=5, c_hr=1, c_lr=1, noise=0):
    rng = np.random.default_rng(seed)
    planted = [(1, -2), (0, 0), (-2, 1), (2, 2), (-1, -1)][:n]
    hr, lr = R.planted_pair(rng, n, c_hr, c_lr, SIDE, SIDE, S, RADIUS, planted)
    if noise:
        lr = np.clip(lr.astype(np.int64) + rng.integers(-noise, noise + 1, size=lr.shape), 0, 255).astype(np.uint8)
    return hr, lr, planted


def _held(ds):
    return [np.asarray(x.cpu() if torch.is_tensor(x) else x) for x in (ds.hr_images, ds.lr_images)]


def _items(ds):
    return [[np.asarray(torch.as_tensor(side).cpu()) for side in ds[i]] for i in range(len(ds))]


def _check_dataset(make, hr, lr, planted):
    """``make(hr, lr, **kw)`` builds the dataset from the two stacks."""
    from pssr2_amd.util import register_pairs
    res = S * (SIDE - 2 * R.margin(S, RADIUS))
    want = register_pairs(hr, lr, radius=RADIUS)
    assert want.shift.tolist() == [list(t) for t in planted]
    ds = make(hr, lr, hr_res=res, lr_scale=S, register=RADIUS)
    held = _held(ds)
    np.testing.assert_array_equal(held[0], want.hr)
    np.testing.assert_array_equal(held[1], want.lr)
    assert ds.shifts.tolist() == want.shift.tolist() and ds.scores.tolist() == want.score.tolist() and ds.crop_res == res
    aligned = make(want.hr, want.lr, hr_res=res, lr_scale=S)
    assert aligned.shifts is None and aligned.scores is None
    for a, b in zip(_items(ds), _items(aligned)):
        assert a[0].dtype == b[0].dtype and np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1])
    # without the keyword: the stacks as they came, and items that are those bytes (val_split=1: no rotation is drawn)
    plain = make(hr, lr, hr_res=S * SIDE, lr_scale=S)
    held = _held(plain)
    np.testing.assert_array_equal(held[0], hr)
    np.testing.assert_array_equal(held[1], lr)
    for i, (a, b) in enumerate(_items(plain)):
        assert a.dtype == np.float32 and np.array_equal(a, hr[i]) and np.array_equal(b, lr[i])


def test_paired_array_dataset_registers():
    from pssr2_amd.data import PairedArrayDataset
    _check_dataset(PairedArrayDataset, *_planted_stack(20))
    ds = PairedArrayDataset(*_planted_stack(20)[:2], hr_res=32, lr_scale=S, register=RADIUS)
    assert type(ds.hr_images) is np.ndarray and type(ds.lr_images) is np.ndarray


def test_device_paired_tile_dataset_registers():
    from pssr2_amd.data import DevicePairedTileDataset
    hr, lr, planted = _planted_stack(21, c_hr=2, c_lr=4)
    _check_dataset(DevicePairedTileDataset, hr, lr, planted)
    ds = DevicePairedTileDataset(torch.tensor(hr).cuda(), torch.tensor(lr).cuda(), hr_res=32, lr_scale=S, register=RADIUS)
    assert ds.hr_images.is_cuda and ds.lr_images.is_cuda and ds.hr_images.shape == (5, 2, 32, 32) and ds.lr_images.shape == (5, 4, 16, 16)
    assert ds.depths == (2, 4) and ds.shifts.tolist() == [list(t) for t in planted]


def test_paired_image_dataset_registers(tmp_path):
    from PIL import Image
    from pssr2_amd.data import PairedImageDataset
    hr, lr, planted = _planted_stack(22)

    def make(hr_stack, lr_stack, **kw):
        root = tmp_path / f"set{len(list(tmp_path.iterdir()))}"
        for side, stack in (("hr", hr_stack), ("lr", lr_stack)):
            (root / side).mkdir(parents=True)
            for i, item in enumerate(stack):
                Image.fromarray(item[0]).save(root / side / f"pair{i}.tif")
        return PairedImageDataset(str(root / "hr"), str(root / "lr"), **kw)

    _check_dataset(make, hr, lr, planted)


def test_objective_on_a_registered_dataset_is_the_objective_on_the_aligned_stack():
    """approximate_crappifier's noise-profile objective, evaluated once: a DevicePairedTileDataset(register=3) built from a planted-shift
    stack gives the bits of the hand-aligned stack, and not those of the unregistered one (whose every edge is "noise")."""
    from pssr2_amd import AdditiveGaussian
    from pssr2_amd.data import DevicePairedTileDataset
    from pssr2_amd.train import _Crappifier_Objective
    hr, lr, planted = _planted_stack(23, noise=6)
    res = S * (SIDE - 2 * R.margin(S, RADIUS))
    aligned = [R.crop_ref(hr[i], lr[i], t, RADIUS) for i, t in enumerate(planted)]
    by_hand = DevicePairedTileDataset(np.stack([a[0] for a in aligned]), np.stack([a[1] for a in aligned]), hr_res=res, lr_scale=S)
    registered = DevicePairedTileDataset(hr, lr, hr_res=res, lr_scale=S, register=RADIUS)
    assert registered.shifts.tolist() == [list(t) for t in planted]
    unregistered = DevicePairedTileDataset(hr, lr, hr_res=S * SIDE, lr_scale=S)
    values = []
    for ds in (by_hand, registered, unregistered):
        obj = _Crappifier_Objective(AdditiveGaussian, ds, len(ds), device="cuda", seed=3)
        random.seed(11)
        values.append(obj.sample([4.0, 1.0]))
    assert np.isfinite(values).all()
    assert values[1] == values[0]
    assert values[2] != values[0]
