"""The resolution-scaling-function search on the device: the fused sums kernel and the reduce kernel against the numpy restatement of
tests/_rsf_ref.py, util.estimate_rsf on planted candidates, util.consistency_map(rsf=...) and test_metrics("rsf").  Everything after the
host-made tap table is integer arithmetic on the same bytes, and the choice is made from the same integers, so every comparison is ==."""
import warnings

import numpy as np
import pytest
import torch

import _consistency_ref as C
import _rsf_ref as F

pytestmark = pytest.mark.gpu

SCALES = (1, 2, 3, 4, 8, 16)
INNER = ((1, 1), (5, 65), (33, 40))           # h' x w': one output, a wide strip over several blocks, blocks with remainders on both axes
PLANES_CAP = 1024                             # grid.y of the kernels: planes beyond it take the stride loop
HALVES = [0.5 * i for i in range(17)]
GRIDS = {                                     # (K, R) -> the candidates
    (1, 0): [0.0],
    (2, 3): [0.0, 1.0],
    (17, 24): HALVES,
    (64, 32): [10.6 * i / 63 for i in range(64)],
}


def _table(s, key):
    rows, radius = F.table(s, GRIDS[key])
    assert (len(rows), radius) == key
    return rows, radius


def _sums_case(y, l, rows, radius, want=None):
    """``want``: the rows where the definitions give them in closed form (constant planes); else the restatement's."""
    from pssr2_amd import ops
    got = ops.rsf_moments_u8(torch.tensor(y).cuda(), torch.tensor(l).cuda(), np.array(rows, dtype=np.int32), radius)
    planes = l.size // (l.shape[-1] * l.shape[-2])
    assert got.dtype == torch.int64 and got.shape == (planes, 3 * len(rows) + 2)
    if want is None:
        want = F.sums_ref(y.reshape(-1, *y.shape[-2:]), l.reshape(-1, *l.shape[-2:]), rows, radius)
    assert got.cpu().tolist() == want
    return want


# ------------------------------------------------------------------------------------------------ the sums table
@pytest.mark.parametrize("key", list(GRIDS))
@pytest.mark.parametrize("s", SCALES)
def test_sums_match_the_restatement(s, key):
    rng = np.random.default_rng(100 * s + key[0])
    rows, radius = _table(s, key)
    m = F.margin(s, radius)
    for hc, wc in INNER:
        h, w = hc + 2 * m, wc + 2 * m
        for planes in (1, 3):
            _sums_case(rng.integers(0, 256, size=(planes, s * h, s * w), dtype=np.uint8), rng.integers(0, 256, size=(planes, h, w), dtype=np.uint8),
                       rows, radius)
        for v in (0, 255):                     # a row sums to 2^22 (+ 1 for Pillow's own at s = 3): both passes give v back
            n = hc * wc
            _sums_case(np.full((1, s * h, s * w), v, dtype=np.uint8), np.full((1, h, w), v, dtype=np.uint8), rows, radius,
                       want=[[v * n, v * v * n, v * v * n] * len(rows) + [v * n, v * v * n]])
    flat = np.full((1, s * (1 + 2 * m), s * (1 + 2 * m)), 255, dtype=np.uint8)       # ... which the restatement says too
    assert F.sums_ref(flat, flat[:, ::s, ::s], rows[:2], radius) == [[255, 255 * 255, 255 * 255] * len(rows[:2]) + [255, 255 * 255]]


def test_sums_when_a_workgroup_walks_several_blocks():
    """128 planes leave 32 workgroups to a plane, and a 163 x 163 window has 36 blocks of 32 x 32 outputs: workgroups take two, and add
    the second into the slots the first one wrote."""
    from pssr2_amd import _lib
    rng = np.random.default_rng(1)
    s, planes = 2, 128
    rows, radius = _table(s, (2, 3))
    assert _lib.lib().pssr_rsf_block(s, radius) == 32
    h = w = 163 + 2 * F.margin(s, radius)
    assert _lib.lib().pssr_rsf_moments_workspace_bytes(planes, h, w, s, 2, radius) // (8 * 8 * planes) < 36
    _sums_case(rng.integers(0, 256, size=(planes, s * h, s * w), dtype=np.uint8), rng.integers(0, 256, size=(planes, h, w), dtype=np.uint8), rows, radius)
    # ... and small blocks: at s = 16 and the largest radius a block has 8 x 8 outputs, a 41 x 49 window has 42 of them, and 128 planes
    # leave 32 workgroups to a plane.  Four different planes, each 32 times: the restatement is taken of the four
    s, planes = 16, 128
    rows, radius = F.table(s, [10.6])
    assert radius == 32 and _lib.lib().pssr_rsf_block(s, radius) == 8
    h, w = 41 + 2 * F.margin(s, radius), 49 + 2 * F.margin(s, radius)
    assert _lib.lib().pssr_rsf_moments_workspace_bytes(planes, h, w, s, 1, radius) // (5 * 8 * planes) < 42
    y, l = rng.integers(0, 256, size=(4, s * h, s * w), dtype=np.uint8), rng.integers(0, 256, size=(4, h, w), dtype=np.uint8)
    _sums_case(np.tile(y, (32, 1, 1)), np.tile(l, (32, 1, 1)), rows, radius, want=F.sums_ref(y, l, rows, radius) * 32)


def test_sums_with_more_partial_rows_than_the_fold_has_threads():
    """One plane, s = 1, one candidate at radius 0 (m = 1): a 544 x 544 window is 17 x 17 blocks of 32 x 32 outputs, one per workgroup, so
    the fold adds 289 partial rows of 3 K + 2 = 5 sums.  The workspace is one such row per workgroup and plane."""
    from pssr2_amd import _lib
    rows = _lib.lib().pssr_rsf_moments_workspace_bytes(1, 546, 546, 1, 1, 0) // (8 * 5)
    assert rows > 256
    rng = np.random.default_rng(5)
    table, radius = _table(1, (1, 0))
    _sums_case(rng.integers(0, 256, size=(1, 546, 546), dtype=np.uint8), rng.integers(0, 256, size=(1, 546, 546), dtype=np.uint8), table, radius)


def test_sums_leading_dimensions_and_odd_addresses():
    """[N, C, ...] inputs, and a sharp buffer that starts at every address modulo 4 (the 16-byte staging must fall back to bytes at the
    buffer's ends and shift inside it)."""
    from pssr2_amd import ops
    rng = np.random.default_rng(2)
    rows, radius = _table(3, (2, 3))
    taps = np.array(rows, dtype=np.int32)
    y, l = rng.integers(0, 256, size=(2, 3, 27, 39), dtype=np.uint8), rng.integers(0, 256, size=(2, 3, 9, 13), dtype=np.uint8)
    want = _sums_case(y, l, rows, radius)
    for off in range(1, 5):
        buf = torch.full((y.size + 8,), 255, dtype=torch.uint8, device="cuda")
        buf[off:off + y.size] = torch.tensor(y.reshape(-1)).cuda()                          # y at byte offset `off` of the buffer
        view = buf[off:off + y.size].view(2, 3, 27, 39)
        assert view.data_ptr() % 4 == off % 4 and view.is_contiguous()
        assert ops.rsf_moments_u8(view, torch.tensor(l).cuda(), taps, radius).cpu().tolist() == want
        d = ops.rsf_reduce_u8(view, taps, radius, [1, 0, 1, 1, 0, 0]).cpu().numpy()
        for p, k in enumerate([1, 0, 1, 1, 0, 0]):
            np.testing.assert_array_equal(d.reshape(6, *d.shape[-2:])[p], F.reduce_k(y.reshape(6, 27, 39)[p], rows[k], 3, radius))
    # a plane that is the whole buffer: the first and the last piece of every block's rows are the buffer's ends
    for s, key in ((1, (1, 0)), (2, (2, 3))):
        rows, radius = _table(s, key)
        m = F.margin(s, radius)
        _sums_case(rng.integers(0, 256, size=(1, s * (3 + 2 * m), s * (3 + 2 * m)), dtype=np.uint8),
                   rng.integers(0, 256, size=(1, 3 + 2 * m, 3 + 2 * m), dtype=np.uint8), rows, radius)


def test_sums_more_planes_than_the_grid():
    rng = np.random.default_rng(3)
    planes = PLANES_CAP + 1
    rows, radius = _table(2, (1, 0))
    _sums_case(rng.integers(0, 256, size=(planes, 6, 6), dtype=np.uint8), rng.integers(0, 256, size=(planes, 3, 3), dtype=np.uint8), rows, radius)
    rows, radius = _table(2, (2, 3))
    _sums_case(rng.integers(0, 256, size=(planes, 16, 18), dtype=np.uint8), rng.integers(0, 256, size=(planes, 8, 9), dtype=np.uint8), rows, radius)


def test_sums_pass_32_bits():
    rows, radius = _table(1, (1, 0))
    want = _sums_case(np.full((1, 302, 302), 255, dtype=np.uint8), np.full((1, 302, 302), 255, dtype=np.uint8), rows, radius)
    assert want[0] == [90000 * 255, 90000 * 255 * 255, 90000 * 255 * 255, 90000 * 255, 90000 * 255 * 255] and want[0][1] > 1 << 32


def test_sums_are_the_same_bits_on_every_run():
    from pssr2_amd import ops
    rng = np.random.default_rng(4)
    y = torch.tensor(rng.integers(0, 256, size=(5, 4 * 64, 4 * 75), dtype=np.uint8)).cuda()
    l = torch.tensor(rng.integers(0, 256, size=(5, 64, 75), dtype=np.uint8)).cuda()
    taps, radius = ops.rsf_taps(4, F.DEFAULT_SIGMAS)
    first = ops.rsf_moments_u8(y, l, taps, radius)
    assert all(torch.equal(ops.rsf_moments_u8(y, l, taps, radius), first) for _ in range(3))
    sel = [k % 33 for k in (0, 32, 7, 7, 19)]
    d = ops.rsf_reduce_u8(y, taps, radius, sel)
    assert all(torch.equal(ops.rsf_reduce_u8(y, taps, radius, sel), d) for _ in range(3))


# ------------------------------------------------------------------------------------------------ the reduce kernel
@pytest.mark.parametrize("s", SCALES)
def test_reduce_matches_the_restatement_with_mixed_sel(s):
    from pssr2_amd import ops
    rng = np.random.default_rng(200 + s)
    for key in ((2, 3), (17, 24)):
        rows, radius = _table(s, key)
        taps = np.array(rows, dtype=np.int32)
        m = F.margin(s, radius)
        for hc, wc in ((1, 1), (33, 40)):
            h, w = hc + 2 * m, wc + 2 * m
            y = rng.integers(0, 256, size=(2, 2, s * h, s * w), dtype=np.uint8)
            sel = [int(v) for v in rng.integers(0, key[0], size=4)]
            sel[0], sel[-1] = key[0] - 1, 0
            got = ops.rsf_reduce_u8(torch.tensor(y).cuda(), taps, radius, sel)
            assert got.dtype == torch.uint8 and got.shape == (2, 2, hc, wc)
            for p, k in enumerate(sel):
                np.testing.assert_array_equal(got.cpu().numpy().reshape(4, hc, wc)[p], F.reduce_k(y.reshape(4, s * h, s * w)[p], rows[k], s, radius))
            for bad in (sel[:-1], [key[0]] + sel[1:], [-1] + sel[1:]):
                with pytest.raises(ValueError, match="sel"):
                    ops.rsf_reduce_u8(torch.tensor(y).cuda(), taps, radius, bad)


@pytest.mark.parametrize("s", SCALES)
def test_the_sigma_zero_row_is_the_device_reduction(s):
    """With the sigma = 0 row, D == bilinear_down_u8(Y)[m:h-m, m:w-m] bit for bit, whatever R."""
    from pssr2_amd import ops
    rng = np.random.default_rng(300 + s)
    for radius in (0, 3, 24):
        m = F.margin(s, radius)
        h, w = 33 + 2 * m, 40 + 2 * m
        y = torch.tensor(rng.integers(0, 256, size=(3, s * h, s * w), dtype=np.uint8)).cuda()
        taps, rad = ops.rsf_taps(s, [radius / 3.0, 0.0], radius)            # a wide row beside it: the table has its full width
        assert rad == radius
        got = ops.rsf_reduce_u8(y, taps, radius, [1, 1, 1])
        assert torch.equal(got, ops.bilinear_down_u8(y, h, w)[:, m:h - m, m:w - m])


def test_ops_refuse_bad_arguments_on_the_device():
    from pssr2_amd import ops
    y, l = torch.zeros(2, 48, 48, dtype=torch.uint8, device="cuda"), torch.zeros(2, 12, 12, dtype=torch.uint8, device="cuda")
    taps, radius = ops.rsf_taps(4, [0.0, 1.0])
    assert ops.rsf_moments_u8(y, l, taps, radius).shape == (2, 8)
    wide, wide_radius = ops.rsf_taps(4, [0.0, 6.5])                                          # R = 20, m = 6: nothing is left of 12 rows
    for bad in (dict(y=y[:1]), dict(y=y.float()), dict(l=l.cpu()), dict(taps=torch.tensor(taps).cuda()), dict(taps=taps[:, :-2]), dict(taps=-taps),
                dict(taps=ops.rsf_taps(2, [0.0, 1.0])[0]), dict(radius=4), dict(taps=wide, radius=wide_radius)):
        kw = dict(dict(y=y, l=l, taps=taps, radius=radius), **bad)
        with pytest.raises(ValueError):
            ops.rsf_moments_u8(kw["y"], kw["l"], kw["taps"], kw["radius"])
    with pytest.raises(ValueError, match="margin"):
        ops.rsf_reduce_u8(y, wide, wide_radius, [0, 0])
    with pytest.raises(ValueError, match="multiple"):
        ops.rsf_reduce_u8(y[:, :46], taps, radius, [0, 0])


# ------------------------------------------------------------------------------------------------ estimate_rsf
def _same_rsf(got, want, curve_on_device=False):
    curve = got.curve.cpu().numpy() if curve_on_device else got.curve
    assert torch.is_tensor(got.curve) == curve_on_device and curve.dtype == np.float64
    for a, b in zip((got.sigma, got.fwhm, got.score, curve, got.index), want[:5]):
        assert np.asarray(a).tolist() == np.asarray(b).tolist()
    assert got.margin == want[5]


@pytest.mark.parametrize("c_lr,c_hat", [(3, 1), (3, 3), (4, 2)])
def test_estimate_rsf_finds_planted_candidates(c_lr, c_hat):
    from pssr2_amd.util import estimate_rsf
    rng = np.random.default_rng(10 * c_lr + c_hat)
    s, sigmas = 2, HALVES[:9]                                # 0 .. 4: R = 12, m = 7
    rows, radius = F.table(s, sigmas)
    planted = [3, 0, 7, 5]
    hat, lr = F.planted_pair(rng, 4, c_hat, c_lr, 21, 24, s, rows, radius, planted)
    want = F.estimate_ref(lr, hat, sigmas)
    assert want[4].tolist() == planted and want[2].tolist() == [1.0] * 4 and want[0].tolist() == [sigmas[k] for k in planted]
    with warnings.catch_warnings():
        warnings.simplefilter("error")                     # no choice lies on the end of the grid
        _same_rsf(estimate_rsf(lr, hat, sigmas=sigmas), want)
        _same_rsf(estimate_rsf(torch.tensor(lr).cuda(), torch.tensor(hat).cuda(), sigmas=np.array(sigmas), to_numpy=False), want, True)
        _same_rsf(estimate_rsf(lr, torch.tensor(hat).cuda(), sigmas=sigmas, pixel_size=0.5), F.estimate_ref(lr, hat, sigmas, pixel_size=0.5))
        one = estimate_rsf(lr[2], hat[2], sigmas=sigmas)                    # one pair without the batch axis
        pooled = estimate_rsf(lr, hat, sigmas=sigmas, pool="all")
    assert (one.sigma, one.index, one.score, one.fwhm) == (3.5, 7, 1.0, F.FWHM * 3.5) and one.curve.tolist() == want[3][2].tolist()
    assert type(one.sigma) is float and type(one.index) is int and one.curve.shape == (9,)
    want_all = F.estimate_ref(lr, hat, sigmas, pool="all")
    _same_rsf(pooled, want_all)
    assert len(set(pooled.index.tolist())) == 1 and 0 < pooled.score[0] < 1.0 and pooled.curve.shape == (4, 9)


def test_estimate_rsf_with_noise_and_the_default_grid():
    """The measured side carries noise (scores below 1) and the grid is the default one: K = 33, R = 24, at s = 4."""
    from pssr2_amd.util import estimate_rsf
    rng = np.random.default_rng(7)
    rows, radius = F.table(4, F.DEFAULT_SIGMAS)
    planted = [8, 20]                                        # sigma 2 and 5
    hat, lr = F.planted_pair(rng, 2, 1, 1, 30, 32, 4, rows, radius, planted)
    hat = np.repeat(np.repeat(hat[..., ::8, ::8], 8, axis=-2), 8, axis=-1)                  # coarse texture: neighbouring widths differ visibly
    for i, k in enumerate(planted):
        lr[i, :, 7:-7, 7:-7] = F.reduce_k(hat[i], rows[k], 4, radius)
    lr = np.clip(lr.astype(np.int64) + rng.integers(-3, 4, size=lr.shape), 0, 255).astype(np.uint8)
    want = F.estimate_ref(lr, hat)
    assert want[4].tolist() == planted and all(0.0 < v < 1.0 for v in want[2]) and want[5] == 7
    _same_rsf(estimate_rsf(lr, hat), want)


def test_estimate_rsf_warns_at_the_end_of_the_grid():
    from pssr2_amd.util import estimate_rsf
    rng = np.random.default_rng(8)
    sigmas = [0.0, 1.0, 2.0]
    rows, radius = F.table(2, sigmas)
    hat, lr = F.planted_pair(rng, 3, 1, 1, 16, 16, 2, rows, radius, [1, 2, 2])
    with pytest.warns(UserWarning, match=r"item\(s\) \[1, 2\]"):
        got = estimate_rsf(lr, hat, sigmas=sigmas)
    assert got.index.tolist() == [1, 2, 2]
    with warnings.catch_warnings():
        warnings.simplefilter("error")                     # a grid of one has no end to warn about
        assert estimate_rsf(lr, hat, sigmas=[2.0]).index.tolist() == [0] * 3
    # a constant pair chooses candidate 0 with score 0
    flat = estimate_rsf(np.full((1, 1, 16, 16), 9, dtype=np.uint8), np.full((1, 1, 32, 32), 200, dtype=np.uint8), sigmas=sigmas)
    assert flat.index.tolist() == [0] and flat.score.tolist() == [0.0] and flat.curve.tolist() == [[0.0] * 3]


# ------------------------------------------------------------------------------------------------ consistency_map(rsf=...)
def _same_consistency(got, want, to_numpy=True):
    from pssr2_amd.util import RSFConsistency
    assert type(got) is RSFConsistency
    cmap = got.map if to_numpy else got.map.cpu().numpy()
    assert (type(got.map) is np.ndarray) == to_numpy and cmap.dtype == np.uint8
    np.testing.assert_array_equal(cmap, want[0])
    for a, b in zip((got.alpha, got.beta, got.rse, got.rsp, got.sigma), want[1:6]):
        assert a.dtype == np.float64 and a.tolist() == b.tolist()
    assert got.margin == want[6]


@pytest.mark.parametrize("fit", C.FITS)
def test_consistency_map_after_a_fitted_or_given_rsf(fit):
    from pssr2_amd.util import Consistency, consistency_map
    rng = np.random.default_rng(11)
    s = 2
    rows, radius = F.table(s, F.DEFAULT_SIGMAS)
    m = F.margin(s, radius)
    h, w = 9 + 2 * m, 12 + 2 * m
    planted = [6, 14, 0]                                     # sigma 1.5, 3.5, 0
    hat, lr = F.planted_pair(rng, 3, 2, 3, h, w, s, rows, radius, planted)
    want = F.consistency_ref(lr, hat, "fit", fit)
    assert want[5].tolist() == [1.5, 3.5, 0.0] and want[6] == m
    got = consistency_map(lr, hat, fit=fit, rsf="fit")
    _same_consistency(got, want)
    assert got.map.shape == (3, 2, 9, 12) and got.rsp.tolist() == [[1.0, 1.0]] * 3
    if fit == "affine":                                      # the planted pair is explained exactly: nothing is marked
        assert not got.map.any() and got.rse.tolist() == [[0.0, 0.0]] * 3 and got.alpha.tolist() == [[1.0, 1.0]] * 3
    _same_consistency(consistency_map(torch.tensor(lr).cuda(), torch.tensor(hat).cuda(), fit=fit, rsf="fit", to_numpy=False), want, to_numpy=False)
    # without the keyword: the result of before, in its five fields, and it marks the pair that the bilinear model does not explain
    plain = consistency_map(lr, hat, fit=fit)
    old = C.consistency_ref(lr, hat, fit)
    assert type(plain) is Consistency and plain.map.shape == (3, 2, h, w)
    np.testing.assert_array_equal(plain.map, old[0])
    assert all(a.tolist() == b.tolist() for a, b in zip(plain[1:], old[1:]))
    assert plain.map[0, :, m:h - m, m:w - m].any() and plain.map[1, :, m:h - m, m:w - m].any()
    none = consistency_map(lr, hat, fit=fit, rsf=None)
    assert type(none) is Consistency and all(np.array_equal(a, b) for a, b in zip(none, plain))
    # a given width for every item, and one per item
    for given in (2.0, 0.0, [1.5, 3.5, 0.0], np.array([3.0, 3.0, 0.25])):
        _same_consistency(consistency_map(lr, hat, fit=fit, rsf=given), F.consistency_ref(lr, hat, given, fit))
    one = consistency_map(lr[1], hat[1], fit=fit, rsf=3.5)                  # one pair without the batch axis
    want1 = F.consistency_ref(lr[1:2], hat[1:2], 3.5, fit)
    np.testing.assert_array_equal(one.map, want1[0][0])
    assert one.sigma == 3.5 and one.rse.tolist() == want1[3][0].tolist() and one.margin == 7 and one.map.shape == (2, h - 14, w - 14)   # R = 11


# ------------------------------------------------------------------------------------------------ test_metrics
class _Enlarge(torch.nn.Module):
    """A probe model: every LR pixel as a 2 x 2 block plus a ramp, so that the prediction has edges that its input does not."""

    def forward(self, x):
        y = x.repeat_interleave(2, dim=-2).repeat_interleave(2, dim=-1)
        i = torch.arange(y.shape[-1], dtype=y.dtype, device=y.device)
        return y + 0.25 * i.view(1, 1, 1, -1)


class _Pairs(torch.utils.data.Dataset):
    """A paired dataset in memory: uint8 LR images [1, 32, 32] with HR [1, 64, 64], handed over as float32."""
    is_lr, extra_hr_files = False, None

    def __init__(self, n=2, seed=9, crop_res=64):
        rng = np.random.default_rng(seed)
        self.lr_scale = 2
        self.lrs = rng.integers(0, 128, size=(n, 1, 32, 32), dtype=np.uint8)
        self.hrs = rng.integers(0, 256, size=(n, 1, 64, 64), dtype=np.uint8)
        self.val_idx, self.crop_res = list(range(n)), crop_res

    def __len__(self):
        return len(self.lrs)

    def _get_name(self, i):
        return f"img{i}"

    def __getitem__(self, i):
        return torch.tensor(self.hrs[i]).float(), torch.tensor(self.lrs[i]).float()


@pytest.mark.parametrize("norm", [False, True])
def test_test_metrics_rsf(norm):
    from pssr2_amd.predict import predict_images, test_metrics
    ds = _Pairs()
    default = test_metrics(_Enlarge(), ds, device="cuda", metrics=("psnr",), norm=norm, avg=False)
    pred = predict_images(_Enlarge(), ds, device="cuda", batch_size=1, out_dir=None)["img0"]
    want = F.estimate_ref(ds.lrs[:1], pred[None])
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        got = test_metrics(_Enlarge(), ds, device="cuda", metrics=("psnr", "rsf"), norm=norm, avg=False)
        assert got == {"psnr": default["psnr"], "rsf": [want[0][0]] * 2}                      # every iteration: dataset[0]
        assert test_metrics(_Enlarge(), ds, device="cuda", metrics="rsf", norm=norm) == {"rsf": want[0][0]}
        ds.crop_res = 56                                     # the LR side is cut as the prediction is
        want = F.estimate_ref(ds.lrs[:1, :, :28, :28], pred[None, :, :56, :56])
        assert test_metrics(_Enlarge(), ds, device="cuda", metrics=("rsf",), norm=norm, avg=False) == {"rsf": [want[0][0]] * 2}
