"""Consistency maps on the device: the fused reduction + moments kernel and the map kernel against the numpy restatement of
tests/_consistency_ref.py (and the reduction against the two-launch kernel it shares its taps with), util.consistency_map, and the
drivers through probe models and one real model.  Everything after the fit is integer arithmetic and the fit is the same Python
expression on the same integers, so every comparison is with ==."""
import numpy as np
import pytest
import torch

import _consistency_ref as R

pytestmark = pytest.mark.gpu

SCALES = (1, 2, 3, 4, 8, 16)
SIZES = ((1, 1), (7, 5), (32, 32), (33, 40), (5, 65))
PLANES_CAP = 1024                     # grid.y of both kernels: planes beyond it take the stride loop


def _same_stats(got, want):
    """Consistency against consistency_ref's tuple: bytes of the map, and the float64 statistics bit for bit."""
    assert got.map.dtype == np.uint8 and got.map.shape == want[0].shape
    np.testing.assert_array_equal(got.map, want[0])
    for name, w in zip(("alpha", "beta", "rse", "rsp"), want[1:]):
        g = getattr(got, name)
        assert g.dtype == np.float64 and g.shape == w.shape, name
        assert g.tolist() == w.tolist(), name


# ------------------------------------------------------------------------------------------------ reduction + moments
def _reduce_case(y, l):
    from pssr2_amd import ops
    h, w = l.shape[-2:]
    want_d = R.reduce_ref(y, h, w)
    yd, ld = torch.tensor(y).cuda(), torch.tensor(l).cuda()
    d, sums = ops.reduce_moments_u8(yd, ld)
    assert d.dtype == torch.uint8 and d.shape == ld.shape and sums.dtype == torch.int64 and sums.shape == (l.size // (h * w), 5)
    np.testing.assert_array_equal(d.cpu().numpy(), want_d)
    assert torch.equal(d, ops.bilinear_down_u8(yd, h, w))                 # the two-launch reduction it shares its taps with
    want = [list(R.moments_ref(a, b)) for a, b in zip(want_d.reshape(-1, h, w), l.reshape(-1, h, w))]
    assert sums.cpu().tolist() == want
    return want


@pytest.mark.parametrize("planes", [1, 3])
@pytest.mark.parametrize("h,w", SIZES)
@pytest.mark.parametrize("s", SCALES)
def test_reduce_moments_matches_numpy_and_the_two_launch_reduction(s, h, w, planes):
    rng = np.random.default_rng(1000 * s + 10 * h + planes)
    l = rng.integers(0, 256, size=(planes, h, w), dtype=np.uint8)
    _reduce_case(rng.integers(0, 256, size=(planes, h * s, w * s), dtype=np.uint8), l)
    for v in (0, 255):
        want = _reduce_case(np.full((planes, h * s, w * s), v, dtype=np.uint8), np.full((planes, h, w), v, dtype=np.uint8))
        assert want[0] == [v * h * w, v * h * w] + [v * v * h * w] * 3


def test_reduce_moments_leading_dimensions_and_odd_addresses():
    """[N, C, ...] inputs, and a prediction that starts at every address modulo 4 (the dword staging must fall back to bytes at the
    buffer's ends and shift inside it)."""
    from pssr2_amd import ops
    rng = np.random.default_rng(5)
    y, l = rng.integers(0, 256, size=(2, 3, 21, 15), dtype=np.uint8), rng.integers(0, 256, size=(2, 3, 7, 5), dtype=np.uint8)
    d, sums = ops.reduce_moments_u8(torch.tensor(y).cuda(), torch.tensor(l).cuda())
    np.testing.assert_array_equal(d.cpu().numpy(), R.reduce_ref(y, 7, 5))
    for off in range(1, 5):
        buf = torch.full((y.size + 8,), 255, dtype=torch.uint8, device="cuda")
        buf[off:off + y.size] = torch.tensor(y.reshape(-1)).cuda()                          # y at byte offset `off` of the buffer
        view = buf[off:off + y.size].view(2, 3, 21, 15)
        assert view.data_ptr() % 4 == off % 4 and view.is_contiguous()
        d2, sums2 = ops.reduce_moments_u8(view, torch.tensor(l).cuda())
        assert torch.equal(d2, d) and torch.equal(sums2, sums)


def test_reduce_moments_more_planes_than_the_grid():
    rng = np.random.default_rng(6)
    planes = PLANES_CAP + 1
    _reduce_case(rng.integers(0, 256, size=(planes, 4, 4), dtype=np.uint8), rng.integers(0, 256, size=(planes, 2, 2), dtype=np.uint8))


def test_reduce_moments_sums_pass_32_bits():
    want = _reduce_case(np.full((1, 300, 300), 255, dtype=np.uint8), np.full((1, 300, 300), 255, dtype=np.uint8))
    assert want[0][2] == 90000 * 255 * 255 > 1 << 32


def test_reduce_moments_more_blocks_of_outputs_than_workgroups():
    """A plane of more 32 x 32 blocks than the launch has workgroups for it: every workgroup walks several."""
    rng = np.random.default_rng(7)
    h, w = 32 * 70, 32 * 70
    assert (h // 32) * (w // 32) > 4096
    _reduce_case(rng.integers(0, 256, size=(1, h, w), dtype=np.uint8), rng.integers(0, 256, size=(1, h, w), dtype=np.uint8))


def test_ops_refuse_bad_shapes():
    from pssr2_amd import ops
    z = lambda *s: torch.zeros(*s, dtype=torch.uint8, device="cuda")      # noqa: E731
    for y, l in ((z(1, 8, 9), z(1, 4, 4)), (z(1, 68, 68), z(1, 4, 4)), (z(1, 3, 3), z(1, 4, 4)), (z(2, 8, 8), z(1, 4, 4)), (z(8, 8), z(1, 4, 4))):
        with pytest.raises(ValueError):
            ops.reduce_moments_u8(y, l)
    with pytest.raises(ValueError):
        ops.reduce_moments_u8(z(1, 8, 8).float(), z(1, 4, 4))
    lut = torch.zeros(1, 256, dtype=torch.int32, device="cuda")
    for d, l, t in ((z(1, 4, 4), z(1, 4, 5), lut), (z(1, 4, 4), z(1, 4, 4), lut.long()), (z(2, 4, 4), z(2, 4, 4), lut), (z(1, 4, 4), z(1, 4, 4), lut.cpu())):
        with pytest.raises(ValueError):
            ops.consistency_map_u8(d, l, t)


# ------------------------------------------------------------------------------------------------ map + sse
@pytest.mark.parametrize("planes", [1, 3])
@pytest.mark.parametrize("pixels", [1, 255, 256, 257, 90000])
def test_consistency_map_matches_numpy(pixels, planes):
    from pssr2_amd import ops
    rng = np.random.default_rng(pixels + planes)
    d = rng.integers(0, 256, size=(planes, 1, pixels), dtype=np.uint8)
    l = rng.integers(0, 256, size=(planes, 1, pixels), dtype=np.uint8)
    lut = rng.integers(-65536, 131072, size=(planes, 256)).astype(np.int32)
    lut[:, 0], lut[:, 255], lut[:, 7] = -65536, 131071, 0
    d[:, 0, 0], l[:, 0, 0] = 0, 255                                       # the largest |256 L - P|: 65280 + 65536
    if pixels > 1:
        d[:, 0, 1], l[:, 0, 1] = 255, 0                                   # ... and 131071 on the other side
    got, sse = ops.consistency_map_u8(torch.tensor(d).cuda(), torch.tensor(l).cuda(), torch.tensor(lut).cuda())
    assert got.dtype == torch.uint8 and got.shape == d.shape and sse.dtype == torch.int64 and sse.shape == (planes,)
    for p in range(planes):
        want, want_sse = R.map_ref(d[p], l[p], lut[p])
        np.testing.assert_array_equal(got[p].cpu().numpy(), want)
        assert int(sse[p]) == want_sse
    assert got[0, 0, 0] == 255


def test_consistency_map_more_planes_than_the_grid_and_a_large_sse():
    from pssr2_amd import ops
    rng = np.random.default_rng(8)
    planes = PLANES_CAP + 1
    d, l = rng.integers(0, 256, size=(planes, 2, 2), dtype=np.uint8), rng.integers(0, 256, size=(planes, 2, 2), dtype=np.uint8)
    lut = rng.integers(-65536, 131072, size=(planes, 256)).astype(np.int32)
    got, sse = ops.consistency_map_u8(torch.tensor(d).cuda(), torch.tensor(l).cuda(), torch.tensor(lut).cuda())
    want = [R.map_ref(d[p], l[p], lut[p]) for p in range(planes)]
    np.testing.assert_array_equal(got.cpu().numpy(), np.stack([w[0] for w in want]))
    assert sse.cpu().tolist() == [w[1] for w in want]
    # every pixel at the largest error: 300 x 300 x 131071^2 is far beyond 2^32 (and beyond 2^53, where a double would round)
    d, l = np.zeros((1, 300, 300), dtype=np.uint8), np.zeros((1, 300, 300), dtype=np.uint8)
    lut = np.full((1, 256), 131071, dtype=np.int32)
    got, sse = ops.consistency_map_u8(torch.tensor(d).cuda(), torch.tensor(l).cuda(), torch.tensor(lut).cuda())
    assert int(sse[0]) == 90000 * 131071 ** 2 and bool((got == 255).all())


@pytest.mark.parametrize("pixels", [258 * 4096, 257 * 4096 + 1])
def test_consistency_map_more_partial_rows_than_the_fold_has_threads(pixels):
    """One plane of more than 256 workgroups, on the 16-byte path and on the scalar path: the fold's 256 threads take more than one
    partial row each.  The workspace is one 64-bit partial sum per workgroup and plane."""
    from pssr2_amd import _lib, ops
    rows = _lib.lib().pssr_consistency_map_workspace_bytes(1, pixels) // 8
    assert rows > 256
    rng = np.random.default_rng(pixels)
    d, l = rng.integers(0, 256, size=(1, 1, pixels), dtype=np.uint8), rng.integers(0, 256, size=(1, 1, pixels), dtype=np.uint8)
    lut = rng.integers(-65536, 131072, size=(1, 256)).astype(np.int32)
    got, sse = ops.consistency_map_u8(torch.tensor(d).cuda(), torch.tensor(l).cuda(), torch.tensor(lut).cuda())
    want, want_sse = R.map_ref(d[0], l[0], lut[0])
    np.testing.assert_array_equal(got[0].cpu().numpy(), want)
    assert sse.cpu().tolist() == [want_sse]


# ------------------------------------------------------------------------------------------------ util.consistency_map
@pytest.mark.parametrize("fit", R.FITS)
@pytest.mark.parametrize("m,c", [(3, 1), (3, 3), (4, 2)])
def test_consistency_map_against_the_restatement(m, c, fit):
    from pssr2_amd.util import Consistency, consistency_map
    rng = np.random.default_rng(10 * m + c)
    lr = rng.integers(0, 256, size=(2, m, 9, 13), dtype=np.uint8)
    # a prediction that does follow its input (gain 1.5, offset -20 on the centre frames, enlarged) with noise, so that the fit matters
    base = R.slice_center(lr, c).astype(np.float64).repeat(4, axis=-2).repeat(4, axis=-1)
    hat = np.clip(np.round(1.5 * base - 20 + rng.normal(0, 6, size=base.shape)), 0, 255).astype(np.uint8)
    hat[1, 0] = 200                                                        # one constant plane: the den == 0 branch
    want = R.consistency_ref(lr, hat, fit)
    got = consistency_map(lr, hat, fit=fit)
    assert isinstance(got, Consistency) and got.map.shape == (2, c, 9, 13)
    _same_stats(got, want)
    assert got.rsp[1, 0] == 0.0 and (fit == "identity" or got.alpha[1, 0] == 0.0)
    if fit == "affine":
        assert got.alpha[0, 0] > 0.5 and got.rsp[0, 0] > 0.8                # the prediction does follow its input
    # device tensors in, a device map out; and single items without the batch axis
    dev = consistency_map(torch.tensor(lr).cuda(), torch.tensor(hat).cuda(), fit=fit, to_numpy=False)
    assert torch.is_tensor(dev.map) and dev.map.is_cuda and dev.map.dtype == torch.uint8
    _same_stats(dev._replace(map=dev.map.cpu().numpy()), want)
    one = consistency_map(lr[1], hat[1], fit=fit)
    _same_stats(one, tuple(v[1] for v in want))


# ------------------------------------------------------------------------------------------------ the drivers, with probes
class _Centre(torch.nn.Module):
    """gain * (centre frame) + 3.25, every pixel repeated s x s: exact in float32 for the gains used."""

    def __init__(self, s=2, gain=0.5):
        super().__init__()
        self.s, self.gain = s, gain

    def forward(self, x):
        c = x.shape[1] // 2
        y = self.gain * x[:, c:c + 1] + 3.25
        return y.repeat_interleave(self.s, dim=-2).repeat_interleave(self.s, dim=-1)


class _Positional(_Centre):
    """... plus 3 col - 2 row of the tile-local output coordinate: every member and every tile predicts something else."""

    def forward(self, x):
        y = super().forward(x)
        i = torch.arange(y.shape[-1], dtype=y.dtype, device=y.device)
        j = torch.arange(y.shape[-2], dtype=y.dtype, device=y.device)
        return y + 3 * i.view(1, 1, 1, -1) - 2 * j.view(1, 1, -1, 1)


class _Frames(torch.nn.Module):
    """Every frame its own plane (C_out = m), enlarged 2 x 2."""

    def forward(self, x):
        return (0.75 * x + 1.0).repeat_interleave(2, dim=-2).repeat_interleave(2, dim=-1)


@pytest.fixture(scope="module")
def probe_stack():
    return np.random.default_rng(7).integers(0, 128, size=(5, 45, 38), dtype=np.uint8)


# keywords, frames of the stack used, (m, step, n_slices)
SHEET_PATHS = {
    "plain": (dict(), 1, (1, 1, 1)),
    "cover": (dict(cover=True), 1, (1, 1, 1)),
    "stacked": (dict(n_frames=3, slide=True), 5, (3, 1, 3)),
    "linear": (dict(blend="linear"), 1, (1, 1, 1)),
    "ensemble": (dict(cover=True, ensemble=8), 3, (3, 3, 1)),
    "linear_stacked_ensemble": (dict(n_frames=3, slide=True, blend="linear", ensemble=2), 5, (3, 1, 3)),
}


def _sheet_want(stack, sheet, m, step, n_slices, stacked, fit="affine"):
    """The restatement applied to the sheet the call returned, against the LR region that sheet covers."""
    hat = sheet if stacked else sheet[None]
    lh, lw = hat.shape[-2] // 2, hat.shape[-1] // 2
    lr = np.stack([stack[k * step:k * step + m, :lh, :lw] for k in range(n_slices)])
    want = R.consistency_ref(lr, hat, fit)
    return want if stacked else tuple(v[0] for v in want)


@pytest.mark.parametrize("path", list(SHEET_PATHS))
def test_predict_sheet_consistency_on_every_path(probe_stack, path):
    from pssr2_amd.predict import predict_sheet
    from pssr2_amd.util import Consistency
    kw, frames, (m, step, n_slices) = SHEET_PATHS[path]
    stack = probe_stack[:frames]
    stacked = "n_frames" in kw
    common = dict(tile_res=16, overlap=4, margin=1, batch_size=5, **kw)
    sheet_only = predict_sheet(_Positional(), stack, consistency=False, **common)
    assert isinstance(sheet_only, np.ndarray)
    np.testing.assert_array_equal(predict_sheet(_Positional(), stack, **common), sheet_only)
    sheet, cons = predict_sheet(_Positional(), stack, consistency=True, **common)
    np.testing.assert_array_equal(sheet, sheet_only)                      # the sheet does not change
    assert isinstance(cons, Consistency) and cons.map.shape == sheet.shape[:-2] + (sheet.shape[-2] // 2, sheet.shape[-1] // 2)
    assert cons.rse.shape == sheet.shape[:-2]
    _same_stats(cons, _sheet_want(stack, sheet, m, step, n_slices, stacked))
    assert cons.map.any() and (cons.rse > 0).all()                        # the positional term is not in the LR image
    # with the spread, on the device, and the other fit
    sheet2, spread, cons2 = predict_sheet(_Positional(), stack, consistency=True, spread=True, fit="identity", to_numpy=False, **common)
    only2, spread_only = predict_sheet(_Positional(), stack, spread=True, **common)
    assert sheet2.is_cuda and spread.is_cuda and cons2.map.is_cuda
    np.testing.assert_array_equal(sheet2.cpu().numpy(), sheet_only)
    np.testing.assert_array_equal(only2, sheet_only)
    np.testing.assert_array_equal(spread.cpu().numpy(), spread_only)
    _same_stats(cons2._replace(map=cons2.map.cpu().numpy()), _sheet_want(stack, sheet, m, step, n_slices, stacked, "identity"))
    assert (cons2.alpha == 1.0).all() and (cons2.beta == 0.0).all()


def test_predict_sheet_consistency_of_a_faithful_model_is_small(probe_stack):
    """The centre-frame probe without the positional term: the reduced prediction is a smoothed gain * LR + 3.25, which correlates with
    the LR image; an all-frames model gives one fit per plane; more planes than frames is refused."""
    from pssr2_amd.predict import predict_sheet
    sheet, cons = predict_sheet(_Centre(), probe_stack[:1], tile_res=16, overlap=4, cover=True, consistency=True)
    _same_stats(cons, _sheet_want(probe_stack[:1], sheet, 1, 1, 1, False))
    assert cons.rsp[0] > 0.6 and cons.alpha[0] > 0.8
    sheet, cons = predict_sheet(_Frames(), probe_stack[:3], tile_res=16, overlap=4, cover=True, consistency=True)
    assert sheet.shape == (3, 90, 76) and cons.map.shape == (3, 45, 38) and cons.alpha.shape == (3,)
    _same_stats(cons, _sheet_want(probe_stack[:3], sheet, 3, 3, 1, False))
    with pytest.raises(ValueError, match="planes"):
        predict_sheet(_Wider(), probe_stack[:1], tile_res=16, overlap=4, consistency=True)


class _Wider(torch.nn.Module):
    """Two planes from one frame."""

    def forward(self, x):
        y = x.repeat_interleave(2, dim=-2).repeat_interleave(2, dim=-1)
        return torch.cat([y, y + 1], dim=1)


class _Pairs(torch.utils.data.Dataset):
    """A paired dataset in memory: uint8 LR images [1, 32, 32] with HR [1, 64, 64], handed over as float32, or as uint8 when ``compact``."""
    is_lr, extra_hr_files = False, None

    def __init__(self, n=5, seed=9, crop_res=64, compact=False, scale=2):
        rng = np.random.default_rng(seed)
        self.lr_scale = scale
        self.lrs = rng.integers(0, 128, size=(n, 1, 32, 32), dtype=np.uint8)
        self.hrs = rng.integers(0, 256, size=(n, 1, 32 * scale, 32 * scale), dtype=np.uint8)
        self.val_idx, self.crop_res, self.compact = list(range(n)), crop_res, compact

    def __len__(self):
        return len(self.lrs)

    def _get_name(self, i):
        return f"img{i}"

    def __getitem__(self, i):
        hr, lr = torch.tensor(self.hrs[i]), torch.tensor(self.lrs[i])
        return (hr, lr) if self.compact else (hr.float(), lr.float())


def _same_preds(a, b):
    assert list(a) == list(b)
    for k in a:
        assert a[k].dtype == b[k].dtype == np.uint8 and a[k].shape == b[k].shape
        np.testing.assert_array_equal(a[k], b[k])


def _check_scores(scores, ds, preds, crop, fit="affine"):
    """Every item's Consistency against the restatement of the prediction handed out and the item's LR side cut to crop // 2."""
    assert list(scores) == list(preds)
    for i, name in enumerate(preds):
        want = R.consistency_ref(ds.lrs[i:i + 1, :, :crop // 2, :crop // 2], preds[name][None], fit)
        assert scores[name].map.shape == (1, crop // 2, crop // 2) and scores[name].rse.shape == (1,)
        _same_stats(scores[name], tuple(v[0] for v in want))


@pytest.mark.parametrize("compact", [False, True])
@pytest.mark.parametrize("crop", [64, 40])
def test_predict_images_consistency(crop, compact):
    from pssr2_amd.predict import predict_images
    ds = _Pairs(crop_res=crop, compact=compact)
    plain = predict_images(_Positional(), ds, device="cuda", batch_size=2, out_dir=None)
    _same_preds(predict_images(_Positional(), ds, device="cuda", batch_size=2, out_dir=None, consistency=False), plain)
    preds, scores = predict_images(_Positional(), ds, device="cuda", batch_size=2, out_dir=None, consistency=True)
    _same_preds(preds, plain)
    _check_scores(scores, ds, preds, crop)
    assert all(s.map.any() for s in scores.values())
    # with the ensemble and its spread: the ensembled prediction is what is scored, and the dict comes last
    ens, spreads = predict_images(_Positional(), ds, device="cuda", batch_size=2, out_dir=None, ensemble=4, spread=True)
    got = predict_images(_Positional(), ds, device="cuda", batch_size=2, out_dir=None, ensemble=4, spread=True, consistency=True, fit="identity")
    assert len(got) == 3
    _same_preds(got[0], ens)
    _same_preds(got[1], spreads)
    _check_scores(got[2], ds, ens, crop, "identity")
    # norm changes the prediction handed out, not what is scored
    normed, scores_n = predict_images(_Positional(), ds, device="cuda", batch_size=2, out_dir=None, norm=True, consistency=True)
    _same_preds(normed, predict_images(_Positional(), ds, device="cuda", batch_size=2, out_dir=None, norm=True))
    _check_scores(scores_n, ds, preds, crop)


def test_predict_images_consistency_files_and_a_bad_crop(tmp_path):
    from PIL import Image
    from pssr2_amd.predict import predict_images
    ds = _Pairs(crop_res=48)
    preds, spreads, scores = predict_images(_Positional(), ds, device="cuda", batch_size=2, out_dir=None, ensemble=4, spread=True, consistency=True)
    assert predict_images(_Positional(), ds, device="cuda", batch_size=2, out_dir=str(tmp_path), prefix="run", ensemble=4, spread=True,
                          consistency=True) is None
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted(f"run_img{i}{tail}.tif" for i in range(5) for tail in ("", "_spread", "_consistency"))
    for i in range(5):
        for tail, want in (("", preds), ("_spread", spreads)):
            with Image.open(tmp_path / f"run_img{i}{tail}.tif") as im:
                np.testing.assert_array_equal(np.asarray(im), want[f"img{i}"][0])
        with Image.open(tmp_path / f"run_img{i}_consistency.tif") as im:
            assert im.size == (24, 24)
            np.testing.assert_array_equal(np.asarray(im), scores[f"img{i}"].map[0])
    predict_images(_Positional(), ds, device="cuda", batch_size=2, out_dir=str(tmp_path / "plain"))
    assert sorted(p.name for p in (tmp_path / "plain").iterdir()) == [f"img{i}.tif" for i in range(5)]
    ds.crop_res = 41
    with pytest.raises(ValueError, match="multiple of the model's scale"):
        predict_images(_Positional(), ds, device="cuda", batch_size=2, out_dir=None, consistency=True)
    assert predict_images(_Positional(), ds, device="cuda", batch_size=2, out_dir=None)["img0"].shape == (1, 41, 41)


@pytest.mark.parametrize("norm", [False, True])
def test_test_metrics_rse_and_rsp(norm):
    from pssr2_amd.predict import predict_images, test_metrics
    ds = _Pairs(n=2, crop_res=48)
    default = test_metrics(_Positional(), ds, device="cuda", norm=norm, avg=False)
    assert set(default) == {"mse", "pixel", "psnr", "ssim"}
    pred = predict_images(_Positional(), ds, device="cuda", batch_size=1, out_dir=None)["img0"]
    for fit in R.FITS:
        got = test_metrics(_Positional(), ds, device="cuda", metrics=("psnr", "rse", "rsp"), norm=norm, avg=False, fit=fit)
        want = R.consistency_ref(ds.lrs[:1, :, :24, :24], pred[None], fit)
        assert got == {"psnr": default["psnr"], "rse": [want[3][0, 0]] * 2, "rsp": [want[4][0, 0]] * 2}      # every iteration: dataset[0]
    rse = R.consistency_ref(ds.lrs[:1, :, :24, :24], pred[None])[3][0, 0]      # the default fit is the affine one
    assert rse > 0 and test_metrics(_Positional(), ds, device="cuda", metrics="rse", norm=norm) == {"rse": rse}
    got8 = test_metrics(_Positional(), ds, device="cuda", metrics=("rse",), norm=norm, avg=False, ensemble=8)
    pred8 = predict_images(_Positional(), ds, device="cuda", batch_size=1, out_dir=None, ensemble=8)["img0"]
    assert got8 == {"rse": [R.consistency_ref(ds.lrs[:1, :, :24, :24], pred8[None])[3][0, 0]] * 2}


# ------------------------------------------------------------------------------------------------ a real model
def test_real_model_sheet_consistency_is_a_function_of_its_bytes():
    from oracle import model_ref as M
    from pssr2_amd.models import ResUNet
    from pssr2_amd.predict import predict_sheet
    model = ResUNet(hidden=[16, 32])
    model.load_state_dict(M.make_state_dict(hidden=(16, 32), seed=6))
    model.compute_dtype = torch.bfloat16
    yy, xx = np.mgrid[0:80, 0:72]
    lr = np.clip(110 + 80 * np.sin(yy / 6.0) * np.cos(xx / 5.0) + np.random.default_rng(3).normal(0, 4, size=yy.shape), 0, 255).astype(np.uint8)
    sheet, cons = predict_sheet(model, lr[None], tile_res=32, overlap=8, batch_size=4, cover=True, consistency=True)
    assert sheet.shape == (1, 320, 288) and cons.map.shape == (1, 80, 72)
    want = R.consistency_ref(lr[None, None], sheet[None])
    _same_stats(cons, tuple(v[0] for v in want))
