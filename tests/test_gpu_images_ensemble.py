"""The self-ensemble of predict_images / test_metrics and the spread maps: the three kernels (pssr_dihedral_batch_u8 / _f32,
pssr_ensemble_reduce_u8, pssr_spread_stack_u8) against the numpy restatements of tests/_ensemble_ref.py and against the kernels whose
composition they replace, the drivers through two probe models that are exact in float32, predict_sheet(spread=True), and a real model.
Every comparison is byte for byte."""
import math

import numpy as np
import pytest
import torch

import _blend_ref as B
import _ensemble_ref as R

pytestmark = pytest.mark.gpu

ENSEMBLES = (1, 2, 4, 8)
Y_CAP, X_CAP = 65535, 1024          # the grid caps of the block kernels: planes over blockIdx.y, 32 x 32 blocks over blockIdx.x


# ------------------------------------------------------------------------------------------------ forward turn
def _turn_case(n, m, s, E, dtype, seed=0):
    from pssr2_amd import ops
    x = np.random.default_rng(seed).integers(0, 256, size=(n, m, s, s), dtype=np.uint8)
    if dtype == "f32":
        x = x.astype(np.float32) + np.float32(0.25)                       # not representable in uint8: a float path that quantised would show
    got = ops.dihedral_batch(torch.tensor(x).cuda(), E)
    assert got.dtype == torch.float32 and got.shape == (n * E, m, s, s) and got.is_contiguous()
    np.testing.assert_array_equal(got.cpu().numpy(), R.members_ref(x, E))


@pytest.mark.parametrize("dtype", ["u8", "f32"])
@pytest.mark.parametrize("E", ENSEMBLES)
@pytest.mark.parametrize("n,m", [(1, 1), (3, 2)])
@pytest.mark.parametrize("s", [1, 10, 32, 33, 40])
def test_dihedral_batch_matches_numpy(s, n, m, E, dtype):
    _turn_case(n, m, s, E, dtype, seed=s)


@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_dihedral_batch_more_planes_than_the_grid(dtype):
    n, m = Y_CAP // 3 + 1, 3
    assert n * m > Y_CAP
    _turn_case(n, m, 1, 2, dtype)


@pytest.mark.parametrize("dtype", ["u8", "f32"])
def test_dihedral_batch_more_blocks_than_the_grid(dtype):
    s = 32 * 33
    assert (s // 32) ** 2 > X_CAP
    _turn_case(1, 1, s, 8, dtype)


def test_dihedral_batch_refuses_bad_arguments():
    from pssr2_amd import ops
    x = torch.zeros(2, 1, 8, 8, dtype=torch.uint8, device="cuda")
    with pytest.raises(RuntimeError, match="ensemble"):
        ops.dihedral_batch(x, 3)
    with pytest.raises(AssertionError):
        ops.dihedral_batch(torch.zeros(2, 1, 8, 9, device="cuda"), 2)


# ------------------------------------------------------------------------------------------------ reduce
def _floats(shape, seed):
    """float32 with everything the clip and the truncation can get wrong: negatives, values above 255, 254.999, -0.0, exact integers,
    +-1e9, and a few NaN."""
    rng = np.random.default_rng(seed)
    x = rng.uniform(-40.0, 300.0, size=shape).astype(np.float32)
    flat = x.reshape(-1)
    special = np.array([254.999, -0.0, 0.0, 1.0, 17.0, 254.0, 255.0, 255.5, 256.0, -3.0, 0.999, 1e9, -1e9, np.nan], dtype=np.float32)
    if flat.size >= special.size * 8:
        flat[rng.choice(flat.size, size=special.size * 8, replace=False)] = np.tile(special, 8)
    else:
        flat[:] = np.resize(special, flat.size)
    flat[::7] = np.floor(flat[::7])
    return x


def _reduce_case(n, c, s, E, seed=0):
    from pssr2_amd import ops
    y = _floats((n * E, c, s, s), seed)
    want_mean, want_spread = R.reduce_ref(y, E)
    dev = torch.tensor(y).cuda()
    mean, spread = ops.ensemble_reduce_u8(dev, E, spread=True)
    assert mean.shape == spread.shape == (n, c, s, s) and mean.dtype == spread.dtype == torch.uint8
    np.testing.assert_array_equal(mean.cpu().numpy(), want_mean)
    np.testing.assert_array_equal(spread.cpu().numpy(), want_spread)
    alone = ops.ensemble_reduce_u8(dev, E)
    assert torch.is_tensor(alone) and torch.equal(alone, mean)            # the spread pointer moves nothing
    # the composition it replaces: every member quantised and turned back into a uint8 buffer, reduced in torch integers
    q = torch.zeros(y.shape, dtype=torch.uint8, device="cuda")
    ops.clip_u8_dihedral(dev, q, E, 0)
    q = q.view(n, E, c, s, s).to(torch.int32)
    assert torch.equal(mean, (q.sum(1) // E).to(torch.uint8))
    assert torch.equal(spread, (q.amax(1) - q.amin(1)).to(torch.uint8))
    if E == 1:
        plain = torch.zeros(y.shape, dtype=torch.uint8, device="cuda")
        ops.clip_u8(dev, plain)
        assert torch.equal(mean, plain) and not spread.any()
    elif s > 1:
        assert spread.any()


@pytest.mark.parametrize("E", ENSEMBLES)
@pytest.mark.parametrize("n,c", [(1, 1), (3, 2)])
@pytest.mark.parametrize("s", [1, 10, 32, 33, 40])
def test_ensemble_reduce_matches_numpy_and_the_existing_kernels(s, n, c, E):
    _reduce_case(n, c, s, E, seed=s)


def test_ensemble_reduce_more_planes_than_the_grid():
    n, c = Y_CAP // 3 + 1, 3
    assert n * c > Y_CAP
    _reduce_case(n, c, 1, 2)


def test_ensemble_reduce_more_blocks_than_the_grid():
    _reduce_case(1, 1, 32 * 33, 8)


def test_ensemble_reduce_refuses_bad_arguments():
    from pssr2_amd import ops
    with pytest.raises(RuntimeError, match="ensemble"):
        ops.ensemble_reduce_u8(torch.zeros(6, 1, 8, 8, device="cuda"), 3)
    with pytest.raises(AssertionError):
        ops.ensemble_reduce_u8(torch.zeros(6, 1, 8, 8, device="cuda"), 4)


# ------------------------------------------------------------------------------------------------ sheet spread
# n_slices, c, n_rows, n_cols, S, O, M, crop (None: the whole stitched sheet)
STITCH_CASES = ([(2, 2, 3, 4, 12, 4, m, None) for m in (0, 1, 2, 3)]             # 2 M > O at M = 3: uncovered pixels
                + [(1, 1, 5, 5, 8, 6, m, None) for m in (0, 1)]                  # up to four tiles over a pixel per axis
                + [(1, 1, 1, 3, 12, 4, 1, None), (1, 1, 3, 1, 12, 4, 1, None)]   # no neighbour on an axis
                + [(1, 2, 2, 3, 12, 0, 0, None)]                                 # no overlap
                + [(2, 2, 3, 4, 12, 4, 1, (23, 30))]                             # a crop inside the 28 x 36 sheet
                + [(1, 1, 1, 2, 300, 40, 2, (300, 555))])                        # rows wider than one workgroup's 256 threads


@pytest.mark.parametrize("ensemble", [1, 8])
@pytest.mark.parametrize("case", STITCH_CASES, ids=lambda c: "-".join(str(v) for v in c[:7]) + ("-crop" if c[7] else ""))
def test_spread_stack_matches_numpy(case, ensemble):
    from pssr2_amd import ops
    n_slices, c, n_rows, n_cols, S, O, M, crop = case
    tiles = np.random.default_rng(21).integers(0, 256, size=(n_slices * n_rows * n_cols * ensemble, c, S, S), dtype=np.uint8)
    out_h, out_w = crop or (n_rows * (S - O) + O, n_cols * (S - O) + O)
    want = R.spread_stack_ref(tiles, n_slices, n_rows, n_cols, O, M, out_h, out_w, ensemble)
    dev = torch.tensor(tiles).cuda()
    got = ops.spread_stack_u8(dev, n_slices, n_rows, n_cols, O, M, out_h, out_w, ensemble)
    assert got.shape == (n_slices, c, out_h, out_w) and got.dtype == torch.uint8
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    if M == 3:                                                            # the gap stays 0, as in the stitched sheet
        full = np.full(tiles.shape, 255, dtype=np.uint8)
        gap = B.blend_ref(full, n_slices, n_rows, n_cols, O, M, out_h, out_w, "average", ensemble) == 0
        assert gap.any() and not want[gap].any()
    if O <= 2 * M and ensemble == 1:                                      # the margins leave one prediction per pixel at the most
        assert not want.any()
    else:
        assert want.any()


def test_spread_stack_refuses_a_crop_beyond_the_sheet():
    from pssr2_amd import ops
    dev = torch.zeros(3 * 3 * 8, 1, 64, 64, dtype=torch.uint8, device="cuda")
    assert ops.spread_stack_u8(dev, 1, 3, 3, 32, 0, 128, 128, 8).shape == (1, 1, 128, 128)
    with pytest.raises(RuntimeError, match="crop"):
        ops.spread_stack_u8(dev, 1, 3, 3, 32, 0, 129, 128, 8)
    with pytest.raises(RuntimeError, match="ensemble"):
        ops.spread_stack_u8(dev[:45], 1, 3, 3, 32, 0, 128, 128, 5)


# ------------------------------------------------------------------------------------------------ the drivers, with exact probes
class _Equivariant(torch.nn.Module):
    """0.5 * (sum of the frames) + 3.25, every pixel repeated 2 x 2: multiples of 0.25 far below 2**24, so exact in float32, and it
    commutes with every rotation and flip."""

    def forward(self, x):
        y = 0.5 * x.sum(1, keepdim=True) + 3.25
        return y.repeat_interleave(2, dim=-2).repeat_interleave(2, dim=-1)


class _Positional(_Equivariant):
    """... plus 3 col - 2 row of the tile-local output coordinate: not equivariant, so every member predicts something else."""

    def forward(self, x):
        y = super().forward(x)
        n = y.shape[-1]
        i = torch.arange(n, dtype=y.dtype, device=y.device)
        return y + 3 * i.view(1, 1, 1, n) - 2 * i.view(1, 1, n, 1)


def _probe_f64(lr, positional):
    """The two probes restated in float64 on [n, m, s, s]."""
    y = (0.5 * lr.astype(np.float64).sum(1, keepdims=True) + 3.25).repeat(2, axis=-2).repeat(2, axis=-1)
    if positional:
        i = np.arange(y.shape[-1], dtype=np.float64)
        y = y + 3 * i.reshape(1, 1, 1, -1) - 2 * i.reshape(1, 1, -1, 1)
    return y


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


def _same(a, b):
    assert list(a) == list(b)
    for k in a:
        assert a[k].dtype == b[k].dtype == np.uint8 and a[k].shape == b[k].shape
        np.testing.assert_array_equal(a[k], b[k])


@pytest.mark.parametrize("compact", [False, True])
def test_ensemble_of_an_equivariant_model_changes_nothing(compact):
    from pssr2_amd.predict import predict_images
    ds = _Pairs(compact=compact)
    one = predict_images(_Equivariant(), ds, device="cuda", batch_size=2, out_dir=None)
    assert list(one) == [f"img{i}" for i in range(5)] and one["img0"].shape == (1, 64, 64) and one["img0"].max() > one["img0"].min()
    for E in (2, 4, 8):
        preds, spreads = predict_images(_Equivariant(), ds, device="cuda", batch_size=2, out_dir=None, ensemble=E, spread=True)
        _same(preds, one)
        assert list(spreads) == list(one) and all(v.shape == (1, 64, 64) and v.dtype == np.uint8 and not v.any() for v in spreads.values())
        _same(predict_images(_Equivariant(), ds, device="cuda", batch_size=2, out_dir=None, ensemble=E), one)
    _same(predict_images(_Equivariant(), ds, device="cuda", batch_size=2, out_dir=None, ensemble=1), one)


@pytest.mark.parametrize("E", [2, 8])
@pytest.mark.parametrize("crop_res", [64, 40])
def test_positional_probe_against_numpy(E, crop_res):
    from pssr2_amd.predict import predict_images
    ds = _Pairs(crop_res=crop_res)
    members = R.members_ref(ds.lrs, E)
    y = _probe_f64(members, True)
    assert any((B.U_d(R.clip_u8(y[d]), d) != R.clip_u8(y[0])).any() for d in range(1, E))      # the members do differ
    mean, spread = R.reduce_ref(y, E)
    assert spread.any()
    want = ({f"img{i}": mean[i, :, :crop_res, :crop_res] for i in range(5)}, {f"img{i}": spread[i, :, :crop_res, :crop_res] for i in range(5)})
    for batch in (1, 2, 3, 64):                                           # the batch size moves nothing
        preds, spreads = predict_images(_Positional(), ds, device="cuda", batch_size=batch, out_dir=None, ensemble=E, spread=True)
        _same(preds, want[0])
        _same(spreads, want[1])
    ds.compact = True
    _same(predict_images(_Positional(), ds, device="cuda", batch_size=2, out_dir=None, ensemble=E), want[0])


def test_normalised_ensemble_and_files(tmp_path):
    from PIL import Image
    from pssr2_amd import ops
    from pssr2_amd.predict import predict_images
    ds = _Pairs(crop_res=48)
    preds, spreads = predict_images(_Positional(), ds, device="cuda", batch_size=2, out_dir=None, ensemble=4, spread=True)
    predict_images(_Positional(), ds, device="cuda", batch_size=2, out_dir=str(tmp_path), prefix="run", ensemble=4, spread=True)
    assert sorted(p.name for p in tmp_path.iterdir()) == sorted([f"run_img{i}.tif" for i in range(5)] + [f"run_img{i}_spread.tif" for i in range(5)])
    for i in range(5):
        with Image.open(tmp_path / f"run_img{i}.tif") as im:
            assert im.size == (48, 48)
            np.testing.assert_array_equal(np.asarray(im), preds[f"img{i}"][0])
        with Image.open(tmp_path / f"run_img{i}_spread.tif") as im:
            assert im.size == (48, 48)
            np.testing.assert_array_equal(np.asarray(im), spreads[f"img{i}"][0])
    predict_images(_Positional(), ds, device="cuda", batch_size=2, out_dir=str(tmp_path / "plain"), ensemble=4)
    assert sorted(p.name for p in (tmp_path / "plain").iterdir()) == [f"img{i}.tif" for i in range(5)]
    # norm=True normalises the ensembled prediction (whole, then cropped, as the plain call does) and leaves the spread alone
    mean, _ = R.reduce_ref(_probe_f64(R.members_ref(ds.lrs, 4), True), 4)
    normed, same_spreads = predict_images(_Positional(), ds, device="cuda", batch_size=5, out_dir=None, norm=True, ensemble=4, spread=True)
    _, hat = ops.normalize_preds_u8(torch.tensor(ds.hrs).cuda(), torch.tensor(mean).cuda())
    _same(normed, {f"img{i}": hat[i, :, :48, :48].cpu().numpy() for i in range(5)})
    _same(same_spreads, spreads)


def _metrics_of(hr, hat):
    """test_metrics' figures from ops.image_metrics_u8 for one uint8 pair [1, 1, H, W] on the device."""
    from pssr2_amd import ops
    from pssr2_amd.util import pixel_metric
    stats = ops.image_metrics_u8(hr, hat).reshape(1, 1, 2).cpu()
    err = float(stats[0, :, 0].sum()) / hr[0].numel()
    return {"mse": err / 255 ** 2, "pixel": pixel_metric(err / 255 ** 2, 255), "psnr": 10 * math.log10(255 ** 2 / err), "ssim": float(stats[0, 0, 1])}


@pytest.mark.parametrize("norm", [False, True])
def test_test_metrics_of_the_ensemble(norm):
    from pssr2_amd import ops
    from pssr2_amd.predict import test_metrics
    ds = _Pairs(n=2)
    one = test_metrics(_Equivariant(), ds, device="cuda", norm=norm, avg=False)
    assert len(one["psnr"]) == 2 and set(one) == {"mse", "pixel", "psnr", "ssim"}
    assert test_metrics(_Equivariant(), ds, device="cuda", norm=norm, avg=False, ensemble=8) == one
    assert test_metrics(_Equivariant(), ds, device="cuda", norm=norm, avg=False, ensemble=1) == one
    mean, _ = R.reduce_ref(_probe_f64(R.members_ref(ds.lrs[:1], 8), True), 8)
    hr, hat = torch.tensor(ds.hrs[:1]).cuda(), torch.tensor(mean).cuda()
    if norm:
        hr, hat = ops.normalize_preds_u8(hr, hat)
    want = _metrics_of(hr, hat)
    got = test_metrics(_Positional(), ds, device="cuda", norm=norm, avg=False, ensemble=8)
    assert got == {k: [v, v] for k, v in want.items()}                    # every iteration evaluates dataset[0], as upstream
    assert got != test_metrics(_Positional(), ds, device="cuda", norm=norm, avg=False)
    assert test_metrics(_Positional(), ds, device="cuda", norm=norm, ensemble=8) == want


def test_ensemble_needs_square_items_and_outputs():
    from pssr2_amd.predict import _ensemble_pred

    class Wide(torch.nn.Module):
        def forward(self, x):
            return x[..., :-1]

    with pytest.raises(ValueError, match="square"):
        _ensemble_pred(_Equivariant(), torch.zeros(2, 1, 8, 12, device="cuda"), 4, 2)
    with pytest.raises(ValueError, match="square"):
        _ensemble_pred(Wide(), torch.zeros(2, 1, 8, 8, device="cuda"), 4, 2)


# ------------------------------------------------------------------------------------------------ predict_sheet(spread=True)
@pytest.fixture(scope="module")
def probe_stack():
    return np.random.default_rng(7).integers(0, 128, size=(5, 45, 38), dtype=np.uint8)


def _restated_sheet_members(stack, positional, tile, stride, n_rows, n_cols, n_slices, m, step, ens):
    """cut -> probe -> truncate -> turn back, restated: dihedral_tiles_ref, the probe in float64, U_d."""
    lr = B.dihedral_tiles_ref(stack, m, step, tile, stride, n_rows, n_cols, n_slices, ens)
    q = R.clip_u8(_probe_f64(lr, positional))
    return np.stack([B.U_d(q[g], g % ens) for g in range(len(q))])


# keywords, frames of the stack used, (m, step, n_slices), blend, ensemble
SHEET_PATHS = {
    "plain": (dict(), 1, (1, 1, 1), "average", 1),
    "cover": (dict(cover=True), 1, (1, 1, 1), "average", 1),
    "stacked": (dict(n_frames=3, slide=True), 5, (3, 1, 3), "average", 1),
    "mixed": (dict(cover=True, blend="linear", ensemble=8), 3, (3, 3, 1), "linear", 8),
    "mixed_stacked": (dict(n_frames=3, slide=True, blend="linear", ensemble=2), 5, (3, 1, 3), "linear", 2),
}


@pytest.mark.parametrize("path", list(SHEET_PATHS))
def test_predict_sheet_spread_on_every_path(probe_stack, path):
    from pssr2_amd.predict import predict_sheet
    kw, frames, (m, step, n_slices), blend, ens = SHEET_PATHS[path]
    stack = probe_stack[:frames]
    f, h, w = stack.shape
    tile, overlap, margin = 16, 4, 1
    stride = tile - overlap
    common = dict(tile_res=tile, overlap=overlap, margin=margin, batch_size=5, **kw)
    sheet_only = predict_sheet(_Positional(), stack, **common)
    sheet, spread = predict_sheet(_Positional(), stack, spread=True, **common)
    np.testing.assert_array_equal(sheet, sheet_only)                      # the sheet does not change
    assert spread.shape == sheet.shape and spread.dtype == np.uint8
    cover = bool(kw.get("cover"))
    n_rows, n_cols = (B.grid(h, tile, stride), B.grid(w, tile, stride)) if cover else ((h - tile) // stride + 1, (w - tile) // stride + 1)
    out_h, out_w = (2 * h, 2 * w) if cover else (2 * (n_rows * stride + overlap), 2 * (n_cols * stride + overlap))
    preds = _restated_sheet_members(stack, True, tile, stride, n_rows, n_cols, n_slices, m, step, ens)
    want_sheet = B.blend_ref(preds, n_slices, n_rows, n_cols, overlap * 2, margin, out_h, out_w, blend, ens)
    want = R.spread_stack_ref(preds, n_slices, n_rows, n_cols, overlap * 2, margin, out_h, out_w, ens)
    stacked = "n_frames" in kw
    np.testing.assert_array_equal(sheet, want_sheet if stacked else want_sheet[0])
    np.testing.assert_array_equal(spread, want if stacked else want[0])
    assert spread.any()                                                   # the positional probe disagrees with itself at every seam
    dev_sheet, dev_spread = predict_sheet(_Positional(), torch.tensor(stack), spread=True, to_numpy=False, **common)
    assert dev_sheet.is_cuda and dev_spread.is_cuda and dev_spread.dtype == torch.uint8
    np.testing.assert_array_equal(dev_spread.cpu().numpy(), spread)


def test_predict_sheet_spread_of_an_equivariant_model_without_overlap_is_zero(probe_stack):
    from pssr2_amd.predict import predict_sheet
    sheet, spread = predict_sheet(_Equivariant(), probe_stack[:1], tile_res=16, overlap=0, batch_size=7, cover=True, ensemble=8, spread=True)
    assert sheet.shape == spread.shape == (1, 90, 76) and sheet.max() > sheet.min()
    assert not spread.any()
    # ... and with an overlap too: every tile predicts the same value for a pixel it shares
    sheet, spread = predict_sheet(_Equivariant(), probe_stack[:1], tile_res=16, overlap=4, batch_size=7, cover=True, ensemble=8, spread=True)
    assert not spread.any()


# ------------------------------------------------------------------------------------------------ a real model
def test_real_model_ensemble_against_its_own_members():
    from oracle import model_ref as M
    from pssr2_amd import ops
    from pssr2_amd.models import ResUNet
    from pssr2_amd.predict import predict_images
    model = ResUNet(hidden=[16, 32])
    model.load_state_dict(M.make_state_dict(hidden=(16, 32), seed=6))
    model.compute_dtype = torch.bfloat16
    ds, batch, E = _Pairs(n=5, seed=3, crop_res=128, scale=4), 3, 4
    ds.lrs = np.random.default_rng(3).integers(0, 256, size=ds.lrs.shape, dtype=np.uint8)
    preds, spreads = predict_images(model, ds, device="cuda", batch_size=batch, out_dir=None, ensemble=E, spread=True)
    assert list(preds) == list(spreads) == [f"img{i}" for i in range(5)]
    model.cuda().eval()
    # the documented chunking: per batch of the loop, the n * E members in sequence order in chunks of at most `batch` items
    with torch.no_grad():
        for i0 in range(0, 5, batch):
            lr = torch.tensor(ds.lrs[i0:i0 + batch]).float().cuda()
            members = ops.dihedral_batch(lr, E)
            y = np.concatenate([model(members[g0:g0 + batch]).contiguous().float().cpu().numpy() for g0 in range(0, len(members), batch)])
            assert y.shape == (len(lr) * E, 1, 128, 128)
            mean, spread = R.reduce_ref(y, E)
            assert spread.any()
            for j in range(len(lr)):
                np.testing.assert_array_equal(preds[f"img{i0 + j}"], mean[j])
                np.testing.assert_array_equal(spreads[f"img{i0 + j}"], spread[j])
