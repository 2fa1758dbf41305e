"""predict_sheet over sheets of any size (``cover``) and over frame stacks (``n_frames`` / ``slide``): the two stack kernels of
csrc/tiles.hip against numpy restatements, the plumbing against an exact probe model, and a real model against the calls and the
dataset pipeline the new arguments replace.  Every comparison is byte for byte."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu


def _padded(stack, size, stride, tiles_y, tiles_x):
    """The stack reflect-padded at the bottom / right to the extent of a tiles_y x tiles_x grid (np.pad semantics)."""
    f, h, w = stack.shape
    ext_h, ext_w = (tiles_y - 1) * stride + size, (tiles_x - 1) * stride + size
    return np.pad(stack, ((0, 0), (0, max(ext_h - h, 0)), (0, max(ext_w - w, 0))), mode="reflect")


def _stack_tiles_ref(stack, m, frame_step, size, stride, tiles_y, tiles_x, n_slices):
    """float32 [n_slices * tiles_y * tiles_x, m, size, size], slice-major: pad, slice the windows, cast."""
    pad = _padded(stack, size, stride, tiles_y, tiles_x)
    return np.stack([pad[k * frame_step:k * frame_step + m, ty * stride:ty * stride + size, tx * stride:tx * stride + size]
                     for k in range(n_slices) for ty in range(tiles_y) for tx in range(tiles_x)]).astype(np.float32)


def _grid(n, size, stride):
    return -(-max(n - size, 0) // stride) + 1


# frames, h, w, m, frame_step, size, stride, n_slices
STACK_CASES = {
    "slide_fold_both": (7, 45, 38, 3, 1, 16, 12, 5),
    "disjoint_fold_both": (7, 45, 38, 3, 3, 16, 12, 2),
    "repeated_fold_one_tile": (2, 5, 9, 2, 2, 16, 12, 1),
    "scalar_path_odd_rows": (1, 50, 41, 1, 1, 10, 7, 1),
}


@pytest.mark.parametrize("case", list(STACK_CASES))
def test_stack_tiles_match_numpy(case):
    from pssr2_amd import ops
    frames, h, w, m, frame_step, size, stride, n_slices = STACK_CASES[case]
    stack = np.random.default_rng(1).integers(0, 256, size=(frames, h, w), dtype=np.uint8)
    tiles_y, tiles_x = _grid(h, size, stride), _grid(w, size, stride)
    want = _stack_tiles_ref(stack, m, frame_step, size, stride, tiles_y, tiles_x, n_slices)
    n = n_slices * tiles_y * tiles_x
    assert want.shape == (n, m, size, size)
    dev = torch.tensor(stack).cuda()
    got = ops.stack_tiles_u8(dev, m, frame_step, size, stride, tiles_y, tiles_x, 0, n)
    assert got.dtype == torch.float32
    np.testing.assert_array_equal(got.cpu().numpy(), want)
    if case == "slide_fold_both":      # 12 tiles per slice fetched in fives: ranges that straddle the slice boundaries
        pieces = [ops.stack_tiles_u8(dev, m, frame_step, size, stride, tiles_y, tiles_x, t0, min(5, n - t0)) for t0 in range(0, n, 5)]
        np.testing.assert_array_equal(torch.cat(pieces).cpu().numpy(), want)


def test_stack_tiles_without_fold_equal_sliding_tiles():
    from pssr2_amd import ops
    sheet = np.random.default_rng(2).integers(0, 256, size=(3, 45, 38), dtype=np.uint8)
    dev = torch.tensor(sheet).cuda()
    tiles_y, tiles_x = (45 - 16) // 12 + 1, (38 - 16) // 12 + 1               # whole windows only: 3 x 2, nothing reflected
    want = ops.sliding_tiles_u8(dev, 16, 12, 0, tiles_y * tiles_x)
    got = ops.stack_tiles_u8(dev, 3, 3, 16, 12, tiles_y, tiles_x, 0, tiles_y * tiles_x)
    np.testing.assert_array_equal(got.cpu().numpy(), want.cpu().numpy())
    np.testing.assert_array_equal(got.cpu().numpy(), _stack_tiles_ref(sheet, 3, 3, 16, 12, tiles_y, tiles_x, 1))
    with pytest.raises(RuntimeError, match="leaves the stack"):
        ops.stack_tiles_u8(dev, 3, 3, 16, 12, tiles_y, tiles_x, 0, tiles_y * tiles_x + 1)


@pytest.mark.parametrize("margin", [0, 3])
def test_patch_stack_matches_patch_images(margin):
    from pssr2_amd import ops
    from pssr2_amd.util import _patch_images
    n_slices, c, n_rows, n_cols, size, ov = 3, 2, 3, 4, 32, 8
    tiles = np.random.default_rng(4).integers(0, 256, size=(n_slices * n_rows * n_cols, c, size, size), dtype=np.uint8)
    dev = torch.tensor(tiles).cuda()
    full_h, full_w = n_rows * (size - ov) + ov, n_cols * (size - ov) + ov
    per = n_rows * n_cols
    want = np.stack([np.stack([np.asarray(_patch_images(tiles[k * per:(k + 1) * per, ch], n_cols, n_rows, ov, margin), dtype=np.uint8)
                               for ch in range(c)]) for k in range(n_slices)])
    assert want.shape == (n_slices, c, full_h, full_w) == (3, 2, 80, 104)
    for out_h, out_w in ((full_h, full_w), (70, 95)):
        got = ops.patch_stack_u8(dev, n_slices, n_rows, n_cols, ov, margin, out_h, out_w)
        assert got.shape == (n_slices, c, out_h, out_w) and got.dtype == torch.uint8
        np.testing.assert_array_equal(got.cpu().numpy(), want[:, :, :out_h, :out_w])
    full = ops.patch_stack_u8(dev, n_slices, n_rows, n_cols, ov, margin, full_h, full_w).cpu().numpy()
    for k in range(n_slices):
        np.testing.assert_array_equal(full[k], ops.patch_tiles_u8(dev[k * per:(k + 1) * per], n_rows, n_cols, ov, margin).cpu().numpy())
    with pytest.raises(RuntimeError, match="crop"):
        ops.patch_stack_u8(dev, n_slices, n_rows, n_cols, ov, margin, full_h + 1, full_w)


# ------------------------------------------------------------------------------------------------ plumbing, with an exact probe
class _Probe(torch.nn.Module):
    """(x * w).sum(1) / 4 with small integer weights, 2x nearest up-sampling: multiples of 0.25 far below 2**24, so float32 is exact
    whatever the order of summation, and each output pixel tells which frames and which sheet pixel it came from."""

    def forward(self, x):
        w = torch.tensor(_probe_weights(x.shape[1]), dtype=x.dtype, device=x.device).view(1, -1, 1, 1)
        y = (x * w).sum(1, keepdim=True) / 4
        return y.repeat_interleave(2, dim=-2).repeat_interleave(2, dim=-1)


def _probe_weights(c):
    return [1, 2, 1] if c == 3 else [1 + (i * 2) % 3 for i in range(c)]


def _probe_expected(stack, tile, overlap, margin, n_frames, slide, cover):
    """numpy: pad, cut, apply the probe, truncate to uint8, _patch_images(..., overlap * 2, margin), cast, crop."""
    from pssr2_amd.util import _patch_images
    frames, h, w = stack.shape
    stride = tile - overlap
    m = frames if n_frames == -1 else n_frames
    step = 1 if slide else m
    n_slices = 1 if n_frames == -1 else (frames - m + 1 if slide else frames // m)
    n_rows, n_cols = (_grid(h, tile, stride), _grid(w, tile, stride)) if cover else ((h - tile) // stride + 1, (w - tile) // stride + 1)
    lr = _stack_tiles_ref(stack, m, step, tile, stride, n_rows, n_cols, n_slices).astype(np.float64)
    y = (lr * np.asarray(_probe_weights(m), dtype=np.float64).reshape(1, -1, 1, 1)).sum(1) / 4
    y = np.clip(y.repeat(2, axis=-2).repeat(2, axis=-1), 0, 255).astype(np.uint8)
    per = n_rows * n_cols
    out = np.stack([np.asarray(_patch_images(y[k * per:(k + 1) * per], n_cols, n_rows, overlap * 2, margin), dtype=np.uint8)[None]
                    for k in range(n_slices)])
    if cover:
        out = out[..., :h * 2, :w * 2]
    return out[0] if n_frames == -1 else out


@pytest.fixture(scope="module")
def probe_stack():
    # values up to 63: the weighted sums / 4 stay below 256, so the uint8 truncation is of distinct values, not of a clipped plateau
    stack = np.random.default_rng(7).integers(0, 64, size=(6, 45, 38), dtype=np.uint8)
    return stack


@pytest.mark.parametrize("n_frames,slide,cover,shape", [(3, True, True, (4, 1, 90, 76)), (3, False, True, (2, 1, 90, 76)),
                                                        (-1, False, True, (1, 90, 76)), (3, True, False, (4, 1, 80, 56))])
def test_predict_sheet_plumbing_is_exact(probe_stack, n_frames, slide, cover, shape):
    from pssr2_amd.predict import predict_sheet
    got = predict_sheet(_Probe(), probe_stack, tile_res=16, overlap=4, margin=2, batch_size=7, n_frames=n_frames, slide=slide, cover=cover)
    assert got.shape == shape and got.dtype == np.uint8
    np.testing.assert_array_equal(got, _probe_expected(probe_stack, 16, 4, 2, n_frames, slide, cover))
    dev = predict_sheet(_Probe(), torch.tensor(probe_stack), tile_res=16, overlap=4, margin=2, batch_size=64, n_frames=n_frames, slide=slide,
                        cover=cover, to_numpy=False)
    assert dev.is_cuda
    np.testing.assert_array_equal(dev.cpu().numpy(), got)                   # the batch size moves nothing


def test_predict_sheet_covers_a_sheet_smaller_than_a_tile():
    from pssr2_amd.predict import predict_sheet
    sheet = np.random.default_rng(8).integers(0, 64, size=(1, 5, 9), dtype=np.uint8)
    got = predict_sheet(_Probe(), sheet, tile_res=16, overlap=4, margin=2, cover=True)
    assert got.shape == (1, 10, 18)
    np.testing.assert_array_equal(got, _probe_expected(sheet, 16, 4, 2, -1, False, True))
    np.testing.assert_array_equal(got[0], (sheet[0] // 4).repeat(2, axis=0).repeat(2, axis=1))     # one tile: the probe of the sheet itself


# ------------------------------------------------------------------------------------------------ a real model
def _resunet(channels=1, seed=None):
    from pssr2_amd.models import ResUNet
    if seed is None:
        from oracle import model_ref as M
        model = ResUNet(hidden=[16, 32])
        model.load_state_dict(M.make_state_dict(hidden=(16, 32), seed=6))
    else:
        torch.manual_seed(seed)
        model = ResUNet(channels=channels, hidden=[16, 32])
    model.compute_dtype = torch.bfloat16
    return model


def test_cover_equals_the_host_padded_sheet():
    from pssr2_amd.predict import predict_sheet
    model = _resunet()
    sheet = np.random.default_rng(3).integers(0, 256, size=(1, 100, 90), dtype=np.uint8)
    kw = dict(tile_res=32, overlap=8, margin=3, batch_size=7)
    padded = np.pad(sheet, ((0, 0), (0, 4), (0, 14)), mode="reflect")
    assert padded.shape == (1, 104, 104)
    want = predict_sheet(model, padded, **kw)
    assert want.shape == (1, 416, 416)
    got = predict_sheet(model, sheet, cover=True, **kw)
    assert got.shape == (1, 400, 360)
    np.testing.assert_array_equal(got, want[:, :400, :360])
    fits = np.random.default_rng(5).integers(0, 256, size=(1, 104, 80), dtype=np.uint8)      # on the grid already: nothing to extend
    np.testing.assert_array_equal(predict_sheet(model, fits, cover=True, **kw), predict_sheet(model, fits, **kw))


def test_stack_equals_per_slice_calls_and_the_dataset_pipeline():
    from pssr2_amd.data import SlidingSheetDataset
    from pssr2_amd.predict import predict_images, predict_sheet
    from pssr2_amd.util import _patch_images
    model = _resunet(channels=[3, 1], seed=12)
    stack = np.random.default_rng(9).integers(0, 256, size=(5, 56, 56), dtype=np.uint8)
    kw = dict(tile_res=32, overlap=8, batch_size=4)               # 2 x 2 tiles per slice: every batch is one slice's four tiles
    got = predict_sheet(model, stack, n_frames=3, slide=True, **kw)
    assert got.shape == (3, 1, 224, 224) and got.dtype == np.uint8
    np.testing.assert_array_equal(got, np.stack([predict_sheet(model, stack[k:k + 3], **kw) for k in range(3)]))
    ds = SlidingSheetDataset([stack], 32, -1, None, 8, n_frames=3, slide=True, val_split=1)
    assert len(ds) == 12
    preds = predict_images(model, ds, device="cuda", batch_size=4, out_dir=None)
    for k in range(3):
        batched = np.asarray([preds[f"sheet0_{t}_{k}"].squeeze() for t in range(4)])
        np.testing.assert_array_equal(got[k, 0], np.asarray(_patch_images(batched, 2, 2, 8 * 4, 0), dtype=np.uint8))


# ------------------------------------------------------------------------------------------------ errors
def test_predict_sheet_errors():
    from pssr2_amd.predict import predict_sheet
    probe = _Probe()
    sheet = np.zeros((2, 40, 40), dtype=np.uint8)
    with pytest.raises(ValueError, match="2 frames"):
        predict_sheet(probe, sheet, tile_res=16, overlap=4, n_frames=3)
    with pytest.raises(ValueError, match="smaller than one tile"):
        predict_sheet(probe, np.zeros((1, 12, 40), dtype=np.uint8), tile_res=16, overlap=4)
    for shape in ((1, 1, 40), (1, 40, 1)):
        with pytest.raises(ValueError, match="length 1"):
            predict_sheet(probe, np.zeros(shape, dtype=np.uint8), tile_res=16, overlap=4, cover=True)
    for cover in (False, True):
        with pytest.raises(ValueError, match="margin"):
            predict_sheet(probe, sheet, tile_res=16, overlap=4, margin=5, cover=cover)
