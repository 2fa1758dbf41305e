"""pssr_collage_rows_u8 against the reference's own collage bytes and a numpy restatement, predict_collage against a composition the
test builds from ``_pred_array`` / ``normalize_preds`` and Pillow, preprocess_dataset on the device datasets against the host ones.
Everything here is bit-exact."""
import random
import struct

import numpy as np
import pytest
import torch

from _collage_ref import compose, to_u8

pytestmark = pytest.mark.gpu

FILL = 0xAB


# ------------------------------------------------------------------------------------------------ the reference's bytes
@pytest.mark.parametrize("case", ["a", "b", "c", "d", "e"])
def test_collage_row_reproduces_the_reference(golden, case):
    """tests/golden/collage.npz: the reference's ``_collage_preds(norm=False)`` on float inputs in [-20, 280]."""
    from pssr2_amd.predict import _collage_row
    g = golden("collage.npz")
    crop_res, lr_scale = (int(v) for v in g[f"{case}/meta"])
    want = g[f"{case}/collage"]
    lr, hr_hat = torch.from_numpy(g[f"{case}/lr"]).cuda(), torch.from_numpy(g[f"{case}/hr_hat"]).cuda()
    hr = torch.from_numpy(g[f"{case}/hr"]).cuda() if f"{case}/hr" in g.files else None
    assert want.shape == (crop_res, crop_res * (2 if hr is None else 3))
    canvas = torch.full(want.shape, FILL, dtype=torch.uint8, device="cuda")
    _collage_row(canvas, 0, lr, hr_hat, hr, False, crop_res, lr_scale)
    assert np.array_equal(canvas.cpu().numpy(), want)


# ------------------------------------------------------------------------------------------------ the kernel against numpy
def _sources(h, w, sh, sw, pad, seed=0):
    """Three images, three panels of h x w: uint8 [3, sh, sw] enlarged through tables, float32 and uint8 identity panels that are crops
    of [3, h + 2, w + pad] arrays (row pitch w + pad).  Returns the numpy panels and the matching device panels."""
    from pssr2_amd.ops import nearest_index
    r = np.random.default_rng(seed)
    low = r.integers(0, 256, (3, sh, sw), dtype=np.uint8)
    mid = r.uniform(-20, 280, (3, h + 2, w + pad)).astype(np.float32)
    top = r.integers(0, 256, (3, h + 2, w + pad), dtype=np.uint8)
    yi, xi = nearest_index(sh, h), nearest_index(sw, w)
    host = [(low, yi, xi), mid[:, :h, :w], top[:, :h, :w]]
    dev = [(torch.from_numpy(low).cuda(), torch.from_numpy(yi).cuda(), torch.from_numpy(xi).cuda()),
           torch.from_numpy(mid).cuda()[:, :h, :w], torch.from_numpy(top).cuda()[:, :h, :w]]
    return host, dev


def _run(dev, h, w, n_panels=3, canvas=None):
    """Rows 1..3 of a five-slot canvas prefilled with 0xAB (row0 = 1, one spare slot at the end)."""
    from pssr2_amd import ops
    if canvas is None:
        canvas = torch.full((5 * h, n_panels * w), FILL, dtype=torch.uint8, device="cuda")
    ops.collage_rows_u8(dev, canvas, 1)
    return canvas.cpu().numpy()


@pytest.mark.parametrize("h,w,sh,sw,pad", [(32, 32, 8, 8, 16), (30, 30, 7, 7, 2), (32, 48, 8, 12, 0), (32, 32, 8, 8, 3), (48, 32, 16, 11, 16)],
                         ids=["vec-pitch48", "scalar-w30", "32x48", "vec-misaligned-rows", "48x32"])
def test_three_panels_three_images(h, w, sh, sw, pad):
    host, dev = _sources(h, w, sh, sw, pad)
    blank = np.full((5 * h, 3 * w), FILL, dtype=np.uint8)
    got, want = _run(dev, h, w), compose(blank, host, 1)
    assert np.array_equal(got[h:4 * h], want[h:4 * h])
    assert (got[:h] == FILL).all() and (got[4 * h:] == FILL).all()          # bytes outside the three rows are untouched
    assert len(np.unique(got[h:4 * h, :w])) > 50 and len(np.unique(got[h:4 * h, w:2 * w])) > 50


@pytest.mark.parametrize("n_panels", [1, 2])
def test_fewer_panels_and_a_wider_canvas(n_panels):
    host, dev = _sources(32, 32, 8, 8, 16, seed=1)
    canvas = torch.full((5 * 32, 112), FILL, dtype=torch.uint8, device="cuda")          # pitch 112 > n_panels * 32
    got = _run(dev[:n_panels], 32, 32, n_panels, canvas)
    assert np.array_equal(got, compose(np.full((160, 112), FILL, dtype=np.uint8), host[:n_panels], 1))


def test_misaligned_canvas_and_source_views():
    """A canvas view and a source view that start one byte into their buffers: byte accesses, the same bytes."""
    h = w = 32
    host, dev = _sources(h, w, 8, 8, 16, seed=2)
    want = _run(dev, h, w)
    buf = torch.full((5 * h * 3 * w + 16,), FILL, dtype=torch.uint8, device="cuda")
    view = buf[1:1 + 5 * h * 3 * w].view(5 * h, 3 * w)
    assert view.data_ptr() % 16 == 1
    assert np.array_equal(_run(dev, h, w, canvas=view), want)
    assert int(buf[0]) == FILL and (buf[1 + 5 * h * 3 * w:] == FILL).all()
    top = dev[2].contiguous()
    shifted = torch.empty(top.numel() + 16, dtype=torch.uint8, device="cuda")[1:1 + top.numel()].view(top.shape)
    shifted.copy_(top)
    assert shifted.data_ptr() % 16 == 1
    assert np.array_equal(_run([dev[0], dev[1], shifted], h, w), want)


@pytest.mark.parametrize("w", [32, 30])
def test_float_sources_clip_and_truncate(w):
    """-0.5 -> 0, 0.999 -> 0, 254.999 -> 254, 255.5 -> 255, 300 -> 255, through the identity loads and through a table."""
    from pssr2_amd import ops
    special = np.array([-0.5, 0.999, 254.999, 255.5, 300.0, 1.0, 255.0, -300.0], dtype=np.float32)
    src = np.tile(special, 3 * w * w // 8 + 1)[:3 * w * w].reshape(3, w, w)
    assert np.array_equal(to_u8(special), [0, 0, 254, 255, 255, 1, 255, 0])
    dev = torch.from_numpy(src).cuda()
    flip = np.arange(w - 1, -1, -1, dtype=np.int32)
    tables = torch.from_numpy(flip).cuda()
    canvas = torch.full((3 * w, 2 * w), FILL, dtype=torch.uint8, device="cuda")
    ops.collage_rows_u8([dev, (dev, tables, tables)], canvas, 0)
    assert np.array_equal(canvas.cpu().numpy(), compose(np.zeros((3 * w, 2 * w), np.uint8), [src, (src, flip, flip)], 0))


@pytest.mark.parametrize("w,sw", [(32, 8), (30, 7)])
def test_table_entries_outside_the_source_give_zero(w, sw):
    from pssr2_amd import ops
    host, dev = _sources(w, w, sw, sw, 0, seed=3)
    good = _run(dev, w, w)
    yi, xi = host[0][1].copy(), host[0][2].copy()
    xi[5], xi[w - 2], yi[3], yi[w - 1] = sw, -1, sw, -1
    bad = (dev[0][0], torch.from_numpy(yi).cuda(), torch.from_numpy(xi).cuda())
    got = _run([bad, dev[1], dev[2]], w, w)
    assert np.array_equal(got, compose(np.full(good.shape, FILL, np.uint8), [(host[0][0], yi, xi), host[1], host[2]], 1))
    rows = np.zeros(5 * w, dtype=bool)
    cols = np.zeros(3 * w, dtype=bool)
    for i in (1, 2, 3):
        rows[[i * w + 3, i * w + w - 1]] = True
    cols[[5, w - 2]] = True
    hit = (rows[:, None] & (np.arange(3 * w) < w)[None, :]) | ((np.arange(5 * w) >= w) & (np.arange(5 * w) < 4 * w))[:, None] & cols[None, :]
    assert (got[hit] == 0).all() and np.array_equal(got[~hit], good[~hit])
    assert (good[hit] != 0).any()
    # the identity past the end of a source smaller than the panel: zeros, nothing read
    small = torch.from_numpy(host[2][:, :w - 3, :w - 5].copy()).cuda()
    yi_id, xi_id = torch.arange(w, dtype=torch.int32, device="cuda"), torch.arange(w, dtype=torch.int32, device="cuda")
    canvas = torch.full((3 * w, w), FILL, dtype=torch.uint8, device="cuda")
    ops.collage_rows_u8([(small, yi_id, xi_id)], canvas, 0)
    want = np.zeros((3, w, w), np.uint8)
    want[:, :w - 3, :w - 5] = host[2][:, :w - 3, :w - 5]
    assert np.array_equal(canvas.cpu().numpy(), want.reshape(3 * w, w))


def test_ops_wrapper_rejects_what_does_not_fit():
    from pssr2_amd import ops
    _, dev = _sources(32, 32, 8, 8, 0)
    canvas = torch.zeros(4 * 32, 96, dtype=torch.uint8, device="cuda")
    with pytest.raises(ValueError, match="do not fit"):
        ops.collage_rows_u8(dev, canvas, 2)                              # rows 2..4 of a four-slot canvas
    with pytest.raises(ValueError, match="do not fit"):
        ops.collage_rows_u8(dev, canvas[:, :95], 0)
    with pytest.raises(ValueError, match="one index table"):
        ops.collage_rows_u8([(dev[0][0], dev[0][1], None)], canvas, 0)
    with pytest.raises(ValueError, match="differ"):
        ops.collage_rows_u8([dev[1], dev[2][:, :16]], canvas, 0)
    with pytest.raises(ValueError, match="1 to 3"):
        ops.collage_rows_u8([], canvas, 0)
    assert int(canvas.sum()) == 0


# ------------------------------------------------------------------------------------------------ predict_collage
@pytest.fixture(scope="module")
def tiles():
    from pssr2_amd.data import synthetic_em_tile
    return np.stack([synthetic_em_tile(i, 64) for i in range(6)])


@pytest.fixture(scope="module")
def model():
    from pssr2_amd.models import ResUNet
    torch.manual_seed(0)
    return ResUNet(hidden=[16, 32]).cuda().eval()


def _paired(tiles, **kw):
    from pssr2_amd.data import ArrayDataset
    args = dict(hr_res=64, lr_scale=4, crappifier=None, val_split=0.34, rotation=True)
    args.update(kw)
    return ArrayDataset(tiles, **args)


def _read_png(path):
    from PIL import Image
    with Image.open(path) as im:
        assert im.mode == "L"
        return np.asarray(im, dtype=np.uint8).copy()


def _expected(model, ds, norm, n_images):
    """The reference's composition built from this package's pinned pieces: ``_pred_array`` per item, ``util.normalize_preds`` twice,
    Pillow's nearest resize and paste (pssr/predict.py:117-130, 213-243)."""
    from PIL import Image
    from pssr2_amd.data import _RandomIterIdx
    from pssr2_amd.predict import _pred_array
    from pssr2_amd.util import normalize_preds
    res, scale = ds.crop_res, ds.lr_scale
    collage = Image.new("L", (res * (2 if ds.is_lr else 3), res * n_images))
    order = list(_RandomIterIdx(ds.val_idx, seed=True)) if len(ds.val_idx) < len(ds) else list(ds.val_idx)
    with torch.no_grad():
        for row, idx in enumerate(order[:n_images]):
            if ds.is_lr:
                hr, lr = None, ds[idx].cuda().unsqueeze(0)
            else:
                hr, lr = (t.cuda().unsqueeze(0) for t in ds[idx])
            hr_hat = _pred_array(model(lr))[:, :, :res, :res]
            lr = _pred_array(lr)[:, :, :res // scale, :res // scale]
            hr = None if hr is None else _pred_array(hr)[:, :, :res, :res]
            if norm:
                hr, hr_hat = normalize_preds(hr, hr_hat)
                _, lr = normalize_preds(hr, lr)
            images = [Image.fromarray(lr[0, 0]).resize((hr_hat.shape[-1], hr_hat.shape[-2]), Image.Resampling.NEAREST), Image.fromarray(hr_hat[0, 0])]
            images += [] if hr is None else [Image.fromarray(hr[0, 0])]
            for p, image in enumerate(images):
                collage.paste(image, (p * res, row * res))
    return np.asarray(collage, dtype=np.uint8), order


@pytest.mark.parametrize("norm", [False, True])
def test_predict_collage_equals_the_host_composition(tiles, model, tmp_path, norm):
    from pssr2_amd import predict_collage
    ds = _paired(tiles)
    assert len(ds.val_idx) == 2
    want, order = _expected(model, ds, norm, 2)
    assert sorted(order) == sorted(ds.val_idx)
    assert predict_collage(model, ds, device="cuda", norm=norm, n_images=2, out_dir=str(tmp_path)) is None
    got = _read_png(tmp_path / "collage_2.png")
    assert got.shape == (128, 192)
    assert np.array_equal(got, want)
    assert all(len(np.unique(got[:, p * 64:(p + 1) * 64])) > 20 for p in range(3))
    if not norm:                                              # the HR panel is the validation tile itself, unrotated, in the seeded order
        assert np.array_equal(got[:64, 128:], tiles[order[0], 0]) and np.array_equal(got[64:, 128:], tiles[order[1], 0])


def test_predict_collage_lr_mode_and_errors(tiles, model, tmp_path):
    from pssr2_amd.predict import predict_collage
    ds = _paired(tiles[:, :, :32, :32], hr_res=32, lr_scale=-1)
    assert ds.is_lr and ds.crop_res == 32 and ds.lr_scale == 1
    with pytest.raises(ValueError, match="paired"):
        predict_collage(model, ds, device="cuda", norm=True, out_dir=str(tmp_path))
    predict_collage(model, ds, device="cuda", norm=False, n_images=2, prefix="lr", out_dir=str(tmp_path / "sub"))
    got = _read_png(tmp_path / "sub" / "lr_collage_2.png")
    want, _ = _expected(model, ds, False, 2)
    assert got.shape == (64, 64) and np.array_equal(got, want)          # two panels: LR (identity map) and prediction
    with pytest.raises(RuntimeError, match="no CPU fallback"):
        predict_collage(model, _paired(tiles), device="cpu", norm=False, out_dir=str(tmp_path / "cpu"))
    model.cuda()
    assert not (tmp_path / "cpu").exists()


def test_predict_collage_row_count_and_callbacks(tiles, model, tmp_path):
    from pssr2_amd.predict import predict_collage
    ds = _paired(tiles)
    want, _ = _expected(model, ds, False, 4)
    calls, seen = [], []

    def plain():
        calls.append(len(calls))

    def with_locals(loc):
        seen.append((loc["idx"], loc["data_idx"], loc["collage"].is_cuda, tuple(loc["collage"].shape)))

    predict_collage(model, ds, device="cuda", norm=False, n_images=4, out_dir=str(tmp_path), callbacks=[plain, with_locals])
    got = _read_png(tmp_path / "collage_4.png")
    assert got.shape == (256, 192) and np.array_equal(got, want)
    assert (got[128:] == 0).all() and (got[:128] != 0).any()              # two validation items: rows 2 and 3 stay black
    assert calls == [0, 1] and [s[0] for s in seen] == [0, 1] and all(s[2] and s[3] == (256, 192) for s in seen)
    calls.clear(), seen.clear()
    predict_collage(model, ds, device="cuda", norm=False, n_images=1, out_dir=str(tmp_path), callbacks=[plain, with_locals])
    assert calls == [0] and len(seen) == 1                                # one row, whatever the callbacks
    assert np.array_equal(_read_png(tmp_path / "collage_1.png"), want[:64])
    predict_collage(model, ds, device="cuda", norm=False, out_dir=str(tmp_path))        # default: min(50, len(dataset)) rows
    assert _read_png(tmp_path / "collage_6.png").shape == (384, 192)


def test_predict_collage_rejects_mismatched_scale(tiles, tmp_path):
    from pssr2_amd.models import ResUNet
    from pssr2_amd.predict import predict_collage
    torch.manual_seed(1)
    half = ResUNet(hidden=[16, 32], scale=2, depth=1).cuda()
    with pytest.raises(ValueError, match="differ in size"):
        predict_collage(half, _paired(tiles), device="cuda", norm=False, out_dir=str(tmp_path))


# ------------------------------------------------------------------------------------------------ preprocess_dataset on the device classes
def _read_tif(path):
    from PIL import Image
    with Image.open(path) as im:
        pages = []
        for k in range(getattr(im, "n_frames", 1)):
            im.seek(k)
            pages.append(np.asarray(im, dtype=np.uint8).copy())
    return np.stack(pages)


def _same_files(a, b, n, sides=("lr", "hr")):
    for side in sides:
        names = sorted(p.name for p in (a / side).iterdir())
        assert len(names) == n and names == sorted(p.name for p in (b / side).iterdir())
        for name in names:
            assert (a / side / name).read_bytes() == (b / side / name).read_bytes(), (side, name)
            assert np.array_equal(_read_tif(a / side / name), _read_tif(b / side / name))


def test_preprocess_device_tiles_equal_the_host_files(tmp_path):
    from pssr2_amd import preprocess_dataset
    from pssr2_amd.data import ArrayDataset, DeviceTileDataset
    images = np.random.default_rng(5).integers(0, 256, (5, 1, 40, 40), dtype=np.uint8)
    kw = dict(hr_res=32, lr_scale=4, crappifier=None, val_split=0.2, rotation=True, names=[f"tile{i}" for i in range(5)])
    host, dev = ArrayDataset(images, **kw), DeviceTileDataset(images, **kw)
    preprocess_dataset(host, True, str(tmp_path / "host"))
    random.seed(4)
    state = random.getstate()
    counter = int(dev.tile_counter)
    preprocess_dataset(dev, True, str(tmp_path / "dev"), batch_size=2)          # batches of 2, 2, 1
    assert random.getstate() == state
    assert int(dev.tile_counter) == counter + 5                                # the Philox tile counter advances as for any batch
    _same_files(tmp_path / "host", tmp_path / "dev", 5)
    assert _read_tif(tmp_path / "dev" / "lr" / "tile3.tif").shape == (1, 8, 8)
    # a training index still rotates afterwards: draw_items without pp makes the reference's two draws per index, as before
    train = [i for i in range(5) if i not in dev.val_idx]
    random.seed(9)
    table = dev.draw_items(train + dev.val_idx)
    after = random.getstate()
    random.seed(9)
    drawn = [[bool(random.getrandbits(1)), random.choice((1, 2, (1, 2)))] for _ in train]
    assert random.getstate() == after
    rows = [struct.unpack("<Qiiii", table[k].cpu().numpy().tobytes()) for k in range(5)]
    assert [(r[3], r[4]) for r in rows[:4]] == [(int(d[0]), 3 if d[1] == (1, 2) else d[1]) for d in drawn]
    assert (rows[4][3], rows[4][4]) == (0, -1)
    assert [(r[3], r[4]) for r in [struct.unpack("<Qiiii", t.cpu().numpy().tobytes()) for t in dev.draw_items(train, pp=True)]] == [(0, -1)] * 4
    assert random.getstate() == after


def test_preprocess_device_sheets_equal_the_host_files(tmp_path):
    from pssr2_amd.data import DeviceSlidingDataset, SlidingSheetDataset, preprocess_dataset
    sheet = np.random.default_rng(6).integers(0, 256, (1, 72, 72), dtype=np.uint8)
    kw = dict(hr_res=32, lr_scale=4, crappifier=None, overlap=12, val_split=0.2, rotation=True)
    host, dev = SlidingSheetDataset([sheet], **kw), DeviceSlidingDataset([sheet], **kw)
    assert len(host) == len(dev) == 9
    preprocess_dataset(host, True, str(tmp_path / "host"))
    preprocess_dataset(dev, True, str(tmp_path / "dev"), batch_size=2)
    _same_files(tmp_path / "host", tmp_path / "dev", 9)


def test_preprocess_device_pairs_equal_the_host_files(tmp_path):
    from pssr2_amd.data import DevicePairedTileDataset, PairedArrayDataset, preprocess_dataset
    r = np.random.default_rng(7)
    hr, lr = r.integers(0, 256, (3, 1, 40, 40), dtype=np.uint8), r.integers(0, 256, (3, 1, 10, 10), dtype=np.uint8)
    kw = dict(hr_res=32, lr_scale=4, val_split=0.34, rotation=True)
    host, dev = PairedArrayDataset(hr, lr, **kw), DevicePairedTileDataset(hr, lr, **kw)
    preprocess_dataset(host, False, str(tmp_path / "host"))
    preprocess_dataset(dev, False, str(tmp_path / "dev"), batch_size=2)
    _same_files(tmp_path / "host", tmp_path / "dev", 3, sides=("lr",))
    assert not (tmp_path / "dev" / "hr").exists()
    assert np.array_equal(_read_tif(tmp_path / "dev" / "lr" / "image1.tif"), lr[1][:, 1:9, 1:9])
