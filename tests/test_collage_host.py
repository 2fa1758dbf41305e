"""Host side of predict_collage / preprocess_dataset (no GPU): Pillow's NEAREST index map, the argument checks of
pssr_collage_rows_u8, preprocess_dataset over host datasets, the ``pp`` argument of ArrayDataset, the lazy exports."""
import ctypes
import random
from pathlib import Path

import numpy as np
import pytest

ROOT = Path(__file__).resolve().parent.parent


@pytest.mark.parametrize("src,dst", [(8, 32), (7, 30), (31, 126), (127, 510), (16, 16), (4, 16), (5, 17)])
def test_nearest_index_is_pillows_map(src, dst):
    """The table equals the index map read out of Image.resize(NEAREST) on an int32 ramp, along both axes."""
    from PIL import Image
    from pssr2_amd.ops import nearest_index
    table = nearest_index(src, dst)
    assert table.dtype == np.int32 and table.shape == (dst,)
    ramp = np.arange(src, dtype=np.int32)
    wide = np.asarray(Image.fromarray(np.broadcast_to(ramp, (3, src)).copy()).resize((dst, 3), Image.Resampling.NEAREST))
    tall = np.asarray(Image.fromarray(np.broadcast_to(ramp[:, None], (src, 3)).copy()).resize((3, dst), Image.Resampling.NEAREST))
    assert np.array_equal(wide[1], table) and np.array_equal(tall[:, 1], table)


def test_nearest_table_is_cached_per_size_and_device():
    import torch
    from pssr2_amd.ops import nearest_index, nearest_table
    a, b = nearest_table(7, 30, "cpu"), nearest_table(7, 30, "cpu")
    assert a is b and a.dtype == torch.int32 and np.array_equal(a.numpy(), nearest_index(7, 30))
    assert nearest_table(7, 31, "cpu") is not a
    with pytest.raises(ValueError):
        nearest_index(0, 4)


def _lib():
    import torch  # noqa: F401  (one HIP runtime per process: torch's)
    path = ROOT / "pssr2_amd" / "libpssr_mi355.so"
    if not path.exists():
        import __graft_entry__ as g
        g.build()
    lib = ctypes.CDLL(str(path))
    lib.pssr_last_error.restype = ctypes.c_char_p
    return lib


def test_collage_argument_validation_without_gpu():
    """Every check happens before the launch: an error code and a message, no crash, no device needed."""
    from pssr2_amd import _lib as L
    lib = _lib()
    assert lib.pssr_abi_version() == 5
    assert ctypes.sizeof(L.CollagePanel) == 48
    fn = lib.pssr_collage_rows_u8
    fn.argtypes = [ctypes.c_void_p, ctypes.c_int, ctypes.c_void_p, ctypes.c_int64, ctypes.c_int, ctypes.c_int, ctypes.c_int, ctypes.c_int,
                   ctypes.c_void_p]
    assert fn(None, 1, None, 64, 0, 1, 16, 16, None) == -1 and b"null" in lib.pssr_last_error()
    fake = 0x1000          # never dereferenced: every call below fails its checks
    panels = (L.CollagePanel * 3)()
    for p in panels:
        p.src, p.image_stride, p.row_pitch, p.src_h, p.src_w = fake, 256, 16, 16, 16
    ptr = ctypes.cast(panels, ctypes.c_void_p)
    assert fn(ptr, 1, None, 64, 0, 1, 16, 16, None) == -1 and b"null" in lib.pssr_last_error()
    for n_panels in (0, 4):
        assert fn(ptr, n_panels, fake, 64, 0, 1, 16, 16, None) == -1 and b"n_panels" in lib.pssr_last_error()
    for n, h, w, row0 in ((0, 16, 16, 0), (1, 0, 16, 0), (1, 16, -1, 0), (1, 16, 16, -1)):
        assert fn(ptr, 1, fake, 64, row0, n, h, w, None) == -1 and b"positive" in lib.pssr_last_error()
    assert fn(ptr, 3, fake, 47, 0, 1, 16, 16, None) == -1 and b"canvas_pitch" in lib.pssr_last_error()
    assert fn(ptr, 1, fake, 64, 0, 65536, 16, 16, None) == -1 and b"grid limit" in lib.pssr_last_error()
    assert fn(ptr, 1, fake, 1 << 20, 0, 1, 1 << 16, 1 << 16, None) == -1 and b"grid limit" in lib.pssr_last_error()
    panels[1].xi = fake                                  # one table without the other
    assert fn(ptr, 2, fake, 64, 0, 1, 16, 16, None) == -1 and b"one index table" in lib.pssr_last_error()
    panels[1].xi, panels[1].src = None, None
    assert fn(ptr, 2, fake, 64, 0, 1, 16, 16, None) == -1 and b"null" in lib.pssr_last_error()
    panels[1].src, panels[1].src_w = fake, 0
    assert fn(ptr, 2, fake, 64, 0, 1, 16, 16, None) == -1 and b"src_w" in lib.pssr_last_error()


def test_lazy_exports_resolve():
    import pssr2_amd
    from pssr2_amd.data import preprocess_dataset
    from pssr2_amd.predict import predict_collage
    assert pssr2_amd.predict_collage is predict_collage and pssr2_amd.preprocess_dataset is preprocess_dataset


# ------------------------------------------------------------------------------------------------ preprocess_dataset (host datasets)
def _images(frames=1):
    return np.random.default_rng(5).integers(0, 256, (5, frames, 40, 40), dtype=np.uint8)


def _read_tif(path):
    from PIL import Image
    with Image.open(path) as im:
        pages = []
        for k in range(getattr(im, "n_frames", 1)):
            im.seek(k)
            pages.append(np.asarray(im, dtype=np.uint8).copy())
    return np.stack(pages)


def _dataset(crappifier, frames=1, **kw):
    from pssr2_amd.data import ArrayDataset
    return ArrayDataset(_images(frames), hr_res=32, lr_scale=4, crappifier=crappifier, val_split=0.2, rotation=True,
                        names=[f"tile{i}" for i in range(5)], **kw)


@pytest.mark.parametrize("noisy", [False, True])
def test_preprocess_dataset_writes_the_unrotated_items(tmp_path, noisy):
    from pssr2_amd.crappifiers import AdditiveGaussian
    from pssr2_amd.data import _resize_bilinear_u8, _square_crop, preprocess_dataset
    ds = _dataset(AdditiveGaussian(5) if noisy else None)
    assert len(ds.val_idx) == 1                              # four training indices: rotated unless pp
    np.random.seed(3)
    random.seed(3)
    state = random.getstate()
    preprocess_dataset(ds, out_dir=str(tmp_path / "out"))
    assert random.getstate() == state                       # no rotation was drawn
    assert sorted(p.name for p in (tmp_path / "out" / "lr").iterdir()) == [f"tile{i}.tif" for i in range(5)]
    assert not (tmp_path / "out" / "hr").exists()
    np.random.seed(3)                                        # an equally seeded second pass over the items themselves
    for idx in range(5):
        hr, lr = ds.__getitem__(idx, pp=True)
        got = _read_tif(tmp_path / "out" / "lr" / f"tile{idx}.tif")
        assert got.shape == (1, 8, 8) and np.array_equal(got, np.asarray(lr, dtype=np.uint8))
        if not noisy:                                        # the Pillow reduction of the unrotated crop, training indices included
            assert np.array_equal(got, _resize_bilinear_u8(_square_crop(ds.images[idx], 32), 8))
            assert np.array_equal(hr.numpy(), _square_crop(ds.images[idx], 32))


def test_preprocess_dataset_hr_folder_and_frames(tmp_path):
    from pssr2_amd.data import _square_crop, preprocess_dataset
    ds = _dataset(None, frames=3)
    preprocess_dataset(ds, preprocess_hr=True, out_dir=str(tmp_path / "out"))
    for idx in range(5):
        hr, lr = _read_tif(tmp_path / "out" / "hr" / f"tile{idx}.tif"), _read_tif(tmp_path / "out" / "lr" / f"tile{idx}.tif")
        assert hr.shape == (3, 32, 32) and lr.shape == (3, 8, 8)            # one page per frame
        assert np.array_equal(hr, _square_crop(ds.images[idx], 32))


def test_preprocess_dataset_rejects_lr_mode(tmp_path):
    from pssr2_amd.data import ArrayDataset, preprocess_dataset
    ds = ArrayDataset(_images(), hr_res=32, lr_scale=-1, crappifier=None)
    assert ds.is_lr
    with pytest.raises(ValueError, match="LR-mode"):
        preprocess_dataset(ds, out_dir=str(tmp_path / "out"))
    assert not (tmp_path / "out").exists()


def test_getitem_draws_as_before_and_pp_draws_nothing():
    """Without ``pp`` a training index consumes the same two ``random`` draws as ever and gives ``_gen_pair``'s pair for them; with
    ``pp`` (or for a validation index) nothing is drawn."""
    from pssr2_amd.data import _gen_pair
    ds = _dataset(None)
    train = [i for i in range(5) if i not in ds.val_idx]
    random.seed(11)
    got = [ds[i] for i in train]
    after = random.getstate()
    random.seed(11)
    for i, (hr, lr) in zip(train, got):
        rot = [bool(random.getrandbits(1)), random.choice((1, 2, (1, 2)))]
        want_hr, want_lr = _gen_pair(ds.images[i], 32, 4, rot, None, None, None)
        assert np.array_equal(hr.numpy(), want_hr.numpy()) and np.array_equal(lr.numpy(), want_lr.numpy())
    assert random.getstate() == after
    assert any(not np.array_equal(hr.numpy(), ds.__getitem__(i, pp=True)[0].numpy()) for i, (hr, _) in zip(train, got))
    random.seed(11)
    state = random.getstate()
    ds.__getitem__(train[0], pp=True), ds[ds.val_idx[0]]
    assert random.getstate() == state
