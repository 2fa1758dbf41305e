"""Sheet datasets against the reference's recorded quantities (tests/golden/sliding.npz, tools/gen_golden_sliding.py): the array classes
from the recorded sheets, the file classes from multi-page tifs written into tmp_path.  No GPU."""
import random
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch

GOLD = Path(__file__).resolve().parent / "golden"
HR_RES, OVERLAP, LR_SCALE = 32, 8, 4
CONFIGS = {"slide31": dict(n_frames=[3, 1], slide=True), "pairs2": dict(n_frames=2, slide=False), "all": dict(n_frames=-1, slide=False)}
SPLITS = ((0.25, 0), (0.25, None), (1, 0), (1, None))
NAMES = ["sheet00", "sheet01"]


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD / "sliding.npz", allow_pickle=False)


def _sheets(gold):
    return [gold[f"hr_in/{k}"] for k in range(2)], [gold[f"lr_in/{k}"] for k in range(2)]


def _write_tifs(folder, stacks):
    from PIL import Image
    folder.mkdir(parents=True)
    for i, st in enumerate(stacks):
        pages = [Image.fromarray(f) for f in st]
        pages[0].save(folder / f"sheet{i:02d}.tif", save_all=True, append_images=pages[1:])
    return folder


def _make(kind, gold, tmp_path, **kw):
    from pssr2_amd.data import SlidingDataset, SlidingSheetDataset
    hr, _ = _sheets(gold)
    kw = dict(dict(hr_res=HR_RES, lr_scale=LR_SCALE, crappifier=None, overlap=OVERLAP), **kw)
    if kind == "array":
        return SlidingSheetDataset(hr, names=NAMES, **kw)
    folder = tmp_path / "hr"
    return SlidingDataset(folder if folder.exists() else _write_tifs(folder, hr), **kw)


def _make_paired(kind, gold, tmp_path, **kw):
    from pssr2_amd.data import PairedSlidingArrayDataset, PairedSlidingDataset
    hr, lr = _sheets(gold)
    kw = dict(dict(hr_res=HR_RES, lr_scale=LR_SCALE, overlap=OVERLAP, n_frames=[1, 3], slide=True), **kw)
    if kind == "array":
        return PairedSlidingArrayDataset(hr, lr, names=NAMES, **kw)
    hp, lp = tmp_path / "hr", tmp_path / "lr"
    return PairedSlidingDataset(hp if hp.exists() else _write_tifs(hp, hr), lp if lp.exists() else _write_tifs(lp, lr), **kw)


def _same(item, hr, lr):
    assert item[0].dtype == torch.float32 and item[1].dtype == torch.float32
    assert item[0].shape == hr.shape and item[1].shape == lr.shape
    assert np.array_equal(item[0].numpy(), hr) and np.array_equal(item[1].numpy(), lr)


def _recorded_items(gold, key):
    return [(a, b) for k in range(2) for a, b in zip(gold[f"{key}/hr/{k}"], gold[f"{key}/lr/{k}"])]


@pytest.mark.parametrize("kind", ["array", "files"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_counts_names_and_items_equal_the_reference(gold, tmp_path, kind, name):
    key = f"cfg/{name}"
    ds = _make(kind, gold, tmp_path, val_split=1, **CONFIGS[name])
    assert len(ds) == int(gold[f"{key}/len"]) == {"slide31": 52, "pairs2": 43, "all": 17}[name]
    assert ds.tiles == gold[f"{key}/tiles"].tolist() == [9, 8] and ds.slices == gold[f"{key}/slices"].tolist()
    assert ds.stride == HR_RES - OVERLAP and ds.crop_res == HR_RES and ds.is_lr is False and ds.extra_hr_files is None
    assert [ds._get_name(i) for i in range(len(ds))] == gold[f"{key}/names"].tolist()
    items = _recorded_items(gold, key)
    assert len(items) == len(ds)
    for i, (hr, lr) in enumerate(items):
        _same(ds[i], hr, lr)
    with pytest.raises(IndexError, match=f"Tried to retrieve invalid image. Index {len(ds)} is not less than {len(ds)} total image frame slices."):
        ds[len(ds)]


@pytest.mark.parametrize("kind", ["array", "files"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_splits_and_repr_equal_the_reference(gold, tmp_path, kind, name):
    for split, seed in SPLITS:
        ds = _make(kind, gold, tmp_path, val_split=split, split_seed=seed, **CONFIGS[name])
        key = f"cfg/{name}/split_{split}_{seed}"
        assert ds.val_idx == gold[f"{key}/val_idx"].tolist()
        if kind == "files":
            assert repr(ds).replace(str(tmp_path / "hr"), "{HR}") == str(gold[f"{key}/repr"])
        else:
            assert repr(ds).splitlines()[-1] == str(gold[f"{key}/repr"]).splitlines()[-1]


@pytest.mark.parametrize("kind", ["array", "files"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_six_rotation_draws_equal_the_reference(gold, tmp_path, kind, name):
    key = f"cfg/{name}"
    ds = _make(kind, gold, tmp_path, val_split=0.25, split_seed=0, **CONFIGS[name])
    idx = int(gold[f"{key}/rot_idx"])
    assert idx not in ds.val_idx
    seen = set()
    for k, seed in enumerate(gold["draw_seeds"]):
        random.seed(int(seed))
        item = ds[idx]
        _same(item, gold[f"{key}/rot_hr"][k], gold[f"{key}/rot_lr"][k])
        seen.add(item[0].numpy().tobytes())
    assert len(seen) == 6                                   # six different orientations, none of them skipped
    random.seed(int(gold["draw_seeds"][5]))
    plain = ds.__getitem__(idx, pp=True)                    # pp: no rotation, no draw
    assert np.array_equal(plain[0].numpy(), _make(kind, gold, tmp_path, val_split=1, **CONFIGS[name])[idx][0].numpy())


@pytest.mark.parametrize("kind", ["array", "files"])
def test_lr_mode_equals_the_reference(gold, tmp_path, kind, capsys):
    with warnings.catch_warnings():
        warnings.simplefilter("error")
        ds = _make(kind, gold, tmp_path, lr_scale=-1, n_frames=2, val_split=1)
    assert "LR mode is enabled, dataset will load only unmodified low-resolution images." in capsys.readouterr().out
    assert ds.is_lr and len(ds) == int(gold["lrmode/len"]) == len(gold["lrmode/items"])
    for i in range(len(ds)):
        item = ds[i]
        assert item.dtype == torch.float32 and np.array_equal(item.numpy(), gold["lrmode/items"][i])
    if kind == "files":
        assert repr(ds).replace(str(tmp_path / "hr"), "{HR}") == str(gold["lrmode/repr"])
    with pytest.warns(UserWarning, match="val_split is less than 1, not all low-resolution images will be used in prediciton."):
        _make(kind, gold, tmp_path, lr_scale=-1, n_frames=2, val_split=0.5)


@pytest.mark.parametrize("kind", ["array", "files"])
def test_paired_equals_the_reference(gold, tmp_path, kind):
    ds = _make_paired(kind, gold, tmp_path)
    assert len(ds) == int(gold["paired/len"]) == 52
    assert ds.tiles == gold["paired/tiles"].tolist() and ds.slices == gold["paired/slices"].tolist()
    assert ds.val_idx == gold["paired/val_idx"].tolist() == list(range(52)) and ds.is_lr is False and ds.crop_res == HR_RES
    assert [ds._get_name(i) for i in range(len(ds))] == gold["paired/names"].tolist()
    if kind == "files":
        assert repr(ds).replace(str(tmp_path / "hr"), "{HR}").replace(str(tmp_path / "lr"), "{LR}") == str(gold["paired/repr"])
    for i, (hr, lr) in enumerate(_recorded_items(gold, "paired")):
        _same(ds[i], hr, lr)
    with pytest.raises(IndexError, match="Tried to retrieve invalid image. Index 52 is not less than 52 total image frame slices."):
        ds[52]
    tr = _make_paired(kind, gold, tmp_path, val_split=0.25)
    assert tr.val_idx == gold["paired/split_0.25_None/val_idx"].tolist()
    idx = int(gold["paired/rot_idx"])
    for k, seed in enumerate(gold["draw_seeds"]):
        random.seed(int(seed))
        _same(tr[idx], gold["paired/rot_hr"][k], gold["paired/rot_lr"][k])


def test_paired_lr_side_counts_its_row_on_the_lr_sheet():
    """The reference's quirk: the LR window of tile t starts at (t // tiles_y_lr, t % tiles_y_lr) * (stride // lr_scale) with tiles_y_lr
    counted on the LR sheet.  HR 64 x 64 has 2 windows per row; an LR sheet of 16 x 24 (wider than 64 / 4) has 3."""
    from pssr2_amd.data import PairedSlidingArrayDataset
    r = np.random.default_rng(3)
    hr, lr = r.integers(0, 256, (1, 64, 64), dtype=np.uint8), r.integers(0, 256, (1, 16, 24), dtype=np.uint8)
    ds = PairedSlidingArrayDataset([hr], [lr], hr_res=32, lr_scale=4, overlap=0)
    assert ds.tiles == [4]
    a, b = ds[2]                                            # HR: row 1, column 0; LR with 3 per row: row 0, column 2
    assert np.array_equal(a.numpy(), hr[:, 32:64, 0:32]) and np.array_equal(b.numpy(), lr[:, 0:8, 16:24])


def test_compact_items_are_uint8(gold, tmp_path):
    ds = _make("array", gold, tmp_path, val_split=1, **CONFIGS["slide31"])
    want = ds[5]
    ds.compact = True
    got = ds[5]
    assert got[0].dtype == torch.uint8 and got[1].dtype == torch.uint8
    assert torch.equal(got[0].float(), want[0]) and torch.equal(got[1].float(), want[1])


def test_error_messages(gold, tmp_path):
    from pssr2_amd.data import PairedSlidingArrayDataset, PairedSlidingDataset, SlidingDataset, SlidingSheetDataset
    hr, lr = _sheets(gold)
    missing, empty = tmp_path / "nowhere", tmp_path / "empty"
    empty.mkdir()
    folder = _write_tifs(tmp_path / "hr", hr)
    with pytest.raises(FileNotFoundError, match=f'Path "{missing}" does not exist.'):
        SlidingDataset(missing)
    with pytest.raises(FileNotFoundError, match=f'Path "{missing}" does not exist.'):
        PairedSlidingDataset(folder, str(missing))
    with pytest.raises(FileNotFoundError, match=f'No .tif files exist in path "{empty}".'):
        SlidingDataset(str(empty))
    with pytest.raises(FileNotFoundError, match=f'No .tif files exist in path "{empty}".'):
        PairedSlidingDataset(folder, empty)
    for make in (lambda: SlidingDataset(folder, hr_res=32, overlap=32), lambda: SlidingSheetDataset(hr, hr_res=32, overlap=40),
                 lambda: PairedSlidingDataset(folder, folder, hr_res=32, overlap=32), lambda: PairedSlidingArrayDataset(hr, lr, hr_res=16, overlap=16)):
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            with pytest.raises(ValueError, match="hr_res must be greater than overlap. Given values are .* respectively."):
                make()
    one = _write_tifs(tmp_path / "one", lr[:1])
    with pytest.raises(FileNotFoundError, match="Mismatch between amounts of high-low-resolution images. Found 2 high-resolution and 1 "
                                                "low-resolution images."):
        PairedSlidingDataset(folder, one)
    with pytest.raises(ValueError, match="Mismatch between amounts of high-low-resolution images. Found 2 high-resolution and 1 "
                                         "low-resolution images."):
        PairedSlidingArrayDataset(hr, lr[:1])
    with pytest.warns(UserWarning, match="hr_path is equal to lr_path! Consider using SlidingDataset instead."):
        PairedSlidingDataset(folder, folder, hr_res=HR_RES, overlap=OVERLAP)
    with pytest.raises(ValueError, match="uint8"):
        SlidingSheetDataset([hr[0].astype(np.float32)])


def test_czi_and_extra_path_are_not_implemented(gold, tmp_path):
    from pssr2_amd.data import PairedSlidingDataset, SlidingDataset
    hr, _ = _sheets(gold)
    folder = _write_tifs(tmp_path / "hr", hr)
    with pytest.raises(NotImplementedError, match="czi"):
        SlidingDataset(folder, extension="czi")
    with pytest.raises(NotImplementedError, match="czi"), pytest.warns(UserWarning, match="hr_path is equal to lr_path"):
        PairedSlidingDataset(folder, folder, extension="czi")
    with pytest.raises(NotImplementedError, match="extra_path"):
        SlidingDataset(folder, extra_path=folder)


def test_a_sheet_smaller_than_hr_res_contributes_no_tiles(gold):
    from pssr2_amd.data import SlidingSheetDataset
    hr, _ = _sheets(gold)
    small = np.zeros((6, 31, 200), dtype=np.uint8)
    ds = SlidingSheetDataset([hr[0], small, hr[1][0]], hr_res=HR_RES, lr_scale=LR_SCALE, crappifier=None, overlap=OVERLAP, val_split=1)
    assert ds.tiles == [9, 0, 8] and len(ds) == 17          # (a 2-D sheet is one frame)
    assert ds._get_name(8) == "sheet0_8_0" and ds._get_name(9) == "sheet2_0_0"
    assert np.array_equal(ds[9][0].numpy(), hr[1][:1, :32, :32])


def test_preload_false_and_exports(gold, tmp_path):
    import pssr2_amd
    hr, _ = _sheets(gold)
    folder = _write_tifs(tmp_path / "hr", hr)
    a = pssr2_amd.SlidingDataset(folder, HR_RES, LR_SCALE, None, OVERLAP, preload=False, val_split=1)
    b = pssr2_amd.SlidingDataset(folder, HR_RES, LR_SCALE, None, OVERLAP, val_split=1)
    assert len(a) == len(b) == 17 and torch.equal(a[3][1], b[3][1])
    for name in ("SlidingSheetDataset", "PairedSlidingArrayDataset", "PairedSlidingDataset", "DeviceSlidingDataset", "DevicePairedSlidingDataset"):
        assert getattr(pssr2_amd, name).__name__ == name


def test_gather_windows_validates_before_launching():
    """Null pointers, non-positive c / res and an item count outside the grid limit are PSSR_ERR_ARG; no device is needed to be told so."""
    import ctypes
    import pssr2_amd._lib as L
    if not L._LIB_PATH.exists():
        import __graft_entry__ as g
        g.build()
    lib, p = L.lib(), ctypes.c_void_p(64)                   # never dereferenced: every call below fails its checks
    assert ctypes.sizeof(L.SheetDesc) == 24 and ctypes.sizeof(L.WindowItem) == 24
    for args in ((None, 1, p, 1, p, 1, 32), (p, 1, None, 1, p, 1, 32), (p, 1, p, 1, None, 1, 32), (p, 0, p, 1, p, 1, 32), (p, 1, p, 0, p, 1, 32),
                 (p, 1, p, 65536, p, 1, 32), (p, 1, p, 1, p, 0, 32), (p, 1, p, 1, p, 1, 0), (p, 1, p, 1, p, 1, -16)):
        assert lib.pssr_gather_windows_u8(*args, None) == -1 and b"gather_windows" in lib.pssr_last_error()
