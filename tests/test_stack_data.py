"""Tile datasets over multi-frame stacks against the reference's recorded quantities (tests/golden/stacks.npz,
tools/gen_golden_stacks.py): ``ArrayDataset`` from the recorded stacks, ``ImageDataset`` from multi-page tifs written into tmp_path.
Every comparison is bit for bit.  No GPU."""
import random
from pathlib import Path

import numpy as np
import pytest
import torch

GOLD = Path(__file__).resolve().parent / "golden"
HR_RES, LR_SCALE = 32, 4
CONFIGS = {"f31": [3, 1], "f13": [1, 3], "f2": 2, "all": -1}
SLICES = {"f31": [2, 1, 0, 0], "f13": [2, 1, 0, 0], "f2": [3, 2, 1, 0], "all": [1, 1, 1, 1]}
SPLITS = ((0.25, 1), (0.25, 0), (0.75, None), (1, None))
NAMES = ["im00", "im01", "im02", "im03"]


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD / "stacks.npz", allow_pickle=False)


def _stacks(gold):
    return [gold[f"hr_in/{k}"] for k in range(4)]


def _write_tifs(folder, stacks, stem="im"):
    from PIL import Image
    folder.mkdir(parents=True)
    for i, st in enumerate(stacks):
        pages = [Image.fromarray(f) for f in st]
        pages[0].save(folder / f"{stem}{i:02d}.tif", save_all=True, append_images=pages[1:])
    return folder


def _make(kind, gold, tmp_path, **kw):
    from pssr2_amd.data import ArrayDataset, ImageDataset
    kw = dict(dict(hr_res=HR_RES, lr_scale=LR_SCALE, crappifier=None), **kw)
    if kind == "array":
        return ArrayDataset(_stacks(gold), names=NAMES, **kw)
    folder = tmp_path / "hr"
    return ImageDataset(folder if folder.exists() else _write_tifs(folder, _stacks(gold)), **kw)


def _same(item, hr, lr):
    assert item[0].dtype == torch.float32 and item[1].dtype == torch.float32
    assert item[0].shape == hr.shape and item[1].shape == lr.shape
    assert np.array_equal(item[0].numpy(), hr) and np.array_equal(item[1].numpy(), lr)


def test_fixture_is_what_the_reference_was_seen_to_give(gold):
    assert [gold[f"hr_in/{k}"].shape for k in range(4)] == [(7, 40, 36), (5, 24, 30), (2, 32, 32), (1, 32, 32)]
    for name in CONFIGS:
        assert gold[f"cfg/{name}/slices"].tolist() == SLICES[name] and int(gold[f"cfg/{name}/len"]) == sum(SLICES[name])
    val = lambda name: [gold[f"cfg/{name}/split_{s}_{seed}/val_idx"].tolist() for s, seed in SPLITS]
    assert val("f31") == val("f13") == [[2], [0, 1], [2], [0, 1, 2]]
    assert val("f2") == [[3, 4], [0, 1, 2], [3, 4, 5], [0, 1, 2, 3, 4, 5]]
    assert gold["cfg/f31/names"].tolist() == gold["cfg/f13/names"].tolist() == ["im00_0", "im00_1", "im01_0"]
    assert gold["cfg/f2/names"].tolist() == ["im00_0", "im00_1", "im00_2", "im01_0", "im01_1", "im02_0"]
    assert gold["cfg/all/names"].tolist() == NAMES
    assert gold["cfg/f31/hr/0"].shape == (1, 32, 32) and gold["cfg/f31/lr/0"].shape == (3, 8, 8)
    assert gold["cfg/f13/hr/0"].shape == (3, 32, 32) and gold["cfg/f13/lr/0"].shape == (1, 8, 8)
    assert [gold[f"cfg/all/hr/{i}"].shape[0] for i in range(4)] == [7, 5, 2, 1]
    assert int(gold["cfg/f31/rot_idx"]) == 0 and int(gold["cfg/f31/rot0_idx"]) == 2
    assert int(gold["lrmode/len"]) == 6 and gold["lrmode/items"].shape == (6, 2, 8, 8)


@pytest.mark.parametrize("kind", ["array", "files"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_counts_names_and_items_equal_the_reference(gold, tmp_path, kind, name):
    key = f"cfg/{name}"
    ds = _make(kind, gold, tmp_path, val_split=1, n_frames=CONFIGS[name])
    assert len(ds) == int(gold[f"{key}/len"]) and ds.slices == gold[f"{key}/slices"].tolist()
    assert ds.crop_res == HR_RES and ds.is_lr is False and ds.extra_hr_files is None and ds.hr_res == HR_RES and ds.lr_scale == LR_SCALE
    assert ds.n_frames == (None if name == "all" else ([CONFIGS[name]] * 2 if name == "f2" else CONFIGS[name]))
    assert isinstance(ds.images, list) and len(ds.images) == 4                 # shapes differ: the list
    assert [ds._get_name(i) for i in range(len(ds))] == gold[f"{key}/names"].tolist()
    if kind == "files":
        assert repr(ds).replace(str(tmp_path / "hr"), "{HR}") == str(gold[f"{key}/repr"])
        assert ds.hr_files == [f"{n}.tif" for n in NAMES]
    else:
        assert repr(ds).splitlines()[-1] == str(gold[f"{key}/repr"]).splitlines()[-1]
    random.seed(5)
    state = random.getstate()
    for i in range(len(ds)):
        _same(ds.__getitem__(i, pp=True), gold[f"{key}/hr/{i}"], gold[f"{key}/lr/{i}"])
        _same(ds[i], gold[f"{key}/hr/{i}"], gold[f"{key}/lr/{i}"])             # val_split = 1: validation items, not rotated either
    assert random.getstate() == state                                           # no draw for validation items or pp
    with pytest.raises(IndexError, match=f"Tried to retrieve invalid image. Index {len(ds)} is not less than {len(ds)} total image frame slices."):
        ds[len(ds)]


@pytest.mark.parametrize("kind", ["array", "files"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_splits_equal_the_reference(gold, tmp_path, kind, name):
    for split, seed in SPLITS:
        ds = _make(kind, gold, tmp_path, val_split=split, split_seed=seed, n_frames=CONFIGS[name])
        assert ds.val_idx == gold[f"cfg/{name}/split_{split}_{seed}/val_idx"].tolist()
        if split == 0.25:
            assert 0 < len(ds.val_idx) < len(ds)


def _check_draws(ds, gold, key):
    idx = int(gold[f"{key}_idx"])
    assert idx not in ds.val_idx
    seen = set()
    for k, seed in enumerate(gold["draw_seeds"]):
        random.seed(int(seed))
        item = ds[idx]
        after = random.getstate()
        _same(item, gold[f"{key}_hr"][k], gold[f"{key}_lr"][k])
        assert random.random() == float(gold[f"{key}_state"][k])                # the reference's next draw
        random.seed(int(seed))
        random.getrandbits(1), random.choice((1, 2, (1, 2)))
        assert random.getstate() == after                                       # exactly its two draws
        seen.add(item[0].numpy().tobytes())
    assert len(seen) == 6                                                       # six different orientations


@pytest.mark.parametrize("kind", ["array", "files"])
@pytest.mark.parametrize("name", list(CONFIGS))
def test_six_rotation_draws_equal_the_reference(gold, tmp_path, kind, name):
    """The first training item of split (0.25, 1) is slice 0 of file 0 (cropped); that of split (0.25, 0) in f31 is index 2, the only
    slice of file 1 (reflect-padded)."""
    _check_draws(_make(kind, gold, tmp_path, val_split=0.25, split_seed=1, n_frames=CONFIGS[name]), gold, f"cfg/{name}/rot")
    if name == "f31":
        _check_draws(_make(kind, gold, tmp_path, val_split=0.25, split_seed=0, n_frames=[3, 1]), gold, "cfg/f31/rot0")


@pytest.mark.parametrize("kind", ["array", "files"])
def test_lr_mode_equals_the_reference(gold, tmp_path, kind):
    ds = _make(kind, gold, tmp_path, hr_res=8, lr_scale=-1, n_frames=2, val_split=1)
    assert ds.is_lr and len(ds) == int(gold["lrmode/len"]) == 6 and ds.lr_scale == 1 and ds.crop_res == 8
    for i in range(6):
        item = ds[i]
        assert item.dtype == torch.float32 and item.shape == (2, 8, 8) and np.array_equal(item.numpy(), gold["lrmode/items"][i])
    if kind == "files":
        assert repr(ds).replace(str(tmp_path / "hr"), "{HR}") == str(gold["lrmode/repr"])


def test_upstream_smoke_test_at_an_eighth_of_its_resolution(tmp_path):
    """The reference's tests/test_data.py: 5 files of 10 frames, n_frames = 2 -> 5 * (10 // 2) items of 2 frames."""
    from pssr2_amd.data import ImageDataset
    n_images, n_channels, n_frames, res, scale = 5, 10, 2, 512 // 8, 4
    r = np.random.default_rng(0)
    folder = _write_tifs(tmp_path / "smoke", [r.integers(0, 256, (n_channels, res, res), dtype=np.uint8) for _ in range(n_images)])
    ds = ImageDataset(folder, hr_res=res, lr_scale=scale, n_frames=n_frames)
    assert len(ds) == n_images * (n_channels // n_frames) == 25
    hr, lr = ds[0]
    assert hr.shape == (n_frames, res, res) and lr.shape == (n_frames, res // scale, res // scale)
    assert isinstance(ds.images, np.ndarray) and ds.images.shape == (5, 10, res, res)      # one shape: the single array
    assert ds._get_name(0) == "im00_0" and ds._get_name(24) == "im04_4"


def test_compact_items_are_uint8(gold, tmp_path):
    for name in ("f31", "f2"):
        ds = _make("array", gold, tmp_path, val_split=1, n_frames=CONFIGS[name])
        want = [ds[i] for i in range(len(ds))]
        ds.compact = True
        for i, (hr, lr) in enumerate(want):
            got = ds[i]
            assert got[0].dtype == torch.uint8 and got[1].dtype == torch.uint8
            assert torch.equal(got[0].float(), hr) and torch.equal(got[1].float(), lr)


@pytest.mark.parametrize("kind", ["array", "files"])
def test_preprocess_dataset_writes_the_recorded_slices(gold, tmp_path, kind):
    from PIL import Image
    from pssr2_amd.data import preprocess_dataset
    ds = _make(kind, gold, tmp_path, val_split=0.25, split_seed=0, n_frames=2)          # training items too: pp never rotates
    out = tmp_path / "pp"
    preprocess_dataset(ds, preprocess_hr=True, out_dir=str(out))
    names = gold["cfg/f2/names"].tolist()
    assert sorted(p.name for p in (out / "lr").iterdir()) == sorted(p.name for p in (out / "hr").iterdir()) == [f"{n}.tif" for n in names]
    for i, n in enumerate(names):
        for side in ("lr", "hr"):
            with Image.open(out / side / f"{n}.tif") as im:
                pages = []
                for k in range(im.n_frames):
                    im.seek(k)
                    pages.append(np.array(im))
            assert np.array_equal(np.stack(pages), gold[f"cfg/f2/{side}/{i}"])


def test_all_frames_of_equal_stacks_behave_as_before():
    """``n_frames=-1`` with [N, C, H, W] (and [N, H, W]) input: one item per stack, all its frames, the plain names, ``images`` one array."""
    from pssr2_amd.data import ArrayDataset, _gen_pair
    r = np.random.default_rng(2)
    images = r.integers(0, 256, (5, 3, 40, 40), dtype=np.uint8)
    for given in (images, list(images), torch.from_numpy(images)):
        ds = ArrayDataset(given, hr_res=32, lr_scale=4, crappifier=None, val_split=0.4, split_seed=0)
        assert isinstance(ds.images, np.ndarray) and np.array_equal(ds.images, images)
        assert len(ds) == 5 and ds.slices == [1] * 5 and ds.n_frames is None and len(ds.val_idx) == 2
        assert [ds._get_name(i) for i in range(5)] == [f"image{i}" for i in range(5)]
        for i in range(5):
            want = _gen_pair(images[i], 32, 4, False, None, None, None)
            got = ds.__getitem__(i, pp=True)
            assert got[0].shape == (3, 32, 32) and torch.equal(got[0], want[0]) and torch.equal(got[1], want[1])
        assert torch.equal(ds.__getitem__(-1, pp=True)[0], ds.__getitem__(4, pp=True)[0])
    flat = ArrayDataset(images[:, 0], hr_res=32, lr_scale=4, crappifier=None, names=list("abcde"))
    assert flat.images.shape == (5, 1, 40, 40) and flat._get_name(3) == "d" and flat[0][0].shape == (1, 32, 32)
    with pytest.raises(ValueError, match="ArrayDataset expects uint8 images"):
        ArrayDataset(images.astype(np.float32))
    with pytest.raises(ValueError, match="ArrayDataset expects uint8 images"):
        ArrayDataset([images[0], images[1, :2].astype(np.int16)])


def test_slices_of_equal_stacks_and_a_file_of_its_own_size(tmp_path):
    """One shape: ``images`` stays the array and is cut all the same; a 2-D page among stacks is one frame."""
    from pssr2_amd.data import ArrayDataset, ImageDataset
    r = np.random.default_rng(4)
    images = r.integers(0, 256, (3, 5, 32, 32), dtype=np.uint8)
    ds = ArrayDataset(images, hr_res=32, lr_scale=4, crappifier=None, n_frames=[2, 1], val_split=1)
    assert isinstance(ds.images, np.ndarray) and ds.slices == [2, 2, 2] and len(ds) == 6 and ds._get_name(3) == "image1_1"
    hr, lr = ds[3]
    assert np.array_equal(hr.numpy(), images[1, 3:4]) and lr.shape == (2, 8, 8)         # centre of frames 2..3, even count: the upper one
    mixed = ArrayDataset([images[0], images[1, 0, :20, :24]], hr_res=32, lr_scale=4, crappifier=None, val_split=1)
    assert isinstance(mixed.images, list) and mixed.images[1].shape == (1, 20, 24) and len(mixed) == 2 and mixed[1][0].shape == (1, 32, 32)
    folder = _write_tifs(tmp_path / "sizes", [images[0], images[1, :2, :20, :24]])
    files = ImageDataset(folder, hr_res=32, lr_scale=4, crappifier=None, n_frames=2, val_split=1)     # no "equally sized" error
    assert files.slices == [2, 1] and [files._get_name(i) for i in range(3)] == ["im00_0", "im00_1", "im01_0"]
    assert np.array_equal(files[1][0].numpy(), images[0, 2:4])


def test_extra_path_is_not_implemented(gold, tmp_path):
    from pssr2_amd.data import ImageDataset
    folder = _write_tifs(tmp_path / "hr", _stacks(gold))
    with pytest.raises(NotImplementedError, match="extra_path is not supported by pssr2_amd.ImageDataset"):
        ImageDataset(folder, n_frames=[3, 1], extra_path=folder)


def test_exports():
    import pssr2_amd
    for name in ("ArrayDataset", "ImageDataset", "DeviceTileDataset"):
        assert getattr(pssr2_amd, name).__name__ == name and getattr(pssr2_amd, name) is getattr(pssr2_amd.data, name)
