"""Paired datasets against the reference's recorded items (tests/golden/paired.npz, tools/gen_golden_paired.py) and the built-in
Bayesian minimiser.  No GPU."""
import random
import warnings
from pathlib import Path

import numpy as np
import pytest
import torch

GOLD = Path(__file__).resolve().parent / "golden"
HR_RES, LR_SCALE = 32, 4
CASES = ("equal", "crop", "pad", "nonsq")


@pytest.fixture(scope="module")
def gold():
    return np.load(GOLD / "paired.npz", allow_pickle=False)


def _images(name):
    d = np.load(GOLD / "paired.npz", allow_pickle=False)
    return d[f"geo/{name}/hr_in"], d[f"geo/{name}/lr_in"]


def _folders(tmp_path, name):
    from PIL import Image
    hr, lr = _images(name)
    for side, images in (("hr", hr), ("lr", lr)):
        (tmp_path / name / side).mkdir(parents=True)
        for i, im in enumerate(images):
            Image.fromarray(im[0]).save(tmp_path / name / side / f"pair{i:02d}.png")
    return tmp_path / name / "hr", tmp_path / name / "lr"


def _make(kind, tmp_path, name, **kw):
    from pssr2_amd.data import PairedArrayDataset, PairedImageDataset
    if kind == "array":
        hr, lr = _images(name)
        return PairedArrayDataset(hr, lr, HR_RES, LR_SCALE, names=[f"pair{i:02d}" for i in range(len(hr))], **kw)
    hp, lp = _folders(tmp_path, name)
    return PairedImageDataset(hp, lp, HR_RES, LR_SCALE, extension="png", **kw)


def _same(item, hr, lr):
    assert item[0].dtype == torch.float32 and item[1].dtype == torch.float32
    assert np.array_equal(item[0].numpy(), hr) and np.array_equal(item[1].numpy(), lr)


@pytest.mark.parametrize("kind", ["array", "files"])
@pytest.mark.parametrize("name", CASES)
def test_items_equal_the_reference(gold, tmp_path, kind, name):
    ds = _make(kind, tmp_path, name)
    assert len(ds) == len(gold[f"geo/{name}/hr"])
    assert ds.val_idx == list(range(len(ds))) and ds.is_lr is False and ds.extra_hr_files is None
    for i in range(len(ds)):
        _same(ds[i], gold[f"geo/{name}/hr"][i], gold[f"geo/{name}/lr"][i])
    with pytest.raises(IndexError):
        ds[len(ds)]


@pytest.mark.parametrize("kind", ["array", "files"])
@pytest.mark.parametrize("name", ["equal", "nonsq"])
def test_six_rotation_draws_equal_the_reference(gold, tmp_path, kind, name):
    ds = _make(kind, tmp_path, name, val_split=0.25)
    assert 0 not in ds.val_idx
    seen = set()
    for k, seed in enumerate(gold["geo/draw_seeds"]):
        random.seed(int(seed))
        item = ds[0]
        _same(item, gold[f"geo/{name}/rot_hr"][k], gold[f"geo/{name}/rot_lr"][k])
        seen.add(item[0].numpy().tobytes())
    assert len(seen) == 6                       # six different geometries
    random.seed(int(gold["geo/draw_seeds"][5]))
    a, b = ds.__getitem__(0, pp=True)           # preprocessing mode: no rotation, no draw
    _same((a, b), gold[f"geo/{name}/hr"][0], gold[f"geo/{name}/lr"][0])


def test_compact_items_are_uint8_with_the_same_values(gold, tmp_path):
    ds = _make("array", tmp_path, "pad")
    ds.compact = True
    hr, lr = ds[1]
    assert hr.dtype == torch.uint8 and lr.dtype == torch.uint8
    assert np.array_equal(hr.numpy(), gold["geo/pad/hr"][1]) and np.array_equal(lr.numpy(), gold["geo/pad/lr"][1])


def test_centre_frame_slicing_equals_the_reference(gold):
    from pssr2_amd.data import PairedArrayDataset
    hr, lr = gold["frames/hr_in"], gold["frames/lr_in"]
    ds = PairedArrayDataset(np.stack([hr, hr]), np.stack([lr, lr]), HR_RES, LR_SCALE, n_frames=[3, 1], val_split=0.5)
    assert ds.n_frames == [3, 1] and ds.val_idx == [1]
    _same(ds[1], gold["frames/plain_hr"], gold["frames/plain_lr"])
    assert tuple(ds[1][0].shape) == (1, 32, 32) and tuple(ds[1][1].shape) == (3, 8, 8)
    random.seed(int(gold["frames/seed"]))
    _same(ds[0], gold["frames/rot_hr"], gold["frames/rot_lr"])
    assert ds._get_name(0) == "image0_0"


@pytest.mark.parametrize("kind", ["array", "files"])
@pytest.mark.parametrize("split", [1, 0.25])
@pytest.mark.parametrize("seed", [None, 3])
def test_split_names_len_repr(gold, tmp_path, kind, split, seed):
    ds = _make(kind, tmp_path, "equal", val_split=split, split_seed=seed)
    key = f"geo/split_{split}_{seed}"
    assert ds.val_idx == gold[f"{key}/val_idx"].tolist()
    assert len(ds) == int(gold[f"{key}/len"])
    assert [ds._get_name(i) for i in range(len(ds))] == gold[f"{key}/names"].tolist()
    assert ds.crop_res == 32 and ds.hr_res == 32 and ds.lr_scale == 4 and ds.n_frames is None
    if kind == "files":
        want = str(gold[f"{key}/repr"]).replace("{HR}", str(ds.hr_path)).replace("{LR}", str(ds.lr_path))
        assert repr(ds) == want
    else:
        assert repr(ds).splitlines()[-1] == str(gold[f"{key}/repr"]).splitlines()[-1]
        assert "8 paired images with 8 total frame slices" in repr(ds)


def test_reference_defaults():
    import inspect
    from pssr2_amd.data import PairedArrayDataset, PairedImageDataset
    for cls in (PairedArrayDataset, PairedImageDataset):
        p = inspect.signature(cls.__init__).parameters
        assert p["val_split"].default == 1 and p["split_seed"].default is None and p["rotation"].default is True
        assert p["hr_res"].default == 512 and p["lr_scale"].default == 4 and p["n_frames"].default == -1
    assert inspect.signature(PairedImageDataset.__init__).parameters["extension"].default == "tif"


def test_reference_errors_and_warning(tmp_path):
    from pssr2_amd.data import PairedArrayDataset, PairedImageDataset
    hp, lp = _folders(tmp_path, "pad")
    with pytest.raises(FileNotFoundError, match="does not exist"):
        PairedImageDataset(tmp_path / "nowhere", lp, extension="png")
    with pytest.raises(FileNotFoundError, match="does not exist"):
        PairedImageDataset(hp, str(tmp_path / "nowhere"), extension="png")
    with pytest.raises(FileNotFoundError, match="No .tif files"):
        PairedImageDataset(hp, lp)
    (lp / "pair02.png").unlink()
    with pytest.raises(FileNotFoundError, match="Mismatch between amounts"):
        PairedImageDataset(hp, lp, extension="png")
    with pytest.warns(UserWarning, match="hr_path is equal to lr_path"):
        PairedImageDataset(str(hp), str(hp), HR_RES, 1, extension="png")
    (lp / "pair02.png").write_bytes((lp / "pair01.png").read_bytes())
    with warnings.catch_warnings():
        warnings.simplefilter("error")              # different folders: no warning
        PairedImageDataset(hp, lp, HR_RES, LR_SCALE, extension="png")
    with pytest.raises(ValueError, match="uint8"):
        PairedArrayDataset(np.zeros((2, 1, 8, 8), np.float32), np.zeros((2, 1, 2, 2), np.uint8))
    with pytest.raises(ValueError, match="Mismatch"):
        PairedArrayDataset(np.zeros((2, 1, 8, 8), np.uint8), np.zeros((3, 1, 2, 2), np.uint8))


def test_exports():
    import pssr2_amd
    from pssr2_amd import data, train
    assert pssr2_amd.PairedArrayDataset is data.PairedArrayDataset and pssr2_amd.PairedImageDataset is data.PairedImageDataset
    assert pssr2_amd.DevicePairedTileDataset is data.DevicePairedTileDataset
    assert pssr2_amd.approximate_crappifier is train.approximate_crappifier
    # the replay path of train_paired is detected by these two names (pssr2_amd/fastpath.py): the paired device dataset has neither
    assert not hasattr(data.DevicePairedTileDataset, "draw_items") and not hasattr(data.DevicePairedTileDataset, "device_batch")


# ------------------------------------------------------------------------------------------ bayes.gp_minimize
def _bowl(p):
    return (p[0] - 3) ** 2 + (p[1] + 1) ** 2


def test_gp_minimize_is_deterministic_and_consistent():
    from pssr2_amd.bayes import gp_minimize
    a = gp_minimize(_bowl, [(0.0, 10.0), (-5.0, 5.0)], n_calls=20, random_state=7)
    b = gp_minimize(_bowl, [(0.0, 10.0), (-5.0, 5.0)], n_calls=20, random_state=7)
    c = gp_minimize(_bowl, [(0.0, 10.0), (-5.0, 5.0)], n_calls=20, random_state=8)
    assert a.x_iters == b.x_iters and np.array_equal(a.func_vals, b.func_vals)
    assert a.x_iters != c.x_iters
    assert len(a.func_vals) == 20 and len(a.x_iters) == 20
    assert a.fun == min(a.func_vals) and _bowl(a.x) == a.fun
    assert all(0 <= p[0] <= 10 and -5 <= p[1] <= 5 for p in a.x_iters)


@pytest.mark.parametrize("seed", range(5))
def test_gp_minimize_finds_the_bowl(seed):
    from pssr2_amd.bayes import gp_minimize
    r = gp_minimize(_bowl, [(0, 10), (-5, 5)], n_calls=40, random_state=seed)
    dist = float(np.hypot(r.x[0] - 3, r.x[1] + 1))
    print(f"seed {seed}: x = {r.x}, distance {dist:.3f}")
    assert dist <= 0.5


def test_gp_minimize_dimensions():
    from pssr2_amd.bayes import gp_minimize

    class Real:
        def __init__(self, low, high):
            self.low, self.high = low, high

    class Integer(Real):
        pass

    r = gp_minimize(_bowl, [(0, 10), (-5, 5)], n_calls=12, random_state=0)
    assert all(type(v) is int for p in r.x_iters for v in p)
    r = gp_minimize(_bowl, [(0, 10), (-5.0, 5.0)], n_calls=12, random_state=0)
    assert all(type(p[0]) is int and type(p[1]) is float for p in r.x_iters)
    r = gp_minimize(_bowl, [Integer(0, 10), Real(-5, 5)], n_calls=12, random_state=0)
    assert all(type(p[0]) is int and type(p[1]) is float for p in r.x_iters)
    r = gp_minimize(_bowl, [(0.0, 10.0), (-5.0, 5.0)], n_calls=12, random_state=0, x0=[3.5, -1.5])
    assert r.x_iters[0] == [3.5, -1.5] and len(r.func_vals) == 12
    r = gp_minimize(_bowl, [(0.0, 10.0), (-5.0, 5.0)], n_calls=12, random_state=0, x0=[[3.5, -1.5]], y0=[0.5])
    assert len(r.func_vals) == 13 and r.func_vals[0] == 0.5
    for bad in ([("a", "b", "c")], [("low", "high")], [(0.0, 10.0), ("x", "y")]):
        with pytest.raises(ValueError, match="categorical"):
            gp_minimize(_bowl, bad, n_calls=5)
    with pytest.raises(TypeError, match="acq_func"):
        gp_minimize(_bowl, [(0.0, 1.0), (0.0, 1.0)], n_calls=5, acq_func="EI")


def test_gp_minimize_needs_neither_scipy_nor_sklearn():
    src = (Path(__file__).resolve().parent.parent / "pssr2_amd" / "bayes.py").read_text()
    assert "import scipy" not in src and "from scipy" not in src and "sklearn" not in src
