"""Write tests/golden/stacks.npz from the GENUINE reference (runs only where the reference checkout exists).

TEST INFRASTRUCTURE ONLY, like tools/gen_golden_sliding.py; ``oracle.gen_golden.import_reference`` is used unchanged.  ``tifffile`` is
absent, so after the import this tool gives the stub module that tool's ``imread`` written with Pillow: the reference's own tif branch
(pssr/data.py:566-577) then reads the multi-page tifs that Pillow wrote.  Every dataset is built with ``crappifier=None``: the
reference's crappifiers need the absent scikit-image, and only ``None`` makes LR bit-exact.  Data only:

* ``hr_in/<k>``: the four tile stacks ``im00 ... im03`` of shapes (7, 40, 36), (5, 24, 30), (2, 32, 32), (1, 32, 32) -- a non-square
  centre crop, a reflect pad, and files with too few frames; ``hr_res`` 32, ``lr_scale`` 4 throughout;
* ``cfg/<name>/...`` for the reference's ``ImageDataset`` with ``n_frames=[3, 1]`` (``f31``), ``[1, 3]`` (``f13``), ``2`` (``f2``) and
  ``-1`` (``all``): ``len``, ``slices``, the names, ``repr`` (folder name replaced by ``{HR}``), every item with ``pp=True``
  (``hr/<i>``, ``lr/<i>``: item i; the items of ``all`` differ in depth), and ``split_<split>_<seed>/val_idx`` for the splits
  (0.25, 1), (0.25, 0), (0.75, None), (1, None);
* ``cfg/<name>/rot_idx``, ``rot_hr``, ``rot_lr``: the first training item of the split (0.25, 1) -- file 0, cropped -- under the six
  ``random.seed`` values of ``six_draw_seeds()``, and ``rot_state``: ``random.random()`` drawn right after each item (the state the
  reference's two draws leave); ``cfg/f31/rot0_*``: the same for the first training item of the split (0.25, 0), index 2, the padded file;
* ``lrmode/...``: one LR-mode dataset (``hr_res=8, lr_scale=-1, n_frames=2, val_split=1``): ``len``, ``repr``, every item.

Items are stored as uint8 (asserted to equal the reference's float32 tensors) to keep the file small.

    python tools/gen_golden_stacks.py
"""
from __future__ import annotations

import random
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tools"))
OUT = ROOT / "tests" / "golden" / "stacks.npz"

SHAPES = ((7, 40, 36), (5, 24, 30), (2, 32, 32), (1, 32, 32))
HR_RES, LR_SCALE = 32, 4
CONFIGS = {"f31": [3, 1], "f13": [1, 3], "f2": 2, "all": -1}
SPLITS = ((0.25, 1), (0.25, 0), (0.75, None), (1, None))


def stacks():
    """Noise over four grey levels: as sensitive to a wrong position, orientation or frame as full-range noise (the geometry moves
    pixels, it does not compute with them; the reduction's arithmetic has its own fixture, pairs.npz) at a quarter of the file size."""
    r = np.random.default_rng(71)
    return [np.array([3, 90, 171, 252], dtype=np.uint8)[r.integers(0, 4, s)] for s in SHAPES]


def write_tifs(folder, images):
    from PIL import Image
    folder.mkdir(parents=True)
    for i, st in enumerate(images):
        pages = [Image.fromarray(f) for f in st]
        pages[0].save(folder / f"im{i:02d}.tif", save_all=True, append_images=pages[1:])


def _six_draws(out, key, ds, seeds):
    from gen_golden_sliding import _pairs
    idx = next(i for i in range(len(ds)) if i not in ds.val_idx)
    drawn, state = [], []
    for s in seeds:
        random.seed(s)
        drawn.append(ds[idx])
        state.append(random.random())
    out[f"{key}_idx"], (out[f"{key}_hr"], out[f"{key}_lr"]), out[f"{key}_state"] = np.array(idx), _pairs(drawn), np.array(state)


def gen(out, tmp):
    from gen_golden_paired import six_draw_seeds
    from gen_golden_sliding import _u8
    from pssr.data import ImageDataset
    images = stacks()
    hp = tmp / "hr"
    write_tifs(hp, images)
    for k, a in enumerate(images):
        out[f"hr_in/{k}"] = a
    seeds = six_draw_seeds()
    out["draw_seeds"] = np.array(seeds)
    common = dict(hr_res=HR_RES, lr_scale=LR_SCALE, crappifier=None)

    for name, nf in CONFIGS.items():
        key = f"cfg/{name}"
        ds = ImageDataset(hp, **common, n_frames=nf, val_split=1)
        out[f"{key}/len"], out[f"{key}/slices"] = np.array(len(ds)), np.array(ds.slices)
        out[f"{key}/names"] = np.array([ds._get_name(i) for i in range(len(ds))])
        out[f"{key}/repr"] = np.array(repr(ds).replace(str(hp), "{HR}"))
        for i in range(len(ds)):
            hr, lr = ds.__getitem__(i, pp=True)
            out[f"{key}/hr/{i}"], out[f"{key}/lr/{i}"] = _u8(hr), _u8(lr)
        for split, seed in SPLITS:
            d = ImageDataset(hp, **common, n_frames=nf, val_split=split, split_seed=seed)
            out[f"{key}/split_{split}_{seed}/val_idx"] = np.array(d.val_idx)
        _six_draws(out, f"{key}/rot", ImageDataset(hp, **common, n_frames=nf, val_split=0.25, split_seed=1), seeds)
        print(name, "len", len(ds), "slices", ds.slices, "names", out[f"{key}/names"].tolist())
    _six_draws(out, "cfg/f31/rot0", ImageDataset(hp, **common, n_frames=[3, 1], val_split=0.25, split_seed=0), seeds)

    ds = ImageDataset(hp, hr_res=8, lr_scale=-1, crappifier=None, n_frames=2, val_split=1)
    out["lrmode/len"], out["lrmode/repr"] = np.array(len(ds)), np.array(repr(ds).replace(str(hp), "{HR}"))
    out["lrmode/items"] = np.stack([_u8(ds[i]) for i in range(len(ds))])


def save(path, arrays):
    """``np.savez_compressed`` with a fixed time stamp on every member, so that the file regenerates byte for byte."""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", zipfile.ZIP_DEFLATED) as z:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            info = zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0))
            info.compress_type, info.external_attr = zipfile.ZIP_DEFLATED, 0o644 << 16
            z.writestr(info, buf.getvalue())


if __name__ == "__main__":
    from gen_golden_sliding import pillow_imread
    from oracle.gen_golden import import_reference
    import_reference()
    sys.modules["tifffile"].imread = pillow_imread
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        gen(out, Path(tmp))
    save(OUT, out)
    print("wrote", OUT.name, OUT.stat().st_size // 1024, "KiB")
    assert OUT.stat().st_size < 100 * 1024, OUT
