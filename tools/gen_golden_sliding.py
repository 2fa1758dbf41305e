"""Write tests/golden/sliding.npz from the GENUINE reference (runs only where the reference checkout exists).

TEST INFRASTRUCTURE ONLY, like tools/gen_golden_paired.py; ``oracle.gen_golden.import_reference`` is used unchanged.  ``tifffile`` is
absent, so after the import this tool gives the stub module an ``imread`` written with Pillow (frames stacked, 2-D for a single page):
the reference's own tif branch (pssr/data.py:620-624) then reads the multi-page tifs that Pillow wrote.  Every dataset is built with
``crappifier=None``: the reference's crappifiers need the absent scikit-image, and only ``None`` makes LR bit-exact.  Data only:

* ``hr_in/<k>``, ``lr_in/<k>``: the sheets -- HR (6, 100, 90) and (4, 70, 121), LR (6, 25, 22) and (4, 17, 30); ``hr_res`` 32,
  ``overlap`` 8, ``lr_scale`` 4 throughout;
* ``cfg/<name>/...`` for the reference's ``SlidingDataset`` with ``n_frames=[3, 1], slide=True`` (``slide31``), ``n_frames=2,
  slide=False`` (``pairs2``) and ``n_frames=-1`` (``all``): ``len``, ``tiles``, ``slices``, the names, every item (``hr/<k>``,
  ``lr/<k>``: those of sheet k, in order; from a dataset with ``val_split=1``, i.e. without rotation), ``val_idx`` / ``repr`` (folder
  name replaced by ``{HR}``) for ``val_split`` 0.25 / 1 with ``split_seed`` 0 / None, and the first training item of the (0.25, 0)
  split (``rot_idx``) under the six ``random.seed`` values of ``six_draw_seeds()`` (``rot_hr``, ``rot_lr``);
* ``lrmode/...``: one LR-mode dataset (``lr_scale=-1``, ``n_frames=2``) over the HR sheets: ``len``, ``repr``, every item;
* ``paired/...``: the reference's ``PairedSlidingDataset`` with ``n_frames=[1, 3], slide=True``: ``len``, ``tiles``, ``slices``,
  names, ``repr`` (``{HR}`` / ``{LR}``), ``val_idx``, every item, and ``rot_*`` as above from a ``val_split=0.25`` dataset.

Items are stored as uint8 (asserted to equal the reference's float32 tensors) to keep the file small.

    python tools/gen_golden_sliding.py
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
OUT = ROOT / "tests" / "golden" / "sliding.npz"

HR_SHAPES, LR_SHAPES = ((6, 100, 90), (4, 70, 121)), ((6, 25, 22), (4, 17, 30))
HR_RES, OVERLAP, LR_SCALE = 32, 8, 4
CONFIGS = {"slide31": dict(n_frames=[3, 1], slide=True), "pairs2": dict(n_frames=2, slide=False), "all": dict(n_frames=-1, slide=False)}
SPLITS = ((0.25, 0), (0.25, None), (1, 0), (1, None))


def sheets():
    r = np.random.default_rng(62)
    return [r.integers(0, 256, s, dtype=np.uint8) for s in HR_SHAPES], [r.integers(0, 256, s, dtype=np.uint8) for s in LR_SHAPES]


def write_tifs(folder, stacks):
    from PIL import Image
    folder.mkdir(parents=True)
    for i, st in enumerate(stacks):
        pages = [Image.fromarray(f) for f in st]
        pages[0].save(folder / f"sheet{i:02d}.tif", save_all=True, append_images=pages[1:])


def pillow_imread(path):
    from PIL import Image
    im = Image.open(path)
    frames = []
    for k in range(getattr(im, "n_frames", 1)):
        im.seek(k)
        frames.append(np.array(im))
    return frames[0] if len(frames) == 1 else np.stack(frames)


def _u8(t):
    a = t.numpy()
    u = a.astype(np.uint8)
    assert a.dtype == np.float32 and np.array_equal(u, a)
    return u


def _pairs(items):
    return np.stack([_u8(a) for a, _ in items]), np.stack([_u8(b) for _, b in items])


def _by_sheet(out, key, ds, items):
    """``<key>/hr/<k>``, ``<key>/lr/<k>``: the items of sheet k stacked (sheets differ in frames, so their items may differ in depth)."""
    pos = 0
    for k, (t, s) in enumerate(zip(ds.tiles, ds.slices)):
        out[f"{key}/hr/{k}"], out[f"{key}/lr/{k}"] = _pairs(items[pos:pos + t * s])
        pos += t * s


def _six_draws(ds, seeds):
    idx = next(i for i in range(len(ds)) if i not in ds.val_idx)
    drawn = []
    for s in seeds:
        random.seed(s)
        drawn.append(ds[idx])
    return (np.array(idx),) + _pairs(drawn)


def gen(out, tmp):
    from gen_golden_paired import six_draw_seeds
    from pssr.data import PairedSlidingDataset, SlidingDataset
    hr, lr = sheets()
    hp, lp = tmp / "hr", tmp / "lr"
    write_tifs(hp, hr), write_tifs(lp, lr)
    for k, (a, b) in enumerate(zip(hr, lr)):
        out[f"hr_in/{k}"], out[f"lr_in/{k}"] = a, b
    seeds = six_draw_seeds()
    out["draw_seeds"] = np.array(seeds)
    common = dict(hr_res=HR_RES, lr_scale=LR_SCALE, crappifier=None, overlap=OVERLAP)

    for name, cfg in CONFIGS.items():
        key = f"cfg/{name}"
        ds = SlidingDataset(hp, **common, **cfg, val_split=1)
        out[f"{key}/len"], out[f"{key}/tiles"], out[f"{key}/slices"] = np.array(len(ds)), np.array(ds.tiles), np.array(ds.slices)
        out[f"{key}/names"] = np.array([ds._get_name(i) for i in range(len(ds))])
        _by_sheet(out, key, ds, [ds[i] for i in range(len(ds))])
        for split, seed in SPLITS:
            d = SlidingDataset(hp, **common, **cfg, val_split=split, split_seed=seed)
            out[f"{key}/split_{split}_{seed}/val_idx"] = np.array(d.val_idx)
            out[f"{key}/split_{split}_{seed}/repr"] = np.array(repr(d).replace(str(hp), "{HR}"))
        tr = SlidingDataset(hp, **common, **cfg, val_split=0.25, split_seed=0)
        out[f"{key}/rot_idx"], out[f"{key}/rot_hr"], out[f"{key}/rot_lr"] = _six_draws(tr, seeds)
        print(name, "len", len(ds), "tiles", ds.tiles, "slices", ds.slices)

    ds = SlidingDataset(hp, hr_res=HR_RES, lr_scale=-1, crappifier=None, overlap=OVERLAP, n_frames=2, val_split=1)
    out["lrmode/len"], out["lrmode/repr"] = np.array(len(ds)), np.array(repr(ds).replace(str(hp), "{HR}"))
    out["lrmode/items"] = np.stack([_u8(ds[i]) for i in range(len(ds))])

    cfg = dict(hr_res=HR_RES, lr_scale=LR_SCALE, overlap=OVERLAP, n_frames=[1, 3], slide=True)
    ds = PairedSlidingDataset(hp, lp, **cfg)
    out["paired/len"], out["paired/tiles"], out["paired/slices"] = np.array(len(ds)), np.array(ds.tiles), np.array(ds.slices)
    out["paired/names"] = np.array([ds._get_name(i) for i in range(len(ds))])
    out["paired/repr"] = np.array(repr(ds).replace(str(hp), "{HR}").replace(str(lp), "{LR}"))
    out["paired/val_idx"] = np.array(ds.val_idx)
    _by_sheet(out, "paired", ds, [ds[i] for i in range(len(ds))])
    tr = PairedSlidingDataset(hp, lp, **cfg, val_split=0.25)
    out["paired/split_0.25_None/val_idx"] = np.array(tr.val_idx)
    out["paired/rot_idx"], out["paired/rot_hr"], out["paired/rot_lr"] = _six_draws(tr, seeds)
    print("paired len", len(ds), "tiles", ds.tiles, "slices", ds.slices)


if __name__ == "__main__":
    from oracle.gen_golden import import_reference
    import_reference()
    sys.modules["tifffile"].imread = pillow_imread
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        gen(out, Path(tmp))
    np.savez_compressed(OUT, **out)
    print("wrote", OUT.name, OUT.stat().st_size // 1024, "KiB")
    assert OUT.stat().st_size < 1 << 20, OUT
