"""Write tests/golden/paired.npz and tests/golden/paired_poisson.npz from the GENUINE reference (runs only where the reference checkout
exists).  Two files because the recorded float32 noise fields do not compress and no committed file may pass 1 MiB: every
``obj/poisson/...`` entry goes to the second file, everything else to the first.

TEST INFRASTRUCTURE ONLY, like tools/gen_golden_crappifier.py; ``oracle.gen_golden.import_reference`` is used unchanged (it already
stands in for the absent ``skopt`` / ``skopt.space``, which ``pssr.train`` imports and no fixture executes).  Data only:

* ``geo/<case>/...``: the input images (``hr_in``, ``lr_in``) and the items of the reference's ``PairedImageDataset`` over png files written to a temporary folder (``tifffile`` is
  absent) for pairs of equal size, larger than ``hr_res`` (crop), smaller (reflect pad) and non-square; for the ``equal`` and
  ``nonsq`` cases also item 0 under six ``random.seed`` values that make the dataset draw each of the six (rot90, flip) combinations;
  ``val_idx`` / names / ``len`` / ``repr`` (folder names replaced by ``{HR}`` / ``{LR}``) for ``val_split`` 1 / 0.25 with
  ``split_seed`` None / 3;
* ``frames/...``: ``pssr.data._transform_pair`` on 3-frame stacks with ``n_frames=[3, 1]`` (a png holds one frame, so the dataset
  itself cannot reach the centre-frame slicing), without and with a rotation;
* ``obj/...``: 8 pairs, HR 256^2 from an integer formula (``objective_pairs`` below: exact on every platform), ``lr_scale=2``,
  LR = Pillow reduction + N(2, 9), rounded and clipped.  For ``AdditiveGaussian(9, 2)`` and ``Poisson(0.7, 1)``: the value of the
  reference's ``_Crappifier_Objective.sample`` with ``n_samples = 8`` under ``random.seed(11)`` / ``np.random.seed(12)``, the sample
  order, the reduced HR and the ``lr_hat`` arrays it drew in that order (recorded by a factory passed as ``crappifier`` whose
  instances call the reference class and keep the result; stored as float32, the cast the objective applies), and the two terms
  of every image recomputed with the reference's expressions from those arrays.  Plus the reference's curve: 16 repeated values at
  each of intensity {3, 6, 9, 12, 15} x gain {0, 2, 4} (``np.random.seed(100 + point)``, ``random.seed(200 + point)``).

    python tools/gen_golden_paired.py
"""
from __future__ import annotations

import random
import sys
import tempfile
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
OUT = ROOT / "tests" / "golden" / "paired.npz"

GEO_CASES = {        # name: (HR (H, W), LR (h, w), files); hr_res 32, lr_scale 4 throughout
    "equal": ((32, 32), (8, 8), 8),
    "crop": ((48, 48), (12, 12), 3),
    "pad": ((24, 24), (6, 6), 3),
    "nonsq": ((40, 28), (10, 7), 3),
}
GEO_HR_RES, GEO_LR_SCALE = 32, 4
CURVE_INTENSITY, CURVE_GAIN, CURVE_REPEATS = (3, 6, 9, 12, 15), (0, 2, 4), 16


def geo_images(name):
    (H, W), (h, w), n = GEO_CASES[name]
    r = np.random.default_rng(sorted(GEO_CASES).index(name) + 40)
    return r.integers(0, 256, (n, 1, H, W), dtype=np.uint8), r.integers(0, 256, (n, 1, h, w), dtype=np.uint8)


def six_draw_seeds():
    """One ``random.seed`` value per (rot90, flip) combination of the dataset's two draws, in a fixed order."""
    want = [(rot, flip) for rot in (False, True) for flip in (1, 2, (1, 2))]
    seeds = {}
    s = 0
    while len(seeds) < len(want):
        random.seed(s)
        draw = (bool(random.getrandbits(1)), random.choice((1, 2, (1, 2))))
        seeds.setdefault(draw, s)
        s += 1
    return [seeds[d] for d in want]


def objective_pairs():
    """(hr uint8 [8, 1, 256, 256], lr uint8 [8, 1, 128, 128]): an integer pattern of ramps, blocks and dark / bright bands."""
    from PIL import Image
    y, x = np.mgrid[0:256, 0:256]
    hr = []
    for i in range(8):
        v = 30 + (x * 3 + y * 5 + 17 * i) % 97 + ((x // 16 + y // 16 + i) % 5) * 24 + ((x * y + 7 * i) % 13)
        v = np.where(y < 12, (x + i) % 9, v)                      # a dark band: the real LR is clipped at 0 there
        v = np.where(y >= 244, 250 + (x + i) % 6, v)              # a bright band: clipped at 255
        hr.append(np.clip(v, 0, 255).astype(np.uint8)[None])
    hr = np.stack(hr)
    ds = np.stack([[np.asarray(Image.fromarray(ch).resize((128, 128), Image.Resampling.BILINEAR)) for ch in im] for im in hr])
    noise = np.random.RandomState(77).normal(2, 9, ds.shape)
    return hr, np.clip(np.round(ds + noise), 0, 255).astype(np.uint8)


def write_pngs(folder, images):
    from PIL import Image
    folder.mkdir(parents=True)
    for i, im in enumerate(images):
        Image.fromarray(im[0]).save(folder / f"pair{i:02d}.png")


def gen_geometry(out, tmp):
    from pssr.data import PairedImageDataset
    seeds = six_draw_seeds()
    out["geo/draw_seeds"] = np.array(seeds)
    for name in GEO_CASES:
        hr, lr = geo_images(name)
        hp, lp = tmp / name / "hr", tmp / name / "lr"
        write_pngs(hp, hr), write_pngs(lp, lr)
        out[f"geo/{name}/hr_in"], out[f"geo/{name}/lr_in"] = hr, lr
        ds = PairedImageDataset(hp, lp, GEO_HR_RES, GEO_LR_SCALE, extension="png")
        items = [ds[i] for i in range(len(ds))]
        out[f"geo/{name}/hr"] = np.stack([a.numpy() for a, _ in items])
        out[f"geo/{name}/lr"] = np.stack([b.numpy() for _, b in items])
        if name in ("equal", "nonsq"):
            tr = PairedImageDataset(hp, lp, GEO_HR_RES, GEO_LR_SCALE, extension="png", val_split=0.25)
            assert 0 not in tr.val_idx
            drawn = []
            for s in seeds:
                random.seed(s)
                drawn.append(tr[0])
            out[f"geo/{name}/rot_hr"] = np.stack([a.numpy() for a, _ in drawn])
            out[f"geo/{name}/rot_lr"] = np.stack([b.numpy() for _, b in drawn])
        if name == "equal":
            for split in (1, 0.25):
                for seed in (None, 3):
                    d = PairedImageDataset(hp, lp, GEO_HR_RES, GEO_LR_SCALE, extension="png", val_split=split, split_seed=seed)
                    key = f"geo/split_{split}_{seed}"
                    out[f"{key}/val_idx"] = np.array(d.val_idx)
                    out[f"{key}/len"] = np.array(len(d))
                    out[f"{key}/names"] = np.array([d._get_name(i) for i in range(len(d))])
                    out[f"{key}/repr"] = np.array(repr(d).replace(str(hp), "{HR}").replace(str(lp), "{LR}"))


def gen_frames(out):
    from pssr.data import _transform_pair
    r = np.random.default_rng(9)
    hr, lr = r.integers(0, 256, (3, 40, 40), dtype=np.uint8), r.integers(0, 256, (3, 10, 10), dtype=np.uint8)
    out["frames/hr_in"], out["frames/lr_in"] = hr, lr
    seed = six_draw_seeds()[5]                     # (True, (1, 2))
    out["frames/seed"] = np.array(seed)
    for tag, rot in (("plain", False), ("rot", [True, (1, 2)])):
        a, b = _transform_pair(hr, lr, GEO_HR_RES, GEO_HR_RES // GEO_LR_SCALE, rot, None, [3, 1])
        out[f"frames/{tag}_hr"], out[f"frames/{tag}_lr"] = a.numpy(), b.numpy()


def _terms(lr, lr_hat, ds_hr):
    """The two terms of one image with the reference's expressions (pssr/train.py:372-382), from recorded arrays."""
    pred = lr_hat.astype(np.float32) - ds_hr.astype(np.float32)
    target = lr.astype(np.float32) - ds_hr.astype(np.float32)
    bins = np.arange(-256, 256)
    p, _ = np.histogram(pred.flatten(), bins)
    t, _ = np.histogram(target.flatten(), bins)
    return np.mean((t - p) ** 2) / (lr.shape[-1] ** 2), abs(target.mean() - pred.mean())


def gen_objective(out, tmp):
    import pssr.crappifiers as RC
    from pssr.data import PairedImageDataset
    from pssr.train import _Crappifier_Objective
    hr, lr = objective_pairs()
    hp, lp = tmp / "obj" / "hr", tmp / "obj" / "lr"
    write_pngs(hp, hr), write_pngs(lp, lr)
    ds = PairedImageDataset(hp, lp, 256, 2, extension="png")
    out["obj/hr"], out["obj/lr"] = hr, lr

    for tag, cls, params in (("gaussian", RC.AdditiveGaussian, [9, 2]), ("poisson", RC.Poisson, [0.7, 1])):
        drawn, inputs = [], []

        class Recorder:
            def __init__(self, *p):
                self.inner = cls(*p)

            def crappify(self, image):
                inputs.append(np.array(image))
                drawn.append(self.inner.crappify(image))
                return drawn[-1]

        random.seed(11)
        order = list(range(len(ds)))
        random.shuffle(order)
        random.seed(11)
        np.random.seed(12)
        value = _Crappifier_Objective(Recorder, ds, 8).sample(params)
        out[f"obj/{tag}/params"], out[f"obj/{tag}/value"], out[f"obj/{tag}/order"] = np.array(params, dtype=np.float64), np.array(value), np.array(order)
        out[f"obj/{tag}/lr_hat"] = np.stack(drawn).astype(np.float32)
        if tag == "gaussian":
            out["obj/ds_hr"] = np.stack(inputs)[np.argsort(order)]            # in dataset order
        terms = np.array([_terms(lr[i], d, x) for i, d, x in zip(order, drawn, inputs)])
        assert abs(terms.sum(axis=1).mean() - value) < 1e-12, (terms.sum(axis=1).mean(), value)
        out[f"obj/{tag}/terms"] = terms

    curve = np.zeros((len(CURVE_INTENSITY), len(CURVE_GAIN), CURVE_REPEATS))
    obj = _Crappifier_Objective(RC.AdditiveGaussian, ds, 8)
    for a, intensity in enumerate(CURVE_INTENSITY):
        for b, gain in enumerate(CURVE_GAIN):
            point = a * len(CURVE_GAIN) + b
            np.random.seed(100 + point)
            random.seed(200 + point)
            curve[a, b] = [obj.sample([intensity, gain]) for _ in range(CURVE_REPEATS)]
    out["obj/curve"], out["obj/curve_intensity"], out["obj/curve_gain"] = curve, np.array(CURVE_INTENSITY), np.array(CURVE_GAIN)


if __name__ == "__main__":
    from oracle.gen_golden import import_reference
    import_reference()
    out = {}
    with tempfile.TemporaryDirectory() as tmp:
        gen_geometry(out, Path(tmp))
        gen_frames(out)
        gen_objective(out, Path(tmp))
    second = OUT.with_name("paired_poisson.npz")
    np.savez_compressed(OUT, **{k: v for k, v in out.items() if not k.startswith("obj/poisson/")})
    np.savez_compressed(second, **{k: v for k, v in out.items() if k.startswith("obj/poisson/")})
    for f in (OUT, second):
        print("wrote", f.name, f.stat().st_size // 1024, "KiB")
        assert f.stat().st_size < 1 << 20, f
    print("curve mean", out["obj/curve"].mean(axis=2).round(4).tolist(), "std", out["obj/curve"].std(axis=2, ddof=1).round(4).tolist())
