"""Write tests/golden/collage.npz from the GENUINE reference (runs only where the reference checkout exists).

TEST INFRASTRUCTURE ONLY, like tools/gen_golden_paired.py; ``oracle.gen_golden.import_reference`` is used unchanged.  Data only: for
every case the float32 inputs and the bytes of the image the reference's own
``pssr.predict._collage_preds(lr, hr_hat, hr, norm=False, max_images=1, crop_res, lr_scale)`` returns (``norm=True`` needs
scikit-image's ``resize``, which is absent: that path is tested against ``util.normalize_preds`` instead).

Inputs are drawn from ``default_rng`` over [-20, 280], so clipping to [0, 255] and the truncation of the uint8 cast both matter; the
high-resolution image holds integers, as a dataset's does.

  case  LR          prediction / HR      crop_res  lr_scale
  a     1x1x8^2     32^2                 32        4          integer ratio, 16-byte stores
  b     as a        as a                 30        4          LR 7 -> 30: non-integer ratio, byte stores
  c     1x3x8^2     32^2                 32        4          centre frame 1 of the LR stack
  d     1x1x16^2    64^2, no HR          16        1          LR mode: identity map, two panels
  e     1x1x16^2    64^2, no HR          16        4          LR mode: LR 4 -> 16

    python tools/gen_golden_collage.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
OUT = ROOT / "tests" / "golden" / "collage.npz"

CASES = {        # name: (LR frames, LR size, HR size, has HR, crop_res, lr_scale)
    "a": (1, 8, 32, True, 32, 4),
    "b": (1, 8, 32, True, 30, 4),
    "c": (3, 8, 32, True, 32, 4),
    "d": (1, 16, 64, False, 16, 1),
    "e": (1, 16, 64, False, 16, 4),
}


def case_inputs(name):
    frames, lr_size, hr_size, has_hr, _, _ = CASES[name]
    r = np.random.default_rng(sorted(CASES).index(name) + 70)
    lr = r.uniform(-20, 280, (1, frames, lr_size, lr_size)).astype(np.float32)
    hr_hat = r.uniform(-20, 280, (1, 1, hr_size, hr_size)).astype(np.float32)
    hr = np.floor(r.uniform(-20, 280, (1, 1, hr_size, hr_size))).astype(np.float32) if has_hr else None
    return lr, hr_hat, hr


if __name__ == "__main__":
    import torch
    from oracle.gen_golden import import_reference
    import_reference()
    from pssr.predict import _collage_preds
    out = {"cases": np.array(sorted(CASES))}
    for name in sorted(CASES):
        lr, hr_hat, hr = case_inputs(name)
        crop_res, lr_scale = CASES[name][4:]
        image = _collage_preds(torch.from_numpy(lr), torch.from_numpy(hr_hat), None if hr is None else torch.from_numpy(hr), False, 1,
                               crop_res, lr_scale)
        assert image.mode == "L" and image.size == (crop_res * (3 if hr is not None else 2), crop_res), (name, image.mode, image.size)
        out[f"{name}/lr"], out[f"{name}/hr_hat"] = lr, hr_hat
        if hr is not None:
            out[f"{name}/hr"] = hr
        out[f"{name}/meta"] = np.array([crop_res, lr_scale])
        out[f"{name}/collage"] = np.asarray(image, dtype=np.uint8)
    np.savez_compressed(OUT, **out)
    print("wrote", OUT.name, OUT.stat().st_size // 1024, "KiB")
    assert OUT.stat().st_size < 1 << 20, OUT
