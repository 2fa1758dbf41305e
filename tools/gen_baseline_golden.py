"""Write tests/golden/baseline_pil.npz: real Pillow enlargements (``Image.resize`` with BILINEAR and BICUBIC, mode "L") that pin the
definition B1 of include/pssr_mi355.h and its restatement in tests/_baseline_ref.py.  Data only.  Needs Pillow; the version that wrote
the committed file is stored in it.

  name         input                                     r
  rnd_<h>x<w>  default_rng(h * 1000 + w) integers        as tests/_baseline_ref.PIL_CASES
  bin_<h>x<w>  the same generator's 0 / 255 values       the same
  checker      4 x 4 checkerboard of 0 / 255             8     (overshoot clipped in both passes)
  one          1 x 1, value 200                          8

Per case: ``<name>_in`` uint8 [h, w], ``<name>_r`` int, ``<name>_bilinear`` / ``<name>_bicubic`` uint8 [h r, w r].

    python tools/gen_baseline_golden.py
"""
from __future__ import annotations

import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT / "tests"))
OUT = ROOT / "tests" / "golden" / "baseline_pil.npz"


def cases():
    from _baseline_ref import PIL_CASES, checkerboard
    out = {}
    for h, w, r in PIL_CASES:
        rng = np.random.default_rng(h * 1000 + w)
        out[f"rnd_{h}x{w}"] = (rng.integers(0, 256, (h, w)).astype(np.uint8), r)
        out[f"bin_{h}x{w}"] = ((rng.integers(0, 2, (h, w)) * 255).astype(np.uint8), r)
    out["checker"] = (checkerboard(4, 4), 8)
    out["one"] = (np.full((1, 1), 200, dtype=np.uint8), 8)
    return out


def pil_resize(x, r, filter):
    from PIL import Image
    resample = {"bilinear": Image.BILINEAR, "bicubic": Image.BICUBIC}[filter]
    h, w = x.shape
    return np.asarray(Image.fromarray(x, mode="L").resize((w * r, h * r), resample))


def main():
    import PIL
    data = {"pillow_version": np.array(PIL.__version__)}
    for name, (x, r) in cases().items():
        data[f"{name}_in"], data[f"{name}_r"] = x, np.array(r)
        for filter in ("bilinear", "bicubic"):
            data[f"{name}_{filter}"] = pil_resize(x, r, filter)
    np.savez_compressed(OUT, **data)
    print(f"wrote {OUT} ({OUT.stat().st_size} bytes, Pillow {PIL.__version__})")


if __name__ == "__main__":
    main()
