"""Write tests/golden/swinir.npz from the GENUINE reference (runs only where the reference checkout exists).

TEST INFRASTRUCTURE ONLY, like tools/gen_golden_collage.py; ``oracle.gen_golden.import_reference`` is used unchanged.  It stands
``timm.layers.to_2tuple`` / ``trunc_normal_`` in with placeholders that raise; after it returns, those two names are replaced on the
stub module and on the imported ``pssr.models.swinir`` by a tuple helper and ``torch.nn.init.trunc_normal_`` (initial values are
overwritten by the shared weights anyway).  The reference's SwinIR then builds, runs and back-propagates on the CPU.

Data only.  Weights and inputs are not stored: tests/_swinir_cases.py draws them for this tool and for the tests.  Per case:

  keys / shapes      the reference's ``state_dict`` keys and shapes
  y, g/<parameter>   the float64 model's training-mode output and the gradients of sum(y * cotangent), rounded to float32
  err_out, err_grad  the reference's own float32 run against its float64 run: max |f32 - f64| / max |f64|, for the output and as
                     the maximum over the gradient tensors -- the yardstick of the tests

and once ``sig_names`` / ``sig_defaults``: the reference constructor's parameters and the repr of their defaults.  If the file would
exceed 1 MiB, gradient tensors of 20 k elements and more are left out for the case with the most parameters.

    python tools/gen_golden_swinir.py
"""
from __future__ import annotations

import inspect
import sys
from pathlib import Path

import numpy as np

ROOT = Path(__file__).resolve().parent.parent
sys.path.insert(0, str(ROOT))
sys.path.insert(0, str(ROOT / "tests"))
OUT = ROOT / "tests" / "golden" / "swinir.npz"
LIMIT = 1 << 20


def reference_swinir():
    import torch
    from oracle.gen_golden import import_reference
    import_reference()

    def to_2tuple(v):
        return tuple(v) if isinstance(v, (tuple, list)) else (v, v)

    layers = sys.modules["timm.layers"]
    layers.to_2tuple, layers.trunc_normal_ = to_2tuple, torch.nn.init.trunc_normal_
    import pssr.models.swinir as ref
    ref.to_2tuple, ref.trunc_normal_ = to_2tuple, torch.nn.init.trunc_normal_
    return ref.SwinIR


def generate(ref_cls, skip_large_for=None):
    import torch
    from _swinir_cases import CASES, rel_err, run_case
    out = {"cases": np.array(sorted(CASES))}
    sig = inspect.signature(ref_cls.__init__)
    names = [n for n in sig.parameters if n != "self"]
    out["sig_names"], out["sig_defaults"] = np.array(names), np.array([repr(sig.parameters[n].default) for n in names])
    sizes = {}
    for name in sorted(CASES):
        kwargs = CASES[name][0]
        y64, g64 = run_case(ref_cls(**kwargs), name, torch.float64)
        y32, g32 = run_case(ref_cls(**kwargs), name, torch.float32)
        sd = ref_cls(**kwargs).state_dict()
        out[f"{name}/keys"] = np.array(list(sd))
        out[f"{name}/shapes"] = np.array([",".join(str(s) for s in v.shape) for v in sd.values()])
        out[f"{name}/y"] = y64.numpy().astype(np.float32)
        assert all(float(g.abs().max()) > 0 for g in g64.values()), name
        for k, g in g64.items():
            if name == skip_large_for and g.numel() >= 20000:
                continue
            out[f"{name}/g/{k}"] = g.numpy().astype(np.float32)
        out[f"{name}/err_out"] = np.float64(rel_err(y32.numpy(), y64.numpy()))
        out[f"{name}/err_grad"] = np.float64(max(rel_err(g32[k].numpy(), g64[k].numpy()) for k in g64))
        sizes[name] = sum(g.numel() for g in g64.values())
        print(name, "err_out %.3g" % out[f"{name}/err_out"], "err_grad %.3g" % out[f"{name}/err_grad"], "parameters", sizes[name])
    return out, max(sizes, key=sizes.get)


if __name__ == "__main__":
    cls = reference_swinir()
    out, largest = generate(cls)
    np.savez_compressed(OUT, **out)
    if OUT.stat().st_size >= LIMIT:
        out, _ = generate(cls, skip_large_for=largest)
        np.savez_compressed(OUT, **out)
    print("wrote", OUT.name, OUT.stat().st_size // 1024, "KiB")
    assert OUT.stat().st_size < LIMIT, OUT
