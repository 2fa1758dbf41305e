"""Benchmark of the collage composition of predict_collage (pssr2_amd/predict.py: ``_collage_row`` -> csrc/collage.hip) against the host
composition it replaces, for 50 items of 512^2 (LR 128^2), the forward pass left out of both (the predictions are made once, float32
in HBM, values in [-20, 280]).

  device  50 x ``_collage_row`` into a uint8 canvas in HBM (with ``norm``: clip, two ``normalize_preds`` kernels, one collage launch per
          item; without: one collage launch per item straight from the float tensors), then ONE device-to-host copy of the canvas;
  host    per item three ``_pred_array`` round trips, (``norm``) ``util.normalize_preds`` twice, Pillow NEAREST resize and three pastes.

Neither side writes the PNG.  The two compositions are compared byte for byte first.  ``--rounds`` rounds, the two sides alternating, a
host clock around work that ends in a device synchronise; median / minimum / maximum per side, milliseconds per collage.  Prints one JSON
line.   python tools/diag/bench_collage.py [--rounds 7] [--items 50] [--res 512]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--items", type=int, default=50)
    ap.add_argument("--res", type=int, default=512)
    ap.add_argument("--scale", type=int, default=4)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_collage needs an MI355X")
    from PIL import Image
    from pssr2_amd.predict import _collage_row, _pred_array
    from pssr2_amd.util import normalize_preds
    n, res, scale = args.items, args.res, args.scale
    g = torch.Generator().manual_seed(0)
    items = [(torch.floor(torch.rand(1, 1, res // scale, res // scale, generator=g) * 256).cuda(),
              (torch.rand(1, 1, res, res, generator=g) * 300 - 20).cuda(),
              torch.floor(torch.rand(1, 1, res, res, generator=g) * 256).cuda()) for _ in range(n)]

    def device(norm):
        canvas = torch.zeros(res * n, res * 3, dtype=torch.uint8, device="cuda")
        for row, (lr, hr_hat, hr) in enumerate(items):
            _collage_row(canvas, row, lr, hr_hat, hr, norm, res, scale)
        return canvas.cpu().numpy()                       # synchronises

    def host(norm):
        collage = Image.new("L", (res * 3, res * n))
        for row, (lr, hr_hat, hr) in enumerate(items):
            lr, hr_hat, hr = _pred_array(lr), _pred_array(hr_hat), _pred_array(hr)
            if norm:
                hr, hr_hat = normalize_preds(hr, hr_hat)
                _, lr = normalize_preds(hr, lr)
            panels = [Image.fromarray(lr[0, 0]).resize((res, res), Image.Resampling.NEAREST), Image.fromarray(hr_hat[0, 0]), Image.fromarray(hr[0, 0])]
            for p, image in enumerate(panels):
                collage.paste(image, (p * res, row * res))
        torch.cuda.synchronize()
        return np.asarray(collage, dtype=np.uint8)

    out = {"items": n, "res": res, "lr_scale": scale, "canvas_bytes": n * res * res * 3, "rounds": args.rounds}
    for norm in (False, True):
        if not np.array_equal(device(norm), host(norm)):          # also the warm-up of every shape
            raise SystemExit(f"norm={norm}: device and host compositions disagree")
        times = {"device": [], "host": []}
        for _ in range(args.rounds):
            for name, fn in (("device", device), ("host", host)):
                torch.cuda.synchronize()
                t0 = time.perf_counter()
                fn(norm)
                times[name].append((time.perf_counter() - t0) * 1e3)
        out[f"norm_{norm}"] = {k: {"median_ms": round(statistics.median(v), 2), "min_ms": round(min(v), 2), "max_ms": round(max(v), 2)}
                               for k, v in times.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
