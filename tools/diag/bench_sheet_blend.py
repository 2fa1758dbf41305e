"""Cost of predict_sheet's ``blend`` / ``ensemble`` path (pssr2_amd/predict.py -> csrc/tiles.hip: pssr_dihedral_tiles_u8,
pssr_clip_u8_dihedral, pssr_blend_stack_u8) on one ``--size``² uint8 sheet, default ResUNet in bf16, tiles of 128 with overlap 32,
batch 128:

  calls    predict_sheet(to_numpy=False) with (blend, ensemble) = (average, 1) -- the path and kernels of a call without the keywords, the
           reference point -- (linear, 1), (average, 8), (linear, 8)
  kernels  each new kernel alone over every batch of an ensemble-8 call (the cut and the quantisation once per batch of 128 items, the
           stitch once), against the bytes it must move: cut 1 B read + 4 B written per LR pixel of every item, quantise 4 B + 1 B per
           output pixel of every item, stitch 1 B read per output pixel of every item + 1 B written per pixel of the sheet

``--rounds`` rounds of ``--reps`` calls, the configurations alternating, a host clock around work that ends in a device synchronise;
median / minimum / maximum in milliseconds per call.  Prints one JSON line.
    python tools/diag/bench_sheet_blend.py [--rounds 5] [--reps 3] [--size 2048]"""
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
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--size", type=int, default=2048)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_sheet_blend needs an MI355X")
    from pssr2_amd import ops
    from pssr2_amd.models import ResUNet
    from pssr2_amd.predict import predict_sheet
    tile, overlap, batch, scale, ens = 128, 32, 128, 4, 8
    stride = tile - overlap
    torch.manual_seed(0)
    model = ResUNet(channels=1).cuda().eval()
    model.compute_dtype = torch.bfloat16
    sheet = torch.from_numpy(np.random.default_rng(7).integers(0, 256, size=(1, args.size, args.size), dtype=np.uint8)).cuda()
    n_rows = n_cols = (args.size - tile) // stride + 1
    n_tiles, n_items, S = n_rows * n_cols, n_rows * n_cols * ens, tile * scale
    out_hw = (n_rows * stride + overlap) * scale
    out = {"size": args.size, "tiles": n_tiles, "tile_res": tile, "overlap": overlap, "batch": batch, "rounds": args.rounds, "reps": args.reps}

    def call(blend, ensemble):
        return lambda: predict_sheet(model, sheet, tile_res=tile, overlap=overlap, batch_size=batch, to_numpy=False, blend=blend, ensemble=ensemble)

    y = torch.rand(batch, 1, S, S, device="cuda") * 300 - 20
    preds = torch.randint(0, 256, (n_items, 1, S, S), dtype=torch.uint8, device="cuda")
    batches = [(g0, min(batch, n_items - g0)) for g0 in range(0, n_items, batch)]

    def cut():
        for g0, n in batches:
            ops.dihedral_tiles_u8(sheet, 1, 1, tile, stride, n_rows, n_cols, ens, g0, n)

    def quantise():
        for g0, n in batches:
            ops.clip_u8_dihedral(y[:n], preds[g0:g0 + n], ens, g0)

    def stitch(blend):
        return lambda: ops.blend_stack_u8(preds, 1, n_rows, n_cols, overlap * scale, 0, out_hw, out_hw, blend, ens)

    sides = [("call_average_1", call("average", 1), None), ("call_linear_1", call("linear", 1), None),
             ("call_average_8", call("average", 8), None), ("call_linear_8", call("linear", 8), None),
             ("kernel_cut_8", cut, n_items * tile * tile * 5), ("kernel_quantise_8", quantise, n_items * S * S * 5),
             ("kernel_stitch_average_8", stitch("average"), n_items * S * S + out_hw * out_hw),
             ("kernel_stitch_linear_8", stitch("linear"), n_items * S * S + out_hw * out_hw)]
    if not torch.equal(call("average", 1)(), predict_sheet(model, sheet, tile_res=tile, overlap=overlap, batch_size=batch, to_numpy=False)):
        raise SystemExit("blend='average', ensemble=1 and the call without the keywords disagree")
    times = {name: [] for name, _, _ in sides}
    for name, fn, _ in sides:              # warm-up
        fn()
    for _ in range(args.rounds):
        for name, fn, _ in sides:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(args.reps):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / args.reps)
    for name, _, nbytes in sides:
        v = times[name]
        out[name] = {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
        if nbytes:
            out[name]["bytes"] = nbytes
            out[name]["GBps_at_median"] = round(nbytes / statistics.median(v) / 1e6, 1)
    med = {k: v["median_ms"] for k, v in out.items() if isinstance(v, dict)}
    out["linear_over_average_at_1"] = round(med["call_linear_1"] / med["call_average_1"], 4)
    out["not_network_share_of_linear_8"] = round((med["kernel_cut_8"] + med["kernel_quantise_8"] + med["kernel_stitch_linear_8"]) / med["call_linear_8"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
