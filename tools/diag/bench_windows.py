"""Micro-benchmark of pssr_gather_windows_u8 (csrc/windows.hip): a batch of 32 windows of 1 x 512^2 out of one 1 x 4096 x 4096 sheet
(stride 384: origins k * 384, so most rows are misaligned), against pssr_gen_pair_geometry_u8 (csrc/crappify.hip) on the same 32 windows
pre-cut into contiguous 512^2 stacks, with the same orientations.  Three runs: no rotation, every item rotated (flips cycling), and the
six (rot90, flip) draws of the reference mixed.  Both launches must move 16 MB (8 MB read, 8 MB written).

Per run and kernel: ``--windows`` timing windows of ``--iters`` back-to-back launches between two device events, the two kernels
alternating window by window; the median, minimum and maximum of the per-launch times are reported, and the outputs are compared first.
The 16 MB live in the Infinity Cache after the first launch: the figures are the kernels' steady state inside a training loop that
re-reads resident sheets, not HBM-cold reads.  Prints one JSON line.   python tools/diag/bench_windows.py [--iters 500] [--windows 7]"""
import argparse
import json
import os
import random
import statistics
import sys

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

RES, SHEET, STRIDE, BATCH = 512, 4096, 384, 32
DRAWS = [(rot, flip) for rot in (False, True) for flip in (1, 2, (1, 2))]


def orientations(kind):
    if kind == "none":
        return [False] * BATCH
    if kind == "rotated":
        return [[True, (1, 2, (1, 2))[i % 3]] for i in range(BATCH)]
    return [list(DRAWS[i % 6]) for i in random.Random(3).sample(range(BATCH), BATCH)]


def window_time(fn, iters):
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters * 1e3          # microseconds per launch


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=500)
    ap.add_argument("--windows", type=int, default=7)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_windows needs an MI355X")
    from pssr2_amd import _lib as L, data as D

    sheet = torch.from_numpy(np.random.default_rng(0).integers(0, 256, (1, SHEET, SHEET), dtype=np.uint8)).cuda()
    bank = D._SheetBank([sheet], "cuda", "bench_windows")
    per_row = (SHEET - RES) // STRIDE + 1
    tiles = random.Random(1).sample(range(per_row * per_row), BATCH)
    origins = [(t // per_row * STRIDE, t % per_row * STRIDE) for t in tiles]
    cut = torch.stack([sheet[:, y:y + RES, x:x + RES] for y, x in origins]).contiguous()
    moved = 2 * BATCH * RES * RES
    out = {"batch": BATCH, "res": RES, "sheet": [1, SHEET, SHEET], "stride": STRIDE, "bytes_moved": moved, "iters": args.iters, "windows": args.windows}
    lib = L.lib()
    for kind in ("none", "rotated", "mixed"):
        rots = orientations(kind)
        items = D._window_rows([(0, 0, y, x, rot) for (y, x), rot in zip(origins, rots)]).cuda()
        table = D._gather_table(cut, range(BATCH), rots)
        new, old = torch.empty_like(cut), torch.empty_like(cut)

        def run_new():
            L.check(lib.pssr_gather_windows_u8(L.ptr(bank.table), 1, L.ptr(items), BATCH, L.ptr(new), 1, RES, L.stream_ptr()), "pssr_gather_windows_u8")

        def run_old():
            L.check(lib.pssr_gen_pair_geometry_u8(L.ptr(table), BATCH, L.ptr(old), 1, RES, L.stream_ptr()), "pssr_gen_pair_geometry_u8")

        run_new(), run_old()
        torch.cuda.synchronize()
        if not torch.equal(new, old):
            raise SystemExit(f"{kind}: the two kernels disagree")
        for fn in (run_new, run_old):                # warm-up
            window_time(fn, 50)
        times = {"gather_windows": [], "gen_pair_geometry": []}
        for _ in range(args.windows):
            times["gather_windows"].append(window_time(run_new, args.iters))
            times["gen_pair_geometry"].append(window_time(run_old, args.iters))
        out[kind] = {k: {"median_us": round(statistics.median(v), 2), "min_us": round(min(v), 2), "max_us": round(max(v), 2),
                         "gb_per_s_at_median": round(moved / statistics.median(v) / 1e3, 1)} for k, v in times.items()}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
