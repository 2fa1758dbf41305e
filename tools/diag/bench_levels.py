"""Cost of the level table of estimate_noise (pssr2_amd/util.py: estimate_noise -> csrc/levels.hip: pssr_level_moments_u8), one MI355X, two
shapes, each with white-noise and with constant inputs (a constant plane puts every lane of a wave on one LDS word: the kernel's worst case):

  batch    [32, 1, 128, 128] reduced items against their LR items
  plane    one 2048 x 2048 LR plane (``--plane`` sets the side)

and for each of them
  fused          ops.level_moments_u8: the table launch and its fold launch
  composition    what a user could write from torch: the plane and level of every pixel as one int64 index, then five passes into int64
                 [planes * 256] -- torch.bincount for the three counts, index_add_ of int64 values for sum L and sum L^2
  the fused launch's rate over its algorithmic bytes, 2 n per plane, beside the 6.3 TB/s of a streaming copy

Outputs are compared with == before anything is timed.  Every shape is warmed up; ``--rounds`` rounds of ``--kernel-reps`` fused calls
and ``--reps`` compositions, the two sides alternating within a round, a host clock around work that ends in a device synchronise; median /
minimum / maximum in milliseconds per call.  Prints one JSON line.
    python tools/diag/bench_levels.py [--rounds 5] [--reps 3] [--kernel-reps 10] [--plane 2048]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

COPY_GBPS = 6300.0      # the streaming-copy figure of DESIGN section 4


def composition(d, l):
    planes = d.shape[0]

    def run():
        index = (d.reshape(planes, -1).to(torch.int64) + 256 * torch.arange(planes, device=d.device)[:, None]).reshape(-1)
        x = l.reshape(-1).to(torch.int64)
        size = planes * 256
        cols = [torch.bincount(index, minlength=size),
                torch.zeros(size, dtype=torch.int64, device=d.device).index_add_(0, index, x),
                torch.zeros(size, dtype=torch.int64, device=d.device).index_add_(0, index, x * x),
                torch.bincount(index[x == 0], minlength=size),
                torch.bincount(index[x == 255], minlength=size)]
        return torch.stack(cols, dim=-1).view(planes, 256, 5)
    return run


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=10)
    ap.add_argument("--plane", type=int, default=2048)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_levels needs an MI355X")
    from pssr2_amd import ops
    out = {"rounds": args.rounds, "reps": args.reps, "kernel_reps": args.kernel_reps, "plane": args.plane}
    gen = torch.Generator(device="cuda").manual_seed(7)
    sides = []
    for name, planes, side in (("batch", 32, 128), ("plane", 1, args.plane)):
        for kind in ("noise", "constant"):
            if kind == "noise":
                d = torch.randint(0, 256, (planes, side, side), dtype=torch.uint8, device="cuda", generator=gen)
                l = torch.randint(0, 256, (planes, side, side), dtype=torch.uint8, device="cuda", generator=gen)
            else:
                d = torch.full((planes, side, side), 255, dtype=torch.uint8, device="cuda")
                l = torch.full((planes, side, side), 255, dtype=torch.uint8, device="cuda")
            comp = composition(d, l)
            if not torch.equal(ops.level_moments_u8(d, l), comp()):
                raise SystemExit(f"{name}_{kind}: pssr_level_moments_u8 and the composition disagree")
            sides += [(f"{name}_{kind}_fused", lambda d=d, l=l: ops.level_moments_u8(d, l), 2 * planes * side * side, args.kernel_reps),
                      (f"{name}_{kind}_composition", comp, None, args.reps)]

    times = {name: [] for name, _, _, _ in sides}
    for name, fn, _, _ in sides:              # warm-up of every shape
        fn()
    for _ in range(args.rounds):
        for name, fn, _, reps in sides:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / reps)
    for name, _, nbytes, _ in sides:
        v = times[name]
        out[name] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
        if nbytes:
            out[name]["bytes"] = nbytes
            out[name]["GBps_at_median"] = round(nbytes / statistics.median(v) / 1e6, 1)
            out[name]["share_of_streaming_copy"] = round(nbytes / statistics.median(v) / 1e6 / COPY_GBPS, 4)
    for name in ("batch_noise", "batch_constant", "plane_noise", "plane_constant"):
        out[f"{name}_fused_over_composition"] = round(out[f"{name}_fused"]["median_ms"] / out[f"{name}_composition"]["median_ms"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
