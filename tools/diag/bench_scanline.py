"""Cost of the row sums of estimate_scan_phase (pssr2_amd/util.py: estimate_scan_phase -> csrc/scanline.hip: pssr_line_moments_u8), one
MI355X, radius 8 (17 candidates), two shapes:

  batch    [32, 1, 128, 128]
  sheet    one 4096 x 4096 plane (``--sheet`` sets the side)

and for each of them
  fused          the one launch
  composition    what it replaces, from what the package had before: two strided row copies (the odd rows; the even rows), the rounded
                 mean of every odd row's two neighbours (torch, uint8), and ops.register_shifts_u8 of the odd rows against that mean at
                 scale 1.  It searches (2R+1)^2 shifts where the scan phase needs 2R+1, loses half a grey level in the mean, and gives
                 one set of sums per plane, not per row: the ratio says what the fused kernel saves, not how fast it is.
  the fused launch's rate over its algorithmic bytes (the plane read once, the sums written), beside the 6.3 TB/s of a streaming copy

Outputs are compared before anything is timed.  With m = 1 + R the margin of the registration, the fused sums of the odd rows of
x[2m : 2(n - m) + 1, 1 : W - 1] cover the pixels of the composition's shifts (0, k): sum O_k and sum O_k^2 must be equal, and
0 <= 2 sum D Lc - sum O_k E <= sum O_k (the mean drops the low bit of E).  Every shape is warmed up; ``--rounds`` rounds of
``--kernel-reps`` fused launches and ``--reps`` compositions, the two sides alternating within a round, a host clock around work that ends
in a device synchronise; median / minimum / maximum in milliseconds per call.  Prints one JSON line.
    python tools/diag/bench_scanline.py [--rounds 5] [--reps 5] [--kernel-reps 20] [--sheet 4096] [--radius 8]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

COPY_GBPS = 6300.0      # the streaming-copy figure of DESIGN section 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--sheet", type=int, default=4096)
    ap.add_argument("--radius", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_scanline needs an MI355X")
    from pssr2_amd import ops
    R = args.radius
    T, m = 2 * R + 1, ops.register_margin(1, R)
    out = {"radius": R, "candidates": T, "rounds": args.rounds, "reps": args.reps, "kernel_reps": args.kernel_reps, "sheet": args.sheet}
    gen = torch.Generator(device="cuda").manual_seed(7)

    def composition(x):
        def run():
            odd, even = x[..., 1::2, :].contiguous(), x[..., 0::2, :].contiguous()
            mean = ((even[..., :-1, :].to(torch.int16) + even[..., 1:, :].to(torch.int16) + 1) >> 1).to(torch.uint8)
            return ops.register_shifts_u8(odd[..., :mean.shape[-2], :].contiguous(), mean, R)
        return run

    sides = []
    for name, planes, side in (("batch", 32, 128), ("sheet", 1, args.sheet)):
        x = torch.randint(0, 256, (planes, 1, side, side), dtype=torch.uint8, device="cuda", generator=gen)
        table = composition(x)().reshape(planes, -1)                     # [planes, 3 T^2 + 2], shift (ty, tx) at row (ty + R) T + tx + R
        n = (side - 1) // 2                                              # rows of the mean
        fused = ops.line_moments_u8(x[..., 2 * m:2 * (n - m) + 1, 1:side - 1], R)[:, 0::2].sum(1)      # the odd rows of the window
        for k in range(-R, R + 1):
            t, f = 3 * (R * T + k + R), 3 * (k + R)
            if not (torch.equal(table[:, t], fused[:, f]) and torch.equal(table[:, t + 1], fused[:, f + 1])):
                raise SystemExit(f"{name}: pssr_line_moments_u8 and the composition disagree at k = {k}")
            low = 2 * table[:, t + 2] - fused[:, f + 2]
            if not bool(((low >= 0) & (low <= fused[:, f])).all()):
                raise SystemExit(f"{name}: sum O_k E and the composition's sum D Lc are further apart than the mean's low bit at k = {k}")
        rows = side - 2
        nbytes = planes * (side * side + rows * (3 * T + 2) * 8)
        sides += [(f"{name}_fused", lambda x=x: ops.line_moments_u8(x, R), nbytes, args.kernel_reps), (f"{name}_composition", composition(x), None, args.reps)]

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
    for name in ("batch", "sheet"):
        out[f"{name}_fused_over_composition"] = round(out[f"{name}_fused"]["median_ms"] / out[f"{name}_composition"]["median_ms"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
