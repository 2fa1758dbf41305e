"""Cost of the shift search of register_pairs (pssr2_amd/util.py: register_pairs -> csrc/register.hip: pssr_register_shifts_u8), one MI355X,
two shapes at scale 4 and radius 8 (289 shifts):

  batch    [32, 1, 512, 512] HR items against [32, 1, 128, 128] LR items
  sheet    one 8192 x 8192 HR plane against its 2048 x 2048 LR plane (``--sheet-lr`` sets the LR side)

and for each of them
  fused          the fused launch (with its tap and fold launches)
  composition    what it replaces, from the ops the package had before: for every shift t a crop of ``hr`` -- the window of D_t and a ring of
                 one LR pixel, so that no output inside the ring uses a border tap -- made contiguous, and ops.reduce_moments_u8 on it
  the fused launch's rate over its algorithmic bytes, s^2 n + n per plane (hr read, lr read), beside the 6.3 TB/s of a streaming copy

Outputs are compared before anything is timed: the table of the fused launch against the sums of every shift taken in torch int64 from the
composition's reduced image without its ring, bit for bit.  Every shape is warmed up; ``--rounds`` rounds of ``--kernel-reps`` fused
launches and ``--reps`` compositions, the two sides alternating within a round, a host clock around work that ends in a device
synchronise; median / minimum / maximum in milliseconds per call.  Prints one JSON line.
    python tools/diag/bench_register.py [--rounds 5] [--reps 2] [--kernel-reps 20] [--sheet-lr 2048] [--radius 8]"""
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
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--kernel-reps", type=int, default=20)
    ap.add_argument("--sheet-lr", type=int, default=2048)
    ap.add_argument("--radius", type=int, default=8)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_register needs an MI355X")
    from pssr2_amd import ops
    scale, radius = 4, args.radius
    m = ops.register_margin(scale, radius)
    shifts = [(ty, tx) for ty in range(-radius, radius + 1) for tx in range(-radius, radius + 1)]
    out = {"scale": scale, "radius": radius, "shifts": len(shifts), "rounds": args.rounds, "reps": args.reps, "kernel_reps": args.kernel_reps,
           "sheet_lr": args.sheet_lr}
    gen = torch.Generator(device="cuda").manual_seed(7)

    def composition(hr, lr, keep=False):
        h, w = lr.shape[-2:]
        ring = lr[..., m - 1:h - m + 1, m - 1:w - m + 1].contiguous()

        def run():
            kept = []
            for ty, tx in shifts:
                cut = hr[..., scale * (m - 1) + ty:scale * (h - m + 1) + ty, scale * (m - 1) + tx:scale * (w - m + 1) + tx].contiguous()
                d, sums = ops.reduce_moments_u8(cut, ring)
                if keep:
                    d = d[..., 1:-1, 1:-1].flatten(-2).to(torch.int64)
                    kept.append((d.sum(-1), (d * d).sum(-1)))
            return kept if keep else sums
        return run

    sides = []
    for name, planes, side in (("batch", 32, 128), ("sheet", 1, args.sheet_lr)):
        lr = torch.randint(0, 256, (planes, 1, side, side), dtype=torch.uint8, device="cuda", generator=gen)
        hr = torch.randint(0, 256, (planes, 1, side * scale, side * scale), dtype=torch.uint8, device="cuda", generator=gen)
        table = ops.register_shifts_u8(hr, lr, radius)
        # the composition's reduced images without their ring, against the table: sum D and sum D^2 here, sum D Lc in a second pass
        lc = lr[..., m:side - m, m:side - m].flatten(-2).to(torch.int64).flatten(0, 1)
        for t, (sd, sdd) in enumerate(composition(hr, lr, keep=True)()):
            if not (torch.equal(table[:, 3 * t], sd.flatten()) and torch.equal(table[:, 3 * t + 1], sdd.flatten())):
                raise SystemExit(f"{name}: pssr_register_shifts_u8 and the composition disagree at shift {shifts[t]}")
        for t, (ty, tx) in enumerate(shifts):
            cut = hr[..., scale * (m - 1) + ty:scale * (side - m + 1) + ty, scale * (m - 1) + tx:scale * (side - m + 1) + tx].contiguous()
            d = ops.reduce_moments_u8(cut, lr[..., m - 1:side - m + 1, m - 1:side - m + 1].contiguous())[0]
            d = d[..., 1:-1, 1:-1].flatten(-2).to(torch.int64).flatten(0, 1)
            if not torch.equal(table[:, 3 * t + 2], (d * lc).sum(-1)):
                raise SystemExit(f"{name}: pssr_register_shifts_u8 and the composition disagree on sum D Lc at shift {(ty, tx)}")
        if not (torch.equal(table[:, -2], lc.sum(-1)) and torch.equal(table[:, -1], (lc * lc).sum(-1))):
            raise SystemExit(f"{name}: the LR sums disagree")
        del lc, d, cut
        n = side * side
        sides += [(f"{name}_fused", lambda hr=hr, lr=lr: ops.register_shifts_u8(hr, lr, radius), planes * n * (scale * scale + 1), args.kernel_reps),
                  (f"{name}_composition", composition(hr, lr), None, args.reps)]

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
