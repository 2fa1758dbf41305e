"""Cost of the blur search of estimate_rsf (pssr2_amd/util.py: estimate_rsf -> csrc/rsf.hip: pssr_rsf_moments_u8), one MI355X, two shapes at
scale 4 with the default candidates (0, 0.25, .. 8 HR pixels: K = 33, R = 24):

  batch    [32, 1, 512, 512] sharp items against [32, 1, 128, 128] LR items
  sheet    one 8192 x 8192 sharp plane against its 2048 x 2048 LR plane (``--sheet-lr`` sets the LR side)

and for each of them
  fused          the fused launch (with the upload of its tap table and its fold launch)
  composition    what a user could write from the ops the package had before, which is not this code: for every candidate a float
                 ops.gaussian_blur of the sharp image (none for sigma = 0), ops.clip_u8 to quantise it, ops.reduce_moments_u8 on the result.
                 Its blur replicates the edge, reaches int(4 sigma + .5) pixels and rounds once more, and it sums over the whole plane
  the fused launch's rate over its algorithmic bytes, s^2 n + n per plane (sharp read, lr read), beside the 6.3 TB/s of a streaming copy

Outputs are compared before anything is timed.  The two sides round differently, so bytes are compared only where they must agree: the
fused table's row of sigma = 0 against the composition's unblurred reduction, cropped to the margin, summed in torch int64, bit for bit.
Beyond that the LR side is planted -- every plane's interior is D_k of its own sharp plane for a known k per plane (pssr_rsf_reduce_u8) --
and the candidate each side chooses per plane is reported beside the planted one.  Every shape is warmed up; ``--rounds`` rounds of
``--kernel-reps`` fused launches and ``--reps`` compositions, the two sides alternating within a round, a host clock around work that ends
in a device synchronise; median / minimum / maximum in milliseconds per call.  Prints one JSON line.
    python tools/diag/bench_rsf.py [--rounds 5] [--reps 1] [--kernel-reps 10] [--sheet-lr 2048]"""
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
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--kernel-reps", type=int, default=10)
    ap.add_argument("--sheet-lr", type=int, default=2048)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_rsf needs an MI355X")
    from pssr2_amd import ops
    from pssr2_amd.util import RSF_SIGMAS, _rsf_choose
    scale, sigmas = 4, list(RSF_SIGMAS)
    taps, radius = ops.rsf_taps(scale, sigmas)
    K, m = len(sigmas), ops.register_margin(scale, radius)
    out = {"scale": scale, "candidates": K, "radius": radius, "margin": m, "rounds": args.rounds, "reps": args.reps, "kernel_reps": args.kernel_reps,
           "sheet_lr": args.sheet_lr}
    gen = torch.Generator(device="cuda").manual_seed(7)

    def composition(y, l, keep=False):
        def run():
            x = ops.u8_to_f32(y)
            q = torch.empty_like(y)
            rows, first = [], None
            for sigma in sigmas:
                if sigma > 0:
                    ops.clip_u8(ops.gaussian_blur(x, sigma, 0.0, 0), q)
                d, sums = ops.reduce_moments_u8(q if sigma > 0 else y, l)
                if keep:
                    rows.append(sums)
                    first = d if first is None else first
            return (rows, first) if keep else sums
        return run

    sides = []
    for name, planes, side in (("batch", 32, 128), ("sheet", 1, args.sheet_lr)):
        n_in = side - 2 * m
        y = torch.randint(0, 256, (planes, 1, side * scale, side * scale), dtype=torch.uint8, device="cuda", generator=gen)
        l = torch.randint(0, 256, (planes, 1, side, side), dtype=torch.uint8, device="cuda", generator=gen)
        planted = [(5 + 7 * p) % K for p in range(planes)]
        l[..., m:side - m, m:side - m] = ops.rsf_reduce_u8(y, taps, radius, planted)
        table = ops.rsf_moments_u8(y, l, taps, radius)
        rows, d0 = composition(y, l, keep=True)()
        # the row of sigma = 0 against the composition's unblurred reduction inside the margin, bit for bit
        d0 = d0[..., m:side - m, m:side - m].flatten(-2).to(torch.int64).flatten(0, 1)
        lc = l[..., m:side - m, m:side - m].flatten(-2).to(torch.int64).flatten(0, 1)
        want = torch.stack([d0.sum(-1), (d0 * d0).sum(-1), (d0 * lc).sum(-1), lc.sum(-1), (lc * lc).sum(-1)], dim=-1)
        if not torch.equal(table[:, [0, 1, 2, 3 * K, 3 * K + 1]], want):
            raise SystemExit(f"{name}: pssr_rsf_moments_u8 and the composition disagree on the row of sigma = 0")
        del d0, lc, want
        fused_rows = table.cpu().tolist()
        fused_choice = [_rsf_choose(n_in * n_in, [r], K)[0] for r in fused_rows]
        comp = torch.stack(rows).cpu().tolist()                     # [K][planes][5]: Sd, Sl, Sdd, Sdl, Sll over the whole plane
        comp_choice = []
        for p in range(planes):
            row = [v for k in range(K) for v in (comp[k][p][0], comp[k][p][2], comp[k][p][3])] + [comp[0][p][1], comp[0][p][4]]
            comp_choice.append(_rsf_choose(side * side, [row], K)[0])
        out[f"{name}_planted_sigma"] = [sigmas[k] for k in planted]
        out[f"{name}_fused_agrees"] = sum(a == b for a, b in zip(fused_choice, planted))
        out[f"{name}_composition_sigma"] = [sigmas[k] for k in comp_choice]
        out[f"{name}_composition_agrees"] = sum(a == b for a, b in zip(comp_choice, planted))
        n = side * side
        sides += [(f"{name}_fused", lambda y=y, l=l: ops.rsf_moments_u8(y, l, taps, radius), planes * n * (scale * scale + 1), args.kernel_reps),
                  (f"{name}_composition", composition(y, l), None, args.reps)]

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
