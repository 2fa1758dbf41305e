"""Cost of the classical baselines (pssr2_amd/util.py: nlm_denoise / upsample -> csrc/baseline.hip: pssr_nlm_u8 / pssr_upsample_u8), one
MI355X, two shapes:

  batch    [32, 1, 128, 128]
  sheet    one 4096 x 4096 plane (``--sheet`` sets the side)

nlm_u8 at (p, s) = (2, 7) and (3, 10), h = 12, sigma = 10, beside
  composition    torch on the same device computing the same integers: the plane padded by edge replication, per offset one shifted
                 copy, the squared difference in int32, a separable box sum (P + P shifted adds), q, a gather from the table, the two
                 int64 accumulators; one division at the end.  Outputs are compared with == before anything is timed.
  the rate in patch multiply-adds per second: planes H W (2s + 1)^2 P^2 over the time (what the brute-force form would execute; the
  kernel issues 2 P packed dot products per candidate instead).
upsample_u8 at r = 4, both filters, beside
  the byte floor: the input read once and the output written once at the 6.3 TB/s of a streaming copy.

Every shape is warmed up; ``--rounds`` rounds of ``--kernel-reps`` launches and ``--reps`` compositions, the sides alternating within a
round, a host clock around work that ends in a device synchronise; median / minimum / maximum in milliseconds per call.  Prints one
JSON line.
    python tools/diag/bench_baseline.py [--rounds 5] [--reps 1] [--kernel-reps 10] [--sheet 4096]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch
import torch.nn.functional as F

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

COPY_GBPS = 6300.0      # the streaming-copy figure of DESIGN section 4


def nlm_composition(x, p, s, qmul, qshift, bias, lut):
    """B2 of include/pssr_mi355.h in torch ops: uint8 [planes, 1, H, W] -> uint8 of the same shape."""
    H, W = x.shape[-2:]
    m, P = s + p, 2 * p + 1
    T = F.pad(x.float(), (m, m, m, m), mode="replicate").to(torch.int32)
    a = T[..., s:s + H + 2 * p, s:s + W + 2 * p]
    ys, xs = torch.arange(H, device=x.device), torch.arange(W, device=x.device)
    num = torch.zeros(x.shape, dtype=torch.int64, device=x.device)
    den = torch.zeros_like(num)
    for dy in range(-s, s + 1):
        for dx in range(-s, s + 1):
            d = a - T[..., s + dy:s + dy + H + 2 * p, s + dx:s + dx + W + 2 * p]
            d = d * d
            row = d[..., :, 0:W]
            for k in range(1, P):
                row = row + d[..., :, k:k + W]
            ssd = row[..., 0:H, :]
            for k in range(1, P):
                ssd = ssd + row[..., k:k + H, :]
            q = ((ssd - bias).clamp_(min=0).to(torch.int64) * qmul >> qshift).clamp_(max=255)
            inside = ((ys + dy >= 0) & (ys + dy < H))[:, None] & ((xs + dx >= 0) & (xs + dx < W))[None, :]
            wgt = lut[q] * inside
            num += wgt * T[..., m + dy:m + dy + H, m + dx:m + dx + W]
            den += wgt
    return ((num + (den >> 1)) // den).to(torch.uint8)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=1)
    ap.add_argument("--kernel-reps", type=int, default=10)
    ap.add_argument("--sheet", type=int, default=4096)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_baseline needs an MI355X")
    from pssr2_amd import ops, util
    out = {"rounds": args.rounds, "reps": args.reps, "kernel_reps": args.kernel_reps, "sheet": args.sheet}
    gen = torch.Generator(device="cuda").manual_seed(7)
    lut = torch.tensor(ops.NLM_LUT, dtype=torch.int64, device="cuda")
    sides = []
    for name, planes, side in (("batch", 32, 128), ("sheet", 1, args.sheet)):
        x = torch.randint(0, 256, (planes, 1, side, side), dtype=torch.uint8, device="cuda", generator=gen)
        for p, s in ((2, 7), (3, 10)):
            prm = util._nlm_params(12.0, 10.0, 2 * p + 1)
            if not torch.equal(ops.nlm_u8(x, p, s, *prm), nlm_composition(x, p, s, *prm, lut)):
                raise SystemExit(f"{name}: pssr_nlm_u8 and the composition disagree at p = {p}, s = {s}")
            madds = planes * side * side * (2 * s + 1) ** 2 * (2 * p + 1) ** 2
            sides.append((f"{name}_nlm_p{p}s{s}", lambda x=x, p=p, s=s, prm=prm: ops.nlm_u8(x, p, s, *prm), ("madds", madds), args.kernel_reps))
            sides.append((f"{name}_nlm_p{p}s{s}_composition", lambda x=x, p=p, s=s, prm=prm: nlm_composition(x, p, s, *prm, lut), None, args.reps))
        for filter in ops.UPSAMPLE_FILTERS:
            sides.append((f"{name}_upsample4_{filter}", lambda x=x, filter=filter: ops.upsample_u8(x, 4, filter), ("bytes", planes * side * side * 17),
                          args.kernel_reps))

    times = {name: [] for name, _, _, _ in sides}
    for _, fn, _, _ in sides:              # warm-up of every shape
        fn()
    for _ in range(args.rounds):
        for name, fn, _, reps in sides:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / reps)
    for name, _, work, _ in sides:
        v = times[name]
        med = statistics.median(v)
        out[name] = {"median_ms": round(med, 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
        if work and work[0] == "madds":
            out[name]["patch_madds"] = work[1]
            out[name]["Tmadds_per_s_at_median"] = round(work[1] / med / 1e9, 3)
            out[name]["over_composition"] = round(med / statistics.median(times[name + "_composition"]), 5)
        elif work:
            out[name]["bytes"] = work[1]
            out[name]["GBps_at_median"] = round(work[1] / med / 1e6, 1)
            out[name]["share_of_streaming_copy"] = round(work[1] / med / 1e6 / COPY_GBPS, 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
