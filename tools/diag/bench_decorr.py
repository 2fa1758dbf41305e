"""Cost of the ring sums of util.decorr (pssr2_amd/ops.py: decorr_rings_u8 -> csrc/frc.hip: pssr_decorr_rings_u8), one MI355X, two shapes
at block side 512 under the Hann window:

  batch    [32, 1, 512, 512]: 32 blocks
  sheet    one 8192 x 8192 plane: 256 blocks

and for each of them
  fused          the four launches of pssr_decorr_rings_u8 (block means, row pass, column pass with the ring reduction, fold)
  composition    what a user could write: the blocks as float32 minus their mean times the window, torch.fft.rfft2, abs and its square
                 weighted for the half spectrum, and index_add_ into float64 ring sums, all on the device (left out, and said so, where
                 this torch build has no device FFT)
  pair           ops.frc_rings_u8(a, a) of the same tree: the cost yardstick for the halved MFMA work (twice the products, no mean pass)
  the f32 MFMA rate of the fused launches over their 12 n^2 (n / 2 + 1) floating-point operations per block (two real n x n x K
  products in the row pass, four in the column pass), beside the 157.3 TFLOP/s of the f32-input MFMA
  ``--split``: the device time of each kernel from torch.profiler, one call per shape

Outputs are compared before anything is timed: the fused sums against the composition evaluated in float64, in the units and within the
rule of tests/test_gpu_decorr.py: per ring r >= 1 |A - A_ref| / sqrt(pop[r] P_ref[r]) and |P - P_ref| / P_ref[r], ring 0 in the units of
the whole block, within 8 x the distance of float32 matrix products in numpy from the float64 FFT on exactly these inputs (seeded host
arrays; checked at the default sizes, for which it was measured).  The distance of the float32 composition (the one that is timed) from
the float64 one is reported beside it.  Every shape is warmed up; ``--rounds`` rounds of ``--kernel-reps`` fused or pair calls and
``--reps`` compositions, the sides alternating within a round, a host clock around work that ends in a device synchronise; median /
minimum / maximum in milliseconds per call.  Prints one JSON line.
    python tools/diag/bench_decorr.py [--rounds 5] [--reps 5] [--kernel-reps 10] [--sheet 8192] [--block 512] [--split]"""
import argparse
import json
import os
import re
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

MFMA_F32_TFLOPS = 157.3
# (err_A, err_P) of tests/_decorr_ref.py's ``errors(rings_f32, rings_ref)`` on exactly the default inputs below, measured on a CPU; the
# fused sums must lie within MARGIN times that of the float64 composition: the tests' rule
F32_ERROR = {"batch": (3.395e-07, 7.915e-07), "sheet": (6.717e-07, 1.381e-06)}
MARGIN = 8


def inputs(n, sheet):
    """The two seeded host arrays, in this order: the seed's stream."""
    rng = np.random.default_rng(7)
    return [(name, rng.integers(0, 256, size=shape, dtype=np.uint8)) for name, shape in (("batch", (32, 1, n, n)), ("sheet", (1, 1, sheet, sheet)))]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--kernel-reps", type=int, default=10)
    ap.add_argument("--sheet", type=int, default=8192)
    ap.add_argument("--block", type=int, default=512)
    ap.add_argument("--split", action="store_true")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_decorr needs an MI355X")
    from pssr2_amd import ops
    n = args.block
    R, K = n // 2, n // 2 + 1
    out = {"block": n, "window": "hann", "rounds": args.rounds, "reps": args.reps, "kernel_reps": args.kernel_reps, "sheet": args.sheet}
    x = torch.arange(n, device="cuda", dtype=torch.float64)
    w = torch.sin(torch.pi * (x + 0.5) / n) ** 2
    w2 = w[:, None] * w[None, :]
    f = torch.arange(n, device="cuda")
    fy = torch.where(f <= R, f, f - n)
    ring = torch.floor(torch.sqrt((fy[:, None] ** 2 + f[None, :K] ** 2).double()) + 0.5).long()
    keep = (ring <= R).flatten()
    ring_kept = ring.flatten()[keep]
    weight = torch.ones(K, device="cuda")
    weight[1:R] = 2
    pop = torch.zeros(R + 1, dtype=torch.float64, device="cuda").index_add_(0, ring_kept, weight.double().expand(n, K).flatten()[keep])

    def composition(a, dtype=torch.float32):
        planes, H, W = a.shape[0] * a.shape[1], a.shape[-2], a.shape[-1]
        nby, nbx = H // n, W // n
        t = a.reshape(planes, H, W)[:, (H - nby * n) // 2:(H - nby * n) // 2 + nby * n, (W - nbx * n) // 2:(W - nbx * n) // 2 + nbx * n]
        blocks = t.reshape(planes, nby, n, nbx, n).permute(0, 1, 3, 2, 4).reshape(planes * nby * nbx, n, n)

        def run():
            # step 1 of the definitions: the integer sum, divided in double, rounded once to float32
            m = (blocks.sum(dim=(-2, -1), dtype=torch.int64).double() / (n * n)).float()
            c = blocks.float() - m[:, None, None]
            mod = torch.fft.rfft2(c.to(dtype) * w2.to(dtype)).abs()
            terms = torch.stack([mod * weight, mod * mod * weight], dim=-1).flatten(1, 2)[:, keep].double()
            return torch.zeros(terms.shape[0], R + 1, 2, dtype=torch.float64, device="cuda").index_add_(1, ring_kept, terms)
        return run

    def errors(got, ref):
        total = ref[..., 1].sum(dim=-1, keepdim=True)
        scale_a, scale_p = (pop * ref[..., 1]).sqrt(), ref[..., 1].clone()
        scale_a[..., :1], scale_p[..., :1] = total.sqrt(), total
        return ((got[..., 0] - ref[..., 0]).abs() / scale_a).max().item(), ((got[..., 1] - ref[..., 1]).abs() / scale_p).max().item()

    sides = []
    for name, host in inputs(n, args.sheet):
        a = torch.from_numpy(host).cuda()
        fused = ops.decorr_rings_u8(a, n)
        nblocks = fused.shape[0] * fused.shape[1]
        flops = 12 * n * n * K * nblocks
        sides.append((f"{name}_fused", lambda a=a: ops.decorr_rings_u8(a, n), flops, args.kernel_reps))
        sides.append((f"{name}_pair", lambda a=a: ops.frc_rings_u8(a, a, n), 2 * flops, args.kernel_reps))
        try:
            comp = composition(a)
            got32 = comp().reshape(fused.shape)
            want = composition(a, torch.float64)().reshape(fused.shape)
        except Exception as e:                                  # a torch build without a device FFT
            out[f"{name}_composition"] = f"not available: {str(e).splitlines()[0][:120]}"
        else:
            err, err32 = errors(fused, want), errors(got32, want)
            out[f"{name}_error_fused"], out[f"{name}_error_composition"] = err, err32
            if args.block == 512 and args.sheet == 8192 and not (err[0] <= MARGIN * F32_ERROR[name][0] and err[1] <= MARGIN * F32_ERROR[name][1]):
                raise SystemExit(f"{name}: pssr_decorr_rings_u8 is {err[0]:.3e} (A) and {err[1]:.3e} (P) from the float64 composition, "
                                 f"the float32 one {err32[0]:.3e} and {err32[1]:.3e}")
            sides.append((f"{name}_composition", comp, None, args.reps))
        if args.split:
            from torch.profiler import ProfilerActivity, profile
            with profile(activities=[ProfilerActivity.CUDA]) as prof:
                ops.decorr_rings_u8(a, n)
                torch.cuda.synchronize()
            out[f"{name}_kernels_us"] = {}
            for e in prof.key_averages():                       # device time of every launch of a kernel, summed over the call's chunks
                m = re.search(r"frc_\w+_kernel", e.key)
                if m:
                    total = getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)
                    out[f"{name}_kernels_us"][m.group(0)] = round(out[f"{name}_kernels_us"].get(m.group(0), 0.0) + total, 1)

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
    for name, _, flops, _ in sides:
        v = times[name]
        out[name] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
        if flops:
            out[name]["flops"] = flops
            out[name]["TFLOPs_at_median"] = round(flops / statistics.median(v) / 1e9, 2)
            out[name]["share_of_f32_mfma_peak"] = round(flops / statistics.median(v) / 1e9 / MFMA_F32_TFLOPS, 4)
    for name in ("batch", "sheet"):
        out[f"{name}_fused_over_pair"] = round(out[f"{name}_fused"]["median_ms"] / out[f"{name}_pair"]["median_ms"], 4)
        if isinstance(out.get(f"{name}_composition"), dict):
            out[f"{name}_fused_over_composition"] = round(out[f"{name}_fused"]["median_ms"] / out[f"{name}_composition"]["median_ms"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
