"""Cost of the (ring, sector) sums of util.frc_sectors (pssr2_amd/ops.py: frc_sectors_u8 -> csrc/frc.hip: pssr_frc_sectors_u8), one MI355X,
the two shapes of bench_frc.py at block side 512 under the Hann window, at S = 2 and S = 8 sectors:

  batch    [32, 1, 512, 512] against the same shape: 32 blocks
  sheet    one 8192 x 8192 plane against another: 256 blocks

and for each of them
  sectors_S      the three launches of pssr_frc_sectors_u8 (row pass, column pass with the sectorial reduction, fold)
  rings          the unsectored pssr_frc_rings_u8 of the same tree: the yardstick for what the S-fold partial rows and the sector
                 pointer cost beside the shared transform
  composition_S  what a user could write: the blocks as float32 times the window, torch.fft.rfft2, the three products weighted for the
                 half spectrum, and index_add_ over ring * S + sector into float64 (left out, and said so, without a device FFT)
  ``--split``: the device time of each kernel from torch.profiler, one call per shape and S

Outputs are compared before anything is timed: the sector sums, added over the sectors, against the unsectored call within 1e-12
sqrt(Saa Sbb) (regrouping a ring's fewer than 3300 terms), and every cell against the composition evaluated in float64 within the rule of
tests/test_gpu_sectors.py: 8 x the distance of the float32 numpy restatement from the float64 FFT on exactly these inputs (seeded host
arrays, bench_frc.py's; checked at the default sizes, for which it was measured), in units of the whole ring's sqrt(Saa Sbb).  Medians of
``--rounds`` rounds with minimum and maximum, the sides alternating within a round; a host clock around work that ends in a device
synchronise.  Prints one JSON line.
    python tools/diag/bench_sectors.py [--rounds 5] [--reps 5] [--kernel-reps 10] [--sheet 8192] [--block 512] [--split]"""
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

SECTORS = (2, 8)
# max over the cells of |sectors_f32 - sectors_ref| / sqrt(Saa Sbb) of the whole ring (tests/_sector_ref.py) on exactly the default inputs
# below, measured on a CPU
F32_ERROR = {("batch", 2): 6.583e-05, ("batch", 8): 4.059e-05, ("sheet", 2): 1.149e-04, ("sheet", 8): 8.783e-05}
MARGIN = 8


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
        raise SystemExit("bench_sectors needs an MI355X")
    from pssr2_amd import ops
    n = args.block
    R, K = n // 2, n // 2 + 1
    out = {"block": n, "window": "hann", "sectors": list(SECTORS), "rounds": args.rounds, "reps": args.reps, "kernel_reps": args.kernel_reps,
           "sheet": args.sheet}
    rng = np.random.default_rng(7)
    x = torch.arange(n, device="cuda", dtype=torch.float64)
    w = torch.sin(torch.pi * (x + 0.5) / n) ** 2
    w2 = w[:, None] * w[None, :]
    f = torch.arange(n, device="cuda")
    fy = torch.where(f <= R, f, f - n)
    ring = torch.floor(torch.sqrt((fy[:, None] ** 2 + f[None, :K] ** 2).double()) + 0.5).long()
    keep = (ring <= R).flatten()
    weight = torch.ones(K, device="cuda")
    weight[1:R] = 2

    def cells_of(S):
        """ring * S + sector of the kept columns, from the integer rule of include/pssr_mi355.h."""
        bx, by = (torch.from_numpy(t.astype(np.int64)).cuda() for t in ops.frc_sector_bounds(S))
        up = fy[:, None] >= 0
        gx, gy = torch.where(up, f[None, :K], -f[None, :K]), fy[:, None].abs().expand(n, K)
        sector = (bx[:, None, None] * gy - by[:, None, None] * gx >= 0).sum(dim=0) % S
        return (ring * S + sector).flatten()[keep]

    def composition(a, b, S, dtype=torch.float32):
        planes, H, W = a.shape[0] * a.shape[1], a.shape[-2], a.shape[-1]
        nby, nbx = H // n, W // n
        cells = cells_of(S)

        def blocks(t):
            t = t.reshape(planes, H, W)[:, (H - nby * n) // 2:(H - nby * n) // 2 + nby * n, (W - nbx * n) // 2:(W - nbx * n) // 2 + nbx * n]
            return t.reshape(planes, nby, n, nbx, n).permute(0, 1, 3, 2, 4).reshape(planes * nby * nbx, n, n)

        def run():
            fa, fb = torch.fft.rfft2(blocks(a).to(dtype) * w2.to(dtype)), torch.fft.rfft2(blocks(b).to(dtype) * w2.to(dtype))
            terms = torch.stack([(fa * fb.conj()).real * weight, (fa.real ** 2 + fa.imag ** 2) * weight, (fb.real ** 2 + fb.imag ** 2) * weight], dim=-1)
            terms = terms.flatten(1, 2)[:, keep].double()
            return torch.zeros(terms.shape[0], (R + 1) * S, 3, dtype=torch.float64, device="cuda").index_add_(1, cells, terms)
        return run

    sides = []
    for name, shape in (("batch", (32, 1, n, n)), ("sheet", (1, 1, args.sheet, args.sheet))):         # this order: the seed's stream
        a = rng.integers(0, 256, size=shape, dtype=np.uint8)      # host arrays from a seed: the bound below was measured on exactly these
        b = np.clip(a.astype(np.int16) + rng.integers(-40, 41, size=shape, dtype=np.int16), 0, 255).astype(np.uint8)
        a, b = torch.from_numpy(a).cuda(), torch.from_numpy(b).cuda()
        rings = ops.frc_rings_u8(a, b, n)
        scale = (rings[..., 1] * rings[..., 2]).sqrt()
        sides.append((f"{name}_rings", lambda a=a, b=b: ops.frc_rings_u8(a, b, n), args.kernel_reps))
        for S in SECTORS:
            fused = ops.frc_sectors_u8(a, b, n, S)
            if not ((fused.sum(dim=-2) - rings).abs() <= 1e-12 * scale[..., None]).all():
                raise SystemExit(f"{name}, S = {S}: the sectors do not add up to the ring sums")
            sides.append((f"{name}_sectors_{S}", lambda a=a, b=b, S=S: ops.frc_sectors_u8(a, b, n, S), args.kernel_reps))
            try:
                comp = composition(a, b, S)
                got32 = comp().reshape(fused.shape)
                want = composition(a, b, S, torch.float64)().reshape(fused.shape)
            except Exception as e:                              # a torch build without a device FFT
                out[f"{name}_composition_{S}"] = f"not available: {str(e).splitlines()[0][:120]}"
            else:
                whole = want.sum(dim=-2)
                unit = (whole[..., 1] * whole[..., 2]).sqrt()[..., None, None]
                err, err32 = ((fused - want).abs() / unit).max().item(), ((got32 - want).abs() / unit).max().item()
                out[f"{name}_error_sectors_{S}"], out[f"{name}_error_composition_{S}"] = err, err32
                if args.block == 512 and args.sheet == 8192 and not err <= MARGIN * F32_ERROR[name, S]:
                    raise SystemExit(f"{name}, S = {S}: pssr_frc_sectors_u8 is {err:.3e} of sqrt(Saa Sbb) from the float64 composition, the float32 "
                                     f"one {err32:.3e}")
                sides.append((f"{name}_composition_{S}", comp, args.reps))
            if args.split:
                from torch.profiler import ProfilerActivity, profile
                with profile(activities=[ProfilerActivity.CUDA]) as prof:
                    ops.frc_sectors_u8(a, b, n, S)
                    torch.cuda.synchronize()
                split = out[f"{name}_kernels_us_{S}"] = {}
                for e in prof.key_averages():                   # device time of every launch of a kernel, summed over the call's chunks
                    m = re.search(r"frc_\w+_kernel", e.key)
                    if m:
                        total = getattr(e, "device_time_total", None) or getattr(e, "cuda_time_total", 0.0)
                        split[m.group(0)] = round(split.get(m.group(0), 0.0) + total, 1)

    times = {name: [] for name, _, _ in sides}
    for name, fn, _ in sides:                 # warm-up of every shape
        fn()
    for _ in range(args.rounds):
        for name, fn, reps in sides:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / reps)
    for name, _, _ in sides:
        v = times[name]
        out[name] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
    for name in ("batch", "sheet"):
        for S in SECTORS:
            out[f"{name}_sectors_{S}_over_rings"] = round(out[f"{name}_sectors_{S}"]["median_ms"] / out[f"{name}_rings"]["median_ms"], 4)
            if isinstance(out.get(f"{name}_composition_{S}"), dict):
                out[f"{name}_sectors_{S}_over_composition"] = round(out[f"{name}_sectors_{S}"]["median_ms"] / out[f"{name}_composition_{S}"]["median_ms"], 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
