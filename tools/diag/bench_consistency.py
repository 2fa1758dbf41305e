"""Cost of the consistency maps (pssr2_amd/util.py: consistency_map -> csrc/consistency.hip: pssr_reduce_moments_u8, pssr_consistency_map_u8),
one MI355X, two shapes at scale 4:

  batch    [32, 1, 512, 512] predictions against [32, 1, 128, 128] LR items (a predict_images batch)
  sheet    one 16384 x 16384 sheet plane against its 4096 x 4096 LR sheet (``--sheet-lr`` sets the LR side)

and for each of them
  reduce_fused         the fused reduction + moments launch (with its tap-table and fold launches)
  reduce_composition   what it replaces: ops.bilinear_down_u8 (two launches, an [H][w] intermediate in HBM) plus torch's int64 sums over d and l
  map                  the map + squared-error launch
  the fused launch's rate over its algorithmic bytes, s^2 n + 2 n per plane (y read, l read, d written), beside the 6.3 TB/s of a streaming copy

  sheet_call           predict_sheet on bench_sheet_blend.py's ``--size``^2 sheet (default ResUNet in bf16, tiles of 128, overlap 32, batch 128)
                       with consistency=False and True: the surcharge of the whole feature on a call

Outputs are compared before anything is timed (the fused launch against the composition, bit for bit).  Every shape is warmed up; ``--rounds``
rounds of ``--kernel-reps`` launches (``--reps`` calls for predict_sheet), so that a window is milliseconds and not one launch, the
configurations alternating within a round, a host clock around work that ends in a device synchronise; median / minimum / maximum in
milliseconds per call.  Prints one JSON line.
    python tools/diag/bench_consistency.py [--rounds 5] [--reps 3] [--kernel-reps 50] [--sheet-lr 4096] [--size 2048]"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))

COPY_GBPS = 6300.0      # the streaming-copy figure of DESIGN section 4


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--kernel-reps", type=int, default=50)
    ap.add_argument("--sheet-lr", type=int, default=4096)
    ap.add_argument("--size", type=int, default=2048)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_consistency needs an MI355X")
    from pssr2_amd import ops
    from pssr2_amd.models import ResUNet
    from pssr2_amd.predict import predict_sheet
    from pssr2_amd.util import _consistency_fit
    scale = 4
    out = {"scale": scale, "rounds": args.rounds, "reps": args.reps, "kernel_reps": args.kernel_reps, "sheet_lr": args.sheet_lr, "sheet_size": args.size}
    gen = torch.Generator(device="cuda").manual_seed(7)

    def composition(y, l):
        def run():
            d = ops.bilinear_down_u8(y, *l.shape[-2:])
            df, lf = d.flatten(-2).to(torch.int64).flatten(0, -2), l.flatten(-2).to(torch.int64).flatten(0, -2)
            return d, torch.stack([df.sum(-1), lf.sum(-1), (df * df).sum(-1), (df * lf).sum(-1), (lf * lf).sum(-1)], -1)
        return run

    sides = []
    for name, planes, side in (("batch", 32, 128), ("sheet", 1, args.sheet_lr)):
        l = torch.randint(0, 256, (planes, 1, side, side), dtype=torch.uint8, device="cuda", generator=gen)
        y = torch.randint(0, 256, (planes, 1, side * scale, side * scale), dtype=torch.uint8, device="cuda", generator=gen)
        d, sums = ops.reduce_moments_u8(y, l)
        want_d, want_sums = composition(y, l)()
        if not (torch.equal(d, want_d) and torch.equal(sums, want_sums)):
            raise SystemExit(f"{name}: pssr_reduce_moments_u8 and the composition of bilinear_down_u8 + torch disagree")
        n = side * side
        lut = torch.tensor([_consistency_fit(n, row, "affine")[3] for row in sums.cpu().tolist()], dtype=torch.int32).cuda()
        cmap, sse = ops.consistency_map_u8(d, l, lut)
        e = (256 * l.to(torch.int64) - lut.to(torch.int64).gather(1, d.flatten(1).to(torch.int64)).view(d.shape)).abs()
        if not (torch.equal(cmap, ((e + 128) >> 8).clamp(max=255).to(torch.uint8)) and torch.equal(sse, (e * e).flatten(1).sum(1))):
            raise SystemExit(f"{name}: pssr_consistency_map_u8 and torch disagree")
        del want_d, want_sums, e, cmap, sse
        sides += [(f"{name}_reduce_fused", lambda y=y, l=l: ops.reduce_moments_u8(y, l), planes * n * (scale * scale + 2)),
                  (f"{name}_reduce_composition", composition(y, l), None),
                  (f"{name}_map", lambda d=d, l=l, lut=lut: ops.consistency_map_u8(d, l, lut), planes * n * 3)]

    torch.manual_seed(0)
    model = ResUNet(channels=1).cuda().eval()
    model.compute_dtype = torch.bfloat16
    sheet = torch.from_numpy(np.random.default_rng(7).integers(0, 256, size=(1, args.size, args.size), dtype=np.uint8)).cuda()

    def sheet_call(consistency):
        return lambda: predict_sheet(model, sheet, tile_res=128, overlap=32, batch_size=128, to_numpy=False, consistency=consistency)

    if not torch.equal(sheet_call(True)()[0], sheet_call(False)()):
        raise SystemExit("predict_sheet: consistency=True changed the sheet")
    sides += [("sheet_call", sheet_call(False), None), ("sheet_call_consistency", sheet_call(True), None)]

    times = {name: [] for name, _, _ in sides}
    for name, fn, _ in sides:              # warm-up of every shape
        fn()
    for _ in range(args.rounds):
        for name, fn, _ in sides:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            reps = args.reps if name.startswith("sheet_call") else args.kernel_reps
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / reps)
    for name, _, nbytes in sides:
        v = times[name]
        out[name] = {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4)}
        if nbytes:
            out[name]["bytes"] = nbytes
            out[name]["GBps_at_median"] = round(nbytes / statistics.median(v) / 1e6, 1)
            out[name]["share_of_streaming_copy"] = round(nbytes / statistics.median(v) / 1e6 / COPY_GBPS, 3)
    med = {k: v["median_ms"] for k, v in out.items() if isinstance(v, dict)}
    for name in ("batch", "sheet"):
        out[f"{name}_fused_over_composition"] = round(med[f"{name}_reduce_fused"] / med[f"{name}_reduce_composition"], 3)
    out["sheet_call_surcharge_ms"] = round(med["sheet_call_consistency"] - med["sheet_call"], 3)
    out["sheet_call_surcharge_share"] = round(med["sheet_call_consistency"] / med["sheet_call"] - 1, 4)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
