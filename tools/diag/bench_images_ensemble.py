"""Cost of the self-ensemble of predict_images and of the spread maps (pssr2_amd/predict.py -> csrc/tiles.hip: pssr_dihedral_batch_u8 / _f32,
pssr_ensemble_reduce_u8, pssr_spread_stack_u8), default ResUNet in bf16, one MI355X:

  images   predict_images(out_dir=None) over ``--tiles`` HBM-resident 128² -> 512² pairs (DevicePairedTileDataset, no noise: every call
           predicts the same pixels), batch 32: ``ensemble=1`` on the ordinary loop (PSSR_HOST_GRAPH=0: the like-for-like reference, the
           loop the ensemble takes), ``ensemble=1`` as shipped (the captured forward: for orientation), ``ensemble=8`` without and with ``spread``
  reduce   pssr_ensemble_reduce_u8 alone at [32 * 8, 1, 512, 512], without and with the spread, against the composition of existing pieces
           that gives the same maps (clip_u8_dihedral into a uint8 buffer, then torch's integer sum, division, amax, amin), and its rate
           over the bytes it must move: 4 E + 1 (+ 1 with the spread) per output pixel
  turn     pssr_dihedral_batch_f32 / _u8 alone for that batch, [32, 1, 128, 128] -> [256, 1, 128, 128]: 4 (1) B read per LR pixel, 4 E written
  sheet    pssr_spread_stack_u8 alone and predict_sheet(spread=True) against spread=False on bench_sheet_blend.py's ``--size``² sheet
           (tiles of 128, overlap 32, batch 128), for ``ensemble`` 1 and 8

Outputs are compared before anything is timed.  ``--rounds`` rounds of ``--reps`` calls (``--kernel-reps`` launches for a kernel alone, so that
its window is milliseconds and not one launch), the configurations alternating, a host clock around work that ends in a device synchronise;
median / minimum / maximum in milliseconds per call.  Prints one JSON line.
    python tools/diag/bench_images_ensemble.py [--rounds 5] [--reps 3] [--kernel-reps 50] [--tiles 256] [--size 2048]"""
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
    ap.add_argument("--kernel-reps", type=int, default=50)
    ap.add_argument("--tiles", type=int, default=256)
    ap.add_argument("--size", type=int, default=2048)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_images_ensemble needs an MI355X")
    from pssr2_amd import ops
    from pssr2_amd.data import DevicePairedTileDataset
    from pssr2_amd.models import ResUNet
    from pssr2_amd.predict import predict_images, predict_sheet
    lr_res, scale, batch, ens = 128, 4, 32, 8
    S = lr_res * scale
    torch.manual_seed(0)
    model = ResUNet(channels=1).cuda().eval()
    model.compute_dtype = torch.bfloat16
    rng = np.random.default_rng(7)
    ds = DevicePairedTileDataset(rng.integers(0, 256, size=(args.tiles, 1, S, S), dtype=np.uint8),
                                 rng.integers(0, 256, size=(args.tiles, 1, lr_res, lr_res), dtype=np.uint8), hr_res=S, lr_scale=scale, val_split=1,
                                 rotation=False, device="cuda")
    out = {"tiles": args.tiles, "lr_res": lr_res, "batch": batch, "sheet_size": args.size, "rounds": args.rounds, "reps": args.reps,
           "kernel_reps": args.kernel_reps}

    def images(ordinary, **kw):
        def run():
            old = os.environ.get("PSSR_HOST_GRAPH")
            if ordinary:
                os.environ["PSSR_HOST_GRAPH"] = "0"
            try:
                return predict_images(model, ds, device="cuda", batch_size=batch, out_dir=None, **kw)
            finally:
                if ordinary:
                    os.environ.pop("PSSR_HOST_GRAPH") if old is None else os.environ.__setitem__("PSSR_HOST_GRAPH", old)
        return run

    # ---- the kernels alone
    y = torch.rand(batch * ens, 1, S, S, device="cuda") * 300 - 20
    lr_f32 = torch.randint(0, 256, (batch, 1, lr_res, lr_res), device="cuda").float()
    lr_u8 = lr_f32.to(torch.uint8)
    q = torch.empty(y.shape, dtype=torch.uint8, device="cuda")

    def composition(spread):
        def run():
            ops.clip_u8_dihedral(y, q, ens, 0)
            m = q.view(batch, ens, 1, S, S)
            mean = (m.sum(1, dtype=torch.int32) // ens).to(torch.uint8)
            return (mean, m.amax(1) - m.amin(1)) if spread else mean
        return run

    mean, dif = ops.ensemble_reduce_u8(y, ens, spread=True)
    want_mean, want_dif = composition(True)()
    if not (torch.equal(mean, want_mean) and torch.equal(dif, want_dif) and torch.equal(ops.ensemble_reduce_u8(y, ens), want_mean)):
        raise SystemExit("pssr_ensemble_reduce_u8 and the composition of clip_u8_dihedral + torch disagree")
    if not torch.equal(ops.dihedral_batch(lr_u8, ens), ops.dihedral_batch(lr_f32, ens)):
        raise SystemExit("pssr_dihedral_batch_u8 and pssr_dihedral_batch_f32 disagree")
    del mean, dif, want_mean, want_dif

    # ---- the sheet
    tile, overlap, sheet_batch = 128, 32, 128
    stride = tile - overlap
    sheet = torch.from_numpy(rng.integers(0, 256, size=(1, args.size, args.size), dtype=np.uint8)).cuda()
    n_rows = n_cols = (args.size - tile) // stride + 1
    out_hw = (n_rows * stride + overlap) * scale
    preds = {e: torch.randint(0, 256, (n_rows * n_cols * e, 1, S, S), dtype=torch.uint8, device="cuda") for e in (1, ens)}

    def sheet_call(e, spread):
        return lambda: predict_sheet(model, sheet, tile_res=tile, overlap=overlap, batch_size=sheet_batch, to_numpy=False, ensemble=e, spread=spread)

    def sheet_kernel(e):
        return lambda: ops.spread_stack_u8(preds[e], 1, n_rows, n_cols, overlap * scale, 0, out_hw, out_hw, e)

    for e in (1, ens):
        if not torch.equal(sheet_call(e, True)()[0], sheet_call(e, False)()):
            raise SystemExit(f"predict_sheet(ensemble={e}): spread=True changed the sheet")

    # ---- predict_images: the outputs agree before anything is timed
    ref = images(True)()
    shipped = images(False)()
    out["shipped_equals_ordinary_loop"] = all(np.array_equal(ref[k], shipped[k]) for k in ref)
    e8, e8_spread = images(False, ensemble=ens)(), images(False, ensemble=ens, spread=True)()
    if not all(np.array_equal(e8[k], e8_spread[0][k]) for k in ref) or list(e8) != list(ref):
        raise SystemExit("predict_images(ensemble=8): spread=True changed the prediction")
    out["ensemble8_pixels_differing_from_ensemble1"] = round(float(np.mean([np.mean(e8[k] != ref[k]) for k in ref])), 4)
    del ref, shipped, e8, e8_spread

    px = batch * S * S
    sides = [("images_ensemble1_ordinary_loop", images(True), None), ("images_ensemble1_as_shipped", images(False), None),
             ("images_ensemble8", images(False, ensemble=ens), None), ("images_ensemble8_spread", images(False, ensemble=ens, spread=True), None),
             ("reduce_kernel", lambda: ops.ensemble_reduce_u8(y, ens), px * (4 * ens + 1)),
             ("reduce_kernel_spread", lambda: ops.ensemble_reduce_u8(y, ens, spread=True), px * (4 * ens + 2)),
             ("reduce_composition", composition(False), None), ("reduce_composition_spread", composition(True), None),
             ("turn_kernel_f32", lambda: ops.dihedral_batch(lr_f32, ens), lr_f32.numel() * (4 + 4 * ens)),
             ("turn_kernel_u8", lambda: ops.dihedral_batch(lr_u8, ens), lr_u8.numel() * (1 + 4 * ens)),
             ("sheet_spread_kernel_1", sheet_kernel(1), preds[1].numel() + out_hw * out_hw),
             ("sheet_spread_kernel_8", sheet_kernel(ens), preds[ens].numel() + out_hw * out_hw),
             ("sheet_call_1", sheet_call(1, False), None), ("sheet_call_1_spread", sheet_call(1, True), None),
             ("sheet_call_8", sheet_call(ens, False), None), ("sheet_call_8_spread", sheet_call(ens, True), None)]
    times = {name: [] for name, _, _ in sides}
    for name, fn, _ in sides:              # warm-up of every shape
        fn()
    for _ in range(args.rounds):
        for name, fn, _ in sides:
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            reps = args.reps if name.startswith(("images_", "sheet_call_")) else args.kernel_reps
            for _ in range(reps):
                fn()
            torch.cuda.synchronize()
            times[name].append((time.perf_counter() - t0) * 1e3 / reps)
    for name, _, nbytes in sides:
        v = times[name]
        out[name] = {"median_ms": round(statistics.median(v), 3), "min_ms": round(min(v), 3), "max_ms": round(max(v), 3)}
        if nbytes:
            out[name]["bytes"] = nbytes
            out[name]["GBps_at_median"] = round(nbytes / statistics.median(v) / 1e6, 1)
    med = {k: v["median_ms"] for k, v in out.items() if isinstance(v, dict)}
    launches = -(-args.tiles // batch)
    out["ensemble8_over_ordinary_ensemble1"] = round(med["images_ensemble8"] / med["images_ensemble1_ordinary_loop"], 3)
    out["new_launches_share_of_ensemble8_spread"] = round(launches * (med["turn_kernel_f32"] + med["reduce_kernel_spread"]) / med["images_ensemble8_spread"], 4)
    out["reduce_over_composition"] = round(med["reduce_kernel_spread"] / med["reduce_composition_spread"], 3)
    print(json.dumps(out))


if __name__ == "__main__":
    main()
