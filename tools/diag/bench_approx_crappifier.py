"""Time of one call of approximate_crappifier's objective (pssr2_amd/train.py:_Crappifier_Objective.sample) on the device for N pairs of
512^2 -> 128^2, its launches one by one (HIP events), the one-off construction, and the same formula in numpy on one host thread
(per pair: Pillow reduction of HR, AdditiveGaussian on numpy, two np.histogram, two means -- what pssr/train.py:354-386 does per call).
The profile kernel is reported against its algorithmic bytes (5 B per value for a float32 first operand, 2 B for uint8) at the
6.3 TB/s a streaming copy reaches on an MI355X.  Prints one JSON line per N.

    python tools/diag/bench_approx_crappifier.py [--pairs 256 2048] [--iters 50] [--host-pairs 32] [--lib path/to/libpssr_mi355_<variant>.so]
"""
import argparse
import json
import os
import random
import sys
import time

import numpy as np
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
COPY_TBS = 6.3


def timed(fn, iters):
    """Mean milliseconds per call between two device events, after a warm-up call."""
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def make_pairs(n, base=32):
    """n pairs from `base` synthetic tiles (rolled copies beyond that): uint8 HR [n, 1, 512, 512], LR = reduction + N(2, 9)."""
    from pssr2_amd.data import _resize_bilinear_u8, synthetic_em_tile
    tiles = [synthetic_em_tile(i, 512) for i in range(min(n, base))]
    hr = np.stack([np.roll(tiles[i % len(tiles)], 17 * (i // len(tiles)), axis=-1) for i in range(n)])
    ds = np.stack([_resize_bilinear_u8(t, 128) for t in hr])
    lr = np.clip(np.round(ds + np.random.RandomState(1).normal(2, 9, ds.shape)), 0, 255).astype(np.uint8)
    return hr, lr


def host_objective(hr, lr, params):
    """The objective of one call on the host, written from its definition; returns (value, seconds in the reduction alone)."""
    from pssr2_amd.crappifiers import AdditiveGaussian
    from pssr2_amd.data import _resize_bilinear_u8
    bins, losses, t_reduce = np.arange(-256, 256), [], 0.0
    for h, l in zip(hr, lr):
        t0 = time.perf_counter()
        ds = _resize_bilinear_u8(h, l.shape[-1])
        t_reduce += time.perf_counter() - t0
        base = ds.astype(np.float32)
        pred = AdditiveGaussian(*params).crappify(ds).astype(np.float32) - base
        target = l.astype(np.float32) - base
        p, t = np.histogram(pred.ravel(), bins)[0], np.histogram(target.ravel(), bins)[0]
        losses.append(np.mean((t - p) ** 2) / l.shape[-1] ** 2 + abs(target.mean() - pred.mean()))
    return sum(losses) / len(losses), t_reduce


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--pairs", type=int, nargs="+", default=[256, 2048])
    ap.add_argument("--iters", type=int, default=50)
    ap.add_argument("--host-pairs", type=int, default=32)
    ap.add_argument("--lib", default=None, help="a variant build of the library to load instead of the package's")
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_approx_crappifier needs an MI355X; there is nothing to measure on the host alone")
    from pssr2_amd import _lib as L, ops
    if args.lib:
        from pathlib import Path
        L._LIB_PATH = Path(args.lib).resolve()
    from pssr2_amd.crappifiers import AdditiveGaussian
    from pssr2_amd.data import DevicePairedTileDataset
    from pssr2_amd.train import _Crappifier_Objective

    for n in args.pairs:
        hr, lr = make_pairs(n)
        ds = DevicePairedTileDataset(hr, lr, 512, 4)
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        obj = _Crappifier_Objective(AdditiveGaussian, ds, n, device="cuda", seed=0)
        torch.cuda.synchronize()
        out = {"pairs": n, "lr": [1, 128, 128], "lib": args.lib or "package", "construct_ms": (time.perf_counter() - t0) * 1e3}
        random.seed(0)
        obj.sample([9.0, 2.0])
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(args.iters):
            value = obj.sample([9.0, 2.0])            # ends in .item(): a device synchronise
        out["call_ms"] = (time.perf_counter() - t0) * 1e3 / args.iters
        out["value"] = value
        # the launches of a call, one by one
        idx = torch.randperm(n, device="cuda")
        sel = obj.ds_hr.index_select(0, idx)
        x = ops.u8_to_f32(sel)
        lr_hat = ops.crappify_gaussian(x, 9.0, 2.0, 0.0, 0, 0, 0)
        ph, ps = ops.noise_profile(lr_hat, sel)
        lr_dev = ds.lr_images.contiguous()
        values = sel.numel()
        out["gather_ms"] = timed(lambda: obj.ds_hr.index_select(0, idx), args.iters)
        out["u8_to_f32_ms"] = timed(lambda: ops.u8_to_f32(sel), args.iters)
        out["crappify_ms"] = timed(lambda: ops.crappify_gaussian(x, 9.0, 2.0, 0.0, 0, 0, 0), args.iters)
        out["profile_f32_ms"] = timed(lambda: ops.noise_profile(lr_hat, sel), args.iters)
        out["profile_u8_ms"] = timed(lambda: ops.noise_profile(lr_dev, obj.ds_hr), args.iters)
        out["loss_ms"] = timed(lambda: ops.noise_profile_loss(ph, ps, obj.target_hist, obj.target_sum, obj.per_image, 128), args.iters)
        for key, bytes_per in (("profile_f32", 5), ("profile_u8", 2)):
            floor_ms = values * bytes_per / (COPY_TBS * 1e12) * 1e3
            out[f"{key}_floor_ms"] = floor_ms
            out[f"{key}_TBs"] = values * bytes_per / (out[f"{key}_ms"] * 1e-3) / 1e12
            out[f"{key}_share_of_copy"] = floor_ms / out[f"{key}_ms"]
        # the host: one thread, a subset, scaled per pair
        m = min(args.host_pairs, n)
        np.random.seed(0)
        host_objective(hr[:2], lr[:2], (9.0, 2.0))
        t0 = time.perf_counter()
        _, t_reduce = host_objective(hr[:m], lr[:m], (9.0, 2.0))
        per_pair = (time.perf_counter() - t0) / m
        out["host_pairs_timed"] = m
        out["host_ms_per_pair"] = per_pair * 1e3
        out["host_ms_per_pair_without_reduction"] = (per_pair - t_reduce / m) * 1e3
        out["host_call_ms_scaled"] = per_pair * n * 1e3
        out["speedup_per_call"] = out["host_call_ms_scaled"] / out["call_ms"]
        print(json.dumps(out), flush=True)
        del obj, ds, sel, x, lr_hat, lr_dev
        torch.cuda.empty_cache()


if __name__ == "__main__":
    main()
