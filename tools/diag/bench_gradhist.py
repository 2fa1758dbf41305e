"""Micro-benchmark of the GradHist kernels (csrc/hist.hip): forward + backward of both histograms of one crappifier-loss step
(batch 16, 1x128^2 noise profiles, 512 bins, sigma 5) against the reference's formula (pssr/models/_blocks.py:94-112) in torch on
the same GPU.  Prints one JSON line.   python tools/diag/bench_gradhist.py [--iters 50]"""
import argparse
import json
import os
import sys

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def torch_gradhist(x, bins=512, lo=-256, hi=256, sigma=5):
    batch, size = x.shape[0], x[0].numel()
    delta = float(hi - lo) / float(bins)
    centers = (float(lo) + delta * (torch.arange(bins).float() + 0.5)).to(x.device)
    s = torch.sigmoid((x.flatten(start_dim=1)[:, None, :] - centers[:, None]) * sigma)
    diff = torch.cat([torch.ones((batch, 1, size), device=x.device), s], 1) - torch.cat([s, torch.zeros((batch, 1, size), device=x.device)], 1)
    return diff.sum(-1)[:, :-1]


def timed(fn, iters):
    fn()
    torch.cuda.synchronize()
    a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    a.record()
    for _ in range(iters):
        fn()
    b.record()
    torch.cuda.synchronize()
    return a.elapsed_time(b) / iters


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--iters", type=int, default=50)
    args = ap.parse_args()
    from pssr2_amd.models import GradHist
    gen = torch.Generator().manual_seed(0)
    p = (torch.randn(16, 1, 128, 128, generator=gen) * 13).cuda().requires_grad_(True)
    t = (torch.randn(16, 1, 128, 128, generator=gen) * 13).cuda()
    g = torch.randn(16, 512, generator=gen).cuda()
    hist = GradHist()

    def step(fn):
        def run():
            p.grad = None
            hp, ht = fn(p), fn(t)
            ((hp - ht) * g).sum().backward()
        return run

    def hip_fwd():
        with torch.no_grad():
            hist(p), hist(t)

    out = {"shape": [16, 1, 128, 128], "bins": 512, "sigma": 5,
           "hip_fwd_ms": timed(hip_fwd, args.iters), "hip_fwd_bwd_ms": timed(step(hist), args.iters)}
    out["torch_fwd_bwd_ms"] = timed(step(torch_gradhist), max(3, args.iters // 10))
    torch.cuda.reset_peak_memory_stats()
    step(torch_gradhist)()
    torch.cuda.synchronize()
    out["torch_peak_gb"] = torch.cuda.max_memory_allocated() / 1e9
    print(json.dumps(out))


if __name__ == "__main__":
    main()
