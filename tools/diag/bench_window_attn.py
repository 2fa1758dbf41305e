"""Benchmark of the fused shifted-window attention (pssr2_amd/ops.py: ``window_attn_fwd`` / ``window_attn_bwd`` -> csrc/window_attn.hip)
against the torch composition it replaces inside a SwinIR block, at the default configuration: batch 8, 128 x 128 tokens, C = 96,
6 heads, window 8, shift 4.  Both sides start from the output of the qkv Linear, [B, H, W, 3C], and end with the attention output
[B, H, W, C] (forward) or with the gradients of qkv and of the bias table (forward + backward); the Linears are left out of both.

  fused        one forward launch; two backward launches (the second adds the bias-table partial sums)
  composition  roll, window partition, q k^T, bias gather, mask add, softmax, P v, window reverse, roll back, and autograd's backward

The results are compared first (also the warm-up).  ``--rounds`` rounds of ``--reps`` calls, the two sides alternating, a host clock
around work that ends in a device synchronise; median / minimum / maximum per side in milliseconds per call, and the peak of
``torch.cuda.max_memory_allocated`` over one call on top of the inputs.  Prints one JSON line.
    python tools/diag/bench_window_attn.py [--rounds 7] [--reps 10] [--batch 8] [--size 128]"""
import argparse
import json
import os
import statistics
import sys
import time

import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rounds", type=int, default=7)
    ap.add_argument("--reps", type=int, default=10)
    ap.add_argument("--batch", type=int, default=8)
    ap.add_argument("--size", type=int, default=128)
    args = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("bench_window_attn needs an MI355X")
    from pssr2_amd import ops
    from pssr2_amd.swinir import SwinTransformerBlock, window_partition, window_reverse
    b, h, w, c, heads, ws, shift = args.batch, args.size, args.size, 96, 6, 8, 4
    n, scale = ws * ws, (c // heads) ** -0.5
    block = SwinTransformerBlock(c, (h, w), heads, window_size=ws, shift_size=shift).cuda()
    index, mask_f32 = block.attn.relative_position_index.view(-1), block.attn_mask
    g = torch.Generator().manual_seed(0)
    out = {"batch": b, "size": h, "channels": c, "heads": heads, "window": ws, "shift": shift, "rounds": args.rounds, "reps": args.reps}

    for dtype, tag in ((torch.float32, "f32"), (torch.bfloat16, "bf16")):
        qkv = torch.randn(b, h, w, 3 * c, generator=g).cuda().to(dtype)
        dout = torch.randn(b, h, w, c, generator=g).cuda().to(dtype)
        bias = (0.5 * torch.randn((2 * ws - 1) ** 2, heads, generator=g)).cuda()
        mask = mask_f32.to(dtype)

        def composition(qkv, bias):
            x = torch.roll(qkv, (-shift, -shift), (1, 2))
            win = window_partition(x, ws).view(-1, n, 3, heads, c // heads).permute(2, 0, 3, 1, 4)
            q, k, v = win[0], win[1], win[2]
            attn = (q * scale) @ k.transpose(-2, -1)
            attn = attn + bias.to(dtype)[index].view(n, n, heads).permute(2, 0, 1).contiguous().unsqueeze(0)
            nw = mask.shape[0]
            attn = (attn.view(-1, nw, heads, n, n) + mask.unsqueeze(1).unsqueeze(0)).view(-1, heads, n, n)
            o = (torch.softmax(attn, dim=-1) @ v).transpose(1, 2).reshape(-1, ws, ws, c)
            return torch.roll(window_reverse(o, ws, h, w), (shift, shift), (1, 2))

        def fused_fwd():
            return ops.window_attn_fwd(qkv, bias, heads, ws, shift, scale)[0]

        def comp_fwd():
            with torch.no_grad():
                return composition(qkv, bias)

        def fused_fwd_bwd():
            o, lse = ops.window_attn_fwd(qkv, bias, heads, ws, shift, scale)
            return ops.window_attn_bwd(qkv, bias, lse, dout, heads, ws, shift, scale)

        def comp_fwd_bwd():
            q, bt = qkv.detach().requires_grad_(True), bias.detach().requires_grad_(True)
            composition(q, bt).backward(dout)
            return q.grad, bt.grad

        def close(a, b_, what):
            err = float((a.float() - b_.float()).abs().max() / b_.float().abs().max())
            if not err < (1e-4 if dtype == torch.float32 else 1e-1):          # a wrong index, mask or bias shows at 1e-1 and above
                raise SystemExit(f"{tag} {what}: fused and composition disagree ({err:.3g})")
            return err

        agree = {"out": close(fused_fwd(), comp_fwd(), "out")}
        (dq_f, db_f), (dq_c, db_c) = fused_fwd_bwd(), comp_fwd_bwd()
        agree["dqkv"], agree["dbias"] = close(dq_f, dq_c, "dqkv"), close(db_f, db_c, "dbias")
        del dq_f, db_f, dq_c, db_c
        res = {"max_rel_difference": {k: float(f"{v:.3g}") for k, v in agree.items()}}
        for leg, sides in (("forward", (("fused", fused_fwd), ("composition", comp_fwd))),
                           ("forward_backward", (("fused", fused_fwd_bwd), ("composition", comp_fwd_bwd)))):
            times, peak = {name: [] for name, _ in sides}, {}
            for name, fn in sides:
                torch.cuda.synchronize()
                torch.cuda.empty_cache()
                base = torch.cuda.memory_allocated()
                torch.cuda.reset_peak_memory_stats()
                fn()
                torch.cuda.synchronize()
                peak[name] = round((torch.cuda.max_memory_allocated() - base) / 2 ** 20, 1)
            for _ in range(args.rounds):
                for name, fn in sides:
                    torch.cuda.synchronize()
                    t0 = time.perf_counter()
                    for _ in range(args.reps):
                        fn()
                    torch.cuda.synchronize()
                    times[name].append((time.perf_counter() - t0) * 1e3 / args.reps)
            res[leg] = {name: {"median_ms": round(statistics.median(v), 4), "min_ms": round(min(v), 4), "max_ms": round(max(v), 4),
                               "peak_mib": peak[name]} for name, v in times.items()}
        out[tag] = res
    print(json.dumps(out))


if __name__ == "__main__":
    main()
