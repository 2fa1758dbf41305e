"""Cases, weights and inputs shared by tools/gen_golden_swinir.py and the SwinIR tests (tests/golden/swinir.npz stores neither weights
nor inputs: both sides draw them here from ``numpy.random.default_rng``)."""
from __future__ import annotations

import math

import numpy as np
import torch

# name: (constructor arguments, input shape).  All with drop_path_rate=0: the stochastic-depth stream is not pinned.
CASES = {
    # one group, window 8 on 16 x 24 = input_resolution: the mask buffer, head dim 16
    "a": (dict(image_size=(16, 24), channels=1, scale=2, embed_dim=32, depths=[2], num_heads=[2], window_size=8,
               upsampler="pixelshuffledirect", drop_path_rate=0), (2, 1, 16, 24)),
    # 3 -> 1 channels, window 4, head dims 10 and 30: rows that are not 16-byte aligned
    "b": (dict(image_size=12, channels=[3, 1], scale=4, embed_dim=30, depths=[2, 2], num_heads=[3, 1], window_size=4,
               upsampler="pixelshuffledirect", drop_path_rate=0), (2, 3, 12, 12)),
    # 13 x 19 is reflect-padded to 16 x 24, which is not input_resolution (32 x 32): the mask is made per call
    "c": (dict(image_size=32, channels=1, scale=2, embed_dim=32, depths=[2], num_heads=[2], window_size=8, upsampler="pixelshuffle",
               drop_path_rate=0), (2, 1, 13, 19)),
    # no upsampler, 3conv tails, absolute position embedding
    "d": (dict(image_size=16, channels=1, scale=2, embed_dim=32, depths=[2], num_heads=[2], window_size=8, upsampler=None,
               resi_connection="3conv", ape=True, drop_path_rate=0), (2, 1, 16, 16)),
}
SEED = {"a": 301, "b": 302, "c": 303, "d": 304}


def fill_state(model, seed):
    """Fills every floating-point ``state_dict`` entry except the attn_mask buffers, in sorted key order: LayerNorm weights 1 + 0.2 n,
    bias tables 0.5 n, matrices and conv weights 1.5 n / sqrt(fan_in), vectors and the position embedding 0.1 n (n standard normal)."""
    rng = np.random.default_rng(seed)
    sd = model.state_dict()
    with torch.no_grad():
        for key in sorted(sd):
            t = sd[key]
            if not t.is_floating_point() or key.endswith("attn_mask"):
                continue
            n = rng.standard_normal(tuple(t.shape))
            if key.endswith("relative_position_bias_table"):
                v = 0.5 * n
            elif key.endswith("absolute_pos_embed") or (t.dim() == 1 and not key.endswith(".weight")):
                v = 0.1 * n
            elif t.dim() == 1:
                v = 1 + 0.2 * n
            else:
                v = n * 1.5 / math.sqrt(int(np.prod(t.shape[1:])))
            t.copy_(torch.from_numpy(v).to(t.dtype))
    return model


def case_input(name):
    """float64 input in [0, 1)."""
    return np.random.default_rng(SEED[name] + 1000).uniform(0, 1, CASES[name][1])


def case_cotangent(name, shape):
    """float64 standard-normal cotangent of the output."""
    return np.random.default_rng(SEED[name] + 2000).standard_normal(tuple(shape))


def run_case(model, name, dtype=torch.float32, device="cpu", train=True):
    """Output and parameter gradients of sum(y * cotangent) with the shared weights: (y, {parameter name: gradient})."""
    model = fill_state(model.to(dtype), SEED[name]).to(device)
    model.train(train)
    model.zero_grad(set_to_none=True)
    x = torch.from_numpy(case_input(name)).to(dtype).to(device)
    y = model(x)
    ct = torch.from_numpy(case_cotangent(name, y.shape)).to(dtype).to(device)
    (y * ct).sum().backward()
    return y.detach(), {k: p.grad.detach() for k, p in model.named_parameters()}


def rel_err(got, want):
    """max |got - want| / max |want| in float64."""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.abs(got - want).max() / np.abs(want).max())
