"""Plain references of the per-channel / pointwise kernels of csrc/elementwise.hip (tests/test_elementwise_ref64.py pins them against
torch autograd, tests/test_gpu_elementwise_ops.py compares the kernels with them).

torch on the CPU, one function per operation, no project imports.  Every function computes in float64 whatever it is given, except
`nchw_to_nhwc` and `stripe_fold`, whose kernels are specified in f32 and are restated in f32.  NHWC tensors are [n, h, w, c] or
[npix, c]; nothing here knows about channel strides or offsets: the tests slice.
"""
from __future__ import annotations

import numpy as np
import torch

F64 = torch.float64


def _d(t):
    return None if t is None else torch.as_tensor(t).to(F64)


def nchw_stats(x, pre_scale=1.0, pre_shift=0.0):
    """Per-channel (sum, sum of squares) of x * pre_scale + pre_shift over n, h, w of an NCHW tensor."""
    v = _d(x) * pre_scale + pre_shift
    return v.sum((0, 2, 3)), (v * v).sum((0, 2, 3))


def bn_finalize(s1, s2, count, gamma=None, beta=None, eps=1e-5, momentum=0.1, running=None):
    """Training-mode BatchNorm bookkeeping from the sums: dict with scale = gamma * invstd, shift = beta - mean * scale, mean, invstd,
    var (biased, clamped at 0) and, with running = (mean, var), the updated running_mean / running_var.  The running variance takes
    the unbiased estimate var * count / (count - 1), the biased one for count == 1.  gamma defaults to 1, beta to 0."""
    s1, s2 = _d(s1), _d(s2)
    mu = s1 / count
    var = torch.clamp(s2 / count - mu * mu, min=0.0)
    invstd = 1.0 / torch.sqrt(var + eps)
    g = torch.ones_like(mu) if gamma is None else _d(gamma)
    b = torch.zeros_like(mu) if beta is None else _d(beta)
    out = {"scale": g * invstd, "shift": b - mu * g * invstd, "mean": mu, "invstd": invstd, "var": var}
    if running is not None:
        unbiased = var * count / (count - 1) if count > 1 else var
        out["running_mean"] = (1.0 - momentum) * _d(running[0]) + momentum * mu
        out["running_var"] = (1.0 - momentum) * _d(running[1]) + momentum * unbiased
    return out


def bn_eval_affine(gamma, beta, running_mean, running_var, eps=1e-5):
    """Eval-mode BatchNorm as (scale, shift)."""
    invstd = 1.0 / torch.sqrt(_d(running_var) + eps)
    scale = _d(gamma) * invstd
    return scale, _d(beta) - _d(running_mean) * scale


def bn_bwd_coefs(s1, s2, count, gamma, mean, invstd):
    """From s1 = sum g, s2 = sum g * xhat: the coefficients of dx = A g + B x + C, and dgamma = s2, dbeta = s1."""
    s1, s2, g, mu, inv = _d(s1), _d(s2), _d(gamma), _d(mean), _d(invstd)
    c1, c2 = s1 / count, s2 / count
    return {"A": g * inv, "B": -g * inv * inv * c2, "C": g * inv * (mu * inv * c2 - c1), "dgamma": s2, "dbeta": s1}


def _normalised(x, pre_scale, pre_shift, scale, shift):
    return (_d(x) * pre_scale + pre_shift) * _d(scale)[None, :, None, None] + _d(shift)[None, :, None, None]


def input_im2col(x, scale, shift, xc, pre_scale=1 / 128, pre_shift=-1.0):
    """xcol[n, y, x, ch * 9 + tap] = bn(x * pre_scale + pre_shift)[n, ch, y + tap // 3 - 1, x + tap % 3 - 1]; taps outside the image
    are zero (not `shift`), channels >= 9 c are zero.  x: NCHW."""
    n, c, h, w = x.shape
    xn = torch.zeros(n, c, h + 2, w + 2, dtype=F64)
    xn[:, :, 1:-1, 1:-1] = _normalised(x, pre_scale, pre_shift, scale, shift)
    out = torch.zeros(n, h, w, xc, dtype=F64)
    for ch in range(c):
        for tap in range(9):
            ky, kx = tap // 3, tap % 3
            out[..., ch * 9 + tap] = xn[:, ch, ky:ky + h, kx:kx + w]
    return out


def input_norm_fold(dxcols, dpatch, pk, n, c, h, w):
    """Gradient wrt the normalised input [n, c, h, w]: the transpose of input_im2col applied to every tensor of `dxcols`
    ([n, h, w, xc] each) plus, with dpatch [n, h / pk, w / pk, pc], the transpose of the patchify stem, where pixel (y, x) of channel ch
    is element ch * pk * pk + (y % pk) * pk + x % pk of patch (y // pk, x // pk)."""
    G = torch.zeros(n, c, h + 2, w + 2, dtype=F64)
    for d in dxcols:
        d = _d(d)
        for ch in range(c):
            for tap in range(9):
                ky, kx = tap // 3, tap % 3
                G[:, ch, ky:ky + h, kx:kx + w] += d[..., ch * 9 + tap]        # xcol[q][tap] = x0[q + (ky - 1, kx - 1)]
    g = G[:, :, 1:-1, 1:-1].clone()
    if dpatch is not None:
        hp, wp = h // pk, w // pk
        dp = _d(dpatch)[..., :c * pk * pk].reshape(n, hp, wp, c, pk, pk)
        g += dp.permute(0, 3, 1, 4, 2, 5).reshape(n, c, h, w)
    return g


def input_norm_bwd(dxcols, dpatch, pk, x, mean, invstd, pre_scale=1 / 128, pre_shift=-1.0):
    """(g, sum g, sum g * xhat) per channel with g = input_norm_fold(...) and xhat = (x * pre_scale + pre_shift - mean) * invstd."""
    n, c, h, w = x.shape
    g = input_norm_fold(dxcols, dpatch, pk, n, c, h, w)
    xhat = (_d(x) * pre_scale + pre_shift - _d(mean)[None, :, None, None]) * _d(invstd)[None, :, None, None]
    return g, g.sum((0, 2, 3)), (g * xhat).sum((0, 2, 3))


def _windows(t, ho, wo):
    """[n, h, w, c] -> the four taps of every 2x2 window in row-major order, each [n, ho, wo, c]."""
    t = t[:, :2 * ho, :2 * wo]
    return [t[:, 0::2, 0::2], t[:, 0::2, 1::2], t[:, 1::2, 0::2], t[:, 1::2, 1::2]]


def maxpool2(x):
    """max_pool2d(kernel 2, stride 2) of NHWC [n, h, w, c] with floor: an odd trailing row / column is dropped."""
    x = _d(x)
    a, b, c, d = _windows(x, x.shape[1] // 2, x.shape[2] // 2)
    return torch.maximum(torch.maximum(a, b), torch.maximum(c, d))


def maxpool2_bwd(act, dpool, dskip=None):
    """dskip (or 0) + the pooled gradient routed to the FIRST maximum of each window in row-major order; odd trailing rows / columns
    receive only dskip."""
    act, dpool = _d(act), _d(dpool)
    n, h, w, c = act.shape
    ho, wo = h // 2, w // 2
    v = _windows(act, ho, wo)
    best, bv = torch.zeros_like(v[0], dtype=torch.int64), v[0]
    for k in range(1, 4):
        upd = v[k] > bv
        best, bv = torch.where(upd, torch.full_like(best, k), best), torch.where(upd, v[k], bv)
    out = torch.zeros(n, h, w, c, dtype=F64) if dskip is None else _d(dskip).clone()
    for k, (dy, dx) in enumerate(((0, 0), (0, 1), (1, 0), (1, 1))):
        out[:, dy:2 * ho:2, dx:2 * wo:2] += torch.where(best == k, dpool, torch.zeros_like(dpool))
    return out


def relu_bwd_stats(dout, out, y, mean, invstd):
    """dz = dout where out > 0 else 0, and per channel (sum dz, sum dz * (y - mean) * invstd).  Tensors [npix, c]."""
    dout = _d(dout)
    dz = torch.where(_d(out) > 0, dout, torch.zeros_like(dout))
    return dz, dz.sum(0), (dz * (_d(y) - _d(mean)) * _d(invstd)).sum(0)


def bn_bwd_apply(g, y, a, b, c):
    """a * g + b * y + c with per-channel a, b, c.  Tensors [npix, c]."""
    return _d(a) * _d(g) + _d(b) * _d(y) + _d(c)


def channel_sum(x):
    """Per-channel sum of [npix, c]."""
    return _d(x).sum(0)


def nchw_to_nhwc(x, cs, scale):
    """f32 NCHW -> NHWC [n, h, w, cs] of x * scale (one f32 product, as the kernel forms it); channels >= c are zero."""
    n, c, h, w = x.shape
    out = torch.zeros(n, h, w, cs, dtype=torch.float32)
    out[..., :c] = (x.float() * torch.tensor(scale, dtype=torch.float32)).permute(0, 2, 3, 1)
    return out


def clip_u8(x):
    """np.clip(x, 0, 255).astype(np.uint8): truncation toward zero."""
    return np.clip(np.asarray(x, dtype=np.float32), 0, 255).astype(np.uint8)


def stripe_fold(src, old=None):
    """float32(sum over the stripes of src [stripes, n] in f64) (+ old, one f32 addition).  Meant for sums that are exact in f64."""
    s = np.asarray(src, dtype=np.float64).sum(0).astype(np.float32)
    return s if old is None else (np.asarray(old, dtype=np.float32) + s).astype(np.float32)
