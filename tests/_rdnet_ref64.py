"""Plain references of the RDNet kernels of csrc/rdnet.hip (tests/test_rdnet_ref64.py pins them against torch autograd,
tests/test_gpu_rdnet_exact.py compares the kernels with them).

torch on the CPU, one function per operation, no project imports.  Every function computes in float64 whatever it is given, except
`dw_pack`, which only moves values and keeps their type.  Images are NCHW [n, c, h, w], the [N, C] side tensors of the ESE gate are
[n, c]; nothing here knows about channel strides or offsets: the tests slice.  Where a result is a sum, the function also returns the
sum of the absolute values of its terms, which the tests' error bounds are relative to.
"""
from __future__ import annotations

import torch

F64 = torch.float64


def _d(t):
    return None if t is None else torch.as_tensor(t).to(F64)


def _ch(v):
    return _d(v)[None, :, None, None]


# ---- stem ----------------------------------------------------------------------------------------------------------------------
def patchify(x, ps, pc, scale, shift, pre_scale=1 / 128, pre_shift=-1.0):
    """[n, h / ps, w / ps, pc]: channel ci * ps * ps + dy * ps + dx holds (x[n, ci, oy * ps + dy, ox * ps + dx] * pre_scale + pre_shift)
    * scale[ci] + shift[ci]; channels from c * ps * ps on are zero."""
    x = _d(x)
    n, c, h, w = x.shape
    v = (x * pre_scale + pre_shift) * _ch(scale) + _ch(shift)
    out = torch.zeros(n, h // ps, w // ps, pc, dtype=F64)
    for ci in range(c):
        for dy in range(ps):
            for dx in range(ps):
                out[..., ci * ps * ps + dy * ps + dx] = v[:, ci, dy::ps, dx::ps]
    return out


# ---- depthwise 7x7 -------------------------------------------------------------------------------------------------------------
def dw_pack(w, flip=False):
    """[C, 1, 7, 7] -> [49, C]: row `tap` holds w[:, tap], or w[:, 48 - tap] (the kernel rotated by 180 degrees) with flip."""
    c = w.shape[0]
    flat = w.reshape(c, 49)
    out = torch.empty(49, c, dtype=w.dtype)
    for tap in range(49):
        out[tap] = flat[:, 48 - tap if flip else tap]
    return out


def _padded(x):
    x = _d(x)
    n, c, h, w = x.shape
    p = torch.zeros(n, c, h + 6, w + 6, dtype=F64)
    p[:, :, 3:3 + h, 3:3 + w] = x
    return p


def dwconv7(x, w, bias=None):
    """out[n, c, y, x] = bias[c] + sum_{ky, kx} x[n, c, y + ky - 3, x + kx - 3] * w[c, 0, ky, kx], zero outside the image, as 49
    shifted adds.  Returns (out, sum of |terms|)."""
    n, c, h, wd = x.shape
    p, w = _padded(x), _d(w)
    out = torch.zeros(n, c, h, wd, dtype=F64)
    mag = torch.zeros(n, c, h, wd, dtype=F64)
    if bias is not None:
        out += _ch(bias)
        mag += _ch(bias).abs()
    for ky in range(7):
        for kx in range(7):
            t = p[:, :, ky:ky + h, kx:kx + wd] * w[None, :, 0, ky, kx, None, None]
            out += t
            mag += t.abs()
    return out, mag


def dwconv7_dgrad(dy, w):
    """dx[n, c, y, x] = sum_{ky, kx} dy[n, c, y - ky + 3, x - kx + 3] * w[c, 0, ky, kx].  Returns (dx, sum of |terms|)."""
    n, c, h, wd = dy.shape
    p, w = _padded(dy), _d(w)
    dx = torch.zeros(n, c, h, wd, dtype=F64)
    mag = torch.zeros(n, c, h, wd, dtype=F64)
    for ky in range(7):
        for kx in range(7):
            t = p[:, :, 6 - ky:6 - ky + h, 6 - kx:6 - kx + wd] * w[None, :, 0, ky, kx, None, None]
            dx += t
            mag += t.abs()
    return dx, mag


def dwconv7_wgrad(dy, x):
    """dw[c, ky * 7 + kx] = sum_{n, y, x} dy[n, c, y, x] * x[n, c, y + ky - 3, x + kx - 3].  Returns (dw [C, 49], sum of |terms|)."""
    n, c, h, wd = x.shape
    p, dy = _padded(x), _d(dy)
    dw = torch.zeros(c, 49, dtype=F64)
    mag = torch.zeros(c, 49, dtype=F64)
    for ky in range(7):
        for kx in range(7):
            t = dy * p[:, :, ky:ky + h, kx:kx + wd]
            dw[:, ky * 7 + kx] = t.sum((0, 2, 3))
            mag[:, ky * 7 + kx] = t.abs().sum((0, 2, 3))
    return dw, mag


# ---- LayerNorm2d ---------------------------------------------------------------------------------------------------------------
def layernorm2d_fwd(x, gamma, beta, eps):
    """Layer norm over the channels of every pixel, biased variance, eps inside the square root.  Returns (out [n, c, h, w],
    mean [n, h, w], rstd [n, h, w])."""
    x = _d(x)
    c = x.shape[1]
    mean = x.sum(1) / c
    var = ((x - mean[:, None]) ** 2).sum(1) / c
    rstd = 1.0 / torch.sqrt(var + eps)
    return (x - mean[:, None]) * rstd[:, None] * _ch(gamma) + _ch(beta), mean, rstd


def layernorm2d_bwd(g, x, gamma, mean, rstd):
    """From the saved mean and rstd [n, h, w]: dx = rstd * (g gamma - mean_c(g gamma) - xhat mean_c(g gamma xhat)), dgamma = sum g xhat,
    dbeta = sum g over n, h, w.  Returns (dx, dgamma, dbeta, sum |g xhat|, sum |g|)."""
    g, x, mean, rstd = _d(g), _d(x), _d(mean), _d(rstd)
    c = x.shape[1]
    xhat = (x - mean[:, None]) * rstd[:, None]
    gg = g * _ch(gamma)
    m1 = gg.sum(1, keepdim=True) / c
    m2 = (gg * xhat).sum(1, keepdim=True) / c
    dx = rstd[:, None] * (gg - m1 - xhat * m2)
    t = g * xhat
    return dx, t.sum((0, 2, 3)), g.sum((0, 2, 3)), t.abs().sum((0, 2, 3)), g.abs().sum((0, 2, 3))


def s2d_fold(v, c_pad, fill=0.0):
    """NCHW [n, c, h, w] -> the 2x2 space-to-depth layout [n, h / 2, w / 2, 4 * c_pad]: pixel (y, x) lies at (y / 2, x / 2), channels
    ((y & 1) * 2 + (x & 1)) * c_pad + [0, c); the channels [c, c_pad) of each of the four groups hold `fill`."""
    n, c, h, w = v.shape
    out = torch.full((n, h // 2, w // 2, 4 * c_pad), fill, dtype=v.dtype)
    for y in range(h):
        for x in range(w):
            base = ((y & 1) * 2 + (x & 1)) * c_pad
            out[:, y // 2, x // 2, base:base + c] = v[:, :, y, x]
    return out


def s2d_unfold(t, c, c_pad):
    """Inverse of s2d_fold: [n, h / 2, w / 2, 4 * c_pad] -> NCHW [n, c, h, w]; the pad channels are dropped."""
    n, h2, w2, _ = t.shape
    out = torch.empty(n, c, 2 * h2, 2 * w2, dtype=t.dtype)
    for y in range(2 * h2):
        for x in range(2 * w2):
            base = ((y & 1) * 2 + (x & 1)) * c_pad
            out[:, :, y, x] = t[:, y // 2, x // 2, base:base + c]
    return out


# ---- Effective-SE gate and layer scale -----------------------------------------------------------------------------------------
def image_channel_dot(a, b=None, scale=1.0):
    """[n, c]: scale * sum over the pixels of an image of a * b (b = None: of a); a, b are [n, hw, c].  Returns (sums, sum of |terms|)."""
    t = _d(a) * (1.0 if b is None else _d(b)) * scale
    return t.sum(1), t.abs().sum(1)


def ese_gate(s, w, b):
    """u[n, co] = b[co] + sum_ci w[co, ci] s[n, ci]; gate = relu6(u + 3) / 6.  Returns (u, gate, sum of |terms| of u)."""
    s, w, b = _d(s), _d(w), _d(b)
    t = s[:, None, :] * w[None]                                        # [n, co, ci]
    u = t.sum(2) + b
    return u, torch.clamp(u + 3.0, 0.0, 6.0) / 6.0, t.abs().sum(2) + b.abs()


def scale_nc(t, gate, gamma, add=None):
    """out[n, p, c] = t[n, p, c] * gate[n, c] * gamma[c] + add[n, c]; gate = None: 1, add = None: 0; t is [n, hw, c]."""
    out = _d(t) * _d(gamma)
    if gate is not None:
        out = out * _d(gate)[:, None, :]
    if add is not None:
        out = out + _d(add)[:, None, :]
    return out


def ese_bwd(A, gamma, hw, gate=None, u=None, s=None, w=None):
    """Backward of out = t * gate * gamma on the [N, C] side tensors, A[n, c] = sum over pixels of dout * t.
    Without the gate: dict(dgamma = sum_n A).  With it: du = (|u| < 3) A gamma / 6, dgamma = sum_n A gate, db_fc = sum_n du,
    dW_fc[co, ci] = sum_n du[n, co] s[n, ci], add[n, ci] = (1 / hw) sum_co w[co, ci] du[n, co].  Every sum `k` comes with its sum of
    |terms| as `k_abs`."""
    A, gamma = _d(A), _d(gamma)
    if gate is None:
        return {"dgamma": A.sum(0), "dgamma_abs": A.abs().sum(0)}
    gate, u, s, w = _d(gate), _d(u), _d(s), _d(w)
    du = torch.where(u.abs() < 3.0, A * gamma / 6.0, torch.zeros_like(A))
    tg = A * gate
    tw = du[:, :, None] * s[:, None, :]                                # [n, co, ci]
    ta = w[None] * du[:, :, None] / hw                                 # [n, co, ci]
    return {"du": du, "dgamma": tg.sum(0), "dgamma_abs": tg.abs().sum(0), "db_fc": du.sum(0), "db_fc_abs": du.abs().sum(0),
            "dW_fc": tw.sum(0), "dW_fc_abs": tw.abs().sum(0), "add": ta.sum(1), "add_abs": ta.abs().sum(1)}
