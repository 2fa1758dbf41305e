"""Reference of the GradHist kernels of csrc/hist.hip and the error measure their tests use (tests/test_hist_ref64.py,
tests/test_gpu_hist_ops.py).

Plain torch, on whichever device the inputs live, chunked over pixels.  `hist_fwd` and `hist_bwd` take a `dtype`, so the same code is
the f64 reference and the f32 yardstick.  The centres are always the reference's fp32 tensor float(lo) + delta * (arange(bins).float()
+ 0.5), widened afterwards.  `hist_bwd` takes what the C ABI of pssr_gradhist_bwd takes:
    x     = clamp?(xa) - xb
    g_eff = (g - g_ref) * g_scale * dev_scale,     G_k = g_eff[k+1] [k+1 < bins] - g_eff[k]
    dx    = sigma * sum_k s_k (1 - s_k) G_k  (+ dx_in when accumulating),  0 where the clamp cut (xa outside [0, 255], bounds inclusive)
Non-finite values follow torch: a NaN pixel gives a NaN histogram row and a NaN dx (0 under a clamp that cut it: torch.clamp's
gradient mask is false for NaN); +-inf pixels count as sigmoid says, so a -inf pixel adds s_{-1} - s_0 = 1 to bin 0.

The reference knows nothing about the kernels' skip windows.  `drop_below` exists for the sensitivity tests only: it drops the terms
with sigma (x - c) < -drop_below, which is what a window that is too tight does.

Error measures (every bin and every pixel enters; a reference entry that is not finite must be matched exactly in kind):
    q_h  = max_{b,j} |h - h64| / (2^-24 S[b,j] + 1e-13 N),        S[b,j] = sum_i (s_{j-1}(x_i) + s_j(x_i)) in f64, s_{-1} = 1
           2^-24 S is one rounding unit of the operands each term subtracts; 1e-13 N is the skip loss the header of hist.hip documents
           (e^-30 ~ 9.4e-14 per pixel), rounded up.
    q_dx = max_{b,i} |dx - dx64| / (2^-24 (W[b,i] + |dx64|) + T), W[b,i] = sigma sum_k s_k (1 - s_k) |G_k| (1 + |z_ik|),  z_ik = sigma (x_i - c_k)
           with G the scaled combined gradient above (|g_scale * dev_scale| is inside it), T = sigma max|G| e^-30 / (1 - e^-(sigma delta))
           the header's bound of the dropped sum.
"""
from __future__ import annotations

import math

import numpy as np
import torch

EPS24 = 2.0 ** -24
SKIP_PER_PIXEL = 1e-13
HI_Z, LO_Z = 19.0, 31.0             # the kernels' windows, used only to PLACE pixels (plant_edges)
CHUNK_ELEMS = 1 << 22               # batch * bins * pixels of one chunk


def centres(bins, lo, hi, device="cpu", dtype=torch.float64):
    delta = float(hi - lo) / float(bins)
    return (float(lo) + delta * (torch.arange(bins).float() + 0.5)).to(device=device, dtype=dtype)


def _chunks(batch, bins, n):
    step = max(1, CHUNK_ELEMS // max(1, batch * bins))
    return [(i, min(i + step, n)) for i in range(0, n, step)]


def hist_fwd(x, bins, lo, hi, sigma, dtype=torch.float64, with_s=False, drop_below=None):
    """h [B, bins] of x [B, ...]; with_s: also S [B, bins] (see the module docstring)."""
    B = x.shape[0]
    xf = x.reshape(B, -1).to(dtype)
    c = centres(bins, lo, hi, x.device, dtype)
    h = torch.zeros(B, bins, dtype=dtype, device=x.device)
    S = torch.zeros(B, bins, dtype=dtype, device=x.device)
    for i0, i1 in _chunks(B, bins, xf.shape[1]):
        z = (xf[:, None, i0:i1] - c[:, None]) * sigma                                  # [B, bins, n]
        s = torch.sigmoid(z)
        ones = torch.ones(B, 1, s.shape[-1], dtype=dtype, device=x.device)
        sm = torch.cat([ones, s[:, :-1]], 1)
        term = sm - s
        if drop_below is not None:
            zm = torch.cat([torch.zeros_like(z[:, :1]), z[:, :-1]], 1)                 # bin 0 has no lower sigmoid: never dropped
            term = torch.where(zm < -drop_below, torch.zeros_like(term), term)
        h = h + term.sum(-1)
        if with_s:
            S = S + (sm + s).detach().sum(-1)
    return (h, S) if with_s else h


def _g_eff(g, g_ref, dev_scale, g_scale, dtype):
    ge = g.to(dtype)
    if g_ref is not None:
        ge = ge - g_ref.to(dtype)
    ge = ge * g_scale
    if dev_scale is not None:
        ge = ge * dev_scale.to(dtype).reshape(())
    return ge


def hist_bwd(xa, g, bins, lo, hi, sigma, xb=None, g_ref=None, dev_scale=None, g_scale=1.0, clamp=False, dx_in=None,
             dtype=torch.float64, with_w=False, drop_below=None):
    """dx (shape of xa) as pssr_gradhist_bwd defines it; with_w: also (W, T), W of dx's shape and T a float."""
    B = xa.shape[0]
    a = xa.reshape(B, -1).to(dtype)
    xf = a.clamp(0, 255) if clamp else a
    if xb is not None:
        xf = xf - xb.reshape(B, -1).to(dtype)
    c = centres(bins, lo, hi, xa.device, dtype)
    ge = _g_eff(g, g_ref, dev_scale, g_scale, dtype)
    G = torch.cat([ge[:, 1:], torch.zeros(B, 1, dtype=dtype, device=xa.device)], 1) - ge
    dx = torch.zeros_like(xf)
    W = torch.zeros_like(xf)
    for i0, i1 in _chunks(B, bins, xf.shape[1]):
        z = (xf[:, None, i0:i1] - c[:, None]) * sigma
        s = torch.sigmoid(z)
        t = s * (1 - s) * G[:, :, None]
        if drop_below is not None:
            t = torch.where(z < -drop_below, torch.zeros_like(t), t)
        dx[:, i0:i1] = sigma * t.sum(1)
        if with_w:
            W[:, i0:i1] = sigma * (s * (1 - s) * G.abs()[:, :, None] * (1 + z.abs())).sum(1)
    if dx_in is not None:
        dx = dx + dx_in.reshape(B, -1).to(dtype)
    if clamp:
        dx = torch.where((a >= 0) & (a <= 255), dx, torch.zeros_like(dx))
    dx = dx.reshape(xa.shape)
    if not with_w:
        return dx
    delta = float(hi - lo) / float(bins)
    T = float(sigma) * G.abs().max().item() * math.exp(-30.0) / (1.0 - math.exp(-float(sigma) * delta))
    return dx, W.reshape(xa.shape), T


def _q(got, ref64, tol):
    """max |got - ref64| / tol over the finite reference entries; inf if a non-finite reference entry is not matched in kind (NaN for
    NaN, the same infinity for an infinity) or a finite one is answered by a non-finite value."""
    got, ref64, tol = (t.detach().double().cpu() for t in (got, ref64, tol))
    got = got.reshape(ref64.shape)
    fin = torch.isfinite(ref64)
    if not torch.equal(torch.isnan(got), torch.isnan(ref64)):
        return float("inf")
    if not torch.equal(got[~fin & ~torch.isnan(ref64)], ref64[~fin & ~torch.isnan(ref64)]):
        return float("inf")
    if not fin.any():
        return 0.0
    if not torch.isfinite(got[fin]).all():
        return float("inf")
    return ((got[fin] - ref64[fin]).abs() / tol[fin]).max().item()


def q_h(h, h64, S, n):
    return _q(h, h64, EPS24 * S.double() + SKIP_PER_PIXEL * n)


def worst_bin(h, h64, S, n):
    """(b, j) of the finite entry that sets q_h, for messages."""
    tol = (EPS24 * S.double() + SKIP_PER_PIXEL * n).cpu()
    e = (h.detach().double().cpu() - h64.double().cpu()).abs() / tol
    e = torch.where(torch.isfinite(e), e, torch.zeros_like(e))
    return divmod(int(e.argmax()), h64.shape[1])


def q_dx(dx, dx64, W, T):
    tol = EPS24 * (W.double() + dx64.double().abs()) + T
    tol = torch.where(torch.isfinite(tol), tol, torch.ones_like(tol))          # non-finite entries are compared in kind, not by q
    return _q(dx, dx64, tol)


def old_metric(h, h64):
    """tests/test_gpu_crappifier.py's measure: each image's worst bin error over that image's largest bin."""
    return ((h.double() - h64.double()).abs().amax(1) / h64.double().abs().amax(1)).max().item()


# ---------------------------------------------------------------------------------------------- inputs
def inputs(shape, std, seed):
    """Profile-like values (tests/test_gpu_crappifier.py's _inputs, on the CPU): normal, every 97th value on an integer (a bin edge of
    the default configuration), six values far outside the range or at 0 / 0.5."""
    gen = torch.Generator().manual_seed(seed)
    x = torch.randn(shape, generator=gen) * std
    x.view(-1)[::97] = torch.round(x.view(-1)[::97])
    far = torch.tensor([3.0 * std * 40, -3.0 * std * 40, 1e4, -1e4, 0.0, 0.5])
    m = min(6, x.numel())
    x.view(-1)[:m] = far[:m]
    return x


def wave_bounds(bins):
    """(j0, j1) of a few of the forward's 64-bin waves: the first two, one in the middle, the last two (ragged when bins % 64)."""
    waves = [(j0, min(j0 + 64, bins)) for j0 in range(0, bins, 64)]
    pick = sorted({0, 1, len(waves) // 2, len(waves) - 2, len(waves) - 1} & set(range(len(waves))))
    return [waves[i] for i in pick]


def edge_values(bins, lo, hi, sigma, above_range=True):
    """Pixel values on the kernels' window ends, computed in f32 the way the kernels compute them (centre: an f32 multiply then an f32
    add; offset: an f32 divide): for k = j1 - 1 and k = j0 - 1 of wave_bounds, c_k + 19 / sigma and c_k - 31 / sigma with the f32
    neighbour on either side.  These are also where the backward's k range gains or loses bin k.  Then values below the whole range,
    c_0 - z / sigma for z = 13, 16, 20, 25, 29: every bin of such a pixel is in the tail.

    above_range=False leaves out the planted values above the last centre (c_{bins-1} + 19 / sigma and its neighbours, and for few
    bins those of lower k).  There z = sigma (x - c_k) is large for EVERY k, and any f32 evaluation of s_k (1 - s_k) carries the
    2^-24 absolute error of 1 - s_k into a value of size e^-z (at z >= 19: 0 or 2^-24 for a true 5.6e-9).  One such pixel puts the f32
    yardstick's q_dx near 2e4 (it is 2 .. 40 without), and the bound derived from it would say little about the other pixels.  The
    backward is therefore measured on both sets.  The forward is not affected: its terms there are exactly 0 in f32 and below 1e-13
    in f64."""
    f = np.float32
    delta = f((float(hi) - float(lo)) / float(bins))
    ks = sorted({k for j0, j1 in wave_bounds(bins) for k in (j0 - 1, j1 - 1) if k >= 0})
    out = []
    c_last = f(lo) + delta * (f(bins - 1) + f(0.5))
    for k in ks:
        ck = f(lo) + delta * (f(k) + f(0.5))
        for e in (ck + f(HI_Z) / f(sigma), ck - f(LO_Z) / f(sigma)):
            if e > c_last and not above_range:
                continue
            out += [e, np.nextafter(e, f(np.inf)), np.nextafter(e, f(-np.inf))]
    c0 = f(lo) + delta * f(0.5)
    out += [c0 - f(z) / f(sigma) for z in (13, 16, 20, 25, 29)]
    return torch.tensor(np.asarray(out, dtype=np.float32))


def plant_edges(x, bins, lo, hi, sigma, start=6, above_range=True):
    """Write edge_values into x (in place) from flat index `start` on, spread over the images where the first one has no room; as many
    as fit."""
    e = edge_values(bins, lo, hi, sigma, above_range)
    B = x.shape[0]
    xf = x.view(B, -1)
    n = xf.shape[1]
    per = max(1, min(n - start, -(-e.numel() // B)))
    for b in range(B):
        part = e[b * per:(b + 1) * per]
        if part.numel() and n > start:
            xf[b, start:start + part.numel()] = part[:n - start]
    return x


DEF, WIDE = (512, (-256.0, 256.0), 5.0), (64, (-32.0, 32.0), 0.5)
RAGGED = (300, (-100.0, 200.0), 2.0)                    # a ragged last wave (300 = 4 * 64 + 44) and a ragged second chunk
MAX_BINS = 8192                                         # PSSR_HIST_MAX_BINS
# (name, (bins, (lo, hi), sigma), shape): every configuration at least once, every shape at least once
CASES = [
    ("def-1320", DEF, (3, 1, 40, 33)),                  # N = 1320, not a multiple of the 256-pixel tile
    ("def-67tiles", DEF, (2, 1, 129, 131)),             # 67 tiles > HIST_MAX_WG = 64: workgroups 0 .. 2 take two tiles
    ("def-3ch", DEF, (2, 3, 17, 19)),
    ("wide-63", WIDE, (2, 1, 9, 7)),                    # N = 63 < 256
    ("wide-3ch", WIDE, (2, 3, 17, 19)),
    ("ragged-300", RAGGED, (3, 1, 40, 33)),
    ("bins-65", (65, (-65.0, 65.0), 3.0), (2, 1, 9, 7)),                # one bin into a second wave
    ("bins-257", (257, (-128.5, 128.5), 4.0), (3, 1, 40, 33)),          # one bin into a second chunk
    ("bins-1", (1, (-8.0, 8.0), 1.5), (2, 1, 9, 7)),
    ("bins-1000", (1000, (-256.0, 256.0), 5.0), (3, 1, 40, 33)),        # four chunks, the last ragged
    ("bins-max", (MAX_BINS, (-256.0, 256.0), 20.0), (1, 1, 15, 20)),    # N = 300
]
CASE_IDS = [c[0] for c in CASES]


def case_inputs(shape, cfg, seed, std=None, above_range=True):
    """inputs() scaled to the configuration's range plus plant_edges."""
    bins, (lo, hi), sigma = cfg
    std = (hi - lo) / 20.0 if std is None else std
    x = inputs(shape, std, seed) + (lo + hi) / 2.0
    return plant_edges(x, bins, lo, hi, sigma, above_range=above_range)
