"""Plain restatement of the Philox-driven noise kernels of csrc/crappify.hip (tests/test_noise_ref.py pins it against published
known answers and numpy's own generators, tests/test_gpu_noise_streams.py compares the kernels with it value for value).

numpy only, no torch, no project imports.  The device streams are counter based -- every output is a pure function of
(seed, tile, pixel) -- and the arithmetic is float64 ending in a float32, so the comparison is for equality.  Two things can differ
between a host and a device evaluation of the same formula: the last bit of log / cos / exp / lgamma, and whether `a * b + c` was
contracted into one fused operation.  Both move a float64 by a relative ~1e-16, which matters only where the value then falls on the
other side of a decision.  So

  * every function that ends in a float32 cast or a rint also returns `fragile`: the elements whose float64 value lies next to,
    but not exactly on, a half-integer (when rounding) or a clip bound, within a relative 1e-9, or a float32 rounding midpoint,
    within a relative 1e-13 (FRAGILE_MID_REL says why that window is narrower).  A value that lies EXACTLY on one (x = 10,
    mix = 0.5: 5 + y / 2 + 4) came out of exact arithmetic on small dyadic numbers, which no contraction changes, and is kept: it
    is what checks round-half-to-even on the device;
  * `poisson` and `saltpepper` also return the smallest relative margin by which any comparison that steers them was decided.

Shapes: x is float32 [tiles, ...]; a tile's pixels are numbered in memory order.  Tile indices and seeds are uint64 and wrap.
"""
from __future__ import annotations

import numpy as np

U64 = np.uint64
M32 = U64(0xFFFFFFFF)
CLIP, ROUND_CLIP = 1, 2          # flags: bit 0 clips to [0, 255], bit 1 rounds half to even and clips
TILE_COUNTER, TILE_SUB = (1 << 64) - 1, 7      # the counter / sub of the per-tile scalar draw
FRAGILE_REL = 1e-9               # window around a half-integer (rint) or a clip bound, relative to the value
# Window around a float32 rounding midpoint, relative to the magnitude of the terms of the sum.  float32 values lie a relative
# 2^-23 .. 2^-24 apart, so a window of 1e-9 would take in 2e-9 / 2^-23 = 1.7 .. 3.4 % of ALL values; the host and the device differ by a
# few units of 2^-53 = 1.1e-16 in log, cos and a fused multiply-add, and 1e-13 is a hundred times that while taking in 3e-6.
FRAGILE_MID_REL = 1e-13
U01_MAX = 1.0 - 2.0 ** -53       # the largest double below 1


def _u64(v):
    """Python ints / arrays -> uint64 array, modulo 2^64."""
    if isinstance(v, (int, np.integer)):
        return np.array(int(v) % (1 << 64), dtype=U64)
    return np.asarray(v).astype(U64)


# ---- Philox4x32-10 -------------------------------------------------------------------------------------------------------------
def philox4x32_10(c0, c1, c2, c3, k0, k1):
    """Ten rounds of Philox4x32 on uint64 arrays that hold 32-bit words; the key is bumped after each round."""
    c0, c1, c2, c3, k0, k1 = np.broadcast_arrays(*(_u64(v) & M32 for v in (c0, c1, c2, c3, k0, k1)))
    for _ in range(10):
        p0, p1 = U64(0xD2511F53) * c0, U64(0xCD9E8D57) * c2          # 32 x 32 -> 64 bits: no wrap
        c0, c1, c2, c3 = (p1 >> U64(32)) ^ c1 ^ k0, p1 & M32, (p0 >> U64(32)) ^ c3 ^ k1, p0 & M32
        k0, k1 = (k0 + U64(0x9E3779B9)) & M32, (k1 + U64(0xBB67AE85)) & M32
    return c0, c1, c2, c3


def stream_key(seed, tile):
    """(low, high) words of seed ^ (tile * 0x9E3779B97F4A7C15 + 0xD1B54A32D192ED03) mod 2^64: the tile is folded into the key."""
    with np.errstate(over="ignore"):
        k = _u64(seed) ^ (_u64(tile) * U64(0x9E3779B97F4A7C15) + U64(0xD1B54A32D192ED03))
    return k & M32, k >> U64(32)


def draw(seed, tile, counter, sub):
    """Four 32-bit words of the stream of (seed, tile) at `counter` (64 bits: c0 low, c1 high), `sub` in c2, 0x1BD11BDA in c3."""
    k0, k1 = stream_key(seed, tile)
    counter = _u64(counter)
    return philox4x32_10(counter & M32, counter >> U64(32), sub, 0x1BD11BDA, k0, k1)


def u01(hi, lo):
    """53 bits of (hi, lo) as a double strictly inside (0, 1).  v + 0.5 is a tie for v >= 2^52 and rounds to even, which at the very
    last v (all bits set) is 2^53: that one value is held below 1."""
    v = ((_u64(hi) << U64(32)) | _u64(lo)) >> U64(11)
    return np.minimum((v.astype(np.float64) + 0.5) * 2.0 ** -53, U01_MAX)


def normal(r):
    """Box-Muller normal from the four words of one draw."""
    u1, u2 = u01(r[0], r[1]), u01(r[2], r[3])
    return np.sqrt(-2.0 * np.log(u1)) * np.cos(6.283185307179586 * u2)


def tile_intensity(seed, tile, intensity, spread):
    """float64 per tile: `intensity` (as the float32 the C ABI receives) if spread <= 0, else max(intensity + spread * N, 0) with N
    the normal of the tile's scalar draw."""
    intensity, spread = float(np.float32(intensity)), float(np.float32(spread))
    tile = _u64(tile)
    if not spread > 0:
        return np.full(tile.shape, intensity)
    return np.maximum(intensity + spread * normal(draw(seed, tile, TILE_COUNTER, TILE_SUB)), 0.0)


# ---- the end of every kernel: round, clip, float32 ---------------------------------------------------------------------------------
def finish(v, flags):
    """rint (half to even) for flag 2, clip to [0, 255] for flags 1 or 2; float64 in and out."""
    v = np.asarray(v, dtype=np.float64)
    if flags & 2:
        v = np.rint(v)
    if flags & 3:
        v = np.clip(v, 0.0, 255.0)
    return v


def _near(v, target, scale, rel=FRAGILE_REL):
    d = np.abs(v - target)
    return (d > 0) & (d <= rel * scale)


def to_f32(v, flags, scale=None):
    """(float32(finish(v, flags)), fragile) of float64 v; `scale` is the sum of the magnitudes of the terms v was added up from
    (|v| if not given): what the float32 midpoint window is relative to."""
    v = np.asarray(v, dtype=np.float64)
    scale = np.abs(v) if scale is None else scale
    fragile = np.zeros(v.shape, dtype=bool)
    if flags & 2:
        fragile |= _near(v, np.floor(v) + 0.5, np.maximum(np.abs(v), 1.0))
        v = np.rint(v)
    if flags & 3:
        fragile |= _near(v, 0.0, 1.0) | _near(v, 255.0, 255.0)
        v = np.clip(v, 0.0, 255.0)
    out = v.astype(np.float32)
    f = out.astype(np.float64)
    other = np.nextafter(out, np.where(v >= f, np.float32(np.inf), np.float32(-np.inf)).astype(np.float32)).astype(np.float64)
    # an integer or a clip bound is a float32 already: only a value that the cast itself rounds can sit next to a midpoint
    fragile |= _near(v, 0.5 * (f + other), scale, FRAGILE_MID_REL) & (v != f)
    return out, fragile


def _tiles_pixels(x, tile_offset):
    """x as float64 [tiles, per_tile], the wrapped tile indices [tiles, 1] and the pixel counters [1, per_tile]."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim >= 2
    tiles = x.shape[0]
    x64 = x.reshape(tiles, -1).astype(np.float64)
    with np.errstate(over="ignore"):
        tile = _u64(tile_offset) + np.arange(tiles, dtype=U64)
    return x64, tile[:, None], np.arange(x64.shape[1], dtype=U64)[None, :]


# ---- additive Gaussian ---------------------------------------------------------------------------------------------------------
def gaussian(x, intensity, gain, spread, seed, tile_offset, flags):
    """x + gain + intensity_t * N(pixel): (float32 like x, fragile)."""
    x64, tile, pix = _tiles_pixels(x, tile_offset)
    ti = tile_intensity(seed, tile, intensity, spread)
    nz = float(np.float32(gain)) + ti * normal(draw(seed, tile, pix, 0))
    out, fragile = to_f32(x64 + nz, flags, np.abs(x64) + np.abs(nz) + abs(float(np.float32(gain))))
    return out.reshape(np.shape(x)), fragile.reshape(np.shape(x))


# ---- Poisson -------------------------------------------------------------------------------------------------------------------
def _gap(a, b, scale):
    """Smallest |a - b| / scale over the elements (inf when there are none)."""
    with np.errstate(invalid="ignore", divide="ignore"):
        g = np.abs(a - b) / scale
    g = g[np.isfinite(g)]
    return float(g.min()) if g.size else np.inf


def poisson_draw(seed, tile, pix, lam):
    """Poisson(lam) per element from the stream of (seed, tile) at counter pix, subs 1, 2, ...: the Knuth product below 10 (two
    uniforms per round, at most 64 rounds), Hoermann's PTRS transformed rejection from 10 on (one round per sub, floor(lam + 0.5) after
    256 rejections); 0 for lam <= 0.  tile, pix and lam broadcast.  Returns (float64 draws, smallest relative margin): the margin is
    taken over `prod > e^-lam`, the floor argument against the nearest integer, `V <= vr` and the final log comparison."""
    from scipy.special import gammaln
    tile, pix, lam = np.broadcast_arrays(_u64(tile), _u64(pix), np.asarray(lam, dtype=np.float64))
    shape = lam.shape
    tile, pix, lam = tile.ravel(), pix.ravel(), lam.ravel()
    out = np.zeros(lam.shape)
    margin = np.inf

    idx = np.flatnonzero((lam > 0) & (lam < 10.0))
    enlam = np.exp(-lam[idx])
    prod, count = np.ones(idx.size), np.zeros(idx.size)
    for it in range(64):
        if not idx.size:
            break
        r = draw(seed, tile[idx], pix[idx], it + 1)
        u, u_second = u01(r[0], r[1]), u01(r[2], r[3])
        for j in range(2):
            prod = prod * u
            margin = min(margin, _gap(prod, enlam, enlam))
            go = prod > enlam
            out[idx[~go]] = count[~go]
            idx, enlam, prod, count = idx[go], enlam[go], prod[go], count[go] + 1.0
            if j == 0:
                u = u_second[go]          # the second uniform goes to those that are still multiplying
    out[idx] = count                      # 64 rounds without a stop: the count so far

    idx = np.flatnonzero(lam >= 10.0)
    for it in range(256):
        if not idx.size:
            break
        l = lam[idx]
        slam, loglam = np.sqrt(l), np.log(l)
        b = 0.931 + 2.53 * slam
        a = -0.059 + 0.02483 * b
        invalpha = 1.1239 + 1.1328 / (b - 3.4)
        vr = 0.9277 - 3.6224 / (b - 2.0)
        r = draw(seed, tile[idx], pix[idx], it + 1)
        U, V = u01(r[0], r[1]) - 0.5, u01(r[2], r[3])
        us = 0.5 - np.abs(U)
        arg = (2.0 * a / us + b) * U + l + 0.43
        k = np.floor(arg)
        wide = us >= 0.07
        margin = min(margin, _gap(V[wide], vr[wide], vr[wide]))
        take = wide & (V <= vr)
        tail = ~take & (us < 0.013) & (V > us)          # rejected whatever k is (both sides are exact): k steers nothing there
        margin = min(margin, _gap(arg[~tail], np.rint(arg[~tail]), np.maximum(np.abs(arg[~tail]), 1.0)))
        skip = tail | (~take & (k < 0.0))
        test = ~take & ~skip
        with np.errstate(invalid="ignore"):
            t_lv, t_la, t_lb = np.log(V), np.log(invalpha), np.log(a / (us * us) + b)
            t_kl, t_lg = k * loglam, gammaln(k + 1.0)
            lhs, rhs = t_lv + t_la - t_lb, -l + t_kl - t_lg
            scale = np.abs(t_lv) + np.abs(t_la) + np.abs(t_lb) + l + np.abs(t_kl) + np.abs(t_lg)
            margin = min(margin, _gap(lhs[test], rhs[test], scale[test]))
            take |= test & (lhs <= rhs)
        out[idx[take]] = k[take]
        idx = idx[~take]
    out[idx] = np.floor(lam[idx] + 0.5)
    return out.reshape(shape), margin


def poisson(x, intensity, gain, spread, seed, tile_offset, flags):
    """x * (1 - mix_t) + Poisson(max(x, 0)) * mix_t + gain: (float32 like x, fragile, margin of the draws)."""
    x64, tile, pix = _tiles_pixels(x, tile_offset)
    y, margin = poisson_draw(seed, tile, pix, np.maximum(x64, 0.0))
    mix = tile_intensity(seed, tile, intensity, spread)
    gain = float(np.float32(gain))
    out, fragile = to_f32(x64 * (1.0 - mix) + y * mix + gain, flags, np.abs(x64) + np.abs(y * mix) + abs(gain))
    return out.reshape(np.shape(x)), fragile.reshape(np.shape(x)), margin


# ---- salt and pepper -----------------------------------------------------------------------------------------------------------
def saltpepper(x, amount, gain, spread, seed, tile_offset, flags):
    """clip(x + gain, 0, 255), then with probability amount_t a pixel becomes 255 or 0, each with probability 1/2; both uniforms come
    from the pixel's draw at sub 0.  Returns (float32 like x, fragile, relative margin of `u <= amount_t`)."""
    x64, tile, pix = _tiles_pixels(x, tile_offset)
    a = np.broadcast_to(tile_intensity(seed, tile, amount, spread), x64.shape)
    r = draw(seed, tile, pix, 0)
    u, side = u01(r[0], r[1]), u01(r[2], r[3])
    v = np.clip(x64 + float(np.float32(gain)), 0.0, 255.0)
    v = np.where(u <= a, np.where(side <= 0.5, 255.0, 0.0), v)
    out, fragile = to_f32(v, flags)
    return out.reshape(np.shape(x)), fragile.reshape(np.shape(x)), _gap(u, a, a)


# ---- blur with a per-tile sigma ------------------------------------------------------------------------------------------------
def blur_sigma(seed, tiles, tile_offset, sigma, spread):
    """float64 [tiles]: the sigma each tile is blurred with, max(N(sigma, spread), 0) from the tile's scalar draw."""
    with np.errstate(over="ignore"):
        tile = _u64(tile_offset) + np.arange(tiles, dtype=U64)
    return tile_intensity(seed, tile, sigma, spread)


def _blur_pass(img, sigma, radius, axis):
    """One pass of the separable Gaussian over float32 [planes, h, w]: unnormalised weights exp(-t^2 / (2 sigma^2)) for |t| <= radius,
    edge replication, float64 sums divided by the sum of the weights, float32 result."""
    n = img.shape[axis]
    t = np.arange(-radius, radius + 1, dtype=np.float64)
    w = np.exp(-0.5 / (sigma * sigma) * t * t)
    padded = np.take(img, np.clip(np.arange(-radius, n + radius), 0, n - 1), axis=axis).astype(np.float64)
    acc = np.zeros(img.shape, dtype=np.float64)
    for k in range(2 * radius + 1):
        sl = [slice(None)] * 3
        sl[axis] = slice(k, k + n)
        acc += w[k] * padded[tuple(sl)]
    return (acc / w.sum()).astype(np.float32)


def blur_tiles(x, sigmas, gain, flags):
    """x float32 [tiles, planes, h, w], one float64 sigma per tile: rows then columns, radius int(4 * float32(sigma) + 0.5), float32
    between the passes, then + gain and the finish; a tile whose sigma is not positive only gets the gain.  (float32, fragile)."""
    x = np.asarray(x)
    assert x.dtype == np.float32 and x.ndim == 4
    v = np.empty(x.shape, dtype=np.float64)
    for t, sigma in enumerate(np.asarray(sigmas, dtype=np.float64)):
        img = x[t]
        if sigma > 0.0:
            radius = int(4.0 * float(np.float32(sigma)) + 0.5)
            img = _blur_pass(_blur_pass(img, sigma, radius, 1), sigma, radius, 2)
        v[t] = img.astype(np.float64) + float(np.float32(gain))
    return to_f32(v, flags)
