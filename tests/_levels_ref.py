"""The definitions of the noise measurement (include/pssr_mi355.h: "The noise model of a pair, measured") restated from the text and not
from the product code: the level table by numpy.add.at in int64, the fit in fractions.Fraction up to the two square roots, the whole of
util.estimate_noise through tests/_rsf_ref.py and tests/_consistency_ref.py for D and Lc, and the scenes and plantings of the tests."""
import math
from fractions import Fraction

import numpy as np

import _consistency_ref as C
import _rsf_ref as F

FIELDS = ("poisson", "gaussian", "gain", "saltpepper", "slope", "intercept", "alpha", "beta", "levels", "found", "table", "sigma", "margin")
# (i, g, s, amount) of the recovery tests: additive only, shot noise only, both with a gain, with salt and pepper, noiseless
PLANTINGS = ((0, 0, 5, 0), (1, 0, 0, 0), (0.5, 3, 4, 0), (1, -2, 6, 0.01), (0.7, 0, 2, 0.02), (0, 0, 0, 0))


def table_ref(d, l):
    """int64 [planes, 256, 5] of uint8 d, l [planes, ...]: per level of d the count, sum l, sum l^2, #{l = 0}, #{l = 255}."""
    d, l = np.asarray(d), np.asarray(l)
    assert d.dtype == np.uint8 and l.dtype == np.uint8 and d.shape == l.shape
    planes = d.shape[0]
    out = np.zeros((planes, 256, 5), dtype=np.int64)
    v = d.reshape(planes, -1).astype(np.int64)
    x = l.reshape(planes, -1).astype(np.int64)
    p = np.broadcast_to(np.arange(planes)[:, None], v.shape)
    for col, what in enumerate((np.ones_like(x), x, x * x, (x == 0).astype(np.int64), (x == 255).astype(np.int64))):
        np.add.at(out[..., col], (p, v), what)
    return out


def fit_ref(table, min_count=32, guard=4.0):
    """The ten fitted fields of one [256][5] table, in exact rationals up to the two square roots (and the float conversions)."""
    rows = [[int(x) for x in r] for r in np.asarray(table).tolist()]
    guard = Fraction(guard)
    n_bright, n_dark = sum(r[0] for r in rows[128:]), sum(r[0] for r in rows[:128])
    pepper = Fraction(sum(r[3] for r in rows[128:]), n_bright) if n_bright else Fraction(0)
    salt = Fraction(sum(r[4] for r in rows[:128]), n_dark) if n_dark else Fraction(0)
    if n_bright and n_dark:
        amount = pepper + salt
    else:
        amount = 2 * (pepper if n_bright else salt)
    used = []
    for v, (n, s1, s2, n0, n255) in enumerate(rows):
        k = n - n0 - n255
        s1, s2 = s1 - 255 * n255, s2 - 255 * 255 * n255
        if k < min_count or k < 2:
            continue
        mean = Fraction(s1, k)
        var = (Fraction(s2) - Fraction(s1 * s1, k)) / (k - 1)
        # mean - guard sd > 0 and mean + guard sd < 255, with sd = sqrt(var), without the root
        reach2 = guard * guard * var
        if mean > 0 and mean * mean > reach2 and mean < 255 and (255 - mean) ** 2 > reach2:
            used.append((v, k, mean, var))
    if not used:
        return dict(poisson=0.0, gaussian=0.0, gain=0.0, saltpepper=float(100 * amount), slope=0.0, intercept=0.0, alpha=0.0, beta=0.0, levels=0,
                    found=False)
    total = sum(k for _, k, _, _ in used)
    vbar = Fraction(sum(k * v for v, k, _, _ in used), total)
    mbar = sum(k * mean for _, k, mean, _ in used) / total
    qbar = sum(k * var for _, k, _, var in used) / total
    gain = sum(k * (mean - v) for v, k, mean, _ in used) / total
    if len(used) < 2:
        slope, intercept, alpha, beta = Fraction(0), qbar, Fraction(1), gain
    else:
        svv = sum(k * (v - vbar) ** 2 for v, k, _, _ in used)
        slope = sum(k * (v - vbar) * (var - qbar) for v, k, _, var in used) / svv
        alpha = sum(k * (v - vbar) * (mean - mbar) for v, k, mean, _ in used) / svv
        intercept, beta = qbar - slope * vbar, mbar - alpha * vbar
    return dict(poisson=math.sqrt(max(slope, 0)), gaussian=math.sqrt(max(intercept, 0)), gain=float(gain), saltpepper=float(100 * amount),
                slope=float(slope), intercept=float(intercept), alpha=float(alpha), beta=float(beta), levels=len(used), found=True)


def pair_ref(lr, hr, rsf=None):
    """(D, Lc, sigma [N], margin) of uint8 arrays lr [N, m, h, w] and hr [N, C, s*h, s*w]: both sides as util.estimate_noise compares them."""
    lr, hr = np.asarray(lr), np.asarray(hr)
    n_img, c = hr.shape[:2]
    h, w = lr.shape[-2:]
    s = hr.shape[-2] // h
    frames = C.slice_center(lr, c)
    if rsf is None:
        return np.stack([C.reduce_ref(hr[i], h, w) for i in range(n_img)]), frames, np.zeros(n_img), 0
    if isinstance(rsf, str):
        sigmas = F.DEFAULT_SIGMAS
        per_item = F.estimate_ref(lr, hr)[4].tolist()
    elif np.ndim(rsf) == 0:
        sigmas, per_item = [float(rsf)], [0] * n_img
    else:
        sigmas = sorted({float(v) for v in rsf})
        per_item = [sigmas.index(float(v)) for v in rsf]
    rows, radius = F.table(s, sigmas)
    m = F.margin(s, radius)
    d = np.stack([F.reduce_k(hr[i], rows[per_item[i]], s, radius) for i in range(n_img)])
    return d, frames[..., m:h - m, m:w - m], np.array([sigmas[k] for k in per_item], dtype=np.float64), m


def estimate_ref(lr, hr, rsf=None, pool="all", min_count=32, guard=4.0):
    """The whole of util.estimate_noise for batched uint8 arrays: a dict of the thirteen fields (scalars for pool "all", arrays for "item")."""
    d, lc, sigma, m = pair_ref(lr, hr, rsf)
    n_img, c = d.shape[:2]
    table = table_ref(d.reshape(n_img * c, -1), np.ascontiguousarray(lc).reshape(n_img * c, -1)).reshape(n_img, c, 256, 5)
    if pool == "all":
        table = table.sum(axis=(0, 1))
        return dict(fit_ref(table, min_count, guard), table=table, sigma=float(sigma.sum() / n_img), margin=m)
    table = table.sum(axis=1)
    fits = [fit_ref(t, min_count, guard) for t in table]
    out = {k: np.array([f[k] for f in fits]) for k in fits[0]}
    return dict(out, table=table, sigma=sigma, margin=m)


def scene(planes, h, w, seed):
    """uint8 [planes, h, w]: a ramp over the levels 40 .. 200 along x plus N(0, 3), rounded."""
    rng = np.random.default_rng(seed)
    ramp = np.linspace(40.0, 200.0, w)[None, None, :]
    return np.clip(np.rint(ramp + rng.normal(0.0, 3.0, size=(planes, h, w))), 0, 255).astype(np.uint8)


def plant(d, i, g, s, amount, seed):
    """L = clip8(rint(D (1 - i) + i Poisson(D) + g + N(0, s))), then a share ``amount`` of the pixels set to 0 or 255 with equal odds."""
    rng = np.random.default_rng(seed)
    d = np.asarray(d).astype(np.float64)
    x = d * (1 - i) + i * rng.poisson(d) + g + (rng.normal(0.0, s, size=d.shape) if s else 0.0)
    out = np.clip(np.rint(x), 0, 255).astype(np.uint8)
    if amount:
        flipped, salted = rng.random(d.shape) < amount, rng.random(d.shape) < 0.5
        out[flipped & salted] = 255
        out[flipped & ~salted] = 0
    return out
