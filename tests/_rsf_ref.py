"""The definitions of the resolution-scaling-function search (include/pssr_mi355.h: "Estimate of the resolution-scaling function")
restated in numpy int64 and Python ints, from the definitions and not from the kernel: the tap table, D_k by two strided passes, the
sums, the choice with fractions, and the whole of util.estimate_rsf and util.consistency_map(rsf=...).  tests/test_rsf_host.py checks
the sigma = 0 row against PIL.Image.resize itself."""
import math
from fractions import Fraction

import numpy as np

import _consistency_ref as C
import _register_ref as R

PRECISION_BITS = C.PRECISION_BITS
ONE = 1 << PRECISION_BITS
DEFAULT_SIGMAS = [0.25 * i for i in range(33)]
FWHM = 2.0 * math.sqrt(2.0 * math.log(2.0))

margin = R.margin


def rad(sigma):
    return 0 if sigma == 0 else math.ceil(3 * sigma)


def table(s, sigmas, radius=None):
    """(rows [K][2 s + 2 R] of Python ints, R)."""
    interior = R.interior_taps(s)
    big = max(rad(v) for v in sigmas)
    if radius is None:
        radius = big
    assert radius >= big
    rows = []
    for sigma in sigmas:
        r = rad(sigma)
        if sigma == 0:
            ks = list(interior)
        else:
            g = [math.exp(-(i * i) / (2.0 * sigma * sigma)) for i in range(-r, r + 1)]
            norm = math.fsum(g)
            g = [v / norm for v in g]
            t = [k / ONE for k in interior]
            ks = []
            for n in range(2 * s + 2 * r):
                terms = [g[i] * t[n - i] for i in range(2 * r + 1) if 0 <= n - i < 2 * s]
                ks.append(math.floor(math.fsum(terms) * ONE + 0.5))
            ks[ks.index(max(ks))] += ONE - sum(ks)
        rows.append([0] * (radius - r) + ks + [0] * (radius - r))
    return rows, radius


def _strided_pass(img, row, s, n_out, start):
    """uint8 [..., n] -> uint8 [..., n_out]: output x applies the row to img[..., start + s x + j], then clip8."""
    wide = img.astype(np.int64)
    acc = np.full(img.shape[:-1] + (n_out,), 1 << (PRECISION_BITS - 1), dtype=np.int64)
    for j, k in enumerate(row):
        if k:
            acc += wide[..., start + j:start + j + s * (n_out - 1) + 1:s] * int(k)
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def reduce_k(y, row, s, radius):
    """D of uint8 planes y [..., s*h, s*w] for one row of a table: uint8 [..., h - 2m, w - 2m]."""
    y = np.asarray(y)
    h, w = y.shape[-2] // s, y.shape[-1] // s
    assert y.dtype == np.uint8 and y.shape[-2:] == (s * h, s * w) and len(row) == 2 * s + 2 * radius
    m = margin(s, radius)
    hc, wc = h - 2 * m, w - 2 * m
    assert hc >= 1 and wc >= 1
    start = s * m - s // 2 - radius
    assert start >= 0 and start + s * (hc - 1) + len(row) <= s * h and start + s * (wc - 1) + len(row) <= s * w
    t = _strided_pass(y, row, s, wc, start)
    return np.swapaxes(_strided_pass(np.swapaxes(t, -1, -2), row, s, hc, start), -1, -2)


def sums_ref(y, l, rows, radius):
    """Python-int rows [planes][3 K + 2] of uint8 planes y [planes, s*h, s*w] and l [planes, h, w]."""
    y, l = np.asarray(y), np.asarray(l)
    h, w = l.shape[-2:]
    s = y.shape[-2] // h
    m = margin(s, radius)
    return sums_of([reduce_k(y, row, s, radius) for row in rows], l[..., m:h - m, m:w - m])


def sums_of(ds, lc):
    """The rows of the K reduced stacks ``ds`` (each uint8 [planes, h', w']) against ``lc`` [planes, h', w']."""
    lc = np.asarray(lc).astype(np.int64)
    cols = []                                    # int64 is exact here: no sum passes 2^28 * 255^2
    for d in ds:
        d = np.asarray(d).astype(np.int64)
        cols += [d.sum(axis=(-2, -1)), (d * d).sum(axis=(-2, -1)), (d * lc).sum(axis=(-2, -1))]
    cols += [lc.sum(axis=(-2, -1)), (lc * lc).sum(axis=(-2, -1))]
    return [[int(v) for v in r] for r in np.stack(cols, axis=-1)]


def choose_ref(n, rows, K):
    """(k, curve) from the rows of the pooled planes: exact rational scores, the smaller index on a tie."""
    pooled = [sum(r[q] for r in rows) for q in range(3 * K + 2)]
    sl, sll = pooled[-2:]
    denl = n * sll - sl ** 2
    scored, curve = [], []
    for k in range(K):
        sd, sdd, sdl = pooled[3 * k:3 * k + 3]
        num, den = n * sdl - sd * sl, n * sdd - sd ** 2
        ok = den != 0 and denl != 0
        scored.append((-(Fraction(num * abs(num), den * denl) if ok else Fraction(0)), k))
        curve.append(num / math.sqrt(den * denl) if ok else 0.0)
    return min(scored)[1], curve


def planted_pair(rng, n_img, c_hat, c_lr, h, w, s, rows, radius, k_true):
    """Random sharp items and LR items whose centre frames are, inside the margin, D_k of the sharp item for a known k per item (the other
    LR frames and the margin are random): (hat [N, C, s*h, s*w], lr [N, c, h, w])."""
    m = margin(s, radius)
    hat = rng.integers(0, 256, size=(n_img, c_hat, s * h, s * w), dtype=np.uint8)
    lr = rng.integers(0, 256, size=(n_img, c_lr, h, w), dtype=np.uint8)
    centre = C.slice_center(lr, c_hat)           # a view: writing it writes lr
    for i, k in enumerate(k_true):
        centre[i, :, m:h - m, m:w - m] = reduce_k(hat[i], rows[k], s, radius)
    return hat, lr


def estimate_ref(lr, hat, sigmas=None, pool="item", pixel_size=1.0):
    """The whole of util.estimate_rsf for uint8 arrays [N, m, h, w] and [N, C, s*h, s*w]: (sigma, fwhm, score [N], curve [N, K],
    index [N], margin)."""
    lr, hat = np.asarray(lr), np.asarray(hat)
    sigmas = DEFAULT_SIGMAS if sigmas is None else list(sigmas)
    n_img, c = hat.shape[:2]
    h, w = lr.shape[-2:]
    s = hat.shape[-2] // h
    rows, radius = table(s, sigmas)
    m = margin(s, radius)
    n = c * (h - 2 * m) * (w - 2 * m)
    frames = C.slice_center(lr, c)
    sums = [sums_ref(hat[i], frames[i], rows, radius) for i in range(n_img)]
    if pool == "all":
        chosen = [choose_ref(n_img * n, [r for item in sums for r in item], len(sigmas))] * n_img
    else:
        chosen = [choose_ref(n, item, len(sigmas)) for item in sums]
    sigma = np.array([sigmas[k] * pixel_size for k, _ in chosen], dtype=np.float64)
    return (sigma, FWHM * sigma, np.array([curve[k] for k, curve in chosen], dtype=np.float64),
            np.array([curve for _, curve in chosen], dtype=np.float64), np.array([k for k, _ in chosen], dtype=np.int64), m)


def consistency_ref(lr, hat, rsf, fit="affine"):
    """The whole of util.consistency_map(rsf=...) for uint8 arrays: (map [N, C, h', w'], alpha, beta, rse, rsp [N, C], sigma [N], margin).
    ``rsf``: "fit", one sigma, or one per item."""
    lr, hat = np.asarray(lr), np.asarray(hat)
    n_img, c = hat.shape[:2]
    h, w = lr.shape[-2:]
    s = hat.shape[-2] // h
    if isinstance(rsf, str):
        sigmas = DEFAULT_SIGMAS
        per_item = estimate_ref(lr, hat)[4].tolist()
    elif np.ndim(rsf) == 0:
        sigmas, per_item = [float(rsf)], [0] * n_img
    else:
        sigmas = sorted({float(v) for v in rsf})
        per_item = [sigmas.index(float(v)) for v in rsf]
    rows, radius = table(s, sigmas)
    m = margin(s, radius)
    hc, wc = h - 2 * m, w - 2 * m
    frames = C.slice_center(lr, c)[..., m:h - m, m:w - m]
    cmap = np.empty((n_img, c, hc, wc), dtype=np.uint8)
    stats = np.empty((4, n_img, c), dtype=np.float64)
    for i in range(n_img):
        d = reduce_k(hat[i], rows[per_item[i]], s, radius)
        for j in range(c):
            alpha, beta, rsp = C.fit_ref(hc * wc, C.moments_ref(d[j], frames[i, j]), fit)
            cmap[i, j], sse = C.map_ref(d[j], frames[i, j], C.table_ref(alpha, beta))
            stats[:, i, j] = alpha, beta, C.rse_ref(sse, hc * wc), rsp
    return cmap, stats[0], stats[1], stats[2], stats[3], np.array([sigmas[k] for k in per_item], dtype=np.float64), m
