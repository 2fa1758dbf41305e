"""The consistency definitions (include/pssr_mi355.h: "Consistency of a prediction with its own low-resolution input") restated in numpy
int64 and Python ints, from the definitions and not from the kernels: Pillow's 8-bit bilinear taps, the two-pass reduction with the
uint8 rounding between the passes, the five moments, the fit, the table, the map and rse.  tests/test_consistency_host.py checks the
reduction against PIL.Image.resize itself."""
import math

import numpy as np

PRECISION_BITS = 32 - 8 - 2
FITS = ("affine", "identity")


def taps(out_size, in_size):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc for the triangle filter: ``[(xmin, [k ...]) ...]``, one per output index.
    Python floats are C doubles, and the operations are in Pillow's order."""
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = 1.0 * filterscale
    ss = 1.0 / filterscale
    out = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        ws = []
        for x in range(xmax - xmin):
            a = abs((x + xmin - center + 0.5) * ss)
            ws.append(1.0 - a if a < 1.0 else 0.0)
        ww = sum(ws)            # left to right from 0.0, as the C loop
        ks = []
        for v in ws:
            v = v / ww if ww != 0.0 else v
            ks.append(int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS)))
        out.append((xmin, ks))
    return out


def _clip8(v):
    return np.clip(v >> PRECISION_BITS, 0, 255).astype(np.uint8)


def _pass(img, out_size):
    """One resampling pass along the last axis of a uint8 array [..., in_size]."""
    res = np.empty(img.shape[:-1] + (out_size,), dtype=np.uint8)
    wide = img.astype(np.int64)
    for xx, (xmin, ks) in enumerate(taps(out_size, img.shape[-1])):
        acc = np.full(img.shape[:-1], 1 << (PRECISION_BITS - 1), dtype=np.int64)
        for j, k in enumerate(ks):
            acc += wide[..., xmin + j] * k
        res[..., xx] = _clip8(acc)
    return res


def reduce_ref(y, h, w):
    """uint8 [..., H, W] -> uint8 [..., h, w]: horizontal pass, uint8, vertical pass (Pillow's order for a two-axis resize)."""
    y = np.asarray(y)
    assert y.dtype == np.uint8
    tmp = _pass(y, w)
    return np.swapaxes(_pass(np.swapaxes(tmp, -1, -2), h), -1, -2)


def moments_ref(d, l):
    """Python ints (Sd, Sl, Sdd, Sdl, Sll) of one plane pair."""
    d, l = np.asarray(d).astype(np.int64).reshape(-1), np.asarray(l).astype(np.int64).reshape(-1)
    return int(d.sum()), int(l.sum()), int((d * d).sum()), int((d * l).sum()), int((l * l).sum())


def fit_ref(n, sums, fit="affine"):
    """(alpha, beta, rsp) in the definitions' own expressions."""
    sd, sl, sdd, sdl, sll = sums
    num = n * sdl - sd * sl
    den = n * sdd - sd ** 2
    denl = n * sll - sl ** 2
    if fit == "affine":
        if den == 0:
            alpha, beta = 0.0, sl / n
        else:
            alpha = num / den
            beta = (sl - alpha * sd) / n
    elif fit == "identity":
        alpha, beta = 1.0, 0.0
    else:
        raise ValueError(fit)
    rsp = num / math.sqrt(den * denl) if den > 0 and denl > 0 else 0.0
    return alpha, beta, rsp


def table_ref(alpha, beta):
    return np.array([min(max(round(256.0 * (alpha * d + beta)), -65536), 131071) for d in range(256)], dtype=np.int32)


def map_ref(d, l, table):
    """(uint8 map like d, Python int sse) of one plane pair."""
    e = np.abs(256 * np.asarray(l).astype(np.int64) - np.asarray(table).astype(np.int64)[np.asarray(d)])
    return np.minimum(255, (e + 128) >> 8).astype(np.uint8), int((e * e).sum())


def rse_ref(sse, n):
    return math.sqrt(sse / n) / 256


def slice_center(a, n_frames):
    """``_slice_center`` (the centre ``n_frames`` frames of [..., C, H, W])."""
    center, half = a.shape[-3] // 2, n_frames // 2
    return a[..., center - half:center + half + (n_frames % 2), :, :]


def consistency_ref(lr, hat, fit="affine"):
    """The whole of util.consistency_map for uint8 arrays [N, m, h, w] and [N, C, H, W]: (map [N, C, h, w], alpha, beta, rse, rsp
    float64 [N, C])."""
    lr, hat = np.asarray(lr), np.asarray(hat)
    n_img, c = hat.shape[:2]
    frames = slice_center(lr, c)
    h, w = frames.shape[-2:]
    d = reduce_ref(hat, h, w)
    cmap = np.empty((n_img, c, h, w), dtype=np.uint8)
    stats = np.empty((4, n_img, c), dtype=np.float64)
    for i in range(n_img):
        for j in range(c):
            alpha, beta, rsp = fit_ref(h * w, moments_ref(d[i, j], frames[i, j]), fit)
            cmap[i, j], sse = map_ref(d[i, j], frames[i, j], table_ref(alpha, beta))
            stats[:, i, j] = alpha, beta, rse_ref(sse, h * w), rsp
    return cmap, stats[0], stats[1], stats[2], stats[3]
