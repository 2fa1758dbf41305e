"""The registration definitions (include/pssr_mi355.h: "Registration of real (HR, LR) pairs") restated in numpy int64 and Python ints, from
the definitions and not from the kernel: the interior taps, the dense filtered map, D_t, the sums, the choice and the crop.
tests/test_register_host.py checks D_t against PIL.Image.resize itself."""
import math

import numpy as np

import _consistency_ref as C

PRECISION_BITS = C.PRECISION_BITS


def margin(s, radius):
    return 1 + -(-radius // s)


def shifts(radius):
    """Every (ty, tx) in row-index order."""
    return [(ty, tx) for ty in range(-radius, radius + 1) for tx in range(-radius, radius + 1)]


def interior_taps(s):
    """The 2 s coefficients of an interior output of Pillow's reduction by s (output 1 of 4, reduced from 4 s), which start at input
    index s x - s // 2."""
    xmin, ks = C.taps(4, 4 * s)[1]
    assert xmin == s - s // 2 and len(ks) == 2 * s
    return ks


def _filter_last(img, ks):
    """uint8 [..., n] -> uint8 [..., n - len(ks) + 1]: position j applies the taps to img[..., j : j + len(ks)], then clip8."""
    n = img.shape[-1] - len(ks) + 1
    wide = img.astype(np.int64)
    acc = np.full(img.shape[:-1] + (n,), 1 << (PRECISION_BITS - 1), dtype=np.int64)
    for j, k in enumerate(ks):
        acc += wide[..., j:j + n] * k
    return np.clip(acc >> PRECISION_BITS, 0, 255).astype(np.uint8)


def dense(hr, s):
    """The filtered map at every HR position whose tap window lies inside the plane: F[Y - s // 2][X - s // 2] is the two-pass reduction
    (horizontal, clip8, vertical, clip8) whose windows start s // 2 before HR position (Y, X)."""
    ks = interior_taps(s)
    tmp = _filter_last(np.asarray(hr), ks)
    return np.swapaxes(_filter_last(np.swapaxes(tmp, -1, -2), ks), -1, -2)


def reduced_windows(hr, h, w, radius):
    """{(ty, tx): D_t uint8 [..., h', w']} of uint8 planes [..., s*h, s*w]."""
    hr = np.asarray(hr)
    s = hr.shape[-2] // h
    assert hr.dtype == np.uint8 and hr.shape[-2:] == (s * h, s * w)
    m = margin(s, radius)
    hc, wc = h - 2 * m, w - 2 * m
    assert hc >= 1 and wc >= 1
    f = dense(hr, s)
    out = {}
    for ty, tx in shifts(radius):
        y0, x0 = s * m + ty - s // 2, s * m + tx - s // 2
        assert y0 >= 0 and x0 >= 0 and y0 + s * (hc - 1) < f.shape[-2] and x0 + s * (wc - 1) < f.shape[-1]
        out[(ty, tx)] = f[..., y0:y0 + s * (hc - 1) + 1:s, x0:x0 + s * (wc - 1) + 1:s]
    return out


def sums_ref(hr, lr, radius):
    """Python-int rows [planes][3 T + 2] of uint8 planes hr [planes, s*h, s*w] and lr [planes, h, w]."""
    hr, lr = np.asarray(hr), np.asarray(lr)
    h, w = lr.shape[-2:]
    s = hr.shape[-2] // h
    m = margin(s, radius)
    windows = reduced_windows(hr, h, w, radius)
    lc = lr[..., m:h - m, m:w - m].astype(np.int64)
    cols = []                                    # int64 is exact here: no sum passes 2^28 * 255^2
    for t in shifts(radius):
        d = windows[t].astype(np.int64)
        cols += [d.sum(axis=(-2, -1)), (d * d).sum(axis=(-2, -1)), (d * lc).sum(axis=(-2, -1))]
    cols += [lc.sum(axis=(-2, -1)), (lc * lc).sum(axis=(-2, -1))]
    return [[int(v) for v in row] for row in np.stack(cols, axis=-1)]


def choose_ref(n, rows, radius):
    """((ty, tx), score) of one item from its planes' rows: pooled sums, exact rational scores (fractions of Python ints), the tie rule."""
    from fractions import Fraction
    t_count = (2 * radius + 1) ** 2
    pooled = [sum(r[q] for r in rows) for q in range(3 * t_count + 2)]
    sl, sll = pooled[-2:]
    denl = n * sll - sl ** 2
    scored = []
    for i, (ty, tx) in enumerate(shifts(radius)):
        sd, sdd, sdl = pooled[3 * i:3 * i + 3]
        num, den = n * sdl - sd * sl, n * sdd - sd ** 2
        ok = den != 0 and denl != 0
        score = Fraction(num * abs(num), den * denl) if ok else Fraction(0)
        scored.append((-score, ty * ty + tx * tx, ty, tx, num / math.sqrt(den * denl) if ok else 0.0))
    best = min(scored)
    return (best[2], best[3]), best[4]


def crop_ref(hr, lr, shift, radius):
    """(hr_out, lr_out) of one item [C, s*h, s*w] / [c, h, w] for its chosen shift."""
    h, w = lr.shape[-2:]
    s = hr.shape[-2] // h
    m = margin(s, radius)
    ty, tx = shift
    return hr[..., s * m + ty:s * (h - m) + ty, s * m + tx:s * (w - m) + tx], lr[..., m:h - m, m:w - m]


def register_ref(hr, lr, radius):
    """The whole of util.register_pairs for uint8 arrays [N, C, s*h, s*w] and [N, c, h, w]: (hr_out, lr_out, shift [N, 2], score [N], m)."""
    hr, lr = np.asarray(hr), np.asarray(lr)
    n_img, c_hr = hr.shape[:2]
    h, w = lr.shape[-2:]
    s = hr.shape[-2] // h
    m = margin(s, radius)
    frames = C.slice_center(lr, c_hr)
    outs, shift, score = [], [], []
    for i in range(n_img):
        t, sc = choose_ref(c_hr * (h - 2 * m) * (w - 2 * m), sums_ref(hr[i], frames[i], radius), radius)
        outs.append(crop_ref(hr[i], lr[i], t, radius))
        shift.append(t)
        score.append(sc)
    return (np.stack([o[0] for o in outs]), np.stack([o[1] for o in outs]), np.array(shift, dtype=np.int64).reshape(n_img, 2),
            np.array(score, dtype=np.float64), m)


def planted_pair(rng, n_img, c_hr, c_lr, h, w, s, radius, shifts_per_item):
    """Random HR items and LR items whose centre frames are the restated reduction of the HR item moved by a known shift per item (the
    other LR frames and the LR margin are random): (hr [N, C, s*h, s*w], lr [N, c, h, w])."""
    m = margin(s, radius)
    hr = rng.integers(0, 256, size=(n_img, c_hr, s * h, s * w), dtype=np.uint8)
    lr = rng.integers(0, 256, size=(n_img, c_lr, h, w), dtype=np.uint8)
    centre = C.slice_center(lr, c_hr)           # a view: writing it writes lr
    for i, t in enumerate(shifts_per_item):
        centre[i, :, m:h - m, m:w - m] = reduced_windows(hr[i], h, w, radius)[tuple(t)]
    return hr, lr
