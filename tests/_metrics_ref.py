"""CPU helpers of the csrc/metrics.hip tests (tests/test_metrics_ref.py, tests/test_gpu_metrics.py).  No GPU import.

* `chunked_pairwise_sum_f32`: numpy's float32 add-reduction of a contiguous array written out step by step.  numpy walks the array in
  pieces of its ufunc buffer size (8192 elements), starts from 0 and adds each piece's PAIRWISE sum in order.  The pairwise sum of n
  elements is: n < 8 -- left to right; n <= 128 -- 8 accumulators over the leading n - n % 8 elements, combined as
  ((r0 + r1) + (r2 + r3)) + ((r4 + r5) + (r6 + r7)), then the remaining n % 8 elements added one by one; otherwise the sum of the two
  halves' pairwise sums, the first half being n // 2 rounded down to a multiple of 8.  tests/test_metrics_ref.py pins this against
  np.add.reduce bit for bit; the kernel rests on the same statement.
* `ssim_exact`, `ssd_exact`: the image metrics from exact integers.  With window sums sa, sb, saa, sbb, sab (N = 49 pixels),
  K1 = 1/100, K2 = 3/100 and L = 255 the per-pixel SSIM is (A1 A2) / (B1 B2) with the integers
      A1 = 2 sa sb D + C1 N^2                       B1 = (sa^2 + sb^2) D + C1 N^2
      A2 = 2 (N sab - sa sb) D + C2 N (N - 1)       B2 = (N saa - sa^2 + N sbb - sb^2) D + C2 N (N - 1)
  where D = 10^4, C1 = 65025 = (K1 L)^2 D, C2 = 585225 = (K2 L)^2 D (the common denominators N^2 D and N (N - 1) D cancel).  Each
  pixel's value is the correctly rounded quotient of two Python ints (|value| <= 1, so at most 2^-54 off), the mean is math.fsum
  of those over the interior, divided once: at most about 2e-16 from the true mean.
* `normalize_preds_raw_cov`: oracle.metrics_ref.normalize_preds with the covariance formed as pssr_normalize_preds_resized_u8 forms
  it, from the raw bytes in float64.
* seeded image makers and the case lists both test modules share.
"""
from __future__ import annotations

import math

import numpy as np

NPY_BUF = 8192
F32 = np.float32


# ------------------------------------------------------------------ numpy's float32 summation
def _pairwise_f32(a):
    n = len(a)
    if n < 8:
        res = F32(-0.0)                    # numpy starts from -0.0 so that a sum of negative zeros keeps its sign
        for v in a:
            res = F32(res + v)
        return res
    if n <= 128:
        lead = n - n % 8
        r = a[:8].copy()
        for i in range(8, lead, 8):
            r = r + a[i:i + 8]             # eight independent float32 accumulators
        res = F32(F32(F32(r[0] + r[1]) + F32(r[2] + r[3])) + F32(F32(r[4] + r[5]) + F32(r[6] + r[7])))
        for v in a[lead:]:
            res = F32(res + v)
        return res
    half = n // 2
    half -= half % 8
    return F32(_pairwise_f32(a[:half]) + _pairwise_f32(a[half:]))


def chunked_pairwise_sum_f32(values):
    """np.add.reduce(values, axis=None) of a C-contiguous float32 array of any rank, as a float32 scalar."""
    a = np.ascontiguousarray(values, dtype=F32).ravel()
    acc = F32(0.0)
    for lo in range(0, len(a), NPY_BUF):
        acc = F32(acc + _pairwise_f32(a[lo:lo + NPY_BUF]))
    return acc


def tail_of(n):
    """Length of the last piece of an n-element reduction and whether full pieces precede it."""
    return (n - 1) % NPY_BUF + 1, n > NPY_BUF


# ------------------------------------------------------------------ exact image metrics
WIN, _D, _C1, _C2 = 7, 10 ** 4, 65025, 585225


def _window_sums(x):
    """Exact sums of the int64 image x over every full WIN x WIN window: [h - 6, w - 6] int64."""
    c = np.zeros((x.shape[0] + 1, x.shape[1] + 1), np.int64)
    c[1:, 1:] = x.cumsum(0).cumsum(1)
    return c[WIN:, WIN:] - c[:-WIN, WIN:] - c[WIN:, :-WIN] + c[:-WIN, :-WIN]


def ssim_terms_exact(a, b):
    """Per interior pixel the exact integers (A1 A2, B1 B2) of the module docstring, as object arrays of Python ints."""
    a, b = np.asarray(a), np.asarray(b)
    assert a.dtype == np.uint8 and b.dtype == np.uint8 and a.shape == b.shape and a.ndim == 2 and min(a.shape) >= WIN
    a, b = a.astype(np.int64), b.astype(np.int64)
    sa, sb, saa, sbb, sab = (_window_sums(v) for v in (a, b, a * a, b * b, a * b))
    n = WIN * WIN
    a1 = 2 * sa * sb * _D + _C1 * n * n                                   # every factor stays below 2^43
    b1 = (sa * sa + sb * sb) * _D + _C1 * n * n
    a2 = 2 * (n * sab - sa * sb) * _D + _C2 * n * (n - 1)
    b2 = ((n * saa - sa * sa) + (n * sbb - sb * sb)) * _D + _C2 * n * (n - 1)
    return a1.astype(object) * a2.astype(object), b1.astype(object) * b2.astype(object)


def ssim_exact(a, b):
    """Mean SSIM of two uint8 images (7x7 uniform window, K1 .01, K2 .03, sample covariance, data range 255, interior mean)."""
    num, den = ssim_terms_exact(a, b)
    vals = [p / q for p, q in zip(num.ravel().tolist(), den.ravel().tolist())]        # int / int is correctly rounded
    return math.fsum(vals) / len(vals)


def ssd_exact(a, b):
    d = np.asarray(a).astype(np.int64).ravel() - np.asarray(b).astype(np.int64).ravel()
    return sum((d * d).tolist())


# ------------------------------------------------------------------ image makers (uint8, any shape [..., H, W]; every call is seeded)
def random_image(shape, seed, lo=0, hi=255):
    return np.random.default_rng(seed).integers(lo, hi + 1, size=shape, dtype=np.uint8)


def flat(shape, value):
    return np.full(shape, value, np.uint8)


def blocks(shape, high=255, block=9):
    """Checkerboard of block x block squares: 0 and `high`."""
    yy, xx = np.indices(shape[-2:])
    board = (((yy // block) + (xx // block)) % 2 * high).astype(np.uint8)
    return np.broadcast_to(board, shape).copy()


def sparse(shape, k, value, seed):
    """Zeros with k pixels of `value` per image, at seeded positions."""
    rng = np.random.default_rng(seed)
    px = shape[-2] * shape[-1]
    out = np.zeros((int(np.prod(shape)) // px, px), np.uint8)
    for img in out:
        img[rng.choice(px, size=k, replace=False)] = value
    return out.reshape(shape)


def two_level(shape, low, high, seed):
    return np.where(np.random.default_rng(seed).random(shape) < 0.5, low, high).astype(np.uint8)


def gradient(shape):
    """A diagonal ramp from 0 to 255."""
    h, w = shape[-2:]
    ramp = np.add.outer(np.arange(h, dtype=np.float64), np.arange(w, dtype=np.float64)) / max(h + w - 2, 1) * 255
    return np.broadcast_to(np.round(ramp).astype(np.uint8), shape).copy()


def saturated(shape, seed, noise=0.0):
    """A Gaussian-blurred field (sigma 3, unit spread per image) scaled by 300 grey levels around 127.5: about two thirds of the
    pixels clip to 0 or 255, in large connected regions.  `noise` adds white noise of that many grey levels before the clip; the field
    itself depends on `seed` alone, so two calls with different `noise` give a pair with the same structure."""
    from scipy import ndimage as ndi
    rng = np.random.default_rng(seed)
    field = ndi.gaussian_filter(rng.normal(size=shape), (0,) * (len(shape) - 2) + (3, 3), mode="reflect")
    field -= field.mean(axis=(-2, -1), keepdims=True)
    field /= np.maximum(field.std(axis=(-2, -1), keepdims=True), 1e-30)
    return np.clip(127.5 + 300 * field + noise * rng.normal(size=shape), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------ normalize_preds, equal sizes: the shared cases
# (B, H, W) -> pixel count, tail piece: see tail_of() and the docstring of tests/test_gpu_metrics.py
NORM_SHAPES = [(2, 1, 2), (1, 1, 7), (1, 3, 3), (1, 1, 128), (1, 3, 43), (1, 10, 13), (1, 8, 17),
               (1, 1, 8191), (1, 8192, 1), (1, 1, 8193), (1, 8199, 1), (2, 91, 91), (1, 64, 130), (1, 8327, 1),
               (3, 100, 100), (1, 129, 127), (1, 181, 181), (2, 300, 211)]
NORM_CONTENTS = ["correlated", "anti", "saturated"]
NORM_PERCENTILES = [(0.1, 99.9), (2.0, 98.0)]


def norm_pair(shape, content):
    seed = sum(shape)
    if content == "correlated":                                             # as test_normalize_preds_bit_exact_vs_oracle
        rng = np.random.default_rng(seed)
        base = rng.normal(120, 40, size=shape)
        hr = np.clip(base + rng.normal(0, 5, size=shape), 0, 255).astype(np.uint8)
        return hr, np.clip(0.7 * base + 30 + rng.normal(0, 9, size=shape), 0, 255).astype(np.uint8)
    if content == "anti":
        hr = norm_pair(shape, "correlated")[0]
        return hr, 255 - hr
    if content == "saturated":
        return saturated(shape, seed), saturated(shape, seed, noise=20.0)
    raise KeyError(content)


EDGE_SHAPE = (1, 100, 100)
EDGE_PERCENTILES = [(0.0, 100.0), (50.0, 50.0), (0.0, 0.0), (100.0, 100.0), (0.1, 0.1)]


def edge_pair():
    """The correlated pair kept off grey level 0, so that a low percentile of the ground truth is never 0 (base_max = 0 is the
    degenerate sparse case, tested on its own)."""
    hr, hat = norm_pair(EDGE_SHAPE, "correlated")
    return np.maximum(hr, 3), hat


def distribution_pairs():
    """name -> (hr, hat, percentile pairs): ground truths whose histogram has two levels, four adjacent levels, or 50 bright pixels.
    The 50 bright pixels are 0.5 % of the image, so only the default (0.1, 99.9) leaves them a non-zero upper percentile; at (2, 98) that
    image is the degenerate sparse case."""
    s, rng = EDGE_SHAPE, np.random.default_rng(11)
    out = {}
    for name, hr, pcts in (("two_level", two_level(s, 3, 4, 12), NORM_PERCENTILES), ("narrow", random_image(s, 13, 120, 123), NORM_PERCENTILES),
                           ("sparse50", sparse(s, 50, 200, 14), NORM_PERCENTILES[:1])):
        out[name] = (hr, np.clip(0.5 * hr + 20 + rng.normal(0, 3, size=s), 0, 255).astype(np.uint8), pcts)
    return out


DEGENERATE_SHAPE = (2, 100, 100)


def degenerate_cases():
    """name -> (hr, hat, zero_hr, zero_hat): per image of the batch, whether that side's reference value is NaN (-> byte 0)."""
    s = DEGENERATE_SHAPE
    ordinary = norm_pair(s, "correlated")
    sp = sparse(s, 4, 255, 21)
    mixed_hr, mixed_hat = ordinary[0].copy(), ordinary[1].copy()
    mixed_hr[0] = 77                                                       # image 0 degenerate, image 1 ordinary
    return {
        "constant_hr": (flat(s, 77), random_image(s, 22), [True, True], [True, True]),
        "constant_hat": (random_image(s, 23), flat(s, 77), [False, False], [True, True]),
        "both_zero": (flat(s, 0), flat(s, 0), [True, True], [True, True]),
        "sparse4": (sp, np.clip(sp // 2 + random_image(s, 24, 0, 20), 0, 255).astype(np.uint8), [True, True], [True, True]),
        "mixed": (mixed_hr, mixed_hat, [True, False], [True, False]),
    }


def oracle_normalize(hr, hat, pmin=0.1, pmax=99.9):
    """oracle.metrics_ref.normalize_preds and the warnings it emitted (a degenerate input announces itself by `invalid value`)."""
    import warnings
    from oracle import metrics_ref as M
    with warnings.catch_warnings(record=True) as caught:
        warnings.simplefilter("always")
        a, b = M.normalize_preds(hr, hat, pmin, pmax)
    return a, b, [str(w.message) for w in caught]


# ------------------------------------------------------------------ normalize_preds, a prediction of another size
RESIZED_SHAPES = [((2, 40, 90), (2, 100, 90)),        # shrink along y only
                  ((1, 50, 90), (1, 120, 60)),        # shrink y, enlarge x
                  ((1, 91, 91), (1, 181, 181)),       # both reductions have tail pieces, shrinking
                  ((1, 181, 181), (1, 91, 91))]       # the same, enlarging


def resized_pair(hr_shape, hat_shape):
    """As test_normalize_preds_with_a_prediction_of_another_size_vs_oracle builds its pair: a smooth field, the prediction its resize."""
    from scipy import ndimage as ndi
    rng = np.random.default_rng(sum(hr_shape) + sum(hat_shape))
    base = ndi.gaussian_filter(rng.normal(120, 40, size=hr_shape), (0, 2, 2)) * 2.5 - 180
    hr = np.clip(base + rng.normal(0, 5, size=hr_shape), 0, 255).astype(np.uint8)
    zoom = (1, hat_shape[1] / hr_shape[1], hat_shape[2] / hr_shape[2])
    hat = np.clip(0.7 * ndi.zoom(base, zoom, order=1, grid_mode=True, mode="mirror") + 30 + rng.normal(0, 6, size=hat_shape), 0, 255)
    return hr, hat.astype(np.uint8)


def normalize_preds_raw_cov(hr, hat, pmin=0.1, pmax=99.9):
    """oracle.metrics_ref.normalize_preds for [n, H, W] / [n, h, w] bytes, except for the covariance: the oracle takes
    np.cov(resize(hat - mean), hr_norm) of float32 images; the device takes, in float64 and from the raw bytes,
        cov = [sum(r * hr) - sum(r) * sum(hr) / n] / (n - 1) / denom,    r = float32(resize_restated(hat)),
    with denom = x_max - x_min + 1e-20 of the ground truth's percentile normalisation (the resize is linear with weights summing to
    one and hr_norm is affine in hr, so the two agree up to rounding)."""
    from oracle import metrics_ref as M
    outs_a, outs_b = [], []
    for g, p in zip(np.asarray(hr), np.asarray(hat)):
        g32, p32 = g.astype(F32), p.astype(F32)
        base_max, base_mean = np.percentile(g32, pmax), np.mean(g32)
        denom = F32(F32(np.percentile(g32, pmax)) - F32(np.percentile(g32, pmin))) + F32(1e-20)
        hn = M._normalize_minmax(g32, pmin, pmax)
        p0 = p32 - np.mean(p32)
        hn = hn - np.mean(hn)
        r = M.resize_restated(p32, g.shape).astype(np.float64)
        g64, n = g.astype(np.float64), g.size
        cov = (np.sum(r * g64) - np.sum(r) * np.sum(g64) / n) / (n - 1) / np.float64(denom)
        amp = cov / np.var(p0.flatten())
        p1 = amp * p0
        a1, p2 = (hn - hn.min()) * base_max, (p1 - hn.min()) * base_max
        outs_a.append(a1 / (a1.mean() / base_mean))
        outs_b.append(p2 / (p2.mean() / base_mean))
    return np.asarray(outs_a).clip(0, 255).astype(np.uint8), np.asarray(outs_b).clip(0, 255).astype(np.uint8)


def within_resized_cap(got, want):
    """The project's bound for the prediction side of another size: at most 1 grey level on at most 0.5 % of the pixels."""
    d = np.abs(got.astype(int) - want.astype(int))
    return bool(d.max() <= 1 and (d > 0).mean() <= 5e-3), (int(d.max()), float((d > 0).mean()))


# ------------------------------------------------------------------ image_metrics: the shared cases
METRIC_SHAPES = [(1, 7, 7), (1, 7, 200), (1, 200, 7), (1, 38, 38), (1, 39, 70), (1, 70, 39), (1, 71, 45), (5, 45, 71)]
METRIC_CONTENTS = ["random", "flat", "zeros_255", "blocks", "saturated", "sparse6", "gradient"]


def metric_pair(shape, content):
    seed = sum(shape)
    if content == "random":
        a = random_image(shape, seed)
        b = np.clip(a.astype(np.int32) + np.random.default_rng(seed + 1).integers(-40, 41, size=shape), 0, 255).astype(np.uint8)
        return a, b
    if content == "flat":
        return flat(shape, 255), flat(shape, 254)
    if content == "zeros_255":
        return flat(shape, 0), flat(shape, 255)
    if content == "blocks":
        return blocks(shape, 255), blocks(shape, 250)
    if content == "saturated":
        return saturated(shape, seed), saturated(shape, seed, noise=20.0)
    if content == "sparse6":
        return sparse(shape, 6, 255, seed), sparse(shape, 6, 200, seed + 1)
    if content == "gradient":
        g = gradient(shape)
        return g, np.ascontiguousarray(g[..., ::-1])
    raise KeyError(content)
