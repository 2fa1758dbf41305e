"""The decorrelation-analysis definitions (include/pssr_mi355.h: "Resolution of one image by decorrelation analysis") restated in numpy,
from the definitions and not from the kernel: the block means, the ring sums through numpy's float64 FFT (``rings_ref``) and through the
two matrix products in float32 (``rings_f32``: the yardstick for round-off, not the code under test), the ring populations, the curves,
the peak rule, the filter family and the result in plain Python floats, and the blurred inputs of the tests.  Blocks, tables, the ring map
and the planted images are those of tests/_frc_ref.py."""
import math

import numpy as np

import _frc_ref as F

MIN_DROP = 5e-4
LAST_SIGMA = 0.15


def means(blocks):
    """Step 1: uint8 [..., n, n] -> float32 [...]: the integer sum over n^2, divided in double, rounded once."""
    n = blocks.shape[-1]
    S = blocks.astype(np.int64).sum(axis=(-2, -1))
    return (S.astype(np.float64) / float(n * n)).astype(np.float32)


def centred(blocks):
    """float32 [..., n, n]: float32(a) - m."""
    c = blocks.astype(np.float32) - means(blocks)[..., None, None]
    assert c.dtype == np.float32
    return c


def pop(n):
    """float64 [n // 2 + 1]: coefficients of the full spectrum per kept ring."""
    R = n // 2
    rmap = F.ring_map(n).ravel()
    return np.bincount(rmap[rmap <= R], minlength=R + 1).astype(np.float64)


def _sums_full(spec, n):
    """complex [..., n, n] full spectra -> float64 [..., n // 2 + 1, 2]: sum |F| and sum |F|^2 per ring."""
    R = n // 2
    rmap = F.ring_map(n).ravel()
    keep = rmap <= R
    mod = np.abs(spec).astype(np.float64).reshape(spec.shape[:-2] + (n * n,))
    out = np.zeros(spec.shape[:-2] + (R + 1, 2), dtype=np.float64)
    flat, oflat = mod.reshape(-1, n * n), out.reshape(-1, R + 1, 2)
    for i in range(flat.shape[0]):
        oflat[i, :, 0] = np.bincount(rmap[keep], weights=flat[i, keep], minlength=R + 1)
        oflat[i, :, 1] = np.bincount(rmap[keep], weights=flat[i, keep] ** 2, minlength=R + 1)
    return out


def spectrum_ref(a, n, name="hann"):
    """uint8 [P][H][W] -> complex128 [P][nby * nbx][n][n]: fft2 of (a - m) w (x) w per block, m the float32 mean of step 1."""
    w = F.window(n, name)
    return np.fft.fft2(centred(F.blocks(a, n)).astype(np.float64) * (w[:, None] * w[None, :]))


def rings_ref(a, n, name="hann"):
    """uint8 [P][H][W] -> float64 [P][nby * nbx][n // 2 + 1][2]: numpy's float64 fft2, full spectrum."""
    return _sums_full(spectrum_ref(a, n, name), n)


def rings_f32(a, n, name="hann"):
    """The same sums through the two matrix products in numpy float32 against the float32 tables (the kept columns, the interior ones
    doubled), |F|^2 and its root in float32, sums in float64: how far float32 transforms lie from ``rings_ref``."""
    ct, st = F.tables(n, name)
    R, K = n // 2, n // 2 + 1
    x = centred(F.blocks(a, n))
    tr, ti = x @ ct[:, :K], x @ st[:, :K]
    fr = ct.T @ tr - st.T @ ti
    fi = ct.T @ ti + st.T @ tr
    p = fr * fr + fi * fi
    m = np.sqrt(p)
    assert p.dtype == np.float32 and m.dtype == np.float32
    wgt = np.ones(K, dtype=np.float32)
    wgt[1:R] = 2
    terms = np.stack([wgt * m, wgt * p], axis=-1).astype(np.float64)
    rmap = F.ring_map(n)[:, :K].ravel()
    keep = rmap <= R
    flat = terms.reshape(-1, n * K, 2)
    out = np.zeros((flat.shape[0], R + 1, 2), dtype=np.float64)
    for i in range(flat.shape[0]):
        for k in range(2):
            out[i, :, k] = np.bincount(rmap[keep], weights=flat[i, keep, k], minlength=R + 1)
    return out.reshape(terms.shape[:2] + (R + 1, 2))


def errors(got, ref, n):
    """(err_A, err_P): max over the rings r >= 1 of |A - A_ref| / sqrt(pop[r] P_ref[r]) and of |P - P_ref| / P_ref[r] (rings with
    P_ref = 0 must be matched exactly and count as 0).  Ring 0 is the one coefficient F[0][0], which the mean removal cancels: under
    "none" it is the rounding residue of the float32 mean times n^2, under the Hann window little more, so its own size is no unit for
    its round-off (against P_ref[0] the float32 numpy yardstick itself is off by factors of 1 to 40 at every n whose mean is not
    representable).  Its round-off is that of any other single coefficient, proportional to the spectrum of the block, so ring 0 is
    measured in the units of the whole block: |A - A_ref| / sqrt(sum_rho P_ref[rho]) and |P - P_ref| / sum_rho P_ref[rho].  Ring 0
    enters no curve (step 3)."""
    assert got.shape == ref.shape
    scale_a, scale_p = np.sqrt(pop(n) * ref[..., 1]), ref[..., 1].copy()
    total = ref[..., 1].sum(axis=-1)
    scale_a[..., 0], scale_p[..., 0] = np.sqrt(total), total
    da, dp = np.abs(got[..., 0] - ref[..., 0]), np.abs(got[..., 1] - ref[..., 1])
    zero = scale_p == 0
    assert not da[zero].any() and not dp[zero].any()
    ea = np.divide(da, scale_a, out=np.zeros_like(da), where=~zero)
    ep = np.divide(dp, scale_p, out=np.zeros_like(dp), where=~zero)
    return float(ea.max()), float(ep.max())


# ------------------------------------------------------------------------------------------------ steps 3 - 7 in Python floats
def curve_ref(A, P, M, g):
    """Step 4: lists over rings 0 .. R (ring 0 unused) -> d[0 .. R]."""
    R = len(A) - 1
    power = math.fsum(g[r] * g[r] * P[r] for r in range(1, R + 1))
    d, run = [0.0] * (R + 1), 0.0
    for r in range(1, R + 1):
        run += g[r] * A[r]
        den = math.sqrt(power * M[r])
        d[r] = run / den if den > 0 else 0.0
    return d


def peak_ref(d):
    """Step 5 -> (i, p, d[i]) or None."""
    R = len(d) - 1
    for e in range(R, 1, -1):
        top = max(d[1:e + 1])
        i = next(r for r in range(1, e + 1) if d[r] == top)
        if i == e:
            continue
        if d[i] - min(d[i:e + 1]) >= MIN_DROP:
            bend = d[i - 1] - 2 * d[i] + d[i + 1]
            p = i + 0.5 * (d[i - 1] - d[i + 1]) / bend if bend < 0 else float(i)
            return i, p, d[i]
    return None


def family_ref(R, i0, filters):
    """Step 6: the widths s_j."""
    s0 = min(2 * R / i0, R) if i0 else float(R)
    if filters <= 1:
        return [s0] * filters
    return [s0 * (LAST_SIGMA / s0) ** (j / (filters - 1)) for j in range(filters)]


def resolve_ref(sums, n, filters=10, pixel_size=1.0):
    """Steps 3 - 7 of sums [..., R + 1, 2], every leading axis pooled -> dict(resolution, found, peak, amplitude, curves, chosen, peaks)."""
    R = n // 2
    flat = np.asarray(sums, dtype=np.float64).reshape(-1, R + 1, 2)
    B = flat.shape[0]
    A = [math.fsum(flat[:, r, 0]) for r in range(R + 1)]
    P = [math.fsum(flat[:, r, 1]) for r in range(R + 1)]
    counts = pop(n)
    M = [0.0] * (R + 1)
    for r in range(1, R + 1):
        M[r] = M[r - 1] + B * counts[r]
    curves = [curve_ref(A, P, M, [1.0] * (R + 1))]
    peaks = [peak_ref(curves[0])]
    for s in family_ref(R, peaks[0][0] if peaks[0] else None, filters):
        g = [1.0 - math.exp(-2.0 * s * s * (r / R) ** 2) for r in range(R + 1)]
        curves.append(curve_ref(A, P, M, g))
        peaks.append(peak_ref(curves[-1]))
    chosen = None
    for k, pk in enumerate(peaks):
        if pk is not None and (chosen is None or pk[1] > peaks[chosen][1]):
            chosen = k
    out = dict(curves=np.array(curves), peaks=peaks, chosen=chosen, found=chosen is not None)
    if chosen is None:
        out.update(resolution=2.0 * pixel_size, peak=math.nan, amplitude=0.0)
    else:
        out.update(resolution=pixel_size * n / peaks[chosen][1], peak=peaks[chosen][1], amplitude=peaks[chosen][2])
    return out


# ------------------------------------------------------------------------------------------------ inputs
PLANTED = ((64, 12), (128, 24), (250, 40), (500, 100))


def planted(n, r0, seed):
    return F.planted_pair(n, r0, seed)[0]


def blurred(n, sigma, seed):
    """uint8 [n][n]: white Gaussian noise blurred with a Gaussian of ``sigma`` pixels (in the Fourier domain, periodic), scaled to standard
    deviation 40 around 128, plus Gaussian noise of sigma 6, rounded and clipped."""
    rng = np.random.default_rng(seed)
    f = np.fft.fftfreq(n)
    transfer = np.exp(-2.0 * (np.pi * sigma) ** 2 * (f[:, None] ** 2 + f[None, :] ** 2))
    low = np.fft.ifft2(np.fft.fft2(rng.standard_normal((n, n))) * transfer).real
    low = 128 + 40 * (low - low.mean()) / low.std()
    return np.clip(np.rint(low + 6 * rng.standard_normal((n, n))), 0, 255).astype(np.uint8)


# ------------------------------------------------------------------------------------------------ the GPU tests' bound
# (err_A, err_P) of ``errors(rings_f32, rings_ref)``, the worst over the inputs of ``sums_inputs(n)``, measured on the CPU
# (tests/test_decorr_host.py prints them again and checks that they still hold):
F32_ERROR = {16: (3.334e-07, 7.816e-07), 18: (3.502e-07, 5.016e-07), 30: (2.699e-07, 6.577e-07), 34: (1.733e-07, 4.396e-07),
             64: (2.398e-07, 5.580e-07), 66: (1.952e-07, 4.123e-07), 130: (6.356e-07, 9.622e-07), 500: (2.475e-07, 5.207e-07),
             1024: (4.782e-07, 9.289e-07)}
MARGIN = 8          # the rule of tests/_frc_ref.py: the MFMA's one ascending chain is not numpy's blocked sum
SUMS_SIZES = F.SUMS_SIZES
BIG_SIZES = F.BIG_SIZES


def tol(n):
    return MARGIN * F32_ERROR[n][0], MARGIN * F32_ERROR[n][1]


def sums_inputs(n):
    """``(a, window)`` with a uint8 [1][n][n]: the first image of every case of ``_frc_ref.sums_inputs(n)``."""
    return [(a, name) for a, _, name in F.sums_inputs(n)]


def f32_error(n):
    """The measurement behind F32_ERROR[n]."""
    worst_a = worst_p = 0.0
    for a, name in sums_inputs(n):
        ea, ep = errors(rings_f32(a, n, name), rings_ref(a, n, name), n)
        worst_a, worst_p = max(worst_a, ea), max(worst_p, ep)
    return worst_a, worst_p
