"""The directional-resolution definitions (include/pssr_mi355.h: "Directional resolution", steps S1 - S6) restated in numpy, from the text
and not from the kernel: the boundary vectors, the sector of every coefficient of the full spectrum with the mirror rule, the populations,
the (ring, sector) sums through numpy's float64 FFT (``*_ref``) and through the two float32 matrix products (``*_f32``: the yardstick for
round-off, not the code under test), the per-sector curve with the empty-cell rule, and the anisotropic inputs of the tests.  Blocks,
windows, tables, rings and the isotropic inputs are those of tests/_frc_ref.py and tests/_decorr_ref.py."""
import math

import numpy as np

import _decorr_ref as D
import _frc_ref as F

MAX_SECTORS = 16


def bounds(S):
    """Step S1: (bx, by), int64 [S]."""
    beta = [(j + 0.5) * math.pi / S for j in range(S)]
    return (np.array([round(2 ** 20 * math.cos(b)) for b in beta], dtype=np.int64),
            np.array([round(2 ** 20 * math.sin(b)) for b in beta], dtype=np.int64))


def sector_map(n, S):
    """int64 [n][n]: the sector of every coefficient (ky, kx) of the full spectrum; kx > n / 2 takes the sector of its Hermitian mirror."""
    R = n // 2
    ky, kx = np.meshgrid(np.arange(n, dtype=np.int64), np.arange(n, dtype=np.int64), indexing="ij")
    mirror = kx > R
    ky, kx = np.where(mirror, (n - ky) % n, ky), np.where(mirror, n - kx, kx)
    fy = np.where(ky <= R, ky, ky - n)
    up = fy >= 0
    gx, gy = np.where(up, kx, -kx), np.where(up, fy, -fy)
    bx, by = bounds(S)
    return (bx[:, None, None] * gy[None] - by[:, None, None] * gx[None] >= 0).sum(axis=0) % S


def cell_map(n, S):
    """(cell index ring * S + sector, keep) of the full spectrum, flattened; ``keep`` drops the rings above n // 2."""
    rmap = F.ring_map(n).ravel()
    return rmap * S + sector_map(n, S).ravel(), rmap <= n // 2


def pop(n, S):
    """Step S4: int64 [n // 2 + 1][S]."""
    cells, keep = cell_map(n, S)
    return np.bincount(cells[keep], minlength=(n // 2 + 1) * S).reshape(n // 2 + 1, S)


def _bin(terms, cells, keep, R, S):
    """float64 [..., coefficients, k] -> [..., R + 1, S, k]: bincount over the cells."""
    k = terms.shape[-1]
    flat = terms.reshape(-1, terms.shape[-2], k)
    out = np.zeros((flat.shape[0], (R + 1) * S, k), dtype=np.float64)
    for i in range(flat.shape[0]):
        for q in range(k):
            out[i, :, q] = np.bincount(cells[keep], weights=flat[i, keep, q], minlength=(R + 1) * S)
    return out.reshape(terms.shape[:-2] + (R + 1, S, k))


def sectors_ref(a, b, n, S, name="hann"):
    """uint8 [P][H][W] pair -> float64 [P][nby * nbx][n // 2 + 1][S][3]: ``_frc_ref.rings_ref`` binned by ring * S + sector."""
    w = F.window(n, name)
    w2 = w[:, None] * w[None, :]
    fa = np.fft.fft2(F.blocks(a, n).astype(np.float64) * w2)
    fb = np.fft.fft2(F.blocks(b, n).astype(np.float64) * w2)
    terms = np.stack([(fa * np.conj(fb)).real, np.abs(fa) ** 2, np.abs(fb) ** 2], axis=-1).astype(np.float64)
    cells, keep = cell_map(n, S)
    return _bin(terms.reshape(terms.shape[:2] + (n * n, 3)), cells, keep, n // 2, S)


def decorr_sectors_ref(a, n, S, name="hann"):
    """uint8 [P][H][W] -> float64 [P][nby * nbx][n // 2 + 1][S][2]: ``_decorr_ref.rings_ref`` binned by ring * S + sector."""
    mod = np.abs(D.spectrum_ref(a, n, name)).astype(np.float64)
    terms = np.stack([mod, mod ** 2], axis=-1)
    cells, keep = cell_map(n, S)
    return _bin(terms.reshape(terms.shape[:2] + (n * n, 2)), cells, keep, n // 2, S)


def _half_cells(n, S):
    """The cells of the kept columns kx <= n / 2, flattened [n * K]."""
    K = n // 2 + 1
    rmap = F.ring_map(n)[:, :K].ravel()
    return rmap * S + sector_map(n, S)[:, :K].ravel(), rmap <= n // 2


def _spectrum_f32(x, n, name):
    ct, st = F.tables(n, name)
    K = n // 2 + 1
    tr, ti = x @ ct[:, :K], x @ st[:, :K]
    fr, fi = ct.T @ tr - st.T @ ti, ct.T @ ti + st.T @ tr
    assert fr.dtype == np.float32 and fi.dtype == np.float32
    return fr, fi


def sectors_f32(a, b, n, S, name="hann"):
    """``_frc_ref.rings_f32`` binned by (ring, sector): float32 products of the kept columns, the interior ones doubled, sums in float64."""
    R, K = n // 2, n // 2 + 1
    (far, fai), (fbr, fbi) = (_spectrum_f32(F.blocks(img, n).astype(np.float32), n, name) for img in (a, b))
    wgt = np.ones(K, dtype=np.float32)
    wgt[1:R] = 2
    terms = np.stack([wgt * (far * fbr + fai * fbi), wgt * (far * far + fai * fai), wgt * (fbr * fbr + fbi * fbi)], axis=-1)
    assert terms.dtype == np.float32
    cells, keep = _half_cells(n, S)
    return _bin(terms.astype(np.float64).reshape(terms.shape[:2] + (n * K, 3)), cells, keep, R, S)


def decorr_sectors_f32(a, n, S, name="hann"):
    """``_decorr_ref.rings_f32`` binned by (ring, sector)."""
    R, K = n // 2, n // 2 + 1
    fr, fi = _spectrum_f32(D.centred(F.blocks(a, n)), n, name)
    p = fr * fr + fi * fi
    m = np.sqrt(p)
    assert p.dtype == np.float32 and m.dtype == np.float32
    wgt = np.ones(K, dtype=np.float32)
    wgt[1:R] = 2
    terms = np.stack([wgt * m, wgt * p], axis=-1).astype(np.float64)
    cells, keep = _half_cells(n, S)
    return _bin(terms.reshape(terms.shape[:2] + (n * K, 2)), cells, keep, R, S)


# ------------------------------------------------------------------------------------------------ errors, in the units of the whole ring
def frc_error(got, ref):
    """max over the cells and the three sums of |S - S_ref| / sqrt(Saa_ref Sbb_ref) of the whole ring ([..., R + 1, S, 3] both): a sector
    can be nearly empty of energy, and float32 round-off is absolute in the ring's scale."""
    assert got.shape == ref.shape
    ring = ref.sum(axis=-2)
    return float((np.abs(got - ref) / F.scale_of(ring)[..., None, None]).max())


def decorr_error(got, ref, n):
    """(err_A, err_P) as ``_decorr_ref.errors``, per cell in the units of the whole ring ([..., R + 1, S, 2] both): |A - A_ref| /
    sqrt(pop[r] P_ref[r]) and |P - P_ref| / P_ref[r] with pop and P_ref of the ring; ring 0 in the units of the whole block."""
    assert got.shape == ref.shape
    worst_a = worst_p = 0.0
    ring = ref.sum(axis=-2)
    for s in range(ref.shape[-2]):
        ea, ep = D.errors(ring + (got[..., s, :] - ref[..., s, :]), ring, n)
        worst_a, worst_p = max(worst_a, ea), max(worst_p, ep)
    return worst_a, worst_p


# ------------------------------------------------------------------------------------------------ step S5 in Python floats
def curve_ref(sums, counts, n, threshold=1 / 7, smooth=0, pixel_size=1.0):
    """Step S5 for one sector: sums [..., R + 1, 3] (every leading axis pooled) and the sector's populations counts [R + 1] ->
    (curve with NaN in unpopulated cells, r_star or None, resolution, crossed)."""
    R = n // 2
    pooled = np.asarray(sums, dtype=np.float64).reshape(-1, R + 1, 3).sum(axis=0)
    curve, populated = [], []
    for r in range(R + 1):
        lo, hi = (r, r) if r == 0 else (max(1, r - smooth), min(R, r + smooth))
        populated.append(int(sum(int(counts[i]) for i in range(lo, hi + 1))) > 0)
        sab, saa, sbb = (float(pooled[lo:hi + 1, k].sum()) for k in range(3))
        curve.append(math.nan if not populated[r] else (sab / math.sqrt(saa * sbb) if saa * sbb > 0 else 0.0))
    prev = 0 if populated[0] else None
    for r in range(1, R + 1):
        if not populated[r]:
            continue
        if curve[r] < threshold:
            if prev is None or curve[prev] < threshold:          # ring 0 below the threshold too, or no populated ring before
                r_star = 1.0
            else:
                r_star = prev + (curve[prev] - threshold) / (curve[prev] - curve[r]) * (r - prev)
            return np.array(curve), r_star, (pixel_size * n / r_star if r_star > 0 else math.inf), True
        prev = r
    return np.array(curve), None, 2.0 * pixel_size, False


def decorr_resolve_ref(sums, counts, n, filters=10, pixel_size=1.0):
    """Step S6 for one sector: ``_decorr_ref.resolve_ref`` with M(r) from the sector's populations counts [R + 1]."""
    R = n // 2
    flat = np.asarray(sums, dtype=np.float64).reshape(-1, R + 1, 2)
    A = [math.fsum(flat[:, r, 0]) for r in range(R + 1)]
    P = [math.fsum(flat[:, r, 1]) for r in range(R + 1)]
    M = [0.0] * (R + 1)
    for r in range(1, R + 1):
        M[r] = M[r - 1] + flat.shape[0] * float(counts[r])
    curves = [D.curve_ref(A, P, M, [1.0] * (R + 1))]
    peaks = [D.peak_ref(curves[0])]
    for s in D.family_ref(R, peaks[0][0] if peaks[0] else None, filters):
        curves.append(D.curve_ref(A, P, M, [1.0 - math.exp(-2.0 * s * s * (r / R) ** 2) for r in range(R + 1)]))
        peaks.append(D.peak_ref(curves[-1]))
    chosen = None
    for k, pk in enumerate(peaks):
        if pk is not None and (chosen is None or pk[1] > peaks[chosen][1]):
            chosen = k
    if chosen is None:
        return dict(curves=np.array(curves), found=False, resolution=2.0 * pixel_size, peak=math.nan, amplitude=0.0)
    return dict(curves=np.array(curves), found=True, resolution=pixel_size * n / peaks[chosen][1], peak=peaks[chosen][1], amplitude=peaks[chosen][2])


# ------------------------------------------------------------------------------------------------ inputs
def planted_aniso(n, rx, ry, seed):
    """``_frc_ref.planted_pair`` with the low-pass region (fy / ry)^2 + (fx / rx)^2 <= 1: detail down to n / rx pixels along x, n / ry along y."""
    rng = np.random.default_rng(seed)
    f = np.arange(n, dtype=np.int64)
    f = np.where(f <= n // 2, f, f - n).astype(np.float64)
    spec = np.fft.fft2(rng.standard_normal((n, n)))
    spec[(f[:, None] / ry) ** 2 + (f[None, :] / rx) ** 2 > 1] = 0
    low = np.fft.ifft2(spec).real
    low = 128 + 40 * (low - low.mean()) / low.std()
    return tuple(np.clip(np.rint(low + 6 * rng.standard_normal((n, n))), 0, 255).astype(np.uint8) for _ in range(2))


def blurred_aniso(n, sigma_x, sigma_y, seed):
    """``_decorr_ref.blurred`` with a Gaussian of ``sigma_x`` pixels along x and ``sigma_y`` along y."""
    rng = np.random.default_rng(seed)
    f = np.fft.fftfreq(n)
    transfer = np.exp(-2.0 * np.pi ** 2 * ((sigma_y * f[:, None]) ** 2 + (sigma_x * f[None, :]) ** 2))
    low = np.fft.ifft2(np.fft.fft2(rng.standard_normal((n, n))) * transfer).real
    low = 128 + 40 * (low - low.mean()) / low.std()
    return np.clip(np.rint(low + 6 * rng.standard_normal((n, n))), 0, 255).astype(np.uint8)


ANISO = ((64, 20, 8), (128, 40, 16), (250, 60, 25))     # (n, rx, ry) of the recovery tests, seeds 0 - 2
DECORR_SCENE = (128, 1.0, 3.0, 3)                      # blurred_aniso's arguments for the decorrelation ordering test

# ------------------------------------------------------------------------------------------------ the GPU tests' bound
SUMS_SIZES = F.SUMS_SIZES
SUMS_SECTORS = (2, 3, 4, 8, 16)
BIG = ((500, 2), (1024, 4))                             # (n, S), once each
MARGIN = F.MARGIN                                       # for the reason given in _frc_ref.py


def sums_inputs(n):
    """``(a, b, window)``, a, b uint8 [1][n][n], of the accuracy tests at block side n: white noise, the isotropic planted pair and
    planted_aniso(n, n // 3, n // 8, 7), all under both windows; the two large sizes once each (500: the anisotropic pair under the Hann
    window; 1024: noise, no window)."""
    rng = np.random.default_rng(2000 + n)
    noise = rng.integers(0, 256, size=(2, 1, n, n), dtype=np.uint8)
    qa, qb = planted_aniso(n, n // 3, n // 8, 7)
    if n == 500:
        return [(qa[None], qb[None], "hann")]
    if n == 1024:
        return [(noise[0], noise[1], "none")]
    pa, pb = F.planted_pair(n, n // 5, 7)
    return [(x, y, name) for name in F.WINDOWS for x, y in ((noise[0], noise[1]), (pa[None], pb[None]), (qa[None], qb[None]))]


def sectors_of(n):
    return tuple(S for m, S in BIG if m == n) or SUMS_SECTORS


def f32_error(n):
    """The measurement behind F32_ERROR[n] and DECORR_F32_ERROR[n]: the worst of ``frc_error`` / ``decorr_error`` of the float32 numpy
    restatement over ``sums_inputs(n)`` and ``sectors_of(n)``."""
    worst, worst_a, worst_p = 0.0, 0.0, 0.0
    for a, b, name in sums_inputs(n):
        for S in sectors_of(n):
            worst = max(worst, frc_error(sectors_f32(a, b, n, S, name), sectors_ref(a, b, n, S, name)))
            ea, ep = decorr_error(decorr_sectors_f32(a, n, S, name), decorr_sectors_ref(a, n, S, name), n)
            worst_a, worst_p = max(worst_a, ea), max(worst_p, ep)
    return worst, (worst_a, worst_p)


# measured on the CPU (tests/test_sector_host.py prints them again and checks that they still hold)
F32_ERROR = {16: 1.907e-06, 18: 1.139e-06, 30: 1.334e-06, 34: 1.399e-06, 64: 1.764e-06, 66: 6.703e-06, 130: 8.877e-06, 500: 1.298e-05,
             1024: 4.643e-05}
DECORR_F32_ERROR = {16: (1.869e-07, 4.811e-07), 18: (3.304e-07, 5.148e-07), 30: (2.796e-07, 7.005e-07), 34: (1.727e-07, 4.673e-07),
                    64: (2.690e-07, 5.483e-07), 66: (2.440e-07, 5.081e-07), 130: (5.960e-07, 1.233e-06), 500: (1.536e-07, 3.542e-07),
                    1024: (4.375e-07, 1.028e-06)}


def tol(n):
    return MARGIN * F32_ERROR[n]


def decorr_tol(n):
    return MARGIN * DECORR_F32_ERROR[n][0], MARGIN * DECORR_F32_ERROR[n][1]
