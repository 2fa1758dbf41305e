"""The Fourier-ring-correlation definitions (include/pssr_mi355.h: "Fourier ring correlation") restated in numpy, from the definitions and
not from the kernel: the tables, the ring index (two forms), the ring sums through numpy's float64 FFT (``rings_ref``) and through the two
matrix products in float32 (``rings_f32``: the yardstick for round-off, not the code under test), the curve and the crossing, and the
planted inputs of the tests."""
import math

import numpy as np

WINDOWS = ("hann", "none")


def window(n, name):
    x = np.arange(n, dtype=np.float64)
    return np.sin(np.pi * (x + 0.5) / n) ** 2 if name == "hann" else np.ones(n)


def tables64(n, name):
    """(Ct, St) of step 1 in float64: W = Ct + i St is the window times the DFT matrix."""
    x = np.arange(n, dtype=np.int64)
    m = (x[:, None] * x[None, :]) % n
    angle = 2.0 * np.pi * m / n
    w = window(n, name)[:, None]
    return w * np.cos(angle), -w * np.sin(angle)


def tables(n, name):
    ct, st = tables64(n, name)
    return ct.astype(np.float32), st.astype(np.float32)


def ring_isqrt(fy, kx):
    return (math.isqrt(4 * (fy * fy + kx * kx)) + 1) // 2


def ring_floor(fy, kx):
    return int(math.floor(math.sqrt(fy * fy + kx * kx) + 0.5))


def ring_map(n):
    """int64 [n][n]: the ring of every coefficient of the full spectrum (fx signed like fy); values above n // 2 are dropped."""
    f = np.arange(n, dtype=np.int64)
    f = np.where(f <= n // 2, f, f - n)
    q = f[:, None] ** 2 + f[None, :] ** 2
    r = np.floor(np.sqrt(q.astype(np.float64)) + 0.5).astype(np.int64)      # exact: q < 2^21, and test_frc_host checks it against isqrt
    return r


def grid(H, W, n):
    """(nby, nbx, oy, ox) of the centred grid of blocks."""
    nby, nbx = H // n, W // n
    return nby, nbx, (H - nby * n) // 2, (W - nbx * n) // 2


def blocks(planes, n):
    """uint8 [P][H][W] -> [P][nby * nbx][n][n], the blocks of the centred grid in row-major order."""
    planes = np.asarray(planes)
    P, H, W = planes.shape
    nby, nbx, oy, ox = grid(H, W, n)
    cut = planes[:, oy:oy + nby * n, ox:ox + nbx * n].reshape(P, nby, n, nbx, n)
    return cut.transpose(0, 1, 3, 2, 4).reshape(P, nby * nbx, n, n)


def _ring_sums(fa, fb, n):
    """[..., n, n] complex full spectra -> float64 [..., n // 2 + 1, 3] (Sab, Saa, Sbb)."""
    R = n // 2
    rmap = ring_map(n).ravel()
    keep = rmap <= R
    terms = np.stack([(fa * np.conj(fb)).real, np.abs(fa) ** 2, np.abs(fb) ** 2], axis=-1).astype(np.float64)
    terms = terms.reshape(terms.shape[:-3] + (n * n, 3))
    out = np.zeros(terms.shape[:-2] + (R + 1, 3), dtype=np.float64)
    flat, oflat = terms.reshape(-1, n * n, 3), out.reshape(-1, R + 1, 3)
    for i in range(flat.shape[0]):
        for k in range(3):
            oflat[i, :, k] = np.bincount(rmap[keep], weights=flat[i, keep, k], minlength=R + 1)
    return out


def rings_ref(a, b, n, name="hann"):
    """uint8 [P][H][W] pair -> float64 [P][nby * nbx][n // 2 + 1][3]: numpy's float64 fft2 of block x (w (x) w), full spectrum."""
    w = window(n, name)
    w2 = w[:, None] * w[None, :]
    fa = np.fft.fft2(blocks(a, n).astype(np.float64) * w2)
    fb = np.fft.fft2(blocks(b, n).astype(np.float64) * w2)
    return _ring_sums(fa, fb, n)


def transform_tables64(block, n, name):
    """W^T a W in float64 through the tables: what fft2 of the windowed block is."""
    ct, st = tables64(n, name)
    wm = ct + 1j * st
    return wm.T @ block.astype(np.float64) @ wm


def rings_f32(a, b, n, name="hann"):
    """The same sums through the two matrix products in numpy float32 against the float32 tables (the kept columns, the interior ones
    doubled), products in float32 and sums in float64: how far float32 transforms lie from ``rings_ref``."""
    ct, st = tables(n, name)
    R, K = n // 2, n // 2 + 1
    spectra = []
    for img in (a, b):
        x = blocks(img, n).astype(np.float32)
        tr, ti = x @ ct[:, :K], x @ st[:, :K]                                   # T = a (Ct + i St)[:, :K]
        fr = ct.T @ tr - st.T @ ti                                               # F = (Ct + i St)^T T
        fi = ct.T @ ti + st.T @ tr
        assert fr.dtype == np.float32 and fi.dtype == np.float32
        spectra.append((fr, fi))
    (far, fai), (fbr, fbi) = spectra
    wgt = np.ones(K, dtype=np.float32)
    wgt[1:R] = 2
    terms = np.stack([wgt * (far * fbr + fai * fbi), wgt * (far * far + fai * fai), wgt * (fbr * fbr + fbi * fbi)], axis=-1)
    assert terms.dtype == np.float32
    rmap = ring_map(n)[:, :K].ravel()
    keep = rmap <= R
    flat = terms.astype(np.float64).reshape(-1, n * K, 3)
    out = np.zeros((flat.shape[0], R + 1, 3), dtype=np.float64)
    for i in range(flat.shape[0]):
        for k in range(3):
            out[i, :, k] = np.bincount(rmap[keep], weights=flat[i, keep, k], minlength=R + 1)
    return out.reshape(terms.shape[:2] + (R + 1, 3))


def scale_of(ref):
    """sqrt(Saa Sbb) of ``rings_ref``'s sums, [..., R + 1]: what the bound on every one of the three sums is measured in."""
    return np.sqrt(ref[..., 1] * ref[..., 2])


def curve_ref(sums, n, threshold=1 / 7, smooth=0, pixel_size=1.0):
    """Step 5: (curve, r_star or None, resolution, crossed) of one item from sums [..., R + 1, 3], every leading axis pooled."""
    R = n // 2
    pooled = np.asarray(sums, dtype=np.float64).reshape(-1, R + 1, 3).sum(axis=0)
    curve = []
    for r in range(R + 1):
        lo, hi = (r, r) if r == 0 else (max(1, r - smooth), min(R, r + smooth))
        sab, saa, sbb = (float(pooled[lo:hi + 1, k].sum()) for k in range(3))
        curve.append(sab / math.sqrt(saa * sbb) if saa * sbb > 0 else 0.0)
    for r in range(1, R + 1):
        if curve[r] < threshold:
            if curve[r - 1] < threshold:               # only r == 1: ring 0 itself lies below
                r_star = 1.0
            else:
                r_star = (r - 1) + (curve[r - 1] - threshold) / (curve[r - 1] - curve[r])
            return np.array(curve), r_star, (pixel_size * n / r_star if r_star > 0 else math.inf), True
    return np.array(curve), None, 2.0 * pixel_size, False


def planted_pair(n, r0, seed):
    """Two uint8 [n][n] images of one low-passed field with independent noise: L is Gaussian noise low-passed to the rings <= r0 in the
    Fourier domain, scaled to standard deviation 40 around 128; a, b = clip(rint(L + e)), e independent Gaussian noise of sigma 6."""
    rng = np.random.default_rng(seed)
    spec = np.fft.fft2(rng.standard_normal((n, n)))
    spec[ring_map(n) > r0] = 0
    low = np.fft.ifft2(spec).real
    low = 128 + 40 * (low - low.mean()) / low.std()
    return tuple(np.clip(np.rint(low + 6 * rng.standard_normal((n, n))), 0, 255).astype(np.uint8) for _ in range(2))


# ------------------------------------------------------------------------------------------------ the GPU tests' bound
# max |rings_f32 - rings_ref| / sqrt(Saa_ref Sbb_ref) over all rings, all three sums, both windows and exactly the inputs of
# tests/test_gpu_frc.py (``sums_inputs``), measured on the CPU (tests/test_frc_host.py prints them again and checks that they still hold):
F32_ERROR = {16: 1.634e-06, 18: 1.142e-06, 30: 1.391e-06, 34: 1.331e-06, 64: 3.225e-06, 66: 1.786e-06, 130: 5.769e-06, 500: 1.311e-05,
             1024: 1.478e-04}
MARGIN = 8          # the MFMA's summation order (one ascending chain) is not numpy's blocked one; both grow like a random walk in n
TOL = {n: MARGIN * e for n, e in F32_ERROR.items()}
SUMS_SIZES = (16, 18, 30, 34, 64, 66, 130)
BIG_SIZES = (500, 1024)


def sums_inputs(n):
    """``(a, b, window)`` with a, b uint8 [1][n][n]: what the ring sums are checked on at block side n.  White noise and a planted pair
    (r0 = n // 5), both under both windows; the two large sizes run once each, one plane."""
    rng = np.random.default_rng(1000 + n)
    noise = rng.integers(0, 256, size=(2, 1, n, n), dtype=np.uint8)
    pa, pb = planted_pair(n, n // 5, 7)
    if n == 500:
        return [(pa[None], pb[None], "hann")]
    if n == 1024:
        return [(noise[0], noise[1], "none")]
    return [(x, y, name) for name in WINDOWS for x, y in ((noise[0], noise[1]), (pa[None], pb[None]))]


def f32_error(n):
    """The measurement behind F32_ERROR[n]."""
    worst = 0.0
    for a, b, name in sums_inputs(n):
        ref = rings_ref(a, b, n, name)
        worst = max(worst, float((np.abs(rings_f32(a, b, n, name) - ref) / scale_of(ref)[..., None]).max()))
    return worst
