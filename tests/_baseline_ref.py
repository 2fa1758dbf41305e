"""numpy int64 restatement of the classical baselines (include/pssr_mi355.h, B1 and B2): Pillow's 8-bit bilinear / bicubic enlargement
and the integer non-local means, with plain loops over taps and offsets and whole planes per step.  The device kernels, the host
tests and the committed Pillow fixture are all compared with this file by ``==``."""
import math

import numpy as np

PRECISION_BITS = 22
FILTERS = ("bilinear", "bicubic")


def _bilinear(a):
    a = abs(a)
    return 1.0 - a if a < 1.0 else 0.0


def _bicubic(a):
    A = -0.5
    a = abs(a)
    if a < 1.0:
        return ((A + 2.0) * a - (A + 3.0)) * a * a + 1
    if a < 2.0:
        return (((a - 5) * a + 8) * a - 4) * A
    return 0.0


_FILTER = {"bilinear": (_bilinear, 1.0), "bicubic": (_bicubic, 2.0)}


def taps(in_size, out_size, filter):
    """Pillow's precompute_coeffs + normalize_coeffs_8bpc: per output index ``(xmin, [k...])``, Python floats are C doubles."""
    f, S = _FILTER[filter]
    scale = in_size / out_size
    filterscale = max(scale, 1.0)
    support = S * filterscale
    ss = 1.0 / filterscale
    out = []
    for xx in range(out_size):
        center = (xx + 0.5) * scale
        xmin = max(int(center - support + 0.5), 0)
        xmax = min(int(center + support + 0.5), in_size)
        w = [f((x + xmin - center + 0.5) * ss) for x in range(xmax - xmin)]
        ww = 0.0
        for v in w:
            ww += v
        if ww != 0.0:
            w = [v / ww for v in w]
        out.append((xmin, [int(-0.5 + v * (1 << PRECISION_BITS)) if v < 0 else int(0.5 + v * (1 << PRECISION_BITS)) for v in w]))
    return out


def _pass(x, out_size, filter):
    """One pass along the last axis of an int64 array of 0 .. 255 values -> int64 of 0 .. 255."""
    out = np.empty(x.shape[:-1] + (out_size,), dtype=np.int64)
    for xx, (xmin, k) in enumerate(taps(x.shape[-1], out_size, filter)):
        acc = np.full(x.shape[:-1], 1 << (PRECISION_BITS - 1), dtype=np.int64)
        for i, kk in enumerate(k):
            acc += kk * x[..., xmin + i]
        out[..., xx] = np.clip(acc >> PRECISION_BITS, 0, 255)
    return out


def upsample(x, r, filter):
    """B1: uint8 [..., h, w] -> uint8 [..., h r, w r]: the x pass into a uint8 intermediate, then the y pass."""
    x = np.asarray(x)
    assert x.dtype == np.uint8 and x.ndim >= 2
    mid = _pass(x.astype(np.int64), x.shape[-1] * r, filter)
    out = _pass(np.swapaxes(mid, -1, -2), x.shape[-2] * r, filter)
    return np.swapaxes(out, -1, -2).astype(np.uint8)


def nlm_lut():
    """LUT[q] = rint(16383 exp(-(q + 0.5) / 32)), LUT[255] = 0."""
    return np.array([int(np.rint(16383.0 * math.exp(-(q + 0.5) / 32.0))) if q < 255 else 0 for q in range(256)], dtype=np.int64)


def nlm_params(h, sigma, P):
    """``(qmul, qshift, bias)`` of B2 from the strength ``h`` and the noise level ``sigma`` (grey levels) for ``P x P`` patches."""
    bias = int(np.rint(2.0 * P * P * sigma * sigma))
    for qshift in range(31, -1, -1):
        qmul = int(np.rint(32.0 * 2.0 ** qshift / (P * P * h * h)))
        if qmul <= 1023:
            break
    if qmul < 1:
        raise ValueError(f"h = {h} is too large for {P} x {P} patches")
    return qmul, qshift, bias


def nlm_multi(x, p, s, params):
    """B2 for several ``(qmul, qshift, bias)`` at once (the patch distances do not depend on them): uint8 [..., H, W] -> a list of
    ``(uint8 of the same shape, peak)``, ``peak`` the largest ssd, ssd * qmul and numerator met, for the uint32 bounds.  One
    vectorised step per offset and patch pixel on the plane padded by edge replication, which is the clamping of every coordinate on
    its own: T[u][v] = X[cy(u)][cx(v)]."""
    x = np.asarray(x)
    assert x.dtype == np.uint8 and x.ndim >= 2
    H, W = x.shape[-2:]
    lut = nlm_lut()
    m = s + p
    T = np.pad(x.astype(np.int64), [(0, 0)] * (x.ndim - 2) + [(m, m), (m, m)], mode="edge")

    def at(oy, ox):                  # the plane moved by (oy, ox): X[cy(y + oy)][cx(x + ox)]
        return T[..., m + oy:m + oy + H, m + ox:m + ox + W]

    ys, xs = np.arange(H), np.arange(W)
    acc = [[np.zeros(x.shape, dtype=np.int64), np.zeros(x.shape, dtype=np.int64), {"ssd": 0, "ssd_qmul": 0, "num": 0}] for _ in params]
    for dy in range(-s, s + 1):
        for dx in range(-s, s + 1):
            inside = ((ys + dy >= 0) & (ys + dy < H))[:, None] & ((xs + dx >= 0) & (xs + dx < W))[None, :]
            ssd = np.zeros(x.shape, dtype=np.int64)
            for py in range(-p, p + 1):
                for px in range(-p, p + 1):
                    ssd += (at(py, px) - at(dy + py, dx + px)) ** 2
            v = at(dy, dx)
            for (qmul, qshift, bias), (num, den, peak) in zip(params, acc):
                d = np.maximum(ssd - bias, 0)
                q = np.minimum((d * qmul) >> qshift, 255)
                wgt = np.where(inside, lut[q], 0)
                num += wgt * v
                den += wgt
                peak["ssd"] = max(peak["ssd"], int(ssd.max()))
                peak["ssd_qmul"] = max(peak["ssd_qmul"], int(d.max()) * qmul)
    out = []
    for num, den, peak in acc:
        peak["num"] = int((num + (den >> 1)).max())
        out.append((((num + (den >> 1)) // den).astype(np.uint8), peak))
    return out


def nlm(x, p, s, qmul, qshift, bias):
    """B2 for one set of parameters: ``(out, peak)``."""
    return nlm_multi(x, p, s, [(qmul, qshift, bias)])[0]


def nlm_denoise(x, *, h, sigma=0.0, patch_radius=2, search_radius=7):
    """``nlm`` with the parameters worked out from ``h`` and ``sigma`` as ``util.nlm_denoise`` does."""
    return nlm(x, patch_radius, search_radius, *nlm_params(h, sigma, 2 * patch_radius + 1))[0]


def nlm_scalar(x, p, s, qmul, qshift, bias):
    """B2 for one small plane [H, W] with a quadruple loop of Python ints: the check of ``nlm`` itself."""
    H, W = x.shape
    lut = [int(v) for v in nlm_lut()]
    X = [[int(v) for v in row] for row in x]
    cy = lambda v: min(max(v, 0), H - 1)       # noqa: E731
    cx = lambda v: min(max(v, 0), W - 1)       # noqa: E731
    out = np.zeros((H, W), dtype=np.uint8)
    for y in range(H):
        for xx in range(W):
            num = den = 0
            for dy in range(-s, s + 1):
                for dx in range(-s, s + 1):
                    if not (0 <= y + dy < H and 0 <= xx + dx < W):
                        continue
                    ssd = sum((X[cy(y + py)][cx(xx + px)] - X[cy(y + dy + py)][cx(xx + dx + px)]) ** 2
                              for py in range(-p, p + 1) for px in range(-p, p + 1))
                    wgt = lut[min((max(ssd - bias, 0) * qmul) >> qshift, 255)]
                    num += wgt * X[y + dy][xx + dx]
                    den += wgt
            out[y, xx] = (num + (den >> 1)) // den
    return out


# ---------------------------------------------------------------------------------------------- shared inputs
PIL_CASES = ((5, 7, 4), (16, 16, 2), (3, 40, 3), (33, 17, 5), (1, 9, 4), (64, 64, 4))      # (h, w, r) of the fixture's random cases


def checkerboard(h, w, lo=0, hi=255):
    yy, xx = np.mgrid[:h, :w]
    return np.where((yy + xx) & 1, hi, lo).astype(np.uint8)


def block_image(noise_sigma=20.0):
    """The sanity case of the denoiser: a 48 x 48 plane of 8 x 8 constant blocks and the same with Gaussian noise -> (clean, noisy)."""
    rng = np.random.default_rng(3)
    clean = np.kron(rng.integers(40, 216, (6, 6)), np.ones((8, 8), dtype=np.int64)).astype(np.float64)
    noisy = np.clip(np.rint(clean + rng.normal(0.0, noise_sigma, clean.shape)), 0, 255).astype(np.uint8)
    return clean.astype(np.uint8), noisy


def psnr(a, b):
    err = np.mean((np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)) ** 2)
    return 10.0 * math.log10(255.0 ** 2 / err) if err > 0 else float("inf")
