"""Loss, metrics and small host helpers with the reference's names (pssr/util.py).

``SSIMLoss`` keeps the reference signature and semantics (pssr/util.py:10-52) but runs as two HIP
kernel sweeps over the image pyramid (csrc/loss.hip) instead of ~60 torch ops; the third-party
pytorch_msssim algorithm it stands for is restated in oracle/loss_ref.py.
"""
from __future__ import annotations

import inspect
import math
from collections import namedtuple

import numpy as np
import torch
import torch.nn as nn

from . import ops

MS_WEIGHTS = (0.0448, 0.2856, 0.3001, 0.2363, 0.1333)    # pytorch_msssim default level weights


def _gauss_1d(size: int, sigma: float):
    coords = torch.arange(size, dtype=torch.float) - size // 2
    g = torch.exp(-(coords ** 2) / (2 * sigma ** 2))
    return (g / g.sum()).tolist()


_CONST_CACHE = {}      # small per-shape device constants (kept out of hipGraph capture)


class _SSIMLossFunction(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, y, cfg, in_div=1.0):
        """in_div != 1: the loss of (x / in_div, y / in_div) with the divisions done inside the training kernels (11-tap window, x needing a
        gradient); the returned gradient is wrt the undivided x."""
        if not x.is_cuda:
            raise RuntimeError("pssr2_amd.SSIMLoss runs on an MI355X (HIP) device only; there is no CPU fallback")
        win, mix, ms, k1, k2, data_range, lvl_w = cfg
        x = x.detach().contiguous().float()
        y = y.detach().contiguous().float()
        n, c, h, w = x.shape
        planes, k = n * c, len(win)
        levels = len(lvl_w) if ms else 1
        if ms and min(h, w) <= (k - 1) * 2 ** 4:
            raise AssertionError(f"Image size should be larger than {(k - 1) * 2 ** 4} due to the 4 downsamplings in ms-ssim")
        c1, c2 = (k1 * data_range) ** 2, (k2 * data_range) ** 2
        dev = x.device
        fused_div = in_div != 1.0 and k == 11 and ctx.needs_input_grad[0]
        if in_div != 1.0 and not fused_div:             # the plain kernels take the quotients as tensors
            x, y = x / in_div, y / in_div
        div0 = in_div if fused_div else 1.0
        xs, ys, dims = [x], [y], [(h, w)]
        for lv in range(1, levels):
            hh, ww = dims[-1]
            ho, wo = (hh + 2 * (hh & 1) - 2) // 2 + 1, (ww + 2 * (ww & 1) - 2) // 2 + 1
            xo = torch.empty(planes, ho, wo, device=dev)
            yo = torch.empty(planes, ho, wo, device=dev)
            ops.avgpool2_pair(xs[-1], ys[-1], xo, yo, planes, hh, ww, div0 if lv == 1 else 1.0)
            xs.append(xo), ys.append(yo), dims.append((ho, wo))
        # training with the default 11-tap window: keep the per-position derivatives for the backward pass (ops.ssim_level_fwd_adj);
        # that kernel spreads its sums over `stripes` copies, folded by msssim_weights_striped
        adjs = None
        if k == 11 and ctx.needs_input_grad[0]:
            adjs = [torch.empty(planes * 3 * hh * ww, device=dev) for hh, ww in dims]
        stripes = 16 if adjs is not None else 1
        sstride = levels * planes * 2 + 2
        rows = 2 * stripes if stripes > 1 else 1        # the striped kernel adds every sum as two exact pieces (order-independent)
        sums = torch.zeros(rows * sstride + (sstride if stripes > 1 else 0), dtype=torch.float64, device=dev)      # (+ the folded copy)
        l1_sum = sums[sstride - 2:sstride - 1] if mix < 1 else None
        for l in range(levels):
            hh, ww = dims[l]
            if adjs is not None:
                ops.ssim_level_fwd_adj(xs[l], ys[l], planes, hh, ww, win, c1, c2, l == levels - 1, sums[l * planes * 2:],
                                       l1_sum if l == 0 else None, stripes, sstride, adjs[l], div0 if l == 0 else 1.0)
            else:
                ops.ssim_level_fwd(xs[l], ys[l], planes, hh, ww, win, c1, c2, sums[l * planes * 2:], l1_sum if l == 0 else None)
        ckey = (tuple(dims), k, tuple(lvl_w) if ms else (1.0,), str(dev))
        cached = _CONST_CACHE.get(ckey)
        if cached is None:
            cached = _CONST_CACHE[ckey] = (
                torch.tensor([float((hh - k + 1) * (ww - k + 1)) for hh, ww in dims], dtype=torch.float64, device=dev),
                torch.tensor(list(lvl_w) if ms else [1.0], dtype=torch.float32, device=dev))
        nvalid, lw = cached
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        wts = torch.empty(levels * planes, dtype=torch.float32, device=dev)
        l1c = torch.empty(1, dtype=torch.float32, device=dev)
        if stripes > 1:
            ops.msssim_weights_striped(sums, stripes, sstride, sums[rows * sstride:], levels, planes, nvalid, lw, ms, mix, l1_sum, float(x.numel()),
                                       None, loss, wts, l1c)
            sums = sums[rows * sstride:]                          # the folded copy: what backward's weights pass reads
            l1_sum = sums[levels * planes * 2:levels * planes * 2 + 1] if l1_sum is not None else None
        else:
            ops.msssim_weights(sums, levels, planes, nvalid, lw, ms, mix, l1_sum, float(x.numel()), None, loss, wts, l1c)
        ctx.saved = (xs, ys, dims, sums, nvalid, lw, l1_sum, cfg, planes, x.shape, adjs, div0, in_div if not fused_div else 1.0)
        return loss[0]

    @staticmethod
    def backward(ctx, grad_out):
        xs, ys, dims, sums, nvalid, lw, l1_sum, cfg, planes, shape, adjs, div0, post_div = ctx.saved
        win, mix, ms, k1, k2, data_range, lvl_w = cfg
        levels = len(xs)
        dev = xs[0].device
        c1, c2 = (k1 * data_range) ** 2, (k2 * data_range) ** 2
        go = grad_out.detach().float().reshape(1).contiguous()
        loss = torch.empty(1, dtype=torch.float32, device=dev)
        wts = torch.empty(levels * planes, dtype=torch.float32, device=dev)
        l1c = torch.empty(1, dtype=torch.float32, device=dev)
        ops.msssim_weights(sums, levels, planes, nvalid, lw, ms, mix, l1_sum, float(xs[0].numel()), go, loss, wts, l1c)
        dcoarse, hc, wc = None, 0, 0
        for l in range(levels - 1, -1, -1):
            hh, ww = dims[l]
            dx = torch.empty(planes, hh, ww, device=dev)
            use_ssim = (l == levels - 1)
            l1_arg = l1c if (l == 0 and l1_sum is not None) else None
            if adjs is not None:
                ops.ssim_level_bwd_adj(xs[l], ys[l], adjs[l], planes, hh, ww, win, wts[l * planes:], dcoarse, hc, wc, l1_arg, dx,
                                       div0 if l == 0 else 1.0)
            else:
                ops.ssim_level_bwd(xs[l], ys[l], planes, hh, ww, win, c1, c2, wts[l * planes:], use_ssim, dcoarse, hc, wc, l1_arg, dx)
            dcoarse, hc, wc = dx, hh, ww
        g = dcoarse.view(shape)
        if post_div != 1.0:
            g = g / post_div
        return g, None, None, None


class SSIMLoss(nn.Module):
    def __init__(self, channels: int = 1, mix: float = .8, win_size: int = 11, win_sigma: float = 1.5, ms: bool = True, kwargs=None):
        r"""SSIM / MS-SSIM loss mixed with a Gaussian-weighted L1 term (Zhao et al., 2018), reference
        signature (pssr/util.py:11).  ``kwargs`` accepts the pytorch_msssim options ``K`` and
        ``weights``.  For ``channels > 1`` the L1 window is depthwise (the reference's [1,1,k,k]
        window raises in torch for C > 1).
        """
        super().__init__()
        kwargs = {} if kwargs is None else dict(kwargs)
        if win_size % 2 != 1:
            raise ValueError("Window size should be odd.")
        self.K = tuple(kwargs.pop("K", (0.01, 0.03)))
        self.weights = tuple(kwargs.pop("weights", None) or MS_WEIGHTS)
        if kwargs:
            raise TypeError(f"unsupported pytorch_msssim options on the MI355X path: {sorted(kwargs)}")
        self.win = _gauss_1d(win_size, win_sigma)
        self.channels, self.win_size, self.mix, self.ms = channels, win_size, mix, ms

    def forward(self, input, target):
        if input.shape != target.shape:
            raise ValueError(f"Input images should have the same dimensions, but got {input.shape} and {target.shape}.")
        cfg = (self.win, float(self.mix), bool(self.ms), self.K[0], self.K[1], 1.0, self.weights)
        return _SSIMLossFunction.apply(input, target, cfg)

    def forward_divided(self, input, target, divisor: float):
        """``self(input / divisor, target / divisor)`` -- what pssr/train.py:101 computes with divisor 255 -- without the two quotient
        tensors and the gradient's division pass: the training kernels scale on load (a rounded multiplication by the f32 reciprocal 1/in_div, which is how torch divides a device tensor by a scalar: same values)."""
        if input.shape != target.shape:
            raise ValueError(f"Input images should have the same dimensions, but got {input.shape} and {target.shape}.")
        cfg = (self.win, float(self.mix), bool(self.ms), self.K[0], self.K[1], 1.0, self.weights)
        return _SSIMLossFunction.apply(input, target, cfg, float(divisor))


class _FnCtx:
    """Stand-in autograd context: lets a Function drive another Function's forward / backward inside its own node."""

    def __init__(self, needs_input_grad):
        self.needs_input_grad = needs_input_grad


class _CrappifierLossFunction(torch.autograd.Function):
    """``_crappifier_loss`` (pssr/train.py:388-402) as one autograd node over HIP kernels, gradient wrt ``lr_hat`` only:
    pred = clamp?(lr_hat) - ds_hr, target = lr - ds_hr (pssr_crappifier_profiles); both GradHist histograms in one launch;
    D = mean((H(pred) - H(target))^2) / W_lr^2 and L = D * P (pssr_crappifier_loss_combine) with P = SSIMLoss(pred, target) through
    _SSIMLossFunction's kernels.  Backward: the SSIM backward with grad_out = D * dL, then the histogram backward ADDS
    P * dL * dD/dpred into the same buffer (its dL/dh = 2 (p - t) / (B bins W^2) is formed in the kernel) and masks it where the
    clamp cut."""

    @staticmethod
    def forward(ctx, lr, lr_hat, ds_hr, hist_cfg, ssim_cfg, clamp=False):
        if not (lr.is_cuda and lr_hat.is_cuda and ds_hr.is_cuda):
            raise RuntimeError("pssr2_amd crappifier loss runs on an MI355X (HIP) device only; there is no CPU fallback")
        if not (lr.shape == lr_hat.shape == ds_hr.shape):
            raise ValueError(f"lr, lr_hat and ds_hr must have one shape, got {tuple(lr.shape)}, {tuple(lr_hat.shape)}, {tuple(ds_hr.shape)}")
        lr, lr_hat, ds_hr = (t.detach().contiguous().float() for t in (lr, lr_hat, ds_hr))
        bins, lo, hi, sigma = hist_cfg
        pred, target = torch.empty_like(lr_hat), torch.empty_like(lr)
        ops.crappifier_profiles(lr_hat, lr, ds_hr, pred, target, clamp)
        hp, ht = ops.gradhist_fwd([(pred, None), (target, None)], bins, lo, hi, sigma)
        sctx = _FnCtx((ctx.needs_input_grad[1], False, False, False))
        p_loss = _SSIMLossFunction.forward(sctx, pred, target, ssim_cfg)
        parts = torch.empty(3, dtype=torch.float32, device=lr.device)          # [L, D, P]
        batch, w_lr = lr.shape[0], lr.shape[-1]
        ops.crappifier_loss_combine(hp, ht, p_loss, 1.0 / (batch * bins) / (w_lr * w_lr), parts)
        ctx.state = (lr_hat, ds_hr, hp, ht, parts, sctx, hist_cfg, bool(clamp), batch, w_lr)
        return parts[0]

    @staticmethod
    def backward(ctx, grad_out):
        lr_hat, ds_hr, hp, ht, parts, sctx, (bins, lo, hi, sigma), clamp, batch, w_lr = ctx.state
        go = grad_out.detach().float().reshape(1).contiguous()
        sc = torch.empty(2, dtype=torch.float32, device=go.device)             # [D * dL, P * dL]
        ops.crappifier_loss_bwd_scalars(parts, go, sc)
        g = _SSIMLossFunction.backward(sctx, sc[0:1])[0]
        ops.gradhist_bwd(lr_hat, ds_hr, hp, g, bins, lo, hi, sigma, g_ref=ht, dev_scale=sc[1:2], g_scale=2.0 / (batch * bins * w_lr * w_lr),
                         clamp=clamp, accumulate=True)
        return None, g, None, None, None, None


def ssim(X, Y, data_range=255, win_size=11, win_sigma=1.5):
    """Mean SSIM (the in-loop metric of pssr/train.py:109), forward only."""
    cfg = (_gauss_1d(win_size, win_sigma), 1.0, False, 0.01, 0.03, float(data_range), (1.0,))
    with torch.no_grad():
        return 1 - _SSIMLossFunction.apply(X, Y, cfg)


def pixel_metric(mse: float, image_range: int = 255):
    r"""Average pixel error from a mean squared error (pssr/util.py:207-215)."""
    return math.sqrt(mse) * image_range


def _psnr_metric(mse):
    return 20 * torch.log10(1 / torch.sqrt(mse))


def _force_list(item):
    if type(item) is not list:
        try:
            return list(item)
        except TypeError:
            return [item]
    return item


def _get_callbacks(raw):
    """1-argument callbacks receive ``locals()`` of the driver loop (pssr/util.py:228-231)."""
    callbacks = [] if raw is None else _force_list(raw)
    takes_locals = [len([a for a in inspect.getfullargspec(cb).args if a != "self"]) == 1 for cb in callbacks]
    return callbacks, takes_locals


def _patch_images(batched, n_cols, n_rows, overlap, margin):
    """Overlap-averaged stitching of row-major tiles (pssr/util.py:116-137), host numpy."""
    size = batched.shape[-1]
    step = size - overlap
    H, W = n_rows * step + overlap, n_cols * step + overlap
    acc, cnt = np.zeros((H, W)), np.zeros((H, W))
    for idx in range(n_rows * n_cols):
        row, col = divmod(idx, n_cols)
        top = margin if row != 0 else 0
        bot = margin if row != n_rows - 1 else 0
        lef = margin if col != 0 else 0
        rig = margin if col != n_cols - 1 else 0
        r0, c0 = row * step, col * step
        acc[r0 + top:r0 + size - bot, c0 + lef:c0 + size - rig] += batched[idx, top:batched.shape[1] - bot, lef:batched.shape[2] - rig]
        cnt[r0 + top:r0 + size - bot, c0 + lef:c0 + size - rig] += 1
    cnt[cnt == 0] = 1
    return acc / cnt


def normalize_preds(hr, hr_hat, pmin: float = 0.1, pmax: float = 99.9):
    r"""Normalizes prediction image intensities to ground truth for fair benchmarking (pssr/util.py:139-191), on the MI355X
    (csrc/metrics.hip, bit-exact with the reference's numpy arithmetic).  ``hr`` / ``hr_hat``: uint8 arrays or tensors of the
    same shape ``[..., H, W]`` -- what ``test_metrics`` and ``predict_images(norm=True)`` pass -- or with image sizes that differ
    (pssr/util.py:176-179: the covariance is then taken against ``skimage.transform.resize(prediction, ground-truth shape)``, here
    its scikit-image >= 0.19 / scipy.ndimage definition evaluated on the device; each output keeps its own size).  Returns uint8
    numpy arrays like the reference."""
    import numpy as np
    from . import ops
    dev = hr_hat.device if isinstance(hr_hat, torch.Tensor) and hr_hat.is_cuda else (hr.device if isinstance(hr, torch.Tensor) and hr.is_cuda else "cuda")
    a, b = (t if isinstance(t, torch.Tensor) else torch.as_tensor(np.ascontiguousarray(t)) for t in (hr, hr_hat))
    if a.dim() != b.dim():
        raise ValueError(f"hr and hr_hat must have the same number of dimensions. Dimension lengths are {tuple(a.shape)} and {tuple(b.shape)} respectively.")
    if a.dtype != torch.uint8 or b.dtype != torch.uint8:
        raise TypeError("normalize_preds on the MI355X takes uint8 images (the output of _pred_array), as test_metrics passes them")
    if a.dim() < 2:
        raise ValueError("images need at least 2 dimensions")
    if a.shape != b.shape:
        n_a, n_b = a.numel() // (a.shape[-1] * a.shape[-2]), b.numel() // (b.shape[-1] * b.shape[-2])
        if n_a != n_b:
            raise ValueError(f"hr and hr_hat must have the same number of images. Received {n_a} and {n_b} images respectively.")
        a2, b2 = ops.normalize_preds_resized_u8(a.to(dev).reshape(-1, *a.shape[-2:]), b.to(dev).reshape(-1, *b.shape[-2:]), pmin, pmax)
        return a2.reshape(a.shape).cpu().numpy(), b2.reshape(b.shape).cpu().numpy()
    shape = a.shape
    a2, b2 = ops.normalize_preds_u8(a.to(dev).reshape(-1, *shape[-2:]), b.to(dev).reshape(-1, *shape[-2:]), pmin, pmax)
    return a2.reshape(shape).cpu().numpy(), b2.reshape(shape).cpu().numpy()


Consistency = namedtuple("Consistency", "map alpha beta rse rsp")


def _check_fit(fit):
    if fit not in ops.FITS:
        raise ValueError(f"fit must be one of {ops.FITS}. Given {fit!r}.")


def _pearson_terms(n: int, sd: int, sl: int, sdd: int, sdl: int, sll: int):
    """``(num, den, denl, r)`` from the exact sums of ``D``, ``L``, ``D D``, ``D L`` and ``L L`` over ``n`` pixels (Python ints), in exactly
    the expressions of include/pssr_mi355.h: ``n`` times the covariance and the two variances, and the Pearson correlation
    ``num / sqrt(den denl)`` (0 when ``den`` or ``denl`` is 0)."""
    num, den, denl = n * sdl - sd * sl, n * sdd - sd * sd, n * sll - sl * sl
    return num, den, denl, (num / math.sqrt(den * denl) if den > 0 and denl > 0 else 0.0)


def _u8_image_pair(who, hi, lo, names, roles):
    """The front half of the entry points that score an HR-side stack ``hi`` [N, C, s*h, s*w] against an LR-side stack ``lo`` [N, m, h, w]
    (or both 3-D, without the batch axis): uint8 arrays become tensors, host tensors are refused, ``C <= m``, ``s`` an integer in 1 .. 16,
    at most 2**28 pixels per LR plane.  ``names``: the two arguments' names, ``roles``: what an item of each is, with a gap for its frame
    count.  -> ``(hi, lo, batched, scale, device)``, both tensors 4-D and where they were."""
    tensors = []
    for name, t in zip(names, (hi, lo)):
        if not torch.is_tensor(t):
            t = torch.as_tensor(np.ascontiguousarray(t))
        elif not t.is_cuda:
            raise RuntimeError(f"pssr2_amd.util.{who} runs on an MI355X (HIP) device only; there is no CPU fallback")
        if t.dtype != torch.uint8:
            raise TypeError(f"{who} takes uint8 images; {name} is {t.dtype}")
        tensors.append(t)
    hi, lo = tensors
    if hi.dim() != lo.dim() or hi.dim() not in (3, 4):
        raise ValueError(f"{names[0]} and {names[1]} must both be 4-D, [images, frames, height, width], or both 3-D without the batch axis. "
                         f"Shapes are {tuple(hi.shape)} and {tuple(lo.shape)} respectively.")
    batched = hi.dim() == 4
    if not batched:
        hi, lo = hi[None], lo[None]
    (n_img, c, H, W), (n_lo, m, h, w) = hi.shape, lo.shape
    if n_img != n_lo:
        raise ValueError(f"{names[0]} and {names[1]} must have the same number of images. Received {n_img} and {n_lo} images respectively.")
    if c > m:
        raise ValueError(f"{roles[0].format(c)} cannot be matched with {roles[1].format(m)}.")
    scale = H // h if h else 0
    if min(n_img, c, h, w) < 1 or not 1 <= scale <= 16 or H != scale * h or W != scale * w:
        raise ValueError(f"The size of {names[0]} must be one integer multiple (1 to 16) of the size of {names[1]} along both axes. "
                         f"Sizes are {H}x{W} and {h}x{w} respectively.")
    if h * w > 1 << 28:
        raise ValueError(f"A plane of {names[1]} of {h * w} pixels is above the 2**28 up to which the sums are exact.")
    return hi, lo, batched, scale, hi.device if hi.is_cuda else (lo.device if lo.is_cuda else "cuda")


def _consistency_fit(n: int, sums, fit: str):
    """``(alpha, beta, rsp, table)`` of one plane from its five exact sums ``Sd, Sl, Sdd, Sdl, Sll`` over ``n`` pixels (Python ints), in
    exactly the expressions of include/pssr_mi355.h: the least-squares line ``L ~ alpha D + beta`` (or the identity), the Pearson
    correlation of D and L, and the int32 table ``P[d]`` of the expected LR value in 1/256 grey levels (``round`` is half-to-even)."""
    sd, sl, sdd, sdl, sll = (int(v) for v in sums)
    num, den, _, rsp = _pearson_terms(n, sd, sl, sdd, sdl, sll)
    if fit == "identity":
        alpha, beta = 1.0, 0.0
    elif den == 0:
        alpha, beta = 0.0, sl / n
    else:
        alpha = num / den
        beta = (sl - alpha * sd) / n
    table = [min(max(round(256.0 * (alpha * d + beta)), -65536), 131071) for d in range(256)]
    return alpha, beta, rsp, table


RSF = namedtuple("RSF", "sigma fwhm score curve index margin")
RSFConsistency = namedtuple("RSFConsistency", "map alpha beta rse rsp sigma margin")
RSF_POOLS = ("item", "all")                          # estimate_rsf's ``pool``
RSF_SIGMAS = tuple(0.25 * i for i in range(33))      # estimate_rsf's default candidates: 0, 0.25, .. 8 HR pixels (K = 33, R = 24)
_FWHM = 2.0 * math.sqrt(2.0 * math.log(2.0))


def _rsf_choose(n: int, rows, K: int):
    """``(k, curve)`` from the exact sums of the pooled planes (``rows``: one list of ``3 K + 2`` ints per plane, the layout of
    ``pssr_rsf_moments_u8``) over ``n`` pixels in all, in exactly the expressions of include/pssr_mi355.h: the planes' sums add, the score of
    a candidate is the signed squared Pearson correlation ``num |num| / (den denl)`` (0 when ``den`` or ``denl`` is 0), compared by
    cross-multiplying Python ints; ties go to the smaller ``k``.  ``curve``: the Pearson correlation of every candidate."""
    pooled = [sum(int(v) for v in col) for col in zip(*rows)]
    sl, sll = pooled[3 * K], pooled[3 * K + 1]
    best, curve = None, []                              # (p, q, k): the score p / (q denl), q > 0
    for k in range(K):
        sd, sdd, sdl = pooled[3 * k:3 * k + 3]
        num, den, denl, r = _pearson_terms(n, sd, sl, sdd, sdl, sll)
        p, q = (num * abs(num), den) if den > 0 and denl > 0 else (0, 1)
        if best is None or p * best[1] > best[0] * q:
            best = (p, q, k)
        curve.append(r)
    return best[2], curve


def _rsf_sigmas(sigmas, what="sigmas"):
    """The candidate widths as a list of floats: 1 .. 64 finite numbers >= 0 with ``ceil(3 sigma) <= 32``."""
    if sigmas is None:
        return list(RSF_SIGMAS)
    try:
        sig = [float(v) for v in (sigmas.tolist() if hasattr(sigmas, "tolist") else sigmas)]
    except (TypeError, ValueError):
        raise ValueError(f"{what} must be a sequence of numbers. Given {sigmas!r}.") from None
    if not 1 <= len(sig) <= ops.MAX_RSF_CANDIDATES:
        raise ValueError(f"{what} must hold 1 to {ops.MAX_RSF_CANDIDATES} candidates. Given {len(sig)}.")
    if any(not math.isfinite(v) or v < 0 or ops.rsf_radius(v) > ops.MAX_REGISTER_RADIUS for v in sig):
        raise ValueError(f"{what} must be finite, >= 0 and at most {ops.MAX_REGISTER_RADIUS / 3:.2f} HR pixels (ceil(3 sigma) <= "
                         f"{ops.MAX_REGISTER_RADIUS}). Given {sig}.")
    return sig


def _rsf_sums(who, lr, hr_hat, sig):
    """The shared front half of ``estimate_rsf`` and ``consistency_map(rsf=...)``: the checks of the pair, the centre-frame rule, the tap
    table of the candidates ``sig`` and the one sums launch -> ``(hat, frames, batched, scale, taps, R, m, rows)`` with both tensors on the
    device and ``rows`` the sums on the host, one list of ``3 K + 2`` ints per plane.  Every check comes before any device work."""
    hr_hat, lr, batched, scale, dev = _u8_image_pair(who, hr_hat, lr, ("hr_hat", "lr"), ("A prediction of {} planes", "an input of {} frames"))
    c, (h, w) = hr_hat.shape[1], lr.shape[-2:]
    taps, R = ops.rsf_taps(scale, sig)
    m = ops.register_margin(scale, R)
    if h - 2 * m < 1 or w - 2 * m < 1:
        raise ValueError(f"An LR image of {h}x{w} leaves nothing inside the margin of {m} pixels that a largest sigma of {max(sig)} (radius {R}) "
                         f"at scale {scale} needs on every side.")
    if not (hr_hat.is_cuda or lr.is_cuda or torch.cuda.is_available()):
        raise RuntimeError(f"pssr2_amd.util.{who} needs an MI355X (HIP) device, and none is available; there is no CPU fallback")
    from .data import _slice_center
    hat, frames = hr_hat.to(dev).contiguous(), _slice_center(lr.to(dev), c).contiguous()
    return hat, frames, batched, scale, taps, R, m, ops.rsf_moments_u8(hat, frames, taps, R).cpu().tolist()


def estimate_rsf(lr, hr_hat, *, sigmas=None, pool: str = "item", pixel_size: float = 1.0, to_numpy: bool = True):
    r"""Estimates the resolution-scaling function between sharp images and measured ones: the width of the Gaussian blur that, applied
    before this package's forward model (``_gen_pair``'s Pillow-bilinear reduction), makes ``hr_hat`` look most like ``lr``.  ``lr``: uint8
    array or device tensor [N, m, h, w]; ``hr_hat``: uint8 [N, C, s*h, s*w], ``s`` an integer in 1 .. 16 (or both 3-D, without the batch
    axis) -- a prediction and its own input, or a real HR / LR pair (``register_pairs`` first).  Plane ``j`` meets frame ``j`` of the ``C``
    centre frames of ``lr`` (``_slice_center``).  For every candidate ``sigma`` (``sigmas``: 1 .. 64 widths in HR pixels, finite, >= 0,
    ``ceil(3 sigma) <= 32``; ``None``: 0, 0.25, .. 8) the sharp image is blurred and reduced to the LR grid in integer arithmetic and
    correlated with ``lr`` inside a margin of ``m = 1 + ceil(R / s)`` LR pixels, ``R`` the largest ``ceil(3 sigma)``.  The best intensity fit
    ``L ~ alpha D_sigma + beta`` leaves the residual ``(1 - rho**2) var(L)``, so the candidate with the largest signed squared Pearson
    correlation wins (ties: the first) -- one choice per item, its planes pooled, or with ``pool="all"`` one for the whole batch: one sigma
    for one microscope.  include/pssr_mi355.h has the definitions, exact integers throughout.  Returns
    ``RSF(sigma, fwhm, score, curve, index, margin)``:

    * ``sigma``: float64 [N], the chosen width in HR pixels times ``pixel_size``; ``fwhm = 2 sqrt(2 ln 2) sigma``: a resolution figure that
      needs no second image; ``index``: int [N], the chosen candidate;
    * ``score``: float64 [N], the Pearson correlation at the choice; ``curve``: float64 [N, K], that of every candidate (``pool="all"``: the
      pooled curve in every row); ``margin``: ``m``.

    One sums launch for all candidates (``pssr_rsf_moments_u8``) and one copy of the sums to the host; the choice is made in Python ints.
    A choice on the last candidate of a grid of several emits a ``UserWarning`` naming the items: the optimum may lie beyond the grid.
    ``to_numpy=False`` leaves ``curve`` on the device.  To start ``approximate_crappifier``'s search from the measured blur, pass
    ``sigma`` as the initial value of its ``Blur`` dimension."""
    import warnings
    if pool not in RSF_POOLS:
        raise ValueError(f"pool must be one of {RSF_POOLS}. Given {pool!r}.")
    if isinstance(pixel_size, bool) or not isinstance(pixel_size, (int, float, np.integer, np.floating)) or not pixel_size > 0 \
            or not math.isfinite(pixel_size):
        raise ValueError(f"pixel_size must be a positive number. Given {pixel_size!r}.")
    sig = _rsf_sigmas(sigmas)
    hat, frames, batched, _, _, _, m, rows = _rsf_sums("estimate_rsf", lr, hr_hat, sig)
    (n_img, c), K = hat.shape[:2], len(sig)
    n = c * (frames.shape[-2] - 2 * m) * (frames.shape[-1] - 2 * m)
    if pool == "all":
        chosen = [_rsf_choose(n_img * n, rows, K)] * n_img
    else:
        chosen = [_rsf_choose(n, rows[i * c:(i + 1) * c], K) for i in range(n_img)]
    edge = [i for i, (k, _) in enumerate(chosen) if K > 1 and k == K - 1]
    if edge:
        warnings.warn(f"estimate_rsf: the choice of item(s) {edge} is the last candidate (sigma={sig[-1]}); the optimum may lie beyond the "
                      "grid", UserWarning, stacklevel=2)
    index = np.array([k for k, _ in chosen], dtype=np.int64)
    sigma = np.array([sig[k] * float(pixel_size) for k, _ in chosen], dtype=np.float64)
    score = np.array([curve[k] for k, curve in chosen], dtype=np.float64)
    curve = np.array([curve for _, curve in chosen], dtype=np.float64).reshape(n_img, K)
    fwhm = _FWHM * sigma
    if not batched:
        sigma, fwhm, score, curve, index = float(sigma[0]), float(fwhm[0]), float(score[0]), curve[0], int(index[0])
    return RSF(sigma, fwhm, score, curve if to_numpy else torch.from_numpy(curve).to(hat.device), index, m)


def _rsf_reduced(who, lr, hr_hat, rsf):
    """The shared front half of ``consistency_map(rsf=...)`` and ``estimate_noise(rsf=...)``: the resolution-scaling function fitted
    (``"fit"``) or given (a width in HR pixels, or one per item), one ``_rsf_sums`` launch, and both sides inside its margin ->
    ``(d, lc, rows, sel, sig, per_item, batched, scale, m)`` with ``d`` uint8 [N, C, h - 2m, w - 2m] the blurred reduction of every plane at
    its item's width ``sig[per_item[i]]`` (row ``sel[p]`` of the search sums ``rows``) and ``lc`` the matching frames of ``lr``."""
    if isinstance(rsf, str):
        if rsf != "fit":
            raise ValueError(f'rsf must be None, "fit", a sigma in HR pixels or one sigma per item. Given {rsf!r}.')
        sig, per_item = list(RSF_SIGMAS), None                   # None: chosen from the sums
    elif isinstance(rsf, (int, float, np.integer, np.floating)) and not isinstance(rsf, bool):
        sig, per_item = _rsf_sigmas([rsf], "rsf"), "first"        # the one row, for every item
    else:
        given = _rsf_sigmas(rsf, "rsf")
        sig = sorted(set(given))
        per_item = [sig.index(v) for v in given]
    shape = tuple(hr_hat.shape) if hasattr(hr_hat, "shape") else np.shape(hr_hat)
    if isinstance(per_item, list) and (len(shape) != 4 or len(per_item) != shape[0]):
        raise ValueError(f"rsf as a sequence needs one sigma per item of a 4-D batch. Given {len(per_item)} for a shape of {shape}.")
    hat, frames, batched, scale, taps, R, m, rows = _rsf_sums(who, lr, hr_hat, sig)
    (n_img, c), K = hat.shape[:2], len(sig)
    hc, wc = frames.shape[-2] - 2 * m, frames.shape[-1] - 2 * m
    if per_item is None:
        per_item = [_rsf_choose(c * hc * wc, rows[i * c:(i + 1) * c], K)[0] for i in range(n_img)]
    elif per_item == "first":
        per_item = [0] * n_img
    sel = [k for k in per_item for _ in range(c)]
    d = ops.rsf_reduce_u8(hat, taps, R, sel)
    lc = ops.crop_shift_u8(frames, [(m, m)] * (n_img * c), hc, wc)
    return d, lc, rows, sel, sig, per_item, batched, scale, m


def _consistency_rsf(lr, hr_hat, fit, rsf, to_numpy):
    """``consistency_map(rsf=...)``: the map after a resolution-scaling function has been fitted (``"fit"``) or given (a width in HR pixels,
    or one per item)."""
    d, lc, rows, sel, sig, per_item, batched, _, m = _rsf_reduced("consistency_map", lr, hr_hat, rsf)
    (n_img, c, hc, wc), K = d.shape, len(sig)
    fits = [_consistency_fit(hc * wc, (row[3 * k], row[3 * K], row[3 * k + 1], row[3 * k + 2], row[3 * K + 1]), fit) for row, k in zip(rows, sel)]
    tables = torch.tensor([f[3] for f in fits], dtype=torch.int32).to(d.device)
    cmap, sse = ops.consistency_map_u8(d, lc, tables)
    stats = [np.array([f[k] for f in fits], dtype=np.float64).reshape(n_img, c) for k in range(3)]
    rse = np.array([math.sqrt(v / (hc * wc)) / 256 for v in sse.cpu().tolist()], dtype=np.float64).reshape(n_img, c)
    sigma = np.array([sig[k] for k in per_item], dtype=np.float64)
    if not batched:
        cmap, stats, rse, sigma = cmap[0], [v[0] for v in stats], rse[0], float(sigma[0])
    return RSFConsistency(cmap.cpu().numpy() if to_numpy else cmap, stats[0], stats[1], rse, stats[2], sigma, m)


def consistency_map(lr, hr_hat, *, fit: str = "affine", to_numpy: bool = True, rsf=None):
    r"""Scores predictions against their own low-resolution input, without ground truth: the resolution-scaled error map of the
    super-resolution microscopy literature under this package's forward model (``_gen_pair``'s Pillow-bilinear reduction).  ``lr``: uint8
    array or device tensor [N, m, h, w]; ``hr_hat``: uint8 [N, C, s*h, s*w], ``s`` an integer in 1 .. 16 (or both 3-D, without the batch
    axis).  Plane ``j`` of a prediction is compared with frame ``j`` of the ``C`` centre frames of its input (``_slice_center``, the rule of
    ``n_frames=[lr, hr]``).  Per plane: ``D`` = the prediction reduced to the LR grid (bit for bit ``PIL.Image.resize(..., BILINEAR)``), the
    line ``L ~ alpha D + beta`` fitted by least squares over the plane (``fit="affine"``; ``"identity"``: ``alpha = 1, beta = 0``), and

    * ``map``: uint8 [N, C, h, w], ``|L - (alpha D + beta)|`` rounded to grey levels (saturating at 255): where the prediction, seen through
      the forward model, does not reproduce what was measured;
    * ``rse``: the root mean square of that residual in grey levels, ``rsp``: the Pearson correlation of ``D`` and ``L`` (whatever ``fit``);
    * ``alpha``, ``beta``: the fit.  The four statistics are float64 arrays [N, C].

    One fused reduction + moments launch (``pssr_reduce_moments_u8``), one copy of ``5 N C`` integers to the host, the fit and the 256-entry
    tables in Python from those integers (exact; include/pssr_mi355.h has the expressions), one upload, one map launch
    (``pssr_consistency_map_u8``).  Everything after the fit is integer arithmetic: the result is a pure function of the bytes.
    ``to_numpy=False`` leaves ``map`` in HBM.

    ``rsf`` (keyword-only; ``None``: everything above, untouched) puts a Gaussian resolution-scaling function in front of the reduction, as
    the resolution-scaled error is defined: a prediction that is rightly sharper than the optics behind its input is then not marked at
    every edge.  ``"fit"``: the width that ``estimate_rsf`` chooses per item among its default candidates; a number: that sigma in HR
    pixels for every item; a sequence: one sigma per item.  ``D`` is then the blurred reduction of the chosen width
    (``pssr_rsf_reduce_u8``) inside the margin ``m`` of the search, the fit of every plane comes from that plane's own row of the search
    sums (no second moments launch), and the result is ``RSFConsistency(map, alpha, beta, rse, rsp, sigma, margin)`` with ``map``
    [N, C, h - 2m, w - 2m] and ``sigma`` float64 [N] in HR pixels."""
    _check_fit(fit)
    if rsf is not None:
        return _consistency_rsf(lr, hr_hat, fit, rsf, to_numpy)
    hr_hat, lr, batched, _, dev = _u8_image_pair("consistency_map", hr_hat, lr, ("hr_hat", "lr"), ("A prediction of {} planes", "an input of {} frames"))
    (n_img, c), (h, w) = hr_hat.shape[:2], lr.shape[-2:]
    from .data import _slice_center
    frames = _slice_center(lr.to(dev), c).contiguous()
    d, sums = ops.reduce_moments_u8(hr_hat.to(dev).contiguous(), frames)
    fits = [_consistency_fit(h * w, row, fit) for row in sums.cpu().tolist()]
    tables = torch.tensor([f[3] for f in fits], dtype=torch.int32).to(dev)
    cmap, sse = ops.consistency_map_u8(d, frames, tables)
    stats = [np.array([f[k] for f in fits], dtype=np.float64).reshape(n_img, c) for k in range(3)]
    rse = np.array([math.sqrt(v / (h * w)) / 256 for v in sse.cpu().tolist()], dtype=np.float64).reshape(n_img, c)
    if not batched:
        cmap, stats, rse = cmap[0], [v[0] for v in stats], rse[0]
    return Consistency(cmap.cpu().numpy() if to_numpy else cmap, stats[0], stats[1], rse, stats[2])


NOISE_POOLS = ("all", "item")                        # estimate_noise's ``pool``


class Noise(namedtuple("Noise", "poisson gaussian gain saltpepper slope intercept alpha beta levels found table sigma margin")):
    """What ``estimate_noise`` measured: the crappifier parameters ``poisson`` (the intensity ``i``), ``gaussian`` (the additive width in
    grey levels), ``gain`` (grey levels) and ``saltpepper`` (percent, as the ``SaltPepper`` constructor takes it); the two fitted lines
    ``var ~ slope v + intercept`` and ``mean ~ alpha v + beta`` they come from; ``levels``, how many grey levels the lines rest on, and
    ``found``, whether there was one; the pooled int64 ``table`` [256, 5]; the RSF width ``sigma`` in HR pixels and the ``margin`` in LR
    pixels the pair was compared inside.  Scalars for ``pool="all"`` (and for a pair without the batch axis), arrays [N] for ``"item"``."""
    __slots__ = ()

    def crappifier(self, scale=None, item=None):
        """The measurement as a ``MultiCrappifier(..., clip=True)`` of the stages that are not zero, in the order ``Blur(sigma / scale)``,
        ``Poisson(poisson, gain)``, ``AdditiveGaussian(gaussian)``, ``SaltPepper(saltpepper)``; an empty one where nothing was
        measurable.  ``scale``: the pair's integer scale, needed when ``sigma > 0``: the RSF is measured in HR pixels before the reduction
        and ``Blur`` acts on the LR tile, so the stage has the width ``sigma / scale`` -- the small-sigma approximation that blur and
        reduction commute.  ``item``: which item of a ``pool="item"`` result.  Two uses::

            noise = estimate_noise(lr, hr, rsf="fit")
            dataset = ImageDataset(hr_path, crappifier=noise.crappifier(scale=4))      # train directly with what was measured
            build = lambda i, g, s: MultiCrappifier(Poisson(i, g), AdditiveGaussian(s))
            approximate_crappifier(build, space, pairs,                                # or start the search from it
                                   opt_kwargs={"x0": [noise.poisson, noise.gain, noise.gaussian]})

        (``bayes.gp_minimize`` and skopt both take ``x0``, in the order of the search's dimensions.)"""
        from .crappifiers import AdditiveGaussian, Blur, MultiCrappifier, Poisson, SaltPepper
        if np.ndim(self.poisson):
            if isinstance(item, bool) or not isinstance(item, (int, np.integer)) or not 0 <= item < len(self.poisson):
                raise ValueError(f"crappifier needs item, 0 .. {len(self.poisson) - 1}, for a result of pool=\"item\". Given {item!r}.")
            pick = lambda v: v[item].item()                       # noqa: E731
        elif item is not None:
            raise ValueError(f"item is for a result of pool=\"item\"; this one has scalars. Given {item!r}.")
        else:
            pick = lambda v: v                                   # noqa: E731
        poisson, gaussian, gain, saltpepper, sigma = (float(pick(v)) for v in (self.poisson, self.gaussian, self.gain, self.saltpepper, self.sigma))
        stages = []
        if sigma > 0:
            if isinstance(scale, bool) or not isinstance(scale, (int, np.integer)) or not 1 <= scale <= 16:
                raise ValueError(f"crappifier needs the pair's scale, an int from 1 to 16, to turn sigma={sigma} HR pixels into LR pixels. "
                                 f"Given {scale!r}.")
            stages.append(Blur(sigma / int(scale)))
        if poisson > 0 or gain != 0:
            stages.append(Poisson(poisson, gain))
        if gaussian > 0:
            stages.append(AdditiveGaussian(gaussian))
        if saltpepper > 0:
            stages.append(SaltPepper(saltpepper))
        return MultiCrappifier(*stages, clip=True)


def _noise_fit(table, min_count, guard):
    """``(poisson, gaussian, gain, saltpepper, slope, intercept, alpha, beta, levels, found)`` from one level table (``[256][5]`` ints:
    ``n, sum L, sum L^2, n0, n255`` of every level of ``D``), in exactly the expressions of include/pssr_mi355.h.  The moments of a level
    are quotients of Python ints (exact before the one division); the two lines are fitted in floats, centred."""
    rows = [[int(x) for x in row] for row in table]

    def share(levels, col):
        den = sum(rows[v][0] for v in levels)
        return (sum(rows[v][col] for v in levels) / den if den else 0.0), den

    (pepper, bright), (salt, dark) = share(range(128, 256), 3), share(range(128), 4)
    amount = pepper + salt if bright and dark else 2.0 * (pepper + salt)
    used = []                                            # (v, n', mean, var)
    for v, (n, s1, s2, n0, n255) in enumerate(rows):
        k, s1, s2 = n - n0 - n255, s1 - 255 * n255, s2 - 255 * 255 * n255
        if k < max(min_count, 2):
            continue
        mean, var = s1 / k, (k * s2 - s1 * s1) / (k * (k - 1))
        reach = guard * math.sqrt(var)
        if mean - reach > 0 and mean + reach < 255:
            used.append((float(v), k, mean, var))
    if not used:
        return 0.0, 0.0, 0.0, 100.0 * amount, 0.0, 0.0, 0.0, 0.0, 0, False
    total = sum(k for _, k, _, _ in used)
    vbar = sum(k * v for v, k, _, _ in used) / total
    mbar = sum(k * mean for _, k, mean, _ in used) / total
    qbar = sum(k * var for _, k, _, var in used) / total
    gain = sum(k * (mean - v) for v, k, mean, _ in used) / total
    if len(used) < 2:
        slope, intercept, alpha, beta = 0.0, qbar, 1.0, gain
    else:
        svv = sum(k * (v - vbar) * (v - vbar) for v, k, _, _ in used)
        slope = sum(k * (v - vbar) * (var - qbar) for v, k, _, var in used) / svv
        alpha = sum(k * (v - vbar) * (mean - mbar) for v, k, mean, _ in used) / svv
        intercept, beta = qbar - slope * vbar, mbar - alpha * vbar
    return math.sqrt(max(slope, 0.0)), math.sqrt(max(intercept, 0.0)), gain, 100.0 * amount, slope, intercept, alpha, beta, len(used), True


def estimate_noise(lr, hr, *, rsf=None, pool: str = "all", min_count: int = 32, guard: float = 4.0, to_numpy: bool = True):
    r"""Measures the noise model between a sharp image and a measured one, in the terms of this package's own crappifiers: what
    ``approximate_crappifier`` searches for, read off the pair directly.  ``lr``: uint8 array or device tensor [N, m, h, w]; ``hr``: uint8
    [N, C, s*h, s*w], ``s`` an integer in 1 .. 16 (or both 3-D, without the batch axis) -- a real HR / LR pair (``register_pairs``
    first).  Plane ``j`` meets frame ``j`` of the ``C`` centre frames of ``lr`` (``_slice_center``).  With ``D`` the reduced HR image and
    ``L = clip8(rint(D (1 - i) + i Poisson(D) + g + N(0, sigma_n)))``, on every grey level ``v`` far from the clipping ends
    ``E[L | D = v] = v + g`` and ``Var[L | D = v] = i**2 v + sigma_n**2``: a photon-transfer curve binned by the signal the pair already
    contains.  The slope of the variance against the level gives ``poisson``, its intercept ``gaussian``, the mean residual ``gain``, and
    pixels at exactly 0 on bright levels or 255 on dark ones give ``saltpepper``.  The 1/12 that rounding to integers adds to every
    variance is not taken off the intercept.  include/pssr_mi355.h has the definitions.

    * ``rsf`` (``None``: ``D = bilinear_down_u8(hr)``, margin 0): ``"fit"``, a sigma in HR pixels or one per item, as in
      ``consistency_map(rsf=...)`` -- ``D`` is then the blurred reduction of that width and both sides lose the search's margin ``m``;
    * ``pool``: ``"all"``, one microscope: every plane of every item adds its table (the default: one tile rarely fills enough levels);
      ``"item"``: the planes of an item add theirs;
    * ``min_count`` (>= 2) and ``guard`` (> 0): a level is used when it keeps ``min_count`` unsaturated pixels and its mean stays
      ``guard`` standard deviations inside (0, 255).

    One table launch for the batch (``pssr_level_moments_u8``: exact integers), one copy to the host, the fit in Python
    (``_noise_fit``).  Returns ``Noise(poisson, gaussian, gain, saltpepper, slope, intercept, alpha, beta, levels, found, table, sigma,
    margin)``; ``Noise.crappifier`` turns it into a ``MultiCrappifier``.  ``sigma`` is the RSF width used (``pool="all"``: the mean of the
    items').  ``found = False`` (no level could be used; every parameter but ``saltpepper`` is 0) emits a ``UserWarning`` naming the
    items, and so does ``|alpha - 1| > 0.1``: the crappifier family has no intensity scale, so ``gain`` then means little.
    ``to_numpy=False`` leaves ``table`` on the device."""
    import warnings
    if pool not in NOISE_POOLS:
        raise ValueError(f"pool must be one of {NOISE_POOLS}. Given {pool!r}.")
    if isinstance(min_count, bool) or not isinstance(min_count, (int, np.integer)) or min_count < 2:
        raise ValueError(f"min_count must be an int of at least 2. Given {min_count!r}.")
    if isinstance(guard, bool) or not isinstance(guard, (int, float, np.integer, np.floating)) or not guard > 0 or not math.isfinite(guard):
        raise ValueError(f"guard must be a finite positive number. Given {guard!r}.")
    if rsf is None:
        hr, lr, batched, _, dev = _u8_image_pair("estimate_noise", hr, lr, ("hr", "lr"), ("An HR item of {} planes", "an LR item of {} frames"))
        (n_img, c), (h, w) = hr.shape[:2], lr.shape[-2:]
        if not (hr.is_cuda or lr.is_cuda or torch.cuda.is_available()):
            raise RuntimeError("pssr2_amd.util.estimate_noise needs an MI355X (HIP) device, and none is available; there is no CPU fallback")
        from .data import _slice_center
        lc = _slice_center(lr.to(dev), c).contiguous()
        d = ops.bilinear_down_u8(hr.to(dev).contiguous(), h, w)
        m, sigma = 0, [0.0] * n_img
    else:
        d, lc, _, _, sig, per_item, batched, _, m = _rsf_reduced("estimate_noise", lr, hr, rsf)
        n_img, c = d.shape[:2]
        sigma = [sig[k] for k in per_item]
    table = ops.level_moments_u8(d.reshape(n_img * c, -1), lc.reshape(n_img * c, -1)).view(n_img, c, 256, ops.LEVEL_MOMENTS)
    table = table.sum(dim=(0, 1)) if pool == "all" else table.sum(dim=1)
    host = table.cpu()
    fits = [_noise_fit(t, int(min_count), float(guard)) for t in (host[None] if pool == "all" else host).tolist()]
    whom = "the pooled batch" if pool == "all" else "item(s) {}"
    missing = [i for i, f in enumerate(fits) if not f[9]]
    if missing:
        warnings.warn(f"estimate_noise: no grey level of {whom.format(missing)} keeps {min_count} pixels {guard} standard deviations inside "
                      "(0, 255); nothing but saltpepper could be measured", UserWarning, stacklevel=2)
    scaled = [i for i, f in enumerate(fits) if f[9] and abs(f[6] - 1.0) > 0.1]
    if scaled:
        warnings.warn(f"estimate_noise: the mean of lr follows hr with a slope of {[fits[i][6] for i in scaled]} for {whom.format(scaled)}; "
                      "the crappifiers have no intensity scale, so gain means little here", UserWarning, stacklevel=2)
    if not to_numpy:
        host = table
    else:
        host = host.numpy()
    if pool == "all" or not batched:
        return Noise(*fits[0], host if pool == "all" else host[0], float(sum(sigma) / len(sigma)), m)
    cols = list(zip(*fits))
    fields = [np.array(col, dtype=np.float64) for col in cols[:8]] + [np.array(cols[8], dtype=np.int64), np.array(cols[9], dtype=bool)]
    return Noise(*fields, host, np.array(sigma, dtype=np.float64), m)


Registration = namedtuple("Registration", "hr lr shift score margin")


def _check_radius(radius, what="radius"):
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 0 <= radius <= ops.MAX_REGISTER_RADIUS:
        raise ValueError(f"{what} must be an int from 0 to {ops.MAX_REGISTER_RADIUS} (the search radius in HR pixels). Given {radius!r}.")
    return int(radius)


def _register_choose(n: int, rows, radius: int):
    """``((ty, tx), score)`` of one item from the exact sums of its matched planes (``rows``: one list of ``3 T + 2`` ints per plane, the
    layout of ``pssr_register_shifts_u8``) over ``n`` pixels in all, in exactly the expressions of include/pssr_mi355.h: the planes' sums
    add, the score of a shift is the signed squared Pearson correlation ``num |num| / (den denl)`` (0 when ``den`` or ``denl`` is 0),
    compared by cross-multiplying Python ints; ties go to the smaller ``ty**2 + tx**2``, then ``ty``, then ``tx``."""
    side = 2 * radius + 1
    pooled = [sum(int(v) for v in col) for col in zip(*rows)]
    sl, sll = pooled[3 * side * side], pooled[3 * side * side + 1]
    best = None                                         # (p, q): the score p / (q denl), q > 0; then the tie key and the correlation
    for t in range(side * side):
        sd, sdd, sdl = pooled[3 * t:3 * t + 3]
        ty, tx = t // side - radius, t % side - radius
        num, den, denl, r = _pearson_terms(n, sd, sl, sdd, sdl, sll)
        p, q = (num * abs(num), den) if den > 0 and denl > 0 else (0, 1)
        key = (ty * ty + tx * tx, ty, tx)
        if best is None or p * best[1] > best[0] * q or (p * best[1] == best[0] * q and key < best[2]):
            best = (p, q, key, r)
    return (best[2][1], best[2][2]), best[3]


def register_pairs(hr, lr, *, radius: int = 8, to_numpy: bool = True):
    r"""Aligns real (HR, LR) pairs -- two acquisitions of one field of view, a few HR pixels apart by stage drift and scan offset -- by an
    exhaustive search over integer shifts under this package's forward model (``_gen_pair``'s Pillow-bilinear reduction).  ``hr``: uint8
    array or device tensor [N, C, s*h, s*w]; ``lr``: uint8 [N, c, h, w], ``s`` an integer in 1 .. 16 inferred from the sizes (or both 3-D,
    without the batch axis).  Frame ``j`` of ``hr`` meets frame ``j`` of the ``C`` centre frames of ``lr`` (``_slice_center``, the rule of
    ``n_frames=[lr, hr]``).  For every shift ``(ty, tx)`` of at most ``radius`` HR pixels (0 .. 32) the HR item, moved by the shift and
    reduced to the LR grid, is correlated with the LR item inside a margin of ``m = 1 + ceil(radius / s)`` LR pixels; the shift with the
    largest signed squared Pearson correlation wins, one shift per item (its planes pool their sums; include/pssr_mi355.h has the
    definitions, exact integers throughout).  Returns ``Registration(hr, lr, shift, score, margin)``:

    * ``lr``: uint8 [N, c, h - 2m, w - 2m], every LR frame without the margin; ``hr``: uint8 [N, C, s (h - 2m), s (w - 2m)], the window of
      the HR item that shows the same field of view;
    * ``shift``: int [N, 2], ``(ty, tx)`` in HR pixels: ``hr_out = hr[..., s m + ty : s (h - m) + ty, s m + tx : s (w - m) + tx]``;
    * ``score``: float [N], the Pearson correlation at the chosen shift; ``margin``: ``m``.

    One sums launch (``pssr_register_shifts_u8``), one copy of the sums to the host, the choice in Python ints, one origin upload and two
    crop launches (``pssr_crop_shift_u8``).  A chosen ``|ty|`` or ``|tx|`` equal to ``radius > 0`` emits a ``UserWarning`` naming the
    items: the optimum may then lie outside the window.  ``to_numpy=False`` leaves ``hr`` and ``lr`` in HBM.  ``s = 1`` is taken, so a
    prediction can be aligned to its ground truth."""
    import warnings
    radius = _check_radius(radius)
    hr, lr, batched, scale, dev = _u8_image_pair("register_pairs", hr, lr, ("hr", "lr"), ("An HR item of {} frames", "an LR item of {} frames"))
    (n_img, C), (c, h, w) = hr.shape[:2], lr.shape[1:]
    m = ops.register_margin(scale, radius)
    hc, wc = h - 2 * m, w - 2 * m
    if hc < 1 or wc < 1:
        raise ValueError(f"An LR image of {h}x{w} leaves nothing inside the margin of {m} pixels that radius={radius} at scale {scale} needs on every side.")
    if not (hr.is_cuda or lr.is_cuda or torch.cuda.is_available()):
        raise RuntimeError("pssr2_amd.util.register_pairs needs an MI355X (HIP) device, and none is available; there is no CPU fallback")
    from .data import _slice_center
    hr, lr = hr.to(dev).contiguous(), lr.to(dev).contiguous()
    sums = ops.register_shifts_u8(hr, _slice_center(lr, C).contiguous(), radius).cpu().tolist()
    chosen = [_register_choose(C * hc * wc, sums[i * C:(i + 1) * C], radius) for i in range(n_img)]
    edge = [i for i, ((ty, tx), _) in enumerate(chosen) if radius > 0 and max(abs(ty), abs(tx)) == radius]
    if edge:
        warnings.warn(f"register_pairs: the chosen shift of item(s) {edge} lies on the edge of the search window (radius={radius}); the optimum "
                      "may lie outside it", UserWarning, stacklevel=2)
    origins = [(scale * m + ty, scale * m + tx) for (ty, tx), _ in chosen for _ in range(C)] + [(m, m)] * (n_img * c)
    table = torch.tensor(origins, dtype=torch.int32).to(dev)
    hr_out = ops.crop_shift_u8(hr, origins[:n_img * C], scale * hc, scale * wc, table=table[:n_img * C])
    lr_out = ops.crop_shift_u8(lr, origins[n_img * C:], hc, wc, table=table[n_img * C:])
    shift = np.array([sh for sh, _ in chosen], dtype=np.int64).reshape(n_img, 2)
    score = np.array([sc for _, sc in chosen], dtype=np.float64)
    if not batched:
        hr_out, lr_out, shift, score = hr_out[0], lr_out[0], shift[0], score[0]
    if to_numpy:
        hr_out, lr_out = hr_out.cpu().numpy(), lr_out.cpu().numpy()
    return Registration(hr_out, lr_out, shift, score, m)


SCAN_POOLS = ("all", "item", "plane")                # estimate_scan_phase's ``pool``


class ScanPhaseFit(namedtuple("ScanPhaseFit", "phase shift score curve radius")):
    """What :func:`estimate_scan_phase` returns: ``phase`` (pixels, float), ``shift`` (the integer candidate ``k``), ``score`` (the
    Pearson correlation at ``k``), ``curve`` (the ``2 radius + 1`` correlations, ``k = -radius .. radius``) and ``radius``."""
    __slots__ = ()

    def crappifier(self, spread: float = 0, jitter: float = 0):
        """A :class:`pssr2_amd.crappifiers.ScanPhase` that plants the measured phase (the mean over the pool's items)."""
        from .crappifiers import ScanPhase
        phase = self.phase.cpu().numpy() if torch.is_tensor(self.phase) else self.phase
        return ScanPhase(float(np.mean(phase)), spread=spread, jitter=jitter)


def _check_scan_radius(radius):
    if isinstance(radius, bool) or not isinstance(radius, (int, np.integer)) or not 0 <= radius <= ops.MAX_SCAN_RADIUS:
        raise ValueError(f"radius must be an int from 0 to {ops.MAX_SCAN_RADIUS} (the search radius in pixels). Given {radius!r}.")
    return int(radius)


def _check_scan_pool(pool):
    if pool not in SCAN_POOLS:
        raise ValueError(f"pool must be one of {SCAN_POOLS}. Given {pool!r}.")


def _scan_image(who, lr, radius):
    """The checks of the scan-phase entry points' image: a uint8 array or device tensor [N, c, h, w] or [c, h, w], ``h >= 3``,
    ``w >= 2 radius + 1``, at most 2**28 pixels per plane.  -> ``(4-D tensor where it was, batched)``."""
    if not torch.is_tensor(lr):
        lr = torch.as_tensor(np.ascontiguousarray(lr))
    elif not lr.is_cuda:
        raise RuntimeError(f"pssr2_amd.util.{who} runs on an MI355X (HIP) device only; there is no CPU fallback")
    if lr.dtype != torch.uint8:
        raise TypeError(f"{who} takes uint8 images; lr is {lr.dtype}")
    if lr.dim() not in (3, 4):
        raise ValueError(f"lr must be 4-D, [images, frames, height, width], or 3-D without the batch axis. Its shape is {tuple(lr.shape)}.")
    batched = lr.dim() == 4
    if not batched:
        lr = lr[None]
    n_img, c, h, w = lr.shape
    if min(n_img, c) < 1 or h < 3 or w < 2 * radius + 1:
        raise ValueError(f"lr needs at least one plane of at least 3 rows and 2 * radius + 1 = {2 * radius + 1} columns. Its shape is {tuple(lr.shape)}.")
    if h * w > 1 << 28:
        raise ValueError(f"A plane of lr of {h * w} pixels is above the 2**28 up to which the sums are exact.")
    return lr, batched


def _scan_choose(n: int, sums, radius: int):
    """``(k, phase, score, curve)`` of one pool from its ``3 T + 2`` exact pooled sums (Python ints: ``T`` triples ``sum O_k, sum O_k**2,
    sum O_k E``, then ``sum E, sum E**2``) over ``n`` (row, column) pairs, in exactly the expressions of include/pssr_mi355.h (D4): the
    score of ``k`` is the signed squared Pearson correlation ``num |num| / (den denl)`` (0 when ``den`` or ``denl`` is 0), compared by
    cross-multiplying Python ints; ties go to the smaller ``|k|``, then the smaller ``k``; then the parabola through the float
    correlations at ``k - 1, k, k + 1``."""
    T = 2 * radius + 1
    sl, sll = int(sums[3 * T]), int(sums[3 * T + 1])
    best, curve = None, []
    for t in range(T):
        sd, sdd, sdl = (int(v) for v in sums[3 * t:3 * t + 3])
        k = t - radius
        num, den, denl, r = _pearson_terms(n, sd, sl, sdd, sdl, sll)
        curve.append(r)
        p, q = (num * abs(num), den) if den > 0 and denl > 0 else (0, 1)
        key = (abs(k), k)
        if best is None or p * best[1] > best[0] * q or (p * best[1] == best[0] * q and key < best[2]):
            best = (p, q, key)
    k = best[2][1]
    delta = 0.0
    if abs(k) < radius:
        rm, r0, rp = curve[k + radius - 1], curve[k + radius], curve[k + radius + 1]
        c = rm - 2.0 * r0 + rp
        if c < 0.0:
            delta = min(max(0.5 * (rm - rp) / c, -0.5), 0.5)
    return k, k + delta, curve[k + radius], curve


def estimate_scan_phase(lr, *, radius: int = 8, pool: str = "all", to_numpy: bool = True):
    r"""Measures the scan phase of bidirectionally scanned images: the sideways offset, in pixels, of the odd rows against the even ones
    that a mistimed return sweep leaves (a comb on every vertical edge; it lowers the resolution along x and leaves y alone).  ``lr``:
    uint8 array or device tensor [N, c, h, w] (or 3-D, without the batch axis).  Every interior row, moved by each integer
    ``k = -radius .. radius`` (``radius`` 0 .. 16), is correlated with the sum of its two neighbours; odd rows count at ``k``, even rows
    at ``-k``; the ``k`` with the largest signed squared Pearson correlation wins and a parabola through its neighbours gives the
    fraction (include/pssr_mi355.h has the definitions, exact integers up to the choice).  ``pool``: one estimate for ``"all"`` planes,
    per ``"item"`` or per ``"plane"``.  Returns ``ScanPhaseFit(phase, shift, score, curve, radius)``: scalars and a curve [T] for
    ``pool="all"``, arrays [N] / [N, T] for ``"item"`` and [N, c] / [N, c, T] for ``"plane"`` (without the leading axis for a 3-D input).

    One launch (``pssr_line_moments_u8``), exact int64 pooling on the device, one copy to the host, the choice in Python ints.  A chosen
    ``|k| == radius > 0`` emits a ``UserWarning`` (the optimum may lie outside the window), and so does an image without any
    correlation to choose by (a constant image), whose phase is 0.0.  ``to_numpy=False`` returns the arrays as float64 / int64 tensors."""
    import warnings
    radius = _check_scan_radius(radius)
    _check_scan_pool(pool)
    lr, batched = _scan_image("estimate_scan_phase", lr, radius)
    if not (lr.is_cuda or torch.cuda.is_available()):
        raise RuntimeError("pssr2_amd.util.estimate_scan_phase needs an MI355X (HIP) device, and none is available; there is no CPU fallback")
    n_img, c, h, w = lr.shape
    T = 2 * radius + 1
    sums = ops.line_moments_u8(lr.to("cuda") if not lr.is_cuda else lr, radius)          # [planes, h - 2, 3 T + 2]
    odd, even = sums[:, 0::2].sum(1), sums[:, 1::2].sum(1)                                # rows y = 1, 3, ..  and  y = 2, 4, ..
    even = torch.cat([even[:, :3 * T].reshape(-1, T, 3).flip(1).reshape(-1, 3 * T), even[:, 3 * T:]], 1)      # an even row counts at -k
    pooled = (odd + even).reshape(n_img, c, 3 * T + 2)
    n = (h - 2) * (w - 2 * radius)
    if pool == "all":
        pooled, n, shape = pooled.sum((0, 1))[None], n * n_img * c, ()
    elif pool == "item":
        pooled, n, shape = pooled.sum(1), n * c, (n_img,)
    else:
        pooled, shape = pooled.reshape(n_img * c, -1), (n_img, c)
    chosen = [_scan_choose(n, row, radius) for row in pooled.cpu().tolist()]
    edge = [i for i, ch in enumerate(chosen) if radius > 0 and abs(ch[0]) == radius]
    if edge:
        warnings.warn(f"estimate_scan_phase: the chosen shift of pool item(s) {edge} lies on the edge of the search window (radius={radius}); "
                      "the optimum may lie outside it", UserWarning, stacklevel=2)
    flat = [i for i, ch in enumerate(chosen) if not any(ch[3])]
    if flat:
        warnings.warn(f"estimate_scan_phase: pool item(s) {flat} show no correlation between neighbouring rows at any shift (a constant image?); "
                      "their phase is 0.0", UserWarning, stacklevel=2)
    if not batched and shape:
        shape = shape[1:]
    phase = np.array([ch[1] for ch in chosen], dtype=np.float64).reshape(shape)
    shift = np.array([ch[0] for ch in chosen], dtype=np.int64).reshape(shape)
    score = np.array([ch[2] for ch in chosen], dtype=np.float64).reshape(shape)
    curve = np.array([ch[3] for ch in chosen], dtype=np.float64).reshape(shape + (T,))
    if not to_numpy:
        phase, shift, score, curve = (torch.from_numpy(v) for v in (phase, shift, score, curve))
    if not shape:
        phase, shift, score = float(phase), int(shift), float(score)
    return ScanPhaseFit(phase, shift, score, curve, radius)


def correct_scan_phase(lr, phase=None, *, radius: int = 8, pool: str = "all", to_numpy: bool = True):
    r"""Removes the scan phase of bidirectionally scanned images: the odd rows of every plane move back by ``phase`` pixels (linear
    resampling in steps of 1/256 pixel with edge replication, ``d = -floor(256 phase + 0.5)``: include/pssr_mi355.h, D1 and D5); the even
    rows are copied.  ``lr`` as for :func:`estimate_scan_phase`.  ``phase=None`` estimates it first with ``radius`` and ``pool``; else a
    number, or one value per item of ``pool`` (``"all"``: one; ``"item"``: [N]; ``"plane"``: [N, c]).  Returns ``(corrected, phase)``:
    uint8 of the shape of ``lr`` (a device tensor for ``to_numpy=False``) and the phase that was applied.  Run it in front of
    ``estimate_noise``, ``register_pairs`` or a prediction: a comb biases all three."""
    radius = _check_scan_radius(radius)
    _check_scan_pool(pool)
    lr, batched = _scan_image("correct_scan_phase", lr, 0)
    n_img, c, h, w = lr.shape
    if phase is not None:
        ph = np.asarray(phase.cpu() if torch.is_tensor(phase) else phase, dtype=np.float64)
        want = {"all": (), "item": (n_img,), "plane": (n_img, c)}[pool]
        if not batched:
            want = want[1:]
        if ph.shape not in ((), want) or not np.all(np.isfinite(ph)) or np.any(np.abs(ph) > 64):
            raise ValueError(f"phase must be a finite number of at most 64 pixels, or one per item of pool={pool!r} (shape {want}). Given {phase!r}.")
    if not (lr.is_cuda or torch.cuda.is_available()):
        raise RuntimeError("pssr2_amd.util.correct_scan_phase needs an MI355X (HIP) device, and none is available; there is no CPU fallback")
    lr = lr.to("cuda") if not lr.is_cuda else lr
    if phase is None:
        if w < 2 * radius + 1:
            raise ValueError(f"lr needs at least 2 * radius + 1 = {2 * radius + 1} columns for the estimate. Its shape is {tuple(lr.shape)}.")
        phase = estimate_scan_phase(lr if batched else lr[0], radius=radius, pool=pool).phase
        ph = np.asarray(phase, dtype=np.float64)
    per_plane = np.broadcast_to(ph if ph.ndim == 0 else ph.reshape(n_img, -1), (n_img, c))       # [N] -> [N, 1], [c] -> [1, c]
    d = -np.floor(256.0 * per_plane + 0.5).astype(np.int64)
    table = np.zeros((n_img, c, h), dtype=np.int32)
    table[:, :, 1::2] = d[:, :, None]
    out = ops.shift_rows_u8(lr, torch.from_numpy(table).to(lr.device))
    if not batched:
        out = out[0]
    return (out.cpu().numpy() if to_numpy else out), phase


def _baseline_image(who, lr):
    """The checks of the classical baselines' image, in ``_scan_image``'s order: a uint8 array or device tensor [N, c, h, w] or
    [c, h, w] with at least one pixel and at most 2**28 per plane.  -> ``(4-D tensor where it was, batched)``."""
    if not torch.is_tensor(lr):
        lr = torch.as_tensor(np.ascontiguousarray(lr))
    elif not lr.is_cuda:
        raise RuntimeError(f"pssr2_amd.util.{who} runs on an MI355X (HIP) device only; there is no CPU fallback")
    if lr.dtype != torch.uint8:
        raise TypeError(f"{who} takes uint8 images; lr is {lr.dtype}")
    if lr.dim() not in (3, 4):
        raise ValueError(f"lr must be 4-D, [images, frames, height, width], or 3-D without the batch axis. Its shape is {tuple(lr.shape)}.")
    batched = lr.dim() == 4
    if not batched:
        lr = lr[None]
    if min(lr.shape) < 1:
        raise ValueError(f"lr needs at least one plane of at least one pixel. Its shape is {tuple(lr.shape)}.")
    if lr.shape[-2] * lr.shape[-1] > 1 << 28:
        raise ValueError(f"A plane of lr of {lr.shape[-2] * lr.shape[-1]} pixels is above the 2**28 that a launch takes.")
    return lr, batched


def _baseline_device(who, lr):
    if not (lr.is_cuda or torch.cuda.is_available()):
        raise RuntimeError(f"pssr2_amd.util.{who} needs an MI355X (HIP) device, and none is available; there is no CPU fallback")
    return lr if lr.is_cuda else lr.to("cuda")


def _check_upsample(scale, filter):
    if isinstance(scale, bool) or not isinstance(scale, (int, np.integer)) or not 1 <= scale <= ops.MAX_UPSAMPLE:
        raise ValueError(f"scale must be an int from 1 to {ops.MAX_UPSAMPLE}. Given {scale!r}.")
    if filter not in ops.UPSAMPLE_FILTERS:
        raise ValueError(f"filter must be one of {ops.UPSAMPLE_FILTERS}. Given {filter!r}.")
    return int(scale)


def upsample(lr, scale, *, filter: str = "bicubic", to_numpy: bool = True):
    r"""The "LR-bicubic" row of a super-resolution table: ``lr`` enlarged by the integer ``scale`` (1 .. 8) exactly as Pillow's 8-bit
    ``Image.resize`` enlarges it with ``filter`` ``"bicubic"`` (Keys, a = -0.5) or ``"bilinear"``: the same bytes (B1 of
    include/pssr_mi355.h: 22-bit fixed-point taps, the x pass rounded and clipped to uint8, then the y pass).  ``lr``: uint8 array or
    device tensor [N, c, h, w] (or 3-D, without the batch axis); returns uint8 [..., h scale, w scale], a device tensor for
    ``to_numpy=False``.  One launch (``pssr_upsample_u8``) for all planes."""
    scale = _check_upsample(scale, filter)
    lr, batched = _baseline_image("upsample", lr)
    if lr.shape[-2] * scale * lr.shape[-1] * scale > 1 << 28:
        raise ValueError(f"A plane of lr enlarged {scale} times has {lr.shape[-2] * scale * lr.shape[-1] * scale} pixels, above the 2**28 that a launch takes.")
    out = ops.upsample_u8(_baseline_device("upsample", lr), scale, filter)
    if not batched:
        out = out[0]
    return out.cpu().numpy() if to_numpy else out


def _nlm_params(h, sigma, P):
    """``(qmul, qshift, bias)`` of the integer non-local means (B2 of include/pssr_mi355.h) for ``P x P`` patches:
    ``bias = rint(2 P**2 sigma**2)``; ``qshift`` the largest of 0 .. 31 with ``qmul = rint(32 * 2**qshift / (P**2 h**2)) <= 1023``."""
    if isinstance(h, bool) or not isinstance(h, (int, float, np.integer, np.floating)) or not 0.5 <= h <= 255:
        raise ValueError(f"h must be a number from 0.5 to 255 (the filter strength in grey levels). Given {h!r}.")
    if isinstance(sigma, bool) or not isinstance(sigma, (int, float, np.integer, np.floating)) or not 0 <= sigma <= 255:
        raise ValueError(f"sigma must be a number from 0 to 255 (the noise level in grey levels). Given {sigma!r}.")
    h, sigma = float(h), float(sigma)
    bias = int(np.rint(2.0 * P * P * sigma * sigma))
    for qshift in range(31, -1, -1):
        qmul = int(np.rint(32.0 * 2.0 ** qshift / (P * P * h * h)))
        if qmul <= 1023:
            break
    if qmul < 1:
        raise ValueError(f"h = {h} is too large for {P} x {P} patches: the weights' scale rounds to zero.")
    return qmul, qshift, bias


def _check_nlm(h, sigma, patch_radius, search_radius):
    for name, v, hi in (("patch_radius", patch_radius, ops.MAX_NLM_PATCH), ("search_radius", search_radius, ops.MAX_NLM_SEARCH)):
        if isinstance(v, bool) or not isinstance(v, (int, np.integer)) or not 1 <= v <= hi:
            raise ValueError(f"{name} must be an int from 1 to {hi}. Given {v!r}.")
    return (int(patch_radius), int(search_radius)) + _nlm_params(h, sigma, 2 * int(patch_radius) + 1)


def nlm_denoise(lr, *, h, sigma: float = 0.0, patch_radius: int = 2, search_radius: int = 7, to_numpy: bool = True):
    r"""Non-local means (Buades et al.; the algorithm of scikit-image's ``denoise_nl_means``) for the "LR-denoised" row of a table, in
    integers (B2 of include/pssr_mi355.h), so every run and every machine gives the same bytes.  ``lr``: uint8 array or device tensor
    [N, c, h, w] (or 3-D); every plane is denoised on its own.  A pixel becomes the weighted mean of the pixels within
    ``search_radius`` (1 .. 10) of it; a candidate's weight falls off as ``exp(-max(d - 2 sigma**2, 0) / h**2)`` with ``d`` the mean
    squared difference of the two ``(2 patch_radius + 1)**2`` patches (``patch_radius`` 1 .. 3), quantised to a table of 256 weights.

    ``h`` (grey levels, 0.5 .. 255; keyword-only and required: there is no honest default) is the strength: larger smooths more.
    ``sigma`` is the noise level in grey levels; with it given, scikit-image's guidance is ``h`` of about 0.6 to 0.8 ``sigma``, without it
    somewhat above the noise level.  Nothing here chooses ``h``: ``util.estimate_noise(...).sigma`` measures a pair's noise level, and
    passing it on as ``sigma`` is the caller's step.  Returns uint8 of the shape of ``lr`` (a device tensor for ``to_numpy=False``).
    One launch (``pssr_nlm_u8``) for all planes."""
    p, s, qmul, qshift, bias = _check_nlm(h, sigma, patch_radius, search_radius)
    lr, batched = _baseline_image("nlm_denoise", lr)
    out = ops.nlm_u8(_baseline_device("nlm_denoise", lr), p, s, qmul, qshift, bias)
    if not batched:
        out = out[0]
    return out.cpu().numpy() if to_numpy else out


def _spectral_inputs(who: str, named, block):
    """The checks of the images and the block side that ``frc``, ``decorr`` and their sectorial forms share, in their order (``named``:
    ``(name, image)`` pairs) -> ``(device tensors [N, C, H, W], batched, block, device)``."""
    tensors = []
    for name, t in named:
        host = torch.is_tensor(t) and not t.is_cuda
        if not torch.is_tensor(t):
            t = torch.as_tensor(np.ascontiguousarray(t))
        if t.dtype != torch.uint8:
            raise TypeError(f"{who} takes uint8 images; {name} is {t.dtype}")
        if host:
            raise RuntimeError(f"pssr2_amd.util.{who} runs on an MI355X (HIP) device only; there is no CPU fallback")
        tensors.append(t)
    a = tensors[0]
    if len(tensors) == 2:
        if a.shape != tensors[1].shape or a.dim() not in (2, 3, 4):
            raise ValueError("a and b must have the same shape, [images, planes, height, width] or one [planes, height, width] or [height, width] "
                             f"pair. Shapes are {tuple(a.shape)} and {tuple(tensors[1].shape)} respectively.")
    elif a.dim() not in (2, 3, 4):
        raise ValueError(f"img must be [images, planes, height, width] or one [planes, height, width] or [height, width] image. The shape is {tuple(a.shape)}.")
    batched = a.dim() == 4
    tensors = [t.reshape((1,) * (4 - t.dim()) + tuple(t.shape)) for t in tensors]
    n_img, c, H, W = tensors[0].shape
    if min(n_img, c) < 1 or min(H, W) < ops.FRC_MIN_BLOCK:
        raise ValueError(f"{who} needs at least one plane of at least {ops.FRC_MIN_BLOCK}x{ops.FRC_MIN_BLOCK} pixels. The shape is {tuple(tensors[0].shape)}.")
    if block is None:
        block = min(H, W, ops.FRC_MAX_BLOCK) // 2 * 2
    elif isinstance(block, bool) or not isinstance(block, (int, np.integer)) or block % 2 or not ops.FRC_MIN_BLOCK <= block <= min(H, W, ops.FRC_MAX_BLOCK):
        raise ValueError(f"block must be an even int from {ops.FRC_MIN_BLOCK} to {min(H, W, ops.FRC_MAX_BLOCK)} (the smaller side, at most "
                         f"{ops.FRC_MAX_BLOCK}). Given {block!r}.")
    if not (any(t.is_cuda for t in tensors) or torch.cuda.is_available()):
        raise RuntimeError(f"pssr2_amd.util.{who} needs an MI355X (HIP) device, and none is available; there is no CPU fallback")
    dev = next((t.device for t in tensors if t.is_cuda), "cuda")
    return [t.to(dev) for t in tensors], batched, int(block), dev


FRC = namedtuple("FRC", "curve freq resolution crossed block")


def _frc_resolve(sums, n: int, threshold: float, smooth: int, pixel_size: float):
    """``(curve, resolution, crossed)`` of one item from the ring sums of its planes and blocks (``sums``: float64 [..., n // 2 + 1, 3],
    the layout of ``pssr_frc_rings_u8``; every leading axis pools), in exactly the expressions of step 5 of include/pssr_mi355.h: the
    sums add ring by ring, ``smooth = k`` gives ring ``r >= 1`` the sums of rings ``max(1, r - k) .. min(R, r + k)`` (ring 0 stays alone),
    ``frc[r] = Sab / sqrt(Saa Sbb)`` (0 where ``Saa Sbb <= 0``), the first ``r >= 1`` below ``threshold`` is crossed at
    ``r* = (r - 1) + (frc[r-1] - threshold) / (frc[r-1] - frc[r])`` (``r* = 1`` where ring 0 lies below the threshold too) and
    ``resolution = pixel_size n / r*``; without a crossing the resolution is the sampling limit ``2 pixel_size``.  No device involved."""
    R = n // 2
    pooled = np.asarray(sums, dtype=np.float64).reshape(-1, R + 1, 3).sum(axis=0)
    rings = pooled.copy()
    for r in range(1, R + 1):
        rings[r] = pooled[max(1, r - smooth):min(R, r + smooth) + 1].sum(axis=0)
    curve = np.zeros(R + 1, dtype=np.float64)
    for r in range(R + 1):
        sab, saa, sbb = (float(v) for v in rings[r])
        if saa * sbb > 0:
            curve[r] = sab / math.sqrt(saa * sbb)
    for r in range(1, R + 1):
        if curve[r] < threshold:
            before, here = float(curve[r - 1]), float(curve[r])
            r_star = (r - 1) + (before - threshold) / (before - here) if before >= threshold else 1.0
            return curve, (pixel_size * n / r_star if r_star > 0 else math.inf), True
    return curve, 2.0 * pixel_size, False


def frc(a, b, *, block=None, window: str = "hann", threshold: float = 1 / 7, smooth: int = 0, pixel_size: float = 1.0, to_numpy: bool = True):
    r"""Fourier ring correlation of two images of one field: down to which detail size they agree -- a prediction against its ground truth,
    or two predictions of independent acquisitions.  ``a``, ``b``: uint8 arrays or device tensors of the same shape [N, C, H, W] (or one
    [C, H, W] or [H, W] pair).  Each plane is cut into the centred grid of ``block x block`` blocks (``block`` even, 16 .. 1024;
    ``None``: the largest even side that fits, one block per plane up to 1024 pixels), each block is windowed (``"hann"``, or ``"none"``)
    and transformed, and the two spectra are correlated ring by ring of spatial frequency; an item's planes and blocks pool their sums
    (include/pssr_mi355.h has the definitions).  Returns ``FRC(curve, freq, resolution, crossed, block)``:

    * ``curve``: float64 [N, block // 2 + 1], the correlation of ring ``r``; ``freq``: float64 [block // 2 + 1], ``r / block`` in cycles per
      pixel; ``smooth=k`` pools rings ``r - k .. r + k`` first (never ring 0);
    * ``resolution``: float64 [N], ``pixel_size * block / r*`` at the first crossing ``r*`` of ``threshold`` (1/7 by convention), linearly
      interpolated between rings; ``crossed``: bool [N], ``False`` where the curve never falls below the threshold, and the resolution is
      then the sampling limit ``2 * pixel_size``.

    One sums launch for the whole batch (``pssr_frc_rings_u8``: two matrix products per block on the f32-input MFMA, ring sums in float64 in
    a fixed order) and one copy of the sums to the host; the curve and the crossing are Python floats.  A pair without the batch axis gets
    ``curve`` [block // 2 + 1] and scalars.  ``to_numpy=False`` leaves ``curve`` on the device."""
    if window not in ops.FRC_WINDOWS:
        raise ValueError(f"window must be one of {ops.FRC_WINDOWS}. Given {window!r}.")
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)) or not 0 < threshold < 1:
        raise ValueError(f"threshold must be a number inside (0, 1). Given {threshold!r}.")
    if isinstance(smooth, bool) or not isinstance(smooth, (int, np.integer)) or smooth < 0:
        raise ValueError(f"smooth must be a non-negative int (rings pooled on either side). Given {smooth!r}.")
    if isinstance(pixel_size, bool) or not isinstance(pixel_size, (int, float, np.integer, np.floating)) or not pixel_size > 0:
        raise ValueError(f"pixel_size must be a positive number. Given {pixel_size!r}.")
    (a, b), batched, block, dev = _spectral_inputs("frc", (("a", a), ("b", b)), block)
    n_img, smooth = a.shape[0], int(smooth)
    sums = ops.frc_rings_u8(a, b, block, window).cpu().numpy().reshape(n_img, -1, block // 2 + 1, 3)
    items = [_frc_resolve(sums[i], block, float(threshold), smooth, float(pixel_size)) for i in range(n_img)]
    curve = np.stack([it[0] for it in items])
    resolution = np.array([it[1] for it in items], dtype=np.float64)
    crossed = np.array([it[2] for it in items], dtype=bool)
    freq = np.arange(block // 2 + 1, dtype=np.float64) / block
    if not batched:
        curve, resolution, crossed = curve[0], float(resolution[0]), bool(crossed[0])
    return FRC(curve if to_numpy else torch.from_numpy(curve).to(dev), freq, resolution, crossed, block)


SectorFRC = namedtuple("SectorFRC", "curve freq resolution crossed angles anisotropy block")


def _check_sectors(sectors):
    if isinstance(sectors, bool) or not isinstance(sectors, (int, np.integer)) or not 1 <= sectors <= ops.FRC_MAX_SECTORS:
        raise ValueError(f"sectors must be an int from 1 to {ops.FRC_MAX_SECTORS}. Given {sectors!r}.")


def _frc_resolve_sector(sums, pop, n: int, threshold: float, smooth: int, pixel_size: float):
    """``_frc_resolve`` for one sector (step S5 of include/pssr_mi355.h): ``sums`` float64 [..., n // 2 + 1, 3], the sector's cells, every
    leading axis pooled; ``pop`` [n // 2 + 1], the sector's populations.  ``smooth = k`` pools sums and populations of rings
    ``max(1, r - k) .. min(R, r + k)``; a cell whose pooled population is 0 has the curve value NaN and is skipped: the search walks the
    populated rings ``r >= 1`` in ascending order, and the first one below ``threshold`` is crossed at
    ``r* = r_prev + (c_prev - threshold) / (c_prev - c_r) (r - r_prev)``, ``r_prev`` the populated ring before it (ring 0 counts); ``r* = 1``
    where that ring lies below the threshold too, or where there is none (ring 0 is populated in sector 0 alone)."""
    R = n // 2
    pooled = np.asarray(sums, dtype=np.float64).reshape(-1, R + 1, 3).sum(axis=0)
    pop = np.asarray(pop, dtype=np.int64)
    rings, count = pooled.copy(), pop.copy()
    for r in range(1, R + 1):
        lo, hi = max(1, r - smooth), min(R, r + smooth) + 1
        rings[r], count[r] = pooled[lo:hi].sum(axis=0), pop[lo:hi].sum()
    curve = np.full(R + 1, math.nan, dtype=np.float64)
    for r in range(R + 1):
        if count[r] > 0:
            sab, saa, sbb = (float(v) for v in rings[r])
            curve[r] = sab / math.sqrt(saa * sbb) if saa * sbb > 0 else 0.0
    prev = 0 if count[0] > 0 else None
    for r in range(1, R + 1):
        if count[r] == 0:
            continue
        if curve[r] < threshold:
            r_star = 1.0
            if prev is not None and curve[prev] >= threshold:
                before, here = float(curve[prev]), float(curve[r])
                r_star = prev + (before - threshold) / (before - here) * (r - prev)
            return curve, (pixel_size * n / r_star if r_star > 0 else math.inf), True
        prev = r
    return curve, 2.0 * pixel_size, False


def frc_sectors(a, b, *, sectors: int = 2, block=None, window: str = "hann", threshold: float = 1 / 7, smooth: int = 0, pixel_size: float = 1.0,
                to_numpy: bool = True):
    r"""``frc`` per direction: every ring is cut into ``sectors`` (1 .. 16) sectors of the direction of the frequency vector, sector ``s``
    centred on ``s * 180 / sectors`` degrees, and each sector gets its own curve and crossing.  Sector 0 holds frequencies along ``x``
    (detail along a scan line); with an even count, sector ``sectors // 2`` holds frequencies along ``y`` (detail from line to line).  Inputs,
    ``block``, ``window``, ``threshold``, ``smooth`` and ``pixel_size`` are ``frc``'s (include/pssr_mi355.h, "Directional resolution", has the
    definitions).  Returns ``SectorFRC(curve, freq, resolution, crossed, angles, anisotropy, block)``:

    * ``curve``: float64 [N, sectors, block // 2 + 1], NaN in a (ring, sector) cell that holds no coefficient (low rings of many sectors);
      such cells are skipped by the crossing search, which interpolates between the populated rings on either side; ``freq`` as in ``frc``;
    * ``resolution``, ``crossed``: [N, sectors]; ``angles``: float64 [sectors], the sectors' directions in degrees;
    * ``anisotropy``: float64 [N], the largest over the smallest sector resolution of the item (1: isotropic).

    One sums launch for the whole batch (``pssr_frc_sectors_u8``: the transform of ``frc``, and a fixed-order reduction over (ring, sector)
    cells); ``sectors=1`` is ``frc``.  A pair without the batch axis loses the leading axis everywhere."""
    if window not in ops.FRC_WINDOWS:
        raise ValueError(f"window must be one of {ops.FRC_WINDOWS}. Given {window!r}.")
    _check_sectors(sectors)
    if isinstance(threshold, bool) or not isinstance(threshold, (int, float, np.integer, np.floating)) or not 0 < threshold < 1:
        raise ValueError(f"threshold must be a number inside (0, 1). Given {threshold!r}.")
    if isinstance(smooth, bool) or not isinstance(smooth, (int, np.integer)) or smooth < 0:
        raise ValueError(f"smooth must be a non-negative int (rings pooled on either side). Given {smooth!r}.")
    if isinstance(pixel_size, bool) or not isinstance(pixel_size, (int, float, np.integer, np.floating)) or not pixel_size > 0:
        raise ValueError(f"pixel_size must be a positive number. Given {pixel_size!r}.")
    (a, b), batched, block, dev = _spectral_inputs("frc_sectors", (("a", a), ("b", b)), block)
    n_img, S, smooth = a.shape[0], int(sectors), int(smooth)
    sums = ops.frc_sectors_u8(a, b, block, S, window).cpu().numpy().reshape(n_img, -1, block // 2 + 1, S, 3)
    pop = ops.frc_sector_pop(block, S)
    items = [[_frc_resolve_sector(sums[i, :, :, s], pop[:, s], block, float(threshold), smooth, float(pixel_size)) for s in range(S)]
             for i in range(n_img)]
    curve = np.stack([np.stack([it[0] for it in item]) for item in items])
    resolution = np.array([[it[1] for it in item] for item in items], dtype=np.float64)
    crossed = np.array([[it[2] for it in item] for item in items], dtype=bool)
    anisotropy = resolution.max(axis=1) / resolution.min(axis=1)
    freq = np.arange(block // 2 + 1, dtype=np.float64) / block
    angles = np.arange(S, dtype=np.float64) * 180.0 / S
    if not batched:
        curve, resolution, crossed, anisotropy = curve[0], resolution[0], crossed[0], float(anisotropy[0])
    return SectorFRC(curve if to_numpy else torch.from_numpy(curve).to(dev), freq, resolution, crossed, angles, anisotropy, block)


Decorr = namedtuple("Decorr", "resolution found peak amplitude curves freq block")
DECORR_POOLS = ("item", "block")     # decorr's ``pool``
DECORR_MAX_FILTERS = 64
DECORR_MIN_DROP = 5e-4               # how far a curve must fall behind its maximum for that to count as a peak
DECORR_LAST_SIGMA = 0.15             # the weakest high-pass of the family

_DECORR_POP = {}                     # n -> float64 [n // 2 + 1], the ring populations of the full spectrum


def _decorr_pop(n: int):
    if n not in _DECORR_POP:
        R = n // 2
        f = np.arange(n, dtype=np.int64)
        f = np.where(f <= R, f, f - n)
        q = f[:, None] ** 2 + f[None, :] ** 2
        r = np.floor(np.sqrt(q.astype(np.float64)) + 0.5).astype(np.int64)
        r += (q > r * r + r).astype(np.int64) - ((r > 0) & (q < r * r - r + 1)).astype(np.int64)     # (isqrt(4 q) + 1) // 2 whatever the float root did
        _DECORR_POP[n] = np.bincount(r[r <= R], minlength=R + 1).astype(np.float64)
    return _DECORR_POP[n]


def _decorr_peak(d):
    """Step 5 of include/pssr_mi355.h on one curve ``d[0 .. R]`` -> ``(ring, refined position, amplitude)`` or ``None``."""
    R = len(d) - 1
    for e in range(R, 1, -1):
        i = 1 + int(np.argmax(d[1:e + 1]))                     # the first of equal maxima
        if i == e:
            continue
        if d[i] - d[i:e + 1].min() >= DECORR_MIN_DROP:
            before, here, after = float(d[i - 1]), float(d[i]), float(d[i + 1])
            bend = before - 2.0 * here + after
            return i, (i + 0.5 * (before - after) / bend if bend < 0 else float(i)), here
    return None


def _decorr_resolve(sums, n: int, filters: int, pixel_size: float, pop=None):
    """``(resolution, found, peak, amplitude, curves, chosen)`` of one item (or one block) from the ring sums of the spectra it pools
    (``sums``: float64 [..., n // 2 + 1, 2], the layout of ``pssr_decorr_rings_u8``; every leading axis pools), in exactly the expressions of
    steps 3 - 7 of include/pssr_mi355.h: the sums add ring by ring, ``d_g(r) = sum_{1..r} g A / sqrt(sum_{1..R} g^2 P . M(r))`` for the
    unfiltered curve and the ``filters`` high-passed ones, the peak rule on each, the largest refined peak position ``p*`` (``chosen``: the
    index of its curve, ``None`` without one; ``peak`` is then NaN and ``amplitude`` 0) and ``resolution = pixel_size n / p*``, or the
    sampling limit ``2 pixel_size`` where no curve peaks.  ``pop``: the coefficients per ring of one spectrum, [n // 2 + 1] (``None``: the
    whole rings; ``decorr_sectors`` gives a sector's).  No device involved."""
    R = n // 2
    flat = np.asarray(sums, dtype=np.float64).reshape(-1, R + 1, 2)
    pooled = flat.sum(axis=0)
    A, P = pooled[1:, 0], pooled[1:, 1]
    M = flat.shape[0] * np.cumsum((_decorr_pop(n) if pop is None else np.asarray(pop, dtype=np.float64))[1:])
    rho2 = (np.arange(1, R + 1, dtype=np.float64) / R) ** 2

    def curve(g):
        den = np.sqrt(float((g * g * P).sum()) * M)
        d = np.zeros(R + 1, dtype=np.float64)
        np.divide(np.cumsum(g * A), den, out=d[1:], where=den > 0)
        return d

    curves = [curve(np.ones(R, dtype=np.float64))]
    peaks = [_decorr_peak(curves[0])]
    if filters > 0:
        s0 = min(2.0 * R / peaks[0][0], float(R)) if peaks[0] else float(R)
        for j in range(filters):
            s = s0 * (DECORR_LAST_SIGMA / s0) ** (j / (filters - 1)) if filters > 1 else s0
            curves.append(curve(1.0 - np.exp(-2.0 * s * s * rho2)))
            peaks.append(_decorr_peak(curves[-1]))
    chosen = None
    for k, pk in enumerate(peaks):
        if pk is not None and (chosen is None or pk[1] > peaks[chosen][1]):
            chosen = k
    curves = np.stack(curves)
    if chosen is None:
        return 2.0 * pixel_size, False, math.nan, 0.0, curves, None
    _, p, amplitude = peaks[chosen]
    return pixel_size * n / p, True, p, amplitude, curves, chosen


def _decorr_assemble(sums, n_img: int, c: int, nby: int, nbx: int, n: int, filters: int, pool: str, pixel_size: float, batched: bool, pop=None):
    """The host half of ``decorr``: ``_decorr_resolve`` per item (``pool="item"``) or per block of the grid (``"block"``; the item's planes
    pool either way) of the ring sums of a batch, and the result arrays in their shapes.  ``pop`` goes to ``_decorr_resolve``."""
    R = n // 2
    sums = np.asarray(sums, dtype=np.float64).reshape(n_img, c, nby * nbx, R + 1, 2)
    if pool == "item":
        items = [_decorr_resolve(sums[i], n, filters, pixel_size, pop) for i in range(n_img)]
        shape = (n_img,)
    else:
        items = [_decorr_resolve(sums[i, :, k], n, filters, pixel_size, pop) for i in range(n_img) for k in range(nby * nbx)]
        shape = (n_img, nby, nbx)
    resolution = np.array([it[0] for it in items], dtype=np.float64).reshape(shape)
    found = np.array([it[1] for it in items], dtype=bool).reshape(shape)
    peak = np.array([it[2] for it in items], dtype=np.float64).reshape(shape)
    amplitude = np.array([it[3] for it in items], dtype=np.float64).reshape(shape)
    curves = np.stack([it[4] for it in items]).reshape(shape + (filters + 1, R + 1))
    if not batched:
        resolution, found, peak, amplitude, curves = resolution[0], found[0], peak[0], amplitude[0], curves[0]
        if pool == "item":
            resolution, found, peak, amplitude = float(resolution), bool(found), float(peak), float(amplitude)
    return resolution, found, peak, amplitude, curves


def decorr(img, *, block=None, window: str = "hann", filters: int = 10, pool: str = "item", pixel_size: float = 1.0, to_numpy: bool = True):
    r"""Resolution of one image by decorrelation analysis (Descloux, Grußmayer, Radenovic, Nature Methods 2019): the figure ``frc`` gives
    for a pair, from a single image, with no threshold and no calibration.  ``img``: a uint8 array or device tensor [N, C, H, W] (or one
    [C, H, W] or [H, W] image).  Each plane is cut into the centred grid of ``block x block`` blocks as in ``frc`` (``None``: the largest
    even side that fits, at most 1024), each block loses its own mean, is windowed and transformed, and its spectrum is correlated with its
    normalised self inside a growing disc; the position of that curve's peak, pushed outwards by a family of ``filters`` (0 .. 64) Gaussian
    high-passes, is the cut-off (include/pssr_mi355.h has the definitions).  ``pool="item"`` pools the planes and blocks of an item;
    ``pool="block"`` keeps every block of the grid apart (the planes of an item still pool) and returns a local-resolution map.
    Returns ``Decorr(resolution, found, peak, amplitude, curves, freq, block)``:

    * ``resolution``: float64 [N] (``"block"``: [N, nby, nbx]), ``pixel_size * block / peak``; ``found``: bool of the same shape, ``False``
      where no curve has a peak -- nothing below the sampling limit separates signal from noise -- and the resolution is then
      ``2 * pixel_size``; ``peak``: the refined peak position in rings (NaN where none), ``amplitude``: the curve's value there (0 where none);
    * ``curves``: float64 [N, filters + 1, block // 2 + 1] (``"block"``: [N, nby, nbx, filters + 1, block // 2 + 1]), the unfiltered curve
      first; ``freq``: float64 [block // 2 + 1], ``r / (block * pixel_size)``.

    One sums launch sequence for the whole batch (``pssr_decorr_rings_u8``: the transform as two matrix products per block on the f32-input
    MFMA, two ring sums in float64 in a fixed order -- every filter is a weight per ring of those two sums, so no filter costs a transform)
    and one copy of the sums to the host; the curves and peaks are computed there.  An image without the batch axis gets ``curves``
    [filters + 1, block // 2 + 1] and scalars (maps [nby, nbx]).  ``to_numpy=False`` leaves ``curves`` on the device."""
    if window not in ops.FRC_WINDOWS:
        raise ValueError(f"window must be one of {ops.FRC_WINDOWS}. Given {window!r}.")
    if isinstance(filters, bool) or not isinstance(filters, (int, np.integer)) or not 0 <= filters <= DECORR_MAX_FILTERS:
        raise ValueError(f"filters must be an int from 0 to {DECORR_MAX_FILTERS} (high-passed curves beside the plain one). Given {filters!r}.")
    if pool not in DECORR_POOLS:
        raise ValueError(f"pool must be one of {DECORR_POOLS}. Given {pool!r}.")
    if isinstance(pixel_size, bool) or not isinstance(pixel_size, (int, float, np.integer, np.floating)) or not pixel_size > 0:
        raise ValueError(f"pixel_size must be a positive number. Given {pixel_size!r}.")
    (a,), batched, block, dev = _spectral_inputs("decorr", (("img", img),), block)
    (n_img, c, H, W), filters, pixel_size = a.shape, int(filters), float(pixel_size)
    sums = ops.decorr_rings_u8(a, block, window).cpu().numpy()
    resolution, found, peak, amplitude, curves = _decorr_assemble(sums, n_img, c, H // block, W // block, block, filters, pool, pixel_size, batched)
    freq = np.arange(block // 2 + 1, dtype=np.float64) / (block * pixel_size)
    return Decorr(resolution, found, peak, amplitude, curves if to_numpy else torch.from_numpy(curves).to(dev), freq, block)


SectorDecorr = namedtuple("SectorDecorr", "resolution found peak amplitude curves freq angles anisotropy block")


def decorr_sectors(img, *, sectors: int = 2, block=None, window: str = "hann", filters: int = 10, pool: str = "item", pixel_size: float = 1.0,
                   to_numpy: bool = True):
    r"""``decorr`` per direction: the rings cut into ``sectors`` (1 .. 16) sectors as in ``frc_sectors`` (sector 0: frequencies along ``x``),
    and the curves, the peak rule and the filter family of ``decorr`` run on each sector's two sums, with the sector's own coefficient
    counts in the normalisation (include/pssr_mi355.h, "Directional resolution").  Inputs and the other arguments are ``decorr``'s.  Returns
    ``SectorDecorr(resolution, found, peak, amplitude, curves, freq, angles, anisotropy, block)``: the fields of ``Decorr`` with a sector axis
    after the item axis (``pool="block"``: after the item and the two block axes, a directional local-resolution map) -- ``resolution``
    [N, sectors] or [N, nby, nbx, sectors], ``curves`` [N, sectors, filters + 1, block // 2 + 1] -- ``angles`` float64 [sectors] in degrees,
    and ``anisotropy`` [N] (or [N, nby, nbx]), the largest over the smallest sector resolution.  One sums launch sequence for the whole batch
    (``pssr_decorr_sectors_u8``); ``sectors=1`` is ``decorr``.  An image without the batch axis loses the leading axis everywhere."""
    if window not in ops.FRC_WINDOWS:
        raise ValueError(f"window must be one of {ops.FRC_WINDOWS}. Given {window!r}.")
    _check_sectors(sectors)
    if isinstance(filters, bool) or not isinstance(filters, (int, np.integer)) or not 0 <= filters <= DECORR_MAX_FILTERS:
        raise ValueError(f"filters must be an int from 0 to {DECORR_MAX_FILTERS} (high-passed curves beside the plain one). Given {filters!r}.")
    if pool not in DECORR_POOLS:
        raise ValueError(f"pool must be one of {DECORR_POOLS}. Given {pool!r}.")
    if isinstance(pixel_size, bool) or not isinstance(pixel_size, (int, float, np.integer, np.floating)) or not pixel_size > 0:
        raise ValueError(f"pixel_size must be a positive number. Given {pixel_size!r}.")
    (a,), batched, block, dev = _spectral_inputs("decorr_sectors", (("img", img),), block)
    (n_img, c, H, W), S, filters, pixel_size = a.shape, int(sectors), int(filters), float(pixel_size)
    sums = ops.decorr_sectors_u8(a, block, S, window).cpu().numpy()
    pop = ops.frc_sector_pop(block, S)
    parts = [_decorr_assemble(sums[..., s, :], n_img, c, H // block, W // block, block, filters, pool, pixel_size, True, pop[:, s]) for s in range(S)]
    resolution, found, peak, amplitude = (np.stack([p[k] for p in parts], axis=-1) for k in range(4))
    curves = np.stack([p[4] for p in parts], axis=resolution.ndim - 1)
    anisotropy = resolution.max(axis=-1) / resolution.min(axis=-1)
    freq = np.arange(block // 2 + 1, dtype=np.float64) / (block * pixel_size)
    angles = np.arange(S, dtype=np.float64) * 180.0 / S
    if not batched:
        resolution, found, peak, amplitude, curves, anisotropy = resolution[0], found[0], peak[0], amplitude[0], curves[0], anisotropy[0]
        if pool == "item":
            anisotropy = float(anisotropy)
    return SectorDecorr(resolution, found, peak, amplitude, curves if to_numpy else torch.from_numpy(curves).to(dev), freq, angles, anisotropy, block)


def _sort_tiles(name: str):
    """Sort key of tile names ``{sheet}_{tile}_{slice}[.ext]`` (pssr/util.py:110-114): slice first, then tile."""
    if "." not in name:
        name += "."
    parts = name.replace(".", "_").split("_")
    return int(parts[-2]), int(parts[-3])


def reassemble_sheets(pred_path, lr_path, lr_scale: int, overlap: int = 0, margin: int = 0, out_dir: str = "sheets", *, blend: str = "average"):
    r"""Reassembles image sheets from the tiles predicted for a sliding dataset (pssr/util.py:54-108): same arguments, file naming
    and return value.  ``pred_path`` is a directory of tile images or the dict returned by ``predict_images``; the overlap-averaged
    stitching (with ``margin`` trimming) runs on the MI355X (``pssr_patch_tiles_u8``, bit-exact with ``_patch_images`` + the
    uint8 cast).  Multi-frame sheets are written through Pillow (the reference uses tifffile).  ``blend="linear"`` (keyword-only, not in
    the reference) feathers the overlaps as ``predict_sheet(blend="linear")`` does (``pssr_blend_stack_u8``, all slices in one launch)."""
    import glob
    import os
    import numpy as np
    from PIL import Image
    from . import ops
    if blend not in ops.BLENDS:
        raise ValueError(f"blend must be one of {sorted(ops.BLENDS)}. Given {blend!r}.")
    if margin > overlap:
        raise ValueError(f"The value of margin cannot be greater than overlap. Given {margin} and {overlap} respectively.")
    sheet_files = glob.glob(f"{lr_path}/*.tif", recursive=True)
    if len(sheet_files) == 0:
        raise FileExistsError("No files exist in lr_path.")
    if out_dir:
        os.makedirs(out_dir, exist_ok=True)

    def frames(img):       # pssr/data.py:640-647 (_frame_channel, mode "L")
        return np.stack([np.asarray(f.convert("L"), dtype=np.uint8) for f in _iter_frames(img)])

    def _iter_frames(img):
        for i in range(getattr(img, "n_frames", 1)):
            img.seek(i)
            yield img

    outs = []
    for sheet in sheet_files:
        stem = sheet.split("/")[-1].split(".")[0]
        if type(pred_path) is dict:
            files = sorted([f for f in pred_path if "_".join(f.split("_")[:-2]) == stem], key=_sort_tiles)
            batched = np.asarray([np.asarray(pred_path[f]).squeeze() for f in files])
        else:
            files = sorted(glob.glob(f"{pred_path}/{stem}*"), key=_sort_tiles)
            batched = np.asarray([frames(Image.open(f)).squeeze() for f in files])
        lr_shape = frames(Image.open(sheet)).shape
        size = batched.shape[1]
        n_rows = (lr_shape[1] * lr_scale - size) // (size - overlap * lr_scale) + 1
        n_cols = (lr_shape[2] * lr_scale - batched.shape[2]) // (batched.shape[2] - overlap * lr_scale) + 1
        per = n_rows * n_cols
        tiles = torch.as_tensor(np.ascontiguousarray(batched.astype(np.uint8))).cuda()
        if blend == "average":
            image = np.stack([ops.patch_tiles_u8(tiles[i * per:(i + 1) * per, None].contiguous(), n_rows, n_cols, overlap * lr_scale, margin)[0].cpu().numpy()
                              for i in range(batched.shape[0] // per)])
        else:
            n_slices, step = batched.shape[0] // per, size - overlap * lr_scale
            image = ops.blend_stack_u8(tiles[:n_slices * per, None].contiguous(), n_slices, n_rows, n_cols, overlap * lr_scale, margin,
                                       n_rows * step + overlap * lr_scale, n_cols * step + overlap * lr_scale, blend)[:, 0].cpu().numpy()
        if out_dir:
            ims = [Image.fromarray(f) for f in image]
            ims[0].save(f"{out_dir}/{stem}.tif", save_all=len(ims) > 1, append_images=ims[1:])
        else:
            outs.append(image)
    if out_dir is None:
        return outs
