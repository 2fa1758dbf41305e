"""Per-level reference of the SSIM / MS-SSIM + Gaussian-L1 loss (tests/test_loss_ref64.py, tests/test_gpu_loss_levels.py).

Plain torch on the CPU, one function per launch of csrc/loss.hip: `pool` is the avg-pool kernel, `level` is one forward launch plus
one backward launch of a level, `weights` is the weights kernel.  `level` and `pool` run in the dtype of their inputs, so the same
code gives the f64 reference and the f32 yardstick the GPU tolerances are measured with (`bound`).  Chained over the pyramid
(`compose`) they are oracle.loss_ref.ssim_loss again, which tests/test_loss_ref64.py asserts.

The window is passed as the f32 taps the kernels receive (oracle.loss_ref.gauss_1d) and cast to the working dtype here; the 2-D
window of the L1 term is the f32 outer product of those taps cast afterwards, as oracle.loss_ref.gaussian_l1 forms it.
"""
from __future__ import annotations

import torch
import torch.nn.functional as F

FACTOR = 16.0              # kernel error <= FACTOR * max(E32, 2^-23 max|ref|): the kernels round in another order than torch's f32 conv
EPS32 = 2.0 ** -23


def pool(x):
    """F.avg_pool2d(kernel 2, padding = size % 2) on planes [P, H, W]."""
    return F.avg_pool2d(x[:, None], kernel_size=2, padding=(x.shape[-2] % 2, x.shape[-1] % 2))[:, 0]


def _filter_valid(t, g):
    k = g.numel()
    return F.conv2d(F.conv2d(t, g.view(1, 1, k, 1)), g.view(1, 1, 1, k))


def level(x, y, win, c1, c2, wts, use_ssim, dcoarse=None, l1_coef=0.0):
    """One level on planes x, y [P, H, W] (working dtype = x.dtype); win: 1-D f32 taps; wts [P]; dcoarse [P, HC, WC] or None.

    Returns (sums [P, 2], l1_sum, dx): the per-plane sums of the cs map and of the ssim map over the valid region,
    sum_q |x - y|(q) S(q) with S the zero-padded window mass, and the gradient wrt x of
        sum_p wts[p] sum(map_p) + sum(pool(x) * dcoarse) + l1_coef * l1_sum        (map = ssim map if use_ssim else cs map),
    which is what one pssr_ssim_level_fwd* call plus one pssr_ssim_level_bwd* call compute."""
    dt = x.dtype
    g = win.to(dt)
    k = g.numel()
    xr = x.detach().clone().requires_grad_(True)
    X, Y = xr[:, None], y.detach()[:, None]
    mu1, mu2 = _filter_valid(X, g), _filter_valid(Y, g)
    s1 = _filter_valid(X * X, g) - mu1 * mu1
    s2 = _filter_valid(Y * Y, g) - mu2 * mu2
    s12 = _filter_valid(X * Y, g) - mu1 * mu2
    cs_map = (2 * s12 + c2) / (s1 + s2 + c2)
    ssim_map = ((2 * mu1 * mu2 + c1) / (mu1 * mu1 + mu2 * mu2 + c1)) * cs_map
    cs_sum, ssim_sum = cs_map.flatten(1).sum(1), ssim_map.flatten(1).sum(1)
    win2 = torch.outer(win, win).to(dt)[None, None]
    l1_sum = F.conv2d((X - Y).abs(), win2, padding=k // 2).sum()
    obj = (torch.as_tensor(wts, dtype=dt) * (ssim_sum if use_ssim else cs_sum)).sum()
    if dcoarse is not None:
        obj = obj + (pool(xr) * dcoarse.to(dt)).sum()
    if l1_coef:
        obj = obj + l1_coef * l1_sum
    (dx,) = torch.autograd.grad(obj, xr)
    return torch.stack([cs_sum, ssim_sum], 1).detach(), l1_sum.detach(), dx


def weights(sums, nvalid, level_weights, ms, mix, l1_sum, l1_numel, grad_out=None):
    """The weights kernel in f64.  sums [levels, planes, 2] (cs sum, ssim sum), nvalid [levels], l1_sum a number or None.

    ms:   v_l = relu(mean_l) with mean_l the cs mean (ssim mean at the last level), prod = prod_l v_l^w_l,
          wts[l][p] = d/nvalid_l * go with d = -mix/planes * w_l * prod / v_l, and d = 0 where v_l = 0;
    else: plain SSIM mean of level 0 without relu, wts[0][p] = -mix/planes/nvalid_0 * go (rows above 0 are not defined);
    loss = mix (1 - mean_p) + (1 - mix) l1_sum / l1_numel, l1_coef = (1 - mix) / l1_numel * go; without l1_sum (mix == 1) the
    loss is 1 - mean_p and l1_coef = 0.  Returns (loss, wts [levels, planes], l1_coef) as f64."""
    sums = torch.as_tensor(sums, dtype=torch.float64)
    nvalid = torch.as_tensor(nvalid, dtype=torch.float64)
    lw = torch.as_tensor(level_weights, dtype=torch.float64)
    levels, planes = sums.shape[0], sums.shape[1]
    go = 1.0 if grad_out is None else float(grad_out)
    wts = torch.zeros(levels, planes, dtype=torch.float64)
    if ms:
        mean = torch.stack([sums[l, :, 1 if l == levels - 1 else 0] / nvalid[l] for l in range(levels)])     # [levels, planes]
        v = torch.where(mean > 0, mean, torch.zeros_like(mean))
        prod = torch.prod(v ** lw[:, None], dim=0)
        per_plane = prod
        d = torch.where(v > 0, -mix / planes * lw[:, None] * prod[None] / torch.where(v > 0, v, torch.ones_like(v)), torch.zeros_like(v))
        wts = d / nvalid[:, None] * go
    else:
        per_plane = sums[0, :, 1] / nvalid[0]
        wts[0] = -mix / planes / nvalid[0] * go
    s = per_plane.sum() / planes
    if l1_sum is None:
        return float(1.0 - s), wts, 0.0
    return float(mix * (1.0 - s) + (1.0 - mix) * float(l1_sum) / l1_numel), wts, (1.0 - mix) / l1_numel * go


def compose(x, y, win, c1, c2, level_weights, ms, mix, grad_out=None):
    """pool, level and weights chained as _SSIMLossFunction chains the kernels; x, y [P, H, W].  Returns (loss, dx, means) with
    means [levels, planes] the cs mean of each level (ssim mean at the last)."""
    levels = len(level_weights) if ms else 1
    k = win.numel()
    xs, ys = [x], [y]
    for _ in range(1, levels):
        xs.append(pool(xs[-1])), ys.append(pool(ys[-1]))
    zero = torch.zeros(x.shape[0], dtype=x.dtype)
    fwd = [level(a, b, win, c1, c2, zero, l == levels - 1) for l, (a, b) in enumerate(zip(xs, ys))]
    nvalid = [float((a.shape[-2] - k + 1) * (a.shape[-1] - k + 1)) for a in xs]
    sums = torch.stack([f[0] for f in fwd]).double()
    l1_sum = float(fwd[0][1]) if mix < 1 else None
    loss, wts, l1c = weights(sums, nvalid, level_weights if ms else [1.0], ms, mix, l1_sum, float(x.numel()), grad_out)
    dcoarse = None
    for l in range(levels - 1, -1, -1):
        _, _, dcoarse = level(xs[l], ys[l], win, c1, c2, wts[l].to(x.dtype), l == levels - 1, dcoarse, l1c if l == 0 else 0.0)
    means = torch.stack([sums[l, :, 1 if l == levels - 1 else 0] / nvalid[l] for l in range(levels)])
    return loss, dcoarse, means


def bound(ref64, ref32):
    """(tolerance, denominator) of a max-norm comparison against ref64: E32 = max|ref32 - ref64| is what the same algebra loses
    in f32 on the CPU; the floor is one f32 ulp of the largest reference value."""
    ref64 = torch.as_tensor(ref64, dtype=torch.float64)
    e32 = (torch.as_tensor(ref32).double() - ref64).abs().max().item()
    den = max(e32, EPS32 * ref64.abs().max().item())
    return FACTOR * den, den
