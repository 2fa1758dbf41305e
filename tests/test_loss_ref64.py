"""The per-level loss reference (tests/_loss_ref64.py) against the whole-loss oracle (oracle/loss_ref.py), on the CPU in f64."""
import math

import pytest
import torch

from _loss_ref64 import compose, level, pool, weights
from oracle import loss_ref as Lr

WIN = Lr.gauss_1d(11, 1.5)
C1, C2 = 0.01 ** 2, 0.03 ** 2


def _pair(shape, seed):
    g = torch.Generator().manual_seed(seed)
    y = torch.rand(*shape, generator=g)
    x = y * 0.7 + 0.3 * torch.rand(*shape, generator=g)
    return x.double(), y.double()


@pytest.mark.parametrize("mix", [0.8, 1.0])
@pytest.mark.parametrize("ms", [True, False])
def test_composition_reproduces_oracle(ms, mix):
    """pool -> level -> weights -> level (backward) over the pyramid is oracle.loss_ref.ssim_loss: both are f64 runs of one algebra."""
    x, y = _pair((2, 1, 161, 173), 3)
    xr = x.clone().requires_grad_(True)
    ref = Lr.ssim_loss(xr, y, mix=mix, ms=ms)
    (gref,) = torch.autograd.grad(ref, xr)
    loss, dx, _ = compose(x.flatten(0, 1), y.flatten(0, 1), WIN, C1, C2, Lr.MS_WEIGHTS, ms, mix)
    assert abs(loss - ref.item()) <= 1e-12 * abs(ref.item())
    assert (dx.view_as(gref) - gref).abs().max().item() <= 1e-12 * gref.abs().max().item()


def test_composition_scales_with_grad_out():
    x, y = _pair((1, 1, 161, 161), 4)
    _, dx1, _ = compose(x[0], y[0], WIN, C1, C2, Lr.MS_WEIGHTS, True, 0.8)
    _, dx2, _ = compose(x[0], y[0], WIN, C1, C2, Lr.MS_WEIGHTS, True, 0.8, grad_out=1.5)
    assert (dx2 - 1.5 * dx1).abs().max().item() <= 1e-14 * dx1.abs().max().item()


def test_anticorrelated_input_is_clamped_with_finite_gradient():
    """x = 1 - y: the cs means of levels 0..3 are negative, the relu zeroes the product, and what is left of the gradient is the L1
    term.  The helper and the oracle agree and stay finite."""
    g = torch.Generator().manual_seed(0)
    y = torch.rand(1, 1, 161, 161, generator=g).double()
    x = 1 - y
    xr = x.clone().requires_grad_(True)
    ref = Lr.ssim_loss(xr, y, mix=0.8)
    (gref,) = torch.autograd.grad(ref, xr)
    loss, dx, means = compose(x[0], y[0], WIN, C1, C2, Lr.MS_WEIGHTS, True, 0.8)
    assert math.isfinite(ref.item()) and torch.isfinite(gref).all() and torch.isfinite(dx).all()
    assert (means[:4, 0] < -0.3).all() and means[4, 0] > 0.5, means
    assert means[0, 0] < means[1, 0] < means[2, 0] < means[3, 0]          # -0.99, -0.95, -0.83, -0.39, then ssim +0.60
    assert abs(loss - ref.item()) <= 1e-12 * abs(ref.item())
    assert (dx.view_as(gref) - gref).abs().max().item() <= 1e-12 * gref.abs().max().item()
    # prod = 0: loss = mix + (1 - mix) * l1, gradient = the L1 term alone
    xl = x.clone().requires_grad_(True)
    l1 = Lr.gaussian_l1(xl, y)
    (gl1,) = torch.autograd.grad(0.2 * l1, xl)
    assert abs(loss - (0.8 + 0.2 * l1.item())) <= 1e-12
    assert (dx.view_as(gl1) - gl1).abs().max().item() <= 1e-12 * gl1.abs().max().item()
    assert 0.89 < loss < 0.91                                              # l1 is close to E|1 - 2y| = 1/2 less the border


def test_pool_pads_odd_sizes_on_the_low_side():
    x = torch.arange(1.0, 16.0, dtype=torch.float64).view(1, 3, 5)
    p = pool(x)
    assert p.shape == (1, 2, 3)
    # rows (pad, 0) and (1, 2); columns (pad, 0), (1, 2), (3, 4)
    assert torch.equal(p[0, 0], torch.tensor([1.0, 2 + 3, 4 + 5], dtype=torch.float64) * 0.25)
    assert torch.equal(p[0, 1], torch.tensor([6.0 + 11, 7 + 8 + 12 + 13, 9 + 10 + 14 + 15], dtype=torch.float64) * 0.25)
    assert pool(torch.ones(2, 1, 1, dtype=torch.float64)).shape == (2, 1, 1)
    assert pool(torch.ones(2, 6, 8, dtype=torch.float64)).shape == (2, 3, 4)


def test_level_runs_in_the_dtype_of_its_inputs():
    x, y = _pair((3, 12, 43), 5)
    wts = torch.tensor([0.75, 0.0, -1.25])
    dc = torch.randn(3, 6, 22, generator=torch.Generator().manual_seed(1))
    s64, l64, d64 = level(x, y, WIN, C1, C2, wts, 0, dc, 0.375)
    s32, l32, d32 = level(x.float(), y.float(), WIN, C1, C2, wts, 0, dc, 0.375)
    assert (s64.dtype, d64.dtype, s32.dtype, d32.dtype) == (torch.float64, torch.float64, torch.float32, torch.float32)
    assert s64.shape == (3, 2) and d64.shape == x.shape
    assert 0 < (s32.double() - s64).abs().max().item() < 1e-4 * s64.abs().max().item()
    assert 0 < (d32.double() - d64).abs().max().item() < 1e-4 * d64.abs().max().item()
    assert abs(l32.item() - l64.item()) < 1e-5 * l64.item()


def test_level_gradient_by_finite_differences():
    """autograd of the helper against central differences of its own sums (pool and L1 terms included)."""
    x, y = _pair((1, 12, 13), 6)
    wts = torch.tensor([0.75], dtype=torch.float64)
    dc = torch.randn(1, 6, 7, generator=torch.Generator().manual_seed(2)).double()
    for use_ssim in (0, 1):
        _, _, dx = level(x, y, WIN, C1, C2, wts, use_ssim, dc, 0.375)

        def objective(xx):
            s, l1, _ = level(xx, y, WIN, C1, C2, wts, use_ssim)
            return (wts * s[:, use_ssim]).sum().item() + (pool(xx) * dc).sum().item() + 0.375 * l1.item()

        for (r, c) in [(0, 0), (5, 6), (11, 12), (6, 0)]:
            h = 1e-6
            xp, xm = x.clone(), x.clone()
            xp[0, r, c] += h
            xm[0, r, c] -= h
            fd = (objective(xp) - objective(xm)) / (2 * h)
            assert abs(fd - dx[0, r, c].item()) < 1e-6 * max(1.0, abs(fd)), (use_ssim, r, c, fd, dx[0, r, c].item())


def test_weights_clamp_and_branches():
    sums = torch.tensor([[[3.0, 9.0], [-2.0, 9.0]], [[9.0, 2.0], [9.0, 1.0]]], dtype=torch.float64)       # [2 levels][2 planes][cs, ssim]
    nvalid, lw = [4.0, 2.0], [0.25, 0.75]
    loss, wts, l1c = weights(sums, nvalid, lw, True, 0.5, 6.0, 12.0, 2.0)
    v00, v10 = 0.75, 1.0
    prod0 = v00 ** 0.25 * v10 ** 0.75
    assert abs(loss - (0.5 * (1 - prod0 / 2) + 0.5 * 6.0 / 12.0)) < 1e-15
    assert abs(wts[0, 0].item() - (-0.5 / 2 * 0.25 * prod0 / v00 / 4.0 * 2.0)) < 1e-15
    assert abs(wts[1, 0].item() - (-0.5 / 2 * 0.75 * prod0 / v10 / 2.0 * 2.0)) < 1e-15
    assert wts[0, 1].item() == 0.0 and wts[1, 1].item() == 0.0            # plane 1: negative cs mean at level 0 zeroes its product
    assert l1c == 0.5 / 12.0 * 2.0
    # no L1 sum (mix == 1): the loss drops the mix factor too
    loss1, wts1, l1c1 = weights(sums, nvalid, lw, True, 1.0, None, 12.0)
    assert abs(loss1 - (1 - prod0 / 2)) < 1e-15 and l1c1 == 0.0
    # plain SSIM: level 0's ssim column, no relu
    loss2, wts2, _ = weights(sums[:1] * torch.tensor([1.0, -1.0]), nvalid[:1], [1.0], False, 0.5, 6.0, 12.0)
    assert abs(loss2 - (0.5 * (1 - (-9.0 / 4 - 9.0 / 4) / 2) + 0.25)) < 1e-15
    assert torch.equal(wts2, torch.full((1, 2), -0.5 / 2 / 4.0, dtype=torch.float64))
