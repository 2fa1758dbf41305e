"""tests/_hist_ref64.py checked without a GPU: the f64 GradHist reference against the reference project's own outputs
(tests/golden/crappifier.npz), against autograd, and the error measures q_h / q_dx against a window that is too tight.

The bound the GPU tests (tests/test_gpu_hist_ops.py) apply is `gpu_bound(q_f32) = 4 * max(q_f32, 1)` with q_f32 the measure of the
same code run in f32.  test_tight_window_* are why the measure exists: a forward that drops every term with sigma (x - c_{j-1}) < -12
(19 e-folds tighter than the kernels' window) is invisible to tests/test_gpu_crappifier.py's worst-bin-over-largest-bin measure and
fails this one by orders of magnitude.  Run with -s for the figures.
"""
from pathlib import Path

import numpy as np
import pytest
import torch

import _hist_ref64 as R

GOLD = Path(__file__).parent / "golden"
FACTOR = 4.0


def gpu_bound(q_f32):
    return FACTOR * max(q_f32, 1.0)


def _case(name, cfg, shape, above_range=True):
    bins, (lo, hi), sigma = cfg
    x = R.case_inputs(shape, cfg, 11, above_range=above_range)
    g = torch.randn(shape[0], bins, generator=torch.Generator().manual_seed(12))
    return x, g, (bins, lo, hi, sigma)


def _measure(x, g, args, h, dx):
    h64, S = R.hist_fwd(x, *args, with_s=True)
    dx64, W, T = R.hist_bwd(x, g, *args, with_w=True)
    return R.q_h(h, h64, S, x[0].numel()), R.q_dx(dx, dx64, W, T), h64


@pytest.mark.parametrize("name", ["def", "wide", "c3"])
def test_reference_reproduces_the_fixture(name):
    """The fixture holds the reference project's f32 outputs: they sit as close to the f64 restatement as the f32 restatement does."""
    d = np.load(GOLD / "crappifier.npz")
    bins, lo, hi, sigma = d[f"{name}_cfg"]
    args = (int(bins), float(lo), float(hi), float(sigma))
    x, g = torch.tensor(d[f"{name}_x"]), torch.tensor(d[f"{name}_g"])
    qh, qd, _ = _measure(x, g, args, torch.tensor(d[f"{name}_h"]), torch.tensor(d[f"{name}_dx"]))
    qh32, qd32, _ = _measure(x, g, args, R.hist_fwd(x, *args, dtype=torch.float32), R.hist_bwd(x, g, *args, dtype=torch.float32))
    print(f"{name}: fixture q_h {qh:.3f} q_dx {qd:.3f}; f32 restatement q_h {qh32:.3f} q_dx {qd32:.3f}")
    assert qh <= gpu_bound(qh32) and qd <= gpu_bound(qd32), (qh, qh32, qd, qd32)


@pytest.mark.parametrize("name,cfg,shape", R.CASES, ids=R.CASE_IDS)
def test_f32_restatement_figures(name, cfg, shape):
    """q of the f32 restatement on the CPU for every configuration of the GPU tests, printed; finite is all that is asserted (the
    GPU tests measure their own yardstick on the device)."""
    x, g, args = _case(name, cfg, shape)
    qh, qd, _ = _measure(x, g, args, R.hist_fwd(x, *args, dtype=torch.float32), R.hist_bwd(x, g, *args, dtype=torch.float32))
    x, g, args = _case(name, cfg, shape, above_range=False)
    _, qd_in, _ = _measure(x, g, args, R.hist_fwd(x, *args, dtype=torch.float32), R.hist_bwd(x, g, *args, dtype=torch.float32))
    print(f"{name}: f32 restatement q_h {qh:.3f} q_dx {qd_in:.3f} (with the planted pixels above the last centre: {qd:.3f})")
    assert np.isfinite(qh) and np.isfinite(qd) and np.isfinite(qd_in)


@pytest.mark.parametrize("name,cfg,shape", [c for c in R.CASES if c[0] in ("def-1320", "wide-3ch", "ragged-300")],
                         ids=["def-1320", "wide-3ch", "ragged-300"])
def test_tight_window_fails_the_new_bound_and_passes_the_old(name, cfg, shape):
    x, g, args = _case(name, cfg, shape, above_range=False)
    qh32, qd32, h64 = _measure(x, g, args, R.hist_fwd(x, *args, dtype=torch.float32), R.hist_bwd(x, g, *args, dtype=torch.float32))
    h_mut = R.hist_fwd(x, *args, drop_below=12.0)
    dx_mut = R.hist_bwd(x, g, *args, drop_below=12.0)
    qh, qd, _ = _measure(x, g, args, h_mut, dx_mut)
    old = R.old_metric(h_mut, h64)
    print(f"{name}: tight window q_h {qh:.3g} (bound {gpu_bound(qh32):.3g}) q_dx {qd:.3g} (bound {gpu_bound(qd32):.3g}); "
          f"old measure {old:.3g} (bound 1e-5)")
    assert qh > gpu_bound(qh32), (qh, qh32)
    assert qd > gpu_bound(qd32), (qd, qd32)
    assert old <= 1e-5, old


def test_measures_compare_non_finite_entries_in_kind():
    ref = torch.tensor([[1.0, float("nan"), float("inf")]], dtype=torch.float64)
    tol = torch.ones_like(ref)
    assert R._q(ref.clone(), ref, tol) == 0.0
    assert R._q(torch.tensor([[1.0, 0.0, float("inf")]]), ref, tol) == float("inf")              # NaN answered by a number
    assert R._q(torch.tensor([[1.0, float("nan"), -float("inf")]]), ref, tol) == float("inf")    # the other infinity
    assert R._q(torch.tensor([[float("nan"), float("nan"), float("inf")]]), ref, tol) == float("inf")
    assert R._q(torch.tensor([[3.0, float("nan"), float("inf")]]), ref, tol) == 2.0


def test_non_finite_pixels_follow_torch():
    """A NaN pixel: NaN row, NaN dx, 0 under a clamp that cut it.  -inf adds 1 to bin 0, +inf adds nothing; both have dx = 0."""
    args = (5, -5.0, 5.0, 2.0)
    base = torch.tensor([[0.3, -1.2, 2.5, 4.0], [0.0, 1.0, -3.0, 2.0]])
    g = torch.randn(2, 5, generator=torch.Generator().manual_seed(0))
    h0 = R.hist_fwd(base, *args)
    for v, add0 in ((float("inf"), 0.0), (-float("inf"), 1.0)):
        x = torch.cat([base, torch.tensor([[v], [0.5]])], 1)
        h = R.hist_fwd(x, *args)
        ref = h0[0].clone()
        ref[0] += add0
        assert torch.allclose(h[0], ref, rtol=0, atol=1e-14), (v, h[0], ref)
        assert R.hist_bwd(x, g, *args)[0, -1] == 0
    x = torch.cat([base, torch.tensor([[float("nan")], [0.5]])], 1)
    h = R.hist_fwd(x, *args)
    assert torch.isnan(h[0]).all() and torch.isfinite(h[1]).all()
    dx = R.hist_bwd(x, g, *args)
    assert torch.isnan(dx[0, -1]) and torch.isfinite(dx[0, :-1]).all() and torch.isfinite(dx[1]).all()
    assert R.hist_bwd(x, g, *args, clamp=True)[0, -1] == 0
    assert torch.isnan(R.hist_bwd(x, g, *args, dx_in=torch.ones_like(x))[0, -1])
    # torch's own answer for the clamp
    xt = x.clone().requires_grad_(True)
    (R.hist_fwd(xt.clamp(0, 255), *args)[1] * g[1]).sum().backward()
    assert xt.grad[0, -1] == 0


class _Hist(torch.autograd.Function):
    @staticmethod
    def forward(ctx, x, args):
        ctx.save_for_backward(x)
        ctx.args = args
        return R.hist_fwd(x, *args)

    @staticmethod
    def backward(ctx, g):
        return R.hist_bwd(ctx.saved_tensors[0], g, *ctx.args), None


def test_gradcheck_of_the_reference():
    """hist_bwd is the derivative of hist_fwd (and hist_fwd itself differentiates), bins = 5, a dozen pixels."""
    args = (5, -4.0, 6.0, 1.5)
    x = (torch.randn(2, 6, dtype=torch.float64, generator=torch.Generator().manual_seed(5)) * 3 + 1).requires_grad_(True)
    assert torch.autograd.gradcheck(lambda t: _Hist.apply(t, args), (x,), eps=1e-6, atol=1e-9, rtol=1e-7)
    assert torch.autograd.gradcheck(lambda t: R.hist_fwd(t, *args), (x,), eps=1e-6, atol=1e-9, rtol=1e-7)


def test_backward_abi_inputs_against_autograd():
    """xb, g_ref, both scales, clamp and accumulate of hist_bwd against autograd through the same composition."""
    args = (7, -3.0, 260.0, 0.4)
    gen = torch.Generator().manual_seed(8)
    xa = torch.rand(2, 9, dtype=torch.float64, generator=gen) * 300 - 20
    xa[0, 0], xa[0, 1] = 0.0, 255.0
    xb, g, g_ref = torch.rand(2, 9, dtype=torch.float64, generator=gen) * 40, torch.randn(2, 7, generator=gen), torch.randn(2, 7, generator=gen)
    dev, g_scale, dx_in = torch.tensor([-0.75]), 0.125, torch.randn(2, 9, dtype=torch.float64, generator=gen)
    xt = xa.clone().requires_grad_(True)
    h = R.hist_fwd(xt.clamp(0, 255) - xb, *args)
    obj = (h * ((g.double() - g_ref.double()) * g_scale * dev.double())).sum() + (xt.clamp(0, 255) * dx_in).sum()
    obj.backward()
    got = R.hist_bwd(xa, g, *args, xb=xb, g_ref=g_ref, dev_scale=dev, g_scale=g_scale, clamp=True, dx_in=dx_in)
    assert torch.allclose(got, xt.grad, rtol=1e-10, atol=1e-12)
    assert (got[(xa < 0) | (xa > 255)] == 0).all() and got[0, 0] != 0 and got[0, 1] != 0


def test_edge_values_sit_on_the_window_ends():
    bins, (lo, hi), sigma = R.DEF
    e = R.edge_values(bins, lo, hi, sigma)
    c = R.centres(bins, lo, hi)
    assert (63 in [j1 - 1 for _, j1 in R.wave_bounds(bins)]) and (bins - 1 in [j1 - 1 for _, j1 in R.wave_bounds(bins)])
    z_hi, z_lo = (e[0].double() - c[63]) * sigma, (e[3].double() - c[63]) * sigma
    assert abs(z_hi - 19) < 1e-4 and abs(z_lo + 31) < 1e-4
    assert e[1] > e[0] > e[2] and e[4] > e[3] > e[5]
    assert R.wave_bounds(300)[-1] == (256, 300) and R.wave_bounds(1) == [(0, 1)] and R.wave_bounds(65) == [(0, 64), (64, 65)]
    x = R.case_inputs((2, 1, 9, 7), R.DEF, 1)
    assert all((x == v).any() for v in e)                       # N = 63 holds every planted value
