"""float64 reference of the fused AdamW step and a model of the loss-scale policy (tests/test_optim_ref64.py,
tests/test_gpu_optim_ops.py; the kernels are in csrc/optim.hip).

`adamw64` is the torch.optim.AdamW recurrence -- decoupled weight decay, bias-corrected moments -- on float64 tensors.  The
hyper-parameters are the float32 numbers the entry points receive (`hyper`): float32(0.999), not 0.999.  `adamw_bound` is the
elementwise error an f32 evaluation of one step may have; `VARIANTS` are wrong recurrences that have to leave it.

The error bound.  u = 2^-24 is the unit roundoff of f32.  Every quantity is a sum of terms; c roundings along an expression change it
by at most c u times the sum of the magnitudes of its terms (first order), and the whole bound gets a factor MARGIN = 2:
    m' = b1 m + (1 - b1) gr,  gr = g gs                 roundings: gr, 1 - b1, (1 - b1) gr, b1 m, the sum                  C_M = 5
    v' = b2 v + (1 - b2) gr gr                          roundings: gr (twice: it is squared), 1 - b2, two products, b2 v, the sum
                                                                                                                          C_V = 7
    p' = p (1 - lr wd) - A b1 m / D - A (1 - b1) gr / D,   A = lr / bc1,  D = sqrt(v') / sqrt(bc2) + eps
        p (1 - lr wd): lr wd, 1 - ., the product                                                                              3
        m': as above                                                                                                          5
        D: half of v's 7 (the square root halves a relative error; counted 4), sqrt(v'), sqrt(bc2), the quotient, + eps        8
        m' / D, lr / bc1, A * (.), the final difference                                                                       4
                                                                                                                         C_P = 20
    The bias corrections bc = 1 - b^t are not covered by the count: powf (2 ulp of a number below 1) and the subtraction leave an
    absolute error of up to BC_ULPS u = 3 u in bc, i.e. a RELATIVE error of 3 u / bc -- 2e-4 for b2 = 0.999 at t = 1.  It enters the
    update through A (in full) and through sqrt(bc2) (halved), and gets its own term:  |A m' / D| * (3 u / bc1 + 1.5 u / bc2).
    Underflow: a product below the normal range (g = 1e-25: gr gr = 1e-50) is off by up to the smallest normal number 2^-126 whether
    the hardware flushes or denormalises; that absolute term is added to the bounds of m' and v', and v's reaches D through the square
    root: sqrt(x + d) - sqrt(x) <= sqrt(d).
"""
from __future__ import annotations

from typing import NamedTuple

import numpy as np
import torch

U = 2.0 ** -24
TINY = 2.0 ** -126
MARGIN = 2.0
C_M, C_V, C_P, BC_ULPS = 5, 7, 20, 3


class Hyper(NamedTuple):
    """the f32 arguments of a step, as exact float64 numbers"""
    lr: float
    beta1: float
    beta2: float
    eps: float
    wd: float
    grad_scale: float


def hyper(lr=1e-3, beta1=0.9, beta2=0.999, eps=1e-8, wd=1e-2, grad_scale=1.0) -> Hyper:
    return Hyper(*(float(np.float32(v)) for v in (lr, beta1, beta2, eps, wd, grad_scale)))


def _terms(p, g, m, v, h: Hyper, step: int):
    gr = g * h.grad_scale
    bc1 = 1.0 - h.beta1 ** step
    bc2 = 1.0 - h.beta2 ** step
    m_a, m_b = h.beta1 * m, (1.0 - h.beta1) * gr
    v_a, v_b = h.beta2 * v, (1.0 - h.beta2) * gr * gr
    return gr, bc1, bc2, m_a, m_b, v_a, v_b


def adamw64(p, g, m, v, h: Hyper, step: int):
    """one torch.optim.AdamW step on float64 tensors; step is 1-based.  Returns (p', m', v')."""
    assert p.dtype == g.dtype == m.dtype == v.dtype == torch.float64 and step >= 1
    _, bc1, bc2, m_a, m_b, v_a, v_b = _terms(p, g, m, v, h, step)
    m1, v1 = m_a + m_b, v_a + v_b
    denom = v1.sqrt() / bc2 ** 0.5 + h.eps
    return p * (1.0 - h.lr * h.wd) - (h.lr / bc1) * (m1 / denom), m1, v1


def adamw_bound(p, g, m, v, h: Hyper, step: int):
    """(bound_p, bound_m, bound_v): what an f32 evaluation of the step may differ by from adamw64, elementwise (module docstring)"""
    _, bc1, bc2, m_a, m_b, v_a, v_b = _terms(p, g, m, v, h, step)
    v1 = v_a + v_b
    s_m = m_a.abs() + m_b.abs()
    b_m = C_M * U * s_m + TINY
    b_v = C_V * U * (v_a + v_b) + TINY
    sq_bc2 = bc2 ** 0.5
    denom = v1.sqrt() / sq_bc2 + h.eps
    a = h.lr / bc1
    upd = a * s_m / denom                                               # sum of the magnitudes of the two update terms
    rel_bc = BC_ULPS * U / bc1 + 0.5 * BC_ULPS * U / bc2
    under = a * TINY / denom + upd * (TINY ** 0.5 / sq_bc2) / denom      # m's and v's underflow terms carried into p
    b_p = C_P * U * ((p * (1.0 - h.lr * h.wd)).abs() + upd) + upd * rel_bc + under
    return MARGIN * b_p, MARGIN * b_m, MARGIN * b_v


def ratios(got, want, bound):
    """per quantity, the largest |got - want| / bound (0 / 0 counts as 0; anything non-finite as inf)"""
    out = []
    for g, w, b in zip(got, want, bound):
        err = (g.double() - w).abs()
        r = torch.where(err == 0, torch.zeros_like(err), err / b)
        r = torch.where(torch.isfinite(g.double()) & torch.isfinite(r), r, torch.full_like(r, float("inf")))
        out.append(float(r.max()))
    return out


# ---------------------------------------------------------------------------------------------------------------------
# wrong recurrences: each must leave the bound (tests/test_optim_ref64.py)
def _variant(name):
    def step_fn(p, g, m, v, h: Hyper, step: int):
        gr = g * h.grad_scale
        decay = 1.0 - h.lr * h.wd
        t1, t2 = step, step
        if name == "l2_decay":                  # decay added to the gradient (Adam with L2 regularisation)
            gr, decay = gr + h.wd * p, 1.0
        if name == "no_grad_scale":
            gr = g
        if name == "t_minus_1":
            t1 = t2 = step - 1
        m1 = h.beta1 * m + (1.0 - h.beta1) * gr
        v1 = h.beta2 * v + (1.0 - h.beta2) * gr * gr
        bc1 = 1.0 - h.beta1 ** t1
        bc2 = 1.0 if name == "no_bc2" else 1.0 - h.beta2 ** t2
        if name == "eps_in_sqrt":
            denom = (v1 / bc2 + h.eps).sqrt()
        else:
            denom = v1.sqrt() / bc2 ** 0.5 + h.eps
        with np.errstate(divide="ignore"):
            a = float(np.float64(h.lr) / np.float64(bc1))
        upd = a * (m1 / denom)
        if name == "decay_after":               # the decay applied after the update, to the updated p (see VARIANTS)
            return (p - upd) * decay, m1, v1
        return p * decay - upd, m1, v1
    return step_fn


# "decay_after": subtracting lr wd p_old after the update is the right recurrence in another order -- p - u - lr wd p = p (1 - lr wd) - u
# -- and no input tells the two apart; the wrong form next to it is the decay factor applied to the updated p, which is off by
# lr wd |u|: above the bound only where lr wd is well above BC_ULPS u / bc2 (the "lr0.1" configuration).
VARIANTS = {n: _variant(n) for n in ("l2_decay", "eps_in_sqrt", "no_bc2", "t_minus_1", "decay_after", "no_grad_scale")}


# ---------------------------------------------------------------------------------------------------------------------
# the input sets of the GPU tests
class Config(NamedTuple):
    g_kind: str             # "normal", "zero" (m = v = 0 as well), "tiny" (1e-25), "small" (1e-3 times normal), "big" (1e3 times normal)
    h: Hyper
    step0: int              # step count of the first of the three steps


CONFIGS = {
    "base": Config("normal", hyper(wd=0.05, grad_scale=0.5), 1),
    "lr0.1": Config("normal", hyper(lr=0.1, wd=0.05, grad_scale=0.5), 1),
    "wd0": Config("normal", hyper(wd=0.0), 1),
    "eps1e-3": Config("normal", hyper(wd=0.05, eps=1e-3), 1),
    "beta2_0.99": Config("normal", hyper(wd=0.05, beta2=0.99), 1),
    "late": Config("normal", hyper(wd=0.05), 100000),
    "late_beta2_0.99_eps1e-3_wd0": Config("normal", hyper(wd=0.0, beta2=0.99, eps=1e-3), 100000),
    "g_small_eps1e-3": Config("small", hyper(wd=0.05, eps=1e-3), 1),        # gradients of the size of eps: where eps sits matters
    "g_zero": Config("zero", hyper(wd=0.05), 1),
    "g_tiny": Config("tiny", hyper(wd=0.05), 1),
    "g_tiny_late": Config("tiny", hyper(wd=0.0, eps=1e-3), 100000),
    "g_big_scaled": Config("big", hyper(wd=0.05, grad_scale=1.0 / 4096), 1),
    "g_big_scaled_late_wd0": Config("big", hyper(wd=0.0, beta2=0.99, grad_scale=1.0 / 4096), 100000),
}
STEPS = 3


def inputs(name, n, seed=0):
    """f32 (p, [g of step 0, 1, 2], m, v) of a configuration at size n"""
    cfg = CONFIGS[name]
    gen = torch.Generator().manual_seed(1000 * seed + n % 997 + 7 * sorted(CONFIGS).index(name))
    p = torch.randn(n, generator=gen)
    gs = [torch.randn(n, generator=gen) for _ in range(STEPS)]
    if cfg.g_kind == "zero":
        gs = [torch.zeros(n) for _ in gs]
        m, v = torch.zeros(n), torch.zeros(n)
    else:
        if cfg.g_kind == "tiny":
            gs = [torch.full((n,), 1e-25) * torch.where(g < 0, -1.0, 1.0) for g in gs]
        elif cfg.g_kind in ("big", "small"):
            gs = [g * (1e3 if cfg.g_kind == "big" else 1e-3) for g in gs]
        scale = float(gs[0].abs().max()) * cfg.h.grad_scale
        # moments as earlier steps would have left them: m about a gradient, v about its square (half of them zero: a first step)
        m = torch.randn(n, generator=gen) * scale * (torch.rand(n, generator=gen) < 0.5)
        v = (torch.randn(n, generator=gen) * scale) ** 2 * (m != 0)
    return p, gs, m, v


# ---------------------------------------------------------------------------------------------------------------------
# the loss-scale policy (LossScaler._step_host, amp_update_kernel): the scale is an f32 and is multiplied in f32
class Scaler(NamedTuple):
    scale: np.float32
    good: int
    skipped: int


def scaler_step(s: Scaler, finite: bool, growth, backoff, interval: int) -> Scaler:
    """one step of the policy: a step with a non-finite gradient is skipped, the scale backs off and the run of good steps ends;
    every `interval` good steps in a row the scale grows"""
    if not finite:
        return Scaler(np.float32(s.scale) * np.float32(backoff), 0, s.skipped + 1)
    good = s.good + 1
    return Scaler(np.float32(s.scale) * np.float32(growth) if good % interval == 0 else np.float32(s.scale), good, s.skipped)


FINITE_SEQUENCE = (True, True, True, False, True, True, False, True, True, True, True, False)
POLICIES = ((2.0, 0.5), (1.5, 0.25))        # (growth, backoff), interval 3
INTERVAL = 3
