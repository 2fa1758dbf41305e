"""CPU checks of the float64 AdamW reference, its error bound and the loss-scale policy model (tests/_optim_ref64.py), on the inputs
tests/test_gpu_optim_ops.py uses."""
import numpy as np
import pytest
import torch

import _optim_ref64 as R

SIZES = (1, 5, 1027)


def _f64(*ts):
    return [t.double() for t in ts]


def test_hyper_parameters_are_the_f32_numbers():
    h = R.hyper(beta2=0.999)
    assert h.beta2 == float(np.float32(0.999)) and h.beta2 != 0.999 and h.lr == float(np.float32(1e-3))
    assert all(float(np.float32(v)) == v for cfg in R.CONFIGS.values() for v in cfg.h)


def test_reference_is_the_adamw_recurrence_in_float64():
    """against torch.optim.AdamW run in float64 on the same numbers: equal up to float64 rounding"""
    for name, cfg in R.CONFIGS.items():
        p, gs, m, v = R.inputs(name, 257)
        p, m, v = _f64(p, m, v)
        q = torch.nn.Parameter(p.clone())
        opt = torch.optim.AdamW([q], lr=cfg.h.lr, betas=(cfg.h.beta1, cfg.h.beta2), eps=cfg.h.eps, weight_decay=cfg.h.wd, foreach=False)
        opt.state[q] = dict(step=torch.tensor(float(cfg.step0 - 1)), exp_avg=m.clone(), exp_avg_sq=v.clone())
        for k, g in enumerate(gs):
            q.grad = g.double() * cfg.h.grad_scale
            opt.step()
            p, m, v = R.adamw64(p, g.double(), m, v, cfg.h, cfg.step0 + k)
            st = opt.state[q]
            for got, want in ((q.detach(), p), (st["exp_avg"], m), (st["exp_avg_sq"], v)):
                torch.testing.assert_close(got, want, rtol=1e-12, atol=1e-300)


def test_torch_adamw_in_f32_stays_inside_the_bound():
    """the yardstick: an honest f32 evaluation (another expression order than the kernel's) must fit the bound at every step"""
    worst = [0.0, 0.0, 0.0]
    for name, cfg in R.CONFIGS.items():
        for n in SIZES:
            p, gs, m, v = R.inputs(name, n)
            q = torch.nn.Parameter(p.clone())
            opt = torch.optim.AdamW([q], lr=cfg.h.lr, betas=(cfg.h.beta1, cfg.h.beta2), eps=cfg.h.eps, weight_decay=cfg.h.wd, foreach=False)
            opt.state[q] = dict(step=torch.tensor(float(cfg.step0 - 1)), exp_avg=m.clone(), exp_avg_sq=v.clone())
            for k, g in enumerate(gs):
                st = opt.state[q]
                before = _f64(q.detach().clone(), g, st["exp_avg"].clone(), st["exp_avg_sq"].clone())
                q.grad = g * cfg.h.grad_scale           # a power of two in every configuration: exact
                opt.step()
                want = R.adamw64(*before, cfg.h, cfg.step0 + k)
                bound = R.adamw_bound(*before, cfg.h, cfg.step0 + k)
                r = R.ratios((q.detach(), st["exp_avg"], st["exp_avg_sq"]), want, bound)
                assert max(r) <= 1.0, f"{name} n={n} step {k}: error / bound (p, m, v) = {r}"
                worst = [max(a, b) for a, b in zip(worst, r)]
    print(f"torch.optim.AdamW f32 on the CPU: worst error / bound (p, m, v) = {worst}")
    assert max(worst) > 1e-3, "the bound is orders of magnitude above what f32 does: it would not notice much"


_FIRST_STEP = ("base", "lr0.1", "g_big_scaled")
# where each variant differs by far more than rounding: it must leave the bound there at every size (elsewhere it may coincide with the
# right recurrence: no decay at wd = 0, bias corrections of 1 at step 100 000, eps of 1e-8 beside gradients of order 1 ...)
STRICT = {"l2_decay": _FIRST_STEP, "eps_in_sqrt": ("g_small_eps1e-3",), "no_bc2": _FIRST_STEP, "t_minus_1": _FIRST_STEP,
          "decay_after": ("lr0.1",), "no_grad_scale": _FIRST_STEP}


@pytest.mark.parametrize("variant", list(R.VARIANTS))
def test_wrong_variants_leave_the_bound(variant):
    """each wrong recurrence, evaluated in float64 (no rounding error of its own), is outside the bound for p, m or v on the first
    step of the configurations where it differs at all"""
    left = {}
    for name, cfg in R.CONFIGS.items():
        for n in SIZES:
            p, gs, m, v = R.inputs(name, n)
            args = _f64(p, gs[0], m, v)
            want = R.adamw64(*args, cfg.h, cfg.step0)
            bound = R.adamw_bound(*args, cfg.h, cfg.step0)
            r = R.ratios(R.VARIANTS[variant](*args, cfg.h, cfg.step0), want, bound)
            left[(name, n)] = max(r) > 1.0
            if name in STRICT[variant]:
                assert max(r) > 1.0, f"{variant} stays inside the bound on {name} n={n}: error / bound (p, m, v) = {r}"
    assert any(left.values())
    print(f"{variant} leaves the bound on: {sorted({k[0] for k, out in left.items() if out})}")


def test_the_reference_itself_and_one_f32_ulp_are_inside():
    """ratios() reports 0 for the reference, and a one-ulp change of an f32 result is inside the bound while 64 ulp of p are not"""
    cfg = R.CONFIGS["late"]
    p, gs, m, v = R.inputs("late", 1027)
    args = _f64(p, gs[0], m, v)
    want = R.adamw64(*args, cfg.h, cfg.step0)
    bound = R.adamw_bound(*args, cfg.h, cfg.step0)
    assert R.ratios(want, want, bound) == [0.0, 0.0, 0.0]
    f32 = [w.float() for w in want]
    up = [torch.nextafter(t, torch.full_like(t, float("inf"))) for t in f32]
    assert max(R.ratios(up, want, bound)) <= 1.0
    far = f32[0] * (1 + 64 * 2.0 ** -23)
    assert R.ratios((far, f32[1], f32[2]), want, bound)[0] > 1.0
    nan = f32[0].clone()
    nan[3] = float("nan")
    assert R.ratios((nan, f32[1], f32[2]), want, bound)[0] == float("inf")


@pytest.mark.parametrize("growth,backoff", R.POLICIES)
def test_policy_model_is_lossscaler_step_host(growth, backoff):
    from pssr2_amd.optim import LossScaler
    q = torch.nn.Parameter(torch.ones(4))
    opt = torch.optim.SGD([q], lr=0.0)
    sc = LossScaler(init_scale=2.0 ** 12, growth_factor=growth, backoff_factor=backoff, growth_interval=R.INTERVAL)
    model = R.Scaler(np.float32(2.0 ** 12), 0, 0)
    scales = []
    for finite in R.FINITE_SEQUENCE:
        q.grad = torch.full((4,), 1.0 if finite else float("inf"))
        assert sc.step(opt, [q]) == finite
        model = R.scaler_step(model, finite, growth, backoff, R.INTERVAL)
        assert (sc.scale_value, sc.good_steps, sc.skipped) == (float(model.scale), model.good, model.skipped)
        scales.append(float(model.scale))
    assert model.skipped == 3 and len(set(scales)) >= 3         # the sequence grows and backs off
    assert R.FINITE_SEQUENCE.count(False) == 3 and len(R.FINITE_SEQUENCE) == 12
