"""Bayesian optimisation for ``approximate_crappifier`` when scikit-optimize is absent: numpy only.

``gp_minimize`` keeps the part of ``skopt.gp_minimize``'s interface that ``approximate_crappifier`` uses (arguments ``func``,
``dimensions``, ``n_calls``, ``n_initial_points``, ``random_state``, ``x0``, ``y0``; a result with ``x``, ``fun``, ``x_iters``, ``func_vals``).
It is not a port of skopt and does not reproduce its iterates.

Method: ``n_initial_points`` uniform draws, then per call a Gaussian process on the unit cube -- Matern 5/2 kernel with one length
scale per dimension, targets normalised to zero mean / unit variance, and a noise term because the objective is stochastic (every
call of the crappifier objective draws new noise and a new subset).  Length scales and the noise-to-signal ratio are chosen among
random candidates (the previous choice included) by the marginal likelihood, with the signal variance profiled out in closed form.
The next point maximises the expected improvement over the lowest posterior mean at the points seen so far (with noise, the lowest
observation is biased low), searched over uniform candidates and perturbations of the best points.  Everything random comes from one
``numpy.random.RandomState(random_state)``: the same seed and the same function values give the same iterates.
"""
from __future__ import annotations

import math

import numpy as np

__all__ = ["gp_minimize", "OptimizeResult"]

_N_HYPER, _N_UNIFORM, _N_LOCAL, _XI = 48, 2048, 512, 0.01


class OptimizeResult(dict):
    """Result of ``gp_minimize``: ``x`` (best point seen), ``fun`` (its value), ``x_iters``, ``func_vals``, ``space`` (the bounds)."""
    __getattr__ = dict.get
    __setattr__ = dict.__setitem__


class _Dim:
    def __init__(self, spec):
        if hasattr(spec, "categories") or isinstance(spec, (str, bytes)):
            raise ValueError(f"categorical dimensions are not supported: {spec!r}")
        if hasattr(spec, "low") and hasattr(spec, "high"):
            if getattr(spec, "prior", "uniform") not in (None, "uniform"):
                raise ValueError(f"only uniform priors are supported: {spec!r}")
            low, high = spec.low, spec.high
            is_int = "int" in type(spec).__name__.lower() or (_is_int(low) and _is_int(high) and "real" not in type(spec).__name__.lower())
        else:
            try:
                low, high = spec
            except (TypeError, ValueError):
                raise ValueError(f"a dimension is a (low, high) pair or an object with .low / .high; categorical dimensions are not "
                                 f"supported: {spec!r}") from None
            if not all(_is_int(v) or isinstance(v, (float, np.floating)) for v in (low, high)):
                raise ValueError(f"categorical dimensions are not supported: {spec!r}")
            is_int = _is_int(low) and _is_int(high)
        if not high > low:
            raise ValueError(f"a dimension needs low < high: {spec!r}")
        self.low, self.high, self.is_int = low, high, is_int

    def to_unit(self, v):
        return (float(v) - self.low) / (self.high - self.low)

    def from_unit(self, u):
        v = self.low + u * (self.high - self.low)
        if self.is_int:
            return int(min(max(int(round(v)), self.low), self.high))
        return float(min(max(v, self.low), self.high))


def _is_int(v):
    return isinstance(v, (int, np.integer)) and not isinstance(v, (bool, np.bool_))


def _matern52(a, b, length):
    d = (a[:, None, :] - b[None, :, :]) / length
    r = np.sqrt(5.0 * np.sum(d * d, axis=-1))
    return (1.0 + r + r * r / 3.0) * np.exp(-r)


def _fit(u, z, theta):
    """Cholesky factor, weights, profiled signal variance and log marginal likelihood (up to a constant) for theta = (log length
    scales ..., log noise ratio)."""
    n = len(z)
    length, ratio = np.exp(theta[:-1]), math.exp(theta[-1])
    k = _matern52(u, u, length) + (ratio + 1e-10) * np.eye(n)
    try:
        chol = np.linalg.cholesky(k)
    except np.linalg.LinAlgError:
        return None
    alpha = np.linalg.solve(chol.T, np.linalg.solve(chol, z))
    var = max(float(z @ alpha) / n, 1e-12)
    lml = -0.5 * n * math.log(var) - float(np.sum(np.log(np.diag(chol))))
    return chol, alpha, var, lml


def _posterior(u, fit, theta, cand):
    chol, alpha, var, _ = fit
    ks = _matern52(cand, u, np.exp(theta[:-1]))
    mean = ks @ alpha
    v = np.linalg.solve(chol, ks.T)
    sd = np.sqrt(np.maximum(var * (1.0 - np.sum(v * v, axis=0)), 1e-18))
    return mean, sd


def _norm_cdf(t):
    return 0.5 * (1.0 + np.vectorize(math.erf)(t / math.sqrt(2.0)))


def _expected_improvement(mean, sd, best):
    gap = best - mean - _XI
    t = gap / sd
    return gap * _norm_cdf(t) + sd * np.exp(-0.5 * t * t) / math.sqrt(2.0 * math.pi)


def gp_minimize(func, dimensions, n_calls=100, n_initial_points=10, random_state=None, x0=None, y0=None, **unknown):
    """Minimises the (possibly noisy) ``func(list_of_parameters) -> float`` over ``dimensions``: ``(low, high)`` tuples -- two ints
    make an integer dimension whose values are passed as ``int`` -- or objects with ``.low`` / ``.high`` (skopt's ``Real`` /
    ``Integer`` fit).  ``n_calls`` counts every evaluation of ``func``, the ``n_initial_points`` random ones and those of ``x0``
    included; points of ``x0`` with values in ``y0`` are not evaluated again.  Categorical dimensions and other keywords raise."""
    if unknown:
        raise TypeError(f"gp_minimize() got unexpected keyword arguments {sorted(unknown)}: the built-in minimiser takes n_calls, "
                        "n_initial_points, random_state, x0 and y0")
    dims = [_Dim(d) for d in dimensions]
    if not dims:
        raise ValueError("no dimensions")
    rng = random_state if isinstance(random_state, np.random.RandomState) else np.random.RandomState(random_state)
    nd = len(dims)

    x_iters, func_vals = [], []
    if x0 is not None:
        x0 = [list(x0)] if not isinstance(x0[0], (list, tuple, np.ndarray)) else [list(p) for p in x0]
        y0 = [] if y0 is None else list(np.atleast_1d(y0))
        if len(y0) not in (0, len(x0)):
            raise ValueError("y0 needs one value per point of x0")
        for i, p in enumerate(x0):
            if len(p) != nd:
                raise ValueError("a point of x0 does not match the dimensions")
            x_iters.append(p)
            func_vals.append(float(y0[i]) if y0 else None)
    calls = 0
    for i, p in enumerate(x_iters):
        if func_vals[i] is None:
            func_vals[i] = float(func(p))
            calls += 1
    if n_calls < calls or n_calls <= 0:
        raise ValueError("n_calls must cover the evaluation of x0 and be positive")

    theta = np.concatenate([np.full(nd, math.log(0.3)), [math.log(0.05)]])
    n_random = min(n_initial_points, n_calls - calls)
    while calls < n_calls:
        if n_random > 0:
            unit = rng.uniform(size=nd)
            n_random -= 1
        else:
            u = np.array([[d.to_unit(v) for d, v in zip(dims, p)] for p in x_iters])
            y = np.asarray(func_vals, dtype=np.float64)
            if not np.all(np.isfinite(y)):
                raise ValueError("the objective returned a value that is not finite")
            spread = y.std()
            z = (y - y.mean()) / (spread if spread > 0 else 1.0)
            # hyper-parameters: the previous choice against random candidates, by marginal likelihood
            cands = [theta] + [np.concatenate([rng.uniform(math.log(0.03), math.log(3.0), nd), [rng.uniform(math.log(1e-6), 0.0)]])
                               for _ in range(_N_HYPER)]
            fit = None
            for c in cands:
                f = _fit(u, z, c)
                if f is not None and (fit is None or f[3] > fit[3]):
                    fit, theta = f, c
            if fit is None:
                unit = rng.uniform(size=nd)
            else:
                seen_mean, _ = _posterior(u, fit, theta, u)
                order = np.argsort(seen_mean)
                centres = u[order[:4]]
                local = centres[rng.randint(len(centres), size=_N_LOCAL)] + rng.normal(0.0, 0.05, size=(_N_LOCAL, nd))
                cand = np.clip(np.concatenate([rng.uniform(size=(_N_UNIFORM, nd)), local]), 0.0, 1.0)
                mean, sd = _posterior(u, fit, theta, cand)
                unit = cand[int(np.argmax(_expected_improvement(mean, sd, float(seen_mean.min()))))]
        point = [d.from_unit(float(t)) for d, t in zip(dims, unit)]
        x_iters.append(point)
        func_vals.append(float(func(point)))
        calls += 1

    best = int(np.argmin(func_vals))
    return OptimizeResult(x=list(x_iters[best]), fun=float(func_vals[best]), x_iters=[list(p) for p in x_iters],
                          func_vals=np.asarray(func_vals, dtype=np.float64), space=[(d.low, d.high) for d in dims])
