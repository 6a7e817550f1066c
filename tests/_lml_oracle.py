"""Test infrastructure: the log marginal likelihood from oracle/gp.py's own
factor (the checker, never the product), and the training sets the LML tests
share.  The reference has no GP: the oracle is the specification."""
import functools

import numpy as np

from oracle import gp as ogp


def lml(X, y, lengthscale, sigma_f2=1.0, sigma_n2=1e-6, jitter=0.0):
    """-1/2 ys.alpha - sum log L_ii - n/2 log 2 pi; NaN where K is not positive definite"""
    try:
        g = ogp.GP(X, y, lengthscale=lengthscale, sigma_f2=sigma_f2, sigma_n2=sigma_n2, jitter=jitter)
    except np.linalg.LinAlgError:
        return float("nan")
    return float(-0.5 * g.ys @ g.alpha - np.log(np.diag(g.L)).sum() - 0.5 * len(g.ys) * np.log(2.0 * np.pi))


def lml_grid(X, y, lengthscale, scales, noises=None, sigma_f2=1.0, sigma_n2=1e-6, jitter=0.0):
    """what BatchEngine.gp_lml_grid returns, from the oracle"""
    X = np.asarray(X, dtype=np.float64)
    ell = np.broadcast_to(np.asarray(lengthscale, dtype=np.float64), (X.shape[1],))
    out = np.array([lml(X, y, s * ell, sigma_f2, sigma_n2 if noises is None else noises[j], jitter)
                    for j, s in enumerate(scales)])
    return out, argmax_finite(out)


def argmax_finite(v):
    ok = np.isfinite(v)
    return int(np.argmax(np.where(ok, v, -np.inf))) if ok.any() else -1


@functools.lru_cache(maxsize=None)
def data(n, d, seed=0):
    """y = sum (x - 0.4)^2 + noise over the unit cube"""
    rng = np.random.default_rng(1000 * n + d + seed)
    X = rng.uniform(size=(n, d))
    y = np.sum((X - 0.4) ** 2, axis=1) + 0.01 * rng.standard_normal(n)
    X.setflags(write=False)
    y.setflags(write=False)
    return X, y


def ard_base(d):
    return np.sqrt(d) * np.linspace(0.8, 1.25, d)
