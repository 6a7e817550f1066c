"""surrogate="ssgp" without a GPU: what SharedModel, GpuBatchTechnique and
tune_bandit accept and refuse, and the rule of tests/_ssgp_oracle.py against the
exact GP it approximates.

k^ = (2 sf2 / D) sum_j cos(tau_j(u)) cos(tau_j(u')) has mean k and D terms within 2 sf2 / D of 0:
by Hoeffding all N = n (n + m) entries are within t = sf2 sqrt(8 ln(2 N / 1e-6) / D) of k but with
probability 1e-6 (the draws are fixed by the seed).  With a^ = (K^ + diag)^-1 ys = (ys - Phi w) / diag,
  mu^ - mu = (k^* - k*)^T a^ - k*^T (K + diag)^-1 (K^ - K) a^,  |mu^ - mu| <= t |a^|_1 (1 + |(K + diag)^-1 k*|_1):
an error of the RFF kernel, of order 1 / sqrt(D), not of floating point."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _ssgp_oracle as S  # noqa: E402
from oracle import gp as ogp  # noqa: E402
from uptune_amd import technique as T  # noqa: E402


def test_the_rule_reproduces_the_exact_posterior_mean_at_the_monte_carlo_rate():
    rng = np.random.default_rng(3)
    n, m, d, D, diag, ell = 40, 25, 3, 2048, 1e-2, 0.7
    X, Uc = rng.uniform(size=(n, d)), rng.uniform(size=(m, d))
    y = np.sum((X - 0.4) ** 2, axis=1)
    g = ogp.GP(X, y, lengthscale=ell, sigma_n2=diag)
    mu = g.posterior(Uc)[0]
    mo = S.model(X, y, ell, 1.0, diag, D, seed=11)
    mu_hat = S.features(Uc, ell, mo["Z"], mo["b"], 1.0) @ mo["w"]
    a_hat = (mo["ys"] - S.features(X, ell, mo["Z"], mo["b"], 1.0) @ mo["w"]) / diag
    Ks = np.exp(-0.5 * ogp.sqdist(Uc * g.inv_ell, g.Xs))
    B = np.linalg.solve(g.L @ g.L.T, Ks.T)                               # (K + diag)^-1 k*, [n][m]
    t = np.sqrt(8.0 * np.log(2.0 * n * (n + m) / 1e-6) / D)
    bound = t * np.sum(np.abs(a_hat)) * (1.0 + np.sum(np.abs(B), axis=0))
    assert np.all(np.abs(mu_hat - mu) <= bound)
    # ... and the kernel itself, entry by entry, within t (a wrong amplitude or frequency scale is far outside)
    P, Ps = S.features(X, ell, mo["Z"], mo["b"], 1.0), S.features(Uc, ell, mo["Z"], mo["b"], 1.0)
    K = np.exp(-0.5 * ogp.sqdist(g.Xs, g.Xs))
    assert np.abs(P @ P.T - K).max() <= t and np.abs(Ps @ P.T - Ks).max() <= t


def test_surrogate_ssgp_is_accepted_and_refuses_what_needs_the_exact_gp():
    assert T.SharedModel(surrogate="ssgp", lengthscale=np.array([0.5, 1.0, 2.0])).lengthscale_[2] == 2.0
    m = T.SharedModel(surrogate="ssgp", ssgp_kw={"features": 256}, lengthscale="auto")
    assert m.surrogate == "ssgp" and m.ssgp_kw["features"] == 256 and "ssgp" in T._REFIT
    for acq in ("ei", "ucb"):
        assert T.GpuDifferentialEvolution(surrogate="ssgp", acq=acq, pool=256).model.surrogate == "ssgp"
    assert T.GpuDifferentialEvolution(shared=m, pool=256).surrogate == "ssgp"
    for make in (T.pso_ga_de_bandit, T.bandit_a, T.bandit_b):
        assert make(surrogate="ssgp", ssgp_kw={"features": 128}, pool=256).techniques[0].model.ssgp_kw == {"features": 128}
    reg = T.reference_registry(surrogate="ssgp", pool=256)
    kids = [k for t in reg for k in getattr(t, "techniques", [t]) if hasattr(k, "model")]
    assert kids and all(k.model.surrogate == "ssgp" for k in kids)
    for kw in (dict(ssgp_kw={"rows": 3}), dict(ssgp_kw={"features": 100}), dict(ssgp_kw={"features": 4096}),
               dict(lengthscale="ard"), dict(precision=32), dict(feasibility=True),
               dict(constraints=[("accuracy", ">=", 0.5)]), dict(objectives=[("time", "min"), ("size", "min")])):
        with pytest.raises(ValueError, match="ssgp"):
            T.SharedModel(surrogate="ssgp", **kw)
    with pytest.raises(ValueError, match="belongs to surrogate='ssgp'"):
        T.SharedModel(ssgp_kw={"features": 128})
    for kw in (dict(prune_rows=64), dict(diversify=16), dict(polish=2), dict(acq="ts"), dict(feasibility=True),
               dict(constraints=[("accuracy", ">=", 0.5)]), dict(objectives=[("time", "min"), ("size", "min")])):
        with pytest.raises(ValueError, match="not with a ssgp surrogate"):
            T.GpuDifferentialEvolution(surrogate="ssgp", pool=256, **kw)
    from uptune_amd.tuner import tune_bandit
    assert "ssgp_kw" in tune_bandit.__code__.co_varnames
