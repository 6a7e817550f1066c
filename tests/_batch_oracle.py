"""Test infrastructure: batch-aware selection (include/uthot.h
ut_gp_select_batch) restated in numpy over oracle/gp.py's GP, the checker and
never the product.  The reference has no GP: the rule is the
specification."""
import numpy as np
from scipy.linalg import solve_triangular

from oracle import gp as ogp


def pool(n, p, d):
    return np.random.default_rng(7000 + n).uniform(size=(p, d))


def posterior(gp, U):
    """mu [p], Sigma [p][p] of the shortlist U [p][d]"""
    Us = np.asarray(U, dtype=np.float64) * gp.inv_ell
    Ks = gp.sf2 * np.exp(-0.5 * ogp.sqdist(Us, gp.Xs))
    V = solve_triangular(gp.L, Ks.T, lower=True)
    return Ks @ gp.alpha, gp.sf2 * np.exp(-0.5 * ogp.sqdist(Us, Us)) - V.T @ V


def select(gp, U, k, noise, kind="ei", dup=None, xi=0.0, kappa=2.0, forced=None):
    """k greedy picks (noise = sigma_n2 + jitter of gp's fit).  forced: walk this
    pick sequence instead of the argmax (-1 ends it).  -> dict of pos, score and
    var at pick time (-1, -inf, NaN in an empty slot), best (the step's maximum),
    gap (best to runner-up, relative) and var_after (every variance at the end)"""
    mu, Sig = posterior(gp, U)
    p = len(mu)
    var = np.maximum(np.diag(Sig), 0.0)
    dead = np.zeros(p, dtype=bool) if dup is None else np.asarray(dup) != 0
    G = np.zeros((k, p))
    r = dict(pos=np.full(k, -1), score=np.full(k, -np.inf), var=np.full(k, np.nan), best=np.full(k, -np.inf),
             gap=np.full(k, np.nan))
    for t in range(k):
        s = np.where(dead, -np.inf, ogp.acquisition(mu, var, gp.f_best, kind, xi, kappa))
        j = int(np.argmax(s))   # ties: the smallest position
        if not s[j] > -np.inf or (forced is not None and forced[t] < 0):
            break
        if p > 1:
            s2, s1 = np.partition(s, -2)[-2:]
            r["gap"][t] = (s1 - s2) / abs(s1) if s1 != 0.0 else 0.0
        r["best"][t] = s[j]
        j = j if forced is None else int(forced[t])
        r["pos"][t], r["score"][t], r["var"][t] = j, s[j], var[j]
        c = Sig[:, j] - G[:t].T @ G[:t, j]
        G[t] = c / np.sqrt(c[j] + noise)
        var = np.maximum(var - G[t] ** 2, 0.0)
        dead[j] = True
    r["var_after"] = var
    return r
