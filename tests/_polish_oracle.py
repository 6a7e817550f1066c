"""Test infrastructure: the acquisition's gradient in the unit features and the
projected-ascent polish (include/uthot.h ut_gp_acq_grad, ut_gp_polish)
restated in numpy over oracle/gp.py's GP, the checker and never the product.
The reference has no GP: the rule is the specification.

  k_i = sf2 exp(-1/2 |us - xs_i|^2),  v = L^-1 k,  w = L^-T v
  dmu/du_j  = -(1/ell_j) (us_j sum_i alpha_i k_i - sum_i alpha_i k_i xs_ij)
  dvar/du_j = +(2/ell_j) (us_j sum_i w_i k_i     - sum_i w_i k_i xs_ij)
  EI:  ds = -Phi(z) dmu + phi(z) dvar / (2 sigma);  sigma not > 0: -[I > 0] dmu
  UCB: ds = kappa dvar / (2 sigma) - dmu;           sigma not > 0: -dmu

score_grad(ld=True) takes the GP's fp64 factor L as given and carries its
inverse (the substitutions, by hand), alpha and every product after it in
np.longdouble (Phi alone is scipy's fp64 erfc at z rounded to fp64: 1e-16
relative): it measures the rounding of the restatement, not of the factor."""
import numpy as np
from scipy.linalg import solve_triangular
from scipy.special import erfc

from oracle import gp as ogp

import _lml_oracle as O

# (n, d, p, ell): one padded block; d and p off every tile size; npad = 384
CASES = [(100, 5, 256, 0.5), (200, 37, 300, 2.0), (321, 3, 1024, 0.3)]
TIERS = [(1e-2, 1e-9), (1e-6, 1e-5)]       # (sigma_n2, rtol): the project's tiers (test_gpu_lml.py)
KINDS = ["ei", "ucb"]

_GPS = {}
_CANDS = {}


def gp_of(n, d, ell, sn2):
    key = (n, d, np.asarray(ell, dtype=np.float64).tobytes(), sn2)
    if key not in _GPS:
        X, y = O.data(n, d)
        _GPS[key] = ogp.GP(X, y, lengthscale=ell, sigma_n2=sn2)
    return _GPS[key]


def cands(n, d, p):
    """uniform candidates [p][d]; row 0 a training row (sigma ~ 0), row 1 all zeros, row 2 all ones"""
    key = (n, d, p)
    if key not in _CANDS:
        U = np.random.default_rng(9000 + n).uniform(size=(p, d))
        U[0] = O.data(n, d)[0][n // 2]
        U[1] = 0.0
        U[2] = 1.0
        U.setflags(write=False)
        _CANDS[key] = U
    return _CANDS[key]


def _ld_factor(g):
    """(L^-1, alpha) from g's own fp64 factor, the substitutions carried by hand in np.longdouble"""
    ld = np.longdouble
    L, ys = g.L.astype(ld), g.ys.astype(ld)
    n = len(ys)
    Li = np.zeros((n, n), dtype=ld)
    for i in range(n):
        Li[i, :i] = -(L[i, :i] @ Li[:i, :i]) / L[i, i]
        Li[i, i] = 1 / L[i, i]
    return Li, Li.T @ (Li @ ys)


_LDF = {}


def score_grad(g, U, kind="ei", ld=False, xi=0.0, kappa=2.0):
    """-> dict score, mu, var [p], grad [p][d] (d score / d u), dmu, dvar [p][d].
    ld: everything after g's factor in np.longdouble"""
    T = np.longdouble if ld else np.float64
    U = np.asarray(U, dtype=np.float64).astype(T)
    ie, Xs, sf2 = g.inv_ell.astype(T), g.Xs.astype(T), T(g.sf2)
    Us = U * ie
    d2 = np.sum(Us * Us, axis=1)[:, None] + np.sum(Xs * Xs, axis=1)[None, :] - 2 * (Us @ Xs.T)
    Ks = sf2 * np.exp(-T(0.5) * np.maximum(d2, 0))                       # [p][n]
    if ld:
        if id(g) not in _LDF:
            _LDF[id(g)] = (g, _ld_factor(g))
        Li, alpha = _LDF[id(g)][1]
        V = Li @ Ks.T
        W = Li.T @ V
    else:
        alpha = g.alpha
        V = solve_triangular(g.L, Ks.T, lower=True)
        W = solve_triangular(g.L.T, V, lower=False)
    mu = Ks @ alpha
    var = np.maximum(sf2 - np.sum(V * V, axis=0), 0)
    A, Bw = Ks * alpha[None, :], Ks * W.T
    dmu = -ie * (Us * A.sum(axis=1)[:, None] - A @ Xs)
    dvar = 2 * ie * (Us * Bw.sum(axis=1)[:, None] - Bw @ Xs)
    sigma = np.sqrt(var)
    pos = sigma > 0
    safe = np.where(pos, sigma, 1)
    if kind == "ucb":
        score = T(kappa) * sigma - mu
        cm = -np.ones_like(mu)
        cs = np.where(pos, T(kappa) / (2 * safe), 0)
    else:
        I = T(g.f_best) - mu - T(xi)
        z = np.where(pos, I / safe, 0)
        Phi = (0.5 * erfc(-z.astype(np.float64) / np.sqrt(2.0))).astype(T)
        phi = np.exp(-T(0.5) * z * z) / np.sqrt(2 * np.arccos(T(-1)))
        score = np.where(pos, I * Phi + sigma * phi, np.maximum(I, 0))
        cm = np.where(pos, -Phi, -(I > 0).astype(T))
        cs = np.where(pos, phi / (2 * safe), 0)
    grad = cm[:, None] * dmu + cs[:, None] * dvar
    return dict(score=score, mu=mu, var=var, grad=grad, dmu=dmu, dvar=dvar)


def trial(U, G, ell, eta, free=None):
    """one step's masked gradient and trial point: -> (U' [p][d], N [p], active [p])"""
    U, G = np.asarray(U, dtype=np.float64), np.array(G, dtype=np.float64)
    ell = np.broadcast_to(np.asarray(ell, dtype=np.float64), (U.shape[1],))
    free = np.ones(U.shape[1], dtype=bool) if free is None else np.asarray(free, dtype=bool)
    G[:, ~free] = 0.0
    G[((U <= 0.0) & (G < 0.0)) | ((U >= 1.0) & (G > 0.0))] = 0.0
    N = np.sqrt(np.sum((ell * G) ** 2, axis=1))
    act = np.isfinite(N) & (N > 0.0)
    step = np.asarray(eta, dtype=np.float64)[:, None] * ell ** 2 * G / np.where(act, N, 1.0)[:, None]
    Ut = np.where(act[:, None] & free[None, :], np.clip(U + step, 0.0, 1.0), U)
    return Ut, N, act


def polish(g, U, kind, steps, free=None, dup=None, step0=0.25, step_max=1.0, grow=2.0, shrink=0.5, **acq):
    """the rule on features (no decode): -> dict U [p][d], score, score0 [p], accepted [p]"""
    U = np.array(U, dtype=np.float64)
    ell = 1.0 / g.inv_ell
    dead = np.zeros(len(U), dtype=bool) if dup is None else np.asarray(dup) != 0
    r = score_grad(g, U, kind, **acq)
    s0 = r["score"].copy()
    s, eta = s0.copy(), np.full(len(U), step0)
    accepted = np.zeros(len(U), dtype=bool)
    for _ in range(steps):
        Ut, N, act = trial(U, r["grad"], ell, eta, free)
        act &= ~dead
        st = score_grad(g, Ut, kind, **acq)["score"]
        take = act & (st > s)
        U[take], s[take] = Ut[take], st[take]
        eta = np.where(take, np.minimum(grow * eta, step_max), np.where(act, shrink * eta, eta))
        accepted |= take
        r = score_grad(g, U, kind, **acq)
    return dict(U=U, score=np.where(dead, -np.inf, s), score0=np.where(dead, -np.inf, s0), accepted=accepted)

