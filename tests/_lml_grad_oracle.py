"""Test infrastructure: the gradient of the log marginal likelihood in the log
hyperparameters, analytic, in NumPy fp64 on oracle/gp.py's own factor (the
checker, never the product), with the magnitude of every component's sum.

  W = alpha alpha^T - K^-1,  Kf = sf2 exp(-1/2 |xs_i - xs_j|^2),  M = W o Kf
  g_ell[k] = 1/2 sum_ij M_ij (xs_ik - xs_jk)^2     S_ell[k] = the same over |M_ij|
  g_sf2    = 1/2 sum_ij M_ij                       S_sf2    = 1/2 sum |M_ij|
  g_sn2    = 1/2 sn2 tr W                          S_sn2    = 1/2 sn2 sum |W_ii|

The components are heavily cancelling sums (|g| / S between 2e-9 and 2e-3 at
the tests' shapes), so an error is measured against S, never against g."""
import collections

import numpy as np
from scipy.linalg import solve_triangular

from oracle import gp as ogp

Grad = collections.namedtuple("Grad", "ell sf2 sn2 S_ell S_sf2 S_sn2")


def _components(Xs, alpha, Kinv, sf2, sn2):
    """the six results from the scaled rows, alpha and K^-1, in their own dtype"""
    half = Xs.dtype.type(0.5)
    W = np.outer(alpha, alpha) - Kinv
    sq = np.sum(Xs * Xs, axis=1)
    d2 = np.maximum(sq[:, None] + sq[None, :] - 2 * (Xs @ Xs.T), 0)   # oracle/gp.py sqdist
    M = W * (sf2 * np.exp(-half * d2))
    A = np.abs(M)
    g, S = np.empty(Xs.shape[1], dtype=Xs.dtype), np.empty(Xs.shape[1], dtype=Xs.dtype)
    for k in range(Xs.shape[1]):
        D = (Xs[:, k, None] - Xs[None, :, k]) ** 2
        g[k], S[k] = half * np.sum(M * D), half * np.sum(A * D)
    dg = np.diag(W)
    return Grad(g, half * np.sum(M), half * sn2 * np.sum(dg), S, half * np.sum(A), half * sn2 * np.sum(np.abs(dg)))


def from_gp(g, sigma_n2):
    """the gradient at a fitted oracle GP (its L, alpha, Xs, sf2)"""
    Li = solve_triangular(g.L, np.eye(len(g.ys)), lower=True)
    return _components(g.Xs, g.alpha, Li.T @ Li, g.sf2, float(sigma_n2))


def grad(X, y, lengthscale, sigma_f2=1.0, sigma_n2=1e-6, jitter=0.0):
    """Grad of the LML of (X, y) at the hyperparameters; LinAlgError where K is not positive definite"""
    return from_gp(ogp.GP(X, y, lengthscale=lengthscale, sigma_f2=sigma_f2, sigma_n2=sigma_n2, jitter=jitter), sigma_n2)


def grad_longdouble(X, y, lengthscale, sigma_f2=1.0, sigma_n2=1e-6, jitter=0.0):
    """the same definition with every step in np.longdouble (its own Cholesky
    and triangular inverse, row by row): what the fp64 helper is checked against"""
    ld = np.longdouble
    X, y = np.asarray(X, dtype=ld), np.asarray(y, dtype=ld)
    n, d = X.shape
    Xs = X / np.broadcast_to(np.asarray(lengthscale, dtype=ld), (d,))
    mean = np.mean(y)
    sd = np.sqrt(np.mean((y - mean) ** 2))
    ys = (y - mean) / (sd if sd > 0 else ld(1))
    sq = np.sum(Xs * Xs, axis=1)
    K = ld(sigma_f2) * np.exp(-ld(0.5) * np.maximum(sq[:, None] + sq[None, :] - 2 * (Xs @ Xs.T), 0))
    K[np.diag_indices(n)] += ld(sigma_n2) + ld(jitter)
    L = np.zeros((n, n), dtype=ld)
    for j in range(n):
        L[j, j] = np.sqrt(K[j, j] - L[j, :j] @ L[j, :j])
        L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    Li = np.zeros((n, n), dtype=ld)
    for i in range(n):
        Li[i, :i] = -(L[i, :i] @ Li[:i, :i]) / L[i, i]
        Li[i, i] = 1 / L[i, i]
    alpha = Li.T @ (Li @ ys)
    return _components(Xs, alpha, Li.T @ Li, ld(sigma_f2), ld(sigma_n2))


def errors(got, want):
    """(max over the features of |got - want| / S, the same for sf2, for sn2): got = (ell [d], sf2, sn2)"""
    e = np.max(np.abs(np.asarray(got[0], dtype=np.longdouble) - want.ell) / want.S_ell)
    return float(e), float(abs(got[1] - want.sf2) / want.S_sf2), float(abs(got[2] - want.sn2) / want.S_sn2)
