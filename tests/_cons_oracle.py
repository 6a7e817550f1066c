"""Test infrastructure: the CPU restatement of constrained EI (numpy, fp64) on
the build's own GP (oracle.gp), over feature rows as oracle.space.features
encodes them.  Constraints c_j(x) <= t_j on values C [n][nc] row-aligned with X:

  alpha_j   = GP(X, C[:, j]).alpha            (same inputs, kernel, hyperparameters: same L)
  mu_cj(u)  = k*(u) . alpha_j                 tau_j = (t_j - m_j) / s_j
  P_j(u)    = Phi((tau_j - mu_cj) / sqrt(var));   var == 0: mu_cj <= tau_j ? 1 : 0
  P(u)      = prod_j P_j(u)
  F         = { r : C[r, j] <= t_j for every j },   f_best_c = min_{r in F} ys[r]
  score(u)  = EI(mu, var; f_best_c, xi) P(u)  if F is not empty, else P(u)

Never used by uptune_amd."""
import numpy as np
from scipy.special import erfc

from oracle.gp import GP, acquisition, sqdist


class ConsGP:
    def __init__(self, X, y, C, thresholds, lengthscale, **hyper):
        X = np.asarray(X, dtype=np.float64)
        C = np.asarray(C, dtype=np.float64).reshape(X.shape[0], -1)
        self.thr = np.asarray(thresholds, dtype=np.float64).reshape(-1)
        assert self.thr.shape[0] == C.shape[1]
        self.gp = GP(X, y, lengthscale, **hyper)
        self.cgp = [GP(X, C[:, j], lengthscale, **hyper) for j in range(C.shape[1])]
        self.alpha = np.stack([g.alpha for g in self.cgp], axis=0) if self.cgp else np.zeros((0, X.shape[0]))
        self.tau = np.array([(t - g.mean) / g.std for t, g in zip(self.thr, self.cgp)])
        self.feasible = np.all(C <= self.thr[None, :], axis=1)
        self.n_feasible = int(self.feasible.sum())
        self.f_best_c = float(np.min(self.gp.ys[self.feasible])) if self.n_feasible else float("nan")

    def kstar(self, U):
        Us = np.asarray(U, dtype=np.float64) * self.gp.inv_ell
        return self.gp.sf2 * np.exp(-0.5 * sqdist(Us, self.gp.Xs))

    def mu_c(self, U):
        """[nc][m] standardised constraint means"""
        return self.alpha @ self.kstar(U).T

    def posterior(self, U):
        return self.gp.posterior(U)

    def prob(self, var, mu_c):
        return cons_prob(var, mu_c, self.tau)

    def score(self, mu, var, mu_c, xi=0.0):
        return cons_score(mu, var, mu_c, self.tau, self.f_best_c, self.n_feasible, xi)


def cons_prob(var, mu_c, tau):
    """P [m] from var [m], mu_c [nc][m], tau [nc]; j ascending"""
    var = np.asarray(var, dtype=np.float64)
    sigma = np.sqrt(var)
    P = np.ones_like(var)
    for mc, t in zip(np.asarray(mu_c, dtype=np.float64), np.asarray(tau, dtype=np.float64)):
        with np.errstate(divide="ignore", invalid="ignore"):
            z = (t - mc) / np.where(var == 0.0, 1.0, sigma)
            pj = 0.5 * erfc(-z * 0.70710678118654752440)
        P = P * np.where(var == 0.0, np.where(mc <= t, 1.0, 0.0), pj)
    return P


def cons_score(mu, var, mu_c, tau, f_best_c, n_feasible, xi=0.0):
    P = cons_prob(var, mu_c, tau)
    if n_feasible == 0:
        return P
    return acquisition(np.asarray(mu), np.asarray(var), f_best_c, "ei", xi) * P


def rule_on(score0, mu, var, mu_c, tau, f_best_c, n_feasible, xi=0.0):
    """the score rule applied where an unconstrained score is finite: -inf (a
    duplicate) and NaN (a failed fit) pass through"""
    s = cons_score(mu, var, mu_c, tau, f_best_c, n_feasible, xi)
    return np.where(np.isfinite(score0), s, score0)
