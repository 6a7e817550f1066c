"""CMAState: the host state of the correlated-Gaussian proposals (ut_propose_cma).

CMA-ES (Hansen, "The CMA Evolution Strategy: A Tutorial") over the unit values
of the moving primitive parameters: a mean, a step size sigma and a covariance C
adapted from the ranks of evaluated results.  The sampling factor is the
Cholesky factor A of C, and A^-1 stands where the textbook has C^(-1/2) (the
Cholesky-CMA-ES of Krause, Arnold and Igel 2016), so no eigendecomposition is
taken.  Pure numpy: no device state.  A full covariance only: the diagonal
(sep-CMA) mode that spaces wider than 128 dimensions would need is not built.
"""
from __future__ import annotations

import math
from typing import List, Tuple

import numpy as np

from . import _lib as L

MAX_DN = 128   # ut_propose_cma keeps the whole factor in one workgroup's LDS


def moving_params(spec) -> List[int]:
    """the parameters ut_propose_cma samples: FLOAT, INT, LOGINT and POW2 with lo < hi, in order"""
    return [i for i, p in enumerate(spec.params) if p.kind <= L.UT_POW2 and p.lo < p.hi]


class CMAState:
    def __init__(self, dn: int, lam: int, sigma0: float = 0.3, sigma_min: float = 2.0 ** -20,
                 sigma_max: float = 64.0, cond_max: float = 1e7):
        """dn: dimensions; lam: the results a generation is expected to tell (the
        constants of a tell follow the number actually told)"""
        if not 1 <= int(dn) <= MAX_DN:
            raise ValueError(f"CMAState: dn must be in [1, {MAX_DN}], not {dn}")
        self.dn, self.lam = int(dn), max(int(lam), 2)
        self.sigma0, self.sigma_min = float(sigma0), float(sigma_min)
        self.sigma_max, self.cond_max = float(sigma_max), float(cond_max)
        n = self.dn
        self.chi_n = math.sqrt(n) * (1.0 - 1.0 / (4.0 * n) + 1.0 / (21.0 * n * n))
        self.mean = np.full(n, 0.5)
        self.restarts = self.generation = 0
        self._reset()

    def _reset(self):
        n = self.dn
        self.sigma = self.sigma0
        self.C, self.A = np.eye(n), np.eye(n)
        self.p_sigma, self.p_c = np.zeros(n), np.zeros(n)
        self.t = 0            # tells since the last restart (the h_sigma normalisation)

    def restart(self):
        """sigma, C and both paths start again; the mean is kept"""
        self.restarts += 1
        self._reset()

    def constants(self, lam: int):
        """Hansen's defaults for lam told results -> (w [mu], mu_eff, c_sigma, d_sigma, c_c, c_1, c_mu)"""
        n, mu = self.dn, lam // 2
        w = math.log(mu + 0.5) - np.log(np.arange(1, mu + 1))
        w = w / w.sum()
        mu_eff = 1.0 / float(np.sum(w * w))
        c_sigma = (mu_eff + 2.0) / (n + mu_eff + 5.0)
        d_sigma = 1.0 + 2.0 * max(0.0, math.sqrt((mu_eff - 1.0) / (n + 1.0)) - 1.0) + c_sigma
        c_c = (4.0 + mu_eff / n) / (n + 4.0 + 2.0 * mu_eff / n)
        c_1 = 2.0 / ((n + 1.3) ** 2 + mu_eff)
        c_mu = min(1.0 - c_1, 2.0 * (mu_eff - 2.0 + 1.0 / mu_eff) / ((n + 2.0) ** 2 + mu_eff))
        return w, mu_eff, c_sigma, d_sigma, c_c, c_1, c_mu

    def ask(self) -> Tuple[np.ndarray, float, np.ndarray]:
        """(mean [dn], sigma, A [dn][dn]) of the next generation: x = mean + sigma * A z"""
        return self.mean.copy(), self.sigma, self.A.copy()

    def tell(self, U, order) -> bool:
        """U [dn][k]: the unit points of k evaluated candidates (ut_propose_cma's
        out_unit columns); order: their column indices, best first.  Fewer than
        two is a no-op.  True when the state restarted."""
        U = np.asarray(U, dtype=np.float64).reshape(self.dn, -1)
        order = np.asarray(order, dtype=np.int64).reshape(-1)
        lam = order.size
        if lam < 2:
            return False
        w, mu_eff, c_sigma, d_sigma, c_c, c_1, c_mu = self.constants(lam)
        Y = (U[:, order[:w.size]] - self.mean[:, None]) / self.sigma        # [dn][mu], best first
        y_w = Y @ w
        self.mean = self.mean + self.sigma * y_w
        self.t += 1
        self.generation += 1
        self.p_sigma = (1.0 - c_sigma) * self.p_sigma + math.sqrt(c_sigma * (2.0 - c_sigma) * mu_eff) * \
            np.linalg.solve(self.A, y_w)
        norm = float(np.linalg.norm(self.p_sigma))
        h_sigma = norm / math.sqrt(1.0 - (1.0 - c_sigma) ** (2 * self.t)) < (1.4 + 2.0 / (self.dn + 1.0)) * self.chi_n
        self.p_c = (1.0 - c_c) * self.p_c + (math.sqrt(c_c * (2.0 - c_c) * mu_eff) * y_w if h_sigma else 0.0)
        stall = 0.0 if h_sigma else c_c * (2.0 - c_c)
        C = (1.0 - c_1 - c_mu) * self.C + c_1 * (np.outer(self.p_c, self.p_c) + stall * self.C) + \
            c_mu * (Y * w[None, :]) @ Y.T
        self.sigma = min(self.sigma * math.exp(min(1.0, (c_sigma / d_sigma) * (norm / self.chi_n - 1.0))),
                         self.sigma_max)
        return self._refactor(C)

    def _refactor(self, C) -> bool:
        """C symmetrised and A = chol(C); restarts when sigma has collapsed, C is not
        positive definite or A is ill-conditioned (the trust region's collapse rule)"""
        C = 0.5 * (C + C.T)
        ok = self.sigma >= self.sigma_min and bool(np.isfinite(C).all())
        if ok:
            try:
                A = np.linalg.cholesky(C)
                ok = float(np.linalg.cond(A)) <= self.cond_max
            except np.linalg.LinAlgError:
                ok = False
        if not ok:
            self.restart()
            return True
        self.C, self.A = C, A
        return False
