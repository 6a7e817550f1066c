"""TrustRegion: the host state of the trust-region proposals (ut_propose_tr).

TuRBO-1's rule (Eriksson et al. 2019, "Scalable Global Optimization via Local
Bayesian Optimization"): propose inside a box of side L around the best point,
shaped by the GP's per-feature lengthscales; double L after `succ_tol`
successful rounds in a row, halve it after `fail_tol` failed ones, and start
again at L_init once it falls below L_min.  Pure Python: no device state.
"""
from __future__ import annotations

import math
from typing import Tuple

import numpy as np

from . import _lib as L

_PRIMITIVE = (L.UT_FLOAT, L.UT_INT, L.UT_LOGINT, L.UT_POW2)
_INTEGER = (L.UT_INT, L.UT_LOGINT, L.UT_POW2)   # kinds whose stored values are integers


class TrustRegion:
    def __init__(self, n_move: int, batch: int, L_init: float = 0.8, L_min: float = 2.0 ** -7, L_max: float = 1.6,
                 succ_tol: int = 3, fail_tol: int = None):
        """n_move: the parameters a candidate can move (sets the perturbation
        probability and the default fail_tol); batch: evaluations per round"""
        self.n_move, self.batch = max(int(n_move), 1), max(int(batch), 1)
        self.L_init, self.L_min, self.L_max = float(L_init), float(L_min), float(L_max)
        self.succ_tol = int(succ_tol)
        self.fail_tol = max(4, math.ceil(self.n_move / self.batch)) if fail_tol is None else int(fail_tol)
        self.L = self.L_init
        self.succ = self.fail = 0
        self.restarts = 0

    def judge(self, improved: bool) -> bool:
        """one finished round; True when the region collapsed and was restarted"""
        if improved:
            self.succ, self.fail = self.succ + 1, 0
        else:
            self.succ, self.fail = 0, self.fail + 1
        if self.succ >= self.succ_tol:
            self.L, self.succ = min(2.0 * self.L, self.L_max), 0
        elif self.fail >= self.fail_tol:
            self.L, self.fail = self.L / 2.0, 0
        if self.L < self.L_min:
            self.restarts += 1
            self.L, self.succ, self.fail = self.L_init, 0, 0
            return True
        return False

    def half_widths(self, spec, lengthscale) -> np.ndarray:
        """h[P] in unit space: L * w_p / 2 with w_p = ell_p / geomean(ell) over the
        movable primitive parameters (1 for a scalar lengthscale); at least
        1 / u_span for the integer kinds, so that a neighbouring integer stays
        within reach however small L gets; 0 for single-point ranges (lo == hi)"""
        ps = spec.params
        mov = [i for i, p in enumerate(ps) if p.kind in _PRIMITIVE and p.lo < p.hi]
        h = np.zeros(len(ps))
        if not mov:
            return h
        if np.ndim(lengthscale) == 0:
            w = np.ones(len(mov))
        else:
            ell = np.asarray(lengthscale, dtype=np.float64).reshape(-1)
            e = np.array([ell[ps[i].feat_col] for i in mov])
            w = e / math.exp(float(np.mean(np.log(e))))
        for i, wp in zip(mov, w):
            hp = self.L * float(wp) / 2.0
            if ps[i].kind in _INTEGER:
                hp = max(hp, 1.0 / ps[i].u_span)
            h[i] = hp
        return h

    def probs(self) -> Tuple[float, float]:
        """(prob, cat_prob): about 20 parameters move per candidate; BOOL / ENUM /
        PERM moves have no width, so their rate shrinks with the box instead"""
        prob = min(1.0, 20.0 / self.n_move)
        return prob, prob * min(1.0, self.L / self.L_init)
