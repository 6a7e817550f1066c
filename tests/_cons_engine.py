"""Test infrastructure: the CPU stand-in engine (tests/_oracle_engine.py) plus
the constrained-EI calls, scoring by the restatement (tests/_cons_oracle.py).
It records every gp_fit / gp_cons_set in order, so a test can see that the
values follow each fit and in which row order.  Never used by uptune_amd."""
import numpy as np
import torch

from _cons_oracle import ConsGP, rule_on
from _oracle_engine import OracleEngine


class ConsEngine(OracleEngine):
    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.log = []          # ("fit", X, y) / ("cons", C, thresholds) in call order
        self._fit = None
        self._cons = None      # the values loaded for the current fit (None: none, or stale)

    def gp_fit(self, X, y, lengthscale, **kw):
        self._fit = (np.array(X), np.array(y), lengthscale, {k: v for k, v in kw.items() if k != "wait"})
        self._cons = None
        self.log.append(("fit", self._fit[0], self._fit[1]))
        return super().gp_fit(X, y, lengthscale, **kw)

    def gp_cons_set(self, C, thresholds):
        C = np.array(C, dtype=np.float64).reshape(len(C), -1)
        thr = np.atleast_1d(np.asarray(thresholds, dtype=np.float64))
        assert self._fit is not None and C.shape[0] == self._fit[0].shape[0], "the values are the fit's rows"
        assert np.isfinite(C).all() and not np.isnan(thr).any()
        self.log.append(("cons", C, thr))
        self._cons = (C, thr)

    def gp_cons_clear(self):
        self._cons = None

    def cons_gp(self):
        X, y, ell, hyper = self._fit
        return ConsGP(X, y, self._cons[0], self._cons[1], ell, **hyper)

    def gp_cons_info(self):
        if self._cons is None:
            return {"n": 0, "nc": 0, "n_feasible": 0, "f_best_c": float("nan")}
        g = self.cons_gp()
        return {"n": self._cons[0].shape[0], "nc": self._cons[0].shape[1], "n_feasible": g.n_feasible,
                "f_best_c": g.f_best_c}

    def gp_score(self, feat, m=None, acq=None, dup=None):
        mu, var, sc = super().gp_score(feat, m, acq, dup)
        if self._cons is not None and self.gp_ok:
            g = self.cons_gp()
            U = feat.numpy().T
            xi = (acq or ("ei", 0.0, 2.0))[1]
            s = rule_on(sc.numpy(), mu.numpy(), var.numpy(), g.mu_c(U), g.tau, g.f_best_c, g.n_feasible, xi)
            sc = torch.from_numpy(s)
        return mu, var, sc
