"""Failure-aware scoring on the CPU: the restatement of the kernel vote
(tests/_feas_oracle.py) has the properties the rule promises and finds signal
in the recorded gcc failures, and SharedModel(feasibility=...) hands the
engine exactly the failed configurations' features."""
import copy

import numpy as np
import pytest

from _feas_oracle import auc, feas_prob, gcc_split
from _oracle_engine import OracleEngine
from _spaces import oracle_space


def test_restatement_properties():
    rng = np.random.default_rng(0)
    n, nf, d, m = 40, 7, 5, 200
    X, F = rng.uniform(size=(n, d)), rng.uniform(size=(nf, d))
    U = rng.uniform(-0.5, 1.5, size=(m, d))
    for ell, lam, s in [(0.3, 1.0, 1.0), (2.0, 0.01, 0.5), (np.linspace(0.2, 1.5, d), 3.0, 2.0)]:
        p, s_ok, s_fail = feas_prob(X, F, U, ell, strength=lam, ell_scale=s)
        assert np.all(p >= 0.0) and np.all(p <= 1.0)
        assert np.all(s_ok >= 0.0) and np.all(s_ok <= n) and np.all(s_fail <= nf)
        # rows in any order: the same vote
        p2, _, _ = feas_prob(X[rng.permutation(n)], F[rng.permutation(nf)], U, ell, strength=lam, ell_scale=s)
        np.testing.assert_allclose(p2, p, rtol=1e-12)
    # no failed rows: p >= p0 everywhere (p0 = 1 by default, so any explicit one), = p0 where S_ok underflows
    far = np.full((1, d), 1e3)
    p, s_ok, _ = feas_prob(X, None, np.vstack([U, far]), 0.3, prior=0.6, strength=2.0)
    assert np.all(p >= 0.6) and s_ok[-1] == 0.0 and p[-1] == 0.6
    p, _, _ = feas_prob(X, None, U, 0.3)
    assert np.all(p == 1.0)
    # on a failed row far from every OK row: lambda p0 / (1 + lambda)
    for lam in (1.0, 0.01, 5.0):
        p, s_ok, s_fail = feas_prob(X, far, far, 0.3, strength=lam)
        p0 = n / (n + 1)
        assert s_ok[0] == 0.0 and s_fail[0] == 1.0
        np.testing.assert_allclose(p[0], lam * p0 / (1.0 + lam), rtol=1e-15)


def test_gcc_fixture_vote_ranks_failures_low(golden_dir):
    """the first 1,024 successful recorded runs against the 117 failed ones
    among the first 3,000: the vote (ell = 3, lambda = 1) ranks a held-out
    successful run above a held-out failed one with AUC 0.817 (ell 2: 0.811,
    ell 4: 0.813); 0.75 leaves room for nothing but edits of the restatement"""
    from uptune_amd import spaces
    X_ok, X_fail, U, cand_ok, _ = gcc_split(golden_dir, oracle_space(spaces.gcc()))
    assert X_ok.shape[0] == 1024 and X_fail.shape[0] == 117 and U.shape[0] == 680 and (~cand_ok).sum() == 32
    p, _, _ = feas_prob(X_ok, X_fail, U, 3.0)
    a = auc(p[cand_ok], p[~cand_ok])
    print("gcc fixture: AUC %.4f, p in [%.4f, %.4f]" % (a, p.min(), p.max()))
    assert a >= 0.75
    assert p.min() > 0.85 and p.max() < 1.0      # mild weights: nine runs in ten succeed


class _FeasEngine(OracleEngine):
    """the CPU stand-in plus the feasibility calls: records what it is given and
    weights EI by the restatement's vote"""

    def __init__(self, *a, **kw):
        super().__init__(*a, **kw)
        self.feas_calls = []
        self._fail = None
        self._fit = None

    def gp_fit(self, X, y, lengthscale, **kw):
        self._fit = (np.array(X), lengthscale)
        return super().gp_fit(X, y, lengthscale, **kw)

    def gp_feas_set(self, X_fail, prior=None, strength=1.0, ell_scale=1.0, power=1.0):
        self.feas_calls.append((np.array(X_fail), dict(prior=prior, strength=strength, ell_scale=ell_scale,
                                                       power=power)))
        self._fail = self.feas_calls[-1]

    def gp_score(self, feat, m=None, acq=None, dup=None):
        mu, var, sc = super().gp_score(feat, m, acq, dup)
        if self._fail is not None and len(self._fail[0]) and self.gp_ok:
            import torch
            F, kw = self._fail
            p, _, _ = feas_prob(self._fit[0], F, feat.numpy().T, self._fit[1], prior=kw["prior"],
                                strength=kw["strength"], ell_scale=kw["ell_scale"])
            s = sc.numpy()
            sc = torch.from_numpy(np.where(np.isfinite(s), s * p ** kw["power"], s))
        return mu, var, sc


def _space():
    from uptune_amd.manipulator import ConfigurationManipulator, FloatParameter, IntegerParameter
    return ConfigurationManipulator([FloatParameter("x", 0.0, 1.0), FloatParameter("y", 0.0, 1.0),
                                     IntegerParameter("n", 0, 20)])


def _objective(cfg):
    return float("inf") if cfg["x"] > 0.5 else (cfg["x"] - 0.2) ** 2 + (cfg["y"] - 0.7) ** 2 + 0.01 * cfg["n"]


def _run(feasibility, generations=8):
    from uptune_amd import technique as T
    from uptune_amd.driver import SearchDriver
    tech = T.GpuDifferentialEvolution(pool=64, batch=4, population=16, seed=3, engine_factory=_FeasEngine,
                                      feasibility=feasibility, name="de")
    drv = SearchDriver(_space(), tech, parallelism=4)
    tech = drv.root_technique
    calls_at = []     # after every generation: (failed results so far, calls so far)
    for g in range(generations):
        drv.main(_objective, test_limit=4 * (g + 1) - 1, max_generations=g + 1)
        bad = [r for r in drv.results_query() if not np.isfinite(r.time)]
        calls_at.append((len(bad), len(tech.engine.feas_calls) if tech.engine is not None else 0))
    return drv, tech, calls_at


def test_shared_model_loads_the_failed_rows():
    """fails without the feature: SharedModel has no `feasibility` argument"""
    from uptune_amd import technique as T
    drv, tech, calls_at = _run(True)
    eng, model = tech.engine, tech.model
    bad = [r for r in drv.results_query() if not np.isfinite(r.time)]
    good = [r for r in drv.results_query() if np.isfinite(r.time)]
    assert len(bad) >= 2 and len(good) >= model.min_train, "the run must see failures and fit a model"
    want = eng.features_host([r.configuration.data for r in bad])
    calls = eng.feas_calls
    assert calls, "feasibility=True: the failed rows reach the engine"
    # every call: the failed configurations so far, features as the engine encodes them, in arrival order
    sizes = [len(X) for X, _ in calls]
    assert sizes == sorted(set(sizes)), "rows are sent again only when their number grew: %r" % sizes
    for X, kw in calls:
        np.testing.assert_array_equal(X, want[:len(X)])
        assert kw == dict(prior=None, strength=1.0, ell_scale=1.0, power=1.0)
    # up to date with the last fit, and readable
    seen = [nb for nb, _ in calls_at]
    assert model.n_failed == sizes[-1] and sizes[-1] >= seen[-2]
    # a dict sets the vote's parameters
    _, tech2, _ = _run({"strength": 0.01, "power": 2.0}, generations=6)
    assert tech2.engine.feas_calls and all(kw == dict(prior=None, strength=0.01, ell_scale=1.0, power=2.0)
                                           for _, kw in tech2.engine.feas_calls)
    # off: nothing is loaded
    _, tech0, _ = _run(False, generations=6)
    assert tech0.engine.feas_calls == [] and tech0.model.n_failed == 0
    # a deep copy (one per driver) starts clean
    cp = copy.deepcopy(tech)
    assert cp.model.engine is None and cp.model.n_failed == 0 and cp.model._scan_failed == []
    assert cp.model._fail_sent == 0 and cp.model.feasibility == {}
    # what the weight is not defined for
    for bad_kw in (dict(prune_rows=64), dict(diversify=16), dict(acq="ucb"), dict(surrogate=object())):
        with pytest.raises(ValueError):
            T.GpuDifferentialEvolution(pool=64, batch=4, feasibility=True, **bad_kw)
        sm = T.SharedModel(feasibility=True, engine_factory=_FeasEngine)
        with pytest.raises(ValueError):
            T.GpuGA(pool=64, batch=4, shared=sm, **bad_kw)          # a shared model carries its own setting
        T.GpuDifferentialEvolution(pool=64, batch=4, **bad_kw)     # (fine without the weight)
    with pytest.raises(ValueError):
        T.SharedModel(feasibility={"lambda": 1.0})
    # the factories pass it through
    b = T.pso_ga_de_bandit(pool=64, batch=4, feasibility={"strength": 2.0}, engine_factory=_FeasEngine)
    assert all(t.model.feasibility == {"strength": 2.0} for t in b.techniques)


def test_failures_alone_reach_the_engine():
    """a failed result with no new successful one does not refit, but is loaded"""
    import types

    from uptune_amd.technique import SharedModel

    class Eng:
        spec = types.SimpleNamespace(n_features=2)

        def __init__(self):
            self.fits, self.sets = 0, []

        def features_host(self, cfgs):
            return np.asarray([[c["a"], c["b"]] for c in cfgs], dtype=np.float64)

        def gp_fit(self, X, y, lengthscale, wait=True, **hyper):
            self.fits += 1

        def gp_fit_ok(self):
            return True

        def gp_feas_set(self, X, **kw):
            self.sets.append(np.array(X))

    rows = []

    def add(a, b, t):
        rows.append(types.SimpleNamespace(configuration=types.SimpleNamespace(data={"a": a, "b": b}, hash="h%d" % len(rows)),
                                          time=t, state="OK", id=len(rows)))

    drv = types.SimpleNamespace(results_query=lambda: rows)
    sm = SharedModel(feasibility=True, min_train=2)
    sm.engine = Eng()
    add(0.1, 0.2, 1.0)
    add(0.9, 0.9, float("inf"))
    assert sm.fit(drv) is False and sm.engine.sets == []        # no model yet: no weight
    add(0.3, 0.4, 2.0)
    assert sm.fit(drv) and sm.engine.fits == 1 and sm.n_failed == 1
    np.testing.assert_array_equal(sm.engine.sets[-1], [[0.9, 0.9]])
    assert sm.fit(drv) and len(sm.engine.sets) == 1              # nothing new
    add(0.8, 0.1, float("inf"))
    assert sm.fit(drv) and sm.engine.fits == 1 and sm.n_failed == 2
    np.testing.assert_array_equal(sm.engine.sets[-1], [[0.9, 0.9], [0.8, 0.1]])
