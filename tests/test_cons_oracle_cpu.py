"""Constrained EI on the CPU: the restatement (tests/_cons_oracle.py) has the
properties the definition promises, and SharedModel(constraints=...) hands the
engine the training rows' measured values after every fit, in the fit's row
order.  Every test fails without the feature: there is no `constraints`
argument, no `accuracy` on a Result and no ThresholdAccuracyMinimizeTime."""
import copy
import types

import numpy as np
import pytest

from _cons_engine import ConsEngine
from _cons_oracle import ConsGP, cons_prob
from oracle.gp import GP, acquisition

HYPER = dict(sigma_f2=1.0, sigma_n2=1e-4, jitter=1e-8)


def _data(n=40, d=4, m=150, nc=3, seed=0):
    rng = np.random.default_rng(seed)
    X, U = rng.uniform(size=(n, d)), rng.uniform(-0.2, 1.2, size=(m, d))
    y = np.sin(3.0 * X[:, 0]) + X[:, 1] ** 2 + 0.1 * rng.standard_normal(n)
    C = np.stack([X[:, j % d] * (j + 1.0) + 0.05 * rng.standard_normal(n) + 10.0 * j for j in range(nc)], axis=1)
    return X, y, C, U


def test_constraint_mean_is_a_gp_on_the_same_factor():
    X, y, C, U = _data()
    for ell in (0.3, 2.0, np.array([0.2, 0.5, 1.0, 3.0])):
        g = ConsGP(X, y, C, np.median(C, axis=0), ell, **HYPER)
        mc = g.mu_c(U)
        for j in range(C.shape[1]):
            want = GP(X, C[:, j], ell, **HYPER).posterior(U)[0]
            # the same n-term dot products summed in another order: each within
            # n eps sum |k*_r| |alpha_r| of the exact one (alpha is ~1 / sigma_n2 large)
            bound = 2.0 * len(y) * np.finfo(np.float64).eps * (np.abs(g.kstar(U)) @ np.abs(g.alpha[j]))
            assert np.all(np.abs(mc[j] - want) <= bound), np.max(np.abs(mc[j] - want) / bound)
        # ... and that GP's variance is the objective's: same inputs, kernel, hyperparameters
        np.testing.assert_array_equal(GP(X, C[:, 0], ell, **HYPER).posterior(U)[1], g.posterior(U)[1])


def test_probability_is_a_probability_and_monotone_in_each_threshold():
    X, y, C, U = _data()
    thr = np.median(C, axis=0)
    g = ConsGP(X, y, C, thr, 0.5, **HYPER)
    mu, var = g.posterior(U)
    mc = g.mu_c(U)
    P = g.prob(var, mc)
    assert np.all(P >= 0.0) and np.all(P <= 1.0) and P.min() < 0.5 < P.max()
    for j in range(C.shape[1]):
        prev = None
        for q in (0.0, 0.2, 0.5, 0.8, 1.0):
            t = thr.copy()
            t[j] = np.quantile(C[:, j], q)
            Pq = ConsGP(X, y, C, t, 0.5, **HYPER).prob(var, mc)
            assert prev is None or np.all(Pq >= prev), (j, q)
            prev = Pq
    # var == 0: the step at tau, and -inf / +inf thresholds
    tau = np.array([0.3])
    np.testing.assert_array_equal(cons_prob(np.zeros(3), np.array([[0.2, 0.3, 0.4]]), tau), [1.0, 1.0, 0.0])
    np.testing.assert_array_equal(cons_prob(np.array([0.0, 1.0]), np.zeros((1, 2)), np.array([np.inf])), [1.0, 1.0])
    np.testing.assert_array_equal(cons_prob(np.array([0.0, 1.0]), np.zeros((1, 2)), np.array([-np.inf])), [0.0, 0.0])


def test_all_feasible_and_infinite_thresholds_is_the_unconstrained_score():
    X, y, C, U = _data()
    g = ConsGP(X, y, C, np.full(C.shape[1], np.inf), 0.5, **HYPER)
    mu, var = g.posterior(U)
    assert g.n_feasible == len(y) and g.f_best_c == g.gp.f_best
    for xi in (0.0, 0.01):
        np.testing.assert_array_equal(g.score(mu, var, g.mu_c(U), xi), acquisition(mu, var, g.gp.f_best, "ei", xi))


def test_no_feasible_row_scores_by_the_probability_alone():
    X, y, C, U = _data()
    thr = C.min(axis=0) - 1.0
    g = ConsGP(X, y, C, thr, 0.5, **HYPER)
    mu, var = g.posterior(U)
    assert g.n_feasible == 0 and np.isnan(g.f_best_c)
    np.testing.assert_array_equal(g.score(mu, var, g.mu_c(U)), g.prob(var, g.mu_c(U)))
    # one feasible row: its standardised objective is the incumbent
    r = 17
    thr1 = np.where(np.arange(C.shape[1]) == 0, C[r, 0], np.inf)
    C1 = C.copy()
    C1[:, 0] += np.where(np.arange(len(y)) == r, 0.0, 1.0 + C[:, 0].max() - C[:, 0].min())
    g1 = ConsGP(X, y, C1, thr1, 0.5, **HYPER)
    assert g1.n_feasible == 1 and g1.f_best_c == g1.gp.ys[r]


# -- host plumbing -----------------------------------------------------------
class _Eng:
    """records gp_fit / gp_cons_set in call order"""
    spec = types.SimpleNamespace(n_features=2)

    def __init__(self):
        self.log = []

    def features_host(self, cfgs):
        return np.asarray([[c["a"], c["b"]] for c in cfgs], dtype=np.float64)

    def gp_fit(self, X, y, lengthscale, wait=True, **hyper):
        self.log.append(("fit", np.array(X), np.array(y)))

    def gp_fit_ok(self):
        return True

    def gp_cons_set(self, C, thr):
        self.log.append(("cons", np.array(C), np.array(thr)))


def _rows_driver():
    rows = []

    def add(a, b, t, **extra):
        r = types.SimpleNamespace(configuration=types.SimpleNamespace(data={"a": a, "b": b}, hash="h%d" % len(rows)),
                                  time=t, state="OK", id=len(rows))
        for k, v in extra.items():
            setattr(r, k, v)
        rows.append(r)

    return rows, add, types.SimpleNamespace(results_query=lambda: rows)


def test_shared_model_loads_the_values_after_every_fit_in_the_fit_order():
    from uptune_amd.technique import SharedModel
    rng = np.random.default_rng(5)
    rows, add, drv = _rows_driver()
    sm = SharedModel(constraints=[("accuracy", ">=", 0.5), ("size", "<=", 30.0)], min_train=4)
    sm.engine = _Eng()

    def grow(n):
        while len(rows) < n:
            a, b = rng.uniform(size=2)
            add(a, b, float(rng.uniform()), accuracy=float(a), size=float(100.0 * b))

    def check(n):
        kind, X, y = sm.engine.log[-2]
        kind2, C, thr = sm.engine.log[-1]
        assert (kind, kind2) == ("fit", "cons"), "gp_cons_set follows gp_fit directly"
        assert X.shape == (n, 2) and C.shape == (n, 2)
        # row r of the fit is the result with these features: its values, ">=" negated
        np.testing.assert_array_equal(C[:, 0], -X[:, 0])
        np.testing.assert_array_equal(C[:, 1], 100.0 * X[:, 1])
        np.testing.assert_array_equal(thr, [-0.5, 30.0])
        want = sum(1 for r in rows[:n] if r.accuracy >= 0.5 and r.size <= 30.0)
        assert sm.n_feasible_ == want
        return y

    grow(100)
    assert sm.fit(drv)
    y = check(100)
    assert np.all(np.diff(y) >= 0.0)                       # the first fit: best first
    grow(120)
    assert sm.fit(drv)
    y = check(120)
    assert np.all(np.diff(y[:100]) >= 0.0) and not np.all(np.diff(y) >= 0.0)   # appended in arrival order
    grow(130)                                              # a new padded size: re-sorted, values re-gathered
    assert sm.fit(drv)
    y = check(130)
    assert np.all(np.diff(y) >= 0.0)
    assert sm.fit(drv) and len(sm.engine.log) == 6         # nothing new: neither call again


def test_a_result_without_the_measurement_is_not_used():
    from uptune_amd.technique import SharedModel
    rows, add, drv = _rows_driver()
    sm = SharedModel(constraints=[("accuracy", ">=", 0.5)], min_train=2, feasibility=True)
    sm.engine = _Eng()
    sm.engine.gp_feas_set = lambda X, **kw: sm.engine.log.append(("feas", np.array(X)))
    add(0.1, 0.2, 1.0, accuracy=0.9)
    add(0.3, 0.1, 0.5)                                     # no attribute
    add(0.5, 0.5, 0.7, accuracy=None)
    add(0.6, 0.5, 0.8, accuracy=float("nan"))
    assert sm.fit(drv) is False                            # one usable row only
    add(0.7, 0.7, 2.0, accuracy=0.2)
    assert sm.fit(drv)
    (_, X, y), (_, C, thr) = sm.engine.log[-2:]
    np.testing.assert_array_equal(X, [[0.1, 0.2], [0.7, 0.7]])
    np.testing.assert_array_equal(C, [[-0.9], [-0.2]])
    assert sm.n_feasible_ == 1 and sm.n_failed == 0        # ... and they are not failures either
    assert not any(k[0] == "feas" and len(k[1]) for k in sm.engine.log)


def test_settings_are_checked_and_passed_through():
    from uptune_amd import technique as T
    for bad in ([("accuracy", ">", 1.0)], [("accuracy", ">=", float("nan"))], [("accuracy", ">=")], "accuracy",
                [("a", "<=", 1.0)] * 5):
        with pytest.raises(ValueError):
            T.SharedModel(constraints=bad)
    cons = [("accuracy", ">=", 0.5)]
    for bad_kw in (dict(prune_rows=64), dict(diversify=16), dict(acq="ucb"), dict(surrogate=object())):
        with pytest.raises(ValueError):
            T.GpuDifferentialEvolution(pool=64, batch=4, constraints=cons, **bad_kw)
        sm = T.SharedModel(constraints=cons, engine_factory=ConsEngine)
        with pytest.raises(ValueError):
            T.GpuGA(pool=64, batch=4, shared=sm, **bad_kw)
    b = T.pso_ga_de_bandit(pool=64, batch=4, constraints=cons, engine_factory=ConsEngine)
    assert all(t.model.constraints == [("accuracy", ">=", 0.5)] for t in b.techniques)
    assert T.SharedModel().constraints == []


def test_threshold_objective_orders_acceptable_before_fast():
    from uptune_amd.driver import MinimizeTime, Result, ThresholdAccuracyMinimizeTime
    obj = ThresholdAccuracyMinimizeTime(0.8)
    slow_ok = Result(time=9.0, accuracy=0.85)
    fast_bad = Result(time=1.0, accuracy=0.5)
    fast_ok = Result(time=2.0, accuracy=0.99)
    worse_bad = Result(time=0.1, accuracy=0.4)
    assert obj.lt(slow_ok, fast_bad) and not obj.lt(fast_bad, slow_ok)
    assert obj.lt(fast_ok, slow_ok)                        # above the target only time counts
    assert obj.lt(fast_bad, worse_bad)                     # below it the more accurate one
    assert obj.lte(slow_ok, slow_ok) and not obj.lt(slow_ok, slow_ok)
    assert obj.is_acceptable(slow_ok) and not obj.is_acceptable(fast_bad) and not obj.is_acceptable(Result(time=1.0))
    assert MinimizeTime().lt(fast_bad, slow_ok)            # the default objective is as it was
    assert Result().accuracy is None and Result(time=1.0).time == 1.0


def _space():
    from uptune_amd.manipulator import ConfigurationManipulator, FloatParameter
    return ConfigurationManipulator([FloatParameter("x0", 0.0, 1.0), FloatParameter("x1", 0.0, 1.0)])


def test_driver_round_trip_with_the_stand_in_engine():
    """the driver stores what a mapping objective measures, the objective ranks
    by it, and the model loads it after every fit of a real run"""
    from uptune_amd import technique as T
    from uptune_amd.driver import SearchDriver, ThresholdAccuracyMinimizeTime

    def objective(cfg):
        return {"time": cfg["x0"] + cfg["x1"], "accuracy": cfg["x0"]}

    tech = T.GpuDifferentialEvolution(pool=256, batch=4, population=32, seed=3, engine_factory=ConsEngine,
                                      constraints=[("accuracy", ">=", 0.5)], name="de")
    drv = SearchDriver(_space(), tech, objective=ThresholdAccuracyMinimizeTime(0.5), parallelism=4)
    drv.main(objective, test_limit=8 * 4 - 1, max_generations=8)
    tech = drv.root_technique
    res = drv.results_query()
    assert len(res) >= 24 and all(r.accuracy == r.configuration.data["x0"] for r in res)
    assert drv.best_result.accuracy >= 0.5                 # the objective's best, not the fastest
    eng, model = tech.engine, tech.model
    fits = [i for i, e in enumerate(eng.log) if e[0] == "fit"]
    assert fits and all(eng.log[i + 1][0] == "cons" for i in fits)
    kind, C, thr = eng.log[-1]
    np.testing.assert_array_equal(thr, [-0.5])
    np.testing.assert_array_equal(C[:, 0], -eng.log[-2][1][:, 0])      # x0 is feature 0
    assert model.n_feasible_ == int((C[:, 0] <= -0.5).sum()) == eng.gp_cons_info()["n_feasible"]
    with pytest.raises(ValueError, match="no measurement"):
        drv.report(types.SimpleNamespace(configuration=res[0].configuration, requestor="t", key="k"),
                   {"time": 1.0, "speed": 2.0})
    cp = copy.deepcopy(tech)
    assert cp.model.engine is None and cp.model.n_feasible_ is None and cp.model.constraints == model.constraints
