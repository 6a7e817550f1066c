"""Two objectives without a GPU: the restated front rule and EHVI
(tests/_mo_oracle.py) have the properties the definition promises, the host
side (uptune_amd.pareto, driver.ParetoMinimize) keeps a front, and the settings
refuse what is not built.  Every test but the MinimizeTime one fails without
the feature: uptune_amd.pareto, ParetoMinimize and `objectives=` do not exist."""
import types

import numpy as np
import pytest

from _mo_oracle import ehvi, ehvi_mp, front_rows, gain, psi
from uptune_amd import technique as T
from uptune_amd.driver import Configuration, DesiredResult, MinimizeTime, ParetoMinimize, Result, SearchDriver
from uptune_amd.manipulator import ConfigurationManipulator, FloatParameter
from uptune_amd.pareto import default_ref, hypervolume2d, nondominated


def _front(P, rng, r=(2.0, 2.0)):
    """an ordered front of P points inside the box below r"""
    a = np.sort(rng.uniform(-2.0, r[0] - 0.1, P))
    b = np.sort(rng.uniform(-2.0, r[1] - 0.1, P))[::-1]
    return a, b


def test_gain_is_the_plain_hypervolume_difference():
    """the strips' areas against hypervolume2d(F + point) - hypervolume2d(F),
    point by point; and psi at var == 0 gives exactly that gain"""
    rng = np.random.default_rng(0)
    a, b = _front(7, rng)
    F = np.column_stack([a, b])
    ref = (2.0, 2.0)
    base = hypervolume2d(F, ref)
    pts = rng.uniform(-2.5, 2.5, (200, 2))
    want = np.array([hypervolume2d(np.vstack([F, p]), ref) - base for p in pts])
    got = gain(pts[:, 0], pts[:, 1], a, b, *ref)
    np.testing.assert_allclose(got, want, rtol=0.0, atol=1e-12)
    assert (want > 0).sum() > 50 and (want == 0).sum() > 20
    flat = ehvi(pts[:, 0], np.zeros(200), pts[:, 1], a, b, *ref)
    np.testing.assert_allclose(flat, want, rtol=0.0, atol=1e-12)


@pytest.mark.parametrize("mu,sigma,dominated", [((0.0, 0.0), 0.5, None), ((-1.0, 1.0), 1.0, None),
                                                ((1.5, 1.5), 0.6, True)])
def test_ehvi_is_the_mean_gain_of_a_monte_carlo(mu, sigma, dominated):
    """(the third setting's mean is a dominated point: only its spread gains)"""
    rng = np.random.default_rng(1)
    a, b = _front(9, rng)
    ref = (2.0, 2.0)
    if dominated:
        assert gain(np.array([mu[0]]), np.array([mu[1]]), a, b, *ref)[0] == 0.0
    N = 400000
    y1 = mu[0] + sigma * rng.standard_normal(N)
    y2 = mu[1] + sigma * rng.standard_normal(N)
    g = gain(y1, y2, a, b, *ref)
    want, se = g.mean(), g.std(ddof=1) / np.sqrt(N)
    got = float(ehvi(np.array([mu[0]]), np.array([sigma ** 2]), np.array([mu[1]]), a, b, *ref)[0])
    print("mu %r sigma %g: EHVI %.6g, Monte Carlo %.6g +- %.2g" % (mu, sigma, got, want, se))
    assert se > 0.0 and got >= 0.0 and abs(got - want) <= 4.0 * se


def test_front_rule():
    # identical points keep the smallest row; a strictly ascending, b strictly descending
    a = np.array([0.0, 1.0, 0.0, 2.0, 1.0, -1.0, 0.5])
    b = np.array([1.0, 0.0, 1.0, 3.0, 0.0, 2.0, 0.5])
    rows = front_rows(a, b)
    assert rows.tolist() == [5, 0, 6, 1]
    assert np.all(np.diff(a[rows]) > 0) and np.all(np.diff(b[rows]) < 0)
    assert nondominated(np.column_stack([a, b])).tolist() == rows.tolist()
    # a row with a = r1 exactly is outside the box
    assert front_rows(a, b, r1=1.0, r2=10.0).tolist() == [5, 0, 6]
    # P = 0 and P = n
    assert front_rows(a, b, r1=-5.0, r2=-5.0).size == 0
    t = np.linspace(0.0, 1.0, 11)
    assert front_rows(t, -t).tolist() == list(range(11))
    rng = np.random.default_rng(2)
    for _ in range(20):
        p = np.round(rng.uniform(0, 1, (40, 2)), 1)     # many ties
        assert nondominated(p).tolist() == front_rows(p[:, 0], p[:, 1]).tolist()


def test_empty_front_is_the_product_of_two_improvements():
    mu1, mu2, var = np.array([0.3, -1.0]), np.array([0.1, 2.0]), np.array([0.25, 0.0])
    got = ehvi(mu1, var, mu2, np.zeros(0), np.zeros(0), 1.0, 1.5)
    np.testing.assert_array_equal(got, psi(1.0, mu1, var) * psi(1.5, mu2, var))


def test_a_dominated_row_changes_nothing():
    rng = np.random.default_rng(3)
    a, b = rng.standard_normal(30), rng.standard_normal(30)
    r = (2.5, 2.5)
    rows = front_rows(a, b, *r)
    mu1, mu2, var = rng.standard_normal(50), rng.standard_normal(50), rng.uniform(0.01, 1.0, 50)
    base = ehvi(mu1, var, mu2, a[rows], b[rows], *r)
    a2, b2 = np.append(a, a[rows[0]] + 0.1), np.append(b, b[rows[0]] + 0.1)
    rows2 = front_rows(a2, b2, *r)
    assert rows2.tolist() == rows.tolist()
    np.testing.assert_array_equal(ehvi(mu1, var, mu2, a2[rows2], b2[rows2], *r), base)
    assert (base >= 0.0).all()


def test_hypervolume_agrees_with_a_grid_count():
    rng = np.random.default_rng(4)
    p = rng.uniform(0.0, 1.0, (12, 2))
    ref = (1.0, 0.9)
    G = 1000
    x = (np.arange(G) + 0.5) / G
    X, Y = np.meshgrid(x * ref[0], x * ref[1], indexing="ij")
    dom = np.zeros((G, G), dtype=bool)
    for q in p:
        dom |= (X >= q[0]) & (Y >= q[1])
    want = dom.mean() * ref[0] * ref[1]
    got = hypervolume2d(p, ref)
    print("hypervolume %.6f, grid %.6f" % (got, want))
    assert abs(got - want) <= 2.0 * 12 / G        # at most the cells the front's 2 P edges cross
    assert hypervolume2d(np.zeros((0, 2)), ref) == 0.0
    assert hypervolume2d(p + 2.0, ref) == 0.0


def test_default_ref():
    p = np.array([[1.0, 5.0], [3.0, 5.0], [2.0, 5.0]])
    np.testing.assert_array_equal(default_ref(p), [3.2, 6.0])


def test_fp64_against_forty_digits():
    """the restatement against a 40-digit evaluation to 1e-10 relative wherever
    the value is at least 1e-80 (below, phi's rounding dominates and underflows:
    tests/test_gpu_cons.py's docstring has the argument for EI); a 300-point
    front"""
    rng = np.random.default_rng(5)
    a, b = _front(300, rng)
    K = 48
    mu1, mu2 = rng.uniform(-3.0, 3.0, K), rng.uniform(-3.0, 3.0, K)
    var = 10.0 ** rng.uniform(-6.0, 0.5, K)
    got = ehvi(mu1, var, mu2, a, b, 2.0, 2.0)
    worst, big = 0.0, 0
    for k in range(K):
        want = ehvi_mp(mu1[k], var[k], mu2[k], a, b, 2.0, 2.0)
        if want >= 1e-80:
            big += 1
            worst = max(worst, float(abs(got[k] - want) / want))
        else:
            assert 0.0 <= got[k] <= 2e-80
    print("fp64 vs 40 digits: %d of %d cases >= 1e-80, worst relative error %.3g" % (big, K, worst))
    assert big >= K // 2 and worst <= 1e-10


# ---- the driver's side -------------------------------------------------------
def _result(i, time, size=None):
    r = Result(Configuration(i, "h%d" % i, {"x": i}), time, id=i)
    r.size = size
    return r


def test_pareto_minimize_keeps_the_front():
    o = ParetoMinimize("size")
    stream = [(5.0, 5.0), (6.0, 6.0), (4.0, 7.0), (5.0, 5.0), (3.0, None), (4.5, 4.0), (4.0, 7.0), (1.0, 9.0)]
    want = [True, False, True, False, False, True, False, True]
    rs = [_result(i, t, s) for i, (t, s) in enumerate(stream)]
    assert [o.admit(r) for r in rs] == want
    # (4.5, 4) evicted (5, 5); the front by time
    assert [r.id for r in o.pareto_front()] == [7, 2, 5]
    assert o.lt(rs[5], rs[0]) and not o.lt(rs[0], rs[5]) and not o.lt(rs[2], rs[5]) and not o.lt(rs[5], rs[2])
    assert o.lte(rs[2], rs[5]) and o.lte(rs[5], rs[2]) and not o.lte(rs[0], rs[5])
    assert not o.lt(rs[4], rs[1]) and o.lt(rs[1], rs[4])         # no second measurement: dominates nothing
    m = ParetoMinimize("accuracy", maximize=True)
    hi, lo = _result(0, 1.0), _result(1, 1.0)
    hi.accuracy, lo.accuracy = 0.9, 0.5
    assert m.lt(hi, lo) and not m.lt(lo, hi)
    with pytest.raises(ValueError):
        ParetoMinimize("colour")


class _Fixed(T.SearchTechnique):
    """asks for x = 0, 1, 2, ... in turn"""

    def __init__(self):
        super().__init__(name="fixed")
        self.i = 0

    def desired_configuration(self):
        self.i += 1
        return {"x": float(self.i - 1)}


def _drive(objective, values):
    m = ConfigurationManipulator([FloatParameter("x", 0.0, 100.0)])
    d = SearchDriver(m, _Fixed(), objective=objective, parallelism=1, hash_fn=lambda c: "k%r" % c["x"])
    flags, bests = [], []
    for v in values:
        assert d.run_generation_techniques() == 1
        dr = d.pending_desired_results()[0]
        d.report(dr, v)
        d.process_new_results()
        flags.append(dr.result.was_new_best)
        bests.append(None if d.best_result is None else d.best_result.id)
    return d, flags, bests


def test_driver_credits_admission_and_keeps_the_fastest_member_as_best():
    vals = [dict(time=5.0, size=5.0), dict(time=6.0, size=6.0), dict(time=4.0, size=7.0), 3.0,
            dict(time=4.5, size=4.0), dict(time=4.0, size=6.5)]
    d, flags, bests = _drive(ParetoMinimize("size"), vals)
    assert flags == [True, False, True, False, True, True]
    assert bests == [0, 0, 2, 2, 2, 5]
    front = d.pareto_front()
    assert [(r.time, r.size) for r in front] == [(4.0, 6.5), (4.5, 4.0)]
    from uptune_amd.driver import TuningRunManager
    assert TuningRunManager.get_pareto_front is not None


def test_minimize_time_runs_are_unchanged():
    times = [5.0, 6.0, 4.0, 4.0, 3.0, 7.0]
    d, flags, bests = _drive(MinimizeTime(), times)
    assert flags == [True, False, True, False, True, False]
    assert bests == [0, 0, 2, 2, 4, 4]
    assert [r.id for r in d.pareto_front()] == [4]


# ---- the model's side --------------------------------------------------------
class _Eng:
    """records gp_fit / gp_mo_set in call order"""
    spec = types.SimpleNamespace(n_features=2)

    def __init__(self):
        self.log = []

    def features_host(self, cfgs):
        return np.asarray([[c["a"], c["b"]] for c in cfgs], dtype=np.float64)

    def gp_fit(self, X, y, lengthscale, wait=True, **hyper):
        self.log.append(("fit", np.array(X), np.array(y)))

    def gp_fit_ok(self):
        return True

    def gp_mo_set(self, Y2, ref):
        self.log.append(("mo", np.array(Y2), tuple(ref)))


def _rows_driver():
    rows = []

    def add(a, b, t, **extra):
        r = types.SimpleNamespace(configuration=types.SimpleNamespace(data={"a": a, "b": b}, hash="h%d" % len(rows)),
                                  time=t, state="OK", id=len(rows))
        for k, v in extra.items():
            setattr(r, k, v)
        rows.append(r)

    return rows, add, types.SimpleNamespace(results_query=lambda: rows)


@pytest.mark.parametrize("sense", ["min", "max"])
def test_shared_model_loads_the_second_objective_after_every_fit(sense):
    rng = np.random.default_rng(6)
    rows, add, drv = _rows_driver()
    sm = T.SharedModel(objectives=[("time", "min"), ("accuracy", sense)], min_train=4)
    sm.engine = _Eng()
    sign = -1.0 if sense == "max" else 1.0

    def grow(n):
        while len(rows) < n:
            a, b = rng.uniform(size=2)
            add(a, b, float(rng.uniform()), accuracy=float(7.0 * a))

    def check(n):
        (kind, X, y), (kind2, Y2, ref) = sm.engine.log[-2:]
        assert (kind, kind2) == ("fit", "mo"), "gp_mo_set follows gp_fit directly"
        assert X.shape == (n, 2) and Y2.shape == (n,)
        np.testing.assert_array_equal(Y2, sign * 7.0 * X[:, 0])      # row r's own value, "max" negated
        return y, Y2, ref

    grow(100)
    add(0.5, 0.5, 0.25)                                    # no second measurement: not a row
    assert sm.fit(drv)
    y, Y2, ref0 = check(100)
    np.testing.assert_array_equal(ref0, default_ref(np.column_stack([y, Y2])))
    assert ref0 == sm.ref_point_
    grow(131)
    assert sm.fit(drv)
    y, Y2, ref = check(130)
    assert ref == ref0                                     # held from the first fit on
    assert sm.fit(drv) and len(sm.engine.log) == 4         # nothing new: neither call again
    # a given reference point: raw units, the second coordinate signed as the values are
    sm2 = T.SharedModel(objectives=[("time", "min"), ("accuracy", sense)], ref_point=(2.0, 9.0), min_train=4)
    sm2.engine = _Eng()
    assert sm2.fit(drv) and sm2.engine.log[-1][2] == (2.0, sign * 9.0)
    sm3 = T.SharedModel(objectives=[("time", "min"), ("accuracy", sense)], ref_point=(0.5, 9.0), min_train=4,
                        y_transform="rank")
    sm3.engine = _Eng()
    assert sm3.fit(drv)
    y3, r3 = sm3.engine.log[-2][2], sm3.engine.log[-1][2]
    raw = np.array([r.time for r in rows if hasattr(r, "accuracy")])
    assert abs(np.mean(y3 < r3[0]) - np.mean(raw < 0.5)) <= 1.0 / len(raw)    # the same rank among the rows


# ---- settings ---------------------------------------------------------------
MO = [("time", "min"), ("size", "min")]


def test_settings_refuse_what_is_not_built():
    for bad in ([("time", "min")], [("time", "min"), ("size", "min"), ("energy", "min")], [("size", "min"), ("time", "min")],
                [("time", "max"), ("size", "min")], [("time", "min"), ("colour", "min")], [("time", "min"), ("size", "low")]):
        with pytest.raises(ValueError, match="objectives"):
            T.SharedModel(objectives=bad)
    for bad_kw in (dict(constraints=[("accuracy", ">=", 0.5)]), dict(feasibility=True), dict(surrogate="forest")):
        with pytest.raises(ValueError, match="objectives"):
            T.SharedModel(objectives=MO, **bad_kw)
    with pytest.raises(ValueError, match="ref_point"):
        T.SharedModel(ref_point=(1.0, 2.0))
    with pytest.raises(ValueError, match="ref_point"):
        T.SharedModel(objectives=MO, ref_point=(1.0, float("inf")))
    for bad_kw in (dict(prune_rows=64), dict(diversify=16), dict(acq="ucb"), dict(acq="ts"), dict(polish=2),
                   dict(constraints=[("accuracy", ">=", 0.5)]), dict(feasibility=True), dict(surrogate="forest")):
        with pytest.raises(ValueError, match="objectives"):
            T.GpuDifferentialEvolution(pool=64, batch=4, objectives=MO, **bad_kw)
        with pytest.raises(ValueError):
            T.pso_ga_de_bandit(pool=64, batch=4, objectives=MO, **bad_kw)
    # a shared model carries the setting
    sm = T.SharedModel(objectives=MO)
    with pytest.raises(ValueError, match="objectives"):
        T.GpuDifferentialEvolution(pool=64, batch=4, shared=sm, prune_rows=64)
    b = T.pso_ga_de_bandit(pool=64, batch=4, objectives=[("time", "min"), ("accuracy", "max")], ref_point=(9.0, 0.1))
    assert all(t.model.objectives == [("time", "min"), ("accuracy", "max")] for t in b.techniques)
    assert b.techniques[0].model.ref_point == (9.0, 0.1)
    assert T.SharedModel().objectives == []
