"""The LML gradient oracle (tests/_lml_grad_oracle.py) against central finite
differences of the LML and against a long-double evaluation, and
SharedModel(lengthscale="ard") (technique.py) over an oracle-backed stand-in
engine.  CPU only.

Errors are |got - want| / S with S the sum of the component's absolute terms
(_lml_grad_oracle).  Measured at the shapes below:
  finite differences (h = 1e-5 in log ell): <= 1.6e-10      (bound 1e-9)
  long double, ell: <= 6e-16, sf2: <= 5e-18                 (bound 1e-14)
  long double, sn2: <= 9e-14 at sn2 = 1e-2, 9e-10 at 1e-6   (bounds 1e-12, 1e-8:
  K^-1's diagonal carries cond(K) ~ n sf2 / sn2 roundings, so the bound at 1e-6
  scales to 1e-2 with the noise)"""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _lml_grad_oracle as G  # noqa: E402
import _lml_oracle as O  # noqa: E402
from _oracle_engine import OracleEngine  # noqa: E402
from uptune_amd.manipulator import (BooleanParameter, ConfigurationManipulator, EnumParameter,  # noqa: E402
                                    FloatParameter)
from uptune_amd.technique import SharedModel  # noqa: E402

SHAPES = [(100, 5), (200, 37), (321, 3)]
NOISES = [1e-2, 1e-6]


@pytest.mark.parametrize("sn2", NOISES)
@pytest.mark.parametrize("n,d", SHAPES)
def test_oracle_matches_finite_differences(n, d, sn2):
    X, y = O.data(n, d)
    ell = O.ard_base(d)
    want = G.grad(X, y, ell, sigma_n2=sn2)
    h = 1e-5
    worst = 0.0
    for k in range(d):
        up, dn = ell.copy(), ell.copy()
        up[k] *= np.exp(h)
        dn[k] *= np.exp(-h)
        fd = (O.lml(X, y, up, sigma_n2=sn2) - O.lml(X, y, dn, sigma_n2=sn2)) / (2.0 * h)
        worst = max(worst, abs(fd - want.ell[k]) / want.S_ell[k])
    print(f"finite differences n={n} d={d} sn2={sn2:g}: max |err| / S {worst:.3e}")
    assert worst <= 1e-9


@pytest.mark.parametrize("sn2", NOISES)
@pytest.mark.parametrize("n,d", SHAPES)
def test_oracle_matches_long_double(n, d, sn2):
    X, y = O.data(n, d)
    ell = O.ard_base(d)
    got = G.grad(X, y, ell, sigma_n2=sn2)
    e_ell, e_sf2, e_sn2 = G.errors((got.ell, got.sf2, got.sn2), G.grad_longdouble(X, y, ell, sigma_n2=sn2))
    print(f"long double n={n} d={d} sn2={sn2:g}: ell {e_ell:.3e} sf2 {e_sf2:.3e} sn2 {e_sn2:.3e}")
    assert e_ell <= 1e-14 and e_sf2 <= 1e-14
    assert e_sn2 <= (1e-8 if sn2 == 1e-6 else 1e-12)


# ---------------------------------------------------------------------------
# SharedModel(lengthscale="ard") over the oracle
# ---------------------------------------------------------------------------
class ArdEngine(OracleEngine):
    """OracleEngine with the LML, its gradient and the grid, recording every call"""

    def __init__(self, manip):
        super().__init__(manip)
        self.ells, self.waits, self.grids, self.evals = [], [], [], 0
        self.all_nan = False
        self.flat = False         # every point's LML is the same: nothing improves on the start
        self._sn2 = 0.0

    def gp_fit(self, X, y, lengthscale, **kw):
        self.ells.append(lengthscale)
        self.waits.append(kw.get("wait", True))
        self._fit_xy = (np.array(X), np.array(y))
        self._sn2 = kw.get("sigma_n2", 1e-6)
        super().gp_fit(X, y, lengthscale, **kw)

    def gp_lml(self):
        if self.flat:
            return -1e9
        g = self.gp
        return float(-0.5 * g.ys @ g.alpha - np.log(np.diag(g.L)).sum() - 0.5 * len(g.ys) * np.log(2.0 * np.pi))

    def gp_lml_grad(self):
        self.evals += 1
        r = G.from_gp(self.gp, self._sn2)
        return r.ell, float(r.sf2), float(r.sn2)

    def gp_lml_grid(self, X, y, lengthscale, scales, noises=None, sigma_f2=1.0, sigma_n2=1e-6, jitter=0.0):
        self.grids.append(np.array(scales))
        if self.all_nan:
            return np.full(len(scales), np.nan), -1
        return O.lml_grid(X, y, lengthscale, scales, noises, sigma_f2, sigma_n2, jitter)


def float_manip(d):
    return ConfigurationManipulator([FloatParameter(f"x{k}", 0.0, 1.0) for k in range(d)])


def rows_of(names, X, y):
    return [types.SimpleNamespace(configuration=types.SimpleNamespace(data=dict(zip(names, X[i]))), time=float(y[i]),
                                  state="OK", id=i) for i in range(len(y))]


def rehearsal():
    """n = 80, d = 6: the objective depends on features 0 and 1 only"""
    rng = np.random.default_rng(7)
    X = rng.uniform(size=(80, 6))
    y = np.sin(3.0 * X[:, 0]) + (X[:, 1] - 0.3) ** 2 + 0.01 * rng.standard_normal(80)
    return X, y


def model(manip, **kw):
    m = SharedModel(lengthscale="ard", **kw)
    m.engine = ArdEngine(manip)
    return m


def test_ard_separates_the_features_that_matter():
    X, y = rehearsal()
    m = model(float_manip(6), sigma_n2=1e-4, jitter=0.0)
    rows = rows_of([f"x{k}" for k in range(6)], [list(map(float, r)) for r in X], y)
    assert m.fit(types.SimpleNamespace(results_query=lambda: rows))
    e = m.engine
    n, ell, val = m.ell_history[-1]
    assert n == 80 and ell is m.lengthscale_ and isinstance(ell, np.ndarray) and ell.shape == (6,)
    assert ell.flags["C_CONTIGUOUS"]
    print("ard lengthscales", ell, "lml", val, "evaluations", e.evals)
    assert np.min(ell[2:]) > np.max(ell[:2])
    # never worse than the isotropic start, and every evaluation was a waited fit; the
    # fit that follows the selection is asynchronous and takes the array itself
    grid = e.grids[0]
    start, best = O.lml_grid(m._Xf[:80], m._yf[:80], 1.0, grid, **m.hyper)
    assert val >= start[best]
    assert val == pytest.approx(O.lml(m._Xf[:80], m._yf[:80], ell, **m.hyper), rel=1e-12)
    assert all(e.waits[:-1]) and e.waits[-1] is False and e.ells[-1] is ell
    assert e.evals <= 1 + 2 * 20 * m.ard_maxiter    # L-BFGS-B's line search: at most 20 steps per iteration
    # bounds: every ell within [grid min, 4 grid max]
    assert all(np.all(np.asarray(v) >= grid.min() * (1 - 1e-12)) and np.all(np.asarray(v) <= 4 * grid.max() * (1 + 1e-12))
               for v in e.ells)


class _Driver:
    def __init__(self, d, seed=0):
        self.rows, self.d = [], d
        self.rng = np.random.default_rng(seed)

    def add(self, k):
        for _ in range(k):
            x = self.rng.uniform(size=self.d)
            cfg = {f"x{j}": float(x[j]) for j in range(self.d)}
            t = float(np.sin(3.0 * x[0]) + 0.01 * self.rng.standard_normal())
            self.rows.append(types.SimpleNamespace(configuration=types.SimpleNamespace(data=cfg), time=t, state="OK",
                                                   id=len(self.rows)))

    def results_query(self):
        return self.rows


def test_ard_selects_at_the_first_fit_and_at_a_new_padded_size_only():
    m, d = model(float_manip(3), ard_maxiter=5, sigma_n2=1e-4), _Driver(3)
    d.add(20)
    assert m.fit(d)
    e = m.engine
    assert len(e.grids) == 1 and len(m.ell_history) == 1
    first = m.lengthscale_
    nfit = len(e.ells)
    while len(d.rows) < 128:
        d.add(min(54, 128 - len(d.rows)))
        assert m.fit(d)
    # no selection in between: one fit per call, the same array, bit for bit
    assert len(e.grids) == 1 and len(e.ells) == nfit + 2
    assert all(v is first for v in e.ells[nfit - 1:]) and m.lengthscale_ is first
    before = first.copy()
    d.add(1)                     # 129 rows: a new padded size
    assert m.fit(d)
    assert len(e.grids) == 2 and [h[0] for h in m.ell_history] == [20, 129]
    assert np.array_equal(first, before)          # the earlier array was left as it was
    assert m.lengthscale_ is not first and e.ells[-1] is m.lengthscale_
    assert m.ell_history[-1][2] >= O.lml_grid(m._Xf[:129], m._yf[:129], 1.0, e.grids[-1], **m.hyper)[0].max()


def test_all_nan_grid_or_no_improvement_keeps_the_choice():
    m, d = model(float_manip(3), ard_maxiter=5, sigma_n2=1e-4), _Driver(3, seed=1)
    d.add(100)
    assert m.fit(d)
    first = m.lengthscale_
    m.engine.all_nan = True
    d.add(40)
    assert m.fit(d)
    assert m.lengthscale_ is first and m.engine.ells[-1] is first
    assert m.ell_history[-1][0] == 140 and np.isnan(m.ell_history[-1][2])
    # nothing to keep on a first fit: the grid's median, per feature
    m2, d2 = model(float_manip(3)), _Driver(3, seed=2)
    m2.engine.all_nan = True
    d2.add(10)
    assert m2.fit(d2)
    grid = m2.engine.grids[0]
    assert np.array_equal(m2.lengthscale_, np.full(3, np.median(grid)))
    # no point improves on the start: the isotropic grid choice stays, exactly
    m3, d3 = model(float_manip(3), ard_maxiter=5, sigma_n2=1e-4), _Driver(3, seed=3)
    m3.engine.flat = True
    d3.add(30)
    assert m3.fit(d3)
    grid = m3.engine.grids[0]
    lml, best = O.lml_grid(m3._Xf[:30], m3._yf[:30], 1.0, grid, **m3.hyper)
    assert np.array_equal(m3.lengthscale_, np.full(3, grid[best])) and m3.ell_history[-1][2] == lml[best]


def test_a_point_that_is_not_positive_definite_is_rejected_not_raised():
    class Picky(ArdEngine):
        def gp_fit(self, X, y, lengthscale, **kw):
            super().gp_fit(X, y, lengthscale, **kw)
            if np.ptp(np.asarray(lengthscale, dtype=np.float64)) > 0.0 and kw.get("wait", True):
                self.gp_ok = False     # every anisotropic point fails

    m, d = SharedModel(lengthscale="ard", ard_maxiter=5, sigma_n2=1e-4), _Driver(3, seed=4)
    m.engine = Picky(float_manip(3))
    d.add(30)
    assert m.fit(d)
    grid = m.engine.grids[0]
    _, best = O.lml_grid(m._Xf[:30], m._yf[:30], 1.0, grid, **m.hyper)
    assert np.array_equal(m.lengthscale_, np.full(3, grid[best]))


def test_one_hot_columns_share_one_lengthscale():
    manip = ConfigurationManipulator([FloatParameter("a", 0.0, 1.0), EnumParameter("e1", ["p", "q", "r"]),
                                      BooleanParameter("b"), FloatParameter("c", 0.0, 1.0),
                                      EnumParameter("e2", ["u", "v"])])
    rng = np.random.default_rng(11)
    rows = []
    for i in range(60):
        cfg = {"a": float(rng.uniform()), "e1": "pqr"[rng.integers(3)], "b": bool(rng.integers(2)),
               "c": float(rng.uniform()), "e2": "uv"[rng.integers(2)]}
        t = np.sin(3.0 * cfg["a"]) + (0.5 if cfg["e1"] == "q" else 0.0) + 0.01 * rng.standard_normal()
        rows.append(types.SimpleNamespace(configuration=types.SimpleNamespace(data=cfg), time=float(t), state="OK", id=i))
    m = model(manip, ard_maxiter=10, sigma_n2=1e-4)
    assert m.fit(types.SimpleNamespace(results_query=lambda: rows))
    ell = m.lengthscale_
    assert ell.shape == (8,)                      # a | e1 x 3 | b | c | e2 x 2
    cat = [1, 2, 3, 4, 6, 7]
    assert len({float(v) for v in ell[cat]}) == 1
    assert np.array_equal(m._ell_groups(8), [0, 1, 1, 1, 1, 2, 1, 1])
    assert m.ell_history[-1][2] > O.lml_grid(m._Xf[:60], m._yf[:60], 1.0, m.engine.grids[0], **m.hyper)[0].max()


def test_other_strings_still_raise():
    for s in ("fit", "ARD", ""):
        with pytest.raises(ValueError):
            SharedModel(lengthscale=s)
    assert SharedModel(lengthscale="ard", ard_maxiter=7).ard_maxiter == 7


def test_the_option_reaches_the_model_through_the_techniques():
    from uptune_amd.technique import GpuDifferentialEvolution, pso_ga_de_bandit
    assert GpuDifferentialEvolution(lengthscale="ard").model.lengthscale == "ard"
    models = {id(t.model): t.model for t in pso_ga_de_bandit(lengthscale="ard").techniques}
    assert len(models) == 1 and all(m.lengthscale == "ard" and m.lengthscale_ is None for m in models.values())
