"""SharedModel(lengthscale="auto") (technique.py): the lengthscale is the grid
candidate with the largest log marginal likelihood, chosen at the first fit and
wherever the fit's padded size (128 rows, ut_internal.h NPAD) changes -- never between,
so the device's incremental fits keep identical hyperparameters.  CPU only: the
oracle engine grows a gp_lml_grid built on oracle/gp.py and records every call."""
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _lml_oracle as O  # noqa: E402
from _oracle_engine import OracleEngine  # noqa: E402
from uptune_amd.manipulator import ConfigurationManipulator, FloatParameter  # noqa: E402
from uptune_amd.technique import SharedModel  # noqa: E402

D = 3
GRID = np.sqrt(D) * np.geomspace(0.05, 4.0, 6)


class LmlEngine(OracleEngine):
    def __init__(self):
        super().__init__(ConfigurationManipulator([FloatParameter(f"x{k}", 0.0, 1.0) for k in range(D)]))
        self.ells = []        # the lengthscale of every gp_fit
        self.fit_y = []
        self.grids = []       # (X, y, lengthscale, scales, hyper) of every gp_lml_grid
        self.all_nan = False

    def gp_fit(self, X, y, lengthscale, **kw):
        self.ells.append(lengthscale)
        self.fit_y.append(np.array(y))
        super().gp_fit(X, y, lengthscale, **kw)

    def gp_lml_grid(self, X, y, lengthscale, scales, noises=None, sigma_f2=1.0, sigma_n2=1e-6, jitter=0.0):
        self.grids.append((np.array(X), np.array(y), lengthscale, np.array(scales),
                           dict(sigma_f2=sigma_f2, sigma_n2=sigma_n2, jitter=jitter)))
        if self.all_nan:
            return np.full(len(scales), np.nan), -1
        return O.lml_grid(X, y, lengthscale, scales, noises, sigma_f2, sigma_n2, jitter)


class _Driver:
    def __init__(self, seed=0):
        self.rows = []
        self.rng = np.random.default_rng(seed)

    def add(self, k):
        for _ in range(k):
            x = self.rng.uniform(size=D)
            cfg = {f"x{j}": float(x[j]) for j in range(D)}
            t = float(np.sum((x - 0.4) ** 2) + 0.01 * self.rng.standard_normal())
            self.rows.append(types.SimpleNamespace(configuration=types.SimpleNamespace(data=cfg), time=t, state="OK",
                                                   id=len(self.rows)))

    def results_query(self):
        return self.rows


def model(**kw):
    m = SharedModel(lengthscale="auto", **kw)
    m.engine = LmlEngine()
    return m


def test_selects_at_the_first_fit_and_at_a_new_padded_size_only():
    m, d = model(ell_grid=GRID), _Driver()
    d.add(5)
    assert m.fit(d)
    e = m.engine
    assert len(e.grids) == 1 and len(m.ell_history) == 1
    first = m.lengthscale_
    # fits that share the padded size pass the same lengthscale, bit for bit: the
    # incremental fit's precondition of identical hyperparameters holds
    while len(d.rows) < 128:
        d.add(min(41, 128 - len(d.rows)))
        assert m.fit(d)
    assert len(e.ells) == 4 and len(e.grids) == 1
    assert all(isinstance(v, float) and v == first for v in e.ells)
    # 129 rows: npad 256, the rows are re-sorted and the device refactors: select again
    d.add(1)
    assert m.fit(d)
    assert len(e.grids) == 2 and len(m.ell_history) == 2
    assert e.ells[-1] == m.lengthscale_
    # the choice is the grid's argmax, computed here from the oracle alone
    for (X, y, base, scales, hyp), (n, ell, val) in zip(e.grids, m.ell_history):
        assert base == 1.0 and np.array_equal(scales, GRID) and hyp == m.hyper
        want = np.array([O.lml(X, y, s, **hyp) for s in GRID])
        assert n == len(y) and ell == GRID[int(np.nanargmax(want))] and val == np.nanmax(want)
    assert [h[0] for h in m.ell_history] == [5, 129]
    # the grid saw the fit's own rows and targets
    assert np.array_equal(e.grids[-1][0], m._Xf[:129]) and np.array_equal(e.grids[-1][1], e.fit_y[-1])
    # the same results again: neither a fit nor a selection
    assert m.fit(d) and len(e.ells) == 5 and len(e.grids) == 2


def test_default_grid():
    m, d = model(), _Driver(1)
    d.add(20)
    assert m.fit(d)
    assert np.array_equal(m.engine.grids[0][3], np.sqrt(D) * np.geomspace(0.05, 4.0, 16))
    assert m.lengthscale_ in m.engine.grids[0][3]


def test_all_nan_grid_keeps_the_previous_choice():
    m, d = model(ell_grid=GRID), _Driver(2)
    d.add(100)
    assert m.fit(d)
    first = m.lengthscale_
    m.engine.all_nan = True
    d.add(40)                     # 140 rows: a new padded size
    assert m.fit(d)
    assert len(m.engine.grids) == 2 and m.lengthscale_ == first and m.engine.ells[-1] == first
    assert m.ell_history[-1][:2] == (140, first) and np.isnan(m.ell_history[-1][2])
    # nothing to keep on a first fit: the grid's median
    m2, d2 = model(ell_grid=GRID), _Driver(3)
    m2.engine.all_nan = True
    d2.add(10)
    assert m2.fit(d2)
    assert m2.lengthscale_ == float(np.median(GRID)) and m2.engine.ells == [m2.lengthscale_]


def test_rank_transform_reaches_the_grid():
    from scipy.special import ndtri
    m, d = model(ell_grid=GRID, y_transform="rank"), _Driver(4)
    d.add(50)
    assert m.fit(d)
    y = m.engine.grids[0][1]
    assert np.array_equal(y, m.engine.fit_y[0])
    assert np.array_equal(np.sort(y), ndtri((np.arange(50) + 0.5) / 50))


def test_a_number_never_selects():
    m = SharedModel(lengthscale=0.3)
    m.engine = LmlEngine()
    d = _Driver(5)
    for k in (100, 60):
        d.add(k)
        assert m.fit(d)
    assert m.engine.grids == [] and m.engine.ells == [0.3, 0.3]
    assert m.lengthscale_ == 0.3 and m.ell_history == []
    with pytest.raises(ValueError):
        SharedModel(lengthscale="fit")
