"""The TPE restatement (tests/_tpe_oracle.py) held to the model's own laws, and what
SharedModel / GpuBatchTechnique accept and refuse with surrogate="tpe".  No GPU."""
import numpy as np
import pytest

import _tpe_oracle as TO


def _case(name):
    rng = np.random.default_rng(5)
    if name == "n2":
        return np.array([[0.25, 1.0], [0.8, 0.0]]), np.array([1.0, 0.0]), [0, 1]
    if name == "ties_and_prior":   # heavy ties, copies of the prior's centre, both ends
        X = rng.choice([0.0, 0.5, 0.5, 0.7, 1.0], size=(37, 2))
        return np.c_[X, np.eye(3)[rng.integers(0, 3, 37)]], rng.normal(size=37), [0, 0, 3, -1, -1]
    X = np.c_[rng.uniform(size=(120, 2)), 0.5 + 1e-4 * rng.uniform(size=120)]
    return X, rng.normal(size=120), None


@pytest.mark.parametrize("name", ["n2", "ties_and_prior", "n120_cluster"])
def test_every_density_is_normalised(name):
    X, y, kinds = _case(name)
    fit = TO.Fit(X, y, kinds)
    # composite Gauss-Legendre, 16 points on each of 1,000 cells: the narrowest sigma is 1/100
    gx, gw = np.polynomial.legendre.leggauss(16)
    edges = np.linspace(0.0, 1.0, 1001)
    x = (edges[:-1, None] + (gx + 1) / 2 * np.diff(edges)[:, None]).ravel()
    w = (gw / 2 * np.diff(edges)[:, None]).ravel()
    for j, sets in fit.num.items():
        for comp in sets:
            assert abs(float((TO.density(x, *comp) * w).sum()) - 1.0) < 1e-12, (j,)
    for j, sets in fit.cat.items():
        for lp in sets:
            assert abs(float(np.exp(lp).sum()) - 1.0) < 1e-15, (j,)
    assert fit.num and (kinds is None or fit.cat)


def test_row_order_of_tied_values_does_not_change_the_mixture():
    X, y, kinds = _case("ties_and_prior")
    y = np.arange(37.0)               # a fixed split: rows 0..3 are good
    a = TO.Fit(X, y, kinds)
    perm = np.r_[np.random.default_rng(1).permutation(4), 4 + np.random.default_rng(2).permutation(33)]
    b = TO.Fit(X[perm], y, kinds)
    for j in a.num:
        for s in range(2):
            for u, v in zip(a.components(j, s), b.components(j, s)):
                np.testing.assert_array_equal(u, v)


def test_surrogate_tpe_is_accepted_and_refuses_what_the_forest_refuses():
    from uptune_amd import technique as T
    m = T.SharedModel(surrogate="tpe", tpe_kw={"gamma": 0.2, "precision": 64})
    assert m.surrogate == "tpe" and m.tpe_kw["gamma"] == 0.2
    assert T.GpuDifferentialEvolution(surrogate="tpe", pool=256).model.surrogate == "tpe"
    assert T.GpuDifferentialEvolution(shared=m, pool=256).surrogate == "tpe"
    assert T.pso_ga_de_bandit(surrogate="tpe", pool=256).techniques[0].model.surrogate == "tpe"
    for kw in (dict(tpe_kw={"bandwidth": 1.0}), dict(feasibility=True), dict(constraints=[("accuracy", ">=", 0.5)]),
               dict(objectives=[("time", "min"), ("accuracy", "max")])):
        with pytest.raises(ValueError, match="tpe_kw|TPE surrogate"):
            T.SharedModel(surrogate="tpe", **kw)
    with pytest.raises(ValueError, match="belongs to surrogate='tpe'"):
        T.SharedModel(tpe_kw={"gamma": 0.2})
    for kw in (dict(feasibility=True), dict(constraints=[("accuracy", ">=", 0.5)]), dict(diversify=16), dict(polish=2),
               dict(objectives=[("time", "min"), ("accuracy", "max")]), dict(acq="ts"), dict(acq="ucb"),
               dict(prune_rows=64)):
        with pytest.raises(ValueError, match="not with a TPE surrogate"):
            T.GpuDifferentialEvolution(surrogate="tpe", pool=256, **kw)
    with pytest.raises(ValueError, match="shared model that fits a GP"):
        T.GpuDifferentialEvolution(surrogate="tpe", shared=T.SharedModel(), pool=256)


def test_a_refit_passes_at_most_8192_rows_the_best_and_the_latest():
    from uptune_amd import technique as T
    seen = {}
    m = T.SharedModel(surrogate="tpe")
    m.engine = type("E", (), {"tpe_fit": lambda self, X, y, **kw: seen.update(X=X, y=y)})()
    m._gather = lambda rows, ids: None
    n = m._n = 9000
    m._ya, m._Xa = np.arange(n, 0.0, -1.0) % 7001.0, np.arange(n, dtype=np.float64)[:, None]
    assert m._fit_tpe([None] * n, list(range(n)))
    kept = seen["X"][:, 0].astype(int)
    assert len(kept) == 8192 and (np.diff(kept) > 0).all() and kept[-1] == n - 1
    assert set(np.argsort(m._ya[:n], kind="stable")[:4096]) <= set(kept)
