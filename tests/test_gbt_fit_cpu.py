"""tests/_gbt_fit_oracle.py, the restatement ut_gbt_fit is held to, checked on
its own: a stump against exhaustive Python, boosting that reduces the training
error, the sample fraction, heap order; and what SharedModel / GpuBatchTechnique
accept and refuse with surrogate="gbt".  No GPU."""
import numpy as np
import pytest

import _gbt_fit_oracle as GB
from _rf_fit_oracle import codes_of

SEED = 11


def _data(n, d, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.random((n, d))
    return X, np.sin(5.0 * X[:, 0]) + X[:, 1 % d] ** 2 + 0.1 * rng.standard_normal(n)


def test_one_round_at_depth_1_is_the_brute_force_stump():
    X, y = _data(60, 3)
    shift, scale = float(np.mean(y)), float(np.std(y))
    roots, nodes, pred = GB.fit(X, y, SEED, n_rounds=1, max_depth=1, eta=1.0, reg_lambda=0.0, subsample=1.0,
                                colsample_bylevel=1.0)
    codes = codes_of(X)
    g = [int(np.rint(-float(v) * 65536.0)) for v in np.clip((y - shift) / scale, -32.0, 32.0)]
    best = (-1.0, None, None)
    for j in range(3):
        for b in range(255):
            L = [gi for gi, c in zip(g, codes[:, j]) if c <= b]
            R = [gi for gi, c in zip(g, codes[:, j]) if c > b]
            if L and R:
                gl, gr = float(sum(L)), float(sum(R))
                s = gl * gl / len(L) + gr * gr / len(R)
                if s > best[0]:
                    best = (s, j, b)
    _, j, b = best
    assert roots.tolist() == [0] and nodes.size == 3
    assert (nodes["feature"][0], nodes["left"][0], nodes["right"][0]) == (j, 1, 2)
    assert nodes["threshold"][0] == (b + 1) / 256.0
    left = codes[:, j] <= b
    for side, k in ((left, 1), (~left, 2)):
        G = sum(gi for gi, m in zip(g, side) if m)
        assert nodes["value"][k] == scale * ((-G / int(side.sum())) / 65536.0)
        np.testing.assert_array_equal(pred[side], nodes["value"][k] / scale)


def test_boosting_beats_the_constant_predictor_and_keeps_heap_order():
    X, y = _data(200, 5, seed=1)
    roots, nodes, pred = GB.fit(X, y, SEED, n_rounds=20, max_depth=3, eta=0.3, subsample=1.0, colsample_bylevel=1.0)
    z = (y - np.mean(y)) / np.std(y)
    assert np.sqrt(np.mean((pred - z) ** 2)) < np.sqrt(np.mean(z ** 2))
    assert roots.size == 20 and (np.diff(roots) > 0).all()
    inner = np.flatnonzero(nodes["feature"] >= 0)
    # breadth first with absent nodes skipped: children follow their parent, left before right, in parent order
    assert (nodes["left"][inner] > inner).all() and (nodes["right"][inner] == nodes["left"][inner] + 1).all()
    assert (np.diff(nodes["left"][inner]) > 0).all()


def test_the_sample_fraction():
    frac = GB.sampled(SEED, 3, 4096, 5, 0.4).mean()
    assert abs(frac - 0.4) <= 0.04
    assert GB.sampled(SEED, 3, 4096, 5, 1.0).all()
    assert (GB.sampled(SEED, 3, 4096, 5, 0.4) != GB.sampled(SEED, 4, 4096, 5, 0.4)).any()


def test_surrogate_gbt_is_accepted_and_refuses_what_tpe_refuses():
    from uptune_amd import technique as T
    m = T.SharedModel(surrogate="gbt", gbt_kw={"n_rounds": 20, "max_depth": 4})
    assert m.surrogate == "gbt" and m.gbt_kw["n_rounds"] == 20
    assert T.GpuDifferentialEvolution(surrogate="gbt", pool=256).model.surrogate == "gbt"
    assert T.GpuDifferentialEvolution(shared=m, pool=256).surrogate == "gbt"
    assert T.pso_ga_de_bandit(surrogate="gbt", gbt_kw={"eta": 0.1}, pool=256).techniques[0].model.gbt_kw == {"eta": 0.1}
    for kw in (dict(gbt_kw={"n_estimators": 5}), dict(feasibility=True), dict(constraints=[("accuracy", ">=", 0.5)]),
               dict(objectives=[("time", "min"), ("accuracy", "max")])):
        with pytest.raises(ValueError, match="gbt_kw|gbt surrogate"):
            T.SharedModel(surrogate="gbt", **kw)
    with pytest.raises(ValueError, match="belongs to surrogate='gbt'"):
        T.SharedModel(gbt_kw={"eta": 0.1})
    for kw in (dict(feasibility=True), dict(constraints=[("accuracy", ">=", 0.5)]), dict(diversify=16), dict(polish=2),
               dict(objectives=[("time", "min"), ("accuracy", "max")]), dict(acq="ts"), dict(acq="ucb"),
               dict(prune_rows=64)):
        with pytest.raises(ValueError, match="not with a gbt surrogate"):
            T.GpuDifferentialEvolution(surrogate="gbt", pool=256, **kw)
