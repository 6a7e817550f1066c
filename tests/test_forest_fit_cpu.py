"""The restatement of ut_forest_fit (tests/_rf_fit_oracle.py) held to exact
rational arithmetic at the root, and SharedModel's forest_fit= / forest_kw
validation.  No GPU."""
from fractions import Fraction

import numpy as np
import pytest

import _rf_fit_oracle as RF


def _exact_best(codes, q, min_leaf):
    """every (s, j, b) of the root with unit weights, s an exact Fraction"""
    out = []
    for j in range(codes.shape[1]):
        for b in range(255):
            left = codes[:, j] <= b
            wl, wr = int(left.sum()), int((~left).sum())
            if wl >= min_leaf and wr >= min_leaf:
                sl, sr = int(q[left].sum()), int(q[~left].sum())
                out.append((Fraction(sl * sl, wl) + Fraction(sr * sr, wr), j, b))
    return out


@pytest.mark.parametrize("n,d,min_leaf,seed", [(9, 3, 1, 0), (14, 2, 3, 1), (20, 4, 2, 2)])
def test_root_split_is_the_exact_maximum(n, d, min_leaf, seed):
    rng = np.random.default_rng(seed)
    X, y = rng.uniform(size=(n, d)), rng.normal(size=n)
    codes, q = RF.codes_of(X), RF.quantise(y, float(np.mean(y)), float(np.std(y)))
    cand = _exact_best(codes, q, min_leaf)
    top = max(c[0] for c in cand)
    # an empty bin repeats its left neighbour's gain: the maximum is unique up to that
    winners = [(j, b) for s, j, b in cand if s == top]
    assert len({j for j, _ in winners}) == 1 and len({tuple(codes[:, j] <= b) for j, b in winners}) == 1
    _, nodes = RF.fit(X, y, seed=5, n_trees=1, min_leaf=min_leaf, bootstrap=False)
    assert (int(nodes["feature"][0]), round(nodes["threshold"][0] * 256) - 1) == min(winners)
    assert nodes["left"][0] == 1 and nodes["right"][0] == 2 and nodes["default_left"][0] == 1


def test_shared_model_validates_the_device_fit():
    from uptune_amd import technique as T
    assert T.SharedModel(surrogate="forest").forest_fit == "host"
    m = T.SharedModel(surrogate="forest", forest_fit="device",
                      forest_kw=dict(n_estimators=8, min_samples_leaf=2, max_depth=None, bootstrap=False,
                                     max_features=0.5))
    assert m._device_forest_kw() == dict(n_trees=8, min_leaf=2, max_depth=0, bootstrap=False, feature_frac=0.5)
    with pytest.raises(ValueError, match="'host' or 'device'"):
        T.SharedModel(surrogate="forest", forest_fit="gpu")
    with pytest.raises(ValueError, match="belongs to surrogate='forest'"):
        T.SharedModel(forest_fit="device")
    with pytest.raises(ValueError, match="criterion"):
        T.SharedModel(surrogate="forest", forest_fit="device", forest_kw={"criterion": "absolute_error"})
    for bad in ("sqrt", 0.0, 1.5, True):
        with pytest.raises(ValueError, match="max_features"):
            T.SharedModel(surrogate="forest", forest_fit="device", forest_kw={"max_features": bad})
    # the host fit keeps taking any of sklearn's arguments, and the flag reaches a bandit's shared model
    assert T.SharedModel(surrogate="forest", forest_kw={"criterion": "absolute_error"}).forest_fit == "host"
    meta = T.pso_ga_de_bandit(surrogate="forest", forest_fit="device", pool=64, batch=2)
    assert {t.model.forest_fit for t in meta.techniques} == {"device"}
    assert T.GpuDifferentialEvolution(surrogate="forest", forest_fit="device").model.forest_fit == "device"
