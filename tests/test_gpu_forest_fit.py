"""ut_forest_fit (csrc/forest_fit.hip) against its numpy restatement
(tests/_rf_fit_oracle.py), record by record and bit for bit, at the smallest
shapes at which the kernels can go wrong (16 features per histogram block, 256
rows per partition step, 64 lanes); the fitted forest through both scoring
kernels; ut_forest_get; the refusals; the refitting technique.  Needs a GPU."""
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _rf_fit_oracle as RF  # noqa: E402

SEED = 11
_ENGINE = []


def _engine():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if not _ENGINE:
        from uptune_amd.engine import BatchEngine
        from uptune_amd.manipulator import ConfigurationManipulator, FloatParameter
        _ENGINE.append(BatchEngine(ConfigurationManipulator([FloatParameter("u", 0.0, 1.0)]), seed=SEED))
    return _ENGINE[0]


def _data(kind, n, d):
    rng = np.random.default_rng(n * 131 + d)
    X = rng.uniform(size=(n, d))
    if kind == "const_feature":
        X[:, 0] = 0.37
    elif kind == "twin":        # columns 1 and d - 1 are the same, and the ones that matter
        X[:, d - 1] = X[:, 1]
    elif kind == "edges":       # bin edges, both ends, outside the unit interval, NaN
        X = rng.choice([0.0, 1 / 256, 2 / 256, 127 / 256, 0.5, 254 / 256, 255 / 256, 1.0, -0.5, 1.5, np.nan,
                        np.nextafter(0.5, 0), 1e300], size=(n, d))
    elif kind == "onehot":
        X = (rng.uniform(size=(n, d)) < 0.3).astype(np.float64)
    elif kind == "repeat":      # 1,000 rows drawn from 40
        X = X[rng.integers(0, 40, size=n)]
    Xf = np.clip(np.nan_to_num(X, nan=0.3), -1.0, 2.0)
    y = 3.0 * Xf[:, min(1, d - 1)] + np.sin(5.0 * Xf[:, d // 2]) + 1e3
    if kind != "repeat":
        y = y + 0.1 * rng.normal(size=n)
    if kind == "const_y":
        y = np.full(n, 2.5)
    return X, y


CASES = {
    "n1": ("uniform", 1, 3, dict(n_trees=1, min_leaf=1)),
    "root_is_leaf": ("uniform", 5, 4, dict(n_trees=1, min_leaf=3, bootstrap=False)),
    "one_split": ("uniform", 6, 4, dict(n_trees=1, min_leaf=3, bootstrap=False)),
    "const_y": ("const_y", 40, 5, dict(n_trees=5)),
    "const_feature": ("const_feature", 65, 5, dict(n_trees=5, min_leaf=1)),
    "twin_columns": ("twin", 63, 6, dict(n_trees=5, bootstrap=False)),
    "edges": ("edges", 257, 3, dict(n_trees=5, min_leaf=1)),
    "d1": ("uniform", 63, 1, dict(n_trees=5, min_leaf=1)),
    "d17_frac": ("uniform", 65, 17, dict(n_trees=5, feature_frac=0.3)),
    "d33_frac": ("uniform", 257, 33, dict(n_trees=5, feature_frac=0.3, min_leaf=1)),
    "d63_depth3": ("uniform", 257, 63, dict(n_trees=5, max_depth=3)),
    "d65_depth1": ("uniform", 65, 65, dict(n_trees=5, max_depth=1)),
    "onehot_d200": ("onehot", 120, 200, dict(n_trees=5)),
    "n1000_repeats": ("repeat", 1000, 7, dict(n_trees=5)),
    "n1000_no_bootstrap": ("repeat", 1000, 7, dict(n_trees=1, bootstrap=False, min_leaf=1)),
}


@pytest.mark.parametrize("name", sorted(CASES))
def test_fit_equals_the_restatement(name):
    kind, n, d, kw = CASES[name]
    X, y = _data(kind, n, d)
    e = _engine()
    e.forest_fit(X, y, seed_round=3, **kw)
    roots, nodes = e.forest_get()
    want_roots, want = RF.fit(X, y, SEED, seed_round=3, **kw)
    print(name, "nodes", nodes.size, "want", want.size)
    np.testing.assert_array_equal(roots, want_roots)
    assert nodes.size == want.size
    for field in ("feature", "left", "right", "default_left"):
        np.testing.assert_array_equal(nodes[field], want[field], err_msg=field)
    for field in ("threshold", "value"):
        np.testing.assert_array_equal(nodes[field].view(np.int64), want[field].view(np.int64), err_msg=field)


@pytest.mark.parametrize("kernel", ["lane", "staged"])
def test_fitted_forest_interpolates_its_rows(kernel, monkeypatch):
    monkeypatch.setenv("UT_FOREST_STATS", kernel)
    X, y = _data("uniform", 200, 5)
    assert len({tuple(r) for r in RF.codes_of(X)}) == len(X)
    e = _engine()
    e.forest_fit(X, y, n_trees=2, min_leaf=1, bootstrap=False)
    mu, var, _ = e.forest_score(torch.from_numpy(np.ascontiguousarray(X.T)).cuda(), e.acq("ei"), 0.0)
    shift, scale = float(np.mean(y)), float(np.std(y))
    want = shift + scale * (RF.quantise(y, shift, scale).astype(np.float64) / 65536.0)
    np.testing.assert_array_equal(mu.cpu().numpy().view(np.int64), want.view(np.int64))
    assert (var.cpu().numpy() == 0.0).all()


def test_get_returns_what_was_set_and_refusals_keep_it():
    from sklearn.ensemble import RandomForestRegressor

    from uptune_amd import _lib as L
    from uptune_amd.forest import from_sklearn
    X, y = _data("uniform", 80, 4)
    f = from_sklearn(RandomForestRegressor(n_estimators=3, min_samples_leaf=3, random_state=0).fit(X, y),
                     leaf_var=True)
    e = _engine()
    e.forest_set(f)
    roots, nodes = e.forest_get()
    np.testing.assert_array_equal(roots, f.roots)
    inner = f.nodes["feature"] >= 0
    for field in ("feature", "left", "right", "default_left", "value"):
        np.testing.assert_array_equal(nodes[field], f.nodes[field])
    np.testing.assert_array_equal(nodes["threshold"][inner], f.nodes["threshold"][inner])
    np.testing.assert_array_equal(nodes["threshold"][~inner], f.leaf_var[~inner])
    feat = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()
    good = [t.cpu().numpy() for t in e.forest_score(feat, e.acq("ei"), 0.0)]
    bad_y = y.copy()
    bad_y[7] = np.inf
    for Xb, yb, kw in ((X, bad_y, {}), (X, y, dict(n_trees=0)), (X, y, dict(n_trees=257)), (X, y, dict(min_leaf=0)),
                       (X, y, dict(max_depth=81)), (X, y, dict(feature_frac=0.0)), (X, y, dict(seed_round=1 << 24)),
                       (np.zeros((80, 4097)), y, {})):
        with pytest.raises(L.UthotError, match="UT_EINVAL"):
            e.forest_fit(Xb, yb, **kw)
    par = L.ForestFitParams(4, 3, 0, 1, 1.0, 0.0, 0.0, 0)   # y_scale = 0
    import ctypes as C
    assert e.lib.ut_forest_fit(e.ctx, X.ctypes.data, y.ctypes.data, 80, 4, C.byref(par)) == -1
    assert e.lib.ut_forest_fit(e.ctx, None, y.ctypes.data, 80, 4, C.byref(par)) == -1
    assert e.lib.ut_debug_fail_alloc(e.ctx, 1) == 0
    with pytest.raises(L.UthotError, match="UT_ENOMEM"):
        e.forest_fit(X, y)
    assert e.lib.ut_debug_fail_alloc(e.ctx, 0) == 0
    roots2, nodes2 = e.forest_get()
    np.testing.assert_array_equal(roots2, roots)
    np.testing.assert_array_equal(nodes2, nodes)
    for a, b in zip(good, e.forest_score(feat, e.acq("ei"), 0.0)):
        np.testing.assert_array_equal(a.view(np.int64), b.cpu().numpy().view(np.int64))


def test_technique_refits_on_the_device_without_sklearn(monkeypatch):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    monkeypatch.setitem(sys.modules, "sklearn", None)
    from uptune_amd import technique as T
    from uptune_amd.driver import SearchDriver
    from uptune_amd.manipulator import ConfigurationManipulator, FloatParameter
    man = ConfigurationManipulator([FloatParameter("u%d" % k, 0.0, 1.0) for k in range(6)])
    de = T.GpuDifferentialEvolution(surrogate="forest", forest_fit="device", forest_kw={"n_estimators": 16},
                                    pool=4096, batch=4, seed=2)
    d = SearchDriver(man, de, parallelism=4)
    d.main(lambda c: float(sum((c["u%d" % k] - 0.7) ** 2 for k in range(6))), test_limit=40)
    model = d.root_technique.model
    assert len(d.results) >= 40 and model.fits > 1 and model.fit_seconds > 0
    roots, _ = model.engine.forest_get()
    assert roots.size == 16
    assert d.best_result.time < next(iter(d.results.values())).time
