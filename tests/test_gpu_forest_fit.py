"""ut_forest_fit (csrc/forest_fit.hip) against its numpy restatement
(tests/_rf_fit_oracle.py), record by record and bit for bit, at the smallest
shapes at which the kernels can go wrong (16 features per histogram block, 256
rows per partition step, 64 lanes) and over the edge shapes of
tests/_rf_fit_cases.py (levels of more than 256 nodes, more than 64 feature
blocks, 65 and 256 trees, clamped and tied targets, the limits of n, min_leaf
and max_depth); a fit after other fits in the same context; the fitted forest
through ut_forest_predict and both ut_forest_score kernels at every bin edge
and outside [0, 1], held to routing by integer codes; ut_forest_get; the
refusals; the refitting technique.  Needs a GPU."""
import ctypes as C
import sys

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _forest_stat_oracle as FS  # noqa: E402
import _rf_fit_cases as RC  # noqa: E402
import _rf_fit_oracle as RF  # noqa: E402
from oracle import gp as ogp  # noqa: E402

SEED = RC.SEED
_ENGINE = []


def _engine():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if not _ENGINE:
        from uptune_amd.engine import BatchEngine
        from uptune_amd.manipulator import ConfigurationManipulator, FloatParameter
        _ENGINE.append(BatchEngine(ConfigurationManipulator([FloatParameter("u", 0.0, 1.0)]), seed=SEED))
    return _ENGINE[0]


_data = RC.data


def _fit(e, X, y, y_shift=None, y_scale=None, **kw):
    """engine.forest_fit, or ut_forest_fit itself where a case sets the target's shift and scale"""
    if y_shift is None:
        return e.forest_fit(X, y, seed_round=RC.SEED_ROUND, **kw)
    from uptune_amd import _lib as L
    X, y = np.ascontiguousarray(X, dtype=np.float64), np.ascontiguousarray(y, dtype=np.float64)
    par = L.ForestFitParams(kw.get("n_trees", 64), kw.get("min_leaf", 3), kw.get("max_depth", 0),
                            int(kw.get("bootstrap", True)), kw.get("feature_frac", 1.0), y_shift, y_scale,
                            RC.SEED_ROUND)
    L.check(e.ctx, e.lib.ut_forest_fit(e.ctx, X.ctypes.data, y.ctypes.data, X.shape[0], X.shape[1], C.byref(par)),
            "ut_forest_fit")


def _assert_records_equal(roots, nodes, want_roots, want):
    np.testing.assert_array_equal(roots, want_roots)
    assert nodes.size == want.size
    for field in ("feature", "left", "right", "default_left"):
        np.testing.assert_array_equal(nodes[field], want[field], err_msg=field)
    for field in ("threshold", "value"):
        np.testing.assert_array_equal(nodes[field].view(np.int64), want[field].view(np.int64), err_msg=field)


def _fit_case(e, name):
    """fit a case of the shared table -> (roots, nodes) of the device"""
    ref = RC.reference(name)
    _fit(e, ref["X"], ref["y"], **ref["kw"])
    return e.forest_get()


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
    _assert_records_equal(roots, nodes, want_roots, want)


@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_fit_equals_the_restatement_at_edge_shapes(name):
    """levels wider than k_rf_split's 256-node chunk, more than 64 feature blocks
    (strided over a workgroup), 65 and 256 trees, the target's clamp and rounding
    ties, a node without an eligible feature, the limits of n, min_leaf and
    max_depth: tests/test_forest_fit_cases_cpu.py proves each case reaches its path"""
    ref = RC.reference(name)
    roots, nodes = _fit_case(_engine(), name)
    print(name, "widest level, nodes, largest split feature: device", RC.shape_of(roots, nodes), "restatement",
          RC.shape_of(ref["roots"], ref["nodes"]))
    _assert_records_equal(roots, nodes, ref["roots"], ref["nodes"])


def test_a_fit_does_not_depend_on_the_fits_before_it():
    """every buffer of a context is kept and reused: a small fit after a large
    one, a wide one after a narrow one, and the same fit twice"""
    e = _engine()
    first = _fit_case(e, "wide_levels")
    kind, n, d, kw = CASES["one_split"]
    X, y = _data(kind, n, d)
    _fit(e, X, y, **kw)
    _assert_records_equal(*e.forest_get(), *RF.fit(X, y, SEED, seed_round=RC.SEED_ROUND, **kw))
    for name in ("blocks_65", "wide_levels"):
        ref = RC.reference(name)
        roots, nodes = _fit_case(e, name)
        _assert_records_equal(roots, nodes, ref["roots"], ref["nodes"])
    np.testing.assert_array_equal(roots, first[0])
    assert nodes.tobytes() == first[1].tobytes()
    a = _fit_case(e, "wide_levels_bootstrap")
    b = _fit_case(e, "wide_levels_bootstrap")
    np.testing.assert_array_equal(a[0], b[0])
    assert a[1].tobytes() == b[1].tobytes()


def _feat(X):
    return torch.from_numpy(np.ascontiguousarray(X.T)).cuda()


def _scored(e, feat, f_best, monkeypatch):
    """-> {path: (mu, var or None, score or None)} of ut_forest_predict and both ut_forest_score kernels"""
    out = {"predict": (e.forest_predict(feat)[0].cpu().numpy(), None, None)}
    for kernel in ("lane", "staged"):
        monkeypatch.setenv("UT_FOREST_STATS", kernel)
        out[kernel] = tuple(t.cpu().numpy() for t in e.forest_score(feat, e.acq("ei"), f_best))
    return out


ROUTED_FITS = {
    "edges_T5": ("edges", 257, 3, dict(n_trees=5, min_leaf=1)),
    "d17_T8": ("uniform", 129, 17, dict(n_trees=8, min_leaf=1, feature_frac=0.5)),   # two feature blocks
}


@pytest.mark.parametrize("name", sorted(ROUTED_FITS))
def test_fitted_forest_routes_every_value_where_its_code_went(name, monkeypatch):
    """uthot.h: a split "code <= b", stored as threshold (b + 1) / 256 under LT
    with default_left = 1, sends every x where its code went.  Candidates at,
    just below and just above every bin edge in double and in float32, NaN, -0.0,
    negatives, values above 1, 1e300, both infinities, denormals: pred and mu
    bit for bit the mean over the leaves that RF.route reaches by integer
    comparison of the codes, through ut_forest_predict and both ut_forest_score
    kernels; var and EI as tests/test_gpu_forest_stats.py holds them (its
    oracle and its bounds, on leaves asserted equal to RF.route's)."""
    kind, n, d, kw = ROUTED_FITS[name]
    X, y = _data(kind, n, d)
    e = _engine()
    _fit(e, X, y, **kw)
    roots, nodes = e.forest_get()
    _assert_records_equal(roots, nodes, *RF.fit(X, y, SEED, seed_round=RC.SEED_ROUND, **kw))
    assert (nodes["feature"] >= 0).sum() >= 8 * len(roots)
    cand = RC.candidates(d)
    codes = RF.codes_of(cand)
    want_mu = RF.predict(nodes, roots, codes)
    ref = FS.stats(nodes, roots, 1, float(len(roots)), cand, leaf_var=nodes["threshold"])
    np.testing.assert_array_equal(ref["leaf"], RF.route(nodes, roots, codes))
    np.testing.assert_array_equal(ref["mu"].view(np.int64), want_mu.view(np.int64))
    f_best = float(np.median(y))
    for path, (mu, var, score) in _scored(e, _feat(cand), f_best, monkeypatch).items():
        np.testing.assert_array_equal(mu.view(np.int64), want_mu.view(np.int64), err_msg=path)
        if var is None:
            continue
        err = np.abs(var.astype(np.longdouble) - ref["var_ext_ld"])
        print(name, path, "max |var - var_ext| / tol", float(np.max(err / np.maximum(ref["tol"], 1e-300))))
        assert (var >= 0).all() and (err <= ref["tol"]).all(), path
        want = ogp.acquisition(mu, var, f_best, kind="ei", xi=0.0, kappa=2.0)
        assert (np.abs(score - want) <= 1e-9 * np.abs(want) + 1e-9 * np.max(np.abs(want))).all(), path


def test_training_rows_reach_the_leaves_that_held_them(monkeypatch):
    """the edge-valued training rows (bin edges, NaN, 1e300, -0.5, 1.5) scored
    through the device.  The device returns means, not leaves, so: RF.route
    sends every in-bag row of every tree to a leaf whose rows at fit time
    contained it, and the device's mu is bit for bit the mean over those leaves;
    with one tree and no bootstrap, mu is the value of the very leaf that held
    the row."""
    X, y = _data("edges", 257, 3)
    e = _engine()
    for kw in (dict(n_trees=5, min_leaf=1), dict(n_trees=1, min_leaf=1, bootstrap=False)):
        node_rows = []
        want_roots, want = RF.fit(X, y, SEED, seed_round=RC.SEED_ROUND, node_rows=node_rows, **kw)
        _fit(e, X, y, **kw)
        roots, nodes = e.forest_get()
        _assert_records_equal(roots, nodes, want_roots, want)
        leaf = RF.route(nodes, roots, RF.codes_of(X))
        for t, r in enumerate(roots):
            assert all(i in node_rows[leaf[i, t]] for i in node_rows[r])
        if len(roots) == 1:
            assert sorted(node_rows[0].tolist()) == list(range(len(X)))
            want_mu = nodes["value"][leaf[:, 0]]
        else:
            want_mu = RF.predict(nodes, roots, RF.codes_of(X))
        for path, (mu, _, _) in _scored(e, _feat(X), float(np.min(y)), monkeypatch).items():
            np.testing.assert_array_equal(mu.view(np.int64), want_mu.view(np.int64), err_msg=path)


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

    def kept():
        roots2, nodes2 = e.forest_get()
        np.testing.assert_array_equal(roots2, roots)
        np.testing.assert_array_equal(nodes2, nodes)

    # n = 16385 is one past the documented top; max_depth = n + 1 at n = 80 and at n = 5
    for Xb, yb, kw in ((X, bad_y, {}), (X, y, dict(n_trees=0)), (X, y, dict(n_trees=257)), (X, y, dict(min_leaf=0)),
                       (X, y, dict(max_depth=81)), (X, y, dict(feature_frac=0.0)), (X, y, dict(seed_round=1 << 24)),
                       (np.zeros((80, 4097)), y, {}), (np.zeros((16385, 2)), np.arange(16385.0), {}),
                       (X[:5], y[:5], dict(max_depth=6))):
        with pytest.raises(L.UthotError, match="UT_EINVAL"):
            e.forest_fit(Xb, yb, **kw)
        kept()
    par = L.ForestFitParams(4, 3, 0, 1, 1.0, 0.0, 0.0, 0)   # y_scale = 0
    assert e.lib.ut_forest_fit(e.ctx, X.ctypes.data, y.ctypes.data, 80, 4, C.byref(par)) == -1
    assert e.lib.ut_forest_fit(e.ctx, None, y.ctypes.data, 80, 4, C.byref(par)) == -1
    # bootstrap = 2, y_shift = nan, y_scale = inf: each the only field out of range
    for par in (L.ForestFitParams(4, 3, 0, 2, 1.0, 0.0, 1.0, 0), L.ForestFitParams(4, 3, 0, 1, 1.0, np.nan, 1.0, 0),
                L.ForestFitParams(4, 3, 0, 1, 1.0, 0.0, np.inf, 0)):
        assert e.lib.ut_forest_fit(e.ctx, X.ctypes.data, y.ctypes.data, 80, 4, C.byref(par)) == -1
        kept()
    assert e.lib.ut_debug_fail_alloc(e.ctx, 1) == 0
    with pytest.raises(L.UthotError, match="UT_ENOMEM"):
        e.forest_fit(X, y)
    assert e.lib.ut_debug_fail_alloc(e.ctx, 0) == 0
    kept()
    for a, b in zip(good, e.forest_score(feat, e.acq("ei"), 0.0)):
        np.testing.assert_array_equal(a.view(np.int64), b.cpu().numpy().view(np.int64))
    par = L.ForestFitParams(4, 3, 0, 1, 1.0, 0.0, 1.0, 0)   # with every field in range the same call fits
    assert e.lib.ut_forest_fit(e.ctx, X.ctypes.data, y.ctypes.data, 80, 4, C.byref(par)) == 0
    assert e.forest_get()[0].size == 4


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
