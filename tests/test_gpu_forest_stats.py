"""ut_forest_score on the device (csrc/forest_score.hip) against the numpy
restatement (tests/_forest_stat_oracle.py) over tests/_forest_stat_cases.py,
with both kernels (UT_FOREST_STATS=lane / staged; 700 columns exceed the staged
kernel's LDS budget and take the one-lane kernel either way):

  mu bitwise ut_forest_predict's pred; |var - var_ext| <= tol_i for every
  candidate; var >= 0; score against oracle.gp.acquisition at the device's own
  mu and var within 1e-9 |s| + 1e-9 max |s| (the fp64 tier of
  test_gpu_batch_select.py) for EI (xi 0, 0.01) and UCB (kappa 2); -inf exactly
  on duplicates; the same bits from two calls and from both kernels; NULL
  outputs; the error paths; selection; the refitting technique.  Needs a GPU."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _forest_stat_cases as SC  # noqa: E402
import _forest_stat_oracle as O  # noqa: E402
from oracle import gp as ogp  # noqa: E402
from oracle import select as osel  # noqa: E402

LD = np.longdouble
ACQS = [("ei", 0.0, 2.0), ("ei", 0.01, 2.0), ("ucb", 0.0, 2.0)]
_ENGINES = {}


def _engine(d):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if d not in _ENGINES:
        from uptune_amd.engine import BatchEngine
        from uptune_amd.manipulator import ConfigurationManipulator, FloatParameter
        _ENGINES[d] = BatchEngine(ConfigurationManipulator([FloatParameter("u%d" % k, 0.0, 1.0) for k in range(d)]))
    return _ENGINES[d]


def _feat(X, pad=5):
    """X [m][F] -> a device view [F][m] of rows ld = m + pad apart"""
    m, F = X.shape
    big = torch.full((F, m + pad), float("nan"), dtype=torch.float64, device="cuda")
    big[:, :m] = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()
    return big[:, :m]


def _dup7(m):
    d = np.zeros(m, np.uint8)
    d[::7] = 1
    return d


def _bits(t):
    return t.cpu().numpy().view(np.int64)


@pytest.mark.parametrize("kernel", ["lane", "staged"])
@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_forest_score_matches_restatement(name, kernel, monkeypatch):
    monkeypatch.setenv("UT_FOREST_STATS", kernel)
    f, X, f_best, _ = SC.case(name)
    ref = SC.reference(name)
    m = X.shape[0]
    e = _engine(3)
    e.forest_set(f)
    feat = _feat(X)
    assert feat.stride(0) > m
    dup = _dup7(m)
    dup_d = torch.from_numpy(dup).cuda()
    pred, _ = e.forest_predict(feat)
    first = None
    for kind, xi, kappa in ACQS:
        acq = e.acq(kind, xi=xi, kappa=kappa)
        mu, var, score = e.forest_score(feat, acq, f_best, dup=dup_d)
        again = e.forest_score(feat, acq, f_best, dup=dup_d)
        for a, b in zip((mu, var, score), again):
            np.testing.assert_array_equal(_bits(a), _bits(b))
        np.testing.assert_array_equal(_bits(mu), _bits(pred))
        mu_h, var_h, s_h = mu.cpu().numpy(), var.cpu().numpy(), score.cpu().numpy()
        np.testing.assert_array_equal(mu_h.view(np.int64), ref["mu"].view(np.int64))
        err = np.abs(var_h.astype(LD) - ref["var_ext_ld"])
        print(name, kernel, kind, "max |var - var_ext| / tol", float(np.max(err / np.maximum(ref["tol"], 1e-300))))
        assert (var_h >= 0).all()
        assert (err <= ref["tol"]).all()
        want = ogp.acquisition(mu_h, var_h, f_best, kind=kind, xi=xi, kappa=kappa)
        live = dup == 0
        assert np.isneginf(s_h[~live]).all() and np.isfinite(s_h[live]).all()
        if live.any():
            bound = 1e-9 * np.abs(want[live]) + 1e-9 * np.max(np.abs(want[live]))
            assert (np.abs(s_h[live] - want[live]) <= bound).all()
        if first is None:
            first = (mu_h, var_h)
        else:   # mean and variance do not depend on the acquisition
            np.testing.assert_array_equal(first[0].view(np.int64), mu_h.view(np.int64))
            np.testing.assert_array_equal(first[1].view(np.int64), var_h.view(np.int64))
    # without dup no score is -inf
    _, _, s2 = e.forest_score(feat, e.acq("ei"), f_best)
    assert np.isfinite(s2.cpu().numpy()).all()


@pytest.mark.parametrize("name", ["le_T70_F64_mdev", "le_T13_F64_m63", "rf_offset_mdev"])
def test_both_kernels_give_the_same_bits(name, monkeypatch):
    f, X, f_best, _ = SC.case(name)
    e = _engine(3)
    e.forest_set(f)
    feat = _feat(X)
    out = {}
    for kernel in ("lane", "staged"):
        monkeypatch.setenv("UT_FOREST_STATS", kernel)
        out[kernel] = [_bits(t) for t in e.forest_score(feat, e.acq("ei", xi=0.01), f_best)]
    monkeypatch.delenv("UT_FOREST_STATS")
    out["default"] = [_bits(t) for t in e.forest_score(feat, e.acq("ei", xi=0.01), f_best)]
    for k in ("staged", "default"):
        for a, b in zip(out["lane"], out[k]):
            np.testing.assert_array_equal(a, b)


def test_null_outputs_and_m_zero():
    f, X, f_best, _ = SC.case("le_T13_F64_m63")
    e = _engine(3)
    e.forest_set(f)
    feat = _feat(X)
    m = X.shape[0]
    acq = e.acq("ei")
    full = e.forest_score(feat, acq, f_best)
    for keep in range(3):
        outs = [torch.full((m,), 7.0, dtype=torch.float64, device="cuda") if j == keep else None for j in range(3)]
        ptr = [None if t is None else C.c_void_p(t.data_ptr()) for t in outs]
        rc = e.lib.ut_forest_score(e.ctx, C.c_void_p(feat.data_ptr()), feat.stride(0), m, feat.shape[0], None,
                                   C.byref(acq), float(f_best), *ptr)
        assert rc == 0
        np.testing.assert_array_equal(_bits(outs[keep]), _bits(full[keep]))
    rc = e.lib.ut_forest_score(e.ctx, C.c_void_p(feat.data_ptr()), feat.stride(0), m, feat.shape[0], None,
                               C.byref(acq), float(f_best), None, None, None)
    assert rc == 0
    # m == 0: nothing is launched, nothing is written
    guard = torch.full((4,), 7.0, dtype=torch.float64, device="cuda")
    rc = e.lib.ut_forest_score(e.ctx, C.c_void_p(feat.data_ptr()), feat.stride(0), 0, feat.shape[0], None,
                               C.byref(acq), 0.0, C.c_void_p(guard.data_ptr()), None, None)
    assert rc == 0 and (guard.cpu().numpy() == 7.0).all()


def test_error_paths_leave_the_ensemble_usable():
    from sklearn.ensemble import GradientBoostingRegressor

    from uptune_amd import _lib as L
    from uptune_amd.engine import BatchEngine
    from uptune_amd.manipulator import ConfigurationManipulator, FloatParameter
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    f, X, f_best, _ = SC.case("le_T13_F64_m63")
    ref = SC.reference("le_T13_F64_m63")
    feat = _feat(X)
    m = X.shape[0]
    e = BatchEngine(ConfigurationManipulator([FloatParameter("u", 0.0, 1.0)]))
    try:
        with pytest.raises(L.UthotError, match="UT_EINVAL.*ut_forest_set first"):
            e.forest_score(feat, e.acq("ei"), 0.0)
        lv = np.zeros(5)
        assert e.lib.ut_forest_leaf_var(e.ctx, lv.ctypes.data, 5) == -1
        e.forest_set(f)
        good = [_bits(t) for t in e.forest_score(feat, e.acq("ei"), f_best)]

        def still_good():
            for a, b in zip(good, e.forest_score(feat, e.acq("ei"), f_best)):
                np.testing.assert_array_equal(a, _bits(b))

        # fewer feature columns than the ensemble splits on: both numbers named
        with pytest.raises(L.UthotError, match=r"UT_EINVAL.*splits on feature 63 but n_features is 10"):
            e.forest_score(feat[:10], e.acq("ei"), f_best)
        acq = e.acq("ei")
        args = lambda ld, mm, a: (e.ctx, C.c_void_p(feat.data_ptr()), ld, mm, feat.shape[0], None, a,  # noqa: E731
                                  float(f_best), None, None, None)
        assert e.lib.ut_forest_score(*args(m - 1, m, C.byref(acq))) == -1       # ld < m
        assert e.lib.ut_forest_score(*args(feat.stride(0), -1, C.byref(acq))) == -1
        assert e.lib.ut_forest_score(*args(feat.stride(0), m, None)) == -1      # acq NULL
        bad = L.Acq(kind=7, xi=0.0, kappa=2.0)
        assert e.lib.ut_forest_score(*args(feat.stride(0), m, C.byref(bad))) == -1
        assert e.lib.ut_forest_score(e.ctx, None, feat.stride(0), m, feat.shape[0], None, C.byref(acq), 0.0, None,
                                     None, None) == -1
        still_good()
        # leaf variances: wrong count, negative, NaN and inf at a leaf refuse and change nothing
        leaf0 = int(np.flatnonzero(f.nodes["feature"] < 0)[0])
        for n_nodes, value in ((f.nodes.size - 1, 0.5), (f.nodes.size, -1e-300), (f.nodes.size, np.nan),
                               (f.nodes.size, np.inf)):
            lv = np.nan_to_num(f.leaf_var, nan=0.0)
            lv[leaf0] = value
            assert e.lib.ut_forest_leaf_var(e.ctx, lv.ctypes.data, n_nodes) == -1
            still_good()
        assert e.lib.ut_forest_leaf_var(e.ctx, None, f.nodes.size) == -1
        still_good()
        # a boosted ensemble is refused, and an averaged one loaded afterwards scores as before
        rng = np.random.default_rng(0)
        Xt = rng.uniform(size=(80, 64))
        gb = GradientBoostingRegressor(n_estimators=5, max_depth=2, random_state=0).fit(Xt, Xt[:, 0] + Xt[:, 1])
        e.forest_set(gb)
        with pytest.raises(L.UthotError, match="UT_EUNSUPPORTED.*averaged ensemble"):
            e.forest_score(feat, e.acq("ei"), f_best)
        e.forest_predict(feat)   # the mean of the boosted ensemble is still served
        e.forest_set(f)
        still_good()
        # ut_forest_set clears the leaf variances: the same records without them give the spread of the means
        from uptune_amd.forest import Forest
        e.forest_set(Forest(f.nodes, f.roots, f.rule, f.base, f.scale, f.div))
        _, var0, _ = e.forest_score(feat, e.acq("ei"), f_best)
        ref0 = O.stats(f.nodes, f.roots, f.rule, f.div, X)
        v0 = var0.cpu().numpy()
        assert (np.abs(v0.astype(LD) - ref0["var_ext_ld"]) <= ref0["tol"]).all()
        assert (v0 < good[1].view(np.float64)).any() and (ref["var"] >= ref0["var"]).all()
    finally:
        e.close()


def test_selection_differs_from_the_mean_ranking():
    f, X, f_best, _ = SC.case(SC.SELECT_CASE)
    e = _engine(3)
    e.forest_set(f)
    feat = _feat(X)
    dup = _dup7(X.shape[0])
    dup_d = torch.from_numpy(dup).cuda()
    mu, var, score = e.forest_score(feat, e.acq("ei"), f_best, dup=dup_d)
    idx, _ = e.topk(score, 64, dup=dup_d)
    want = osel.topk(score.cpu().numpy().tolist(), 64, dup=dup.tolist())
    assert idx.cpu().numpy().tolist() == want
    by_mean = osel.topk((-mu.cpu().numpy()).tolist(), 64, dup=dup.tolist())
    overlap = len(set(want) & set(by_mean))
    print("EI top-64 and mean top-64 share", overlap)
    assert overlap < 64


def _sphere(c):
    return float(sum((c["u%d" % k] - 0.7) ** 2 for k in range(6)))


def _tune():
    from uptune_amd import technique as T
    from uptune_amd.driver import SearchDriver
    from uptune_amd.manipulator import ConfigurationManipulator, FloatParameter
    man = ConfigurationManipulator([FloatParameter("u%d" % k, 0.0, 1.0) for k in range(6)])
    de = T.GpuDifferentialEvolution(surrogate="forest", pool=4096, batch=4, seed=2)
    d = SearchDriver(man, de, parallelism=4)
    d.main(_sphere, test_limit=60)
    return d


def test_technique_refits_its_forest():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    d = _tune()
    model = d.root_technique.model
    first = next(iter(d.results.values()))
    assert len(d.results) >= 60 and model.fits > 1 and model.fit_seconds > 0
    assert model.engine.forest.n_trees == 64 and model.engine.forest.leaf_var is not None
    assert d.best_result.time < first.time
    d2 = _tune()
    assert [r.configuration.hash for r in d2.results_query()] == [r.configuration.hash for r in d.results_query()]
