"""The forest kernel (csrc/forest.hip) on the rules and inputs that sklearn
models on clean data never give it: XGBoost's float32 `<` with NaN routed by
default_left, single-leaf and deep chain trees, thresholds that are float32
subnormals or no float32 value at all, a feature matrix whose row stride
exceeds m, sklearn trees queried with NaN; and what ut_forest_set /
ut_forest_predict refuse.  Every comparison is bit-exact against
oracle/forest.py (pinned on the CPU by tests/test_forest.py).  Needs a GPU."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _forest_cases as FC  # noqa: E402
from oracle import forest as of  # noqa: E402

M = FC.M_DEVICE
PAD = 59          # the feature tensor's rows are M + PAD long: ld > m


def _engine(d):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from uptune_amd.engine import BatchEngine
    from uptune_amd.manipulator import ConfigurationManipulator, FloatParameter
    return BatchEngine(ConfigurationManipulator([FloatParameter("u%d" % k, 0.0, 1.0) for k in range(d)]))


def _oracle(f, X):
    return of.predict(f.nodes, f.roots, f.rule, f.base, f.scale, f.div, X)


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def _strided(X, fill):
    """X [m][F] -> device tensor [F][m] that is a view of [F][m + PAD], the padding set to `fill`"""
    m, F = X.shape
    big = torch.full((F, m + PAD), fill, dtype=torch.float64, device="cuda")
    big[:, :m] = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()
    view = big[:, :m]
    assert view.stride(0) == m + PAD
    return view


def _check_against_oracle(e, f, X):
    """pred bit-equal to the oracle through a strided and a dense feature matrix;
    score = sign * pred; -inf exactly on the duplicates"""
    want = _oracle(f, X)
    assert not np.isnan(want).any()
    e.forest_set(f)
    m = X.shape[0]
    # the padding holds NaN (routed by default_left) in one call and a huge value in
    # the other: a kernel that read column i + 1 or row stride m would change its answers
    pred_nan, _ = e.forest_predict(_strided(X, float("nan")))
    pred_big, _ = e.forest_predict(_strided(X, 1e300))
    dense = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()
    pred_dense, score_min = e.forest_predict(dense)
    for got in (pred_nan, pred_big, pred_dense):
        np.testing.assert_array_equal(_bits(got.cpu().numpy()), _bits(want))
    np.testing.assert_array_equal(_bits(score_min.cpu().numpy()), _bits(-want))
    dup = torch.zeros(m, dtype=torch.uint8, device="cuda")
    dup[::5] = 1
    dup[m - 1] = 1
    pred_d, score_max = e.forest_predict(_strided(X, float("nan")), dup=dup, sign=1.0)
    want_score = np.where(dup.cpu().numpy() != 0, -np.inf, want)
    np.testing.assert_array_equal(_bits(pred_d.cpu().numpy()), _bits(want))
    np.testing.assert_array_equal(_bits(score_max.cpu().numpy()), _bits(want_score))
    return want


def test_xgboost_lt_rule_on_device():
    from uptune_amd import _lib as L
    from uptune_amd import forest as F
    e = _engine(5)
    f = F.from_xgboost_json(FC.xgb_doc())
    assert f.rule == L.UT_SPLIT_LT and f.n_trees == 40 and f.base == 0.375
    depth1 = [t for t in range(40) if f.nodes["feature"][f.roots[t]] < 0]
    assert depth1 == [3]                                     # the single-leaf tree
    thr = f.nodes["threshold"][f.nodes["feature"] >= 0]
    assert {0.0, 0.1, FC.SUBNORMAL, 3.0e38} <= set(thr.tolist())   # every special threshold is in use
    X = np.stack([FC.values_around(FC.THRESHOLDS, M, 100 + k) for k in range(5)], axis=1)
    want = _check_against_oracle(e, f, X)
    assert len(set(want.tolist())) > 1000                    # the rows do take different paths


def test_le_rule_double_thresholds_on_device():
    e = _engine(3)
    f = FC.le_forest()
    X = np.stack([FC.values_around(FC.le_thresholds(), M, 200 + k) for k in range(3)], axis=1)
    want = _check_against_oracle(e, f, X)
    assert len(set(want.tolist())) > 300


@pytest.mark.parametrize("train_nan", [False, True], ids=["fit-clean", "fit-nan"])
@pytest.mark.parametrize("kind", ["tree", "forest", "extra"])
def test_sklearn_nan_queries_on_device(kind, train_nan):
    """NaN follows tree_.missing_go_to_left on the device too; an estimator that
    rejects NaN in the installed sklearn is skipped (see tests/test_forest.py)"""
    from uptune_amd import forest as F
    e = _engine(4)
    Xq = FC.nan_queries(m=M, seed=6)
    try:
        model = FC.nan_model(kind, train_nan)
        want = model.predict(Xq)
    except ValueError as ex:
        if not FC.rejects_nan(ex):
            raise
        pytest.skip("%s rejects NaN in this sklearn: %s" % (kind, str(ex)[:80]))
    f = F.from_sklearn(model)
    e.forest_set(f)
    pred, _ = e.forest_predict(_strided(Xq, float("nan")))
    got = pred.cpu().numpy()
    np.testing.assert_array_equal(_bits(got), _bits(_oracle(f, Xq)))
    np.testing.assert_array_equal(_bits(got), _bits(want))


def _bad_forests(good):
    from uptune_amd.forest import Forest
    n = good.nodes.size

    def variant(**kw):
        d = dict(nodes=good.nodes.copy(), roots=good.roots.copy(), rule=good.rule, base=good.base,
                 scale=good.scale, div=good.div)
        d.update(kw)
        return Forest(**d)

    split = int(np.flatnonzero(good.nodes["feature"] >= 0)[-1])
    out = {}
    for name, root in (("root == n_nodes", n), ("root < 0", -1)):
        r = good.roots.copy()
        r[-1] = root
        out[name] = variant(roots=r)
    for name, field, val in (("left == n_nodes", "left", n), ("right < 0", "right", -1)):
        nd = good.nodes.copy()
        nd[field][split] = val
        out[name] = variant(nodes=nd)
    out["div == 0"] = variant(div=0.0)
    out["rule 2"] = variant(rule=2)
    out["rule -1"] = variant(rule=-1)
    out["zero trees"] = variant(roots=np.zeros(0, np.int32))
    return out


def test_forest_set_rejects_bad_ensembles_and_keeps_the_loaded_one():
    from uptune_amd import _lib as L
    e = _engine(3)
    f = FC.le_forest()
    X = np.stack([FC.values_around(FC.le_thresholds(), 300, 300 + k) for k in range(3)], axis=1)
    feat = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()
    e.forest_set(f)
    want = _bits(_oracle(f, X))
    np.testing.assert_array_equal(_bits(e.forest_predict(feat)[0].cpu().numpy()), want)
    for name, bad in _bad_forests(f).items():
        with pytest.raises(L.UthotError):
            e.forest_set(bad)
            pytest.fail("ut_forest_set accepted: " + name)
        assert e.forest is f
        np.testing.assert_array_equal(_bits(e.forest_predict(feat)[0].cpu().numpy()), want, err_msg=name)


def test_forest_predict_needs_every_feature_column_of_the_model():
    """a model that splits on feature 4 and a 4-column matrix: UT_EINVAL naming
    both numbers, not an answer read from column 3"""
    from uptune_amd import _lib as L
    from uptune_amd import forest as F
    e = _engine(6)
    f = F.from_xgboost_json(FC.xgb_doc())
    assert int(f.nodes["feature"].max()) == 4
    X = np.stack([FC.values_around(FC.THRESHOLDS, 300, 400 + k) for k in range(6)], axis=1)
    feat = torch.from_numpy(np.ascontiguousarray(X.T)).cuda()       # [6][300]
    e.forest_set(f)
    want = _bits(_oracle(f, X))
    for nf in (5, 6):       # exactly enough columns, and one to spare
        np.testing.assert_array_equal(_bits(e.forest_predict(feat[:nf])[0].cpu().numpy()), want)
    for nf in (4, 1):
        with pytest.raises(L.UthotError) as ei:
            e.forest_predict(feat[:nf])
        msg = str(ei.value)
        assert "feature 4" in msg and "n_features is %d" % nf in msg, msg
    # a model of fewer features afterwards lowers the requirement again
    g = FC.le_forest()
    e.forest_set(g)
    np.testing.assert_array_equal(_bits(e.forest_predict(feat[:3])[0].cpu().numpy()), _bits(_oracle(g, X[:, :3])))
    with pytest.raises(L.UthotError):
        e.forest_predict(feat[:2])
