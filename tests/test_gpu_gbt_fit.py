"""ut_gbt_fit (csrc/gbt_fit.hip) against its numpy restatement
(tests/_gbt_fit_oracle.py), record by record and bit for bit, at the smallest
shapes at which the kernels can go wrong (16 features per histogram block,
slices = clamp(ceil(256 / 2^L), 1, blocks) workgroups per node, 256 rows per
partition step, heap levels up to 1,024 wide), and the fitted ensemble through
ut_forest_predict; the refusals.  Needs a GPU."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _gbt_fit_oracle as GB  # noqa: E402
import _rf_fit_oracle as RF  # noqa: E402

SEED = 7
_ENGINE = []
ONES = dict(eta=1.0, reg_lambda=1.0, subsample=1.0, colsample_bylevel=1.0)
REF = dict(eta=0.015, reg_lambda=1.0, subsample=0.4, colsample_bylevel=0.5)


def _engine():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if not _ENGINE:
        from uptune_amd.engine import BatchEngine
        from uptune_amd.manipulator import ConfigurationManipulator, FloatParameter
        _ENGINE.append(BatchEngine(ConfigurationManipulator([FloatParameter("u", 0.0, 1.0)]), seed=SEED))
    return _ENGINE[0]


def _data(kind, n, d):
    rng = np.random.default_rng(n * 4099 + d)
    X = rng.random((n, d))
    y = np.sin(6.0 * X[:, 0]) + X[:, d // 2] * X[:, d - 1] + 0.05 * rng.standard_normal(n)
    if kind == "twin":       # columns 1 and 2 identical and the most informative, column 0 constant
        X[:, 0] = 0.5
        X[:, 2] = X[:, 1]
        y = np.cos(4.0 * X[:, 1]) + 0.01 * rng.standard_normal(n)
    elif kind == "const_y":
        y = np.full(n, 3.25)
    elif kind == "far":      # a step of height 2 with noise 0.001, and one target beyond 32 y_scale from y_shift
        y = np.where(X[:, 0] < 0.5, -1.0, 1.0) + 0.001 * rng.standard_normal(n)
        y[5] = 1000.0
    return X, y


# name -> (data, n, d, ut_gbt_fit's arguments): what can go wrong there
CASES = {
    "smallest": ("uniform", 50, 3, dict(n_rounds=3, max_depth=2, **ONES)),
    # padding columns, the sample and level draws, pred carried over rounds for unsampled rows
    "reference_params": ("uniform", 300, 17, dict(n_rounds=8, max_depth=6, **REF)),
    # three feature blocks: several slices per node, the ticket and the cross-workgroup read
    "three_blocks": ("uniform", 64, 40, dict(n_rounds=2, max_depth=3, **ONES)),
    # 66 blocks, 64 slices at level 2: blocks strided over the slices
    "strided_blocks": ("uniform", 64, 16 * 65 + 1, dict(n_rounds=2, max_depth=3, **ONES)),
    # levels up to 1,024 wide, mostly empty grids, heap indexing and the layout scan
    "deep": ("uniform", 2000, 4, dict(n_rounds=2, max_depth=10, min_child=1, **ONES)),
    # ties to the smaller j, then b
    "twin_columns": ("twin", 90, 4, dict(n_rounds=3, max_depth=3, **ONES)),
    # every tree one leaf of value 0
    "const_y": ("const_y", 40, 3, dict(n_rounds=3, max_depth=3, **ONES)),
    # the target's clamp; the gain test: round 0's gains are about 65536^2 n = 3e11, round 1 is left the
    # noise, gains of about (65536 * 0.001)^2 n = 3e5, and stops at its root
    "clamp_and_gamma": ("far", 80, 3, dict(n_rounds=2, max_depth=3, eta=1.0, reg_lambda=0.0, subsample=1.0,
                                           colsample_bylevel=1.0, gamma=1e8, y_shift=0.0, y_scale=1.0)),
    # children refused by count on both sides
    "min_child_7": ("uniform", 40, 3, dict(n_rounds=3, max_depth=4, min_child=7, **ONES)),
}


def _assert_records_equal(roots, nodes, want_roots, want):
    np.testing.assert_array_equal(roots, want_roots)
    assert nodes.size == want.size
    for field in ("feature", "left", "right", "default_left"):
        np.testing.assert_array_equal(nodes[field], want[field], err_msg=field)
    for field in ("threshold", "value"):
        np.testing.assert_array_equal(nodes[field].view(np.int64), want[field].view(np.int64), err_msg=field)


@pytest.mark.parametrize("name", sorted(CASES))
def test_fit_equals_the_restatement(name):
    kind, n, d, kw = CASES[name]
    X, y = _data(kind, n, d)
    e = _engine()
    e.gbt_fit(X, y, seed_round=3, **kw)
    roots, nodes = e.forest_get()
    want_roots, want, _ = GB.fit(X, y, SEED, seed_round=3, **kw)
    sizes = np.diff(np.r_[want_roots, want.size])
    print(name, "nodes", nodes.size, "want", want.size, "tree sizes", sizes.tolist())
    if name == "const_y":
        assert want.size == 3 and (want["value"] == 0.0).all()
    if name == "clamp_and_gamma":
        assert sizes[0] > 1 and sizes[1] == 1 and np.abs(y / 1.0).max() > 32.0
    if name == "deep":
        assert all(len(w) == 11 for w in RF.level_widths(want, want_roots))   # nodes in the 1,024-slot level
    _assert_records_equal(roots, nodes, want_roots, want)
    # 64 fresh rows: pred = y_shift + sum of the leaves' values in tree order, nothing fused
    fresh = np.random.default_rng(1).random((64, d))
    leaf = RF.route(nodes, roots, RF.codes_of(fresh))
    acc = np.full(64, kw.get("y_shift", float(np.mean(y))))
    for t in range(len(roots)):
        acc = acc + nodes["value"][leaf[:, t]]
    pred, _ = e.forest_predict(torch.from_numpy(np.ascontiguousarray(fresh.T)).cuda())
    np.testing.assert_array_equal(pred.cpu().numpy().view(np.int64), acc.view(np.int64))


def test_forest_and_boosted_fits_share_scratch_in_any_order():
    """The two fits stage through one function (csrc/tree_fit.h) into the same scratch: forest 120 x 5, boosted
    64 x 40, boosted 50 x 3, forest 120 x 5 again on one engine, d_pad and n shrinking and growing, so codes,
    candidates or row lists left by the fit before would show.  Every result equals its restatement."""
    e = _engine()
    Xf, yf = _data("uniform", 120, 5)
    want_forest = RF.fit(Xf, yf, SEED, n_trees=3)
    got_forest = []
    for name in (None, "three_blocks", "smallest", None):
        if name is None:
            e.forest_fit(Xf, yf, n_trees=3)
            want_roots, want = want_forest
        else:
            kind, n, d, kw = CASES[name]
            X, y = _data(kind, n, d)
            e.gbt_fit(X, y, seed_round=3, **kw)
            want_roots, want, _ = GB.fit(X, y, SEED, seed_round=3, **kw)
        roots, nodes = e.forest_get()
        _assert_records_equal(roots, nodes, want_roots, want)
        if name is None:
            got_forest.append((roots.tobytes(), nodes.tobytes()))
    assert got_forest[0] == got_forest[1]


def test_refusals_keep_the_loaded_ensemble_and_fits_repeat():
    from uptune_amd import _lib as L
    X, y = _data("uniform", 120, 5)
    e = _engine()
    e.forest_fit(X, y, n_trees=3)
    roots, nodes = e.forest_get()
    bad_y = y.copy()
    bad_y[7] = np.nan
    for Xb, yb, kw in ((X, bad_y, {}), (X, y, dict(n_rounds=0)), (X, y, dict(n_rounds=1025)), (X, y, dict(max_depth=0)),
                       (X, y, dict(max_depth=13)), (X, y, dict(min_child=0)), (X, y, dict(eta=0.0)),
                       (X, y, dict(eta=1.5)), (X, y, dict(reg_lambda=-1.0)), (X, y, dict(gamma=-1.0)),
                       (X, y, dict(subsample=0.0)), (X, y, dict(subsample=1.5)), (X, y, dict(colsample_bylevel=0.0)),
                       (X, y, dict(colsample_bylevel=np.nan)), (X, y, dict(y_scale=0.0)), (X, y, dict(y_shift=np.inf)),
                       (X, y, dict(seed_round=1 << 24)), (np.zeros((120, 4097)), y, {}),
                       (np.zeros((16385, 2)), np.arange(16385.0), {})):
        with pytest.raises(L.UthotError, match="UT_EINVAL"):
            e.gbt_fit(Xb, yb, **kw)
        roots2, nodes2 = e.forest_get()
        np.testing.assert_array_equal(roots2, roots)
        np.testing.assert_array_equal(nodes2, nodes)
    kw = dict(n_rounds=4, max_depth=3, subsample=0.5)
    e.gbt_fit(X, y, seed_round=1, **kw)
    a = e.forest_get()
    with pytest.raises(L.UthotError, match="UT_EUNSUPPORTED"):
        e.forest_score(torch.from_numpy(np.ascontiguousarray(X.T)).cuda(), e.acq("ei"), 0.0)
    e.gbt_fit(X, y, seed_round=1, **kw)
    b = e.forest_get()
    assert a[0].tobytes() == b[0].tobytes() and a[1].tobytes() == b[1].tobytes()
    e.gbt_fit(X, y, seed_round=2, **kw)
    assert e.forest_get()[1].tobytes() != a[1].tobytes()
