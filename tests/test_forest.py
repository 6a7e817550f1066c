"""Tree-ensemble surrogate: flattening of sklearn and
XGBoost-JSON models and the restated traversal, pinned by sklearn's predict
(CPU); the device kernel is checked in tests/test_gpu_forest.py."""
import json

import numpy as np
import pytest

from oracle import forest as of
from uptune_amd import forest as F


def _data(m=400, d=7, seed=0):
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(m, d))
    y = np.sin(6 * X[:, 0]) + X[:, 1] ** 2 - 0.5 * X[:, 2] * X[:, 3] + 0.05 * rng.standard_normal(m)
    return X, y


def _models():
    from sklearn.ensemble import ExtraTreesRegressor, GradientBoostingRegressor, RandomForestRegressor
    from sklearn.tree import DecisionTreeRegressor
    X, y = _data()
    return [DecisionTreeRegressor(max_depth=8, random_state=0).fit(X, y),
            RandomForestRegressor(n_estimators=25, max_depth=9, random_state=0).fit(X, y),
            ExtraTreesRegressor(n_estimators=20, random_state=1).fit(X, y),
            GradientBoostingRegressor(n_estimators=40, max_depth=4, learning_rate=0.07, random_state=0).fit(X, y)]


@pytest.mark.parametrize("k", range(4))
def test_flattened_sklearn_equals_predict(k):
    model = _models()[k]
    f = F.from_sklearn(model)
    Xq, _ = _data(300, 7, seed=5)
    Xq[:40] = np.round(Xq[:40], 2)     # values on (float32-rounded) thresholds
    got = of.predict(f.nodes, f.roots, f.rule, f.base, f.scale, f.div, Xq)
    np.testing.assert_array_equal(got, model.predict(Xq))


def test_xgboost_json_layout():
    # a hand-written 2-tree model in XGBoost's JSON schema (save_model format)
    tree0 = {"left_children": [1, -1, -1], "right_children": [2, -1, -1], "split_indices": [0, 0, 0],
             "split_conditions": [0.5, -1.0, 2.0], "default_left": [1, 0, 0]}
    tree1 = {"left_children": [1, 3, -1, -1, -1], "right_children": [2, 4, -1, -1, -1],
             "split_indices": [1, 2, 0, 0, 0], "split_conditions": [0.25, 0.75, 0.5, -0.125, 0.0625],
             "default_left": [0, 1, 0, 0, 0]}
    doc = {"learner": {"learner_model_param": {"base_score": "5E-1"},
                       "gradient_booster": {"model": {"trees": [tree0, tree1]}}}}
    f = F.from_xgboost_json(json.dumps(doc))
    X = np.array([[0.4, 0.1, 0.9], [0.6, 0.3, 0.0], [0.5, 0.25, 0.75], [np.nan, 0.1, 0.2]])
    got = of.predict(f.nodes, f.roots, f.rule, f.base, f.scale, f.div, X)
    # by hand: row0 -1.0 + (0.1<.25 -> node1: 0.9<.75? no -> node4 .0625); row1 2.0 + 0.5;
    # row2 (x0 == 0.5 is not < 0.5 -> right) 2.0 + (0.25 < 0.25? no -> 0.5); row3 NaN -> left -1.0 + node1 (0.2 < .75 -> -0.125)
    assert got.tolist() == [0.5 - 1.0 + 0.0625, 0.5 + 2.0 + 0.5, 0.5 + 2.0 + 0.5, 0.5 - 1.0 - 0.125]


# --------------------------------------------------------------------------- NaN routing of sklearn trees
@pytest.mark.parametrize("train_nan", [False, True], ids=["fit-clean", "fit-nan"])
@pytest.mark.parametrize("kind", ["tree", "forest", "extra"])
def test_flattened_sklearn_routes_nan_like_predict(kind, train_nan):
    """NaN queries follow tree_.missing_go_to_left (sklearn >= 1.3), not a fixed
    default_left = 1: the flattened model equals model.predict on rows with
    about 20 % NaN.  An estimator whose fit or predict rejects NaN in the
    installed sklearn is skipped (DecisionTreeRegressor before 1.3,
    RandomForestRegressor before 1.4, ExtraTreesRegressor before 1.6; none with
    1.7)."""
    from _forest_cases import nan_model, nan_queries, rejects_nan
    Xq = nan_queries()
    try:
        model = nan_model(kind, train_nan)
        want = model.predict(Xq)
    except ValueError as ex:
        if not rejects_nan(ex):
            raise
        pytest.skip("%s rejects NaN in this sklearn: %s" % (kind, str(ex)[:80]))
    f = F.from_sklearn(model)
    got = of.predict(f.nodes, f.roots, f.rule, f.base, f.scale, f.div, Xq)
    bad = int(np.sum(got != want))
    assert bad == 0, "%d of %d rows differ from %s.predict" % (bad, len(want), type(model).__name__)


# --------------------------------------------------------------------------- XGBoost's rule, by hand
def test_xgboost_lt_rule_hand_table():
    """The oracle's LT branch against a table worked by hand from XGBoost's
    documented rule: left iff float32(x) < float32(split_condition), missing ->
    default_left, prediction = base_score + sum of leaves.

        node0: x0 < 0.5   (missing -> right)
          node1 (left):  x1 < 0.0   (missing -> left)    leaves 1.0 | 2.0
          node2 (right): x1 < 0.1   (missing -> right)   leaves 4.0 | 8.0

    float32(0.1) = 0.100000001490116..., its float32 predecessor is
    0.099999994039535...; float32's predecessor of 0.5 is 0.49999997019767..."""
    tree = {"left_children": [1, 3, 5, -1, -1, -1, -1], "right_children": [2, 4, 6, -1, -1, -1, -1],
            "split_indices": [0, 1, 1, 0, 0, 0, 0], "split_conditions": [0.5, 0.0, 0.1, 1.0, 2.0, 4.0, 8.0],
            "default_left": [0, 1, 0, 0, 0, 0, 0]}
    doc = {"learner": {"learner_model_param": {"base_score": "2.5E-1"},
                       "gradient_booster": {"model": {"trees": [tree]}}}}
    f = F.from_xgboost_json(doc)
    nan, inf = float("nan"), float("inf")
    rows = [
        # x0, x1, leaf
        (0.5, 0.0, 4.0),                        # x0 == threshold: not <, right; 0.0 < 0.1f: left
        (0.49999999999999994, 0.0, 4.0),        # the double just below 0.5 rounds to 0.5f: right
        (0.5000000000000001, 0.0, 4.0),         # the double just above 0.5: right
        (0.4999999701976776, 0.0, 2.0),         # the float32 just below 0.5: left; 0.0 < 0.0 false: right
        (0.25, -0.0, 2.0),                      # -0.0 < 0.0 is false: right
        (-0.0, 0.0, 2.0),                       # -0.0 < 0.5: left; 0.0 < 0.0 false
        (0.25, -1.401298464324817e-45, 1.0),    # the largest negative float32 (a subnormal) < 0.0: left
        (0.25, -1e-50, 2.0),                    # a double that rounds to -0.0f: not < 0.0
        (nan, 0.0, 4.0),                        # missing at node0 (default right), then 0.0 < 0.1f
        (0.25, nan, 1.0),                       # missing at node1: default left
        (0.75, nan, 8.0),                       # missing at node2: default right
        (inf, 0.1, 8.0),                        # +inf right; float32(0.1) == float32(threshold): right
        (-inf, -inf, 1.0),                      # -inf left at both
        (0.25, inf, 2.0),
        (0.75, 0.10000000149011612, 8.0),       # float32(0.1) itself: equal, right
        (0.75, 0.09999999403953552, 4.0),       # the float32 just below float32(0.1): left
        (0.75, 0.09999999999, 8.0),             # < 0.1 as doubles, but rounds to float32(0.1): right
        (0.75, 0.1000000005, 8.0),              # between 0.1 and float32(0.1): rounds to float32(0.1), right
        (0.75, 0.0999999978, 8.0),              # just above the midpoint of those two float32: rounds up, right
        (0.75, 0.09999999776482582, 4.0),       # the midpoint itself: the tie goes to the even mantissa, the lower: left
        (0.75, 0.0999999977, 4.0),              # just below the midpoint: rounds down, left
    ]
    X = np.array([[r[0], r[1]] for r in rows])
    got = of.predict(f.nodes, f.roots, f.rule, f.base, f.scale, f.div, X)
    assert got.tolist() == [0.25 + r[2] for r in rows]
