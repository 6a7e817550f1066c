"""Tree-ensemble inference restated (TEST INFRASTRUCTURE: imported only by
tests/).  The traversal of scikit-learn's tree predict (sklearn/tree/_tree.pyx
`apply`: left iff X[i, feature] <= threshold with X converted to float32) and
the ensemble combinations of ForestRegressor.predict (sum in estimator order,
then / n_estimators) and GradientBoostingRegressor (init constant, then
raw += learning_rate * leaf per stage, predict_stages); XGBoost's documented
rule (left iff x < split_condition in float32, missing -> default_left,
base_score + sum of leaves).  Pinned by sklearn's own predict in
tests/test_forest.py; the XGBoost branch is pinned by a table worked by hand
from that rule (xgboost itself is not installed)."""
import numpy as np

LE, LT = 0, 1


def predict(nodes, roots, rule, base, scale, div, X):
    """nodes: structured array (uptune_amd.forest.NODE_DTYPE); X [m][F] f64"""
    feature, lchild, rchild = nodes["feature"].tolist(), nodes["left"].tolist(), nodes["right"].tolist()
    dleft, value = nodes["default_left"].tolist(), nodes["value"].tolist()
    with np.errstate(over="ignore"):
        # float32 -> float64 is exact and keeps order, so the float32 compares are made on doubles
        X32 = np.asarray(X, np.float64).astype(np.float32).astype(np.float64)
        if rule == LE:
            thr = nodes["threshold"].tolist()                  # sklearn: float32(x) <= the double threshold
        else:
            thr = nodes["threshold"].astype(np.float32).astype(np.float64).tolist()   # float32(x) < float32(thr)
    roots = [int(r) for r in roots]
    base, scale, div = float(base), float(scale), float(div)
    out = np.empty(X32.shape[0])
    for i, row in enumerate(X32.tolist()):
        acc = base
        for nd in roots:
            f = feature[nd]
            while f >= 0:
                x = row[f]
                if x != x:
                    left = dleft[nd] != 0
                elif rule == LE:
                    left = x <= thr[nd]
                else:
                    left = x < thr[nd]
                nd = lchild[nd] if left else rchild[nd]
                f = feature[nd]
            acc += scale * value[nd]
        out[i] = acc / div
    return out
