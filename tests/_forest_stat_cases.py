"""Cases shared by tests/test_forest_stats_cpu.py and tests/test_gpu_forest_stats.py:
hand-built averaged LE forests (T = 1, 13, 70: T no multiple of the four
walking waves, T above one 32-tree chunk; a single-leaf tree and a depth-12
chain among them; 3, 64 and 700 feature columns, the last above any LDS staging
budget) queried around every threshold (NaN, +-inf, +-0, float32 subnormals),
and sklearn RandomForest (min_samples_leaf=3) / ExtraTrees models on targets as
they are and offset by 1e3.  m in {1, 63, 64, 4096 + 37}; the device tests add
ld > m and dup on every 7th candidate."""
import functools

import numpy as np

from _forest_cases import M_DEVICE, le_thresholds, values_around

OFFSET = 1.0e3


def avg_forest(n_trees, n_feat, seed):
    """an averaged LE forest: tree 3 a single leaf and tree 7 a left-leaning
    chain of depth 12 (where T has them), the rest complete trees of depth 1..5;
    leaves carry sklearn's -2 in the threshold field; leaf variances: a third
    exactly 0, the rest uniform in [0, 2)"""
    from uptune_amd import _lib as L
    from uptune_amd.forest import NODE_DTYPE, Forest
    rng = np.random.default_rng(seed)
    thr = le_thresholds()
    recs, roots = [], []

    def split(left, right):
        f = n_feat - 1 if rng.uniform() < 0.1 else int(rng.integers(0, n_feat))   # the last column is used
        return (f, left, right, int(rng.integers(0, 2)), thr[rng.integers(0, len(thr))], 0.0)

    def leaf():
        return (-1, 0, 0, 0, -2.0, float(rng.normal()))

    for t in range(n_trees):
        off = len(recs)
        roots.append(off)
        if t == 3:
            recs.append(leaf())
        elif t == 7:
            for k in range(12):        # node 2k splits: left -> the next split, right -> a leaf
                recs.append(split(off + 2 * k + 2, off + 2 * k + 1))
                recs.append(leaf())
            recs.append(leaf())
        else:
            depth = int(rng.integers(1, 6))
            per = 2 ** (depth + 1) - 1
            for k in range(per):
                recs.append(split(off + 2 * k + 1, off + 2 * k + 2) if 2 * k + 2 < per else leaf())
    nodes = np.array(recs, dtype=NODE_DTYPE)
    lv = np.where(rng.uniform(size=nodes.size) < 1 / 3, 0.0, rng.uniform(0.0, 2.0, size=nodes.size))
    lv[nodes["feature"] >= 0] = np.nan      # read at leaves only
    return Forest(nodes, np.array(roots, np.int32), L.UT_SPLIT_LE, 0.0, 1.0, float(n_trees), lv)


def _train(seed=0, n=300, d=6):
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(n, d))
    y = np.cos(5 * X[:, 0]) + X[:, 1] * X[:, 2] + 0.05 * rng.standard_normal(n)
    return X, y


@functools.lru_cache(maxsize=None)
def sk_model(kind, offset):
    from sklearn.ensemble import ExtraTreesRegressor, RandomForestRegressor
    X, y = _train()
    y = y + (OFFSET if offset else 0.0)
    if kind == "rf":
        return RandomForestRegressor(n_estimators=24, min_samples_leaf=3, random_state=0).fit(X, y)
    return ExtraTreesRegressor(n_estimators=24, min_samples_leaf=2, random_state=0).fit(X, y)


def sk_f_best(offset):
    return float(_train()[1].min() + (OFFSET if offset else 0.0))


# name -> (kind, args, m): the hand-built ones (T, n_feat, seed), the sklearn ones (model, offset)
CASES = {
    "le_T1_F3_m1": ("le", (1, 3, 1), 1),
    "le_T1_F3_m64": ("le", (1, 3, 2), 64),
    "le_T13_F64_m63": ("le", (13, 64, 3), 63),
    "le_T13_F700_m64": ("le", (13, 700, 4), 64),
    "le_T70_F3_mdev": ("le", (70, 3, 5), M_DEVICE),
    "le_T70_F64_mdev": ("le", (70, 64, 6), M_DEVICE),
    "le_T70_F700_m63": ("le", (70, 700, 7), 63),
    "rf_mdev": ("sk", ("rf", False), M_DEVICE),
    "rf_offset_mdev": ("sk", ("rf", True), M_DEVICE),
    "et_m64": ("sk", ("et", False), 64),
    "et_offset_m63": ("sk", ("et", True), 63),
}
OFFSET_CASES = ["rf_offset_mdev", "et_offset_m63"]
SELECT_CASE = "rf_mdev"


@functools.lru_cache(maxsize=None)
def case(name):
    """-> (Forest with leaf_var, queries X [m][F], f_best, the sklearn model or None)"""
    from uptune_amd.forest import from_sklearn
    kind, args, m = CASES[name]
    if kind == "le":
        T, F, seed = args
        f = avg_forest(T, F, seed)
        X = values_around(le_thresholds(), m * F, seed + 100).reshape(m, F)
        return f, X, 0.0, None
    model = sk_model(*args)
    X = np.random.default_rng(len(name)).uniform(size=(m, 6))
    X[: m // 4] = np.round(X[: m // 4], 2)
    return from_sklearn(model, leaf_var=True), X, sk_f_best(args[1]), model


@functools.lru_cache(maxsize=None)
def reference(name):
    """the oracle's stats of the case, computed once and shared (treat as read-only)"""
    import _forest_stat_oracle as O
    f, X, _, _ = case(name)
    return O.stats(f.nodes, f.roots, f.rule, f.div, X, leaf_var=f.leaf_var)
