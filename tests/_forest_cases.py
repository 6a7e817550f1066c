"""Models and query values shared by tests/test_forest.py (CPU) and
tests/test_gpu_forest_rules.py (device): sklearn trees queried with NaN, a
seeded synthetic XGBoost JSON model, a hand-built LE forest, and candidate
values that sit on, and one step to either side of, every split threshold."""
import functools

import numpy as np

M_DEVICE = 4096 + 37          # 17 workgroups of 256, the last one partly filled


# --------------------------------------------------------------------------- sklearn + NaN
def _nan_train(seed=0, m=400, d=4):
    rng = np.random.default_rng(seed)
    X = rng.uniform(size=(m, d))
    y = np.sin(5 * X[:, 0]) + X[:, 1] * X[:, 2] - X[:, 3] + 0.05 * rng.standard_normal(m)
    return X, y


@functools.lru_cache(maxsize=None)
def nan_model(kind, train_nan):
    """kind: tree / forest / extra; train_nan: 10 % of the training features are
    NaN too, so missing_go_to_left differs from split to split"""
    from sklearn.ensemble import ExtraTreesRegressor, RandomForestRegressor
    from sklearn.tree import DecisionTreeRegressor
    X, y = _nan_train()
    if train_nan:
        X = X.copy()
        X[np.random.default_rng(11).uniform(size=X.shape) < 0.10] = np.nan
    model = {"tree": lambda: DecisionTreeRegressor(max_depth=6, random_state=0),
             "forest": lambda: RandomForestRegressor(n_estimators=10, random_state=0),
             "extra": lambda: ExtraTreesRegressor(n_estimators=10, max_depth=8, random_state=0)}[kind]()
    return model.fit(X, y)


def rejects_nan(ex):
    """the ValueError is sklearn's refusal of NaN input (check_array: "Input X contains NaN";
    a tree without missing-value support: "... does not accept missing values ...")"""
    msg = str(ex)
    return "NaN" in msg or "missing values" in msg


def nan_queries(m=400, d=4, seed=5):
    rng = np.random.default_rng(seed)
    Xq = rng.uniform(size=(m, d))
    Xq[rng.uniform(size=Xq.shape) < 0.20] = np.nan
    return Xq


# --------------------------------------------------------------------------- thresholds and values around them
SUBNORMAL = 1e-40             # a float32 subnormal
THRESHOLDS = [k / 16 for k in range(-4, 21)] + [0.0, 0.1, SUBNORMAL, 3.0e38]


def values_around(thresholds, size, seed, nan_frac=0.15):
    """`size` values drawn from: the thresholds, their neighbours in double and
    in float32 (both ways), +-0.0, tiny values (float32 subnormals and one that
    rounds to zero), values beyond float32's range, +-inf and uniform noise;
    about nan_frac of them NaN."""
    rng = np.random.default_rng(seed)
    t = np.asarray(thresholds, np.float64)
    with np.errstate(over="ignore"):
        t32 = t.astype(np.float32)
        special = np.concatenate([
            t, np.nextafter(t, -np.inf), np.nextafter(t, np.inf),
            t32.astype(np.float64),
            np.nextafter(t32, np.float32(-np.inf)).astype(np.float64),
            np.nextafter(t32, np.float32(np.inf)).astype(np.float64),
            [0.0, -0.0, 1e-40, 2e-40, 1e-46, -1e-40, 1e39, -1e39, np.inf, -np.inf]])
    pick = special[rng.integers(0, special.size, size=size)]
    noise = rng.uniform(-0.5, 1.5, size=size)
    out = np.where(rng.uniform(size=size) < 0.7, pick, noise)
    out[rng.uniform(size=size) < nan_frac] = np.nan
    return out


# --------------------------------------------------------------------------- synthetic XGBoost JSON
def _xgb_tree(rng, n_feat, max_depth, shape="random"):
    """one tree in the save_model JSON layout (only the keys from_xgboost_json reads)"""
    lc, rc, si, sc, dl = [], [], [], [], []

    def node():
        for a in (lc, rc, si, dl):
            a.append(0)
        sc.append(0.0)
        return len(lc) - 1

    def leaf(k):
        lc[k] = rc[k] = -1
        sc[k] = float(rng.normal())          # leaves keep their weight in split_conditions

    def grow(k, depth):
        if shape == "leaf" or depth >= max_depth or (shape == "random" and depth > 0 and rng.uniform() < 0.2):
            return leaf(k)
        si[k] = int(rng.integers(0, n_feat))
        sc[k] = float(THRESHOLDS[rng.integers(0, len(THRESHOLDS))])
        dl[k] = int(rng.integers(0, 2))
        lc[k], rc[k] = node(), node()
        grow(lc[k], depth + 1)
        if shape == "chain":
            leaf(rc[k])
        else:
            grow(rc[k], depth + 1)

    grow(node(), 0)
    return {"left_children": lc, "right_children": rc, "split_indices": si, "split_conditions": sc,
            "default_left": dl}


def xgb_doc(seed=20, n_trees=40, n_feat=5):
    """40 trees over 5 features: random shapes up to depth 8, tree 3 a single
    leaf, tree 7 a left-leaning chain of depth 12; base_score 0.375"""
    rng = np.random.default_rng(seed)
    trees = []
    for t in range(n_trees):
        if t == 3:
            trees.append(_xgb_tree(rng, n_feat, 0, "leaf"))
        elif t == 7:
            trees.append(_xgb_tree(rng, n_feat, 12, "chain"))
        else:
            trees.append(_xgb_tree(rng, n_feat, int(rng.integers(1, 9))))
    return {"learner": {"learner_model_param": {"base_score": "3.75E-1"},
                        "gradient_booster": {"model": {"trees": trees}}}}


# --------------------------------------------------------------------------- hand-built LE forest
def le_thresholds():
    """double thresholds that are not float32 values: 0.1, 0.3, 1/3 and the
    midpoints of adjacent float32 values (x on either neighbour decides by the
    double compare, after x itself was rounded to float32)"""
    a = np.array([0.25, 0.5, 0.7, 1.0], np.float32)
    mids = (a.astype(np.float64) + np.nextafter(a, np.float32(np.inf)).astype(np.float64)) / 2
    return [0.1, 0.3, 1.0 / 3.0, 0.0, 0.75] + mids.tolist()


def le_forest(seed=4, n_trees=12, n_feat=3, depth=5):
    """complete trees of the given depth, rule LE, random default_left, averaged (div = T)"""
    from uptune_amd import _lib as L
    from uptune_amd.forest import NODE_DTYPE, Forest
    rng = np.random.default_rng(seed)
    thr = le_thresholds()
    per = 2 ** (depth + 1) - 1
    nodes = np.zeros(n_trees * per, dtype=NODE_DTYPE)
    roots = np.arange(n_trees, dtype=np.int32) * per
    for t in range(n_trees):
        for k in range(per):
            g = t * per + k
            if 2 * k + 2 < per:
                nodes[g] = (int(rng.integers(0, n_feat)), t * per + 2 * k + 1, t * per + 2 * k + 2,
                            int(rng.integers(0, 2)), thr[rng.integers(0, len(thr))], 0.0)
            else:
                nodes[g] = (-1, 0, 0, 0, 0.0, float(rng.normal()))
    return Forest(nodes, roots, L.UT_SPLIT_LE, 0.0, 1.0, float(n_trees))
