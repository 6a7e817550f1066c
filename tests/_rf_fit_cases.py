"""Edge shapes of ut_forest_fit shared by tests/test_forest_fit_cases_cpu.py and
tests/test_gpu_forest_fit.py (TEST INFRASTRUCTURE).  Every case names the path
of csrc/forest_fit.hip it is there for and carries a condition on the
restatement's own output (tests/_rf_fit_oracle.py) that proves the case reaches
it: the CPU test asserts the condition, the GPU test holds the device to the
same restatement, bit for bit.  Also the candidate values at which a fitted
forest's routing could leave "where its code went"."""
import functools

import numpy as np

import _rf_fit_oracle as RF

SEED = 11          # of the engines that fit these cases
SEED_ROUND = 3


def data(kind, n, d):
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


def _blocks(n, d):
    """columns 5 and 1030 identical and the ones that matter: feature blocks 0
    and 64, which the same workgroup of k_rf_hist visits one after the other"""
    rng = np.random.default_rng(23)   # the first seed at which both blocks_65 cases meet their conditions
    X = rng.uniform(size=(n, d))
    X[:, 1030] = X[:, 5]
    return X, 3.0 * X[:, 5] + np.sin(5.0 * X[:, 1029]) + 0.1 * rng.normal(size=n)


TIES = np.array([-9, -6, -3, -2, -1, 0, 1, 2, 5, 8, 65535, -65536])   # z * 65536 = k + 0.5, k even and odd


def _quant(n, d):
    rng = np.random.default_rng(n * 131 + d)
    X = rng.uniform(size=(n, d))
    y = 2.0 * X[:, 0] - X[:, 1] + 0.05 * rng.normal(size=n)
    fixed = np.concatenate([(2.0 * TIES + 1.0) / 131072.0, [40.0, -40.0, 32.0, -32.0, 0.0, 1e300, -1e300]])
    y[:fixed.size] = fixed
    return X, y


def _outlier(n, d):
    rng = np.random.default_rng(1)
    X, y = rng.uniform(size=(n, d)), rng.normal(size=n)
    y[n // 2] = 1e9
    return X, y


def _widest(ref):
    return [max(w) for w in RF.level_widths(ref["nodes"], ref["roots"])]


def _sizes(ref):
    return np.diff(np.append(ref["roots"], ref["nodes"].size))


def _split_features(ref):
    f = ref["nodes"]["feature"]
    return f[f >= 0]


def _c_single_leaves(ref):
    assert ref["nodes"].size == len(ref["roots"]) and (ref["nodes"]["feature"] == -1).all()


def _c_wide(ref):
    assert _widest(ref)[0] > 512          # k_rf_split: three chunks of 256 nodes


def _c_wide_bootstrap(ref):
    a, b = RF.level_widths(ref["nodes"], ref["roots"])
    assert max(a) > 256 and max(b) > 256 and a != b


def _c_blocks_65(ref):
    X = ref["X"]
    assert X.shape[1] == 1040 and np.array_equal(X[:, 5], X[:, 1030])
    assert ref["nodes"]["feature"][ref["roots"][0]] == 5


def _c_blocks_65_frac(ref):
    assert (_split_features(ref) >= 1024).any()


def _c_blocks_129(ref):
    f = _split_features(ref)
    assert sum(bool(((f >= lo) & (f < hi)).any()) for lo, hi in ((0, 1024), (1024, 2048), (2048, 2064))) >= 2


def _c_trees_256(ref):
    assert len(ref["roots"]) == 256 and len(set(_sizes(ref).tolist())) > 1


def _c_trees_65(ref):
    assert len(ref["roots"]) == 65


def _c_no_eligible(ref):
    sizes = _sizes(ref)
    # a root holds all n draws of the bootstrap: W = n >= 2 min_leaf, and its q differ
    assert len(ref["y"]) >= 2 * ref["kw"]["min_leaf"] and (sizes == 1).any() and (sizes > 3).any()
    single = ref["roots"][sizes == 1]
    assert (ref["nodes"]["threshold"][single] > 0.0).all()   # a leaf's variance: its q are not all equal


def _c_quant(ref):
    y = ref["y"]
    q = RF.quantise(y, 0.0, 1.0)
    assert (y > 32.0).any() and (y < -32.0).any() and (y == 32.0).any() and (y == -32.0).any()
    assert q.max() == 32 * 65536 and q.min() == -32 * 65536
    z = y * 65536.0                      # exact: a power of two
    tie = np.flatnonzero((np.abs(z) < 2.0 ** 21) & (z - np.floor(z) == 0.5))
    k = np.floor(z[tie]).astype(np.int64)
    assert tie.size >= 8 and (k % 2 == 0).any() and (k % 2 == 1).any()
    assert (q[tie] == np.where(k % 2 == 0, k, k + 1)).all()   # half to even


def _c_outlier(ref):
    y = ref["y"]
    shift, scale = float(np.mean(y)), float(np.std(y))
    assert ((y - shift) / scale).max() > 32.0 and RF.quantise(y, shift, scale).max() == 32 * 65536


def _c_max_depth_is_n(ref):
    assert ref["kw"]["max_depth"] == len(ref["y"])
    roots, nodes = RF.fit(ref["X"], ref["y"], SEED, seed_round=SEED_ROUND, **dict(ref["kw"], max_depth=0))
    assert np.array_equal(roots, ref["roots"]) and nodes.tobytes() == ref["nodes"].tobytes()
    assert nodes.size > 2 * len(roots)


# name -> (data builder, its arguments, fit arguments, condition)
CASES = {
    "wide_levels": (data, ("uniform", 3000, 3), dict(n_trees=1, min_leaf=1, bootstrap=False), _c_wide),
    "wide_levels_bootstrap": (data, ("uniform", 3000, 3), dict(n_trees=2, min_leaf=1), _c_wide_bootstrap),
    "blocks_65": (_blocks, (48, 1040), dict(n_trees=3, min_leaf=2), _c_blocks_65),
    "blocks_65_frac": (_blocks, (48, 1040), dict(n_trees=3, min_leaf=2, feature_frac=0.05), _c_blocks_65_frac),
    "blocks_129": (data, ("uniform", 32, 2064), dict(n_trees=2, min_leaf=2, feature_frac=0.5), _c_blocks_129),
    "trees_256": (data, ("uniform", 24, 3), dict(n_trees=256, min_leaf=2), _c_trees_256),
    "trees_65": (data, ("uniform", 40, 5), dict(n_trees=65, feature_frac=0.5), _c_trees_65),
    "no_eligible_feature": (data, ("uniform", 130, 2), dict(n_trees=8, min_leaf=1, feature_frac=0.5),
                            _c_no_eligible),
    "quant_ties_and_clamp": (_quant, (64, 2), dict(n_trees=3, y_shift=0.0, y_scale=1.0), _c_quant),
    "outlier_default_scale": (_outlier, (1100, 2), dict(n_trees=2), _c_outlier),
    "min_leaf_above_n": (data, ("uniform", 5, 2), dict(n_trees=2, min_leaf=9), _c_single_leaves),
    "max_depth_is_n": (data, ("uniform", 33, 2), dict(n_trees=2, min_leaf=1, max_depth=33), _c_max_depth_is_n),
    "n_16384": (data, ("uniform", 16384, 2), dict(n_trees=1, min_leaf=3), _c_wide),
}


@functools.lru_cache(maxsize=None)
def reference(name):
    """the case's data, fit arguments and the restatement's records: computed once, shared, not to be written"""
    build, args, kw, _ = CASES[name]
    X, y = build(*args)
    node_rows = []
    roots, nodes = RF.fit(X, y, SEED, seed_round=SEED_ROUND, node_rows=node_rows, **kw)
    return {"X": X, "y": y, "kw": kw, "roots": roots, "nodes": nodes, "node_rows": node_rows}


def check(name):
    CASES[name][3](reference(name))


def shape_of(roots, nodes):
    """(widest level, node count, largest split feature) of fitted records"""
    return max(max(w) for w in RF.level_widths(nodes, roots)), int(nodes.size), int(nodes["feature"].max())


# ---- where a fitted forest could misroute ---------------------------------------
SPECIALS = [np.nan, -0.0, -0.5, -1e-300, 5e-324, 1.0, 1.0 + 2.0 ** -52, 1.5, 1e300, np.inf, -np.inf]


def edge_values():
    """every bin edge k / 256 and its two neighbours, in double and in float32
    widened to double, and the values outside [0, 1]"""
    e = np.arange(257) / 256.0
    e32 = e.astype(np.float32)
    f32 = np.concatenate([e32, np.nextafter(e32, np.float32(0)), np.nextafter(e32, np.float32(1))])
    return np.concatenate([e, np.nextafter(e, 0.0), np.nextafter(e, 1.0), f32.astype(np.float64), SPECIALS])


def candidates(d, m=2000):
    """[m][d]: every column holds every edge value at least once, in its own order"""
    pool = edge_values()
    rng = np.random.default_rng(d)
    C = np.stack([np.concatenate([rng.permutation(pool), rng.choice(pool, m - pool.size)]) for _ in range(d)],
                 axis=1)
    # the values a scoring kernel comparing in double would send left of their
    # code: doubles below the edge k / 256 whose float32 is the edge
    codes = RF.codes_of(C)
    k = np.arange(1, 256)
    below = np.nextafter(k / 256.0, 0.0)
    assert (below < k / 256.0).all() and (RF.codes_of(below) == k).all()
    assert all(np.isin(below, C[:, j]).all() for j in range(d))
    assert sum(np.isnan(v) for v in C[:, 0]) >= 1 and codes.min() == 0 and codes.max() == 255
    return C
