"""ut_forest_fit restated in numpy and Python integers (include/uthot.h states the
definition): 256-bin codes, 16.16 fixed-point targets, Philox bootstrap and
feature draws, breadth-first growth, the split of largest
s = S_L^2 / W_L + S_R^2 / W_R with ties to the smaller feature, then bin.  Every
histogram entry is an integer below 2^53, so np.bincount's float64 sums are exact.

level_widths, route and predict read a fitted forest's records alone: where a
row of codes goes by integer comparison (no float is compared with a
threshold), and the mean uthot.h states for ut_forest_predict's pred."""
import numpy as np

from oracle.philox import draw, umulhi32
from uptune_amd.forest import NODE_DTYPE

OP_RF = 8


def codes_of(X):
    with np.errstate(invalid="ignore", over="ignore"):
        c = np.floor(np.asarray(X, np.float64).astype(np.float32) * np.float32(256))
        return np.where(c > 0, np.minimum(c, 255), 0).astype(np.int64)   # NaN -> 0


def quantise(y, shift, scale):
    return np.rint(np.clip((np.asarray(y, np.float64) - shift) / scale, -32.0, 32.0) * 65536.0).astype(np.int64)


def weights(seed, t, n, round_, bootstrap):
    if not bootstrap:
        return np.ones(n, np.int64)
    words = np.stack(draw(seed, np.arange((n + 3) // 4), t, round_, OP_RF), axis=1).reshape(-1)[:n]
    return np.bincount(umulhi32(words, n).astype(np.int64), minlength=n).astype(np.int64)


def eligible(seed, t, k, d, round_, frac):
    if frac >= 1.0:
        return np.ones(d, bool)
    j = np.arange(d, dtype=np.uint64)
    w = np.stack(draw(seed, (np.uint64(k) << np.uint64(32)) | (j >> np.uint64(2)), 0x10000 | t, round_, OP_RF), axis=1)
    return w[np.arange(d), (j & np.uint64(3)).astype(np.int64)].astype(np.float64) * 2.0 ** -32 < frac


def best_split(codes, w, q, rows, elig, min_leaf):
    """-> (j, b) of the largest s among the valid splits of the node, or None"""
    d = codes.shape[1]
    wv, wq = w[rows], w[rows] * q[rows]
    flat = (codes[rows] + 256 * np.arange(d)).ravel()
    WL = np.cumsum(np.bincount(flat, np.repeat(wv, d), 256 * d).reshape(d, 256), axis=1)[:, :255]
    SL = np.cumsum(np.bincount(flat, np.repeat(wq, d), 256 * d).reshape(d, 256), axis=1)[:, :255]
    WR, SR = float(wv.sum()) - WL, float(wq.sum()) - SL
    valid = (WL >= min_leaf) & (WR >= min_leaf) & elig[:, None]
    if not valid.any():
        return None
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(valid, (SL * SL) / WL + (SR * SR) / WR, -1.0)
    return divmod(int(np.argmax(s)), 255)   # the first maximum: smaller j, then smaller b


def grow(codes, q, w, t, seed, round_, min_leaf, max_depth, frac, shift, scale, node_rows=None):
    """one tree's records, child indices within the tree; node_rows, a list,
    receives every node's rows (those of weight > 0 that reached it)"""
    d = codes.shape[1]
    out, todo = [], [(np.flatnonzero(w > 0), 0)]   # node k is todo[k]: breadth first
    k = 0
    while k < len(todo):
        rows, depth = todo[k]
        W, Q1 = int(w[rows].sum()), int((w[rows] * q[rows]).sum())
        Q2 = int((w[rows] * q[rows] * q[rows]).sum())
        m = float(Q1) / float(W)
        value = shift + scale * (m / 65536.0)
        split = None
        if W >= 2 * min_leaf and depth != (max_depth or -1) and q[rows].min() != q[rows].max():
            split = best_split(codes, w, q, rows, eligible(seed, t, k, d, round_, frac), min_leaf)
        if split is None:
            v = float(Q2) / float(W) - m * m
            out.append((-1, -1, -1, 0, (scale * scale) * ((v if v > 0.0 else 0.0) / 4294967296.0), value))
        else:
            j, b = split
            left = codes[rows, j] <= b
            out.append((j, len(todo), len(todo) + 1, 1, (b + 1) / 256.0, value))
            todo += [(rows[left], depth + 1), (rows[~left], depth + 1)]
        k += 1
    if node_rows is not None:
        node_rows.extend(rows for rows, _ in todo)
    return np.array(out, dtype=NODE_DTYPE)


def fit(X, y, seed, n_trees=64, min_leaf=3, max_depth=0, bootstrap=True, feature_frac=1.0, seed_round=0,
        y_shift=None, y_scale=None, node_rows=None):
    """-> (roots [T] int32, nodes [N] NODE_DTYPE) as ut_forest_get returns them;
    y_shift / y_scale default to engine.forest_fit's: mean and std, 1 for a constant y;
    node_rows, a list, receives the rows of node k of the returned array at [k]"""
    y = np.asarray(y, np.float64)
    shift = float(np.mean(y)) if y_shift is None else y_shift
    scale = (float(np.std(y)) or 1.0) if y_scale is None else y_scale
    codes, q = codes_of(X), quantise(y, shift, scale)
    trees = [grow(codes, q, weights(seed, t, len(y), seed_round, bootstrap), t, seed, seed_round, min_leaf, max_depth,
                  feature_frac, shift, scale, node_rows) for t in range(n_trees)]
    roots = np.cumsum([0] + [len(a) for a in trees[:-1]]).astype(np.int32)
    for a, r in zip(trees, roots):
        inner = a["feature"] >= 0
        a["left"][inner] += r
        a["right"][inner] += r
    return roots, np.concatenate(trees)


def level_widths(nodes, roots):
    """-> per tree, the number of nodes at depth 0, 1, ..: from the records alone"""
    out = []
    for r in roots:
        level, widths = np.array([int(r)]), []
        while level.size:
            widths.append(int(level.size))
            inner = level[nodes["feature"][level] >= 0]
            level = np.concatenate([nodes["left"][inner], nodes["right"][inner]])
        out.append(widths)
    return out


def route(nodes, roots, codes):
    """-> leaf node index [m][T] of integer codes [m][d]: at a split record go
    left iff codes[i, feature] <= round(threshold * 256) - 1.  Where its code
    went: integers only, no x is compared with a threshold"""
    codes = np.asarray(codes, np.int64)
    inner = nodes["feature"] >= 0
    b = np.where(inner, np.rint(np.where(inner, nodes["threshold"], 0.0) * 256.0).astype(np.int64) - 1, -1)
    m = codes.shape[0]
    rows = np.arange(m)
    out = np.empty((m, len(roots)), np.int64)
    for t, r in enumerate(roots):
        nd = np.full(m, int(r), np.int64)
        while True:
            live = inner[nd]
            if not live.any():
                break
            left = codes[rows, np.where(live, nodes["feature"][nd], 0)] <= b[nd]
            nd = np.where(live, np.where(left, nodes["left"][nd], nodes["right"][nd]), nd)
        out[:, t] = nd
    return out


def predict(nodes, roots, codes):
    """-> mu [m] = (0 + sum over trees, in tree order, of leaf value) / T in fp64,
    nothing fused: uthot.h's pred for base 0, scale 1, div T"""
    leaf = route(nodes, roots, codes)
    acc = np.zeros(leaf.shape[0])
    for t in range(len(roots)):
        acc = acc + nodes["value"][leaf[:, t]]
    return acc / float(len(roots))
