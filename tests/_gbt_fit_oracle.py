"""ut_gbt_fit restated in numpy and Python integers (include/uthot.h states the
definition): 256-bin codes, per round 16.16 fixed-point gradients of the squared
error, a Philox row sample and per-level feature draw, trees grown breadth first
by heap index on s = G_L^2 / (H_L + lambda) + G_R^2 / (H_R + lambda) with ties
to the smaller feature, then bin.  Every histogram entry is an integer below
2^53, so np.bincount's float64 sums are exact; every fp64 operation is written
in the order the header states."""
import numpy as np

from _rf_fit_oracle import codes_of
from oracle.philox import draw
from uptune_amd.forest import NODE_DTYPE

OP_GBT = 9


def sampled(seed, r, n, round_, frac):
    if frac >= 1.0:
        return np.ones(n, bool)
    words = np.stack(draw(seed, np.arange((n + 3) // 4), r, round_, OP_GBT), axis=1).reshape(-1)[:n]
    return words.astype(np.float64) < frac * 4294967296.0


def eligible(seed, r, level, d, round_, frac):
    if frac >= 1.0:
        return np.ones(d, bool)
    j = np.arange(d, dtype=np.uint64)
    w = np.stack(draw(seed, (np.uint64(level) << np.uint64(32)) | (j >> np.uint64(2)), 0x10000 | r, round_, OP_GBT),
                 axis=1)
    return w[np.arange(d), (j & np.uint64(3)).astype(np.int64)].astype(np.float64) < frac * 4294967296.0


def step_of(G, H, eta, lam):
    if H == 0:
        return 0.0
    t1 = float(-G) / (float(H) + lam)
    return (eta * t1) / 65536.0


def best_split(codes, g, rows, elig, min_child, lam):
    """-> (s, j, b) of the largest s among the valid splits over the sampled rows, or None"""
    d = codes.shape[1]
    flat = (codes[rows] + 256 * np.arange(d)).ravel()
    HL = np.cumsum(np.bincount(flat, None, 256 * d).reshape(d, 256), axis=1)[:, :255]
    GL = np.cumsum(np.bincount(flat, np.repeat(g[rows], d), 256 * d).reshape(d, 256), axis=1)[:, :255]
    HR, GR = len(rows) - HL, float(g[rows].sum()) - GL
    valid = (HL >= min_child) & (HR >= min_child) & elig[:, None]
    if not valid.any():
        return None
    with np.errstate(divide="ignore", invalid="ignore"):
        s = np.where(valid, (GL * GL) / (HL + lam) + (GR * GR) / (HR + lam), -1.0)
    k = int(np.argmax(s))   # the first maximum: smaller j, then smaller b
    return (float(s.ravel()[k]),) + divmod(k, 255)


def grow(codes, g, samp, pred, r, seed, round_, max_depth, min_child, eta, lam, gamma, colsample, scale):
    """one tree's records in heap order, child indices within the tree; adds the leaves' steps to pred"""
    d = codes.shape[1]
    heap = {0: np.arange(len(g))}   # heap index -> every row that reached the node
    recs = {}
    for level in range(max_depth + 1):
        elig = eligible(seed, r, level, d, round_, colsample)
        for k in range(2 ** level - 1, 2 ** (level + 1) - 1):
            if k not in heap:
                continue
            rows = heap[k]
            srows = rows[samp[rows]]
            G, H = int(g[srows].sum()), len(srows)
            step = step_of(G, H, eta, lam)
            split = best_split(codes, g, srows, elig, min_child, lam) if level < max_depth and H else None
            if split is not None:
                s, j, b = split
                parent = (float(G) * float(G)) / (float(H) + lam)
                if not s - parent > gamma:
                    split = None
            if split is None:
                recs[k] = (-1, -1, -1, 0, 0.0, scale * step)
                pred[rows] = pred[rows] + step
            else:
                left = codes[rows, j] <= b
                recs[k] = (j, 2 * k + 1, 2 * k + 2, 1, (b + 1) / 256.0, scale * step)
                heap[2 * k + 1], heap[2 * k + 2] = rows[left], rows[~left]
    order = sorted(recs)
    pos = {k: i for i, k in enumerate(order)}
    return np.array([recs[k][:1] + ((pos[recs[k][1]], pos[recs[k][2]]) if recs[k][0] >= 0 else (-1, -1)) + recs[k][3:]
                     for k in order], dtype=NODE_DTYPE)


def fit(X, y, seed, n_rounds=300, max_depth=10, min_child=1, eta=0.015, reg_lambda=1.0, gamma=0.0, subsample=0.4,
        colsample_bylevel=0.5, y_shift=None, y_scale=None, seed_round=0):
    """-> (roots [T] int32, nodes [N] NODE_DTYPE as ut_forest_get returns them, pred [n] in normalised units);
    y_shift / y_scale default to engine.gbt_fit's: mean and std, 1 for a constant y"""
    y = np.asarray(y, np.float64)
    shift = float(np.mean(y)) if y_shift is None else y_shift
    scale = (float(np.std(y)) or 1.0) if y_scale is None else y_scale
    codes = codes_of(X)
    z = np.clip((y - shift) / scale, -32.0, 32.0)
    pred = np.zeros(len(y))
    trees = []
    for r in range(n_rounds):
        g = np.rint(np.clip(pred - z, -64.0, 64.0) * 65536.0).astype(np.int64)
        samp = sampled(seed, r, len(y), seed_round, subsample)
        trees.append(grow(codes, g, samp, pred, r, seed, seed_round, max_depth, min_child, eta, reg_lambda, gamma,
                          colsample_bylevel, scale))
    roots = np.cumsum([0] + [len(a) for a in trees[:-1]]).astype(np.int32)
    for a, r0 in zip(trees, roots):
        inner = a["feature"] >= 0
        a["left"][inner] += r0
        a["right"][inner] += r0
    return roots, np.concatenate(trees), pred
