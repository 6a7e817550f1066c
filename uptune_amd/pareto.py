"""Two-objective bookkeeping on the host (numpy, no GPU): the Pareto front of
measured results, its hypervolume, a default reference point.

Both objectives are minimised.  The front rule is the device's
(include/uthot.h, "two objectives"): point r stays iff no point s has
p_s <= p_r in both coordinates and one of p_s[0] < p_r[0], p_s[1] < p_r[1],
s < r -- of identical points the smallest index stays.
"""
from __future__ import annotations

import numpy as np


def _points(points) -> np.ndarray:
    p = np.asarray(points, dtype=np.float64)
    if p.size == 0:
        return p.reshape(0, 2)
    if p.ndim != 2 or p.shape[1] != 2:
        raise ValueError("points: [n][2]")
    return p


def nondominated(points) -> np.ndarray:
    """indices of the non-dominated points, ordered by (first objective, index)
    ascending: the first coordinate then rises strictly and the second falls
    strictly"""
    p = _points(points)
    n = p.shape[0]
    if n == 0:
        return np.zeros(0, dtype=np.int64)
    # sorted by (a, b, index): a point is dominated iff an earlier one in this
    # order has b <= its b (an equal point earlier in the order has the smaller index)
    order = np.lexsort((np.arange(n), p[:, 1], p[:, 0]))
    keep = []
    best_b = np.inf
    for r in order:
        if p[r, 1] < best_b:
            keep.append(r)
            best_b = p[r, 1]
    return np.asarray(keep, dtype=np.int64)


def hypervolume2d(points, ref) -> float:
    """area dominated by `points` inside the box below `ref` (points outside it
    add nothing)"""
    p = _points(points)
    r1, r2 = float(ref[0]), float(ref[1])
    p = p[(p[:, 0] < r1) & (p[:, 1] < r2)]
    f = p[nondominated(p)]
    if f.shape[0] == 0:
        return 0.0
    a = np.append(f[:, 0], r1)
    return float(np.sum((a[1:] - a[:-1]) * (r2 - f[:, 1])))


def default_ref(points) -> np.ndarray:
    """per objective max + 0.1 (max - min), or max + 1 where the range is 0"""
    p = _points(points)
    if p.shape[0] == 0:
        raise ValueError("default_ref: no points")
    hi, lo = p.max(axis=0), p.min(axis=0)
    span = hi - lo
    return hi + np.where(span > 0.0, 0.1 * span, 1.0)
