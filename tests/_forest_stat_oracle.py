"""ut_forest_score restated in numpy (TEST INFRASTRUCTURE): the per-tree leaf
walk, the definition of include/uthot.h in fp64 in tree order, the same
quantities in np.longdouble from the per-tree leaves, and the per-candidate
tolerance

    tol_i = (T + 8) 2^-53 ((D2 + SV) / T + (D1 / T)^2)

-- the rounding of T-term sums of non-negative terms (D2, SV: relative error
at most T u each; D1's error at most T u sum |a_t| <= T u sqrt(T D2), which
squared and divided by T^2 is again of the order of D2 / T) plus the handful
of final operations, all of the order of the variance itself because every
a_t = m_t - m_0 is a difference of leaves, never a leaf's own magnitude."""
import numpy as np


def leaves(nodes, roots, rule, X):
    """leaf node index [m][T] of every row of X [m][F] in every tree; the
    traversal of oracle/forest.py, one tree at a time over all rows"""
    X = np.asarray(X, np.float64)
    with np.errstate(over="ignore", invalid="ignore"):
        X32 = X.astype(np.float32).astype(np.float64)
        thr = nodes["threshold"].astype(np.float64)
        if rule != 0:   # LT: float32(x) < float32(thr)
            thr = thr.astype(np.float32).astype(np.float64)
    feature, lchild, rchild = nodes["feature"], nodes["left"], nodes["right"]
    dleft = nodes["default_left"] != 0
    m = X32.shape[0]
    rows = np.arange(m)
    out = np.empty((m, len(roots)), np.int64)
    for t, r in enumerate(roots):
        nd = np.full(m, int(r), np.int64)
        while True:
            f = feature[nd]
            live = f >= 0
            if not live.any():
                break
            x = X32[rows, np.where(live, f, 0)]
            with np.errstate(invalid="ignore"):
                left = np.where(x != x, dleft[nd], (x <= thr[nd]) if rule == 0 else (x < thr[nd]))
            nd = np.where(live, np.where(left, lchild[nd], rchild[nd]), nd)
        out[:, t] = nd
    return out


def stats(nodes, roots, rule, div, X, leaf_var=None, base=0.0, scale=1.0):
    """-> dict of [m] arrays: mu, var (fp64, tree order, nothing fused), var_ext
    (np.longdouble, rounded to fp64 at the end), var_unshifted (the textbook
    sum m_t^2 / T - mu^2 form in fp64), tol, and leaf [m][T]"""
    lf = leaves(nodes, roots, rule, X)
    T = len(roots)
    val = nodes["value"].astype(np.float64)[lf]                               # [m][T]
    sv = np.zeros_like(val) if leaf_var is None else np.asarray(leaf_var, np.float64)[lf]
    m0 = val[:, 0]
    acc = np.full(val.shape[0], float(base))
    D1, D2, SV, Q = (np.zeros(val.shape[0]) for _ in range(4))
    for t in range(T):
        acc = acc + float(scale) * val[:, t]
        a = val[:, t] - m0
        D1 = D1 + a
        D2 = D2 + a * a
        SV = SV + sv[:, t]
        Q = Q + val[:, t] * val[:, t]
    mu = acc / float(div)
    Td = float(T)
    e = D1 / Td
    v0 = (D2 + SV) / Td - e * e
    var = np.where(v0 > 0.0, v0, 0.0)
    u0 = (Q + SV) / Td - mu * mu
    var_unshifted = np.where(u0 > 0.0, u0, 0.0)
    # extended: the same shifted quantities, every operation in long double
    L = np.longdouble
    aL = val.astype(L) - m0.astype(L)[:, None]
    D1L, D2L, SVL = (np.zeros(val.shape[0], L) for _ in range(3))
    for t in range(T):
        D1L = D1L + aL[:, t]
        D2L = D2L + aL[:, t] * aL[:, t]
        SVL = SVL + sv[:, t].astype(L)
    eL = D1L / L(T)
    vL = (D2L + SVL) / L(T) - eL * eL
    var_ext = np.where(vL > 0, vL, L(0))
    tol = ((T + 8) * 2.0 ** -53 * ((D2L + SVL) / L(T) + eL * eL)).astype(np.float64)
    return {"mu": mu, "var": var, "var_ext": var_ext.astype(np.float64), "var_ext_ld": var_ext,
            "var_unshifted": var_unshifted, "tol": tol, "leaf": lf}
