"""Test infrastructure: the CPU restatement of the feasibility vote (numpy, fp64),
over feature rows as oracle.space.features encodes them.

  k(a, u)   = exp(-1/2 |(a - u) / ell|^2 / s^2)
  S_ok(u)   = sum_r k(x_r, u)        S_fail(u) = sum_q k(f_q, u)
  p(u)      = (S_ok + lambda p0) / (S_ok + S_fail + lambda),  p0 = n / (n + n_f) unless given

Never used by uptune_amd."""
import numpy as np


def kernel_sum(A, U, ell, ell_scale=1.0):
    """sum over the rows of A [n][d] of k(a, u) for every row u of U [m][d]"""
    A, U = np.asarray(A, dtype=np.float64), np.asarray(U, dtype=np.float64)
    if A.shape[0] == 0:
        return np.zeros(U.shape[0])
    ell = np.broadcast_to(np.asarray(ell, dtype=np.float64), (U.shape[1],))
    As, Us = A / ell, U / ell
    out = np.zeros(U.shape[0])
    step = max(1, (1 << 24) // max(A.shape[0], 1))     # candidates per block: bounded memory
    an = np.sum(As * As, axis=1)[:, None]
    for j in range(0, U.shape[0], step):
        u = Us[j:j + step]
        d2 = np.maximum(an + np.sum(u * u, axis=1)[None, :] - 2.0 * (As @ u.T), 0.0)
        out[j:j + step] = np.exp(-0.5 * d2 / (ell_scale * ell_scale)).sum(axis=0)
    return out


def feas_prob(X_ok, X_fail, U, ell, prior=None, strength=1.0, ell_scale=1.0):
    """-> (p, S_ok, S_fail), each [m]"""
    X_ok = np.asarray(X_ok, dtype=np.float64)
    n = X_ok.shape[0]
    nf = 0 if X_fail is None else len(X_fail)
    s_ok = kernel_sum(X_ok, U, ell, ell_scale)
    X_fail = np.zeros((0, X_ok.shape[1])) if nf == 0 else np.asarray(X_fail, dtype=np.float64)
    s_fail = kernel_sum(X_fail, U, ell, ell_scale)
    p0 = n / (n + nf) if prior is None else float(prior)
    p = (s_ok + strength * p0) / (s_ok + s_fail + strength)
    return p, s_ok, s_fail


def auc(pos, neg):
    """P(a positive ranks above a negative), ties half"""
    pos, neg = np.asarray(pos)[:, None], np.asarray(neg)[None, :]
    return float(((pos > neg).sum() + 0.5 * (pos == neg).sum()) / (pos.size * neg.size))


def gcc_split(golden_dir, space):
    """the gcc fixture's split: the first 1,024 successful rows (OK), the failed
    rows among the first 3,000 (failed), rows 3000.. as candidates ->
    (X_ok, X_fail, U, cand_ok mask, (values ok, values fail, values cand))"""
    import os

    from oracle.space import features
    z = np.load(os.path.join(golden_dir, "gcc_history.npz"))
    vals, qor = z["values"], z["qor"]
    fin = np.isfinite(qor)
    ok_rows = np.flatnonzero(fin)[:1024]
    fail_rows = np.flatnonzero(~fin[:3000])
    cand = np.arange(3000, vals.shape[1])
    f = lambda rows: features(space, vals[:, rows]).T.copy()   # noqa: E731
    return f(ok_rows), f(fail_rows), f(cand), fin[cand], (vals[:, ok_rows], vals[:, fail_rows], vals[:, cand])
