"""Test infrastructure: the CPU restatement of two-objective scoring (numpy,
fp64) on the build's own GP (oracle.gp) -- the front rule and the expected
hypervolume improvement of include/uthot.h, "two objectives".  Both objectives
are minimised; Y2 [n] is row-aligned with X.

  y2s, m_2, s_2 = GP(X, Y2).ys, .mean, .std      alpha_2 = GP(X, Y2).alpha   (same L)
  mu_2(u)  = k*(u) . alpha_2                     r_j = (R_j - m_j) / s_j
  F        = rows inside the box that no row dominates (of identical points the smallest row)
  EHVI(u)  = sum_{i = 0..P} max(psi(a_{i+1}; mu_1) - psi(a_i; mu_1), 0) psi(b_i; mu_2)

Never used by uptune_amd."""
import numpy as np
from scipy.special import erfc

from oracle.gp import GP, sqdist


def front_rows(a, b, r1=np.inf, r2=np.inf):
    """rows of the front of the points (a[r], b[r]) inside the box below
    (r1, r2), ordered by (a, r) ascending -- the rule, compare by compare"""
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    n = a.shape[0]
    idx = np.arange(n)
    le = (a[None, :] <= a[:, None]) & (b[None, :] <= b[:, None])              # [r][s]: s <= r in both
    strict = (a[None, :] < a[:, None]) | (b[None, :] < b[:, None]) | (idx[None, :] < idx[:, None])
    keep = (a < r1) & (b < r2) & ~np.any(le & strict, axis=1)
    rows = idx[keep]
    return rows[np.lexsort((rows, a[rows]))]


def psi(t, mu, var):
    """E[(t - Y)+], Y ~ N(mu, var); var == 0: max(t - mu, 0); t = -inf: 0"""
    mu, var = np.asarray(mu, dtype=np.float64), np.asarray(var, dtype=np.float64)
    if np.isneginf(t):
        return np.zeros(np.broadcast(mu, var).shape)
    I = t - mu
    sigma = np.sqrt(var)
    with np.errstate(divide="ignore", invalid="ignore", under="ignore"):
        z = I / np.where(var == 0.0, 1.0, sigma)
        Phi = 0.5 * erfc(-z * 0.70710678118654752440)
        phi = np.exp(-0.5 * z * z) * 0.39894228040143267794
        smooth = I * Phi + sigma * phi
    return np.where(var == 0.0, np.maximum(I, 0.0), smooth)


def ehvi(mu1, var, mu2, a, b, r1, r2):
    """EHVI of candidates (mu1, var, mu2 [m]) against the ordered front (a, b [P])
    inside the box below (r1, r2): strips i = 0 .. P ascending"""
    A = np.concatenate([np.asarray(a, dtype=np.float64), [r1]])    # a_1 .. a_{P+1}
    B = np.concatenate([[r2], np.asarray(b, dtype=np.float64)])    # b_0 .. b_P
    prev = np.zeros(np.shape(mu1))                                 # psi(a_0 = -inf)
    acc = np.zeros(np.shape(mu1))
    for i in range(A.shape[0]):
        nxt = psi(A[i], mu1, var)
        acc = acc + np.maximum(nxt - prev, 0.0) * psi(B[i], mu2, var)
        prev = nxt
    return acc


def gain(y1, y2, a, b, r1, r2):
    """the hypervolume a point (y1, y2) (arrays alike) adds to the ordered front
    (a, b) inside the box: the strips' plain areas"""
    y1, y2 = np.asarray(y1, dtype=np.float64), np.asarray(y2, dtype=np.float64)
    lo = np.concatenate([[-np.inf], np.asarray(a, dtype=np.float64)])
    hi = np.concatenate([np.asarray(a, dtype=np.float64), [r1]])
    top = np.concatenate([[r2], np.asarray(b, dtype=np.float64)])
    g = np.zeros(y1.shape)
    for l, h, t in zip(lo, hi, top):
        g += np.maximum(h - np.maximum(y1, l), 0.0) * np.maximum(t - y2, 0.0)
    return g


def ehvi_mp(mu1, var, mu2, a, b, r1, r2, dps=40):
    """one candidate's EHVI at `dps` digits (mpmath), as an mpf"""
    import mpmath as mp
    with mp.workdps(dps):
        m1, m2, v = mp.mpf(float(mu1)), mp.mpf(float(mu2)), mp.mpf(float(var))
        s = mp.sqrt(v)

        def p(t, m):
            I = mp.mpf(float(t)) - m
            if v == 0:
                return max(I, mp.mpf(0))
            z = I / s
            return I * mp.erfc(-z / mp.sqrt(2)) / 2 + s * mp.exp(-z * z / 2) / mp.sqrt(2 * mp.pi)

        A = [float(x) for x in a] + [float(r1)]
        B = [float(r2)] + [float(x) for x in b]
        prev, acc = mp.mpf(0), mp.mpf(0)
        for t, u in zip(A, B):
            nxt = p(t, m1)
            acc += max(nxt - prev, mp.mpf(0)) * p(u, m2)
            prev = nxt
        return +acc


def rule_on(score0, e):
    """EHVI where a plain score is finite: -inf (a duplicate) and NaN (a failed fit) pass through"""
    return np.where(np.isfinite(score0), e, score0)


class MoGP:
    def __init__(self, X, y, Y2, ref, lengthscale, **hyper):
        X = np.asarray(X, dtype=np.float64)
        self.gp = GP(X, y, lengthscale, **hyper)
        self.gp2 = GP(X, Y2, lengthscale, **hyper)
        self.ys, self.y2s, self.alpha2 = self.gp.ys, self.gp2.ys, self.gp2.alpha
        self.r1 = (float(ref[0]) - self.gp.mean) / self.gp.std
        self.r2 = (float(ref[1]) - self.gp2.mean) / self.gp2.std
        self.rows = front_rows(self.ys, self.y2s, self.r1, self.r2)
        self.a, self.b = self.ys[self.rows], self.y2s[self.rows]

    def kstar(self, U):
        Us = np.asarray(U, dtype=np.float64) * self.gp.inv_ell
        return self.gp.sf2 * np.exp(-0.5 * sqdist(Us, self.gp.Xs))

    def mu2(self, U):
        return self.kstar(U) @ self.alpha2

    def posterior(self, U):
        return self.gp.posterior(U)

    def ehvi(self, mu1, var, mu2):
        return ehvi(mu1, var, mu2, self.a, self.b, self.r1, self.r2)
