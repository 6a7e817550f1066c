"""The TPE surrogate of include/uthot.h restated in numpy: split, bandwidths and
weights in fp64 as stated, Z from math.erf, the rest in np.longdouble.

Error bound of a tier (`Fit.score` returns it), from the documented operation
sequence; u = 2^-24 (f32) or 2^-53 (fp64).  A term exp2(e), e = A t + B, t = d d,
d = round(x - mu): d carries u, t 3u, the rounded A u, the fma one rounding of e,
the rounded B u |B|, so |de| <= u (5 |A t| + 2 |B|); the fit's own fp64 B (Z from
two erf at a few ulps, Z >= 0.34) adds 8 * 2^-53 (1 + |B|) in either tier; exp2
is within 1 ulp = 2u (v_exp_f32; the device library's fp64 exp2); a term below
the normal range (e < -125, -1021) may flush to 0 and counts whole.  A term v_i
is thus off by v_i r_i, r_i = ln 2 |de_i| + 2u, and the sum of the C positive
terms, added in the tier in any order, by sum v_i r_i + (C - 1) u sum v_i; its
fp64 log adds 2^-52 (1 + |log|).  The exact v_i weigh the bound, so the large
|e| of a term that cannot matter beside the prior's weighs nothing.  A
categorical log-probability is held to 4 ulps by the fit's test: 2^-50 |log p|.
logl, logg and the score add these over the features, plus 2^-53 of the summed
magnitudes per fp64 addition (two per feature), widened by 1%."""
import math

import numpy as np

LD = np.longdouble
_erf = np.vectorize(math.erf, otypes=[np.float64])
LOG2E, LN2 = LD(1) / np.log(LD(2)), np.log(LD(2))


def mixture(vals, pw=1.0):
    """one numeric feature of one set -> (mu, sigma) fp64, prior first among equals; w, Z longdouble"""
    s = len(vals)
    v = np.sort(np.asarray(vals, dtype=np.float64))
    pos = int(np.searchsorted(v, 0.5, side="left"))
    mu = np.insert(v, pos, 0.5)
    gaps = np.diff(mu)
    sig = np.maximum(np.concatenate([[0.0], gaps]), np.concatenate([gaps, [0.0]]))
    sig = np.clip(sig, 1.0 / min(100, s + 2), 1.0)
    sig[pos] = 1.0
    w = np.full(s + 1, LD(1) / (LD(s) + LD(pw)))
    w[pos] = LD(pw) / (LD(s) + LD(pw))
    r2 = sig * 1.4142135623730951
    Z = (_erf((1.0 - mu) / r2).astype(LD) - _erf(-mu / r2).astype(LD)) / 2
    return mu, sig, w, Z


def density(x, mu, sig, w, Z):
    """the truncated mixture's density at x (longdouble)"""
    x, mu, sig = np.asarray(x, dtype=LD)[:, None], mu.astype(LD), sig.astype(LD)
    return (w / (sig * np.sqrt(2 * LD(np.pi)) * Z) * np.exp(-((x - mu) ** 2) / (2 * sig * sig))).sum(axis=1)


def cat_logp(counts, s, pw=1.0):
    return np.log((np.asarray(counts, dtype=LD) + LD(pw) / len(counts)) / (LD(s) + LD(pw)))


class Fit:
    def __init__(self, X, y, kinds=None, gamma=0.10, n_good_max=25, prior_weight=1.0):
        X = np.asarray(X, dtype=np.float64)
        self.d, self.pw = X.shape[1], prior_weight
        self.kinds = np.zeros(self.d, dtype=np.int32) if kinds is None else np.asarray(kinds)
        nl = max(1, min(int(math.ceil(gamma * len(y))), n_good_max, len(y) - 1))
        order = np.argsort(np.asarray(y, dtype=np.float64), kind="stable")
        self.sets = np.sort(order[:nl]), np.sort(order[nl:])   # good rows, bad rows, each in row order
        self.num, self.cat = {}, {}
        for j in range(self.d):
            q = self.kinds[j]
            if q == 0:
                self.num[j] = [mixture(X[rows, j], prior_weight) for rows in self.sets]
            elif q >= 1:   # BOOL: the counts of the values 0 and 1
                self.cat[j] = [cat_logp(X[rows, j:j + q].sum(axis=0) if q > 1 else
                                        [len(rows) - X[rows, j].sum(), X[rows, j].sum()], len(rows), prior_weight)
                               for rows in self.sets]

    def components(self, j, set_):
        """what ut_tpe_get reads: (mu, sigma, ln(w / Z)), or (None, None, log p) of a block"""
        if j in self.cat:
            return None, None, self.cat[j][set_]
        mu, sig, w, Z = self.num[j][set_]
        return mu, sig, np.log(w / Z)

    def _log_mixture(self, x, comp, tier):
        mu, sig, w, Z = comp
        u = LD(2) ** (-24 if tier == 32 else -53)
        x = np.asarray(x, dtype=LD)[:, None]
        A = -LOG2E / (2 * sig.astype(LD) ** 2)
        B = np.log2(w / (sig.astype(LD) * np.sqrt(2 * LD(np.pi)) * Z))
        At = A * (x - mu.astype(LD)) ** 2
        v = np.exp2(At + B)
        r = LN2 * (u * (5 * np.abs(At) + 2 * np.abs(B)) + 8 * LD(2) ** -53 * (1 + np.abs(B))) + 2 * u
        r = np.where(At + B < (-125 if tier == 32 else -1021), LD(1), r)
        tot = v.sum(axis=1)
        lg = np.log(tot)
        return lg, (v * r).sum(axis=1) / tot + (len(mu) - 1) * u + LD(2) ** -52 * (1 + np.abs(lg))

    def score(self, F, tier):
        """F [m][d] candidates -> (score, logl, logg), (their bounds), longdouble"""
        F = np.asarray(F, dtype=np.float64)
        val, err, mag = np.zeros((2, len(F)), dtype=LD), np.zeros((2, len(F)), dtype=LD), np.zeros(len(F), dtype=LD)
        for j in range(self.d):
            for s in range(2):
                if j in self.num:
                    lg, e = self._log_mixture(F[:, j], self.num[j][s], tier)
                elif j in self.cat:
                    lg = (self.cat[j][s][(F[:, j] != 0).astype(int)] if self.kinds[j] == 1 else
                          (F[:, j:j + self.kinds[j]].astype(LD) * self.cat[j][s]).sum(axis=1))
                    e = LD(2) ** -50 * np.abs(lg)
                else:
                    continue
                val[s], err[s], mag = val[s] + lg, err[s] + e, mag + np.abs(lg)
        acc = 2 * self.d * LD(2) ** -53 * mag
        bl, bg = 1.01 * (err[0] + acc), 1.01 * (err[1] + acc)
        return (val[0] - val[1], val[0], val[1]), (bl + bg, bl, bg)
