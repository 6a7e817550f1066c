"""Test infrastructure: the Thompson-sampling rule of include/uthot.h
("Thompson sampling") restated in numpy, in fp64 and in np.longdouble (the
conventions of _fit_cases.py: the extended reference needs >= 63 mantissa
bits, have_longdouble()).  The checker and never the product; the reference
has no GP.

Draws.  The counter generator of oracle/philox.py with OP_TS = 7:
  Z[j][k]     = normal_draw(seed, cand = j, stream = k, round_, OP_TS)
  b[j]        = u01(x, y) of draw(seed, j, STREAM_CAND, round_, OP_TS)
  Theta[s][j] = normal_draw(seed, j, s | (1 << STREAM_SUB_SHIFT), round_, OP_TS)
  Eps[s][r]   = normal_draw(seed, r, s | (2 << STREAM_SUB_SHIFT), round_, OP_TS)
normal() below is oracle.mathx.normal_draw over an array of streams (the same
attempts, the same ut_log; test_ts_oracle_cpu.py holds the two equal bit for bit).

Paths, with us = u * inv_ell (inv_ell the fit's fp64 vector: data) and
Zs = fl(Z * INV_2PI), INV_2PI the fp64 nearest of 1 / (2 pi) -- the one place
the 1 / (2 pi) rounding sits, so Zs is data for both precisions:
  tau_j(u) = sum_k Zs[j][k] us_k + b_j,  phi_j = sqrt(2 sf2 / D) cos2pi(tau_j - rint(tau_j))
  g_s = sum_j Theta[s][j] phi_j,  r_s = ys - g_s(X) - sqrt(diag) Eps[s],  a_s = K^-1 r_s
  f_s(u) = g_s(u) + sum_r sf2 exp(-1/2 |xs_r - us|^2) a_s[r]
The fp64 restatement uses cos2pi (ut_core.h's polynomial, restated below bit
for bit); the long-double one the true cosine, so the two differ by at most
COS_ERR sqrt(2 sf2 / D) sum_j |Theta[s][j]| beside their rounding."""
import numpy as np

from oracle import mathx
from oracle import philox as ph

LD = np.longdouble
OP_TS = 7
INV_2PI = 0.15915494309189535
COS_ERR = 1.6e-16            # ut_core.h's UT_COS_ERR (test_ts_oracle_cpu.py measures it)
TIERS = [(1e-2, 1e-9), (1e-6, 1e-5)]       # (sigma_n2, rtol): the project's tiers (_polish_oracle.py)

_COS = (0.28200596845579123, -1.714390711088672, 7.903536371318469, -26.4262567833744, 60.24464137187666,
        -85.45681720669373, 64.9393940226683, -19.739208802178716, 1.0)
_SIN = (0.10422916220813984, -0.7181223017785006, 3.819952584848282, -15.09464257682299, 42.058693944897655,
        -76.70585975306139, 81.60524927607506, -41.34170224039976, 6.283185307179586)


def have_longdouble():
    return np.finfo(LD).nmant >= 63


def cos2pi(t):
    """ut_core.h's cos2pi, operation for operation (t in [-1/2, 1/2])"""
    t = np.asarray(t, dtype=np.float64)
    a = np.where(t < 0.0, -t, t)
    neg = a > 0.25
    a = np.where(neg, 0.5 - a, a)
    sb = a > 0.125
    z = np.where(sb, 0.25 - a, a)
    z2 = z * z
    p = np.where(sb, _SIN[0], _COS[0])
    for cs, cc in zip(_SIN[1:], _COS[1:]):
        p = p * z2 + np.where(sb, cs, cc)
    r = np.where(sb, z * p, p)
    return np.where(neg, -r, r)


def cos_true(t):
    """cos(2 pi t) in long double"""
    return np.cos((LD(2) * LD_PI) * np.asarray(t, dtype=LD))


# pi to 40 digits: more than the 64-bit significand holds
LD_PI = LD("3.141592653589793238462643383279502884197")


def normal(seed, cand, stream, round_, op=OP_TS):
    """oracle.mathx.normal_draw with cand and stream broadcast against each other"""
    cand, stream = np.broadcast_arrays(np.asarray(cand, dtype=np.uint64), np.asarray(stream, dtype=np.uint64))
    shape = cand.shape
    cand, stream = cand.ravel(), stream.ravel()
    out = np.zeros(cand.shape, dtype=np.float64)
    left = np.arange(cand.size)
    for a in range(16):
        if left.size == 0:
            break
        x, y, z, w = ph.draw(seed, cand[left], (stream[left] | np.uint64(a << 24)) & np.uint64(0xFFFFFFFF), round_, op)
        u = 2.0 * ph.u01(x, y) - 1.0
        v = 2.0 * ph.u01(z, w) - 1.0
        s = u * u + v * v
        ok = (s > 0.0) & (s < 1.0)
        ss = s[ok]
        out[left[ok]] = u[ok] * np.sqrt((-2.0 * mathx.ut_log(ss)) / ss)
        left = left[~ok]
    return out.reshape(shape)


def draws(seed, n, d, q, D, round_):
    """-> dict Z [D][d], b [D], Theta [q][D], Eps [q][n]"""
    j = np.arange(D, dtype=np.uint64)
    Z = normal(seed, j[:, None], np.arange(d, dtype=np.uint64)[None, :], round_)
    x, y, _, _ = ph.draw(seed, j, ph.STREAM_CAND, round_, OP_TS)
    b = ph.u01(x, y)
    s = np.arange(q, dtype=np.uint64)[:, None]
    Theta = normal(seed, j[None, :], s | np.uint64(1 << ph.STREAM_SUB_SHIFT), round_)
    Eps = normal(seed, np.arange(n, dtype=np.uint64)[None, :], s | np.uint64(2 << ph.STREAM_SUB_SHIFT), round_)
    return dict(Z=Z, b=b, Theta=Theta, Eps=Eps)


def standardise(y, dtype=np.float64):
    """k_gp_ystats' rule: the population deviation, 1 for a constant y"""
    y = np.asarray(y).astype(dtype)
    mean = np.sum(y) / dtype(len(y))
    sd = np.sqrt(np.sum((y - mean) ** 2) / dtype(len(y)))
    return (y - mean) / (sd if sd > 0 else dtype(1))


def sqdist(A, B):
    """|a_i - b_j|^2 in the difference form (no cancellation) -> [len(A)][len(B)]"""
    out = np.empty((A.shape[0], B.shape[0]), dtype=A.dtype)
    for i in range(A.shape[0]):
        q = A[i][None, :] - B
        out[i] = np.sum(q * q, axis=1)
    return out


def kernel(Xs, Us, sf2):
    """long double: the difference form; fp64: oracle/gp.py's Gram form |x|^2 + |u|^2 - 2 x.u, the form a
    contraction computes (its cancellation is the fp64 restatement's error, and the device's)"""
    dt = Xs.dtype.type
    if dt is LD:
        return dt(sf2) * np.exp(-sqdist(Xs, Us) / dt(2))
    from oracle.gp import sqdist as gram
    return sf2 * np.exp(-0.5 * gram(Xs, Us))


def chol(K):
    """the lower Cholesky factor in K's own precision (numpy has no LAPACK for long double)"""
    n = K.shape[0]
    L = np.zeros_like(K)
    for j in range(n):
        L[j, j] = np.sqrt(K[j, j] - L[j, :j] @ L[j, :j])
        if j + 1 < n:
            L[j + 1:, j] = (K[j + 1:, j] - L[j + 1:, :j] @ L[j, :j]) / L[j, j]
    return L


def solve_k(L, R):
    """K^-1 R^T for K = L L^T by substitution; R [q][n] -> [q][n]"""
    n = L.shape[0]
    Y = np.zeros_like(R.T)
    for i in range(n):
        Y[i] = (R.T[i] - L[i, :i] @ Y[:i]) / L[i, i]
    A = np.zeros_like(Y)
    for i in range(n - 1, -1, -1):
        A[i] = (Y[i] - L[i + 1:, i] @ A[i + 1:]) / L[i, i]
    return A.T


class Fit:
    """the rule's inputs in `dtype`: scaled rows, ys (given, or standardised from y), K = L L^T"""

    def __init__(self, X, y, ell, sf2, sn2, jitter, dtype=np.float64, ys=None):
        X = np.asarray(X, dtype=np.float64)
        self.dtype = dtype
        self.n, self.d = X.shape
        self.inv_ell = 1.0 / np.broadcast_to(np.asarray(ell, dtype=np.float64), (self.d,))   # fp64: data
        self.sf2, self.diag = float(sf2), float(sn2) + float(jitter)
        self.Xs = self.scaled(X)
        self.ys = (standardise(y, dtype) if ys is None else np.asarray(ys)).astype(dtype)
        K = kernel(self.Xs, self.Xs, self.sf2)
        K[np.diag_indices(self.n)] += dtype(self.diag)
        self.K = K
        self.L = chol(K) if dtype is LD else np.linalg.cholesky(K)

    def scaled(self, U):
        U = np.asarray(U, dtype=np.float64)
        if self.dtype is LD:
            return U.astype(LD) * self.inv_ell.astype(LD)[None, :]
        return U * self.inv_ell[None, :]


def prior(fit, dr, Us):
    """g_s at the scaled rows Us [m][d] -> [q][m]"""
    dt = fit.dtype
    D = dr["Z"].shape[0]
    Zs = (dr["Z"] * INV_2PI).astype(dt)
    tau = Us @ Zs.T + dr["b"].astype(dt)[None, :]            # [m][D], turns
    fr = tau - np.rint(tau)
    c = cos_true(fr) if dt is LD else cos2pi(fr)
    amp = np.sqrt(dt(2) * dt(fit.sf2) / dt(D))
    return dr["Theta"].astype(dt) @ (amp * c).T


def weights(fit, dr):
    """A [q][n] = K^-1 r_s, r_s = ys - g_s(X) - sqrt(diag) Eps[s]"""
    dt = fit.dtype
    R = fit.ys[None, :] - prior(fit, dr, fit.Xs) - np.sqrt(dt(fit.diag)) * dr["Eps"].astype(dt)
    return solve_k(fit.L, R)


def evaluate(fit, dr, A, U):
    """f_s(u_i) -> [q][m] for features U [m][d]; A [q][n] as given (the oracle's own or the device's)"""
    Us = fit.scaled(U)
    return prior(fit, dr, Us) + np.asarray(A).astype(fit.dtype) @ kernel(fit.Xs, Us, fit.sf2)


def select(F, dup, k):
    """the pick rule on F [q][m] -> (pos [k] int64, f [k]); an empty slot holds -1, +inf"""
    F = np.asarray(F)
    m = F.shape[1]
    free = np.ones(m, dtype=bool) if dup is None else (np.asarray(dup) == 0)
    free = free.copy()
    pos = np.full(k, -1, dtype=np.int64)
    f = np.full(k, np.inf)
    for s in range(k):
        idx = np.flatnonzero(free)
        if idx.size == 0:
            break
        v = F[s, idx]
        if np.isnan(v.astype(np.float64)).any():
            break
        at = idx[int(np.argmin(v))]                            # (the first of equal minima)
        pos[s], f[s] = at, float(F[s, at])
        free[at] = False
    return pos, f


def gap(F, dup, k):
    """per slot of the free walk: second-best remaining minus best (inf: one candidate left or an empty slot)"""
    F = np.asarray(F)
    free = (np.ones(F.shape[1], dtype=bool) if dup is None else (np.asarray(dup) == 0)).copy()
    out = np.full(k, np.inf)
    pos, _ = select(F, dup, k)
    for s in range(k):
        if pos[s] < 0:
            break
        v = np.sort(F[s, np.flatnonzero(free)])
        if v.size > 1:
            out[s] = float(v[1] - v[0])
        free[pos[s]] = False
    return out


# --------------------------------------------------------------------------- the cases
def mixed_space():
    """every parameter kind of tests/_spaces.py"""
    from _spaces import oracle_space
    from oracle.space import POW2, Param
    from uptune_amd import spaces
    return oracle_space(spaces.perm_mixed()) + [Param("pw", POW2, 1, 1024)]


def _c(n, d, D, m, q, sn2, ell="iso", space=None):
    return dict(name="n%d_d%s_D%d_m%d_q%d_sn%g_%s" % (n, "mix" if space else d, D, m, q, sn2, ell), n=n, d=d, D=D, m=m,
                q=q, sn2=sn2, ell=ell, space=space, sf2=1.0, jitter=1e-8)


# n in {1, 100, 129}, d in {5, 64}, D in {128, 256}, m in {1, 127, 129, 1000}, q in {1, 3, 33, 70}
# (33 and 70 cross the 32-path group), one ARD case, one mixed space, both tiers
CASES = [
    _c(1, 5, 128, 1, 1, 1e-2),
    _c(100, 5, 128, 127, 3, 1e-2),
    _c(100, 5, 256, 1000, 33, 1e-6),
    _c(129, 64, 256, 129, 70, 1e-2),
    _c(129, 64, 128, 1000, 3, 1e-6, ell="ard"),
    _c(100, 0, 128, 129, 33, 1e-2, space="mixed"),
    _c(1, 64, 256, 127, 70, 1e-6),
    _c(100, 5, 128, 127, 3, 1e-2, ell="tiny"),
]


def ids():
    return [c["name"] for c in CASES]


_DATA = {}


def data(c):
    """-> dict X [n][d], y, ell [d], U [m][d] (features), dup [m], space (oracle Params), tr / cand value
    rows [ncols][.]; U's first rows are training rows, its last one lies far from all data; cached, read-only"""
    if c["name"] in _DATA:
        return _DATA[c["name"]]
    from oracle import de as ode
    from oracle.space import FLOAT, Param, features
    n, m = c["n"], c["m"]
    rng = np.random.default_rng(9100 + 7 * n + m)
    if c["space"]:
        space = mixed_space()
        tr = ode.population_init(space, n, seed=8)
        cand = ode.population_init(space, m, seed=7)
    else:
        space = [Param("u%d" % k, FLOAT, 0.0, 1.0) for k in range(c["d"])]
        tr = rng.uniform(0.2, 0.8, size=(c["d"], n))
        cand = rng.uniform(0.2, 0.8, size=(c["d"], m))
        if m > 4:
            cand[:, -1] = 0.0                      # the box's corner; with ell "tiny" K* underflows to 0 there
    ntr = min(n, m // 2)
    cand[:, :ntr] = tr[:, :ntr]                    # candidates equal to training rows
    X = features(space, tr).T.copy()
    U = features(space, cand).T.copy()
    d = X.shape[1]
    if c["ell"] == "ard":
        ell = np.geomspace(0.3, 3.0, d)[rng.permutation(d)]
    elif c["space"]:
        ell = np.full(d, 1.5)
    else:
        ell = np.full(d, 0.01 if c["ell"] == "tiny" else 0.5 if d <= 8 else 2.0)
    y = np.sum((X - 0.4) ** 2, axis=1) + 0.01 * rng.standard_normal(n)
    dup = (rng.uniform(size=m) < 0.15).astype(np.uint8)
    z = dict(X=X, y=y, ell=ell, U=U, dup=dup, space=space, tr=tr, cand=cand, ntr=ntr, d=d)
    for a in z.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    _DATA[c["name"]] = z
    return z


def seed_of(c):
    return 11


def round_of(c):
    return 1 + CASES.index(c)
