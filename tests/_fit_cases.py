"""Test infrastructure: the case table, the extended-precision reference, the
measures and a numpy restatement of the GP fit (gp_fit.hip, k_split_i8 /
k_i8_errsum), whose operands -- L, L^-1, (L^-1)^T, beta, alpha, ys, the f32
copy and the int8 digit planes -- ut_gp_fit_read hands back element by element.
Shared by test_fit_cases_cpu.py (the table, the references and the mutants, on
the CPU) and test_gpu_fit_factor.py (the device held to them).  The checker and
never the product.

Reference.  K_ext: K_ij = sf2 exp(-sum_k ((x_ik - x_jk) / ell_k)^2 / 2) +
diag [i = j], diag = sigma_n2 + jitter, in np.longdouble (>= 63 mantissa bits
asserted) from the raw X, ell, sf2: the difference form has no cancellation,
so its own error is (d + 3) 2^-64 relative.  inv_lower(L, longdouble): the
inverse of a given lower-triangular matrix by row substitution.

Eps_ij, the first-order relative error of k_gp_kmat's element in units of
u = 2^-53, from the code (k_gp_prep_train, k_gp_kmat), with x' = x / ell,
S = |x'_i|^2 + |x'_j|^2:
  x' = fl(x fl(1 / ell)): 2u per component, so the squared distance moves by
      2 |x'_i - x'_j| 2u (|x'_i| + |x'_j|) <= 4u (|x'_i| + |x'_j|)^2 <= 8u S
  the norms: d sequential (fused or not) multiply-adds, (d + 1) u each: (d + 1) u S
  the Gram product (tile64_nt, d products per element in any order):
      2 d u |x'_i| |x'_j| <= d u S
  d2 = fl(fl(xn_i + xn_j) - 2 G): u S + u d2 <= 3u S
so (2d + 12) u S on d2 and (d + 6) u S on the exponent -d2 / 2, which is the
relative error it gives the exponential; exp itself 1 ulp (2u), the product
with sf2 u, the diagonal's sum u:
  Eps_ij = (d + 6) S + 4.

Measures, each max over j <= i < n of |error_ij| / scale_ij in longdouble
(the padded rows are exact identity rows, checked bitwise, so the leading
n x n blocks stand alone):
  chol   L^ L^T - K_ext              over u (|L^| |L^T| + Eps o |K|), rows < l_rows
  inv    X^ - inv_lower(L^)          over u |X^| |L^| |X^|  (componentwise forward bound)
  white  X^ K_ext X^T - I            over u (M M^T + |X^| (Eps o |K|) |X^|^T),
                                     M = |X^| |L_ref|, L_ref LAPACK's fp64 factor
  beta   beta^ - X^ ys^              over gamma_(i+1) (|X^| |ys^|)_i  (the device's own X^, ys^)
  alpha  alpha^ - X^T beta^          over gamma_(n-i) (|X^T| |beta^|)_i
  ys     ys^ - standardise(y)        over ys_bound (below)
gamma_k = k u / (1 - k u) bounds a k-term dot product summed in any order
(k_lower_mv / k_upper_mv: 64 strided partial sums and a butterfly; row i has
i + 1, n - i nonzero terms), so beta, alpha and ys pass at <= 1.

ys_bound, from k_gp_ystats: the sum is 256 strided partials of c = ceil(n / 256)
terms and an 8-level tree, so |dmean| <= (c + 9) u mean|y| (gamma_(c + 8) on the
sum, u on the division); dlt = fl(y - mean^) (u); the sum of squares takes
2u + gamma_(c + 8) per term, the division u, and sd = sqrt(.) halves that and
adds its own rounding (<= 1 ulp): dsd / sd <= ((c + 11) / 2 + 2) u; the final
division <= 1 ulp.  With the sum of dlt zero to first order the mean's error
does not reach sd at first order:
  |dys_i| <= u (|ys_i| (5 + (c + 11) / 2) + (c + 9) mean|y| / sd).
ut_gp_stats' mean and std are held to |dmean| and dsd above, f_best to min ys^.

Yardstick.  chol, inv and white pass at rho_dev <= 4 rho_ref (n <= 64, where one
sqrt's or division's rounding is the whole error: max(4 rho_ref, 1)), rho_ref
the larger of two fp64 numpy fits of the same inputs under the same measure:
(a) lapack(): Gram-form K, np.linalg.cholesky, a triangular solve against I;
(b) restate(): gp_fit.hip's algorithm -- k_gp_kmat's Gram form, the 64-row
blocked right-looking Cholesky with chol_diag_core's reciprocal pivots and
its substitution for the diagonal block's inverse, L_ik = A_ik inv(L_kk)^T,
the trailing update, recursive doubling X21 = -X22 (L21 X11) with the ragged
last pair, and for appends B = K21 L^-T, D = chol(K22 - B B^T),
C = -D^-1 (B L^-1) in APP_KC = 256 chunks summed in chunk order.  (numpy's
products round twice where the device's fused multiply-adds round once and
BLAS orders a sum differently from the MFMA's 4-k groups: what the 4 is for.)
A hard cap holds besides, rho <= n + d + 8: gamma_(n+1) is Cholesky's and the
substitution's backward error constant, the products of recursive doubling
add one gamma_s per level (sum < n), Eps's share is <= 1.

Mutants of restate(), each of which test_fit_cases_cpu.py requires to exceed
4 rho_ref in the measure named, on every tight case (n > 64) it applies to:
  l_tile_f32    a 16 x 16 tile of L rounded to fp32                       chol
  x_tile_f32    a 16 x 16 tile of L^-1 rounded to fp32                    inv
  no_jitter     diag = sigma_n2 alone                                     chol
  upd_chunk     one 16-k chunk dropped from one trailing-update tile      chol
  dbl_chunk     one 16-k chunk dropped from one recursive-doubling tile   inv
  ragged_k      the ragged pair's T = L21 X11 contracted over s2, not s   inv
                (cases with a ragged pair; phase 1 run over s instead of s2
                leaves the matrix and has no restatement, this is its mirror)
  app_stale     an append block's E = B L^-1 from the inverse before the
                previous block's append (chains that append two blocks)   white
"""
import math

import numpy as np

import _ard_cases as A
import _kstar_cases as KC

LD = np.longdouble
U53 = 2.0 ** -53
NB = 64
NPAD = 128
APP_KC = 256
TRB_MIN = 256
FACTOR = 4.0
I8_C = 3.5 * 2.0 ** -49
MEASURES = ("chol", "inv", "white")
MUTANTS = {"l_tile_f32": "chol", "x_tile_f32": "inv", "no_jitter": "chol", "upd_chunk": "chol",
           "dbl_chunk": "inv", "ragged_k": "inv", "app_stale": "white"}


def have_longdouble():
    return np.finfo(LD).nmant >= 63


def npad_of(n):
    return (n + NPAD - 1) // NPAD * NPAD


def levels(npad):
    """recursive doubling's levels: (s, pairs, s2 of the last pair, kernel)"""
    out = []
    s = NB
    while s < npad:
        pairs = (npad - s + 2 * s - 1) // (2 * s)
        s2 = min(s, npad - (pairs - 1) * 2 * s - s)
        out.append((s, pairs, s2, "big" if s >= TRB_MIN else "level"))
        s *= 2
    return out


# --------------------------------------------------------------------------- the cases
def _c(n, d, ell, sf2, sn2, **kw):
    name = "n%d_d%d_%s_sf%g_sn%g" % (n, d, ell, sf2, sn2)
    for k in sorted(kw):
        name += "_%s" % k
    return dict(dict(name=name, n=n, d=d, ell=ell, sf2=sf2, sn2=sn2, jitter=1e-8 * sf2, dup=False, cat=False,
                     panel=False, tight=n > 64), **kw)


# n -> npad and the path: 1, 63, 64, 65 -> 128 (one or two 64-blocks, the second partly or
# wholly identity padding); 128 -> 128; 129 -> 256 (level 128 on k_trinv_level); 300 -> 384
# (level 256 on k_trinv_big, ragged 256 + 128); 520 -> 640 (level 512, ragged 512 + 128);
# 700 -> 768 (level 512, ragged 512 + 256).  ell: "lo" / "hi" as _kstar_cases, or a recipe of
# _ard_cases.ell_vector.  dup: the last 5 rows are the first 5 plus 1e-9 (their Schur
# complement is about diag).  cat: _ard_cases.mixed_space's features (the fit stages the
# categorical K*'s operands beside the factor).  panel: rows that share their one-hot
# codes make the diagonal blocks ill conditioned, and L_ik = A_ik inv(L_kk)^T -- a product
# with an explicit inverse where LAPACK solves -- costs the restatement (and the device)
# about cond(L_kk) / 2 in chol against LAPACK: 40 against 2 on the categorical case, 2.8
# against 0.9 on 520 rows in three dimensions.  The two references are not required to
# agree on chol for such a case; the device's line and the cap hold as ever.
CASES = [
    _c(1, 3, "lo", 1.0, 1e-6),
    _c(63, 33, "hi", 37.0, 1e-2),
    _c(64, 3, "hi", 1e-3, 1e-9),
    _c(65, 64, "lo", 1.0, 1e-6, dup=True),
    _c(128, 33, "lo", 37.0, 1e-9),
    _c(129, 33, "one_short_first", 1.0, 1e-6),
    _c(129, 9, "groups", 1.0, 1e-2, cat=True, panel=True),
    _c(300, 64, "hi", 1.0, 1e-6),
    _c(520, 3, "lo", 1.0, 1e-2, panel=True),
    _c(700, 33, "lo", 1e-3, 1e-9),
]
PATHS = {1: (128, 0), 63: (128, 0), 64: (128, 0), 65: (128, 0), 128: (128, 0), 129: (256, 0),
         300: (384, 128), 520: (640, 128), 700: (768, 256)}     # n -> npad, the ragged pair's s2 (0: none)
# context switches (read when the context is created) x the cases they run on, by n
SWITCHES = [({}, None), ({"UT_CHOL_FUSE": "1"}, (300, 700)), ({"UT_CHOL_FUSE": "0"}, (300, 700)),
            ({"UT_CHOL_MERGED": "0"}, (300,)), ({"UT_TRINV_BIG": "0"}, (300,))]
# append chains of test_gp_fit_append_equals_refit: n0, steps, d (ell 0.5, sf2 1, sn2 1e-6, jitter 1e-8)
CHAINS = [(130, (120,), 8), (513, (1,) * 7 + (3,), 16), (40, (4,) * 6, 7), (700, (60,), 32)]
CHAIN_L_ROWS = {130: 128, 513: 512, 40: 0, 700: 640}


def ids():
    return [c["name"] for c in CASES]


def chain_case(n0, steps, d):
    n = n0 + sum(steps)
    return dict(name="chain_n%d_%s_d%d" % (n0, "x".join(str(s) for s in sorted(set(steps))), d), n=n, n0=n0,
                steps=tuple(steps), d=d, ell="chain", sf2=1.0, sn2=1e-6, jitter=1e-8, dup=False, cat=False,
                panel=False, tight=n > 64)


def ell_of(c):
    d = c["d"]
    if c["ell"] == "lo":
        return np.full(d, 0.2 * KC.sqrt_ish(d))
    if c["ell"] == "hi":
        return np.full(d, 2.0 * KC.sqrt_ish(d))
    if c["ell"] == "chain":
        return np.full(d, 0.5)
    return A.ell_vector(c["ell"], d, 1.5)


_DATA = {}


def data(c):
    """-> dict X [n][d], y [n], ell [d], diag, space, K_ext [n][n] longdouble, eps [n][n],
    ys_ref [n] longdouble, mean, sd; computed once, read-only"""
    if c["name"] not in _DATA:
        n, d = c["n"], c["d"]
        rng = np.random.default_rng(7000 + 10 * n + d)
        if c["cat"]:
            from oracle import de as ode
            from oracle.space import features
            space = A.mixed_space()
            X = features(space, ode.population_init(space, n, seed=8)).T.copy()
            assert X.shape == (n, d)
            ell = np.ascontiguousarray(A.group_values(A.CATEGORICAL[0], space)[A.ell_groups(space)])
        else:
            space = A.float_space(d)
            X = rng.uniform(size=(n, d))
            ell = ell_of(c)
        if c["dup"]:
            X[n - 5:] = X[:5] + 1e-9
        y = np.sum((X - 0.4) ** 2, axis=1) + 0.01 * rng.standard_normal(n)
        diag = c["sn2"] + c["jitter"]
        yl = y.astype(LD)
        mean = np.sum(yl) / LD(n)
        sd = np.sqrt(np.sum((yl - mean) ** 2) / LD(n))
        sd = sd if sd > 0 else LD(1)               # (k_gp_ystats: a constant y keeps sd = 1)
        z = dict(X=X, y=y, ell=ell, diag=diag, space=space, K_ext=k_ext(X, ell, c["sf2"], diag),
                 eps=eps_rel(X, ell), ys_ref=(yl - mean) / sd, mean=mean, sd=sd)
        for a in z.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _DATA[c["name"]] = z
    return _DATA[c["name"]]


# --------------------------------------------------------------------------- the reference
def k_ext(X, ell, sf2, diag):
    assert have_longdouble(), "np.longdouble has fewer than 63 mantissa bits here"
    Xl = X.astype(LD) / np.asarray(ell).astype(LD)[None, :]
    n = X.shape[0]
    K = np.empty((n, n), dtype=LD)
    for i in range(n):
        q = Xl[i][None, :] - Xl
        K[i] = LD(sf2) * np.exp(-np.sum(q * q, axis=1) / LD(2))
    K[np.arange(n), np.arange(n)] += LD(diag)
    return K


def eps_rel(X, ell):
    Xs = X * (1.0 / np.asarray(ell, dtype=np.float64))[None, :]
    xn = np.sum(Xs * Xs, axis=1)
    return (X.shape[1] + 6) * (xn[:, None] + xn[None, :]) + 4.0


def inv_lower(L, dtype=LD):
    """the inverse of lower-triangular L by row substitution, in dtype"""
    L = np.asarray(L).astype(dtype)
    n = L.shape[0]
    X = np.zeros((n, n), dtype=dtype)
    for i in range(n):
        r = -(L[i, :i] @ X[:i, :i]) if i else np.zeros(0, dtype=dtype)
        X[i, :i] = r / L[i, i]
        X[i, i] = dtype(1) / L[i, i]
    return X


def ys_bound(y, ys_ref, sd):
    n = len(y)
    c = (n + 255) // 256
    return U53 * (np.abs(ys_ref).astype(np.float64) * (5.0 + (c + 11) / 2.0)
                  + (c + 9) * float(np.mean(np.abs(y))) / float(sd))


def stats_bounds(y, sd):
    """-> (|dmean|, |dsd|) allowed of ut_gp_stats"""
    c = (len(y) + 255) // 256
    return (c + 9) * U53 * float(np.mean(np.abs(y))), ((c + 11) / 2.0 + 2.0) * U53 * float(sd)


def gamma(k):
    k = np.asarray(k, dtype=np.float64)
    return k * U53 / (1.0 - k * U53)


# --------------------------------------------------------------------------- the measures
def _worst(err, scale, n, rows=None):
    """max over j <= i < rows of |err| / scale -> (rho, (i, j))"""
    rows = n if rows is None else rows
    if rows <= 0:
        return 0.0, (0, 0)
    tri = np.tril(np.ones((rows, rows), dtype=bool))
    with np.errstate(divide="ignore", invalid="ignore"):
        q = np.where(tri, np.abs(err[:rows, :rows]).astype(np.float64) / scale[:rows, :rows], 0.0)
    q = np.where(np.isnan(q), np.inf, q)           # (0 / 0, or a fit that broke down: never a pass)
    at = np.unravel_index(int(np.argmax(q)), q.shape)
    return float(q[at]), (int(at[0]), int(at[1]))


def _tri_abt(Am, Bm, bs=128):
    """the lower triangle (by bs-blocks) of A B^T for B lower triangular: k <= j only,
    a third of the full product's work in longdouble (numpy has no BLAS for it)"""
    n = Bm.shape[0]
    R = np.zeros((Am.shape[0], n), dtype=LD)
    for j0 in range(0, n, bs):
        j1 = min(j0 + bs, n)
        R[j0:, j0:j1] = Am[j0:, :j1] @ Bm[j0:j1, :j1].T
    return R


def m_chol(L, z, n, rows=None):
    L = np.asarray(L)[:n, :n]
    rows = n if rows is None else min(rows, n)
    Ll = L[:rows, :rows].astype(LD)
    scale = U53 * (np.abs(L) @ np.abs(L).T + z["eps"] * np.abs(z["K_ext"]).astype(np.float64))
    return _worst(_tri_abt(Ll, Ll) - z["K_ext"][:rows, :rows], scale, n, rows)


def m_inv(L, X, z, n):
    L, X = np.asarray(L)[:n, :n], np.asarray(X)[:n, :n]
    scale = U53 * (np.abs(X) @ np.abs(L) @ np.abs(X))
    return _worst(X.astype(LD) - inv_lower(L), scale, n)


def m_white(X, z, n):
    X = np.asarray(X)[:n, :n]
    Xl = X.astype(LD)
    Lr = np.linalg.cholesky(z["K_ext"].astype(np.float64))
    M = np.abs(X) @ np.abs(Lr)
    scale = U53 * (M @ M.T + np.abs(X) @ (z["eps"] * np.abs(z["K_ext"]).astype(np.float64)) @ np.abs(X).T)
    W = np.zeros((n, n), dtype=LD)
    for i0 in range(0, n, 128):                    # X^ is lower triangular: k <= i only
        i1 = min(i0 + 128, n)
        W[i0:i1] = Xl[i0:i1, :i1] @ z["K_ext"][:i1]
    return _worst(_tri_abt(W, Xl) - np.eye(n, dtype=LD), scale, n)


def _ratio(err, scale):
    """err / scale, 0 where both are 0 (an exact zero meets a zero bound), inf for an error against a zero bound"""
    err = np.abs(err).astype(np.float64)
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.where(err == 0.0, 0.0, err / scale)


def m_beta(beta, X, ys, n):
    X, ys = np.asarray(X)[:n, :n], np.asarray(ys)[:n]
    ref = X.astype(LD) @ ys.astype(LD)
    scale = gamma(np.arange(n) + 1) * (np.abs(X) @ np.abs(ys))
    q = _ratio(np.asarray(beta)[:n].astype(LD) - ref, scale)
    return float(np.max(q)), int(np.argmax(q))


def m_alpha(alpha, X, beta, n):
    X, beta = np.asarray(X)[:n, :n], np.asarray(beta)[:n]
    ref = X.T.astype(LD) @ beta.astype(LD)
    scale = gamma(n - np.arange(n)) * (np.abs(X).T @ np.abs(beta))
    q = _ratio(np.asarray(alpha)[:n].astype(LD) - ref, scale)
    return float(np.max(q)), int(np.argmax(q))


def m_ys(ys, z, n):
    q = np.abs(np.asarray(ys)[:n].astype(LD) - z["ys_ref"]).astype(np.float64) / ys_bound(z["y"], z["ys_ref"], z["sd"])
    return float(np.max(q)), int(np.argmax(q))


def measures_of(c):
    """the measures a case is held to: a chain's appended rows of gp_K are not L's, so it
    has no inv, and chol only over the rows before the first appended block row"""
    if "steps" not in c:
        return MEASURES
    return ("chol", "white") if CHAIN_L_ROWS[c["n0"]] > 0 else ("white",)


def measure(which, fit, z, n, l_rows=None):
    """one of MEASURES of a fit (dict L, X) -> (rho, (i, j))"""
    if not (np.all(np.isfinite(fit["L"][:n, :n])) and np.all(np.isfinite(fit["X"][:n, :n]))):
        return np.inf, (0, 0)                      # a fit that broke down
    if which == "chol":
        return m_chol(fit["L"], z, n, l_rows)
    if which == "inv":
        return m_inv(fit["L"], fit["X"], z, n)
    return m_white(fit["X"], z, n)


def line(c, rho_a, rho_b):
    """the pass line of rho_dev given the two references' rho"""
    ref = FACTOR * max(rho_a, rho_b)
    return ref if c["n"] > 64 else max(ref, 1.0)


def cap(c):
    return c["n"] + c["d"] + 8


# --------------------------------------------------------------------------- fp64 route (a): LAPACK
def kmat64(X, ell, sf2, diag, npad=None):
    """k_gp_prep_train + k_gp_kmat in numpy: the Gram form, identity padding"""
    n, d = X.shape
    npad = n if npad is None else npad
    Xs = X * (1.0 / np.asarray(ell, dtype=np.float64))[None, :]
    xn = np.zeros(n)
    for k in range(d):
        xn += Xs[:, k] * Xs[:, k]
    d2 = np.maximum(xn[:, None] + xn[None, :] - 2.0 * (Xs @ Xs.T), 0.0)
    K = np.eye(npad)
    K[:n, :n] = sf2 * np.exp(-0.5 * d2)
    K[np.arange(n), np.arange(n)] += diag
    return K


def lapack(c, z):
    K = kmat64(z["X"], z["ell"], c["sf2"], z["diag"])
    L = np.linalg.cholesky(K)
    try:
        from scipy.linalg import solve_triangular
        X = solve_triangular(L, np.eye(c["n"]), lower=True)
    except ImportError:
        X = inv_lower(L, np.float64)
    return dict(L=L, X=np.tril(X))


# --------------------------------------------------------------------------- fp64 route (b): the restatement
def chol_diag(a):
    """chol_diag_core on one 64 x 64 block -> (L, inv(L)): reciprocal pivots, the
    rank-1 updates, then the substitution L X = I with x_s = acc_s (1 / piv_s)"""
    a = a.copy()
    for c in range(NB):
        piv = math.sqrt(a[c, c]) if a[c, c] > 0.0 else math.sqrt(1e-300)
        l = a[:, c] * (1.0 / piv)
        l[:c + 1] = 0.0
        a[c + 1:, c] = l[c + 1:]
        a[c, c] = piv
        keep = a[:, c].copy()
        a -= np.outer(l, l)
        a[:, c] = keep
    L = np.tril(a)
    invd = 1.0 / np.diag(L)
    b = np.eye(NB)
    for s in range(NB):
        lrs = L[:, s].copy()
        lrs[:s + 1] = 0.0
        b -= np.outer(lrs, b[s] * invd[s])
    return L, np.tril(b * invd[:, None])


def _drop(Am, Bm, k0):
    """A B^T of two 64-row operands without the 16-k chunk at k0"""
    keep = np.ones(Am.shape[1], dtype=bool)
    keep[k0:k0 + 16] = False
    return Am[:, keep] @ Bm[:, keep].T


def refit(K, mutant=None):
    """the refit's factor and inverse of padded K [npad][npad] -> (L, Li)"""
    npad = K.shape[0]
    nb = npad // NB
    Kw = K.copy()
    Li = np.zeros((npad, npad))
    for kb in range(nb):
        o = kb * NB
        Kw[o:o + NB, o:o + NB], Li[o:o + NB, o:o + NB] = chol_diag(Kw[o:o + NB, o:o + NB])
        if kb + 1 == nb:
            break
        Kw[o + NB:, o:o + NB] = Kw[o + NB:, o:o + NB] @ Li[o:o + NB, o:o + NB].T          # k_chol_rows
        P = Kw[o + NB:, o:o + NB]
        upd = P @ P.T                                                                      # k_chol_update
        if mutant == "upd_chunk" and kb == 0:
            upd[:NB, :NB] = _drop(P[:NB], P[:NB], 0)
        Kw[o + NB:, o + NB:] -= upd
    L = np.tril(Kw)
    for s, pairs, _, _ in levels(npad):                                                    # k_trinv_level / _big
        for zp in range(pairs):
            o = zp * 2 * s
            s2 = min(s, npad - o - s)
            Bm, Ai = L[o + s:o + s + s2, o:o + s], Li[o:o + s, o:o + s]
            T = Bm @ Ai
            if mutant == "dbl_chunk" and s == NB and zp == 0:
                keep = np.ones(s, dtype=bool)
                keep[:16] = False
                T[:, :NB] = Bm[:, keep] @ Ai[keep, :NB]
            if mutant == "ragged_k" and s2 < s:
                T = Bm[:, :s2] @ Ai[:s2]
            Li[o + s:o + s + s2, o:o + s] = -(Li[o + s:o + s + s2, o + s:o + s + s2] @ T)
    return L, Li


def _chunked(Am, Bm, klo, khi):
    """sum over APP_KC chunks from klo, in chunk order, of A[:, chunk] B[:, chunk]^T"""
    s = np.zeros((Am.shape[0], Bm.shape[0]))
    for k0 in range(klo, khi, APP_KC):
        k1 = min(k0 + APP_KC, khi)
        s = s + Am[:, k0:k1] @ Bm[:, k0:k1].T
    return s


def append(K, L, Li, n0, n, mutant=None, prev=None):
    """block rows n0 // 64 .. (n - 1) // 64 appended to (L, Li) in place; K the new padded
    kernel matrix.  L's appended rows keep only their diagonal blocks, as gp_K does.
    prev: the inverse before the previous block's append (mutant app_stale) -> that of this call's last block"""
    b0, b1 = n0 // NB, (n - 1) // NB
    for b in range(b0, b1 + 1):
        o = b * NB
        before = Li.copy()
        K22 = K[o:o + NB, o:o + NB].copy()
        Bm = np.zeros((NB, o))
        if b > 0:
            for cb in range(b):                                                            # MODE 0
                Bm[:, cb * NB:cb * NB + NB] = _chunked(K[o:o + NB, :o], Li[cb * NB:cb * NB + NB, :o], 0,
                                                       cb * NB + NB)
            K22 -= _chunked(Bm, Bm, 0, o)                                                  # MODE 1
        D, Di = chol_diag(K22)
        L[o:o + NB, :] = 0.0
        L[o:o + NB, o:o + NB] = D
        Li[o:o + NB, :] = 0.0
        Li[o:o + NB, o:o + NB] = Di
        if b > 0:
            src = prev if (mutant == "app_stale" and prev is not None) else Li
            E = np.zeros((NB, o))
            for cb in range(b):                                                            # MODE 2
                E[:, cb * NB:cb * NB + NB] = _chunked(Bm, src[:o, cb * NB:cb * NB + NB].T, cb * NB, o)
            Li[o:o + NB, :o] = -(Di @ E)                                                   # k_app_c
        prev = before
    return prev


def restate(c, z, mutant=None):
    """gp_fit.hip in numpy -> dict L, X [npad][npad], l_rows; a chain case runs its
    refit at n0 and then every append"""
    with np.errstate(over="ignore", invalid="ignore"):     # (a mutant's fit may break down)
        return _restate(c, z, mutant)


def _restate(c, z, mutant):
    assert mutant is None or mutant in MUTANTS
    diag = c["sn2"] if mutant == "no_jitter" else z["diag"]
    n, npad = c["n"], npad_of(c["n"])
    n0 = c.get("n0", n)
    assert npad_of(n0) == npad
    inner = mutant if mutant in ("upd_chunk", "dbl_chunk", "ragged_k") else None
    L, Li = refit(kmat64(z["X"][:n0], z["ell"], c["sf2"], diag, npad), inner)
    l_rows, at, prev = npad, n0, None
    for s in c.get("steps", ()):
        K = kmat64(z["X"][:at + s], z["ell"], c["sf2"], diag, npad)
        l_rows = min(l_rows, at // NB * NB)
        prev = append(K, L, Li, at, at + s, mutant, prev)
        at += s
    if mutant in ("l_tile_f32", "x_tile_f32"):
        Mx = L if mutant == "l_tile_f32" else Li
        i0 = min((n - 16) // 16 * 16, (l_rows - 16) if mutant == "l_tile_f32" else npad)
        Mx[i0:i0 + 16, 16:32] = Mx[i0:i0 + 16, 16:32].astype(np.float32)
    return dict(L=L, X=Li, l_rows=l_rows)


def applies(mutant, c):
    """whether the mutant changes anything on this case"""
    if not c["tight"]:
        return False
    chain = "steps" in c
    if mutant == "app_stale":
        return chain and (c["n"] - 1) // NB > c["n0"] // NB
    if mutant == "ragged_k":   # (a chain's appends rewrite the rows from l_rows on)
        keep = CHAIN_L_ROWS[c["n0"]] if chain else npad_of(c["n"])
        return any(s2 < s and s < keep for s, _, s2, _ in levels(npad_of(c["n"])))
    if chain and mutant == "dbl_chunk":
        return CHAIN_L_ROWS[c["n0"]] >= 2 * NB
    if chain and mutant == "l_tile_f32":
        return CHAIN_L_ROWS[c["n0"]] >= 64
    return True


def mutant_measure(mutant, c):
    """the measure that must catch it: a chain's appended rows of gp_K are not L's, so
    there only white sees the whole inverse"""
    if "steps" in c and mutant != "l_tile_f32":
        return "white"
    return MUTANTS[mutant]


_REF = {}


def references(c, z):
    """-> {measure: (rho_lapack, rho_restate)}, the restatement's l_rows; cached per case"""
    if c["name"] not in _REF:
        a, b = lapack(c, z), restate(c, z)
        _REF[c["name"]] = ({m: (measure(m, a, z, c["n"], b["l_rows"] if m == "chol" else None)[0],
                                measure(m, b, z, c["n"], b["l_rows"] if m == "chol" else None)[0])
                            for m in measures_of(c)}, b["l_rows"])
    return _REF[c["name"]]


# --------------------------------------------------------------------------- the int8 planes, exactly
def i8_row_exp(mx):
    """k_split_i8's ea: ilogb(mx / 0.49) + 1 for mx > 0, else 0"""
    return math.frexp(mx / 0.49)[1] if mx > 0.0 else 0


def i8_expected(X, n, eb):
    """what k_split_i8 must leave for L^-1 = X [npad][npad] with n live rows:
    -> (ea [npad], rs [npad], N [npad][npad] the 48-bit integers rint(X_rk 2^(48 - ea_r)),
    k <= r < n, else 0, e2 [npad])"""
    npad = X.shape[0]
    low = np.tril(np.ones((npad, npad), dtype=bool)) & (np.arange(npad) < n)[:, None]
    Xl = np.where(low, X, 0.0)
    mx = np.max(np.abs(Xl), axis=1)
    ea = np.array([i8_row_exp(float(v)) for v in mx], dtype=np.int64)
    live = (np.arange(npad) < n) & (mx > 0.0)
    rs = np.where(live, np.ldexp(1.0, ea + eb), 0.0)
    N = np.rint(np.ldexp(Xl, (48 - ea)[:, None]))
    kend = np.where(np.arange(npad) < n, np.arange(npad) + 1, 0).astype(np.float64)
    e = kend * I8_C * rs
    return ea, rs, N, e * e


def i8_split_restated(row, kend, eb):
    """i8_biased / k_split_i8 on one row, bit for bit: the biased word of
    fl(x 2^-ea + 24.50196...), its low 48 bits as six bytes each XOR 0x80, and the
    balanced digits' value -> (ea, rs, digits [6][len(row)] int, N [len(row)] int, e2)"""
    row = np.asarray(row, dtype=np.float64)
    mx = float(np.max(np.abs(row[:kend]), initial=0.0))
    ea = i8_row_exp(mx)
    v = np.where(np.arange(len(row)) < kend, row, 0.0)
    bias = float.fromhex("0x1.8808080808080p4")
    w = (np.ldexp(v, -ea) + bias).view(np.uint64) & np.uint64((1 << 48) - 1)
    dg = []
    for p in range(6):                      # plane 0 = byte 5, the most significant
        byte = ((w >> np.uint64(8 * (5 - p))) & np.uint64(255)).astype(np.int64) ^ 0x80
        dg.append(np.where(byte >= 128, byte - 256, byte))
    N = np.zeros(len(row), dtype=np.int64)
    for p in range(6):
        N = N * 256 + dg[p]
    live = kend > 0 and mx > 0.0
    rs = math.ldexp(1.0, ea + eb) if live else 0.0
    e = float(kend) * I8_C * rs
    return ea, rs, np.array(dg), N, e * e


def blk(i, j):
    return "(%d, %d) in 64-block (%d, %d)" % (i, j, i // NB, j // NB)
