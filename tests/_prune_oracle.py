"""Test infrastructure: the selection-exact pruned top-k (include/uthot.h
ut_gp_topk_pruned) restated in numpy fp64 over oracle/gp.py's GP, and the one
table of cases that the CPU and the GPU tests of it share.  The checker and
never the product.

  V       = L^-1 k*                         (one column per candidate)
  var     = max(sf2 - |V|^2, 0)
  var_ub  = max(sf2 - |V[:R]|^2, 0)         R = bound_rows rounded up to a multiple
                                            of 128, clipped to [128, npad]
  bound   = acq(mu, var_ub) (+ 1e-12 relative, the acquisition's own rounding);
            -inf on a duplicate
  set     = the 1024 (or m) best (bound, -index) among the valid candidates
  tau     = the k-th best exact score of the set; -inf if it has fewer than k
  keep    = bound >= tau
  dense   = 2 |keep| > m                    (then every candidate is scored)
  select  = the k best (score, -index) of the kept valid candidates

|V|^2 is summed as |V[:R]|^2 + |V[R:]|^2, so var <= var_ub holds in floating
point as it does on the device; test_prune_oracle_cpu.py checks this posterior
against oracle.gp.GP.posterior.
"""
import numpy as np
from scipy.linalg import solve_triangular
from scipy.special import erfc

from _ard_cases import ell_vector
from oracle import gp as ogp

NPAD = 128   # the device's row tile (gp_npad)
TSET = 1024  # the threshold set


def npad(n):
    return (int(n) + NPAD - 1) // NPAD * NPAD


def bound_rows_used(n, bound_rows):
    """R in rows: gp_npad(bound_rows) clipped to [128, npad(n)] (= stats.bound_rows)"""
    return min(max(npad(bound_rows), NPAD), npad(n))


def posterior(gp, U, rows):
    """-> mu, var, var_ub (the first `rows` rows of L^-1 k*) of U [m][d].  Equal
    candidates are computed once: a BLAS product need not give equal columns
    the same bits, and the ties of a repeated candidate are part of the cases"""
    Uu, inv = np.unique(np.asarray(U, dtype=np.float64), axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    Us = Uu * gp.inv_ell
    Ks = gp.sf2 * np.exp(-0.5 * ogp.sqdist(Us, gp.Xs))
    V = solve_triangular(gp.L, Ks.T, lower=True)
    s_r = np.sum(V[:rows] * V[:rows], axis=0)
    s_all = s_r + np.sum(V[rows:] * V[rows:], axis=0)
    return (Ks @ gp.alpha)[inv], np.maximum(gp.sf2 - s_all, 0.0)[inv], np.maximum(gp.sf2 - s_r, 0.0)[inv]


def rank(score, valid, k):
    """sorted(valid, key=(-score, index))[:k]"""
    v = np.flatnonzero(valid)
    return v[np.lexsort((v, -score[v]))][:k]


def restate(gp, U, acq, k, bound_rows, dup=None):
    """the pruned selection -> dict: score, bound [m] (-inf on duplicates), rows,
    tau, keep [m], dense, sel (positions, best first; at most k)"""
    m = len(U)
    rows = bound_rows_used(gp.Xs.shape[0], bound_rows)
    mu, var, var_ub = posterior(gp, U, rows)
    kw = dict(kind=acq["kind"], xi=acq["xi"], kappa=acq["kappa"])
    valid = np.ones(m, dtype=bool) if dup is None else np.asarray(dup) == 0
    score = ogp.acquisition(mu, var, gp.f_best, **kw)
    bound = ogp.acquisition(mu, var_ub, gp.f_best, **kw)
    bound = bound + np.abs(bound) * 1e-12 + 1e-300
    score = np.where(valid, score, -np.inf)
    bound = np.where(valid, bound, -np.inf)
    tset = rank(bound, valid, min(m, TSET))
    best = tset[np.lexsort((tset, -score[tset]))]
    tau = score[best[k - 1]] if len(best) >= k else -np.inf
    keep = bound >= tau
    dense = 2 * int(keep.sum()) > m
    sel = rank(score, valid if dense else valid & keep, k)
    return dict(mu=mu, var=var, score=score, bound=bound, rows=rows, tau=tau, keep=keep, dense=dense, sel=sel,
                valid=valid)


# --------------------------------------------------------------------------- the cases
# regime: "prunes" (the restated survivors are in (0, m / 4]), "dense" (more than
# m / 2 survive: the device falls back to the dense variance), "flat" (every valid
# score is the same double), "few_valid" (fewer valid candidates than k).
# sn2 and jitter are given relative to sf2 (tests/test_gpu_kstar_q.py's scaling).
# recipe: "cube"    X uniform in the unit cube, half the candidates uniform and half
#                   training points + N(0, 0.05^2) clipped, y = sum (x - 0.3)^2 + 0.05 N
#         "worst"   the same fit; every candidate next to one of the 10 worst
#                   (largest y) training points, + N(0, 0.02^2)
#         "late"    the same fit; every candidate a training point of the second half
#                   of the rows + N(0, 0.05^2) clipped
#         "repeat"  the same fit; one uniform candidate m times
#         "outlier" "cube" with candidates 3, 500, ... (OUTLIERS) at 40.0 in every feature
# dup: "none", "every97", "all_but_10" (only 7, 207, ... are valid), "all"
# The device's survivors, measured on an MI355X, as pass 32 / pass 64 (restated);
# "dense": the call fell back.  Pass 64 keeps exactly the restated set everywhere.
# The f32 pass is as tight on EI, but on the UCB cases of the d = 6, sn2 = 1e-6 fit
# (sum |alpha| ~ 3e5, so its mean widening dmu is ~1.5 against scores ~2 apart) it
# keeps 41-46 % of the batch, just short of the dense fallback.
#   d64_l2 223 / 215 (215), d64_l05 398 / 396 (396), d6_l008 224 / 222 (222), d112_l3 80 / 74 (74),
#   d16_k1 1 / 1 (1), d3_n129 17 / 17 (17), d1_n128 17 / 17 (17), ucb_k2 2133 / 111 (111),
#   ucb_k0 2178 / 64 (64), d64_sf2_37 588 / 573 (573), d64_sf2_1e-3 68 / 66 (66), d6_sf2_1e-3 2295 / 66 (66),
#   d64_noisy 215 / 208 (208), d64_noisy_sf2_37 508 / 498 (498), d64_xi 207 / 202 (202),
#   ucb_sf2_37 2035 / 121 (121), rows_n 32 / 32 (32), rows_10n 64 / 64 (64), m255 1 / 1 (1), m257 17 / 17 (17),
#   m1 dense / dense (1), late_sf2_37 dense / dense (4599), late_sf2_37_xi dense / dense (4559),
#   late_sf2_37_noisy dense / dense (4546), late_d64 dense / dense (4948), k1024 dense / dense (3260),
#   flat_ei0 dense / dense (4948), flat_repeat dense / dense (2000), few_a_ucb dense / dense (10),
#   few_b_ucb dense / dense (2000), few_c_ucb dense / dense (2000), few_a_ei dense / dense (10),
#   few_b_ei dense / dense (2000), outlier 36 / 28 (28)
# One lengthscale per feature (the ard_* cases): the f32 pass stays within 5 % of the restated set.
#   ard_d64_ei 644 / 622 (622), ard_d64_ucb 290 / 279 (279), ard_d33_short_sf2_37 366 / 350 (350),
#   ard_d33_late dense / dense (4672)
OUTLIERS = (3, 500, 501, 777, 1024, 1500, 1998, 1999)


def _c(name, regime, d, n, ell, m, k, bound_rows, kind="ei", xi=0.0, kappa=2.0, sf2=1.0, sn2=1e-6, jitter=1e-8,
       dup="every97", cand_base=0, recipe="cube", seed=0):
    return dict(name=name, regime=regime, d=d, n=n, ell=ell, sf2=sf2, sn2=sn2 * sf2, jitter=jitter * sf2,
                acq=dict(kind=kind, xi=xi, kappa=kappa), m=m, k=k, bound_rows=bound_rows, dup=dup,
                cand_base=cand_base, recipe=recipe, seed=seed)


CASES = [
    # -- the recipes that prune
    _c("d64_l2", "prunes", 64, 1000, 2.0, 5000, 64, 256),
    _c("d64_l05", "prunes", 64, 1000, 0.5, 4097, 64, 256, seed=1),
    _c("d6_l008", "prunes", 6, 640, 0.08, 5000, 64, 256, seed=2),           # most k* below 2^-126
    _c("d112_l3", "prunes", 112, 1024, 3.0, 3000, 32, 384, seed=3),
    _c("d16_k1", "prunes", 16, 512, 1.0, 5000, 1, 256, cand_base=2 ** 40, seed=4),
    _c("d3_n129", "prunes", 3, 129, 0.3, 1025, 17, 1, seed=5),             # one real row in the second tile
    # (d = 1, 128 points: every EI underflows, so UCB; a noisy fit, or sum |alpha| ~ 1e7
    # puts the mean's own rounding above the path tolerance) R = RT: every bound exact, no f32 tile
    _c("d1_n128", "prunes", 1, 128, 0.1, 1023, 17, 128, kind="ucb", kappa=2.0, sn2=1e-2, seed=6),
    _c("ucb_k2", "prunes", 6, 640, 0.6, 5000, 64, 256, kind="ucb", kappa=2.0, seed=7),
    _c("ucb_k0", "prunes", 6, 640, 0.6, 5000, 64, 256, kind="ucb", kappa=0.0, seed=8),   # the score ignores sigma
    # -- scales on a recipe that prunes (sf2 = 1e-3 against a standardised y: every
    # EI underflows, so that scale is UCB)
    _c("d64_sf2_37", "prunes", 64, 1000, 2.0, 5000, 64, 256, sf2=37.0, seed=9),
    _c("d64_sf2_1e-3", "prunes", 64, 1000, 2.0, 5000, 64, 256, kind="ucb", kappa=2.0, sf2=1e-3, seed=10),
    _c("d6_sf2_1e-3", "prunes", 6, 640, 0.6, 5000, 64, 256, kind="ucb", kappa=2.0, sf2=1e-3, seed=10),
    _c("d64_noisy", "prunes", 64, 1000, 2.0, 5000, 64, 256, sn2=1e-2, seed=11),
    _c("d64_noisy_sf2_37", "prunes", 64, 1000, 2.0, 5000, 64, 256, sf2=37.0, sn2=1e-2, seed=12),
    _c("d64_xi", "prunes", 64, 1000, 2.0, 5000, 64, 256, xi=0.1, seed=13),
    _c("ucb_sf2_37", "prunes", 6, 640, 0.6, 5000, 17, 256, kind="ucb", kappa=2.0, sf2=37.0, seed=14),
    # -- bound_rows against n
    _c("rows_n", "prunes", 64, 1000, 2.0, 2000, 32, 1000, seed=15),         # R = RT at n no multiple of 128
    _c("rows_10n", "prunes", 64, 1000, 2.0, 2000, 64, 10000, seed=16),
    # -- batch shapes
    _c("m255", "prunes", 16, 512, 1.0, 255, 1, 256, seed=17),
    _c("m257", "prunes", 3, 129, 0.3, 257, 17, 128, seed=18),
    _c("m1", "dense", 6, 640, 0.6, 1, 1, 256, kind="ucb", kappa=2.0, dup="none", seed=50),
    # -- the recipes that fall back to dense: candidates next to the later training
    # rows, which the first 128 rows of L^-1 k* say little about
    _c("late_sf2_37", "dense", 6, 640, 0.3, 5000, 16, 128, sf2=37.0, recipe="late", seed=40),
    _c("late_sf2_37_xi", "dense", 6, 640, 0.3, 5000, 16, 128, sf2=37.0, xi=0.1, recipe="late", seed=41),
    _c("late_sf2_37_noisy", "dense", 6, 640, 0.3, 5000, 16, 128, sf2=37.0, sn2=1e-2, recipe="late", seed=42),
    _c("late_d64", "dense", 64, 1000, 2.0, 5000, 16, 128, sf2=37.0, recipe="late", seed=40),
    _c("k1024", "dense", 64, 1000, 2.0, 5000, 1024, 256, kind="ucb", kappa=2.0, seed=24),
    # -- ties
    # every EI exactly 0 by underflow (a long lengthscale and xi = 1: z << -38)
    _c("flat_ei0", "flat", 6, 640, 3.0, 5000, 64, 256, xi=1.0, cand_base=7, seed=25),
    _c("flat_repeat", "flat", 16, 512, 1.0, 2000, 16, 128, dup="none", recipe="repeat", seed=26),
    # -- fewer valid candidates than k, most scores negative
    _c("few_a_ucb", "few_valid", 6, 640, 0.6, 10, 16, 256, kind="ucb", kappa=0.5, dup="none", recipe="worst",
       seed=27),
    _c("few_b_ucb", "few_valid", 6, 640, 0.6, 2000, 16, 256, kind="ucb", kappa=0.5, dup="all_but_10",
       recipe="worst", cand_base=100, seed=28),
    _c("few_c_ucb", "few_valid", 6, 640, 0.6, 2000, 16, 256, kind="ucb", kappa=0.5, dup="all", recipe="worst",
       seed=29),
    _c("few_a_ei", "few_valid", 6, 640, 0.6, 10, 16, 256, dup="none", recipe="worst", seed=27),
    _c("few_b_ei", "few_valid", 6, 640, 0.6, 2000, 16, 256, dup="all_but_10", recipe="worst", seed=28),
    # -- candidates the f32 pass cannot bound (rho >= 1/2)
    _c("outlier", "prunes", 16, 256, 0.1, 2000, 16, 128, dup="none", recipe="outlier", seed=30),
    # -- one lengthscale per feature (tests/_ard_cases.py): the f32 pass widens each bound
    # by roundings derived from the |x / ell| norms, which a scalar ell scales as one
    _c("ard_d64_ei", "prunes", 64, 1000, ell_vector("spread", 64), 5000, 64, 256, seed=60),
    _c("ard_d64_ucb", "prunes", 64, 1000, ell_vector("spread", 64), 5000, 64, 256, kind="ucb", kappa=2.0, seed=61),
    _c("ard_d33_short_sf2_37", "prunes", 33, 600, ell_vector("one_short_last", 33, 2.0), 5000, 64, 256, sf2=37.0,
       seed=62),
    _c("ard_d33_late", "dense", 33, 600, ell_vector("spread", 33), 5000, 16, 128, sf2=37.0, recipe="late", seed=63),
]


def case_ids():
    return [c["name"] for c in CASES]


_DATA = {}


def case_data(c):
    """-> dict X [n][d], y [n], U [m][d], dup [m] uint8, gp (oracle GP); cached, never written to"""
    if c["name"] in _DATA:
        return _DATA[c["name"]]
    rng = np.random.default_rng(9000 + c["seed"])
    n, d, m = c["n"], c["d"], c["m"]
    X = rng.uniform(size=(n, d))
    y = np.sum((X - 0.3) ** 2, axis=1) + 0.05 * rng.standard_normal(n)
    if c["recipe"] in ("cube", "outlier"):
        h = m // 2
        near = X[rng.integers(0, n, size=m - h)] + 0.05 * rng.standard_normal((m - h, d))
        U = np.vstack([rng.uniform(size=(h, d)), np.clip(near, 0.0, 1.0)])
        U = U[rng.permutation(m)]
        if c["recipe"] == "outlier":
            U[list(OUTLIERS)] = 40.0
    elif c["recipe"] == "worst":
        worst = np.argsort(y)[-10:]
        U = np.clip(X[worst[rng.integers(0, 10, size=m)]] + 0.02 * rng.standard_normal((m, d)), 0.0, 1.0)
    elif c["recipe"] == "late":
        U = np.clip(X[rng.integers(n // 2, n, size=m)] + 0.05 * rng.standard_normal((m, d)), 0.0, 1.0)
    elif c["recipe"] == "repeat":
        U = np.repeat(rng.uniform(size=(1, d)), m, axis=0)
    else:
        raise ValueError(c["recipe"])
    dup = np.zeros(m, dtype=np.uint8)
    if c["dup"] == "every97":
        dup[::97] = 1
    elif c["dup"] == "all_but_10":
        dup[:] = 1
        dup[7::200] = 0
    elif c["dup"] == "all":
        dup[:] = 1
    elif c["dup"] != "none":
        raise ValueError(c["dup"])
    gp = ogp.GP(X, y, lengthscale=c["ell"], sigma_f2=c["sf2"], sigma_n2=c["sn2"], jitter=c["jitter"])
    for a in (X, y, U, dup):
        a.setflags(write=False)
    _DATA[c["name"]] = dict(X=X, y=y, U=U, dup=dup, gp=gp)
    return _DATA[c["name"]]


_REST = {}


def case_restated(c):
    """restate() of the case, cached"""
    if c["name"] not in _REST:
        z = case_data(c)
        _REST[c["name"]] = restate(z["gp"], z["U"], c["acq"], c["k"], c["bound_rows"], z["dup"])
    return _REST[c["name"]]


# --------------------------------------------------------------------------- shared checks
# how far two evaluations of one posterior may be apart: (rtol, atol) on the
# mean, (rtol, atol / sf2) on the variance
PATH_TOL = (1e-9, 1e-10, 1e-9, 1e-10)     # two device paths (tests/test_gpu_kstar_q.py)
ORACLE_TOL = (1e-5, 1e-9, 1e-5, 1e-8)     # the device against oracle/gp.py (the north star's fp64 tier)


def envelope(mu, var, f_best, acq, sf2, tol, upper=False):
    """the smallest (upper: largest) score of a posterior within tol of (mu, var):
    EI and UCB (kappa >= 0) fall with the mean and rise with the variance"""
    s = -1.0 if upper else 1.0
    mu = mu + s * (tol[0] * np.abs(mu) + tol[1])
    var = np.maximum(var * (1.0 - s * tol[2]) - s * tol[3] * sf2, 0.0)
    out = ogp.acquisition(mu, var, f_best, kind=acq["kind"], xi=acq["xi"], kappa=acq["kappa"])
    if acq["kind"] == "ei" and not upper:
        # scipy's erfc gives 0 where its result would be subnormal (z < -37.6), and
        # oracle.gp's EI = I Phi + sigma phi is then sigma phi, up to z^2 ~ 1400
        # times the EI (rows_n: 1.3e-313 for 9.36e-317, which the device and a
        # 60-digit evaluation both give).  There the reference only says EI >= 0.
        sigma = np.sqrt(var)
        with np.errstate(divide="ignore", invalid="ignore"):
            z = np.where(sigma > 0.0, (f_best - mu - acq["xi"]) / np.where(sigma > 0.0, sigma, 1.0), 0.0)
        out = np.where((sigma > 0.0) & (erfc(-z / np.sqrt(2.0)) < np.finfo(np.float64).tiny), 0.0, out)
    return out


def band_check(idx, top, ref, valid, k, cand_base, band_rel, band_abs):
    """the selection as a band check against reference scores ref [m]: exactly
    kk = min(k, valid) distinct indices then -1, every returned candidate within
    the band of the kk-th best reference score t, every candidate above t + band
    returned, scores non-increasing with bitwise-equal neighbours in index order"""
    idx, top = np.asarray(idx), np.asarray(top)
    valid = np.asarray(valid, dtype=bool)
    kk = min(k, int(valid.sum()))
    assert len(idx) == k
    assert np.all(idx[:kk] >= 0) and np.all(idx[kk:] == -1), idx
    pos = idx[:kk] - cand_base
    assert len(set(pos.tolist())) == kk and np.all((pos >= 0) & (pos < len(ref))), idx
    assert np.all(valid[pos]), "an invalid candidate was selected"
    if kk == 0:
        return
    t = np.sort(ref[valid])[::-1][kk - 1]
    band = band_rel * abs(t) + band_abs
    assert np.all(ref[pos] >= t - band), (ref[pos].min(), t, band)
    must = np.flatnonzero(valid & (ref > t + band))
    assert set(must.tolist()) <= set(pos.tolist()), sorted(set(must.tolist()) - set(pos.tolist()))
    s = top[:kk]
    assert np.all(s[:-1] >= s[1:]), "scores not sorted"
    tie = s[:-1] == s[1:]
    assert np.all(idx[:kk][:-1][tie] < idx[:kk][1:][tie]), "equal scores out of index order"
