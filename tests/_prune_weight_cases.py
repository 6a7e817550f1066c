"""Test infrastructure: the weighted pruned top-k (include/uthot.h
ut_gp_set_prune_weighted) restated in numpy fp64 over tests/_prune_oracle.py
(the fit, the candidates, the posterior and its first-rows bound),
tests/_cons_oracle.py (ConsGP) and tests/_feas_oracle.py (feas_prob), and the
one table of cases that the CPU and the GPU tests of it share.  The checker and
never the product.

  S       = (E P) p^gamma            E = EI(mu, var; f_best_c, xi), 1 with no feasible row
                                     P = prod_j Phi((tau_j - mu_cj) / sigma)   (_cons_oracle.cons_prob)
                                     p = the feasibility vote                  (_feas_oracle.feas_prob)
  bound   = E(var_ub) prod_j Pub_j   Pub_j = 1 where tau_j - mu_cj >= 0,
                                     else Phi((tau_j - mu_cj) / sqrt(var_ub)), 0 at var_ub == 0
            (+ 1e-12 relative + 1e-300 after the product; the vote gets no bound)
  set, tau, keep, dense, select      as _prune_oracle.restate, on S and this bound

Every case is a _prune_oracle case (by name: its fit, candidates, duplicates, k,
bound rows and acquisition) with constraint columns, thresholds, failed rows and
vote parameters added, and the regime the weighted call is in."""
import numpy as np
from scipy.special import erfc

import _prune_oracle as po
from _cons_oracle import ConsGP, cons_prob
from _feas_oracle import feas_prob
from oracle import gp as ogp

TINY = np.finfo(np.float64).tiny


def Phi(z):
    return 0.5 * erfc(-np.asarray(z, dtype=np.float64) * 0.70710678118654752440)


# --------------------------------------------------------------------------- the cases
# base: the _prune_oracle case.  thr: one threshold per constraint column (none: no
# values are loaded).  nfail: failed rows (0: none are loaded).  vote: gp_feas_set's
# keywords.  regime: as _prune_oracle's, of the WEIGHTED call.  helps: the EI-only
# bound on the same scores would leave the regime (dense, or more than m / 4).
# The constraint columns, row-aligned with the fit's X (feature indices mod d):
#   c0 = x0 + x1 + 0.02 N    c1 = x2 x3 + 0.02 N    c2 = x4 - x5 + 0.02 N    c3 = x6 + 0.02 N
# The failed rows: training rows drawn with replacement + N(0, 0.05^2), clipped to the cube.
# tie: a declared tie at the oracle band -- the k-th and (k+1)-th scores are closer than
# 1e-5 |t| + 1e-8 (only the device-path band 1e-9 |t| + 1e-12 separates them).
def _w(name, base, thr=(), nfail=0, regime="prunes", helps=False, tie=False, **vote):
    return dict(name=name, base=base, thr=tuple(float(t) for t in thr), nfail=int(nfail), regime=regime,
                helps=helps, tie=tie, vote=vote)


CASES = [
    # -- one constraint, from half the rows feasible to none (the score is then P alone:
    # the EI-only bound falls dense there)
    _w("t1.0", "d64_l2", [1.0]),
    _w("t0.6", "d64_l2", [0.6]),
    _w("t0.35", "d64_l2", [0.35]),
    # (t = -1: S = P ~ 7e-8 around the k-th best, so the oracle band's 1e-8 floor is 14 % of
    # the scores and wider than the 3.5e-9 gap behind the k-th: a declared tie there)
    _w("t-1_nofeas", "d64_l2", [-1.0], helps=True, tie=True),
    # -- two and four constraints
    _w("two", "d64_l2", [0.8, 0.3]),
    _w("four", "d64_l2", [0.9, 0.35, 0.3, 0.7]),
    # -- the vote alone, and with a constraint
    _w("vote_only", "d64_l2", [], 100),
    _w("t0.6_f100", "d64_l2", [0.6], 100),
    # -- short lengthscale (most k* below 2^-126 at pass 32)
    _w("short_f64", "d6_l008", [0.6], 64),
    # -- the bound covers every row (R = RT): every bound is the exact E P, flagged exact
    _w("rows_n_exact", "rows_n", [0.6]),
    # -- tile edges
    _w("n129_f30", "d3_n129", [0.8], 30),
    _w("m257_f30", "m257", [0.8], 30),
    # -- k = 1 at cand_base = 2^40
    _w("k1_f40", "d16_k1", [0.6], 40),
    # -- other regimes
    _w("late_dense", "late_sf2_37", [0.8], regime="dense"),
    _w("flat", "flat_ei0", [0.8], regime="flat"),
    _w("few_f20", "few_b_ei", [0.8], 20, regime="few_valid"),
    # -- one lengthscale per feature
    _w("ard_f100", "ard_d64_ei", [0.6], 100, helps=True),
    # -- vote parameters
    _w("gamma2", "d64_l2", [0.6], 100, power=2.0),
    _w("prior0.7", "d64_l2", [0.6], 100, prior=0.7, strength=3.0),
    _w("ell_scale0.5", "d64_l2", [0.6], 100, ell_scale=0.5),
]


def case_ids():
    return [w["name"] for w in CASES]


def base_case(w):
    return next(c for c in po.CASES if c["name"] == w["base"])


_DATA = {}


def case_data(w):
    """-> dict: the base case's data (X, y, U, dup, gp), C [n][nc] the constraint values,
    thr [nc], Xf [nfail][d] the failed rows (None: none), cg the ConsGP; cached, never written to"""
    if w["name"] in _DATA:
        return _DATA[w["name"]]
    c = base_case(w)
    z = dict(po.case_data(c))
    X = z["X"]
    n, d = X.shape
    rng = np.random.default_rng(5)
    c01 = np.stack([X[:, 0] + X[:, 1 % d] + 0.02 * rng.standard_normal(n),
                    X[:, 2 % d] * X[:, 3 % d] + 0.02 * rng.standard_normal(n)], 1)
    nf = w["nfail"]
    Xf = None
    if nf:
        Xf = np.clip(X[rng.integers(0, n, nf)] + 0.05 * rng.standard_normal((nf, d)), 0.0, 1.0)
        Xf.setflags(write=False)
    c23 = np.stack([X[:, 4 % d] - X[:, 5 % d] + 0.02 * rng.standard_normal(n),
                    X[:, 6 % d] + 0.02 * rng.standard_normal(n)], 1)
    nc = len(w["thr"])
    C = np.ascontiguousarray(np.hstack([c01, c23])[:, :nc])
    C.setflags(write=False)
    thr = np.array(w["thr"], dtype=np.float64)
    cg = ConsGP(X, z["y"], C, thr, c["ell"], sigma_f2=c["sf2"], sigma_n2=c["sn2"], jitter=c["jitter"])
    z.update(C=C, thr=thr, Xf=Xf, cg=cg)
    _DATA[w["name"]] = z
    return z


def vote_params(w):
    """(prior or None, strength, ell_scale, power) of the case"""
    v = w["vote"]
    return v.get("prior"), v.get("strength", 1.0), v.get("ell_scale", 1.0), v.get("power", 1.0)


def _select(score, bound, valid, k, m):
    tset = po.rank(bound, valid, min(m, po.TSET))
    best = tset[np.lexsort((tset, -score[tset]))]
    tau = score[best[k - 1]] if len(best) >= k else -np.inf
    keep = bound >= tau
    dense = 2 * int(keep.sum()) > m
    sel = po.rank(score, valid if dense else valid & keep, k)
    return tau, keep, dense, sel


def restate_weighted(w):
    """-> dict: mu, var, var_ub, mu_c [nc][m], p [m], valid, rows; score, bound, tau, keep,
    dense, sel of the weighted call; bound_e, tau_e, keep_e, dense_e, sel_e of the EI-only
    bound on the same scores (for comparison)"""
    c, z = base_case(w), case_data(w)
    g, U, cg = z["gp"], z["U"], z["cg"]
    m, k, xi = c["m"], c["k"], c["acq"]["xi"]
    assert c["acq"]["kind"] == "ei"
    rows = po.bound_rows_used(len(z["X"]), c["bound_rows"])
    mu, var, var_ub = po.posterior(g, U, rows)
    valid = z["dup"] == 0
    mu_c = cg.mu_c(U)
    prior, strength, ell_scale, power = vote_params(w)
    if w["nfail"]:
        p, _, _ = feas_prob(z["X"], z["Xf"], U, c["ell"], prior=prior, strength=strength, ell_scale=ell_scale)
    else:
        p = np.ones(m)

    def ei(v):
        return ogp.acquisition(mu, v, cg.f_best_c, "ei", xi) if cg.n_feasible else np.ones(m)

    score = (ei(var) * cons_prob(var, mu_c, cg.tau)) * (p if power == 1.0 else p ** power)
    pub = P_ub(var_ub, mu_c, cg.tau)
    out = dict(mu=mu, var=var, var_ub=var_ub, mu_c=mu_c, p=p, valid=valid, rows=rows)
    score = np.where(valid, score, -np.inf)
    for tag, b in (("", ei(var_ub) * pub), ("_e", ei(var_ub))):
        b = b + np.abs(b) * 1e-12 + 1e-300
        b = np.where(valid, b, -np.inf)
        tau, keep, dense, sel = _select(score, b, valid, k, m)
        out.update({"bound" + tag: b, "tau" + tag: tau, "keep" + tag: keep, "dense" + tag: dense, "sel" + tag: sel})
    out["score"] = score
    return out


def P_ub(var_ub, mu_c, tau):
    """prod_j Pub_j [m] from var_ub [m], mu_c [nc][m], tau [nc]"""
    sub = np.sqrt(np.asarray(var_ub, dtype=np.float64))
    out = np.ones_like(sub)
    for mc, t in zip(np.asarray(mu_c, dtype=np.float64), np.asarray(tau, dtype=np.float64)):
        d = t - mc
        with np.errstate(divide="ignore", invalid="ignore"):
            neg = np.where(sub > 0.0, Phi(d / np.where(sub > 0.0, sub, 1.0)), 0.0)
        out = out * np.where(d >= 0.0, 1.0, neg)
    return out


_REST = {}


def case_restated(w):
    if w["name"] not in _REST:
        _REST[w["name"]] = restate_weighted(w)
    return _REST[w["name"]]


# --------------------------------------------------------------------------- shared checks
def envelope_w(mu, var, mu_c, p, tau, f_best_c, n_feasible, acq, sf2, power, tol, upper=False):
    """the least (upper: greatest) S of a posterior within tol of (mu, var, mu_c, p):
    the EI part is _prune_oracle.envelope (1 with no feasible row); each Phi factor
    is taken at the corners of its (mu_c, sigma) box -- Phi((tau - mu_c) / sigma) is
    monotone in mu_c, and in sigma for a fixed mu_c -- with the mean's tolerance on
    the standardised mu_c; p within the mean's relative tolerance.  Where scipy's
    erfc flushes a subnormal result to 0 the upper side takes the smallest normal
    double instead (_prune_oracle.envelope has the same rule for EI)."""
    s = -1.0 if upper else 1.0
    mu, var, p = (np.asarray(a, dtype=np.float64) for a in (mu, var, p))
    if n_feasible:
        E = po.envelope(mu, var, f_best_c, acq, sf2, tol, upper=upper)
    else:
        E = np.ones_like(mu)
    sig = [np.sqrt(np.maximum(var * (1.0 - q * tol[2]) - q * tol[3] * sf2, 0.0)) for q in (1.0, -1.0)]
    P = np.ones_like(mu)
    for mc, t in zip(np.asarray(mu_c, dtype=np.float64), np.asarray(tau, dtype=np.float64)):
        w = tol[0] * np.abs(mc) + tol[1]
        corners = []
        for mcc in (mc - w, mc + w):
            for sg in sig:
                with np.errstate(divide="ignore", invalid="ignore"):
                    f = Phi((t - mcc) / np.where(sg > 0.0, sg, 1.0))
                f = np.where(sg > 0.0, f, np.where(mcc <= t, 1.0, 0.0))
                if upper:
                    f = np.where((sg > 0.0) & (f < TINY), TINY, f)
                corners.append(f)
        P = P * (np.max(corners, axis=0) if upper else np.min(corners, axis=0))
    pp = np.maximum(p * (1.0 - s * tol[0]), 0.0)
    return (E * P) * (pp if power == 1.0 else pp ** power)


def check_bounds_w(ub, ex, valid, mu, var, mu_c, p, cg, acq, sf2, power, tol):
    """soundness per candidate against a reference within tol, and the exact flags'
    other side; duplicates hold -inf"""
    a = (cg.tau, cg.f_best_c, cg.n_feasible, acq, sf2, power, tol)
    lo = envelope_w(mu, var, mu_c, p, *a)
    hi = envelope_w(mu, var, mu_c, p, *a, upper=True)
    bad = np.flatnonzero(valid & ~(ub >= lo))
    assert bad.size == 0, ("unsound bound", bad[:8], ub[bad[:8]], lo[bad[:8]])
    e = valid & (ex != 0)
    bad = np.flatnonzero(e & ~(ub <= hi))
    assert bad.size == 0, ("exact flag on a bound above the score", bad[:8], ub[bad[:8]], hi[bad[:8]])
    assert np.all(ub[~valid] == -np.inf)
