"""Constrained EI on the device (gp_cons.hip, uthot.h "constrained EI"): the
constraint means mu_cj = k* . alpha_j on the fit's own factor, P = prod_j
Phi((tau_j - mu_cj) / sigma) and score = EI(f_best_c) P against the CPU
restatement (tests/_cons_oracle.py), in every dense scoring call.

Tolerances: RTOL 1e-5 / ATOL 1e-9 on mu_c, as tests/test_gpu_parity.py has for
mu and var (sigma_n2 = 1e-4, jitter = 1e-8); the tail alone (P and the score
from the device's own mu, var, mu_c) at rtol 1e-10; "bitwise" means
assert_array_equal.  Every test fails without the feature: the entry points do
not exist.

Where the score's tail is compared.  EI = I Phi(z) + sigma phi(z) cancels for
z << 0: the two terms agree to 1 - 1 / z^2 while phi = exp(-z^2 / 2) carries a
relative error z^2 eps from the rounding of z alone, so ANY two fp64 evaluations
of the formula differ by about z^4 eps / 2 -- 1e-10 at z = -31 -- until both
underflow to 0 at z < -38.7.  The parity fixture ("apart": var >= 1e-3 for
every candidate) has no candidate in that band, which the test asserts before
it compares every score at rtol 1e-10.  The extra fixtures (candidates among
or on the training rows: var at the noise floor) do, so there the scores are
compared where z >= -20 or the restatement underflowed, and the test asserts
that this covers most of them; mu_c and P are compared everywhere."""
import ctypes

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from _cons_oracle import ConsGP, cons_prob, rule_on  # noqa: E402
from _feas_oracle import feas_prob  # noqa: E402
from _spaces import to_manip  # noqa: E402
from oracle.gp import acquisition  # noqa: E402
from oracle.space import BOOL, ENUM, FLOAT, INT, Param, features  # noqa: E402

RTOL, ATOL = 1e-5, 1e-9
HYPER = dict(sigma_f2=1.0, sigma_n2=1e-4, jitter=1e-8)
UT_EINVAL, UT_EUNSUPPORTED = -1, -4

_ENGINES = {}


def fspace(d):
    return [Param("x%d" % j, FLOAT, 0.0, 1.0) for j in range(d)]


def engine(d):
    """one engine per feature count, reused: handed out with nothing loaded, at precision 64"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from uptune_amd.engine import BatchEngine
    e = _ENGINES.get(d)
    if e is None:
        e = _ENGINES[d] = BatchEngine(to_manip(fspace(d)), device=0, seed=7)
    e.gp_cons_clear()
    e.gp_feas_clear()
    e.gp_set_precision(64)
    e.gp_set_i8_tol(2.0 ** -20)
    e.gp_set_fit_append(True)
    return e


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host(*ts):
    return [t.cpu().numpy() for t in ts]


def cons_values(X, nc, rng):
    """nc smooth measurements of the rows plus noise, on different scales and offsets"""
    d = X.shape[1]
    W = rng.standard_normal((d, nc)) / np.sqrt(d)
    return (np.sin(3.0 * X @ W) + 0.1 * rng.standard_normal((X.shape[0], nc))) * (1.0 + np.arange(nc)) + 5.0 * np.arange(nc)


def data(n, d, m, nc, seed=0, layout="mixed"):
    """X [n][d], y [n], C [n][nc], thresholds [nc], V [d][m] candidate values.
    layout "apart": the rows in [0, 0.3]^d and the candidates in [0.6, 1]^d, so
    that every candidate's variance is well above the noise floor (checked on
    the CPU for every shape and lengthscale used here: min var 2.0e-3)"""
    rng = np.random.default_rng(2000 * seed + n + d + m)
    if layout == "apart":
        X, V = rng.uniform(0.0, 0.3, (n, d)), rng.uniform(0.6, 1.0, (d, m))
    else:
        X, V = rng.uniform(0.0, 1.0, (n, d)), rng.uniform(0.0, 1.0, (d, m))
    y = rng.standard_normal(n)
    C = cons_values(X, nc, rng)
    return X, y, C, np.median(C, axis=0), V


def fit(e, X, y, ell, wait=True):
    e.gp_fit(X, y, lengthscale=ell, wait=wait, **HYPER)


def close(got, want, what=""):
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, err_msg=what)


def tail_close(got, want, what=""):
    """rtol 1e-10 where the restatement is nonzero; where it underflowed, nothing above 1e-300"""
    got, want = np.asarray(got), np.asarray(want)
    nz = want != 0.0
    if nz.any():
        print("%s: max rel err %.3g over %d nonzero" % (what, np.max(np.abs(got[nz] - want[nz]) / np.abs(want[nz])),
                                                          int(nz.sum())))
    np.testing.assert_allclose(got[nz], want[nz], rtol=1e-10, atol=1e-300, err_msg=what)
    assert np.all(np.abs(got[~nz]) <= 1e-300), what


def ei_conditioned(mu, var, f_best_c, xi=0.0):
    """where EI's own formula is good to 1e-10 in fp64 (see the module docstring)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        z = (f_best_c - mu - xi) / np.sqrt(var)
    return ~((z < -20.0) & (z > -38.7))


def both_ways(e, d, V):
    """(P, mu_c) through values= and through features=, each called twice: the same bits"""
    U = features(fspace(d), V)
    a = host(*e.gp_cons_prob(values=dev(V)))
    b = host(*e.gp_cons_prob(features=dev(U)))
    for x, y in zip(a, host(*e.gp_cons_prob(values=dev(V)))):
        np.testing.assert_array_equal(x, y)
    for x, y in zip(b, host(*e.gp_cons_prob(features=dev(U)))):
        np.testing.assert_array_equal(x, y)
    return a, b, U.T


PAD_CASES = [(100, 5, 300), (129, 37, 1)]


@pytest.mark.parametrize("nc", [1, 4])
@pytest.mark.parametrize("n,d,m", PAD_CASES)
def test_padding_and_the_fit_s_own_mean(n, d, m, nc):
    """mu_cj is what an ordinary fit on column j scores as its mean (a device
    path older than the constraints); padding rows and columns add nothing"""
    e = engine(d)
    X, y, C, thr, V = data(n, d, m, nc, seed=1)
    U = features(fspace(d), V)
    want = []
    for j in range(nc):
        fit(e, X, C[:, j], 0.5)
        want.append((host(*e.gp_score_values(dev(V)))[0], host(*e.gp_score(dev(U)))[0]))
    fit(e, X, y, 0.5)
    e.gp_cons_set(C, thr)
    assert e.gp_cons_info()["n"] == n and e.gp_cons_info()["nc"] == nc
    a, b, _ = both_ways(e, d, V)
    for j in range(nc):
        print("n %d nc %d j %d: |mu_c| <= %.3g, max abs diff %.3g / %.3g" % (
            n, nc, j, np.abs(want[j][0]).max(), np.abs(a[1][j] - want[j][0]).max(), np.abs(b[1][j] - want[j][1]).max()))
        close(a[1][j], want[j][0], "values, column %d" % j)
        close(b[1][j], want[j][1], "features, column %d" % j)
    # ell = 0.01: a candidate at 1.0 in every coordinate is >= 48 sqrt(d) lengthscales from every row
    X2 = 0.5 + 0.02 * X
    fit(e, X2, y, 0.01)
    e.gp_cons_set(C, thr)
    g = ConsGP(X2, y, C, thr, 0.01, **HYPER)
    wantP = cons_prob(np.full(m, HYPER["sigma_f2"]), np.zeros((nc, m)), g.tau)
    for P, mu_c in both_ways(e, d, np.ones((d, m)))[:2]:
        assert (mu_c == 0.0).all()
        print("far candidates: P %.17g, restatement %.17g" % (P[0], wantP[0]))
        np.testing.assert_allclose(P, wantP, rtol=1e-12, atol=0.0)


SHAPES = PAD_CASES + [(321, 3, 1024), (130, 64, 4096)]


@pytest.mark.parametrize("n,d,m", SHAPES)
def test_parity_with_the_restatement(n, d, m):
    e = engine(d)
    ells = [0.3, 2.0] + ([np.array([0.2, 1.0, 3.0])] if d == 3 else [])
    acq = e.acq("ei", xi=0.01)
    for layout in ("mixed", "apart"):
        for nc in (1, 2, 4):
            X, y, C, thr, V = data(n, d, m, nc, seed=2, layout=layout)
            for ell in ells:
                what = "%s nc %d ell %r" % (layout, nc, ell)
                fit(e, X, y, ell)
                e.gp_cons_set(C, thr)
                a, b, U = both_ways(e, d, V)
                g = ConsGP(X, y, C, thr, ell, **HYPER)
                w_mu, w_var = g.posterior(U)
                w_mc = g.mu_c(U)
                info = e.gp_cons_info()
                assert info["n_feasible"] == g.n_feasible > 0
                np.testing.assert_allclose(info["f_best_c"], g.f_best_c, rtol=1e-12)
                # (a) the constraint means
                for got in (a, b):
                    print("%s: max |mu_c diff| %.3g (|mu_c| <= %.3g)" % (what, np.abs(got[1] - w_mc).max(),
                                                                         np.abs(w_mc).max()))
                    close(got[1], w_mc, "mu_c, " + what)
                    assert (got[0] >= 0.0).all() and (got[0] <= 1.0).all()
                # (b) the tail on the device's own posterior
                mu, var, sc = host(*e.gp_score_values(dev(V), acq=acq))
                tail_close(a[0], cons_prob(var, a[1], g.tau), "P, " + what)
                ok = ei_conditioned(mu, var, info["f_best_c"], 0.01)
                if layout == "apart":
                    assert ok.all() and ei_conditioned(w_mu, w_var, g.f_best_c, 0.01).all(), what
                assert ok.mean() > 0.8, what
                tail_close(sc[ok], g_score(g, info, mu, var, a[1], 0.01)[ok], "score, " + what)
                # (c) P end to end, within what (a)'s envelopes allow
                if layout == "apart":
                    assert (w_var >= 1e-3).all(), "the fixture keeps every candidate off the noise floor"
                    sig = np.sqrt(w_var)
                    d_sig = (ATOL + RTOL * w_var) / (2.0 * sig)
                    bound = np.zeros(m)
                    for j in range(nc):
                        z = (g.tau[j] - w_mc[j]) / sig
                        bound += 0.3990 * ((ATOL + RTOL * np.abs(w_mc[j])) + np.abs(z) * d_sig) / sig
                    wP = g.prob(w_var, w_mc)
                    for got in (a, b):
                        err = np.abs(got[0] - wP)
                        print("%s: max |dP| %.3g, bound >= %.3g" % (what, err.max(), bound.min()))
                        assert (err <= bound).all(), what


def g_score(g, info, mu, var, mu_c, xi):
    """the score rule with the restatement's tau and the device's incumbent"""
    from _cons_oracle import cons_score
    return cons_score(mu, var, mu_c, g.tau, info["f_best_c"], info["n_feasible"], xi)


MIXED = [Param("x", FLOAT, -2.0, 2.0), Param("n", INT, 1, 40), Param("a", ENUM, options=["p", "q", "r"]),
         Param("b", ENUM, options=list("vwxyz")), Param("f", BOOL)]


@pytest.mark.parametrize("cat", ["1", "0"])
def test_categorical_operands(monkeypatch, cat):
    """ENUM / BOOL blocks: through values= the means take the int8 code product
    (categorical K*), through features= the dense contraction; both are the
    restatement's.  UT_CAT_KSTAR=0: dense either way."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from uptune_amd.engine import BatchEngine
    monkeypatch.setenv("UT_CAT_KSTAR", cat)
    e = BatchEngine(to_manip(MIXED), device=0, seed=3)
    try:
        e.population_init(1024, round_=0)
        vals = e.population_get().contiguous()
        n, m, nc = 150, 700, 3
        feat = features(MIXED, vals.cpu().numpy()).T
        X, U = feat[:n], feat[n:n + m]
        V = vals[:, n:n + m].contiguous()
        rng = np.random.default_rng(11)
        y, C = rng.standard_normal(n), cons_values(X, nc, rng)
        thr = np.median(C, axis=0)
        for ell in (1.2, 0.6):
            fit(e, X, y, ell)
            assert e.gp_kstar_mode() == ("categorical" if cat == "1" else "dense")
            e.gp_cons_set(C, thr)
            a = host(*e.gp_cons_prob(values=V))
            b = host(*e.gp_cons_prob(features=dev(U.T)))
            g = ConsGP(X, y, C, thr, ell, **HYPER)
            w_mc = g.mu_c(U)
            print("cat %s ell %g: max |mu_c diff| %.3g / %.3g" % (cat, ell, np.abs(a[1] - w_mc).max(),
                                                                 np.abs(b[1] - w_mc).max()))
            close(a[1], w_mc), close(b[1], w_mc), close(a[1], b[1])
            mu, var, _ = host(*e.gp_score_values(V))
            tail_close(a[0], cons_prob(var, a[1], g.tau), "P, values")
            for x, y2 in zip(a, host(*e.gp_cons_prob(values=V))):
                np.testing.assert_array_equal(x, y2)
    finally:
        e.close()


def dup7(m):
    d = np.zeros(m, dtype=np.uint8)
    d[::7] = 1
    return d


@pytest.mark.parametrize("prec", [64, 32, 16, 8])
def test_every_tier_takes_the_rule(prec):
    d, n, m, nc = 5, 100, 300, 2
    e = engine(d)
    X, y, C, thr, V = data(n, d, m, nc, seed=3)
    if prec == 8:
        V[:, 1:40:3] = X[:13].T     # on training points the variance bound fails: recomputed in fp64
    e.gp_set_precision(prec)
    fit(e, X, y, 0.5)
    g = ConsGP(X, y, C, thr, 0.5, **HYPER)
    dup = dev(dup7(m))
    isdup = dup7(m) != 0
    acq = e.acq("ei")
    U = features(fspace(d), V)
    for mode in ([None] if prec != 8 else ["some", "all"]):
        if mode == "all":
            e.gp_set_i8_tol(0.0)    # nothing is accepted: the whole round is recomputed in fp64
        e.gp_cons_clear()
        mu0, var0, s0 = host(*e.gp_score_values(dev(V), acq=acq, dup=dup))
        t_mu0, t_var0, t0 = host(*e.gp_score(dev(U), acq=acq, dup=dup))
        if mode is not None:
            rec = e.gp_i8_stats()[0]
            assert (rec == -1) if mode == "all" else (0 < rec < m), rec
        e.gp_cons_set(C, thr)
        info = e.gp_cons_info()
        mu1, var1, s1 = host(*e.gp_score_values(dev(V), acq=acq, dup=dup))
        P, mu_c = host(*e.gp_cons_prob(values=dev(V)))
        np.testing.assert_array_equal(mu1, mu0)
        np.testing.assert_array_equal(var1, var0)
        assert np.isneginf(s0[isdup]).all() and np.isneginf(s1[isdup]).all() and np.isfinite(s1[~isdup]).all()
        want = rule_on(s0, mu1, var1, mu_c, g.tau, info["f_best_c"], info["n_feasible"])
        ok = ~isdup & ei_conditioned(mu1, var1, info["f_best_c"])
        assert ok.sum() > 0.8 * (~isdup).sum()
        tail_close(s1[ok], want[ok], "precision %d %s, values" % (prec, mode))
        assert (s1[~isdup] != s0[~isdup]).any()
        # through the feature matrix (ut_gp_score)
        t_mu1, t_var1, t1 = host(*e.gp_score(dev(U), acq=acq, dup=dup))
        Pf, mu_cf = host(*e.gp_cons_prob(features=dev(U)))
        np.testing.assert_array_equal(t_mu1, t_mu0)
        np.testing.assert_array_equal(t_var1, t_var0)
        want = rule_on(t0, t_mu1, t_var1, mu_cf, g.tau, info["f_best_c"], info["n_feasible"])
        ok = ~isdup & ei_conditioned(t_mu1, t_var1, info["f_best_c"])
        tail_close(t1[ok], want[ok], "precision %d %s, features" % (prec, mode))
        # a caller that wants scores only: the posterior goes through context scratch
        s = torch.empty(m, dtype=torch.float64, device="cuda:0")
        vp = dev(V)
        assert e.lib.ut_gp_score_values(e.ctx, vp.data_ptr(), m, m, ctypes.byref(acq), dup.data_ptr(), None, None,
                                        s.data_ptr()) == 0
        np.testing.assert_array_equal(s.cpu().numpy(), s1)


def _d2h(ptr, count, dtype=np.float64):
    hip = ctypes.CDLL("libamdhip64.so")
    out = np.empty(count, dtype=dtype)
    rc = hip.hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(ptr), ctypes.c_size_t(out.nbytes), 2)
    assert rc == 0, rc
    return out


def _round_state(e, m, ncols):
    """(values [ncols][m], dup [m], mu [m], var [m], score [m]) of the last eager round"""
    e.sync()
    (pv, _, _, pdup, pmu, pvar, psc), ld = e.round_buffers()
    assert pdup, "an eager round keeps its dup mask"
    vals = _d2h(pv, ld * ncols).reshape(ncols, ld)[:, :m].copy()
    return vals, _d2h(pdup, m, np.uint8), _d2h(pmu, m), _d2h(pvar, m), _d2h(psc, m)


def _topk(score, dup, k):
    """indices of the k largest scores, ties to the smallest index; never a duplicate or a NaN"""
    ok = np.flatnonzero((dup == 0) & ~np.isnan(score))
    order = ok[np.lexsort((ok, -score[ok]))]
    return order[:k]


@pytest.mark.parametrize("kind", ["de", "ga"])
def test_rounds_select_by_the_rule(monkeypatch, kind):
    d, n, m, k, nc = 5, 100, 4096, 16, 2
    e = engine(d)
    e.population_init(512, round_=0)
    pop = e.population_get().cpu().numpy()
    X = features(fspace(d), pop[:, :n]).T
    rng = np.random.default_rng(21)
    y, C = rng.standard_normal(n), cons_values(X, nc, rng)
    thr = np.median(C, axis=0)
    fit(e, X, y, 0.3)
    e.history_reset(0)
    parent = pop[:, 7].copy()
    g = ConsGP(X, y, C, thr, 0.3, **HYPER)

    def rnd(lazy):
        monkeypatch.setenv("UT_LAZY_HASH", "1" if lazy else "0")
        if kind == "de":
            out = e.score_round_de(m, k, round_=3, cand_base=0, cr=0.3)
        else:
            out = e.score_round_ga(m, k, parent1=parent, round_=3, cand_base=0, mutation_rate=0.3)
        return host(*out)

    idx0 = rnd(False)[0]
    e.gp_cons_set(C, thr)
    info = e.gp_cons_info()
    idx1, top1, _, vals1 = rnd(False)
    V, dup, mu, var, sc = _round_state(e, m, d)
    P, mu_c = host(*e.gp_cons_prob(values=dev(V)))
    want = g_score(g, info, mu, var, mu_c, 0.0)
    assert np.isneginf(sc[dup != 0]).all()
    # the selection is the top-k of the rule on the round's own posterior; its scores are the rule's
    np.testing.assert_array_equal(idx1, _topk(np.where(dup != 0, -np.inf, want), dup, k))
    np.testing.assert_array_equal(idx1, _topk(sc, dup, k))
    np.testing.assert_array_equal(top1, sc[idx1])
    tail_close(top1, want[idx1], "%s round, the selections' scores" % kind)
    assert set(idx1.tolist()) != set(idx0.tolist())
    if kind == "de":     # (only DE rounds have a lazy form)
        lz0 = e.round_lazy_stats()[0]
        idx2, top2, _, vals2 = rnd(True)
        assert e.round_lazy_stats()[0] == lz0 + 1
        np.testing.assert_array_equal(idx2, idx1)
        np.testing.assert_array_equal(top2, top1)
        np.testing.assert_array_equal(vals2, vals1)


def test_incumbent_is_the_best_feasible_row():
    d, n, m = 5, 100, 300
    e = engine(d)
    X, y, C, thr, V = data(n, d, m, 2, seed=4)
    fit(e, X, y, 0.5)
    acq = e.acq("ei")
    mu0, var0, s0 = host(*e.gp_score_values(dev(V), acq=acq))
    # no feasible row: the score is P
    e.gp_cons_set(C, C.min(axis=0) - 1.0)
    info = e.gp_cons_info()
    assert info["n_feasible"] == 0 and np.isnan(info["f_best_c"]) and info["n"] == n and info["nc"] == 2
    s = host(*e.gp_score_values(dev(V), acq=acq))[2]
    P = host(*e.gp_cons_prob(values=dev(V)))[0]
    np.testing.assert_array_equal(s, P)
    assert (P < 1.0).all()
    # exactly one: its standardised objective, by the fit's own mean and std
    r = 17
    C1 = C.copy()
    C1[:, 0] = np.where(np.arange(n) == r, 0.0, 1.0 + np.arange(n))
    e.gp_cons_set(C1, [0.5, np.inf])
    info = e.gp_cons_info()
    _, mean, std = e.gp_stats()
    assert info["n_feasible"] == 1
    np.testing.assert_allclose(info["f_best_c"], (y[r] - mean) / std, rtol=4e-16)
    # every row feasible, P = 1: bitwise the unconstrained scores
    e.gp_cons_set(C, [1e300, 1e300])
    assert e.gp_cons_info()["n_feasible"] == n
    mu1, var1, s1 = host(*e.gp_score_values(dev(V), acq=acq))
    np.testing.assert_array_equal(host(*e.gp_cons_prob(values=dev(V)))[0], np.ones(m))
    np.testing.assert_array_equal(s1, s0)
    np.testing.assert_array_equal(mu1, mu0)
    np.testing.assert_array_equal(var1, var0)
    e.gp_cons_set(C, [np.inf, np.inf])
    np.testing.assert_array_equal(host(*e.gp_score_values(dev(V), acq=acq))[2], s0)


def test_async_and_append_fits():
    d, n, m, nc = 5, 100, 500, 2
    e = engine(d)
    X, y, C, thr, V = data(n + 10, d, m, nc, seed=5)
    acq = e.acq("ei")
    # waited
    fit(e, X[:n], y[:n], 0.4)
    e.gp_cons_set(C[:n], thr)
    want = host(*e.gp_score_values(dev(V), acq=acq)) + host(*e.gp_cons_prob(values=dev(V)))
    # staged, the values loaded with no host wait in between, then scored at once
    fit(e, X[:n], y[:n], 1.3)
    fit(e, X[:n], y[:n], 0.4, wait=False)
    e.gp_cons_set(C[:n], thr)
    got = host(*e.gp_score_values(dev(V), acq=acq)) + host(*e.gp_cons_prob(values=dev(V)))
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    assert e.gp_fit_ok()
    # ten rows appended and the values reloaded, against a full refit of the same rows
    fit(e, X, y, 0.4)
    assert e.gp_last_fit_kind() == "append"
    e.gp_cons_set(C, thr)
    P_app, mc_app = host(*e.gp_cons_prob(values=dev(V)))
    e.gp_set_fit_append(False)
    fit(e, X, y, 0.4)
    assert e.gp_last_fit_kind() == "refit"
    e.gp_cons_set(C, thr)
    P_ref, mc_ref = host(*e.gp_cons_prob(values=dev(V)))
    print("append against refit: max |dP| %.3g, max |dmu_c| %.3g" % (np.abs(P_app - P_ref).max(),
                                                                     np.abs(mc_app - mc_ref).max()))
    np.testing.assert_allclose(P_app, P_ref, rtol=0.0, atol=1e-9)
    assert not np.array_equal(P_app, want[3])
    # the stage has a time of its own
    e.set_timing(True)
    e.gp_score_values(dev(V), acq=acq)
    assert e.stage_time("cons") > 0.0 and e.stage_time("kstar") > 0.0
    e.set_timing(False)


def test_contract():
    from uptune_amd import _lib as L
    from uptune_amd.engine import BatchEngine
    d, n, m, k, nc = 5, 100, 512, 8, 2
    e = engine(d)
    X, y, C, thr, V = data(n, d, m, nc, seed=6)
    U = features(fspace(d), V)
    e.population_init(256, round_=0)
    e.history_reset(0)
    fit(e, X, y, 0.4)
    ei, ucb = e.acq("ei"), e.acq("ucb")

    def four():
        """the calls that are unsupported while constraints are loaded"""
        a = host(*e.gp_score_values(dev(V), acq=ucb))
        b = host(*e.gp_topk_pruned(dev(U), k, acq=ei, bound_rows=64)[:2])
        c = host(*e.score_round_de_pruned(m, k, round_=2, cr=0.3, bound_rows=64)[:4])
        s = host(*e.gp_select_batch(dev(V[:, :64]), k, acq=ei))
        return a + b + c + s

    before = four()
    plain = host(*e.gp_score_values(dev(V), acq=ei))
    assert e.gp_cons_info() == dict(n=0, nc=0, n_feasible=0, f_best_c=pytest.approx(float("nan"), nan_ok=True))
    np.testing.assert_array_equal(host(*e.gp_cons_prob(values=dev(V)))[0], np.ones(m))     # nothing loaded: P = 1
    e.gp_cons_set(C, thr)
    info0 = e.gp_cons_info()
    P0, mc0 = host(*e.gp_cons_prob(values=dev(V)))
    loaded = host(*e.gp_score_values(dev(V), acq=ei))
    np.testing.assert_array_equal(loaded[0], plain[0])      # mu and var: the same bits
    np.testing.assert_array_equal(loaded[1], plain[1])
    assert (loaded[2] != plain[2]).any()

    # every UT_EINVAL of ut_gp_cons_set leaves what is loaded in place
    def rc(Cp=C.ctypes.data, nn=n, cc=nc, tp=None, t=thr):
        t = np.ascontiguousarray(t, dtype=np.float64)
        return e.lib.ut_gp_cons_set(e.ctx, Cp, nn, cc, t.ctypes.data if tp is None else tp)

    inf_v, nan_v = C.copy(), C.copy()
    inf_v[3, 1] = np.inf
    nan_v[n - 1, 0] = np.nan
    five = np.zeros((n, 5))
    for name, got in [("n", rc(nn=n - 1)), ("nc < 0", rc(cc=-1)), ("nc > 4", rc(Cp=five.ctypes.data, cc=5, t=np.zeros(5))),
                      ("NULL values", rc(Cp=None)), ("NULL thresholds", e.lib.ut_gp_cons_set(e.ctx, C.ctypes.data, n, nc, None)),
                      ("inf value", rc(Cp=inf_v.ctypes.data)), ("nan value", rc(Cp=nan_v.ctypes.data)),
                      ("nan threshold", rc(t=[0.0, float("nan")]))]:
        assert got == UT_EINVAL, name
        assert e.gp_cons_info() == info0, name
    assert rc(t=[float("inf"), float("-inf")]) == 0          # infinite thresholds are allowed
    e.gp_cons_set(C, thr)
    np.testing.assert_array_equal(host(*e.gp_cons_prob(values=dev(V)))[0], P0)
    # gp_cons_prob's own arguments
    out = torch.empty(m, dtype=torch.float64, device="cuda:0")
    vp, up = dev(V), dev(U)
    prob = e.lib.ut_gp_cons_prob
    assert prob(e.ctx, vp.data_ptr(), up.data_ptr(), m, m, out.data_ptr(), None) == UT_EINVAL
    assert prob(e.ctx, None, None, m, m, out.data_ptr(), None) == UT_EINVAL
    assert prob(e.ctx, vp.data_ptr(), None, m, m, None, None) == UT_EINVAL
    assert prob(e.ctx, vp.data_ptr(), None, m - 1, m, out.data_ptr(), None) == UT_EINVAL
    assert prob(e.ctx, vp.data_ptr(), None, m, m, out.data_ptr(), None) == 0       # mu_c_out may be NULL
    np.testing.assert_array_equal(out.cpu().numpy(), P0)
    # unsupported while constraints are loaded, each saying which call and why
    for call, who in [(lambda: e.gp_score_values(dev(V), acq=ucb), "gp_score"),
                      (lambda: e.gp_score(dev(U), acq=ucb), "gp_score"),
                      (lambda: e.gp_topk_pruned(dev(U), k, acq=ei, bound_rows=64), "gp_topk_pruned"),
                      (lambda: e.score_round_de_pruned(m, k, round_=2, cr=0.3, bound_rows=64),
                       "score_round_de_pruned"),
                      (lambda: e.gp_select_batch(dev(V[:, :64]), k, acq=ei), "gp_select_batch")]:
        with pytest.raises(L.UthotError, match="UT_EUNSUPPORTED: %s: constraint values are loaded" % who):
            call()
    # with failed rows loaded as well: EI(f_best_c) P p^gamma, the vote applied last
    F = np.random.default_rng(3).uniform(size=(12, d))
    for gamma in (1.0, 2.0):
        e.gp_feas_set(F, strength=0.5, power=gamma)
        mu, var, both = host(*e.gp_score_values(dev(V), acq=ei))
        p = host(*e.gp_feas_prob(values=dev(V)))[0]
        P = host(*e.gp_cons_prob(values=dev(V)))[0]
        np.testing.assert_array_equal(P, P0)
        np.testing.assert_allclose(both, loaded[2] * p ** gamma, rtol=1e-12)     # the constrained score times p^gamma
        np.testing.assert_allclose(p, feas_prob(X, F, U.T, 0.4, strength=0.5)[0], rtol=1e-5)
    # ... and against EI evaluated here, on a fixture where EI's formula is good to 1e-12 (z^4 eps / 2:
    # |z| < 9.7, module docstring): rows and candidates apart at ell = 1, the failed rows among the candidates
    X2, y2, C2, thr2, V2 = data(n, d, m, nc, seed=6, layout="apart")
    fit(e, X2, y2, 1.0)
    e.gp_cons_set(C2, thr2)
    fb = e.gp_cons_info()["f_best_c"]
    F2 = np.random.default_rng(4).uniform(0.6, 1.0, size=(12, d))
    for gamma in (1.0, 2.0):
        e.gp_feas_set(F2, strength=0.5, power=gamma)
        mu, var, both = host(*e.gp_score_values(dev(V2), acq=ei))
        p = host(*e.gp_feas_prob(values=dev(V2)))[0]
        P = host(*e.gp_cons_prob(values=dev(V2)))[0]
        z = (fb - mu) / np.sqrt(var)
        assert z.min() > -9.0 and (p < 1.0).all() and p.max() > p.min() and P.max() - P.min() > 0.1
        full = acquisition(mu, var, fb, "ei", 0.0) * P * p ** gamma
        print("gamma %g: max rel err of EI(f_best_c) P p^gamma %.3g (z %.2f .. %.2f)" % (
            gamma, np.max(np.abs(both - full) / full), z.min(), z.max()))
        np.testing.assert_allclose(both, full, rtol=1e-12)
    e.gp_feas_clear()
    fit(e, X, y, 0.4)
    e.gp_cons_set(C, thr)
    # a later fit: the values are stale, and every call that would apply them says so
    fit(e, X, y, 0.4)
    for call in (lambda: e.gp_score_values(dev(V), acq=ei), lambda: e.gp_score(dev(U), acq=ei),
                 lambda: e.gp_cons_prob(values=dev(V)), lambda: e.score_round_de(m, k, round_=2, cr=0.3)):
        with pytest.raises(L.UthotError, match="UT_EINVAL.*stale"):
            call()
    e.gp_cons_set(C, thr)                                   # reloaded: as before
    np.testing.assert_array_equal(host(*e.gp_score_values(dev(V), acq=ei))[2], loaded[2])
    fit(e, X, y, 0.4)
    e.gp_cons_clear()                                       # or cleared: the unconstrained bits
    assert e.gp_cons_info()["nc"] == 0
    for x, y2 in zip(host(*e.gp_score_values(dev(V), acq=ei)), plain):
        np.testing.assert_array_equal(x, y2)
    for x, y2 in zip(four(), before):
        np.testing.assert_array_equal(x, y2)
    # no fit: UT_EINVAL
    f = BatchEngine(to_manip(fspace(d)), device=0, seed=8)
    try:
        assert f.lib.ut_gp_cons_set(f.ctx, C.ctypes.data, n, nc, thr.ctypes.data) == UT_EINVAL
        assert f.gp_cons_info()["nc"] == 0
        f.gp_cons_clear()
    finally:
        f.close()


def test_technique_on_the_device():
    """time = x0 + x1 under accuracy = x0 >= 0.5: the unconstrained optimum (0, 0)
    violates the constraint.  One DE round from 64 seeded results selects the
    restatement's top-k of its own pool."""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from uptune_amd import technique as T
    from uptune_amd.driver import SearchDriver, ThresholdAccuracyMinimizeTime
    space = to_manip(fspace(2))

    def objective(cfg):
        return {"time": cfg["x0"] + cfg["x1"], "accuracy": cfg["x0"]}

    cons = [("accuracy", ">=", 0.5)]
    model = T.SharedModel(constraints=cons, lengthscale=0.3, seed=5, **{k: HYPER[k] for k in ("sigma_n2", "jitter")})
    tech = T.GpuDifferentialEvolution(shared=model, pool=4096, batch=8, population=256, seed=5, name="de")
    drv = SearchDriver(space, tech, objective=ThresholdAccuracyMinimizeTime(0.5), parallelism=8)
    rng = np.random.default_rng(12)
    drv.seed_results([{"x0": float(a), "x1": float(b)} for a, b in rng.uniform(size=(64, 2))], objective)
    tech = drv.root_technique
    model = tech.model
    try:
        vals, idx, top, dig, rows = tech._local_round()
        eng = tech.engine
        res = drv.results_query()
        n = len(res)
        info = eng.gp_cons_info()
        n_ok = sum(1 for r in res if r.accuracy >= 0.5)
        assert n == 64 and info["n"] == n and info["nc"] == 1 and info["n_feasible"] == n_ok == model.n_feasible_
        assert drv.best_result.accuracy >= 0.5
        # the restatement on what the model was fitted on, over the round's own pool
        g = ConsGP(model._Xf[:n], model._yf[:n], model._Cf[:n], [-0.5], 0.3, **HYPER)
        np.testing.assert_array_equal(model._Cf[:n, 0], -model._Xf[:n, 0])
        V = vals.cpu().numpy()
        U = features(fspace(2), V).T
        dup = eng.dedup(eng.hash_de(vals, tech.round_base())).cpu().numpy()
        mu, var = g.posterior(U)
        want = g.score(mu, var, g.mu_c(U))
        widx = _topk(np.where(dup != 0, -np.inf, want), dup, tech.batch)
        got = idx.cpu().numpy() - tech.round_base()
        print("technique: %d of %d rows feasible; picks %r, restatement %r; x0 of the picks %r" % (
            n_ok, n, got.tolist(), widx.tolist(), np.round(V[0, got], 3).tolist()))
        np.testing.assert_array_equal(got, widx)
    finally:
        tech.engine.close()
