"""Failure-aware scoring on the device (gp_feas.hip, uthot.h "failure-aware
scoring"): the kernel vote p = (S_ok + lambda p0) / (S_ok + S_fail + lambda)
against its CPU restatement (tests/_feas_oracle.py), and the weight score * p^gamma
in every dense scoring call.  Tolerances are the fp64 tier's:
1e-5 relative, atol 1e-12 on sums that may be ~0; "bitwise" means
assert_array_equal."""
import ctypes
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from _feas_oracle import feas_prob, gcc_split  # noqa: E402
from _spaces import oracle_space, to_manip  # noqa: E402
from oracle.space import BOOL, ENUM, FLOAT, INT, Param, features  # noqa: E402

RTOL, ATOL = 1e-5, 1e-12
UT_EINVAL, UT_EUNSUPPORTED, UT_ENOMEM = -1, -4, -6

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
    e.gp_feas_clear()
    e.gp_set_precision(64)
    e.gp_set_i8_tol(2.0 ** -20)
    return e


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host(*ts):
    return [t.cpu().numpy() for t in ts]


def data(n, nf, d, m, seed=0, lo=0.0, hi=1.0):
    """(X [n][d], F [nf][d], V [d][m] candidate values); float params over [0, 1]"""
    rng = np.random.default_rng(1000 * seed + n + nf + d + m)
    return rng.uniform(lo, hi, (n, d)), rng.uniform(lo, hi, (nf, d)), rng.uniform(lo, hi, (d, m))


def fit(e, X, ell, wait=True, seed=1):
    y = np.random.default_rng(seed).standard_normal(X.shape[0])
    e.gp_fit(X, y, lengthscale=ell, sigma_f2=1.0, sigma_n2=1e-4, jitter=1e-8, wait=wait)
    return y


def close(got, want, what=""):
    np.testing.assert_allclose(got, want, rtol=RTOL, atol=ATOL, err_msg=what)


def both_ways(e, d, V):
    """(p, S_ok, S_fail) through values= and through features=, each called twice: the same bits"""
    U = features(fspace(d), V)
    a = host(*e.gp_feas_prob(values=dev(V)))
    b = host(*e.gp_feas_prob(features=dev(U)))
    for x, y in zip(a, host(*e.gp_feas_prob(values=dev(V)))):
        np.testing.assert_array_equal(x, y)
    for x, y in zip(b, host(*e.gp_feas_prob(features=dev(U)))):
        np.testing.assert_array_equal(x, y)
    return a, b, U.T


PAD_CASES = [(100, 1, 5, 300), (129, 130, 37, 1)]


@pytest.mark.parametrize("n,nf,d,m", PAD_CASES)
def test_padding_rows_and_columns_add_nothing(n, nf, d, m):
    """every lengthscale 50 over points within 0.02 of each other: every k is 1
    to 3e-6, so S_ok is n and S_fail is n_f -- not 128, 256 or anything that
    follows ldk; and from 60 lengthscales away both sums are exactly 0"""
    e = engine(d)
    X, F, V = data(n, nf, d, m, lo=0.5, hi=0.52)
    fit(e, X, 50.0)
    e.gp_feas_set(F)
    for got in both_ways(e, d, V)[:2]:
        p, s_ok, s_fail = got
        print("n %d nf %d: S_ok %.9g .. %.9g, S_fail %.9g .. %.9g" % (n, nf, s_ok.min(), s_ok.max(), s_fail.min(),
                                                                    s_fail.max()))
        np.testing.assert_allclose(s_ok, n, rtol=1e-5)
        np.testing.assert_allclose(s_fail, nf, rtol=1e-5)
        wp, wok, wfail = feas_prob(X, F, features(fspace(d), V).T, 50.0)
        close(s_ok, wok), close(s_fail, wfail), close(p, wp)
    # ell = 0.01: a candidate at 1.0 in every coordinate is >= 48 sqrt(d) lengthscales from every row
    fit(e, X, 0.01)
    far = np.ones((d, m))
    for p, s_ok, s_fail in both_ways(e, d, far)[:2]:
        assert (s_ok == 0.0).all() and (s_fail == 0.0).all()
        np.testing.assert_array_equal(p, np.full(m, n / (n + nf)))


SHAPES = PAD_CASES + [(321, 257, 3, 1024), (130, 128, 64, 4096)]
#         ell, ell_scale, lambda, prior
PARAMS = [(0.3, 1.0, 1.0, None), (2.0, 0.5, 0.01, None), (2.0, 1.0, 1.0, 0.7), (0.3, 0.5, 0.01, None)]


@pytest.mark.parametrize("n,nf,d,m", SHAPES)
def test_parity_with_the_restatement(n, nf, d, m):
    e = engine(d)
    X, F, V = data(n, nf, d, m, seed=2)
    cases = list(PARAMS)
    if d == 3:   # per-feature lengthscales, once
        cases.append((np.array([0.2, 1.0, 3.0]), 1.0, 1.0, None))
    for ell, s, lam, prior in cases:
        fit(e, X, ell)
        e.gp_feas_set(F, prior=prior, strength=lam, ell_scale=s)
        a, b, U = both_ways(e, d, V)
        want = feas_prob(X, F, U, ell, prior=prior, strength=lam, ell_scale=s)
        for got in (a, b):
            for g, w, name in zip(got, want, ("p", "S_ok", "S_fail")):
                close(g, w, "%s at ell %r s %g lambda %g prior %r" % (name, ell, s, lam, prior))
        assert (a[0] >= 0.0).all() and (a[0] <= 1.0).all()


MIXED = [Param("x", FLOAT, -2.0, 2.0), Param("n", INT, 1, 40), Param("a", ENUM, options=["p", "q", "r"]),
         Param("b", ENUM, options=list("vwxyz")), Param("f", BOOL)]


@pytest.mark.parametrize("cat", ["1", "0"])
def test_categorical_operands(monkeypatch, cat):
    """ENUM / BOOL blocks: through values= the vote takes the int8 code product
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
        n, nf, m = 150, 131, 700
        feat = features(MIXED, vals.cpu().numpy()).T
        X, F, U = feat[:n], feat[n:n + nf], feat[n + nf:n + nf + m]
        V = vals[:, n + nf:n + nf + m].contiguous()
        for ell, s, lam in [(1.2, 1.0, 1.0), (0.6, 0.5, 0.01)]:
            fit(e, X, ell)
            assert e.gp_kstar_mode() == ("categorical" if cat == "1" else "dense")
            e.gp_feas_set(F, strength=lam, ell_scale=s)
            a = host(*e.gp_feas_prob(values=V))
            b = host(*e.gp_feas_prob(features=dev(U.T)))
            want = feas_prob(X, F, U, ell, strength=lam, ell_scale=s)
            for g1, g2, w, name in zip(a, b, want, ("p", "S_ok", "S_fail")):
                close(g1, w, name), close(g2, w, name), close(g1, g2, name)
            for x, y in zip(a, host(*e.gp_feas_prob(values=V))):
                np.testing.assert_array_equal(x, y)
        if cat == "1":
            # a failed row that is not one-hot cannot be read as codes: scoring through the code product says which
            bad = F.copy()
            bad[5, 2:5] = [0.5, 0.5, 0.0]
            e.gp_feas_set(bad)
            from uptune_amd._lib import UthotError
            with pytest.raises(UthotError, match="UT_EINVAL.*row 5"):
                e.gp_feas_prob(values=V)
            close(host(*e.gp_feas_prob(features=dev(U.T)))[0], feas_prob(X, bad, U, 0.6)[0])   # the dense one reads it
    finally:
        e.close()


def test_gcc_fixture_on_the_device(golden_dir):
    """the split of the CPU test (1,024 successful rows, 117 failed, 680
    candidates), isotropic ell = 3: 707 features, 552 of them one-hot"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from uptune_amd import spaces
    from uptune_amd.engine import BatchEngine
    manip = spaces.gcc()
    X, F, U, _, (v_ok, _, v_cand) = gcc_split(golden_dir, oracle_space(manip))
    z = np.load(os.path.join(golden_dir, "gcc_history.npz"))
    y = z["qor"][np.flatnonzero(np.isfinite(z["qor"]))[:1024]]
    e = BatchEngine(manip, device=0, seed=1)
    try:
        e.gp_fit(X, y, lengthscale=3.0, sigma_f2=1.0, sigma_n2=1e-6, jitter=1e-8)
        assert e.gp_kstar_mode() == "categorical"
        e.gp_feas_set(F)
        want = feas_prob(X, F, U, 3.0)
        a = host(*e.gp_feas_prob(values=dev(v_cand)))
        b = host(*e.gp_feas_prob(features=dev(U.T)))
        print("gcc on the device: p in [%.4f, %.4f]" % (a[0].min(), a[0].max()))
        for g1, g2, w, name in zip(a, b, want, ("p", "S_ok", "S_fail")):
            close(g1, w, name), close(g2, w, name)
    finally:
        e.close()


def dup7(m):
    d = np.zeros(m, dtype=np.uint8)
    d[::7] = 1
    return d


@pytest.mark.parametrize("prec", [64, 32, 16, 8])
def test_every_tier_takes_the_weight(prec):
    d, n, nf, m = 5, 100, 9, 300
    e = engine(d)
    X, F, V = data(n, nf, d, m, seed=3)
    if prec == 8:
        V[:, 1:40:3] = X[:13].T     # on training points the variance bound fails: recomputed in fp64
    e.gp_set_precision(prec)
    fit(e, X, 0.5)
    dup = dev(dup7(m))
    acq = e.acq("ei")
    modes = [None] if prec != 8 else ["some", "all"]
    for mode in modes:
        if mode == "all":
            e.gp_set_i8_tol(0.0)    # nothing is accepted: the whole round is recomputed in fp64
        e.gp_feas_clear()
        mu0, var0, s0 = host(*e.gp_score_values(dev(V), acq=acq, dup=dup))
        if mode is not None:
            rec = e.gp_i8_stats()[0]
            assert (rec == -1) if mode == "all" else (0 < rec < m), rec
        e.gp_feas_set(F, strength=0.5)
        mu1, var1, s1 = host(*e.gp_score_values(dev(V), acq=acq, dup=dup))
        if mode is not None:
            assert e.gp_i8_stats()[0] == rec
        p = host(*e.gp_feas_prob(values=dev(V)))[0]
        assert (p < 1.0).all() and (p > 0.0).all()
        isdup = dup7(m) != 0
        assert np.isneginf(s0[isdup]).all() and np.isneginf(s1[isdup]).all()
        assert np.isfinite(s0[~isdup]).all()
        np.testing.assert_array_equal(s1[~isdup], (s0 * p)[~isdup])       # gamma = 1: one multiplication
        assert (s1[~isdup] != s0[~isdup]).any()
        np.testing.assert_array_equal(mu1, mu0)
        np.testing.assert_array_equal(var1, var0)
        # through the feature matrix (ut_gp_score): the dense vote over the same rows
        U = features(fspace(d), V)
        e.gp_feas_clear()
        t0 = host(*e.gp_score(dev(U), acq=acq, dup=dup))[2]
        e.gp_feas_set(F, strength=0.5)
        t1 = host(*e.gp_score(dev(U), acq=acq, dup=dup))[2]
        pf = host(*e.gp_feas_prob(features=dev(U)))[0]
        np.testing.assert_array_equal(t1[~isdup], (t0 * pf)[~isdup])
        for gamma in (2.0, 0.5, 0.0):
            e.gp_feas_set(F, strength=0.5, power=gamma)
            sg = host(*e.gp_score_values(dev(V), acq=acq, dup=dup))[2]
            assert np.isneginf(sg[isdup]).all()
            if gamma == 0.0:
                np.testing.assert_array_equal(sg[~isdup], s0[~isdup])
            else:
                close(sg[~isdup], (s0 * p ** gamma)[~isdup], "gamma %g" % gamma)


def _d2h(ptr, count, dtype=np.float64):
    hip = ctypes.CDLL("libamdhip64.so")
    out = np.empty(count, dtype=dtype)
    rc = hip.hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(ptr), ctypes.c_size_t(out.nbytes), 2)
    assert rc == 0, rc
    return out


def _round_state(e, m, ncols):
    """(values [ncols][m], score [m], dup [m]) of the last eager round"""
    e.sync()
    (pv, _, _, pdup, _, _, psc), ld = e.round_buffers()
    assert pdup, "an eager round keeps its dup mask"
    vals = _d2h(pv, ld * ncols).reshape(ncols, ld)[:, :m].copy()
    return vals, _d2h(psc, m), _d2h(pdup, m, np.uint8)


@pytest.mark.parametrize("kind", ["de", "ga"])
def test_rounds_select_by_the_weighted_score(monkeypatch, kind):
    """the same round with its own 8 selections loaded as failed rows
    (lambda = 0.01): it selects topk(unweighted score * p) -- other candidates --
    and the lazy round selects what the eager one does"""
    d, n, m, k = 5, 100, 4096, 8
    e = engine(d)
    e.population_init(512, round_=0)
    pop = e.population_get().cpu().numpy()
    X = features(fspace(d), pop[:, :n]).T
    fit(e, X, 0.3)
    e.history_reset(0)
    parent = pop[:, 7].copy()

    def rnd(lazy):
        monkeypatch.setenv("UT_LAZY_HASH", "1" if lazy else "0")
        if kind == "de":
            out = e.score_round_de(m, k, round_=3, cand_base=0, cr=0.3)
        else:
            out = e.score_round_ga(m, k, parent1=parent, round_=3, cand_base=0, mutation_rate=0.3)
        return host(*out)

    idx0, top0, _, vals0 = rnd(False)
    V, s0, dup = _round_state(e, m, d)
    assert (idx0 >= 0).all()
    e.gp_feas_set(features(fspace(d), vals0).T, strength=0.01, ell_scale=0.5)
    p = host(*e.gp_feas_prob(values=dev(V)))[0]
    idx1, top1, _, vals1 = rnd(False)
    V1, s1, dup1 = _round_state(e, m, d)
    np.testing.assert_array_equal(V1, V)          # the same candidates
    np.testing.assert_array_equal(dup1, dup)
    want = s0 * p                                  # (-inf stays -inf: p > 0)
    np.testing.assert_array_equal(s1, want)
    widx, wtop = host(*e.topk(dev(want), k, dup=dev(dup)))
    np.testing.assert_array_equal(idx1, widx)
    np.testing.assert_array_equal(top1, wtop)
    assert set(idx1.tolist()) != set(idx0.tolist())
    print("%s round: unweighted %r -> weighted %r (p at the old picks %r)" % (kind, idx0.tolist(), idx1.tolist(),
                                                                              np.round(p[idx0], 4).tolist()))
    if kind == "de":     # (only DE rounds have a lazy form)
        lz0 = e.round_lazy_stats()[0]
        idx2, top2, _, vals2 = rnd(True)
        assert e.round_lazy_stats()[0] == lz0 + 1
        np.testing.assert_array_equal(idx2, idx1)
        np.testing.assert_array_equal(top2, top1)
        np.testing.assert_array_equal(vals2, vals1)


def test_refit_append_and_async_fit():
    d, n, nf, m = 5, 100, 40, 500
    e = engine(d)
    X, F, V = data(n + 10, nf, d, m, seed=4)
    U = features(fspace(d), V).T
    y = np.random.default_rng(9).standard_normal(n + 10)
    hyper = dict(sigma_f2=1.0, sigma_n2=1e-4, jitter=1e-8)
    e.gp_fit(X[:n], y[:n], lengthscale=0.3, **hyper)
    e.gp_feas_set(F)
    for g, w in zip(host(*e.gp_feas_prob(values=dev(V))), feas_prob(X[:n], F, U, 0.3)):
        close(g, w)
    # another lengthscale, the rows not loaded again: the operands are the new fit's
    e.gp_fit(X[:n], y[:n], lengthscale=1.1, **hyper)
    assert e.gp_last_fit_kind() == "refit"
    for g, w in zip(host(*e.gp_feas_prob(values=dev(V))), feas_prob(X[:n], F, U, 1.1)):
        close(g, w)
    # ten rows appended: S_ok and the default prior follow the fit in use
    e.gp_fit(X, y, lengthscale=1.1, **hyper)
    assert e.gp_last_fit_kind() == "append"
    sync = host(*e.gp_feas_prob(values=dev(V)))
    want = feas_prob(X, F, U, 1.1)
    for g, w in zip(sync, want):
        close(g, w)
    assert not np.array_equal(sync[1], feas_prob(X[:n], F, U, 1.1)[1])
    # an asynchronous refit and the vote at once: it waits on the device for the scaled inputs
    e.gp_fit(X[:n], y[:n], lengthscale=0.3, **hyper)
    e.gp_fit(X, y, lengthscale=1.1, wait=False, **hyper)
    for g, w in zip(host(*e.gp_feas_prob(values=dev(V))), sync):
        np.testing.assert_array_equal(g, w)
    assert e.gp_fit_ok()
    # the stage has a time of its own
    e.set_timing(True)
    e.gp_score_values(dev(V), acq=e.acq("ei"))
    assert e.stage_time("feas") > 0.0 and e.stage_time("kstar") > 0.0
    e.set_timing(False)


def test_errors_and_non_interference():
    from uptune_amd import _lib as L
    from uptune_amd.engine import BatchEngine
    d, n, nf, m, k = 5, 100, 12, 512, 8
    e = engine(d)
    X, F, V = data(n, nf, d, m, seed=5)
    U = features(fspace(d), V)
    e.population_init(256, round_=0)
    e.history_reset(0)
    fit(e, X, 0.4)
    ei, ucb = e.acq("ei"), e.acq("ucb")

    def four():
        """the calls that are unsupported while rows are loaded"""
        a = host(*e.gp_score_values(dev(V), acq=ucb))
        b = host(*e.gp_topk_pruned(dev(U), k, acq=ei, bound_rows=64)[:2])
        c = host(*e.score_round_de_pruned(m, k, round_=2, cr=0.3, bound_rows=64)[:4])
        s = host(*e.gp_select_batch(dev(V[:, :64]), k, acq=ei))
        return a + b + c + s

    before = four()
    info0 = e.gp_feas_info()
    assert info0["nf"] == 0
    e.gp_feas_set(F, strength=0.5)
    p0 = host(*e.gp_feas_prob(values=dev(V)))
    assert e.gp_feas_info() == dict(nf=nf, prior=None, strength=0.5, ell_scale=1.0, power=1.0)

    def rc(Xp=F.ctypes.data, nn=nf, dd=d, **par):
        q = dict(prior=0.0, strength=1.0, ell_scale=1.0, power=1.0)
        q.update(par)
        return e.lib.ut_gp_feas_set(e.ctx, Xp, nn, dd, ctypes.byref(L.FeasParams(**q)))

    bad_row = F.copy()
    bad_row[3, 2] = np.inf
    nan_row = F.copy()
    nan_row[nf - 1, 0] = np.nan
    inf, nan = float("inf"), float("nan")
    for name, got in [("NULL rows", rc(Xp=None)), ("nf < 0", rc(nn=-1)), ("d", rc(dd=d + 1)),
                      ("inf entry", rc(Xp=bad_row.ctypes.data)), ("nan entry", rc(Xp=nan_row.ctypes.data)),
                      ("strength 0", rc(strength=0.0)), ("strength < 0", rc(strength=-1.0)),
                      ("strength inf", rc(strength=inf)), ("strength nan", rc(strength=nan)),
                      ("ell_scale 0", rc(ell_scale=0.0)), ("ell_scale < 0", rc(ell_scale=-2.0)),
                      ("ell_scale inf", rc(ell_scale=inf)), ("ell_scale nan", rc(ell_scale=nan)),
                      ("power < 0", rc(power=-0.5)), ("power inf", rc(power=inf)), ("power nan", rc(power=nan)),
                      ("prior > 1", rc(prior=1.5)), ("prior nan", rc(prior=nan))]:
        assert got == UT_EINVAL, name
        # ... and what was loaded stays loaded
        assert e.gp_feas_info() == dict(nf=nf, prior=None, strength=0.5, ell_scale=1.0, power=1.0), name
    for x, y in zip(host(*e.gp_feas_prob(values=dev(V))), p0):
        np.testing.assert_array_equal(x, y)
    # the vote's own arguments
    out = torch.empty(m, dtype=torch.float64, device="cuda:0")
    vp, up = dev(V), dev(U)
    prob = e.lib.ut_gp_feas_prob
    assert prob(e.ctx, vp.data_ptr(), up.data_ptr(), m, m, out.data_ptr(), None, None) == UT_EINVAL
    assert prob(e.ctx, None, None, m, m, out.data_ptr(), None, None) == UT_EINVAL
    assert prob(e.ctx, vp.data_ptr(), None, m, m, None, None, None) == UT_EINVAL
    assert prob(e.ctx, vp.data_ptr(), None, m - 1, m, out.data_ptr(), None, None) == UT_EINVAL
    # unsupported while rows are loaded, each saying which call and why
    for call, who in [(lambda: e.gp_score_values(dev(V), acq=ucb), "gp_score"),
                      (lambda: e.gp_score(dev(U), acq=ucb), "gp_score"),
                      (lambda: e.gp_topk_pruned(dev(U), k, acq=ei, bound_rows=64), "gp_topk_pruned"),
                      (lambda: e.score_round_de_pruned(m, k, round_=2, cr=0.3, bound_rows=64),
                       "score_round_de_pruned"),
                      (lambda: e.gp_select_batch(dev(V[:, :64]), k, acq=ei), "gp_select_batch")]:
        with pytest.raises(L.UthotError, match="UT_EUNSUPPORTED: %s: failed rows are loaded" % who):
            call()
    # cleared: all four are back, with the bits they had before any rows were loaded
    e.gp_feas_clear()
    assert e.gp_feas_info()["nf"] == 0
    for x, y in zip(four(), before):
        np.testing.assert_array_equal(x, y)

    # a fresh engine: no fit -> UT_EINVAL as ut_gp_score_values; a failed allocation; device bytes
    e.gp_feas_set(F)
    fit(e, X, 0.4)
    want = host(*e.gp_score_values(dev(V), acq=ei))[2]
    base = e.device_bytes()
    f = BatchEngine(to_manip(fspace(d)), device=0, seed=8)
    try:
        f.gp_feas_set(F)                      # before any fit
        assert f.gp_feas_info()["nf"] == nf
        s = torch.empty(m, dtype=torch.float64, device="cuda:0")
        assert f.lib.ut_gp_feas_prob(f.ctx, vp.data_ptr(), None, m, m, out.data_ptr(), None, None) == \
            f.lib.ut_gp_score_values(f.ctx, vp.data_ptr(), m, m, ctypes.byref(ei), None, None, None,
                                     s.data_ptr()) == UT_EINVAL
        fit(f, X, 0.4)
        L.check(f.ctx, f.lib.ut_debug_fail_alloc(f.ctx, 1), "ut_debug_fail_alloc")
        with pytest.raises(L.UthotError, match="UT_ENOMEM"):
            f.gp_score_values(dev(V), acq=ei)
        got = host(*f.gp_score_values(dev(V), acq=ei))[2]      # the next call succeeds
        np.testing.assert_array_equal(got, want)
        assert f.device_bytes() > base
    finally:
        f.close()
    assert e.device_bytes() == base


def test_technique_loads_failures_on_the_device():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from uptune_amd import technique as T
    from uptune_amd.driver import SearchDriver
    d = 4
    space = to_manip(fspace(d))

    def objective(cfg):      # everything right of x0 = 0.5 fails to build
        if cfg["x0"] > 0.5:
            return float("inf")
        return (cfg["x0"] - 0.1) ** 2 + sum((cfg["x%d" % j] - 0.5) ** 2 for j in range(1, d))

    def run(feasibility):
        tech = T.GpuDifferentialEvolution(feasibility=feasibility, pool=4096, batch=8, population=256, seed=5,
                                          lengthscale=0.3, name="de")
        drv = SearchDriver(space, tech, parallelism=8)
        drv.main(objective, test_limit=6 * 8 - 1, max_generations=6)
        tech = drv.root_technique
        tech.model.fit(drv)       # what the next round would start with: the last generation's results
        return drv, tech

    drv, tech = run(True)
    eng, model = tech.engine, tech.model
    try:
        bad = [r for r in drv.results_query() if not np.isfinite(r.time)]
        good = [r for r in drv.results_query() if np.isfinite(r.time)]
        assert bad and len(good) >= model.min_train
        assert model.n_failed == len(bad)
        info = eng.gp_feas_info()
        assert info["nf"] == len(bad) and info["prior"] is None and info["strength"] == 1.0
        vals = eng.spec.encode_configs([r.configuration.data for r in bad])
        p, s_ok, s_fail = host(*eng.gp_feas_prob(values=dev(vals)))
        p0 = len(good) / (len(good) + len(bad))
        print("technique: %d ok, %d failed, p0 %.4f, p at the failed rows %.4f .. %.4f" % (len(good), len(bad), p0,
                                                                                         p.min(), p.max()))
        assert (s_fail >= 1.0 - 1e-12).all()
        assert (p < p0).all()
    finally:
        eng.close()
    drv0, tech0 = run(False)
    try:
        assert tech0.model.n_failed == 0 and tech0.engine.gp_feas_info()["nf"] == 0
        assert any(not np.isfinite(r.time) for r in drv0.results_query())
    finally:
        tech0.engine.close()
