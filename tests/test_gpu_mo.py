"""Two objectives on the device (gp_mo.hip, uthot.h "two objectives"): the
second objective's mean mu_2 = k* . alpha_2 on the fit's own factor, the Pareto
front of the fit's rows and the expected hypervolume improvement against it,
against the CPU restatement (tests/_mo_oracle.py), in every dense scoring call.

Tolerances are tests/test_gpu_cons.py's: RTOL 1e-5 / ATOL 1e-9 on mu_2 against
the restatement; the tail alone (EHVI restated from the device's own mu, var,
mu_2 and front) at rtol 1e-10 wherever the restated value is >= 1e-80, and in
[0, 2e-80] elsewhere (below that phi's rounding dominates and underflows: that
file's docstring has the argument for EI); every parity case asserts that at
least 90 % of its candidates are in the compared set.  "bitwise" means
assert_array_equal.  Every test fails without the feature: the entry points do
not exist.

Shapes: n = 130 rows (two row tiles, the second ragged), d = 3, m = 257
candidates (a ragged wave and a ragged workgroup).  k_mo_ehvi stages MO_CH = 256
strips of the front in LDS at a time; the P = n = 300 front takes two chunks."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from _ard_cases import by_name, ell_vector  # noqa: E402
from _mo_oracle import MoGP, ehvi, psi, rule_on  # noqa: E402
from _spaces import to_manip  # noqa: E402
from oracle import de as ode  # noqa: E402
from oracle.space import FLOAT, Param, features  # noqa: E402
from uptune_amd.pareto import default_ref, hypervolume2d  # noqa: E402

RTOL, ATOL = 1e-5, 1e-9
HYPER = dict(sigma_f2=1.0, sigma_n2=1e-4, jitter=1e-8)
UT_EINVAL, UT_EUNSUPPORTED = -1, -4
MO_CH = 256
N, D, M = 130, 3, 257

_ENGINES = {}


def fspace(d):
    return [Param("x%d" % j, FLOAT, 0.0, 1.0) for j in range(d)]


def engine(d=D):
    """one engine per feature count, reused: handed out with nothing loaded, at precision 64"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from uptune_amd.engine import BatchEngine
    e = _ENGINES.get(d)
    if e is None:
        e = _ENGINES[d] = BatchEngine(to_manip(fspace(d)), device=0, seed=7)
    e.gp_mo_clear()
    e.gp_cons_clear()
    e.gp_feas_clear()
    e.gp_set_prune_weighted(False)
    e.gp_set_precision(64)
    e.gp_set_i8_tol(2.0 ** -20)
    e.gp_set_fit_append(True)
    return e


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")


def host(*ts):
    return [t.cpu().numpy() for t in ts]


def _d2h(ptr, count, dtype=np.float64):
    import ctypes
    hip = ctypes.CDLL("libamdhip64.so")
    out = np.empty(count, dtype=dtype)
    rc = hip.hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(ptr), ctypes.c_size_t(out.nbytes), 2)
    assert rc == 0, rc
    return out


_DATA = {}


def data(n=N, d=D, m=M, seed=0):
    """X [n][d] in [0, 0.3]^d, y [n] and Y2 [n] two noisy bowls with their minima
    in opposite corners, on different scales and offsets (a front of about a
    dozen rows; smooth, so that the posterior mean away from the rows stays of
    the rows' own size), V [d][m] candidate values in
    [0.6, 1]^d -- test_gpu_cons.py's layout "apart", every candidate's variance
    well above the noise floor.  Computed once per shape, never written to."""
    key = (n, d, m, seed)
    if key not in _DATA:
        rng = np.random.default_rng(3000 * seed + n + d + m)
        X, V = rng.uniform(0.0, 0.3, (n, d)), rng.uniform(0.6, 1.0, (d, m))
        y = 30.0 * np.sum((X - 0.05) ** 2, axis=1) + 0.02 * rng.standard_normal(n)
        Y2 = 10.0 + 90.0 * np.sum((X - 0.25) ** 2, axis=1) + 0.06 * rng.standard_normal(n)
        for a in (X, V, y, Y2):
            a.setflags(write=False)
        _DATA[key] = (X, y, Y2, V)
    return _DATA[key]


def ref_of(y, Y2):
    return default_ref(np.column_stack([y, Y2]))


def fit(e, X, y, ell, wait=True):
    e.gp_fit(X, y, lengthscale=ell, wait=wait, **HYPER)


def ys_of(e, n):
    return e.gp_fit_read("YS")[0].cpu().numpy()[:n]


def tail_close(got, want, what=""):
    """rtol 1e-10 where the restatement is >= 1e-80, [0, 2e-80] elsewhere; at least 90 % compared"""
    got, want = np.asarray(got), np.asarray(want)
    big = want >= 1e-80
    print("%s: %d of %d compared, max rel err %.3g" % (
        what, int(big.sum()), big.size, np.max(np.abs(got[big] - want[big]) / want[big]) if big.any() else 0.0))
    assert big.mean() >= 0.9, what
    np.testing.assert_allclose(got[big], want[big], rtol=1e-10, atol=0.0, err_msg=what)
    assert np.all((got[~big] >= 0.0) & (got[~big] <= 2e-80)), what


def check_front(e, g, y, Y2, ref, what=""):
    """ut_gp_mo_front is the restated front: rows exactly, a and b bitwise the
    device's own ys and y2s there; ut_gp_mo_info agrees with it"""
    n = len(y)
    rows, a, b = e.gp_mo_front()
    info = e.gp_mo_info()
    assert rows.tolist() == g.rows.tolist(), what
    np.testing.assert_array_equal(a, ys_of(e, n)[rows], err_msg=what)
    np.testing.assert_array_equal(b, e.gp_mo_read(0)[rows], err_msg=what)
    assert np.all(np.diff(a) > 0) and np.all(np.diff(b) < 0), what
    assert info["n"] == n and info["P"] == len(rows), what
    np.testing.assert_allclose(info["ref_std"], (g.r1, g.r2), rtol=1e-12, atol=1e-13, err_msg=what)
    want_hv = hypervolume2d(np.column_stack([a, b]), info["ref_std"])
    print("%s: P %d, hv %.17g (host %.17g)" % (what, len(rows), info["hv"], want_hv))
    np.testing.assert_allclose(info["hv"], want_hv, rtol=1e-12, atol=0.0, err_msg=what)
    return rows, a, b, info


def both_ways(e, V):
    """(EHVI, mu_2) through values= and through features=, each called twice: the same bits"""
    U = features(fspace(V.shape[0]), V)
    a = host(*e.gp_mo_score(values=dev(V)))
    b = host(*e.gp_mo_score(features=dev(U)))
    for x, y in zip(a, host(*e.gp_mo_score(values=dev(V)))):
        np.testing.assert_array_equal(x, y)
    for x, y in zip(b, host(*e.gp_mo_score(features=dev(U)))):
        np.testing.assert_array_equal(x, y)
    for x, y in zip(a, b):
        np.testing.assert_array_equal(x, y)
    return a, U


def parity(e, X, y, Y2, ref, V, ell, what):
    """front, mu_2, the tail and the scoring calls of one loaded fit"""
    g = MoGP(X, y, Y2, ref, ell, **HYPER)
    rows, a, b, info = check_front(e, g, y, Y2, ref, what)
    (eh, mu2), U = both_ways(e, V)
    w_mu2 = g.mu2(U.T)
    print("%s: max |mu_2 diff| %.3g (|mu_2| <= %.3g)" % (what, np.abs(mu2 - w_mu2).max(), np.abs(w_mu2).max()))
    np.testing.assert_allclose(mu2, w_mu2, rtol=RTOL, atol=ATOL, err_msg=what)
    # the restatement alone keeps the fixture in the compared set
    w_mu, w_var = g.posterior(U.T)
    assert (g.ehvi(w_mu, w_var, w_mu2) >= 1e-80).mean() >= 0.9, what
    # the tail on the device's own posterior and front; xi is ignored
    mu, var, sc = host(*e.gp_score_values(dev(V), acq=e.acq("ei", xi=0.3)))
    assert (eh >= 0.0).all(), what
    tail_close(eh, ehvi(mu, var, mu2, a, b, *info["ref_std"]), what)
    np.testing.assert_array_equal(sc, eh, err_msg=what)
    mu_f, var_f, sc_f = host(*e.gp_score(dev(U)))
    np.testing.assert_array_equal(sc_f, eh, err_msg=what)
    return g, eh, mu, var


CASES = [("iso", 0.5, 64), ("ard", ell_vector(by_name("n77_d3_hand")["recipe"], D), 64), ("p8", 0.5, 8)]


@pytest.mark.parametrize("name,ell,prec", CASES, ids=[c[0] for c in CASES])
def test_parity_with_the_restatement(name, ell, prec):
    e = engine()
    X, y, Y2, V = data()
    ref = ref_of(y, Y2)
    e.gp_set_precision(prec)
    fit(e, X, y, ell)
    plain = host(*e.gp_score_values(dev(V)))
    e.gp_mo_set(Y2, ref)
    g, eh, mu, var = parity(e, X, y, Y2, ref, V, ell, name)
    assert 6 <= len(g.rows) <= 30, "the generic front has about a dozen members"
    # mu and var are never changed
    np.testing.assert_array_equal(mu, plain[0])
    np.testing.assert_array_equal(var, plain[1])
    # dup gives -inf, EHVI elsewhere
    dup = np.zeros(M, dtype=np.uint8)
    dup[[0, 64, 256]] = 1
    sc = host(*e.gp_score_values(dev(V), dup=dev(dup)))[2]
    np.testing.assert_array_equal(sc, np.where(dup != 0, -np.inf, eh))
    np.testing.assert_array_equal(rule_on(sc, eh), sc)
    # cleared: the plain EI bits
    e.gp_mo_clear()
    assert e.gp_mo_info()["n"] == 0
    for x, w in zip(host(*e.gp_score_values(dev(V))), plain):
        np.testing.assert_array_equal(x, w)


def test_every_row_on_the_front_takes_two_lds_chunks():
    n = 300
    assert n > MO_CH
    e = engine()
    X, y, _, V = data(n=n)
    Y2 = -y
    ref = ref_of(y, Y2)
    fit(e, X, y, 0.5)
    e.gp_mo_set(Y2, ref)
    g, eh, mu, var = parity(e, X, y, Y2, ref, V, 0.5, "P = n")
    assert len(g.rows) == n


def test_an_empty_front_is_the_product_of_two_improvements():
    e = engine()
    X, y, Y2, V = data()
    ref = (y.min() - 1.0, Y2.min() - 1.0)
    fit(e, X, y, 0.5)
    e.gp_mo_set(Y2, ref)
    g = MoGP(X, y, Y2, ref, 0.5, **HYPER)
    rows, a, b, info = check_front(e, g, y, Y2, ref, "P = 0")
    assert len(rows) == 0 and info["hv"] == 0.0
    (eh, mu2), U = both_ways(e, V)
    mu, var, sc = host(*e.gp_score_values(dev(V)))
    want = psi(info["ref_std"][0], mu, var) * psi(info["ref_std"][1], mu2, var)
    tail_close(eh, want, "P = 0")
    np.testing.assert_array_equal(sc, eh)


def test_identical_rows_and_a_row_on_the_box_s_face():
    e = engine()
    X, y, Y2, V = data()
    y, Y2 = y.copy(), Y2.copy()
    # rows 5 and 9 the same point, ahead of every other row in y: row 5 is on the front, row 9 is not
    y[5] = y[9] = y.min() - 0.5
    Y2[5] = Y2[9] = np.median(Y2)
    ref = ref_of(y, Y2)
    fit(e, X, y, 0.5)
    e.gp_mo_set(Y2, ref)
    g, *_ = parity(e, X, y, Y2, ref, V, 0.5, "twins")
    assert 5 in g.rows and 9 not in g.rows
    # the row with the smallest Y2 is on every front that holds it; with R1 its own y it has a = r_1 exactly
    k = int(np.argmin(Y2))
    assert k in g.rows
    face = (y[k], ref[1])
    e.gp_mo_set(Y2, face)
    g2 = MoGP(X, y, Y2, face, 0.5, **HYPER)
    assert g2.r1 == g2.ys[k] and k not in g2.rows and len(g2.rows) > 0
    rows, a, b, info = check_front(e, g2, y, Y2, face, "face")
    assert info["ref_std"][0] == ys_of(e, N)[k] and k not in rows
    # ... and inside when R1 is a little larger
    e.gp_mo_set(Y2, (y[k] + 1e-6, ref[1]))
    assert k in e.gp_mo_front()[0]


def test_score_round_returns_ehvi():
    e = engine()
    X, y, Y2, V = data()
    space = fspace(D)
    m, k = M, 8
    fit(e, X, y, 0.5)
    e.gp_mo_set(Y2, ref_of(y, Y2))
    e.population_init(64, round_=0)
    e.history_reset(0)
    pop = e.population_get().cpu().numpy()
    idx, top, dig, vals = e.score_round_de(m, k, round_=1, cr=0.3)
    idx, top = idx.cpu().numpy(), top.cpu().numpy()
    trial = ode.propose_de_vec(space, pop, 7, 1, 0, m, 0.3, 1)
    np.testing.assert_array_equal(vals.cpu().numpy(), trial[:, idx])
    eh = host(*e.gp_mo_score(values=dev(trial)))[0]
    np.testing.assert_array_equal(top, eh[idx])
    assert (idx >= 0).all() and top[0] == eh.max()
    # a GA round (eager: it keeps every candidate's score and its dup mask)
    idx2, top2, _, _ = host(*e.score_round_ga(m, k, parent1=trial[:, int(idx[0])].copy(), round_=2, mutation_rate=0.3))
    e.sync()
    (pv, _, _, pdup, _, _, psc), ld = e.round_buffers()
    assert pdup and psc
    Vg = _d2h(pv, ld * D).reshape(D, ld)[:, :m].copy()
    dup, sc = _d2h(pdup, m, np.uint8), _d2h(psc, m)
    eg = host(*e.gp_mo_score(values=dev(Vg)))[0]
    np.testing.assert_array_equal(sc, np.where(dup != 0, -np.inf, eg))
    sel = idx2[idx2 >= 0]
    np.testing.assert_array_equal(top2[: len(sel)], eg[sel])


def test_an_asynchronous_fit_followed_at_once_by_the_values():
    e = engine()
    X, y, Y2, V = data()
    ref = ref_of(y, Y2)
    e.gp_set_fit_append(False)
    fit(e, X, y, 0.5)
    e.gp_mo_set(Y2, ref)
    want = host(*e.gp_mo_score(values=dev(V)))
    front = e.gp_mo_front()
    e.gp_mo_clear()
    fit(e, X[::-1].copy(), y[::-1].copy(), 0.4)       # another fit in between
    fit(e, X, y, 0.5, wait=False)
    e.gp_mo_set(Y2, ref)                               # no host wait in between
    got = host(*e.gp_mo_score(values=dev(V)))
    for x, w in zip(got, want):
        np.testing.assert_array_equal(x, w)
    for x, w in zip(e.gp_mo_front(), front):
        np.testing.assert_array_equal(x, w)


def test_refusals_and_the_stale_fit():
    from uptune_amd import _lib as L
    from uptune_amd.engine import BatchEngine
    e = engine()
    X, y, Y2, V = data()
    U = features(fspace(D), V)
    ref = np.ascontiguousarray(ref_of(y, Y2))
    m, k = M, 8
    ei, ucb = e.acq("ei"), e.acq("ucb")
    e.population_init(64, round_=0)
    e.history_reset(0)
    fit(e, X, y, 0.5)
    e.gp_mo_set(Y2, ref)
    info0 = e.gp_mo_info()
    loaded = host(*e.gp_score_values(dev(V)))

    def good():
        assert e.gp_mo_info() == info0
        np.testing.assert_array_equal(host(*e.gp_score_values(dev(V)))[2], loaded[2])

    # every UT_EINVAL of ut_gp_mo_set leaves what is loaded in place
    def rc(Yp=Y2.ctypes.data, nn=N, rp=ref.ctypes.data):
        return e.lib.ut_gp_mo_set(e.ctx, Yp, nn, rp)

    inf_v, nan_r = Y2.copy(), ref.copy()
    inf_v[3] = np.inf
    nan_r[1] = np.nan
    inf_r = np.array([np.inf, ref[1]])
    for name, got in [("n", rc(nn=N - 1)), ("n < 0", rc(nn=-1)), ("NULL values", rc(Yp=None)), ("NULL ref", rc(rp=None)),
                      ("inf value", rc(Yp=inf_v.ctypes.data)), ("nan ref", rc(rp=nan_r.ctypes.data)),
                      ("inf ref", rc(rp=inf_r.ctypes.data))]:
        assert got == UT_EINVAL, name
        good()
    # gp_mo_score's own arguments
    out = torch.empty(m, dtype=torch.float64, device="cuda:0")
    vp, up = dev(V), dev(U)
    score = e.lib.ut_gp_mo_score
    assert score(e.ctx, vp.data_ptr(), up.data_ptr(), m, m, out.data_ptr(), None) == UT_EINVAL
    assert score(e.ctx, None, None, m, m, out.data_ptr(), None) == UT_EINVAL
    assert score(e.ctx, vp.data_ptr(), None, m, m, None, None) == UT_EINVAL
    assert score(e.ctx, vp.data_ptr(), None, m - 1, m, out.data_ptr(), None) == UT_EINVAL
    assert score(e.ctx, vp.data_ptr(), None, m, m, out.data_ptr(), None) == 0       # mu2_out may be NULL
    np.testing.assert_array_equal(out.cpu().numpy(), loaded[2])
    # unsupported while a second objective is loaded, each saying which call
    e.gp_ts_draw(4, 128, 1)
    for weighted in (False, True):
        e.gp_set_prune_weighted(weighted)
        for call, who in [(lambda: e.gp_score_values(dev(V), acq=ucb), "gp_score_values"),
                          (lambda: e.gp_score(dev(U), acq=ucb), "gp_score"),
                          (lambda: e.score_round_de(m, k, round_=2, cr=0.3, acq=ucb), "score_round"),
                          (lambda: e.score_round_ga(m, k, parent1=V[:, 0].copy(), round_=2, acq=ucb), "score_round_ga"),
                          (lambda: e.gp_topk_pruned(dev(U), k, acq=ei, bound_rows=64), "gp_topk_pruned"),
                          (lambda: e.score_round_de_pruned(m, k, round_=2, cr=0.3, bound_rows=64),
                           "score_round_de_pruned"),
                          (lambda: e.gp_select_batch(dev(V[:, :64]), k, acq=ei), "gp_select_batch"),
                          (lambda: e.gp_acq_grad(dev(V[:, :64]), acq=ei), "gp_acq_grad"),
                          (lambda: e.gp_polish(dev(V[:, :64]), 2, acq=ei), "gp_polish"),
                          (lambda: e.gp_ts_select(dev(V), 4), "gp_ts_select"),
                          (lambda: e.gp_cons_set(Y2.reshape(-1, 1), [10.0]), "gp_cons_set"),
                          (lambda: e.gp_feas_set(X[:4]), "gp_feas_set")]:
            with pytest.raises(L.UthotError, match="UT_EUNSUPPORTED: %s: a second objective is loaded" % who):
                call()
        good()
    e.gp_set_prune_weighted(False)
    assert e.gp_cons_info()["nc"] == 0 and e.gp_feas_info()["nf"] == 0
    # ... and the other way round: no second objective beside constraint values or failed rows
    e.gp_mo_clear()
    e.gp_cons_set(Y2.reshape(-1, 1), [10.0])
    with pytest.raises(L.UthotError, match="UT_EUNSUPPORTED: gp_mo_set: constraint values are loaded"):
        e.gp_mo_set(Y2, ref)
    e.gp_cons_clear()
    e.gp_feas_set(X[:4] + 0.5)
    with pytest.raises(L.UthotError, match="UT_EUNSUPPORTED: gp_mo_set: failed rows are loaded"):
        e.gp_mo_set(Y2, ref)
    e.gp_feas_clear()
    assert e.gp_mo_info()["n"] == 0
    with pytest.raises(L.UthotError, match="UT_EINVAL.*no second objective"):
        e.gp_mo_score(values=dev(V))
    e.gp_mo_set(Y2, ref)
    good()
    # a later fit: the values are stale, and every call that would apply them says so
    fit(e, X, y, 0.5)
    for call in (lambda: e.gp_score_values(dev(V), acq=ei), lambda: e.gp_score(dev(U), acq=ei),
                 lambda: e.gp_mo_score(values=dev(V)), lambda: e.score_round_de(m, k, round_=2, cr=0.3),
                 lambda: e.score_round_ga(m, k, parent1=V[:, 0].copy(), round_=2), lambda: e.gp_mo_info(),
                 lambda: e.gp_mo_front()):
        with pytest.raises(L.UthotError, match="UT_EINVAL.*stale"):
            call()
    e.gp_mo_set(Y2, ref)                                    # reloaded: as before
    good()
    fit(e, X, y, 0.5)
    e.gp_mo_clear()                                         # or cleared: the plain call succeeds
    assert np.isfinite(host(*e.gp_score_values(dev(V), acq=ucb))[2]).all()
    # no fit: UT_EINVAL
    f = BatchEngine(to_manip(fspace(D)), device=0, seed=8)
    try:
        assert f.lib.ut_gp_mo_set(f.ctx, Y2.ctypes.data, N, ref.ctypes.data) == UT_EINVAL
        assert f.gp_mo_info()["n"] == 0
        f.gp_mo_clear()
    finally:
        f.close()
