"""Every GP scoring path under one lengthscale per feature, as
SharedModel._select_ard fits them (lengthscale="ard"), on the case table of
tests/_ard_cases.py; test_ard_cases_cpu.py proves on the reference alone that
each case notices a 1/ell taken from the wrong feature and that the oracle is
good to 1 % of the tolerance there.  With one scalar lengthscale a wrong index
into 1/ell, or a vector left over from the previous fit, gives the same bits.

  a  gp_score against oracle/gp.py at precisions 64 / 32 / 16 / 8
     (test_gp_vs_oracle's tolerances)
  b  precision 8: the int8 tier's bounds (test_i8_bound_holds's assertions) with
     K* on the int8 MFMA (gp_kq.hip) and on the fp64 MFMA (UT_KSTAR_Q=0), the two
     forms against each other (test_gpu_kstar_q.py's 1e-9 / 1e-10), the default
     tolerance against the oracle
  c  the categorical K* (one lengthscale over the ENUM / BOOL columns, one per
     numeric feature, one per PERM parameter) against the dense contraction on
     the same engine, a UT_CAT_KSTAR=0 engine and the oracle
  d  the fused DE round at precisions 64 and 8
  f  gp_select_batch and the constraint means
  g  hand-over between fits whose vectors differ in one feature: append /
     refit, the failed rows' cached operands, an async fit behind a queued score
  (e, the pruned top-k, is the ard_* cases of tests/_prune_oracle.py.)

Every test prints its largest error as a fraction of its tolerance.  Measured on
an MI355X, the largest of each path: a 1.8e-4 (precision 64), 0.015 (8), 0.78
(32) and 0.93 (16; both n600_d33_one_short_last at sf2 = 37, whose variances are
held to the unscaled floor 1e-5); b 1.8e-3 of the variance bound and 4.2e-3 of the
mean bound, the two K* forms 0.70 of 1e-9 / 1e-10 apart (n300_d16_spread), 0.023
against the oracle, 10 of 3000 candidates recomputed in every case (the ten next
to training points) with either K*; c 0.77 of 1e-9 / 1e-10 between the forms and
4.6e-3 against the oracle (cat_mixed, cond(K) 8e6; at precisions 32 / 16 its EI is
1.97 / 1.82 of the tier's tolerance on the categorical and on both dense paths
alike, which is what test_categorical_kstar_equals_dense's rule asks); d 2.4e-3;
f 2.7e-6 (select), 7.4e-3 (mu_c) and 0.047 (P's tail, of 1e-10); g 0.98 of 1e-10 / 1e-12 (a precision-8 append against its refit),
bitwise for the failed rows, 2.2e-5 for the async fit.  So gp_kq.hip's error at
the ARD floor stays inside what E and the 2^-20 acceptance allow.

What the table catches, tried by hand on an MI355X (every wrong index in bounds).
1/ell[feat_num[c]] for 1/ell[c] in k_encode_scaled_cat fails test_categorical_kstar
(all 12), test_constraint_means_categorical and
test_failed_rows_follow_the_fit_categorical; column k for num_feat[k] in
k_gp_num_train (the training operands) fails the same 14; an append test that
skips the last feature fails test_append_then_one_lengthscale_changes (both).
A third candidate-side map, k_gp_prep_cand_cat's 1/ell[num_feat[k]], passed
every test with 1/ell[k] in its place: no entry point reached that kernel (the
feature-matrix entry of the pruned top-k always takes the dense K*), and it was
removed with this table.  Needs a GPU."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu
torch = pytest.importorskip("torch")

import _ard_cases as A  # noqa: E402
import _batch_oracle as B  # noqa: E402
from _cons_oracle import ConsGP, cons_prob  # noqa: E402
from _feas_oracle import feas_prob  # noqa: E402
from _spaces import to_manip  # noqa: E402
from oracle import de as ode  # noqa: E402
from oracle import gp as ogp  # noqa: E402
from oracle.space import FLOAT, Param, features  # noqa: E402


def _engine(space, seed=0):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from uptune_amd.engine import BatchEngine
    return BatchEngine(to_manip(space), device=0, seed=seed)


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")   # (a copy: the table's arrays are read-only)


def host(*ts):
    return [t.cpu().numpy() for t in ts]


def _d2h(ptr, m):
    out = np.empty(m, dtype=np.float64)
    rc = ctypes.CDLL("libamdhip64.so").hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(ptr),
                                                 ctypes.c_size_t(out.nbytes), 2)
    assert rc == 0, rc
    return out


def _held(what, got, want, tol):
    """assert_allclose, after printing the largest error as a fraction of the tolerance"""
    w = A.worst(got, want, *tol)
    print("%s: %.3g of the tolerance (rtol %g, atol %g)" % (what, w, tol[0], tol[1]))
    np.testing.assert_allclose(got, want, rtol=tol[0], atol=tol[1], err_msg=what)
    return w


def _var_tol(tol, sf2):
    """the variance's absolute floor is relative to sf2 where that is the tighter one"""
    return (tol[0], tol[1] * min(1.0, sf2))


_SCORES = {}


def _score(c, prec, tol=None, kstar_q=None, monkeypatch=None):
    """(mu, var, ei) of the case's candidates on a fresh engine, and at precision 8
    (recomputed, E, Emu); computed once per setting, never written to"""
    key = (c["name"], prec, tol, kstar_q)
    if key not in _SCORES:
        if kstar_q is not None:
            monkeypatch.setenv("UT_KSTAR_Q", "1" if kstar_q else "0")
        z = A.numeric_data(c)
        e = _engine(A.float_space(c["d"]))
        e.gp_set_precision(prec)
        if tol is not None:
            e.gp_set_i8_tol(tol)
        e.gp_fit(z["X"], z["y"], lengthscale=z["ell"], **A.hyper(c))
        out = host(*e.gp_score(dev(z["U"].T), acq=e.acq("ei")))
        stats = (e.gp_i8_stats()[0],) + e.gp_i8_bounds() if prec == 8 else None
        mode = e.gp_kstar_mode()
        e.close()
        assert mode == "dense"
        for a in out:
            a.setflags(write=False)
        _SCORES[key] = (out, stats)
    return _SCORES[key]


# --------------------------------------------------------------------------- a
@pytest.mark.parametrize("prec", [64, 32, 16, 8])
@pytest.mark.parametrize("c", A.NUMERIC, ids=A.numeric_ids())
def test_gp_score_against_the_oracle(c, prec):
    z = A.numeric_data(c)
    (mu, var, ei), stats = _score(c, prec)
    t_mu, t_var, t_ei = A.tiers(prec)
    if stats:
        print("%s: precision 8 recomputed %d of %d, E %.3g, Emu %.3g" % ((c["name"], stats[0], A.M) + stats[1:]))
    _held("%s prec %d mu" % (c["name"], prec), mu, z["mu"], t_mu)
    _held("%s prec %d var" % (c["name"], prec), var, z["var"], _var_tol(t_var, c["sf2"]))
    _held("%s prec %d ei" % (c["name"], prec), ei, z["ei"], t_ei)


# --------------------------------------------------------------------------- b
I8_CASES = [c for c in A.NUMERIC if c["recipe"] in ("spread", "one_short_first", "one_short_last")]


@pytest.mark.parametrize("c", I8_CASES, ids=[c["name"] for c in I8_CASES])
def test_i8_bounds_and_kstar_forms(monkeypatch, c):
    """at the ARD floor gp_kq.hip's one exponent ea for all scaled training features
    is at its largest; its error grows as 2^(ea + eb) and the variance bound E does
    not count it"""
    z, sf2 = A.numeric_data(c), c["sf2"]
    (mu64, var64, _), _ = _score(c, 64)
    t_mu, t_var, t_ei = A.tiers(8)
    got = {}
    for q in (True, False):
        what = "%s K* on the %s MFMA" % (c["name"], "int8" if q else "fp64")
        # -- the int8 contraction's own results: within the fit's bounds of the fp64 path
        (mu8, var8, ei8), (rec, E, Emu) = _score(c, 8, tol=0.999, kstar_q=q, monkeypatch=monkeypatch)
        assert E > 0.0 and Emu > 0.0 and rec >= 0
        v2 = np.maximum(sf2 - var64, 0.0)
        bound = E * (2 * np.sqrt(v2) + E) + 1e-13 * sf2
        mbound = Emu + 1e-12 * np.maximum(1.0, np.abs(mu64))
        w_v, w_m = float(np.max(np.abs(var8 - var64) / bound)), float(np.max(np.abs(mu8 - mu64) / mbound))
        print("%s, tol 0.999: recomputed %d, E %.3g, Emu %.3g; |var8 - var64| %.3g of its bound, |mu8 - mu64| %.3g" %
              (what, rec, E, Emu, w_v, w_m))
        assert np.all(np.abs(var8 - var64) <= bound), w_v
        assert np.all(np.abs(mu8 - mu64) <= mbound), w_m
        ok = bound <= 2.0 ** -20 * var64
        _held(what + " accepted var", var8[ok], z["var"][ok], (A.RTOL, 1e-8 * sf2))
        # -- the default tolerance: the fp64 tier against the oracle
        (mu, var, ei), (rec_d, _, _) = _score(c, 8, kstar_q=q, monkeypatch=monkeypatch)
        print("%s, default tolerance: recomputed %d of %d" % (what, rec_d, A.M))
        assert 0 <= rec_d <= A.M // 2
        _held(what + " mu", mu, z["mu"], t_mu)
        _held(what + " var", var, z["var"], _var_tol(t_var, sf2))
        _held(what + " ei", ei, z["ei"], t_ei)
        got[q] = ((mu8, var8, ei8), (mu, var, ei))
    # -- the two forms of K*: one tier, 1e-9 relative (1e-10 absolute)
    for name, a, b in (("tol 0.999", got[True][0], got[False][0]), ("default", got[True][1], got[False][1])):
        _held("%s int8 K* against fp64 K*, %s, mu" % (c["name"], name), a[0], b[0], (1e-9, 1e-10))
        _held("%s int8 K* against fp64 K*, %s, var" % (c["name"], name), a[1], b[1], (1e-9, 1e-10 * sf2))
        _held("%s int8 K* against fp64 K*, %s, ei" % (c["name"], name), a[2], b[2], (1e-9, 1e-10))


# --------------------------------------------------------------------------- c
def _cat_engine(c, prec, monkeypatch, cat_kstar):
    z = A.categorical_data(c)
    monkeypatch.setenv("UT_CAT_KSTAR", "1" if cat_kstar else "0")
    e = _engine(z["space"], seed=9)
    e.gp_set_precision(prec)
    e.gp_fit(z["X"], z["y"], lengthscale=z["ell"], **A.hyper(c))
    return e


@pytest.mark.parametrize("prec", [64, 32, 16, 8])
@pytest.mark.parametrize("c", A.CATEGORICAL, ids=A.categorical_ids())
def test_categorical_kstar(monkeypatch, c, prec):
    """the candidates' operands index 1/ell through two maps (row feat_num[c] of
    the fused encoder, num_feat[k] of the feature-matrix form) and the training
    operands through a third; the assertions of test_categorical_kstar_equals_dense"""
    z = A.categorical_data(c)
    e = _cat_engine(c, prec, monkeypatch, True)
    assert e.gp_kstar_mode() == "categorical"
    vals = dev(z["cand"])
    cat = host(*e.gp_score_values(vals, acq=e.acq("ei")))
    enc = host(*e.gp_score(e.encode(vals), acq=e.acq("ei")))
    e.close()
    f = _cat_engine(c, prec, monkeypatch, False)
    assert f.gp_kstar_mode() == "dense"
    dense = host(*f.gp_score_values(vals, acq=f.acq("ei")))
    f.close()
    want = (z["mu"], z["var"], z["ei"])
    names = ("mu", "var", "ei")
    if prec in (64, 8):
        for other, label in ((enc, "gp_score(encode)"), (dense, "UT_CAT_KSTAR=0")):
            for nm, a, b in zip(names, cat, other):
                _held("%s prec %d %s against %s" % (c["name"], prec, nm, label), a, b, (1e-9, 1e-10))
        for nm, a, w in zip(names, cat, want):
            _held("%s prec %d %s against the oracle" % (c["name"], prec, nm), a, w, (A.RTOL, A.ATOL))
    else:
        # (as test_categorical_kstar_equals_dense: on a training point the 32-bit tiers'
        # variance is a cancellation in f32, the dense path's too)
        def err(a, b):
            return float(np.max(np.abs(a - b) / (1e-5 + 1e-3 * np.abs(b))))
        for nm, a, d0, d1, w in zip(names, cat, enc, dense, want):
            print("%s prec %d %s: categorical %.3g, gp_score(encode) %.3g, UT_CAT_KSTAR=0 %.3g of the tolerance" %
                  (c["name"], prec, nm, err(a, w), err(d0, w), err(d1, w)))
            assert err(a, w) <= max(1.0, 1.25 * err(d0, w)), (err(a, w), err(d0, w))
            assert err(a, w) <= max(1.0, 1.25 * err(d1, w)), (err(a, w), err(d1, w))


# --------------------------------------------------------------------------- d
def test_fused_round(monkeypatch):
    """score_round_de on 33 FLOAT parameters under the spread vector: the round's
    values are the oracle's trial, its means and variances (round_buffers) the
    oracle's posterior on every 97th candidate, its picks the oracle's EI, and
    precisions 64 and 8 select the same candidates"""
    d, n, m, k, npop, seed = 33, 600, 8192, 32, 3000, 5
    space = [Param("x%d" % j, FLOAT, -1000.0, 1000.0) for j in range(d)]
    ell = A.ell_vector("spread", d)
    pop = ode.population_init(space, npop, seed=seed)
    X = features(space, pop[:, :n]).T
    y = np.sum((X - 0.45) ** 2, axis=1)
    hyp = dict(sigma_f2=1.0, sigma_n2=1e-6, jitter=1e-8)
    g = ogp.GP(X, y, lengthscale=ell, **hyp)
    trial = ode.propose_de_vec(space, pop, seed, 1, 0, m, 0.3, 1)
    pick = np.arange(0, m, 97)
    mu_o, var_o = g.posterior(features(space, trial[:, pick]).T)
    got = {}
    for prec in (64, 8):
        e = _engine(space, seed=seed)
        e.gp_set_precision(prec)
        e.population_set(dev(pop))
        e.history_reset(0)
        e.gp_fit(X, y, lengthscale=ell, wait=False, **hyp)
        idx, top, dig, sel = e.score_round_de(m, k, round_=1, cand_base=0, cr=0.3)
        e.sync()
        (pv, _, _, _, pmu, pvar, psc), ld = e.round_buffers()
        vals = _d2h(pv, ld * d).reshape(d, ld)[:, :m]
        mu, var, sc = _d2h(pmu, m), _d2h(pvar, m), _d2h(psc, m)
        idx, top = host(idx, top)
        assert e.gp_kstar_mode() == "dense"
        e.close()
        np.testing.assert_array_equal(vals, trial)
        _held("round prec %d mu" % prec, mu[pick], mu_o, (A.RTOL, A.ATOL))
        _held("round prec %d var" % prec, var[pick], var_o, (A.RTOL, 1e-8))
        mu_s, var_s = g.posterior(features(space, trial[:, idx]).T)
        _held("round prec %d selected ei" % prec, top, ogp.acquisition(mu_s, var_s, g.f_best), (A.RTOL, 1e-8))
        np.testing.assert_array_equal(top, sc[idx])
        got[prec] = (idx, top, sc)
    s = np.sort(got[64][2])[::-1]
    apart = np.min(np.abs(np.diff(s[:k + 1]))) > 1e-8 * max(abs(s[0]), 1e-300)
    print("round: the top %d scores are %s 1e-8 relative" % (k + 1, "apart by more than" if apart else "within"))
    _held("round top, precision 8 against 64", got[8][1], got[64][1], (1e-7, 1e-12))
    if apart:
        np.testing.assert_array_equal(got[8][0], got[64][0])


# --------------------------------------------------------------------------- f
def _replay(what, e, g, V, U, k, noise, rtol):
    """test_gpu_batch_select.py's replay check along the device's own picks"""
    dup = np.zeros(U.shape[0], dtype=np.uint8)
    dup[::7] = 1
    pos, score, var = host(*e.gp_select_batch(dev(V), k, acq=e.acq("ei"), dup=dev(dup)))
    w = B.select(g, U, k, noise, kind="ei", dup=dup, forced=pos)
    assert (pos >= 0).all() and (w["pos"] == pos).all()
    bound = rtol * np.abs(w["score"]) + rtol * abs(w["score"][0])
    e_score, e_best, e_var = np.abs(score - w["score"]), w["best"] - w["score"], np.abs(var - w["var"])
    print("%s: score err %.3g, best - pick %.3g of the bound; var err %.3g of rtol (|var| + sf2)" %
          (what, np.max(e_score / bound), np.max(e_best / bound), np.max(e_var / (rtol * (np.abs(w["var"]) + 1.0)))))
    assert (e_score <= bound).all() and (e_best <= bound).all()
    assert (e_var <= rtol * (np.abs(w["var"]) + 1.0)).all()
    assert len(set(pos.tolist())) == k and not dup[pos].any() and (np.diff(score) <= 0.0).all()


def test_select_batch_numeric():
    c = A.by_name("n600_d33_spread")
    z = A.numeric_data(c)
    e = _engine(A.float_space(c["d"]))
    e.gp_fit(z["X"], z["y"], lengthscale=z["ell"], **A.hyper(c))
    U = B.pool(c["n"], 300, c["d"])
    _replay(c["name"], e, z["gp"], U.T, U, 64, c["sn2"] + c["jitter"], 1e-5)   # (sigma_n2 = 1e-6: the 1e-5 tier)
    e.close()


def test_select_batch_categorical(monkeypatch):
    c = A.by_name("cat_mixed")
    z = A.categorical_data(c)
    e = _cat_engine(c, 64, monkeypatch, True)
    assert e.gp_kstar_mode() == "categorical"
    sl = slice(100, 400)
    _replay(c["name"], e, z["gp"], z["cand"][:, sl], z["U"][sl], 48, c["sn2"] + c["jitter"], 1e-5)
    e.close()


CONS_HYPER = dict(sigma_f2=1.0, sigma_n2=1e-4, jitter=1e-8)   # test_gpu_cons.py's, with its tolerances


def _cons_values(X, nc, rng):
    """test_gpu_cons.py's: nc smooth measurements of the rows plus noise, on different scales and offsets"""
    d = X.shape[1]
    W = rng.standard_normal((d, nc)) / np.sqrt(d)
    return (np.sin(3.0 * X @ W) + 0.1 * rng.standard_normal((X.shape[0], nc))) * (1.0 + np.arange(nc)) + 5.0 * np.arange(nc)


def _cons_check(what, e, X, y, ell, V, U, nc=3):
    C = _cons_values(X, nc, np.random.default_rng(11))
    thr = np.median(C, axis=0)
    e.gp_fit(X, y, lengthscale=ell, **CONS_HYPER)
    e.gp_cons_set(C, thr)
    g = ConsGP(X, y, C, thr, ell, **CONS_HYPER)
    info = e.gp_cons_info()
    assert info["n_feasible"] == g.n_feasible > 0
    np.testing.assert_allclose(info["f_best_c"], g.f_best_c, rtol=1e-12)
    w_mc = g.mu_c(U)
    # (each entry point with the variance of its own K*: P's tail magnifies the two forms' rounding)
    for label, got, var in (("values", host(*e.gp_cons_prob(values=dev(V))), host(*e.gp_score_values(dev(V)))[1]),
                            ("features", host(*e.gp_cons_prob(features=dev(U.T))), host(*e.gp_score(dev(U.T)))[1])):
        _held("%s mu_c through %s" % (what, label), got[1], w_mc, (1e-5, 1e-9))
        wP = cons_prob(var, got[1], g.tau)     # the tail on the device's own posterior (rtol 1e-10)
        nz = wP != 0.0
        _held("%s P through %s" % (what, label), got[0][nz], wP[nz], (1e-10, 1e-300))
        assert np.all(np.abs(got[0][~nz]) <= 1e-300)


def test_constraint_means_numeric():
    c = A.by_name("n600_d33_spread")
    z = A.numeric_data(c)
    e = _engine(A.float_space(c["d"]))
    _cons_check(c["name"], e, z["X"], z["y"], z["ell"], z["U"][:1000].T, z["U"][:1000])
    e.close()


def test_constraint_means_categorical(monkeypatch):
    c = A.by_name("cat_mixed")
    z = A.categorical_data(c)
    monkeypatch.setenv("UT_CAT_KSTAR", "1")
    e = _engine(z["space"], seed=9)
    _cons_check(c["name"], e, z["X"], z["y"], z["ell"], z["cand"][:, :1000], z["U"][:1000])
    assert e.gp_kstar_mode() == "categorical"
    e.close()


# --------------------------------------------------------------------------- g
@pytest.mark.parametrize("prec", [64, 8])
def test_append_then_one_lengthscale_changes(prec):
    """ut_gp_fit appends when the rows grow under the same vector (compared per
    feature) and refits when only the LAST feature's lengthscale differs.  Rows
    520 -> 580 -> 620: one padded size (640), which an append needs (500 -> 560
    goes from 512 to 640 padded rows and refits whatever the vector)."""
    c = A.by_name("n600_d33_spread")
    d = c["d"]
    rng = np.random.default_rng(620 + d)
    X = rng.uniform(size=(620, d))
    y = np.sum((X - 0.4) ** 2, axis=1) + 0.01 * rng.standard_normal(620)
    U = rng.uniform(size=(A.M, d))
    U[:10] = X[610:] + 1e-3
    ell = A.ell_vector("spread", d)
    hyp = A.hyper(c)
    t_mu, t_var, _ = A.tiers(prec)
    e = _engine(A.float_space(d))
    e.gp_set_precision(prec)
    e.gp_fit(X[:520], y[:520], lengthscale=ell, **hyp)
    assert e.gp_last_fit_kind() == "refit"
    e.gp_fit(X[:580], y[:580], lengthscale=ell, **hyp)
    assert e.gp_last_fit_kind() == "append"
    mu, var, _ = host(*e.gp_score(dev(U.T)))
    f = _engine(A.float_space(d))
    f.gp_set_precision(prec)
    f.gp_fit(X[:580], y[:580], lengthscale=ell, **hyp)
    mu_f, var_f, _ = host(*f.gp_score(dev(U.T)))
    f.close()
    _held("append prec %d mu against a refit" % prec, mu, mu_f, (1e-10, 1e-12))
    _held("append prec %d var against a refit" % prec, var, var_f, (1e-10, 1e-12))
    g = ogp.GP(X[:580], y[:580], lengthscale=ell, **hyp)
    mu_o, var_o = g.posterior(U)
    _held("append prec %d mu against the oracle" % prec, mu, mu_o, t_mu)
    _held("append prec %d var against the oracle" % prec, var, var_o, t_var)
    ell2 = ell.copy()
    ell2[-1] = ell[-1] * 3.0 if ell[-1] * 3.0 <= 16.0 * np.sqrt(d) else ell[-1] / 3.0
    assert A.in_box(ell2) and np.array_equal(ell2[:-1], ell[:-1])
    e.gp_fit(X, y, lengthscale=ell2, **hyp)
    assert e.gp_last_fit_kind() == "refit"
    mu, var, _ = host(*e.gp_score(dev(U.T)))
    e.close()
    g2 = ogp.GP(X, y, lengthscale=ell2, **hyp)
    mu_o, var_o = g2.posterior(U)
    _held("one lengthscale changed, prec %d mu" % prec, mu, mu_o, t_mu)
    _held("one lengthscale changed, prec %d var" % prec, var, var_o, t_var)


def _feas_handover(make, X, y, F, ell_a, ell_b, cand, hyp):
    """(p, S_ok, S_fail) after a refit under ell_b of an engine that cached the
    failed rows' operands under ell_a, and of a fresh engine"""
    e = make()
    e.gp_fit(X, y, lengthscale=ell_a, **hyp)
    e.gp_feas_set(F)
    first = host(*e.gp_feas_prob(**cand))          # (the operands under ell_a are built here)
    e.gp_fit(X, y, lengthscale=ell_b, **hyp)
    got = host(*e.gp_feas_prob(**cand))
    e.close()
    f = make()
    f.gp_fit(X, y, lengthscale=ell_b, **hyp)
    f.gp_feas_set(F)
    want = host(*f.gp_feas_prob(**cand))
    f.close()
    assert not np.array_equal(first[0], want[0])   # the changed feature matters to the vote
    for a, b in zip(got, want):
        np.testing.assert_array_equal(a, b)
    return got


def test_failed_rows_follow_the_fit_numeric():
    c = A.by_name("n600_d33_spread")
    z, d = A.numeric_data(c), c["d"]
    F = np.random.default_rng(9).uniform(size=(130, d))
    ell_b = z["ell"].copy()
    j = int(np.argmin(ell_b))                      # the shortest lengthscale: the feature the vote depends on most
    ell_b[j] *= 4.0
    U = z["U"][:1000]
    got = _feas_handover(lambda: _engine(A.float_space(d)), z["X"], z["y"], F, z["ell"], ell_b,
                         dict(features=dev(U.T)), A.hyper(c))
    for nm, a, w in zip(("p", "S_ok", "S_fail"), got, feas_prob(z["X"], F, U, ell_b)):
        _held("failed rows after the refit, " + nm, a, w, (1e-5, 1e-12))   # test_gpu_feas.py's


def test_failed_rows_follow_the_fit_categorical(monkeypatch):
    c = A.by_name("cat_mixed")
    z = A.categorical_data(c)
    monkeypatch.setenv("UT_CAT_KSTAR", "1")
    F = features(z["space"], ode.population_init(z["space"], 130, seed=21)).T.copy()
    kinds, gv = z["kinds"], z["gvals"].copy()
    num = [g for g, k in enumerate(kinds) if k == "num"]
    gv[num[int(np.argmin(gv[num]))]] *= 4.0
    ell_b = np.ascontiguousarray(gv[z["gid"]])
    assert A.in_box(ell_b) and int(np.sum(ell_b != z["ell"])) == 1
    got = _feas_handover(lambda: _engine(z["space"], seed=9), z["X"], z["y"], F, z["ell"], ell_b,
                         dict(values=dev(z["cand"][:, :1000])), A.hyper(c))
    for nm, a, w in zip(("p", "S_ok", "S_fail"), got, feas_prob(z["X"], F, z["U"][:1000], ell_b)):
        _held("failed rows after the refit (categorical), " + nm, a, w, (1e-5, 1e-12))


def test_async_fit_behind_a_queued_score():
    """gp_score on 2^16 candidates under fit A, then gp_fit(wait=False) with the
    same rows and vector B (which overwrites the shared 1/ell buffer), then
    gp_score again, all enqueued before anything is read: the first result is
    A's posterior and the second B's (a sample of the candidates against the oracle)"""
    c = A.by_name("n600_d33_spread")
    z, d = A.numeric_data(c), c["d"]
    m = 1 << 16
    U = np.random.default_rng(5).uniform(size=(m, d))
    ell_a, ell_b = z["ell"], np.roll(z["ell"], 1)
    hyp = A.hyper(c)
    e = _engine(A.float_space(d))
    feat = dev(U.T)
    e.gp_fit(z["X"], z["y"], lengthscale=ell_a, **hyp)
    first = e.gp_score(feat)
    e.gp_fit(z["X"], z["y"], lengthscale=ell_b, wait=False, **hyp)
    second = e.gp_score(feat)
    first, second = host(*first), host(*second)
    e.close()
    pick = np.concatenate([np.arange(0, m, 31), np.arange(m - 64, m)])
    for label, got, ell in (("A", first, ell_a), ("B", second, ell_b)):
        g = z["gp"] if label == "A" else ogp.GP(z["X"], z["y"], lengthscale=ell, **hyp)
        mu_o, var_o = g.posterior(U[pick])
        _held("async: the score under fit %s, mu" % label, got[0][pick], mu_o, (A.RTOL, A.ATOL))
        _held("async: the score under fit %s, var" % label, got[1][pick], var_o, (A.RTOL, 1e-8))
