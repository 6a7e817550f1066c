"""Weighted pruning (ut_gp_set_prune_weighted): ut_gp_topk_pruned and
ut_score_round_de_pruned with constraint values and / or failed rows loaded, on
the case table of tests/_prune_weight_cases.py at both bound passes.  Every
bound is held per candidate (ut_gp_prune_bounds) and every selection against
the dense device weighted scores (gp_score with the same rows and values
loaded; path-to-path tolerance) and the numpy restatement (the fp64 tier's).
test_prune_weight_cpu.py proves on the reference alone that every case sits in
its regime and that its selection is decidable, so nothing here is asserted
under a condition.

Survivors measured on an MI355X, pass 32 / pass 64 (restated).  Pass 64 keeps
exactly the restated set everywhere; the f32 pass up to 5 % more.
  t1.0 217 / 209 (209), t0.6 208 / 199 (199), t0.35 201 / 198 (198), t-1_nofeas 376 / 376 (376),
  two 206 / 195 (195), four 250 / 241 (241), vote_only 237 / 228 (228), t0.6_f100 214 / 212 (212),
  short_f64 178 / 178 (178), n129_f30 20 / 20 (20), m257_f30 17 / 17 (17), k1_f40 1 / 1 (1),
  late_dense dense / dense (3867), flat dense / dense (4948), few_f20 dense / dense (2000),
  ard_f100 474 / 460 (460), gamma2 226 / 218 (218), prior0.7 214 / 212 (212), ell_scale0.5 214 / 212 (212);
  rows_n_exact 35 at pass 32 (35; at pass 64 every bound is flagged exact, its count was not recorded);
  the fused categorical round (m = 8192) 754 / 733."""
import ctypes
from types import SimpleNamespace

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import _prune_oracle as po  # noqa: E402
import _prune_weight_cases as pw  # noqa: E402
from _cons_oracle import ConsGP  # noqa: E402
from _spaces import to_manip  # noqa: E402
from oracle import de as ode  # noqa: E402
from oracle.space import BOOL, ENUM, FLOAT, INT, Param, features  # noqa: E402

EI = dict(kind="ei", xi=0.0, kappa=2.0)


def _require_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


def fspace(d):
    return [Param("x%d" % i, FLOAT, 0.0, 1.0) for i in range(d)]


_ENGINES = {}


def _engine(d):
    """one engine per feature count (the features go in as they are: d floats in [0, 1])"""
    _require_gpu()
    if d not in _ENGINES:
        from uptune_amd.engine import BatchEngine
        _ENGINES[d] = BatchEngine(to_manip(fspace(d)), device=0, seed=1)
    return _ENGINES[d]


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def host(*ts):
    return [t.cpu().numpy() for t in ts]


def _d2h(ptr, m, dtype=np.float64):
    hip = ctypes.CDLL("libamdhip64.so")
    out = np.empty(m, dtype=dtype)
    rc = hip.hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(ptr), ctypes.c_size_t(out.nbytes), 2)
    assert rc == 0, rc
    return out


def _unload(e):
    e.gp_cons_clear()
    e.gp_feas_clear()
    e.gp_set_prune_weighted(False)


def _load(e, w, z):
    if w["thr"]:
        e.gp_cons_set(z["C"], z["thr"])
    else:
        e.gp_cons_clear()
    if w["nfail"]:
        e.gp_feas_set(z["Xf"], **w["vote"])
    else:
        e.gp_feas_clear()


def check_call(idx, top, st, ub, ex, valid, k, cand_base, score_d):
    """what holds for every pruned call against the dense device scores score_d
    (-inf on duplicates): the selection, the exact scores, the threshold"""
    kk = min(k, int(valid.sum()))
    pos = idx[:kk] - cand_base
    po.band_check(idx, top, score_d, valid, k, cand_base, 1e-9, 1e-12)
    np.testing.assert_allclose(top[:kk], score_d[pos], rtol=1e-9, atol=1e-12)
    if kk == k:
        t = np.sort(score_d[valid])[::-1][k - 1]
        assert st["threshold"] <= t + 1e-9 * abs(t) + 1e-12, (st, t)
    else:
        assert st["threshold"] == -np.inf, st
    assert np.all(ub[pos] >= st["threshold"]), "a selected candidate's bound is below the threshold"
    if not st["dense"]:
        # an exact flag says the stored bound IS the candidate's score
        e = ex[pos] != 0
        assert np.array_equal(top[:kk][e], ub[pos][e]), (top[:kk][e], ub[pos][e])


_DENSE = {}


def _dense(e, w, c, feat, dup, a):
    """the dense device posterior, constraint means, vote, weighted scores and their
    top-k with the case's rows and values loaded (once for both passes)"""
    if w["name"] not in _DENSE:
        m = c["m"]
        mu, var, score = host(*e.gp_score(feat, acq=a, dup=dup))
        i2, t2 = host(*e.topk(dev(score), c["k"], dup=dup, cand_base=c["cand_base"]))
        mu_c = host(e.gp_cons_prob(features=feat)[1])[0] if w["thr"] else np.zeros((0, m))
        p = host(e.gp_feas_prob(features=feat)[0])[0] if w["nfail"] else np.ones(m)
        _DENSE[w["name"]] = (mu, var, score, i2, t2, mu_c, p)
    return _DENSE[w["name"]]


@pytest.mark.parametrize("prune_pass", [32, 64])
@pytest.mark.parametrize("w", pw.CASES, ids=pw.case_ids())
def test_weighted_bounds_and_selection(w, prune_pass):
    c, z, r = pw.base_case(w), pw.case_data(w), pw.case_restated(w)
    cg, m, k, cb, acq, sf2 = z["cg"], c["m"], c["k"], c["cand_base"], c["acq"], c["sf2"]
    power = pw.vote_params(w)[3]
    e = _engine(c["d"])
    try:
        e.gp_set_prune_pass(prune_pass)
        e.gp_set_prune_weighted(True)
        e.gp_fit(z["X"], z["y"], lengthscale=c["ell"], sigma_f2=sf2, sigma_n2=c["sn2"], jitter=c["jitter"])
        _load(e, w, z)
        feat = dev(z["U"].T)
        dup = None if c["dup"] == "none" else dev(z["dup"])
        valid = z["dup"] == 0
        a = e.acq("ei", xi=acq["xi"], kappa=acq["kappa"])
        idx, top, st = e.gp_topk_pruned(feat, k, acq=a, dup=dup, cand_base=cb, bound_rows=c["bound_rows"])
        ub, ex = host(*e.gp_prune_bounds(m))
        idx, top = host(idx, top)
        mu_d, var_d, score_d, i2, t2, mu_c_d, p_d = _dense(e, w, c, feat, dup, a)
    finally:
        _unload(e)
    kk = min(k, int(valid.sum()))
    ns, ns_e = int(r["keep"].sum()), int(r["keep_e"].sum())
    print("%s pass %d: %s restated survivors %d (EI-only bound %d), exact %d, +inf %d" %
          (w["name"], prune_pass, st, ns, ns_e, int(ex[valid].sum()), int(np.sum(ub == np.inf))))
    # -- soundness, exact flags, duplicates
    pw.check_bounds_w(ub, ex, valid, mu_d, var_d, mu_c_d, p_d, cg, acq, sf2, power, po.PATH_TOL)
    pw.check_bounds_w(ub, ex, valid, r["mu"], r["var"], r["mu_c"], r["p"], cg, acq, sf2, power, po.ORACLE_TOL)
    if w["nfail"]:
        assert not ex.any(), "no bound is exact while failed rows are loaded"
    elif prune_pass == 64 and r["rows"] >= po.npad(c["n"]):
        # (k_prune_bound: the bound GEMM covered every row; the f32 pass keeps its tail term)
        assert ex[valid].all(), "the bound covered every row: every stored double is the exact E P"
    # -- the cap on unusable bounds: no case of this table plants one
    assert not np.any(ub == np.inf)
    # -- selection, exact scores and threshold against the dense device weighted scores
    check_call(idx, top, st, ub, ex, valid, k, cb, score_d)
    np.testing.assert_allclose(top[:kk], t2[:kk], rtol=1e-9, atol=1e-12)
    # -- selection against the restatement
    po.band_check(idx, top, r["score"], valid, k, cb, 1e-5, 1e-8)
    np.testing.assert_allclose(top[:kk], r["score"][idx[:kk] - cb], rtol=1e-5, atol=1e-9)
    # -- stats and regime
    assert st["bound_rows"] == r["rows"]
    if w["regime"] == "prunes":
        assert not st["dense"] and 0 < st["survivors"] < m, st
        assert 2 * st["survivors"] >= ns, (st, ns)
        if prune_pass == 64:   # (the f32 pass may be looser; it is held to "not dense" above)
            assert st["survivors"] <= 2 * ns, (st, ns)
    else:
        assert st["dense"] and st["survivors"] == m, st
    if w["regime"] == "flat":
        assert idx.tolist() == i2.tolist() == (cb + np.flatnonzero(valid)[:kk]).tolist()
    if w["regime"] == "few_valid":
        assert idx.tolist() == i2.tolist()
        assert sorted((idx[:kk] - cb).tolist()) == np.flatnonzero(valid).tolist()


@pytest.mark.parametrize("prune_pass", [32, 64])
@pytest.mark.parametrize("name", ["d64_l2", "d3_n129", "flat_ei0", "outlier"])
def test_identity_with_weights_that_are_one(name, prune_pass):
    """every threshold +inf, every row feasible, no failed rows: bitwise the idx,
    scores, bounds, flags and stats of the same call with nothing loaded (switch on)"""
    c = next(x for x in po.CASES if x["name"] == name)
    z = po.case_data(c)
    e = _engine(c["d"])
    try:
        e.gp_set_prune_pass(prune_pass)
        e.gp_set_prune_weighted(True)
        e.gp_fit(z["X"], z["y"], lengthscale=c["ell"], sigma_f2=c["sf2"], sigma_n2=c["sn2"], jitter=c["jitter"])
        feat = dev(z["U"].T)
        dup = None if c["dup"] == "none" else dev(z["dup"])
        a = e.acq("ei", xi=c["acq"]["xi"])

        def call():
            idx, top, st = e.gp_topk_pruned(feat, c["k"], acq=a, dup=dup, cand_base=c["cand_base"],
                                            bound_rows=c["bound_rows"])
            return host(idx, top, *e.gp_prune_bounds(c["m"])), st

        plain, st0 = call()
        rng = np.random.default_rng(3)
        C = np.stack([z["X"][:, 0] + 0.1 * rng.standard_normal(c["n"]), rng.standard_normal(c["n"])], 1)
        e.gp_cons_set(C, [np.inf, np.inf])
        info = e.gp_cons_info()
        assert info["nc"] == 2 and info["n_feasible"] == c["n"]
        loaded, st1 = call()
    finally:
        _unload(e)
    for x, y in zip(loaded, plain):
        np.testing.assert_array_equal(x, y)
    assert st1 == st0


def test_switch_off_ucb_and_stale_values():
    """off (the default): both entry points refuse as before; on: UCB is refused with
    the dense path's message and values of an earlier fit with UT_EINVAL"""
    _require_gpu()
    from uptune_amd import _lib as L
    d, n, m, k = 5, 100, 512, 8
    e = _engine(d)
    rng = np.random.default_rng(6)
    X = rng.uniform(size=(n, d))
    y = np.sum((X - 0.3) ** 2, axis=1)
    U = rng.uniform(size=(d, m))
    C, F = X[:, :1] + X[:, 1:2], rng.uniform(size=(12, d))
    e.population_init(256, round_=0)
    e.history_reset(0)
    ei, ucb = e.acq("ei"), e.acq("ucb")
    pruned = [(lambda q: e.gp_topk_pruned(dev(U), k, acq=q, bound_rows=64), "gp_topk_pruned"),
              (lambda q: e.score_round_de_pruned(m, k, round_=2, cr=0.3, acq=q, bound_rows=64),
               "score_round_de_pruned")]
    try:
        e.gp_fit(X, y, lengthscale=0.4)
        for load, what in [(lambda: e.gp_cons_set(C, [1.0]), "constraint values"),
                           (lambda: e.gp_feas_set(F), "failed rows")]:
            _unload(e)
            load()
            for call, who in pruned:
                with pytest.raises(L.UthotError, match="UT_EUNSUPPORTED: %s: %s are loaded" % (who, what)):
                    call(ei)
            e.gp_set_prune_weighted(True)
            for call, who in pruned:
                assert int((call(ei)[0] >= 0).sum()) == k
                with pytest.raises(L.UthotError, match="UT_EUNSUPPORTED: gp_score: %s are loaded.*EI only" % what):
                    call(ucb)
            e.gp_set_prune_weighted(False)          # off again: refused again
            for call, who in pruned:
                with pytest.raises(L.UthotError, match="UT_EUNSUPPORTED: %s: %s are loaded" % (who, what)):
                    call(ei)
        _unload(e)
        e.gp_set_prune_weighted(True)
        e.gp_cons_set(C, [1.0])
        e.gp_fit(X, y, lengthscale=0.4)             # a later fit: the values are stale
        for call, who in pruned:
            with pytest.raises(L.UthotError, match="UT_EINVAL.*stale"):
                call(ei)
        e.gp_cons_set(C, [1.0])
        for call, who in pruned:
            assert int((call(ei)[0] >= 0).sum()) == k
    finally:
        _unload(e)


def _mixed_space():
    return [Param("x", FLOAT, -5.0, 5.0), Param("n", INT, 1, 64), Param("flag", BOOL),
            Param("mode", ENUM, options=["a", "b", "c", 4]), Param("y", FLOAT, 0.0, 1.0),
            Param("big", INT, -100000, 2000000)]


@pytest.mark.parametrize("prune_pass", [32, 64])
def test_fused_categorical_round(monkeypatch, prune_pass):
    """ut_score_round_de_pruned on a categorical fit with one constraint and one-hot
    failed rows, against the dense round at the same round_ (its mu, var, weighted
    masked score and dup mask from round_buffers; UT_LAZY_HASH=0 so that they exist)"""
    _require_gpu()
    monkeypatch.setenv("UT_LAZY_HASH", "0")
    from uptune_amd.engine import BatchEngine
    space = _mixed_space()
    e = BatchEngine(to_manip(space), device=0, seed=12)
    try:
        e.gp_set_prune_pass(prune_pass)
        e.gp_set_prune_weighted(True)
        n, m, k, cb, nfail = 512, 8192, 48, 100, 40
        pop = ode.population_init(space, m, seed=12)
        e.population_set(dev(pop))
        X = features(space, pop[:, :n]).T
        y = np.sum((X - 0.6) ** 2, axis=1)
        hyp = dict(lengthscale=0.6, sigma_f2=1.0, sigma_n2=1e-6, jitter=1e-8)
        e.gp_fit(X, y, **hyp)
        assert e.gp_kstar_mode() == "categorical"
        rng = np.random.default_rng(4)
        C = (X[:, 0] + X[:, 7] + 0.02 * rng.standard_normal(n)).reshape(n, 1)
        thr = [float(np.median(C))]
        Xf = features(space, pop[:, n:n + nfail]).T.copy()     # one-hot in the ENUM block, 0 / 1 in the BOOL column
        e.gp_cons_set(C, thr)
        e.gp_feas_set(Xf)
        e.history_reset(0)
        e.history_add(e.hash(dev(pop[:, :n])))
        b = e.score_round_de_pruned(m, k, round_=3, cand_base=cb, cr=0.3, bound_rows=128)
        ub, ex = host(*e.gp_prune_bounds(m))
        st = b[4]
        a = e.score_round_de(m, k, round_=3, cand_base=cb, cr=0.3)
        e.sync()
        (pval, _, _, pdup, pmu, pvar, psc), ld = e.round_buffers()
        assert pdup, "an eager round keeps its dup mask"
        valid = _d2h(pdup, m, np.uint8) == 0
        mu_d, var_d, score_d = _d2h(pmu, m), _d2h(pvar, m), _d2h(psc, m)
        ncols = pop.shape[0]
        V = _d2h(pval, ncols * ld).reshape(ncols, ld)[:, :m]
        mu_c_d = host(e.gp_cons_prob(values=dev(V))[1])[0]
        p_d = host(e.gp_feas_prob(values=dev(V))[0])[0]
    finally:
        e.close()
    print("mixed pass %d: %s valid %d exact %d, p %.3f .. %.3f" % (prune_pass, st, int(valid.sum()),
                                                                 int(ex[valid].sum()), p_d.min(), p_d.max()))
    assert np.all(score_d[~valid] == -np.inf) and int(valid.sum()) > k and not np.all(valid)
    g = ConsGP(X, y, C, thr, 0.6, sigma_f2=1.0, sigma_n2=1e-6, jitter=1e-8)
    assert 0 < g.n_feasible < n and p_d.max() > p_d.min()
    cg = SimpleNamespace(tau=g.tau, f_best_c=g.f_best_c, n_feasible=g.n_feasible)
    pw.check_bounds_w(ub, ex, valid, mu_d, var_d, mu_c_d, p_d, cg, EI, 1.0, 1.0, po.PATH_TOL)
    assert not ex.any() and not np.any(ub == np.inf)
    idx, top = host(b[0], b[1])
    check_call(idx, top, st, ub, ex, valid, k, cb, score_d)
    np.testing.assert_array_equal(idx, a[0].cpu().numpy())
    np.testing.assert_allclose(top, a[1].cpu().numpy(), rtol=1e-9, atol=1e-12)
    assert st["bound_rows"] == 128 and 0 < st["survivors"] <= m


def test_technique_prunes_under_constraints_and_feasibility():
    """GpuDifferentialEvolution(prune_rows=128, constraints, feasibility, prune_weighted=True)
    requests what the same technique with prune_rows=0 requests, for three rounds;
    without prune_weighted the constructor still raises"""
    _require_gpu()
    from uptune_amd import technique as T
    from uptune_amd.driver import SearchDriver, ThresholdAccuracyMinimizeTime
    d = 3
    space = to_manip(fspace(d))
    cons = [("accuracy", ">=", 0.4)]

    def objective(cfg):      # everything right of x2 = 0.8 fails to build
        t = (cfg["x0"] - 0.2) ** 2 + (cfg["x1"] - 0.7) ** 2 + cfg["x2"]
        return {"time": float("inf") if cfg["x2"] > 0.8 else t, "accuracy": cfg["x0"] + 0.5 * cfg["x1"]}

    for kw in (dict(constraints=cons), dict(feasibility=True), dict(constraints=cons, feasibility=True)):
        with pytest.raises(ValueError, match="not with prune_rows"):
            T.GpuDifferentialEvolution(prune_rows=128, pool=4096, batch=8, population=256, seed=5, name="de", **kw)
    for bad in (dict(diversify=64), dict(acq="ucb")):
        with pytest.raises(ValueError):
            T.GpuDifferentialEvolution(prune_rows=128, prune_weighted=True, constraints=cons, feasibility=True,
                                       pool=4096, batch=8, population=256, seed=5, name="de", **bad)

    def run(prune_rows):
        tech = T.GpuDifferentialEvolution(prune_rows=prune_rows, constraints=cons, feasibility=True,
                                          prune_weighted=True, pool=4096, batch=8, population=256, seed=5,
                                          lengthscale=0.3, name="de")
        drv = SearchDriver(space, tech, objective=ThresholdAccuracyMinimizeTime(0.4), parallelism=8)
        rng = np.random.default_rng(12)
        drv.seed_results([{"x%d" % j: float(v) for j, v in enumerate(row)} for row in rng.uniform(size=(96, d))],
                         objective)
        try:
            drv.main(objective, test_limit=10 ** 6, max_generations=3)
            tech = drv.root_technique
            info = (tech.engine.gp_cons_info()["nc"], tech.engine.gp_feas_info()["nf"], tech.model.n_failed)
            return [tuple(sorted(dr.configuration.data.items())) for dr in drv.requests_query()], info
        finally:
            drv.root_technique.engine.close()

    pruned, info = run(128)
    dense, info0 = run(0)
    print("technique: %d requests, constraints %d, failed rows %d" % (len(pruned), info[0], info[1]))
    assert info == info0 and info[0] == 1 and info[1] > 0 and info[1] == info[2]
    assert len(pruned) >= 3 * 8
    assert pruned == dense


def test_closing_returns_the_memory():
    """every buffer of the weighted call is the context's: closing it returns
    ut_device_bytes to where it started"""
    _require_gpu()
    from uptune_amd.engine import BatchEngine
    d, n, m, k = 6, 300, 3000, 16
    e = _engine(d)
    base = e.device_bytes()
    rng = np.random.default_rng(8)
    X = rng.uniform(size=(n, d))
    y = np.sum((X - 0.3) ** 2, axis=1)
    f = BatchEngine(to_manip(fspace(d)), device=0, seed=8)
    try:
        f.gp_set_prune_weighted(True)
        f.gp_fit(X, y, lengthscale=0.5)
        f.gp_cons_set(np.stack([X[:, 0] + X[:, 1], X[:, 2]], 1), [1.0, 0.7])
        f.gp_feas_set(rng.uniform(size=(33, d)), power=2.0)
        for pp in (32, 64):
            f.gp_set_prune_pass(pp)
            idx, top, st = f.gp_topk_pruned(dev(rng.uniform(size=(d, m))), k, bound_rows=128)
            assert int((idx >= 0).sum()) == k
        assert f.device_bytes() > base
    finally:
        f.close()
    assert e.device_bytes() == base
