"""ut_gp_topk_pruned / ut_score_round_de_pruned, every bound per candidate
(ut_gp_prune_bounds), on the case table of tests/_prune_oracle.py: scales,
fit and batch shapes at the tile edges, ties, fewer valid candidates than k,
candidates the f32 pass cannot bound, and the fused categorical round; at both
bound passes.  References: the device's dense gp_score + topk (path-to-path
tolerance) and oracle/gp.py (the fp64 tier's).  test_prune_oracle_cpu.py proves
on the reference alone that every case sits in its regime and that its
selection is decidable, so nothing here is asserted under a condition.

What the table catches, tried by hand on an MI355X.  Before the threshold of a
set with fewer than k valid entries became -inf, few_a_ucb (m = 10, k = 16,
UCB scores -2.2 .. -2.7) returned tau = 0, no survivor, idx 0..9 in index order
and -inf for every score.  A k_prune_bound32 that ignores the mean widening dmu
fails the soundness check of d6_l008, d3_n129, ucb_k0, d6_sf2_1e-3 and m257 at
pass 32.  Halving dmu, dropping its 2^-125 sf2 sum |alpha| term or the 1.001
factor of the tail fails nothing: the f32 mean is within 0.053 dmu of the fp64
mean on every candidate of the table (dmu is a worst-case bound, the roundings
it covers add up like a random walk), the flush term is below an ulp of the
mean unless sum |alpha| > 2^72, and 1.001 covers roundings of ~1e-13."""
import ctypes

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

torch = pytest.importorskip("torch")

import _prune_oracle as po  # noqa: E402
from _spaces import oracle_space, to_manip  # noqa: E402
from oracle import de as ode  # noqa: E402
from oracle import gp as ogp  # noqa: E402
from oracle.space import BOOL, ENUM, FLOAT, INT, Param, features  # noqa: E402

EI = dict(kind="ei", xi=0.0, kappa=2.0)


def _require_gpu():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")


_ENGINES = {}


def _engine(d):
    """one engine per feature count (the features go in as they are: d floats in [0, 1])"""
    _require_gpu()
    if d not in _ENGINES:
        from uptune_amd.engine import BatchEngine
        _ENGINES[d] = BatchEngine(to_manip([Param("x%d" % i, FLOAT, 0.0, 1.0) for i in range(d)]), device=0, seed=1)
    return _ENGINES[d]


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).cuda()


def _d2h(ptr, m, dtype=np.float64):
    hip = ctypes.CDLL("libamdhip64.so")
    out = np.empty(m, dtype=dtype)
    rc = hip.hipMemcpy(ctypes.c_void_p(out.ctypes.data), ctypes.c_void_p(ptr), ctypes.c_size_t(out.nbytes), 2)
    assert rc == 0, rc
    return out


def check_bounds(ub, ex, valid, mu, var, f_best, acq, sf2, tol):
    """soundness per candidate against a reference posterior within tol, and the
    exact flags' other side; duplicates hold -inf"""
    lo = po.envelope(mu, var, f_best, acq, sf2, tol)
    hi = po.envelope(mu, var, f_best, acq, sf2, tol, upper=True)
    bad = np.flatnonzero(valid & ~(ub >= lo))
    assert bad.size == 0, ("unsound bound", bad[:8], ub[bad[:8]], lo[bad[:8]])
    e = valid & (ex != 0)
    bad = np.flatnonzero(e & ~(ub <= hi))
    assert bad.size == 0, ("exact flag on a bound above the score", bad[:8], ub[bad[:8]], hi[bad[:8]])
    assert np.all(ub[~valid] == -np.inf)


def check_call(idx, top, st, ub, ex, valid, k, cand_base, score_d):
    """what holds for every pruned call against the dense device scores score_d
    (-inf on duplicates): the threshold, the exact scores, the selection"""
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


def _dense(e, c, feat, dup, a):
    """the dense device posterior, scores and top-k of the case (once for both passes)"""
    if c["name"] not in _DENSE:
        mu, var, score = e.gp_score(feat, acq=a, dup=dup)
        i2, t2 = e.topk(score, c["k"], dup=dup, cand_base=c["cand_base"])
        _DENSE[c["name"]] = [t.cpu().numpy() for t in (mu, var, score, i2, t2)]
    return _DENSE[c["name"]]


@pytest.mark.parametrize("prune_pass", [32, 64])
@pytest.mark.parametrize("c", po.CASES, ids=po.case_ids())
def test_pruned_bounds_and_selection(c, prune_pass):
    z, r = po.case_data(c), po.case_restated(c)
    g, m, k, cb, acq, sf2 = z["gp"], c["m"], c["k"], c["cand_base"], c["acq"], c["sf2"]
    e = _engine(c["d"])
    e.gp_set_prune_pass(prune_pass)
    e.gp_fit(z["X"], z["y"], lengthscale=c["ell"], sigma_f2=sf2, sigma_n2=c["sn2"], jitter=c["jitter"])
    feat = dev(z["U"].T)
    dup = None if c["dup"] == "none" else dev(z["dup"])
    valid = z["dup"] == 0
    a = e.acq(acq["kind"], xi=acq["xi"], kappa=acq["kappa"])
    idx, top, st = e.gp_topk_pruned(feat, k, acq=a, dup=dup, cand_base=cb, bound_rows=c["bound_rows"])
    ub, ex = [t.cpu().numpy() for t in e.gp_prune_bounds(m)]
    idx, top = idx.cpu().numpy(), top.cpu().numpy()
    mu_d, var_d, score_d, i2, t2 = _dense(e, c, feat, dup, a)
    kk = min(k, int(valid.sum()))
    print("%s pass %d: %s restated survivors %d, exact %d, +inf %d" %
          (c["name"], prune_pass, st, int(r["keep"].sum()), int(ex[valid].sum()), int(np.sum(ub == np.inf))))
    # -- soundness, exact flags, duplicates
    check_bounds(ub, ex, valid, mu_d, var_d, g.f_best, acq, sf2, po.PATH_TOL)
    check_bounds(ub, ex, valid, r["mu"], r["var"], g.f_best, acq, sf2, po.ORACLE_TOL)
    # -- the cap on unusable bounds
    planted = list(po.OUTLIERS) if c["recipe"] == "outlier" and prune_pass == 32 else []
    assert np.flatnonzero(ub == np.inf).tolist() == planted
    # -- threshold, exact scores, selection against the dense device path
    check_call(idx, top, st, ub, ex, valid, k, cb, score_d)
    np.testing.assert_allclose(top[:kk], t2[:kk], rtol=1e-9, atol=1e-12)
    # -- selection against the oracle
    po.band_check(idx, top, r["score"], valid, k, cb, 1e-5, 1e-8)
    np.testing.assert_allclose(top[:kk], r["score"][idx[:kk] - cb], rtol=1e-5, atol=1e-9)
    # -- stats and regime
    assert st["bound_rows"] == r["rows"]
    if c["regime"] == "prunes":
        assert not st["dense"] and 0 < st["survivors"] < m, st
        ns = int(r["keep"].sum())
        assert 2 * st["survivors"] >= ns, (st, ns)
        if prune_pass == 64:   # (the f32 pass may be looser; it is held to "not dense" above)
            assert st["survivors"] <= 2 * ns, (st, ns)
    else:
        assert st["dense"] and st["survivors"] == m, st
    if c["regime"] == "flat":
        # index order (range(cb, cb + kk) but for the duplicates in it)
        assert idx.tolist() == i2.tolist() == (cb + np.flatnonzero(valid)[:kk]).tolist()
    if c["regime"] == "few_valid":
        # exactly the valid candidates, ranked by and returned with their real scores
        assert idx.tolist() == i2.tolist()
        assert sorted((idx[:kk] - cb).tolist()) == np.flatnonzero(valid).tolist()


def test_prune_bounds_argument_errors():
    """ut_gp_prune_bounds: UT_EINVAL before any pruned call and for another m;
    pruning still refuses a fit that is not fp64 (precision 8)"""
    _require_gpu()
    from uptune_amd._lib import UthotError
    from uptune_amd.engine import BatchEngine
    e = BatchEngine(to_manip([Param("x%d" % i, FLOAT, 0.0, 1.0) for i in range(3)]), device=0, seed=2)
    with pytest.raises(UthotError, match="UT_EINVAL|no pruned call"):
        e.gp_prune_bounds(16)
    rng = np.random.default_rng(1)
    X, y = rng.uniform(size=(40, 3)), rng.standard_normal(40)
    e.gp_fit(X, y, lengthscale=0.5)
    feat = dev(rng.uniform(size=(3, 300)))
    e.gp_topk_pruned(feat, 4, bound_rows=128)
    ub, ex = e.gp_prune_bounds(300)
    assert ub.shape == (300,) and ex.dtype == torch.uint8 and bool(torch.isfinite(ub).all())
    for m in (299, 301, 0):
        with pytest.raises(UthotError, match="not the last pruned call"):
            e.gp_prune_bounds(m)
    e.gp_set_precision(8)
    e.gp_fit(X, y, lengthscale=0.5)
    with pytest.raises(UthotError, match="needs an fp64 fit"):
        e.gp_topk_pruned(feat, 4, bound_rows=128)


def _mixed_space():
    return [Param("x", FLOAT, -5.0, 5.0), Param("n", INT, 1, 64), Param("flag", BOOL),
            Param("mode", ENUM, options=["a", "b", "c", 4]), Param("y", FLOAT, 0.0, 1.0),
            Param("big", INT, -100000, 2000000)]


def _hpl_space():
    from uptune_amd import spaces
    return oracle_space(spaces.hpl64())


@pytest.mark.parametrize("prune_pass", [32, 64])
@pytest.mark.parametrize("which,ell,centre", [("mixed", 0.6, 0.6), ("hpl", 1.0, 0.4)])
def test_fused_round_bounds(monkeypatch, which, ell, centre, prune_pass):
    """ut_score_round_de_pruned on a categorical fit: the only place the f32
    bound's categorical terms (Kc = dpad + 1, |c0|) are held per candidate.
    The reference is the dense round at the same round_ (its mu, var, masked
    score and dup mask from round_buffers; UT_LAZY_HASH=0 so that they exist)."""
    _require_gpu()
    monkeypatch.setenv("UT_LAZY_HASH", "0")
    from uptune_amd.engine import BatchEngine
    space = _mixed_space() if which == "mixed" else _hpl_space()
    e = BatchEngine(to_manip(space), device=0, seed=12)
    e.gp_set_prune_pass(prune_pass)
    n, m, k, cb = 512, 8192, 48, 100
    pop = ode.population_init(space, m, seed=12)
    e.population_set(dev(pop))
    X = features(space, pop[:, :n]).T
    y = np.sum((X - centre) ** 2, axis=1)
    hyp = dict(lengthscale=ell, sigma_f2=1.0, sigma_n2=1e-6, jitter=1e-8)
    e.gp_fit(X, y, **hyp)
    assert e.gp_kstar_mode() == "categorical"
    e.history_reset(0)
    e.history_add(e.hash(dev(pop[:, :n])))
    b = e.score_round_de_pruned(m, k, round_=3, cand_base=cb, cr=0.3, bound_rows=128)
    ub, ex = [t.cpu().numpy() for t in e.gp_prune_bounds(m)]
    st = b[4]
    a = e.score_round_de(m, k, round_=3, cand_base=cb, cr=0.3)
    e.sync()
    (_, _, _, pdup, pmu, pvar, psc), _ = e.round_buffers()
    assert pdup, "an eager round keeps its dup mask"
    valid = _d2h(pdup, m, np.uint8) == 0
    mu_d, var_d, score_d = _d2h(pmu, m), _d2h(pvar, m), _d2h(psc, m)
    print("%s pass %d: %s valid %d exact %d" % (which, prune_pass, st, int(valid.sum()), int(ex[valid].sum())))
    assert np.all(score_d[~valid] == -np.inf) and int(valid.sum()) > k
    assert which != "mixed" or not np.all(valid)   # (the mixed space's round has duplicates to mask)
    f_best = ogp.GP(X, y, **hyp).f_best
    check_bounds(ub, ex, valid, mu_d, var_d, f_best, EI, 1.0, po.PATH_TOL)
    assert not np.any(ub == np.inf)
    idx, top = b[0].cpu().numpy(), b[1].cpu().numpy()
    check_call(idx, top, st, ub, ex, valid, k, cb, score_d)
    np.testing.assert_allclose(top, a[1].cpu().numpy(), rtol=1e-9, atol=1e-12)
    assert st["bound_rows"] == 128 and 0 < st["survivors"] <= m
