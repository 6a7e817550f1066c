"""ut_tpe_fit / ut_tpe_score / ut_tpe_get (csrc/tpe.hip) against tests/_tpe_oracle.py
(its docstring derives the bound): at the sort's power-of-two edges (s + 1 = 64,
65, 1024, 1025), the scoring tile (1024) + 1 and one LDS stage (1024) + 3.
ln(w / Z) is held to 16 ulps of its own value; every case has |ln(w / Z)| > 0.25,
so that is no tighter than 64 ulps of w / Z.  Needs a GPU."""
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _tpe_oracle as TO  # noqa: E402

_ENGINES, _RUNS = {}, {}


def _engine(space="mixed"):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if space not in _ENGINES:
        from uptune_amd import manipulator as M, spaces
        from uptune_amd.engine import BatchEngine
        man = spaces.gcc() if space == "gcc" else M.ConfigurationManipulator(
            list(spaces.perm_mixed().params) + [M.EnumParameter("pair", ["x", "y"]),
                                                M.EnumParameter("many", list(range(40))),
                                                M.PowerOfTwoParameter("p2", 1, 1024)])
        _ENGINES[space] = BatchEngine(man, seed=3)
    return _ENGINES[space]


def _uniform(n, d, m, seed=0, **kw):
    rng = np.random.default_rng(1000 * n + d + seed)
    return dict(X=rng.uniform(size=(n, d)), y=rng.normal(size=n), F=rng.uniform(size=(m, d)), kw=kw)


def _special(n=150):
    rng = np.random.default_rng(7)
    X = np.c_[np.full(n, 0.5), rng.choice([0.1, 0.5, 0.9], size=n), rng.choice([0.0, 0.3, 1.0], size=n),
              0.5 + 1e-4 * rng.uniform(size=n)]
    F = rng.uniform(size=(65, 4))
    F[0], F[1] = 0.0, 1.0        # far from the cluster: only the prior's term is left in f32
    return dict(X=X, y=rng.normal(size=n), F=F, kw={})


def _from_space(space, n, m, rows=None):
    e = _engine(space)
    if rows is None:
        e.population_init(n + m, round_=1)
        vals = e.population_get()[:, :n + m].contiguous()
    else:
        vals = torch.from_numpy(np.ascontiguousarray(rows[:, :n + m])).cuda()
    feat = e.encode(vals).T.contiguous().cpu().numpy()
    rng = np.random.default_rng(n)
    return dict(X=feat[:n], y=rng.normal(size=n) + feat[:n, 0], F=feat[n:], kw={}, kinds=e.tpe_kinds())


def _onehot(rng=np.random.default_rng(9)):
    hot = lambda k: np.eye(10)[rng.integers(0, 10, size=(k, 20))].reshape(k, 200)   # noqa: E731
    return dict(X=hot(60), y=rng.normal(size=60), F=hot(63), kw={}, kinds=np.tile([10] + [-1] * 9, 20))


CASES = {
    "n2_d1_m1": lambda: dict(X=np.array([[0.25], [0.8]]), y=np.array([1.0, 0.0]), F=np.array([[0.6]]), kw={}),
    "n37_d17_m63": lambda: _uniform(37, 17, 63),
    "n37_d65_m65": lambda: _uniform(37, 65, 65),
    "n37_d3_tile_plus_1_ld_dup": lambda: dict(_uniform(37, 3, 1025), ld=1100, dup=True),
    "n1000_d3_m65": lambda: _uniform(1000, 3, 65),
    "sort_64_1024": lambda: _uniform(1086, 2, 17, n_good_max=63),
    "sort_65_1025": lambda: _uniform(1088, 2, 17, n_good_max=64),
    "special_columns": _special,
    "mixed_space": lambda: _from_space("mixed", 80, 63),
    "onehot_d200": _onehot,
    "gcc_300_rows": lambda: _from_space("gcc", 300, 39, rows=np.load(
        os.path.join(os.path.dirname(__file__), "golden", "gcc_rows.npz"))["values"]),
}


def _run(name):
    """the case's data, its oracle and what the device gave, both tiers (computed once)"""
    if name in _RUNS:
        return _RUNS[name]
    e = _engine()
    c = CASES[name]()
    m, d = c["F"].shape
    feat = torch.zeros(d, c.get("ld", m), dtype=torch.float64)
    feat[:, :m] = torch.from_numpy(np.ascontiguousarray(c["F"].T))
    dup = (torch.arange(m) % 5 == 0).to(torch.uint8).cuda() if c.get("dup") else None
    out = {"case": c, "oracle": TO.Fit(c["X"], c["y"], c.get("kinds"), **c["kw"]), "dup": dup}
    for tier in (64, 32):
        e.tpe_fit(c["X"], c["y"], kinds=c.get("kinds"), precision=tier, **c["kw"])
        out[tier] = [t.cpu().numpy() for t in e.tpe_score(feat.cuda(), dup=dup, m=m, parts=True)]
    out["get"] = {(j, s): e.tpe_get(j, s) for j in range(d) for s in range(2) if out["oracle"].kinds[j] >= 0}
    _RUNS[name] = out
    return out


@pytest.mark.parametrize("name", sorted(CASES))
def test_fit_equals_the_oracle(name):
    r = _run(name)
    worst = {"lnw": 0.0, "logp": 0.0}
    ulps = lambda got, want: float(np.max(np.abs(got.astype(TO.LD) - want)   # noqa: E731
                                          / np.spacing(np.abs(want.astype(np.float64)))))
    for (j, s), (mu, sg, lw) in r["get"].items():
        wmu, wsg, wlw = r["oracle"].components(j, s)
        assert len(lw) == len(wlw)
        if wmu is None:
            worst["logp"] = max(worst["logp"], ulps(lw, wlw))
            continue
        a, b = np.lexsort((sg, mu)), np.lexsort((wsg, wmu))
        np.testing.assert_array_equal(mu[a].view(np.int64), wmu[b].view(np.int64))
        np.testing.assert_array_equal(sg[a].view(np.int64), wsg[b].view(np.int64))
        assert float(np.min(np.abs(wlw))) > 0.25
        worst["lnw"] = max(worst["lnw"], ulps(lw[a], wlw[b]))
    print(name, "ulps", worst)
    assert worst["lnw"] <= 16 and worst["logp"] <= 4


@pytest.mark.parametrize("name", sorted(CASES))
def test_scores_are_within_the_tiers_bound(name):
    r = _run(name)
    dup = None if r["dup"] is None else r["dup"].cpu().numpy().astype(bool)
    for tier in (64, 32):
        want, bound = r["oracle"].score(r["case"]["F"], tier)
        ratio = []
        for k, (got, w, b) in enumerate(zip(r[tier], want, bound)):
            if k == 0 and dup is not None:
                assert (got[dup] == -np.inf).all()
                got, w, b = got[~dup], w[~dup], b[~dup]
            assert np.isfinite(got).all()
            ratio.append(float(np.max(np.abs(got.astype(TO.LD) - w) / b)))
        print(name, "tier", tier, "error / bound of score, logl, logg", ratio, "largest bound", float(bound[0].max()))
        assert max(ratio) <= 1.0


@pytest.mark.parametrize("name", sorted(CASES))
def test_f32_top16_is_the_fp64_tiers(name):
    r = _run(name)
    s64, s32 = r[64][0], r[32][0]
    bound = np.asarray(r["oracle"].score(r["case"]["F"], 32)[1][0], dtype=np.float64)
    k = min(16, len(s64))
    top32, kth = set(np.argsort(-s32, kind="stable")[:k]), np.sort(s64)[::-1][k - 1]
    assert set(np.flatnonzero(s64 > kth + 2 * bound)) <= top32
    assert not set(np.flatnonzero(s64 < kth - 2 * bound)) & top32


def test_refusals_leave_the_previous_fit():
    from uptune_amd import _lib as L
    from uptune_amd.engine import BatchEngine
    from uptune_amd.manipulator import ConfigurationManipulator, FloatParameter
    e = BatchEngine(ConfigurationManipulator([FloatParameter("u", 0.0, 1.0)]), seed=1)
    feat = torch.rand(3, 40, dtype=torch.float64).cuda()
    with pytest.raises(L.UthotError, match="UT_EINVAL"):
        e.tpe_score(feat)                      # before any fit
    c = _uniform(37, 3, 1)
    e.tpe_fit(c["X"], c["y"], kinds=None)
    before = e.tpe_score(feat).cpu().numpy()
    nan_y, big, hot = c["y"].copy(), c["X"].copy(), np.c_[c["X"][:, :1], np.ones((37, 2))]
    nan_y[5], big[4, 1] = np.nan, 1.5
    for X, y, kinds in ((c["X"][:1], c["y"][:1], None), (c["X"], nan_y, None), (big, c["y"], None),
                        (hot, c["y"], [0, 2, -1]), (np.zeros((8300, 1)), np.arange(8300.0), None)):
        with pytest.raises(L.UthotError, match="UT_EINVAL"):
            e.tpe_fit(X, y, kinds=kinds)
    with pytest.raises(L.UthotError, match="UT_EINVAL"):
        e.tpe_score(feat[:2])                  # the wrong d
    assert e.tpe_info()["n_l"] == 4 and e.tpe_info()["n_g"] == 33
    np.testing.assert_array_equal(e.tpe_score(feat).cpu().numpy().view(np.int64), before.view(np.int64))
    e.close()
