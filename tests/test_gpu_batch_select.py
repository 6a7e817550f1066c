"""Batch-aware selection on the device (csrc/gp_batch.hip, ut_gp_select_batch)
against the rule restated over oracle/gp.py (tests/_batch_oracle.py; the
reference has no GP: SURVEY F2).

The replay check walks the device's own pick sequence through the oracle, so a
near-tie that the two sides break differently does not fail it: at each step
the device's score must be the oracle's score of that pick, and that pick must
be (nearly) the oracle's best, both within rtol |s| + rtol |s_first|.  The
absolute term is there because late EI picks underflow (down to 1e-143 of the
first score).  rtol is the project's tier from test_gpu_lml.py: 1e-9 at
sigma_n2 = 1e-2, 1e-5 at sigma_n2 = 1e-6.

The oracle's own error at these shapes, against the same rule carried in
long double (factor, solves, Sigma and the recursion; acquisition in fp64),
walking the fp64 picks, as |s - s_ld| / |s_first| over the four cases, EI and
UCB: at most 1.8e-12 at sigma_n2 = 1e-2 (three orders inside 1e-9); at
sigma_n2 = 1e-6 at most 2.5e-12 except (321, 3, 1024, 128), 3.9e-10 for UCB and
2.3e-7 for EI, whose first score is itself only 1.4e-7 -- the tie case, still
a factor 40 inside 1e-5.  Relative to each score itself (scores above 1e-6 of
the first) the same runs give at most 1.2e-11 and, for that case, 2.3e-7; the
underflowing EI tail below that is what the absolute term is for.  Variances
at pick time: at most 6.0e-15 and 6.0e-13 absolute.

Variances are differences of quantities of size sigma_f2 = 1, so out_var is
held to rtol (|var| + sigma_f2)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _batch_oracle as B  # noqa: E402
import _lml_oracle as O  # noqa: E402
from _spaces import to_manip  # noqa: E402
from oracle import gp as ogp  # noqa: E402
from oracle.space import BOOL, ENUM, FLOAT, Param  # noqa: E402

pytestmark = pytest.mark.gpu

# (n, d, p, k, ell): one padded block; d and p off the tile sizes; npad = 384; the caps, npad = 256
CASES = [(100, 5, 256, 32, 0.5), (200, 37, 300, 64, 2.0), (321, 3, 1024, 128, 0.3), (130, 5, 4096, 256, 0.5)]
TIERS = [(1e-2, 1e-9), (1e-6, 1e-5)]       # (sigma_n2, rtol)
KINDS = ["ei", "ucb"]
UT_EINVAL, UT_ENOMEM = -1, -6

_ENGINES = {}
_RUNS = {}
_GPS = {}


def engine(d, fresh=False):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from uptune_amd.engine import BatchEngine
    if fresh:
        return BatchEngine(to_manip([Param(f"u{k}", FLOAT, 0.0, 1.0) for k in range(d)]), device=0, seed=0)
    if d not in _ENGINES:
        _ENGINES[d] = engine(d, fresh=True)
    _ENGINES[d].gp_set_precision(64)
    return _ENGINES[d]


def dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def host(*ts):
    return [t.cpu().numpy() for t in ts]


def dup7(p):
    dup = np.zeros(p, dtype=np.uint8)
    dup[::7] = 1
    return dup


def gp_of(n, d, ell, sn2):
    key = (n, d, ell, sn2)
    if key not in _GPS:
        X, y = O.data(n, d)
        _GPS[key] = ogp.GP(X, y, lengthscale=ell, sigma_n2=sn2)
    return _GPS[key]


def fit(e, n, d, ell, sn2):
    X, y = O.data(n, d)
    e.gp_fit(X, y, lengthscale=ell, sigma_n2=sn2)


def run(case, sn2, kind):
    """the device's picks of a case and the oracle's, free and walked along the
    device's sequence; computed once, shared by the tests, never written"""
    key = (case, sn2, kind)
    if key in _RUNS:
        return _RUNS[key]
    n, d, p, k, ell = case
    U, dup = B.pool(n, p, d), dup7(p)
    e = engine(d)
    fit(e, n, d, ell, sn2)
    pos, score, var = host(*e.gp_select_batch(dev(U.T), k, acq=e.acq(kind), dup=dev(dup)))
    g = gp_of(n, d, ell, sn2)
    free = B.select(g, U, k, sn2, kind=kind, dup=dup)
    walk = free if np.array_equal(free["pos"], pos) else B.select(g, U, k, sn2, kind=kind, dup=dup, forced=pos)
    for a in (pos, score, var):
        a.setflags(write=False)
    _RUNS[key] = dict(pos=pos, score=score, var=var, free=free, walk=walk, dup=dup)
    return _RUNS[key]


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("sn2,rtol", TIERS)
@pytest.mark.parametrize("case", CASES)
def test_replay(case, sn2, rtol, kind):
    n, d, p, k, ell = case
    r = run(case, sn2, kind)
    pos, score, var, w = r["pos"], r["score"], r["var"], r["walk"]
    assert (pos >= 0).all() and (w["pos"] == pos).all()      # k < the non-dup candidates: no slot is empty
    bound = rtol * np.abs(w["score"]) + rtol * abs(w["score"][0])
    e_score = np.abs(score - w["score"])
    e_best = w["best"] - w["score"]
    e_var = np.abs(var - w["var"])
    print(f"{case} sn2={sn2:g} {kind}: score err / bound {np.max(e_score / bound):.3e}, "
          f"best - pick / bound {np.max(e_best / bound):.3e}, var err {np.max(e_var):.3e}, "
          f"last / first score {score[-1] / score[0]:.3e}, picks equal the oracle's: "
          f"{np.array_equal(r['free']['pos'], pos)}")
    assert (e_score <= bound).all()
    assert (e_best <= bound).all()
    assert (e_var <= rtol * (np.abs(w["var"]) + 1.0)).all()
    # properties
    assert len(set(pos.tolist())) == k
    assert not r["dup"][pos].any()
    assert (np.diff(score) <= 0.0).all()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES)
def test_exact_picks(case, kind):
    r = run(case, 1e-2, kind)
    gap = float(np.min(r["free"]["gap"]))
    print(f"{case} {kind}: smallest relative gap {gap:.3e}")
    assert gap >= 1e-6
    np.testing.assert_array_equal(r["pos"], r["free"]["pos"])


def test_ties_proceed_by_position():
    """(321, 3, 1024, 128) with EI at sigma_n2 = 1e-6: the late scores underflow
    to exactly 0 on both sides, and a tie goes to the smallest position"""
    r = run(CASES[2], 1e-6, "ei")
    zo, zd = r["free"]["score"] == 0.0, r["score"] == 0.0
    print(f"zero scores: oracle {zo.sum()}, device {zd.sum()}")
    assert zo.sum() >= 100 and zd.sum() >= zo.sum() // 2     # the premise, and the device takes that path too
    assert (np.diff(r["pos"][zd]) > 0).all()
    assert (np.diff(r["free"]["pos"][zo]) > 0).all()


@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("case", CASES[:2])
def test_first_pick_is_the_plain_top1_and_calls_repeat(case, kind):
    n, d, p, k, ell = case
    U, dup = dev(B.pool(n, p, d).T), dev(dup7(p))
    e = engine(d)
    fit(e, n, d, ell, 1e-2)
    acq = e.acq(kind)
    before = host(*e.gp_score_values(U, acq=acq, dup=dup))
    top1 = e.topk(dev(before[2]), 1, dup=dup)[0].cpu().item()
    a = host(*e.gp_select_batch(U, k, acq=acq, dup=dup))
    b = host(*e.gp_select_batch(U, k, acq=acq, dup=dup))
    after = host(*e.gp_score_values(U, acq=acq, dup=dup))
    assert a[0][0] == top1
    for x, y in zip(a, b):                      # two calls: the same bits
        assert x.tobytes() == y.tobytes()
    for x, y in zip(before, after):             # the fit and the scoring path are as they were
        assert x.tobytes() == y.tobytes()
    r = run(case, 1e-2, kind)                   # ... and as an earlier engine state gave them
    assert a[0].tolist() == r["pos"].tolist() and a[1].tobytes() == r["score"].tobytes()


def test_round_buffers_stay_as_they_are():
    import torch
    n, d, p, k, ell = CASES[0]
    e = engine(d, fresh=True)
    fit(e, n, d, ell, 1e-2)
    e.population_init(64, round_=0)
    idx, top, dig, vals = e.score_round_de(512, 8)
    ptrs, ld = e.round_buffers()
    torch.cuda.synchronize()

    hip = ctypes.CDLL("libamdhip64.so")

    def snap():   # values, (features), digests, dup, mu, var, score: whichever the round kept
        out = []
        for q, nbytes in zip(ptrs, [8 * d * ld, 0, 32 * ld, ld, 8 * ld, 8 * ld, 8 * ld]):
            if q and nbytes:
                buf = np.empty(nbytes, dtype=np.uint8)
                assert hip.hipMemcpy(ctypes.c_void_p(buf.ctypes.data), ctypes.c_void_p(q), ctypes.c_size_t(nbytes), 2) == 0
                out.append(buf.tobytes())
        assert len(out) >= 4
        return out
    s0 = snap()
    e.gp_select_batch(dev(B.pool(n, p, d).T), k)
    torch.cuda.synchronize()
    assert e.round_buffers() == (ptrs, ld)
    assert snap() == s0
    assert [t.cpu().tolist() for t in e.score_round_de(512, 8)] == [t.cpu().tolist() for t in (idx, top, dig, vals)]
    e.close()


@pytest.mark.parametrize("sn2,rtol", TIERS)
def test_same_after_precision_8_and_a_refit(sn2, rtol):
    case = CASES[0]
    n, d, p, k, ell = case
    r = run(case, sn2, "ei")
    e = engine(d)
    e.gp_set_precision(8)
    fit(e, n, d, ell, sn2)
    pos, score, var = host(*e.gp_select_batch(dev(B.pool(n, p, d).T), k, acq=e.acq("ei"), dup=dev(dup7(p))))
    e.gp_set_precision(64)
    assert pos.tolist() == r["pos"].tolist()
    assert (np.abs(score - r["score"]) <= rtol * np.abs(r["score"]) + rtol * abs(r["score"][0])).all()


def test_categorical_space_with_either_kstar(monkeypatch):
    import torch
    from uptune_amd.engine import BatchEngine
    space = [Param("a", ENUM, options=["x", "y", "z"]), Param("b", BOOL), Param("c", FLOAT, 0.0, 1.0),
             Param("e", ENUM, options=list("pqrst")), Param("f", FLOAT, -2.0, 2.0)]
    rng = np.random.default_rng(11)
    out = {}
    for flag in ("1", "0"):
        monkeypatch.setenv("UT_CAT_KSTAR", flag)
        e = BatchEngine(to_manip(space), device=0, seed=3)
        e.population_init(512, round_=0)
        vals = e.population_get().contiguous()                 # [ncols][512] values in their domains
        tr, sl = vals[:, :150].contiguous(), vals[:, 150:450].contiguous()
        X = e.encode(tr).cpu().numpy().T
        y = np.sum((X - 0.4) ** 2, axis=1) + 0.01 * rng.standard_normal(150) if flag == "1" else out["y"]
        out["y"] = y
        e.gp_fit(X, y, lengthscale=1.2, sigma_n2=1e-2)
        assert e.gp_kstar_mode() == ("categorical" if flag == "1" else "dense")
        dup = dev(dup7(300))
        _, _, s = e.gp_score_values(sl, acq=e.acq("ei"), dup=dup)
        top1 = e.topk(s, 1, dup=dup)[0].cpu().item()
        res = host(*e.gp_select_batch(sl, 48, acq=e.acq("ei"), dup=dup))
        assert res[0][0] == top1
        # against the oracle on the encoded features
        g = ogp.GP(X, y, lengthscale=1.2, sigma_n2=1e-2)
        w = B.select(g, e.encode(sl).cpu().numpy().T, 48, 1e-2, dup=dup7(300), forced=res[0])
        bound = 1e-9 * np.abs(w["score"]) + 1e-9 * abs(w["score"][0])
        assert (np.abs(res[1] - w["score"]) <= bound).all() and (w["best"] - w["score"] <= bound).all()
        out[flag] = res
        e.close()
        torch.cuda.synchronize()
    assert out["1"][0].tolist() == out["0"][0].tolist()
    bound = 1e-9 * np.abs(out["0"][1]) + 1e-9 * abs(out["0"][1][0])
    assert (np.abs(out["1"][1] - out["0"][1]) <= bound).all()


def test_edges():
    n, d, p, k, ell = CASES[0]
    U, dup = B.pool(n, p, d), dup7(p)
    g = gp_of(n, d, ell, 1e-2)
    e = engine(d)
    fit(e, n, d, ell, 1e-2)
    # k = p over a small shortlist: every candidate, each once
    pos, score, var = host(*e.gp_select_batch(dev(U[:40].T), 40))
    w = B.select(g, U[:40], 40, 1e-2, forced=pos)
    assert sorted(pos.tolist()) == list(range(40))
    assert (np.abs(score - w["score"]) <= 1e-9 * np.abs(w["score"]) + 1e-9 * abs(w["score"][0])).all()
    # p = 1 and k = 1
    pos, score, var = host(*e.gp_select_batch(dev(U[:1].T), 1))
    mu1, var1 = g.posterior(U[:1])
    assert pos.tolist() == [0] and abs(var[0] - var1[0]) <= 1e-9 * (var1[0] + 1.0)
    pos, score, var = host(*e.gp_select_batch(dev(U.T), 1, dup=dev(dup)))
    assert pos.tolist() == [run(CASES[0], 1e-2, "ei")["pos"][0]]
    # more picks than candidates that are not dup: the rest of the slots are empty
    few = np.ones(p, dtype=np.uint8)
    few[[5, 77, 200]] = 0
    pos, score, var = host(*e.gp_select_batch(dev(U.T), 6, dup=dev(few)))
    assert sorted(pos[:3].tolist()) == [5, 77, 200] and pos[3:].tolist() == [-1, -1, -1]
    assert (score[3:] == -np.inf).all() and np.isnan(var[3:]).all() and np.isfinite(score[:3]).all()
    assert pos.tolist() == B.select(g, U, 6, 1e-2, dup=few)["pos"].tolist()
    # every candidate dup: all empty
    pos, score, var = host(*e.gp_select_batch(dev(U.T), 4, dup=dev(np.ones(p, dtype=np.uint8))))
    assert pos.tolist() == [-1] * 4 and (score == -np.inf).all() and np.isnan(var).all()


def test_failed_fit_leaves_every_slot_empty():
    n, d, p, k, ell = CASES[0]
    X, y = O.data(n, d)
    e = engine(d, fresh=True)
    e.gp_fit(X, y, lengthscale=ell, sigma_n2=-2.0, jitter=0.0, wait=False)   # not positive definite
    pos, score, var = host(*e.gp_select_batch(dev(B.pool(n, p, d).T), 8))   # enqueued behind the failing fit
    assert pos.tolist() == [-1] * 8 and (score == -np.inf).all() and np.isnan(var).all()
    assert not e.gp_fit_ok()
    e.close()


def test_bad_arguments_and_failed_allocation():
    import torch
    from uptune_amd import _lib as L
    n, d, p, k, ell = CASES[0]
    e = engine(d, fresh=True)
    U = dev(B.pool(n, p, d).T)
    acq = e.acq("ei")
    out = torch.empty(k, dtype=torch.int64, device="cuda:0")

    def call(values=U.data_ptr(), ld=p, pp=p, a=ctypes.byref(acq), kk=k, o=out.data_ptr()):
        return e.lib.ut_gp_select_batch(e.ctx, values, ld, pp, a, None, kk, o, None, None)
    # no fit at all: what ut_gp_score_values returns
    s = torch.empty(p, dtype=torch.float64, device="cuda:0")
    assert call() == e.lib.ut_gp_score_values(e.ctx, U.data_ptr(), p, p, ctypes.byref(acq), None, None, None,
                                              s.data_ptr()) == UT_EINVAL
    fit(e, n, d, ell, 1e-2)
    for bad in (dict(pp=0), dict(kk=0), dict(kk=p + 1), dict(pp=4097, ld=4097, kk=1), dict(values=None),
                dict(a=None), dict(o=None), dict(ld=p - 1)):
        assert call(**bad) == UT_EINVAL, bad
    with pytest.raises(ValueError):                      # a column count that is not the space's
        e.gp_select_batch(U[:d - 1], k)
    # the scratch goes through the counted allocations
    assert e.lib.ut_debug_fail_alloc(e.ctx, 1) == 0
    assert call() == UT_ENOMEM
    assert e.lib.ut_debug_fail_alloc(e.ctx, 1) == 0
    with pytest.raises(L.UthotError, match="UT_ENOMEM"):
        e.gp_select_batch(U, k)
    pos, score, var = host(*e.gp_select_batch(U, k))     # ... and the following call succeeds
    assert pos.tolist() == B.select(gp_of(n, d, ell, 1e-2), B.pool(n, p, d), k, 1e-2)["pos"].tolist()
    e.close()


def test_diversity_on_a_clustered_pool():
    """256 candidates in 8 clusters of spread 1e-3: the plain top-16 is one
    cluster; the conditioned picks spread over them (the oracle: 7)"""
    n, d = 100, 5
    rng = np.random.default_rng(5)
    U = np.repeat(rng.uniform(size=(8, d)), 32, axis=0) + 1e-3 * rng.standard_normal((256, d))
    ell = 0.3 * np.sqrt(5)
    e = engine(d)
    fit(e, n, d, ell, 1e-2)
    _, _, s = e.gp_score_values(dev(U.T), acq=e.acq("ei"))
    plain = e.topk(s, 16)[0].cpu().numpy()
    assert len(set((plain // 32).tolist())) == 1
    pos = e.gp_select_batch(dev(U.T), 16, acq=e.acq("ei"))[0].cpu().numpy()
    want = B.select(gp_of(n, d, ell, 1e-2), U, 16, 1e-2)["pos"]
    print("clusters: device", sorted(set((pos // 32).tolist())), "oracle", sorted(set((want // 32).tolist())))
    assert len(set((want // 32).tolist())) == 7
    assert len(set((pos // 32).tolist())) >= 4
