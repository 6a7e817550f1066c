"""Thompson sampling on the device (csrc/gp_ts.hip: ut_gp_ts_draw / _eval /
_select / _read) against the rule restated in tests/_ts_oracle.py (the
reference has no GP: SURVEY F2).

Draws: bit for bit.  A: against the long-double solve from the device's own
draws and ys, at the project's tiers (rtol times the path's largest |a|).
Eval: against the long-double paths evaluated from the device's own Z, b,
Theta and A, so the check isolates k_ts_paths; per element the error is at
most 4 x the fp64 numpy restatement's largest error on the same case
(_fit_cases.py's rule) plus COS_ERR sqrt(2 sf2 / D) sum_j |Theta[s][j]| (the
long-double side uses the true cosine).  Neither term comes from the kernel.
Select: exactly the rule applied on the host to the device's own ut_gp_ts_eval
output; the long-double oracle's picks wherever its gap between best and
second-best remaining exceeds twice that tolerance, and within tolerance of
its best remaining value elsewhere -- at most 1 pick in 20 over the table."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _ts_oracle as T  # noqa: E402
from _spaces import to_manip  # noqa: E402

pytestmark = pytest.mark.gpu
LD = T.LD
UT_EINVAL = -1

_ENGINES = {}
_RUNS = {}
_SECOND = {}      # case -> (picks that took the near-tie branch, picks)


def dev(a):
    import torch
    return torch.from_numpy(np.array(a)).to("cuda:0")


def engine(c, fresh=False):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from uptune_amd.engine import BatchEngine
    if fresh or c["name"] not in _ENGINES:
        e = BatchEngine(to_manip(T.data(c)["space"]), device=0, seed=T.seed_of(c))
        if fresh:
            return e
        _ENGINES[c["name"]] = e
    return _ENGINES[c["name"]]


def fit(e, c, **kw):
    z = T.data(c)
    e.gp_fit(z["X"], z["y"], lengthscale=z["ell"], sigma_f2=c["sf2"], sigma_n2=c["sn2"], jitter=c["jitter"], **kw)


def run(c):
    """the device's draws, weights, path values and picks of a case, and the two restatements from the device's
    own operands; computed once, shared by the tests, never written"""
    if c["name"] in _RUNS:
        return _RUNS[c["name"]]
    assert T.have_longdouble()
    z = T.data(c)
    e = engine(c)
    e.gp_set_precision(64)
    fit(e, c)
    e.gp_ts_draw(c["q"], c["D"], round_=T.round_of(c))
    dr = {k: e.gp_ts_read(k) for k in ("Z", "b", "Theta", "Eps")}
    A = e.gp_ts_read("A")
    ys = e.gp_fit_read("YS")[0].cpu().numpy()[:c["n"]].copy()
    cand, dup = dev(z["cand"]), dev(z["dup"])
    F = e.gp_ts_eval(cand).cpu().numpy()
    pos, f = (t.cpu().numpy() for t in e.gp_ts_select(cand, c["q"], dup=dup))
    fld = T.Fit(z["X"], z["y"], z["ell"], c["sf2"], c["sn2"], c["jitter"], LD, ys=ys)
    f64 = T.Fit(z["X"], z["y"], z["ell"], c["sf2"], c["sn2"], c["jitter"], np.float64, ys=ys)
    Fld = T.evaluate(fld, dr, A, z["U"])
    F64 = T.evaluate(f64, dr, A, z["U"])
    e_ref = float(np.max(np.abs(F64.astype(LD) - Fld)))
    amp = np.sqrt(2.0 * c["sf2"] / c["D"])
    tol = 4.0 * e_ref + T.COS_ERR * amp * np.sum(np.abs(dr["Theta"]), axis=1)          # [q]
    r = dict(dr=dr, A=A, ys=ys, F=F, pos=pos, f=f, fld=fld, Fld=Fld, e_ref=e_ref, tol=tol)
    for a in list(dr.values()) + [A, ys, F, pos, f, tol]:
        a.setflags(write=False)
    _RUNS[c["name"]] = r
    return r


@pytest.mark.parametrize("c", T.CASES, ids=T.ids())
def test_draws_bit_for_bit(c):
    r = run(c)
    want = T.draws(T.seed_of(c), c["n"], T.data(c)["d"], c["q"], c["D"], T.round_of(c))
    for k in ("Z", "b", "Theta", "Eps"):
        assert r["dr"][k].shape == want[k].shape, k
        assert np.array_equal(r["dr"][k].view(np.uint64), want[k].view(np.uint64)), k


@pytest.mark.parametrize("c", T.CASES, ids=T.ids())
def test_weights_at_the_tier(c):
    rtol = dict(T.TIERS)[c["sn2"]]
    r = run(c)
    want = T.weights(r["fld"], r["dr"])
    scale = np.max(np.abs(want), axis=1).astype(np.float64)[:, None]
    err = np.abs(r["A"].astype(LD) - want).astype(np.float64)
    print(f"{c['name']}: max |A - A_ld| / max |a_s| = {float(np.max(err / scale)):.3e} (rtol {rtol:g})")
    assert np.isfinite(r["A"]).all()
    assert (err <= rtol * scale).all()


@pytest.mark.parametrize("c", T.CASES, ids=T.ids())
def test_eval_against_long_double(c):
    r = run(c)
    err = np.abs(r["F"].astype(LD) - r["Fld"]).astype(np.float64)
    ratio = err / r["tol"][:, None]
    print(f"{c['name']}: max |F - F_ld| {float(np.max(err)):.3e}, the fp64 restatement's {r['e_ref']:.3e}, "
          f"largest error / tolerance {float(np.max(ratio)):.3f}")
    assert r["F"].shape == (c["q"], c["m"]) and np.isfinite(r["F"]).all()
    assert (ratio <= 1.0).all()


@pytest.mark.parametrize("c", T.CASES, ids=T.ids())
def test_identity_on_training_rows(c):
    """candidates equal to training rows: f_s(x_r) + sqrt(diag) Eps[s][r] + diag a_s[r] = ys[r]"""
    rtol = dict(T.TIERS)[c["sn2"]]
    r, z = run(c), T.data(c)
    ntr, diag = z["ntr"], c["sn2"] + c["jitter"]
    if ntr == 0:
        assert c["m"] == 1
        return
    res = r["F"][:, :ntr] + np.sqrt(diag) * r["dr"]["Eps"][:, :ntr] + diag * r["A"][:, :ntr] - r["ys"][None, :ntr]
    bound = r["tol"] + rtol * diag * np.max(np.abs(r["A"]), axis=1)
    print(f"{c['name']}: largest identity residual / bound {float(np.max(np.abs(res) / bound[:, None])):.3f}")
    assert (np.abs(res) <= bound[:, None]).all()


def test_far_candidate_keeps_the_prior_path_alone():
    c = next(c for c in T.CASES if c["ell"] == "tiny")
    r, z = run(c), T.data(c)
    fld = r["fld"]
    assert float(np.max(T.kernel(fld.Xs, fld.scaled(z["U"][-1:]), 1.0))) == 0.0     # K* underflows, in long double too
    prior = T.prior(fld, r["dr"], fld.scaled(z["U"][-1:]))[:, 0]
    assert (np.abs(r["F"][:, -1].astype(LD) - prior).astype(np.float64) <= r["tol"]).all()
    assert float(np.max(np.abs(r["F"][:, -1]))) > 0.0


@pytest.mark.parametrize("c", T.CASES, ids=T.ids())
def test_select(c):
    r, z = run(c), T.data(c)
    k = c["q"]
    pos, f = T.select(r["F"], z["dup"], k)
    assert r["pos"].tolist() == pos.tolist()
    assert np.array_equal(r["f"], f)
    # the long-double oracle, walked along the device's own picks
    free = z["dup"] == 0
    second = picks = 0
    for s in range(k):
        idx = np.flatnonzero(free)
        if idx.size == 0:
            assert (r["pos"][s:] == -1).all()
            break
        v = r["Fld"][s, idx]
        order = np.argsort(v, kind="stable")
        best = idx[order[0]]
        gap = float(v[order[1]] - v[order[0]]) if idx.size > 1 else np.inf
        at = int(r["pos"][s])
        assert at >= 0 and free[at]
        picks += 1
        if gap > 2.0 * r["tol"][s]:
            assert at == best, (s, at, best, gap)
        else:
            second += 1
            assert abs(float(r["F"][s, at]) - float(v[order[0]])) <= r["tol"][s]
        free[at] = False
    _SECOND[c["name"]] = (second, picks)
    assert len(set(r["pos"][r["pos"] >= 0].tolist())) == int(np.sum(r["pos"] >= 0))


def test_near_ties_are_rare_over_the_table():
    for c in T.CASES:
        if c["name"] not in _SECOND:
            test_select(c)
    second = sum(a for a, _ in _SECOND.values())
    picks = sum(b for _, b in _SECOND.values())
    print(f"{second} of {picks} picks took the near-tie branch")
    assert 20 * second <= picks


def test_edges():
    import torch
    c = T.CASES[2]                                   # m = 1000, q = 33: two path groups
    r, z = run(c), T.data(c)
    e = engine(c)
    cand, m = dev(z["cand"]), c["m"]
    # every candidate a duplicate: every slot empty
    pos, f = (t.cpu().numpy() for t in e.gp_ts_select(cand, 5, dup=dev(np.ones(m, dtype=np.uint8))))
    assert pos.tolist() == [-1] * 5 and np.isposinf(f).all()
    # fewer free candidates than k, across the group boundary: the first three, then empties
    few = np.ones(m, dtype=np.uint8)
    few[[5, 640, 999]] = 0
    pos, f = (t.cpu().numpy() for t in e.gp_ts_select(cand, 33, dup=dev(few)))
    assert sorted(pos[:3].tolist()) == [5, 640, 999] and pos[3:].tolist() == [-1] * 30 and np.isposinf(f[3:]).all()
    assert pos.tolist() == T.select(r["F"], few, 33)[0].tolist()
    # no mask at all, k < q, and a pool narrower than its leading dimension
    pos, f = (t.cpu().numpy() for t in e.gp_ts_select(cand, 7, m=300))
    assert pos.tolist() == T.select(r["F"][:, :300], None, 7)[0].tolist()
    # m = 1, k = q = 1 (the first case): the one candidate
    c1 = T.CASES[0]
    assert run(c1)["pos"].tolist() == ([0] if T.data(c1)["dup"][0] == 0 else [-1])
    e1 = engine(c1)
    pos, f = (t.cpu().numpy() for t in e1.gp_ts_select(dev(T.data(c1)["cand"]), 1))
    assert pos.tolist() == [0] and f[0] == run(c1)["F"][0, 0]
    torch.cuda.synchronize()


def test_two_calls_return_the_same_bits_and_scores_are_untouched():
    c = T.CASES[1]
    z = T.data(c)
    e = engine(c, fresh=True)
    fit(e, c)
    cand, dup = dev(z["cand"]), dev(z["dup"])
    before = [t.cpu().numpy() for t in e.gp_score_values(cand, acq=e.acq("ei"), dup=dup)]
    out = []
    for _ in range(2):
        e.gp_ts_draw(c["q"], c["D"], round_=T.round_of(c))
        A = e.gp_ts_read("A")
        F = e.gp_ts_eval(cand).cpu().numpy()
        pos, f = (t.cpu().numpy() for t in e.gp_ts_select(cand, c["q"], dup=dup))
        out.append((A, F, pos, f))
    for a, b in zip(*out):
        assert np.array_equal(a, b, equal_nan=True)
    # ... the bits of the shared engine's run
    r = run(c)
    assert np.array_equal(out[0][0], r["A"]) and np.array_equal(out[0][1], r["F"])
    assert out[0][2].tolist() == r["pos"].tolist()
    # another key, other paths
    e.gp_ts_draw(c["q"], c["D"], round_=T.round_of(c) + 100)
    assert not np.array_equal(e.gp_ts_eval(cand).cpu().numpy(), r["F"])
    # TS wrote only scratch of its own: EI on the same fit, the same bits
    after = [t.cpu().numpy() for t in e.gp_score_values(cand, acq=e.acq("ei"), dup=dup)]
    for a, b in zip(before, after):
        assert np.array_equal(a.view(np.uint64), b.view(np.uint64))
    e.close()


def test_precision_8_changes_nothing():
    c = T.CASES[1]
    z, r = T.data(c), run(c)
    e = engine(c, fresh=True)
    e.gp_set_precision(8)
    fit(e, c)
    e.gp_ts_draw(c["q"], c["D"], round_=T.round_of(c))
    cand = dev(z["cand"])
    assert np.array_equal(e.gp_ts_read("A"), r["A"])
    assert np.array_equal(e.gp_ts_eval(cand).cpu().numpy(), r["F"])
    assert e.gp_ts_select(cand, c["q"], dup=dev(z["dup"]))[0].cpu().tolist() == r["pos"].tolist()
    e.close()


def test_a_refit_makes_the_draws_stale_and_bad_arguments():
    import torch
    from uptune_amd import _lib as L
    c = T.CASES[1]
    z = T.data(c)
    e = engine(c, fresh=True)
    cand = dev(z["cand"])
    m = c["m"]
    F = torch.empty((c["q"], m), dtype=torch.float64, device="cuda:0")
    out = torch.empty(c["q"], dtype=torch.int64, device="cuda:0")

    def ev(values=cand.data_ptr(), ld=m, mm=m, o=F.data_ptr(), ldf=m):
        return e.lib.ut_gp_ts_eval(e.ctx, values, ld, mm, o, ldf)

    def sel(values=cand.data_ptr(), ld=m, mm=m, k=c["q"], o=out.data_ptr()):
        return e.lib.ut_gp_ts_select(e.ctx, values, ld, mm, None, k, o, None)
    # no fit
    assert e.lib.ut_gp_ts_draw(e.ctx, 3, 128, 0) == UT_EINVAL
    assert ev() == UT_EINVAL and sel() == UT_EINVAL
    fit(e, c)
    # no draw yet
    assert ev() == UT_EINVAL and sel() == UT_EINVAL
    assert e.lib.ut_gp_ts_read(e.ctx, 0, None, (ctypes.c_int32 * 4)()) == UT_EINVAL
    for q, D, rnd in ((0, 128, 0), (257, 128, 0), (3, 64, 0), (3, 0, 0), (3, 200, 0), (3, 4224, 0), (3, 128, 1 << 24)):
        assert e.lib.ut_gp_ts_draw(e.ctx, q, D, rnd) == UT_EINVAL, (q, D, rnd)
    e.gp_ts_draw(c["q"], c["D"], round_=T.round_of(c))
    assert ev() == 0 and sel() == 0
    for bad in (dict(values=None), dict(o=None), dict(ld=m - 1), dict(ldf=m - 1), dict(mm=0)):
        assert ev(**bad) == UT_EINVAL, bad
    for bad in (dict(values=None), dict(o=None), dict(ld=m - 1), dict(k=0), dict(k=c["q"] + 1), dict(mm=0)):
        assert sel(**bad) == UT_EINVAL, bad
    with pytest.raises(ValueError):
        e.gp_ts_eval(cand[:-1])
    # a refit: the paths belong to the earlier fit, whatever it was
    fit(e, c)
    assert ev() == UT_EINVAL and sel() == UT_EINVAL
    with pytest.raises(L.UthotError, match="stale"):
        e.gp_ts_read("A")
    e.gp_ts_draw(c["q"], c["D"], round_=T.round_of(c))
    assert ev() == 0
    assert np.array_equal(F.cpu().numpy(), run(c)["F"])
    # the scratch goes through the counted allocations
    e2 = engine(c, fresh=True)
    fit(e2, c)
    assert e2.lib.ut_debug_fail_alloc(e2.ctx, 1) == 0
    with pytest.raises(L.UthotError, match="UT_ENOMEM"):
        e2.gp_ts_draw(c["q"], c["D"])
    e2.gp_ts_draw(c["q"], c["D"], round_=T.round_of(c))
    assert np.array_equal(e2.gp_ts_read("A"), run(c)["A"])
    e.close()
    e2.close()


def test_failed_fit_leaves_every_slot_empty():
    c = T.CASES[1]
    z = T.data(c)
    e = engine(c, fresh=True)
    e.gp_fit(z["X"], z["y"], lengthscale=z["ell"], sigma_n2=-2.0, jitter=0.0, wait=False)   # not positive definite
    e.gp_ts_draw(4, 128, round_=1)                     # enqueued behind the failing fit
    cand = dev(z["cand"])
    pos, f = (t.cpu().numpy() for t in e.gp_ts_select(cand, 4))
    assert pos.tolist() == [-1] * 4 and np.isposinf(f).all()
    assert np.isnan(e.gp_ts_eval(cand).cpu().numpy()).all()
    assert not e.gp_fit_ok()
    e.close()
