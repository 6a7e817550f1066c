"""Projected-ascent polish on the device (csrc/gp_polish.hip, ut_gp_polish):
the invariants the header promises, the step rule one step at a time against
the rule restated on the host from the device's own gradient
(tests/_polish_oracle.py), and that it climbs.

Tiers are the project's: rtol 1e-9 at sigma_n2 = 1e-2, 1e-5 at sigma_n2 = 1e-6,
scores held to rtol (|s| + max |s|) as in test_gpu_acq_grad.py.  On the
CPU restatement (test_polish_oracle_cpu.py) 8 steps move at least 96 % of the
candidates of the two climbing cases and raise the best score 1.08 to 28
times, so "more than half moved, the best score higher" is far from the edge."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _lml_oracle as O  # noqa: E402
import _polish_oracle as P  # noqa: E402
from _spaces import to_manip  # noqa: E402
from oracle import gp as ogp  # noqa: E402
from oracle import space as osp  # noqa: E402
from oracle.space import BOOL, ENUM, FLOAT, INT, LOGINT, PERM, POW2, Param  # noqa: E402

pytestmark = pytest.mark.gpu

UT_EINVAL = -1
MIXED = [Param("f", FLOAT, -3.0, 5.0), Param("i", INT, 1, 500), Param("l", LOGINT, 1, 4096),
         Param("p", POW2, 2, 256), Param("b", BOOL), Param("e", ENUM, options=list("vwxyz")),
         Param("q", PERM, options=list(range(6))), Param("g", FLOAT, 0.0, 1.0)]
FREE_KINDS = (FLOAT, INT, LOGINT, POW2)
# on MIXED the plain EI underflows for most of the shortlist (its median is 1e-33 of the best): an exploration
# offset xi = -1 gives every candidate an EI gradient to climb, and carries xi through the call
XI = dict(ei=-1.0, ucb=0.0)

_ENGINES = {}
_MIXED = {}


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


def fit(e, case, sn2):
    n, d, p, ell = case
    X, y = O.data(n, d)
    e.gp_fit(X, y, lengthscale=ell, sigma_n2=sn2)


def close(a, b, rtol):
    fin = np.isfinite(b)
    return np.abs(a[fin] - b[fin]) <= rtol * (np.abs(b[fin]) + np.abs(b[fin]).max())


def mixed():
    """an engine over MIXED with a fit in place, its shortlist (device values,
    host features), the oracle GP and the lengthscales; built once"""
    if not _MIXED:
        import torch
        from uptune_amd.engine import BatchEngine
        if not torch.cuda.is_available():
            pytest.skip("needs a GPU")
        e = BatchEngine(to_manip(MIXED), device=0, seed=5)
        e.population_init(512, round_=0)
        vals = e.population_get().contiguous()
        tr, sl = vals[:, :150].contiguous(), vals[:, 150:450].contiguous()
        X = e.encode(tr).cpu().numpy().T
        y = np.sum((X - 0.4) ** 2, axis=1) + 0.01 * np.random.default_rng(3).standard_normal(150)
        ell = 0.5 * O.ard_base(X.shape[1])
        e.gp_fit(X, y, lengthscale=ell, sigma_n2=1e-2)
        free = np.zeros(X.shape[1], dtype=bool)
        for ps in e.spec.params:
            if ps.kind in FREE_KINDS and ps.u_lo < ps.u_hi:
                free[ps.feat_col] = True
        assert free.sum() == 5
        _MIXED.update(e=e, sl=sl, V=sl.cpu().numpy(), U=e.encode(sl).cpu().numpy().T, ell=ell, free=free,
                      g=ogp.GP(X, y, lengthscale=ell, sigma_n2=1e-2))
    return _MIXED


def check_invariants(e, space, sl, V, dup, out, kind, rtol, xi=0.0):
    """what the header promises of one call's outputs (host arrays)"""
    vals, score, score0, moved = out
    live = dup == 0
    assert (score[live] >= score0[live]).all()
    assert (score[~live] == -np.inf).all() and (score0[~live] == -np.inf).all() and not moved[~live].any()
    assert (vals[:, ~live].view(np.int64) == V[:, ~live].view(np.int64)).all()
    still = moved == 0
    assert (vals[:, still].view(np.int64) == V[:, still].view(np.int64)).all()
    assert (score[still & live] == score0[still & live]).all()
    assert (score[moved != 0] > score0[moved != 0]).all()
    # bitwise the gradient call's score on the returned rows, and the scoring path's within the tier
    again = e.gp_acq_grad(dev(vals), acq=e.acq(kind, xi=xi))[0].cpu().numpy()
    assert again[live].tobytes() == score[live].tobytes()
    first = e.gp_acq_grad(sl, acq=e.acq(kind, xi=xi))[0].cpu().numpy()
    assert first[live].tobytes() == score0[live].tobytes()
    dense = e.gp_score_values(dev(vals), acq=e.acq(kind, xi=xi))[2].cpu().numpy()
    assert close(score[live], dense[live], rtol).all()
    # every value is a legal stored value; what is not free is the input's bits
    for ps, op in zip(e.spec.params, space):
        cols = slice(ps.col, ps.col + ps.width)
        got = vals[cols]
        if op.kind not in FREE_KINDS:
            assert (got.view(np.int64) == V[cols].view(np.int64)).all(), op.name
            continue
        assert (got >= op.lo).all() and (got <= op.hi).all(), op.name
        if op.kind in (INT, LOGINT):
            assert (got == np.rint(got)).all(), op.name
        if op.kind == POW2:
            assert (np.log2(got) == np.rint(np.log2(got))).all(), op.name


@pytest.mark.parametrize("kind", P.KINDS)
def test_invariants_on_a_mixed_space(kind):
    m = mixed()
    e, sl, V = m["e"], m["sl"], m["V"]
    p = V.shape[1]
    dup = dup7(p)
    out = host(*e.gp_polish(sl, 8, acq=e.acq(kind, xi=XI[kind]), dup=dev(dup)))
    check_invariants(e, MIXED, sl, V, dup, out, kind, 1e-9, xi=XI[kind])
    print(f"mixed {kind}: {out[3].sum()} of {(dup == 0).sum()} moved, best {out[2].max():.4g} -> {out[1].max():.4g}")
    assert out[3].sum() >= (dup == 0).sum() // 2 and out[1].max() > out[2].max()
    again = host(*e.gp_polish(sl, 8, acq=e.acq(kind, xi=XI[kind]), dup=dev(dup)))
    for x, y in zip(out, again):                         # two calls: the same bits
        assert x.tobytes() == y.tobytes()
    # steps = 0 is the identity
    v0, s, s0, mv = host(*e.gp_polish(sl, 0, acq=e.acq(kind, xi=XI[kind]), dup=dev(dup)))
    assert v0.tobytes() == V.tobytes() and s.tobytes() == s0.tobytes() and not mv.any()
    assert s0.tobytes() == out[2].tobytes()
    # without dup every candidate is live
    out = host(*e.gp_polish(sl, 2, acq=e.acq(kind, xi=XI[kind])))
    check_invariants(e, MIXED, sl, V, np.zeros(p, dtype=np.uint8), out, kind, 1e-9, xi=XI[kind])


@pytest.mark.parametrize("kind", P.KINDS)
def test_one_step_follows_the_rule(kind):
    """steps = 1: the expected trial from the device's own gradient, decoded on
    the host by the oracle's set_unit_value"""
    m = mixed()
    e, sl, V, U, g, ell, free = m["e"], m["sl"], m["V"], m["U"], m["g"], m["ell"], m["free"]
    p = V.shape[1]
    s0, _, _, G = host(*e.gp_acq_grad(sl, acq=e.acq(kind, xi=XI[kind])))
    vals, score, score0, moved = host(*e.gp_polish(sl, 1, acq=e.acq(kind, xi=XI[kind])))
    Ut, N, act = P.trial(U, G.T, ell, np.full(p, 0.25), free)
    assert act.all()
    want = V.copy()
    near = np.zeros((len(e.spec.params), p), dtype=bool)   # a rounding the summation order of N may flip
    tol = {}
    for q, (ps, op) in enumerate(zip(e.spec.params, MIXED)):
        if not free[ps.feat_col] or ps.kind not in FREE_KINDS:
            continue
        u = Ut[:, ps.feat_col]
        want[ps.col] = [osp.set_unit_value(op, float(min(max(x, 0.0), 1.0)), float(c)) for x, c in zip(u, V[ps.col])]
        span = float(op.hi - op.lo)
        tol[q] = 2.0 ** -40 * span
        if ps.kind == LOGINT:
            pre = 2.0 ** (u * ps.u_span + ps.u_lo) - 1.0 + ps.lo
            near[q] = np.abs(np.abs(pre - np.floor(pre)) - 0.5) <= 2.0 ** -40 * span * ps.u_span
        elif ps.kind in (INT, POW2):
            pre = u * ps.u_span + ps.u_lo
            near[q] = np.abs(np.abs(pre - np.floor(pre)) - 0.5) <= 2.0 ** -40 * ps.u_span
    assert near.mean() <= 0.01
    # moved = the trial is accepted on its features and the decoded row still beats s0 (scores by the oracle)
    s_t = P.score_grad(g, Ut, kind, xi=XI[kind])["score"]
    s_v = P.score_grad(g, e.encode(dev(want)).cpu().numpy().T, kind, xi=XI[kind])["score"]
    w0 = P.score_grad(g, U, kind, xi=XI[kind])["score"]
    scale = 1e-9 * (np.abs(w0) + np.abs(w0).max())
    clear = (np.abs(s_t - w0) > scale) & (np.abs(s_v - w0) > scale) & ~near.any(axis=0)
    expect = (s_t > w0) & (s_v > w0)
    print(f"mixed {kind}: moved {moved.sum()} of {p}, expected {expect.sum()}, clear of the tier {clear.sum()}, "
          f"roundings left out {near.sum()}")
    assert clear.sum() >= p // 2                            # (EI's small scores sit inside the tier of the largest)
    assert (moved[clear] != 0).tolist() == expect[clear].tolist()
    mv = moved != 0
    assert mv.sum() >= p // 4
    for q, ps in enumerate(e.spec.params):
        if q not in tol:
            continue
        ok = mv & ~near[q]
        if ps.kind == FLOAT:
            assert (np.abs(vals[ps.col][ok] - want[ps.col][ok]) <= tol[q]).all(), ps.name
        else:
            assert (vals[ps.col][ok] == want[ps.col][ok]).all(), ps.name
    assert (score0 == s0).all()


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("sn2,rtol", P.TIERS)
@pytest.mark.parametrize("case", P.CASES[:2])
def test_it_climbs(case, sn2, rtol, kind):
    n, d, p, ell = case
    e = engine(d)
    fit(e, case, sn2)
    U, dup = P.cands(n, d, p), dup7(p)
    sl = dev(U.T)
    out = host(*e.gp_polish(sl, 8, acq=e.acq(kind), dup=dev(dup)))
    check_invariants(e, [Param(f"u{k}", FLOAT, 0.0, 1.0) for k in range(d)], sl, np.ascontiguousarray(U.T), dup, out,
                     kind, rtol)
    vals, score, score0, moved = out
    live = dup == 0
    print(f"{case} sn2={sn2:g} {kind}: best {score0.max():.4g} -> {score.max():.4g}, "
          f"{moved[live].mean():.1%} of the live candidates moved")
    assert score.max() > score0.max()
    assert moved[live].sum() * 2 >= live.sum()
    assert (vals >= 0.0).all() and (vals <= 1.0).all()


def test_flat_ei_stays():
    """EI at (321, 3, 1024, 0.3), sigma_n2 = 1e-6: a candidate whose device
    gradient is all zero is returned as it came"""
    case = P.CASES[2]
    n, d, p, ell = case
    e = engine(d)
    fit(e, case, 1e-6)
    U = np.ascontiguousarray(P.cands(n, d, p).T)
    G = e.gp_acq_grad(dev(U), acq=e.acq("ei"))[3].cpu().numpy()
    flat = (G == 0.0).all(axis=0)
    vals, score, score0, moved = host(*e.gp_polish(dev(U), 8, acq=e.acq("ei")))
    print(f"flat: {flat.sum()} of {p}; moved {moved.sum()}")
    assert flat.sum() >= 500
    assert (vals[:, flat].view(np.int64) == U[:, flat].view(np.int64)).all() and not moved[flat].any()
    assert (score >= score0).all() and np.isfinite(score).all()


@pytest.mark.parametrize("kind", P.KINDS)
def test_corners_stay_inside_and_projected_components_do_not_count(kind):
    case = P.CASES[0]
    n, d, p, ell = case
    e = engine(d)
    fit(e, case, 1e-2)
    U = P.cands(n, d, p).copy()
    rng = np.random.default_rng(17)
    U[3:35] = rng.integers(0, 2, size=(32, d)).astype(np.float64)      # more corners
    U[35:67] = np.where(rng.uniform(size=(32, d)) < 0.5, U[35:67], rng.integers(0, 2, size=(32, d)))   # faces
    sl = dev(U.T)
    G = e.gp_acq_grad(sl, acq=e.acq(kind))[3].cpu().numpy().T
    vals, score, score0, moved = host(*e.gp_polish(sl, 1, acq=e.acq(kind)))
    Ut, N, act = P.trial(U, G, ell, np.full(p, 0.25))
    outward = ((U <= 0.0) & (G < 0.0)) | ((U >= 1.0) & (G > 0.0))
    assert outward[:67].sum() >= 50                         # the premise: components to project away
    mv = moved != 0
    assert (vals >= 0.0).all() and (vals <= 1.0).all()
    assert (np.abs(vals.T[mv] - Ut[mv]) <= 2.0 ** -40).all()
    assert (vals.T[mv][outward[mv]] == U[mv][outward[mv]]).all()
    # an unclipped move is eta long in lengthscale units, whatever was projected away
    inside = mv & ((Ut > 0.0) & (Ut < 1.0) | outward | (Ut == U)).all(axis=1)
    length = np.sqrt(np.sum(((vals.T - U) / ell) ** 2, axis=1))
    print(f"{kind}: moved {mv.sum()}, unclipped {inside.sum()}, of them with a projected component "
          f"{(inside & outward.any(axis=1)).sum()}")
    assert (inside & outward.any(axis=1)).sum() >= 10
    assert (np.abs(length[inside] - 0.25) <= 1e-9).all()
    vals8 = e.gp_polish(sl, 8, acq=e.acq(kind))[0].cpu().numpy()
    assert (vals8 >= 0.0).all() and (vals8 <= 1.0).all()


def test_bad_arguments_and_failed_allocation():
    import torch
    from uptune_amd import _lib as L
    case = P.CASES[0]
    n, d, p, ell = case
    e = engine(d, fresh=True)
    U = dev(P.cands(n, d, p).T)
    acq = e.acq("ei")
    out = torch.empty((d, p), dtype=torch.float64, device="cuda:0")
    sc = torch.empty(p, dtype=torch.float64, device="cuda:0")

    def call(values=U.data_ptr(), ld=p, pp=p, a=ctypes.byref(acq), steps=2, prm=True, o=out.data_ptr(), ldo=p,
             s=sc.data_ptr(), **par):
        pr = L.PolishParams(steps=steps, pad=0, step0=par.get("step0", 0.0), step_max=par.get("step_max", 0.0),
                            grow=par.get("grow", 0.0), shrink=par.get("shrink", 0.0))
        return e.lib.ut_gp_polish(e.ctx, values, ld, pp, a, None, ctypes.byref(pr) if prm else None, o, ldo, s,
                                  None, None)
    assert call() == UT_EINVAL                           # no fit at all
    fit(e, case, 1e-2)
    assert call() == 0
    for bad in (dict(pp=0), dict(pp=4097, ld=4097, ldo=4097), dict(values=None), dict(a=None), dict(prm=False),
                dict(o=None), dict(s=None), dict(ld=p - 1), dict(ldo=p - 1), dict(steps=-1), dict(step0=-0.5),
                dict(shrink=float("nan")), dict(grow=float("inf"))):
        assert call(**bad) == UT_EINVAL, bad
    with pytest.raises(ValueError):                      # a column count that is not the space's
        e.gp_polish(U[:d - 1], 2)
    X, y = O.data(n, d)
    e.gp_cons_set(np.sum(X, axis=1), [2.5])
    assert call() == UT_EINVAL
    e.gp_cons_clear()
    e.gp_feas_set(np.random.default_rng(1).uniform(size=(7, d)))
    assert call() == UT_EINVAL
    e.gp_feas_clear()
    assert call() == 0
    e2 = engine(d, fresh=True)
    fit(e2, case, 1e-2)
    assert e2.lib.ut_debug_fail_alloc(e2.ctx, 1) == 0
    with pytest.raises(L.UthotError, match="UT_ENOMEM"):
        e2.gp_polish(U, 2)
    assert np.isfinite(e2.gp_polish(U, 2)[1].cpu().numpy()).all()      # ... and the following call succeeds
    e.close()
    e2.close()


def test_failed_fit_moves_nothing():
    case = P.CASES[0]
    n, d, p, ell = case
    X, y = O.data(n, d)
    e = engine(d, fresh=True)
    e.gp_fit(X, y, lengthscale=ell, sigma_n2=-2.0, jitter=0.0, wait=False)   # not positive definite
    U = np.ascontiguousarray(P.cands(n, d, p).T)
    vals, score, score0, moved = host(*e.gp_polish(dev(U), 4))
    assert np.isnan(score).all() and not moved.any() and vals.tobytes() == U.tobytes()
    e.close()
