"""tests/_polish_oracle.py held to account on the CPU, so that the GPU tests of
ut_gp_acq_grad / ut_gp_polish lean on something checked; and the technique's
constructor refusals for polish=.

Candidates: _polish_oracle.cands (uniform; row 0 a training row, row 1 all
zeros, row 2 all ones), the GPU tests' own.

Central differences (h = 1e-6) of ogp.acquisition o GP.posterior carry the
posterior's own rounding divided by 2 h, so they are noise-limited where that
rounding is amplified:
  * UCB at (321, 3, 1024, 0.3) with sigma_n2 = 1e-6 is left out (7.9e-6 of the
    largest |g| on these candidates, from the difference quotient, not from
    score_grad: a smaller h makes it larger, and the long-double check below
    holds the same gradient to 3.9e-11);
  * row 0 is left out at sigma_n2 = 1e-6: there sigma ~ 1e-3, and d sigma =
    d var / (2 sigma) amplifies var's rounding 500 times (1.4e-6 for UCB at
    (200, 37, 300, 2.0), again growing as h shrinks).  That row is held by the
    long-double check.
Measured on the rest: at most 3.1e-8 at sigma_n2 = 1e-2 and 1.5e-7 at 1e-6.
fp64 against long double: at most 1.3e-12 at sigma_n2 = 1e-2 and 3.9e-11 at
1e-6 (worst: UCB at (321, 3, 1024, 0.3))."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _polish_oracle as P  # noqa: E402
from oracle import gp as ogp  # noqa: E402

COMBOS = [(c, t, k) for c in P.CASES for t in P.TIERS for k in P.KINDS]


def _id(v):
    return "-".join(str(x) for x in v) if isinstance(v, tuple) else str(v)


@pytest.mark.parametrize("case,tier,kind", [x for x in COMBOS if not (x[0] == P.CASES[2] and x[1][0] == 1e-6
                                                                      and x[2] == "ucb")], ids=_id)
def test_score_grad_is_the_derivative_of_the_oracle_acquisition(case, tier, kind):
    n, d, p, ell = case
    sn2 = tier[0]
    g, U = P.gp_of(n, d, ell, sn2), P.cands(n, d, p)
    r = P.score_grad(g, U, kind)
    mu, var = g.posterior(U)
    assert np.allclose(r["mu"], mu, rtol=0, atol=1e-9) and np.allclose(r["var"], var, rtol=0, atol=1e-9)
    assert np.allclose(r["score"], ogp.acquisition(mu, var, g.f_best, kind), rtol=0, atol=1e-9)
    h = 1e-6
    fd = np.empty_like(r["grad"])
    for j in range(d):
        e = np.zeros(d)
        e[j] = h
        fd[:, j] = (ogp.acquisition(*g.posterior(U + e), g.f_best, kind)
                    - ogp.acquisition(*g.posterior(U - e), g.f_best, kind)) / (2 * h)
    gm = np.abs(r["grad"]).max()
    rows = slice(1, None) if sn2 == 1e-6 else slice(None)
    err = np.abs(fd - r["grad"])[rows].max() / gm
    print(f"{case} sn2={sn2:g} {kind}: central difference error {err:.2e} of max|g| = {gm:.3g}")
    assert err <= 1e-6


@pytest.mark.parametrize("case,tier,kind", COMBOS, ids=_id)
def test_fp64_agrees_with_long_double(case, tier, kind):
    assert np.finfo(np.longdouble).nmant >= 63
    n, d, p, ell = case
    g, U = P.gp_of(n, d, ell, tier[0]), P.cands(n, d, p)
    a, b = P.score_grad(g, U, kind), P.score_grad(g, U, kind, ld=True)
    gm = np.abs(a["grad"]).max()
    err = float(np.abs(b["grad"] - a["grad"]).max() / gm)
    print(f"{case} sn2={tier[0]:g} {kind}: fp64 - long double {err:.2e} of max|g|")
    assert err <= 1e-10


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("sn2", [t[0] for t in P.TIERS])
@pytest.mark.parametrize("case", P.CASES[:2], ids=_id)
def test_polish_never_lowers_and_raises_the_best(case, sn2, kind):
    n, d, p, ell = case
    g, U = P.gp_of(n, d, ell, sn2), P.cands(n, d, p)
    dup = np.zeros(p, dtype=np.uint8)
    dup[::7] = 1
    r = P.polish(g, U, kind, 8, dup=dup)
    live = dup == 0
    assert (r["score"][live] >= r["score0"][live]).all()
    assert (r["U"][~live] == U[~live]).all() and (r["score"][~live] == -np.inf).all()
    assert (r["U"] >= 0.0).all() and (r["U"] <= 1.0).all()
    # the reported score is the score at the reported point
    assert (P.score_grad(g, r["U"], kind)["score"][live] == r["score"][live]).all()
    print(f"{case} sn2={sn2:g} {kind}: best {r['score0'].max():.4g} -> {r['score'].max():.4g}, "
          f"{r['accepted'][live].mean():.1%} moved")
    assert r["score"].max() > r["score0"].max()
    assert r["accepted"][live].mean() >= 0.5


def test_polish_0_steps_and_masks():
    n, d, p, ell = P.CASES[0]
    g, U = P.gp_of(n, d, ell, 1e-2), P.cands(n, d, p)
    r = P.polish(g, U, "ei", 0)
    assert (r["U"] == U).all() and (r["score"] == r["score0"]).all() and not r["accepted"].any()
    # features that are not free never move; the corners' outward components are projected away
    free = np.array([True, False, True, True, False])
    r = P.polish(g, U, "ucb", 4, free=free)
    assert (r["U"][:, ~free] == U[:, ~free]).all() and r["accepted"].any()
    G = P.score_grad(g, U, "ucb")["grad"]
    Ut, N, act = P.trial(U, G, 1.0 / g.inv_ell, np.full(p, 0.25))
    out1, out2 = G[1] < 0, G[2] > 0                       # row 1 at 0, row 2 at 1
    assert (Ut[1][out1] == 0.0).all() and (Ut[2][out2] == 1.0).all()
    for i, out in ((1, out1), (2, out2)):                # the step's length in lengthscale units is eta
        if act[i] and ((Ut[i] > 0) & (Ut[i] < 1))[~out].all():
            assert abs(np.sqrt(np.sum(((Ut[i] - U[i]) * g.inv_ell) ** 2)) - 0.25) <= 1e-12


KW = dict(pool=4096, batch=8, population=256, seed=3, lengthscale=0.3)


def test_constructor_refusals():
    from uptune_amd import technique as T
    assert T.GpuDifferentialEvolution(**KW).polish == 0
    t = T.GpuDifferentialEvolution(polish=8, **KW)
    assert (t.polish, t.polish_pool) == (8, 64)
    assert T.GpuDifferentialEvolution(polish=8, pool=4096, batch=32, population=256).polish_pool == 128
    assert T.GpuPSO(polish=4, polish_pool=512, diversify=64, name="pso", **KW).polish_pool == 512
    for bad in (dict(polish=8, prune_rows=128), dict(polish=8, surrogate="forest"), dict(polish=8, surrogate=object()),
                dict(polish=8, constraints=[("mem", "<=", 1.0)]), dict(polish=8, feasibility=True),
                dict(polish=8, polish_pool=4), dict(polish=8, polish_pool=4097), dict(polish=-1)):
        with pytest.raises(ValueError):
            T.GpuDifferentialEvolution(**bad, **KW)
    # a shared model carries its own constraints / feasibility / surrogate
    for mk in (dict(constraints=[("mem", "<=", 1.0)]), dict(feasibility=True), dict(surrogate="forest")):
        with pytest.raises(ValueError):
            T.GpuDifferentialEvolution(polish=8, shared=T.SharedModel(**mk), **KW)
    # the factories pass it through
    assert all(t.polish == 4 and t.polish_pool == 64 for t in T.pso_ga_de_bandit(polish=4, **KW).techniques)
    assert all(t.polish == 4 for t in T.bandit_a(polish=4, **KW).techniques)
    assert all(t.polish == 4 for t in T.bandit_b(polish=4, **KW).techniques)
    reg = T.reference_registry(polish=2, **KW)
    assert all(getattr(t, "polish", 2) == 2 for t in reg) and reg[0].polish == 2
