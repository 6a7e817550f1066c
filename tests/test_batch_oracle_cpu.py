"""tests/_batch_oracle.py pinned by a second route (no GPU): conditioning a GP
on a believed observation at a pick is adding the pick to the training set --
a GP's variance does not depend on y -- so after t picks the recursion's
variances must be those of GP(X + picks).posterior.

Tolerance: both routes factor K + sigma_n2 I with sigma_n2 = 1e-2 and sf2 = 1,
condition number at most (n + k) sf2 / sigma_n2 < 2e4, so each is good to about
2e4 * 2^-53 = 2e-12 absolute on variances <= 1; 1e-10 leaves room for the sums."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _batch_oracle as B  # noqa: E402
import _lml_oracle as O  # noqa: E402
from oracle import gp as ogp  # noqa: E402

SN2 = 1e-2


def setup(n=60, d=3, p=80, ell=0.5):
    X, y = O.data(n, d)
    return X, y, ogp.GP(X, y, lengthscale=ell, sigma_n2=SN2), B.pool(n, p, d), ell


@pytest.mark.parametrize("kind", ["ei", "ucb"])
@pytest.mark.parametrize("t", [1, 5, 17])
def test_conditioned_variance_is_the_refit_variance(kind, t):
    X, y, g, U, ell = setup()
    r = B.select(g, U, t, SN2, kind=kind)
    assert (r["pos"] >= 0).all() and len(set(r["pos"].tolist())) == t
    X2 = np.vstack([X, U[r["pos"]]])
    y2 = np.concatenate([y, np.linspace(-3.0, 7.0, t)])   # any y
    _, want = ogp.GP(X2, y2, lengthscale=ell, sigma_n2=SN2).posterior(U)
    np.testing.assert_allclose(r["var_after"], want, rtol=0.0, atol=1e-10)
    # ... and each pick's variance at pick time is that of the refit on the picks before it
    if t > 1:
        _, prev = ogp.GP(X2[:-1], y2[:-1], lengthscale=ell, sigma_n2=SN2).posterior(U)
        assert abs(r["var"][-1] - prev[r["pos"][-1]]) <= 1e-10


@pytest.mark.parametrize("kind", ["ei", "ucb"])
def test_one_pick_is_the_argmax(kind):
    X, y, g, U, ell = setup()
    mu, var = g.posterior(U)
    s = ogp.acquisition(mu, var, g.f_best, kind)
    r = B.select(g, U, 1, SN2, kind=kind)
    assert r["pos"][0] == int(np.argmax(s))
    np.testing.assert_allclose(r["score"][0], s.max(), rtol=1e-9)
    # the first of several picks too, and dup masks it
    dup = np.zeros(len(U), dtype=np.uint8)
    dup[int(np.argmax(s))] = 1
    assert B.select(g, U, 4, SN2, kind=kind)["pos"][0] == int(np.argmax(s))
    assert B.select(g, U, 4, SN2, kind=kind, dup=dup)["pos"][0] == int(np.argmax(np.where(dup != 0, -np.inf, s)))


@pytest.mark.parametrize("kind,kappa", [("ei", 2.0), ("ucb", 2.0), ("ucb", 0.0)])
def test_scores_never_increase(kind, kappa):
    X, y, g, U, ell = setup()
    r = B.select(g, U, 40, SN2, kind=kind, kappa=kappa)
    assert (np.diff(r["score"]) <= 0.0).all()
    assert (r["score"] == r["best"]).all()
    assert len(set(r["pos"].tolist())) == 40


def test_ties_go_to_the_smallest_position():
    X, y, g, U, ell = setup()
    src = int(np.argmin(g.posterior(U)[0]))
    U = U.copy()
    U[[3, 30, 31, 77]] = U[src]         # copies of the best candidate
    group = sorted({3, 30, 31, 77, src})
    r = B.select(g, U, 7, SN2, kind="ucb", kappa=0.0)   # kappa 0: the score is -mu, conditioning moves nothing
    mu, _ = g.posterior(U)
    assert len(set(mu[group].tolist())) == 1   # exact ties
    assert r["pos"][:len(group)].tolist() == group
    assert r["pos"].tolist() == sorted(range(len(U)), key=lambda i: (mu[i], i))[:7]


def test_more_picks_than_candidates_leaves_empty_slots():
    X, y, g, U, ell = setup()
    dup = np.ones(len(U), dtype=np.uint8)
    dup[[4, 9, 11]] = 0
    r = B.select(g, U, 5, SN2, dup=dup)
    assert sorted(r["pos"][:3].tolist()) == [4, 9, 11]
    assert r["pos"][3:].tolist() == [-1, -1] and (r["score"][3:] == -np.inf).all() and np.isnan(r["var"][3:]).all()


def test_forced_walk_reports_the_step_maximum():
    X, y, g, U, ell = setup()
    free = B.select(g, U, 8, SN2)
    walk = B.select(g, U, 8, SN2, forced=free["pos"])
    for key in ("pos", "score", "var", "best"):
        np.testing.assert_array_equal(free[key], walk[key])
