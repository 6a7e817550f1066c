"""The pruned selection on the CPU: the restatement (tests/_prune_oracle.py) is
sound and selects what the dense ranking selects on every case of the shared
table, each case sits in the regime the table claims for it, and its selection
is decidable on the reference alone -- so the GPU tests of the same table
(test_gpu_prune_bounds.py) can assert without conditions."""
import numpy as np
import pytest

import _prune_oracle as po
from oracle import gp as ogp


@pytest.fixture(params=po.CASES, ids=po.case_ids())
def case(request):
    return request.param


def test_case_table_covers_the_edges():
    """the shapes and scales the table exists for are all in it"""
    C = po.CASES
    assert len({c["name"] for c in C}) == len(C)
    assert {1e-3, 37.0} <= {c["sf2"] for c in C}
    assert {1, 3, 112} <= {c["d"] for c in C}
    assert {128, 129, 1000} <= {c["n"] for c in C}
    assert {1, 255, 257, 1023, 1025} <= {c["m"] for c in C}
    assert {1, 17, 1024} <= {c["k"] for c in C}
    assert any(c["cand_base"] == 2 ** 40 for c in C)
    assert any(c["bound_rows"] == 1 for c in C) and any(c["bound_rows"] == c["n"] for c in C)
    assert any(c["bound_rows"] == 10 * c["n"] for c in C)
    assert any(c["n"] == 128 and c["bound_rows"] == 128 for c in C)
    assert any(c["acq"]["kind"] == "ucb" and c["acq"]["kappa"] == 0.0 for c in C)
    assert any(c["acq"]["xi"] == 0.1 for c in C) and any(c["sn2"] == 1e-2 * c["sf2"] for c in C)
    assert {"prunes", "dense", "flat", "few_valid"} == {c["regime"] for c in C}
    assert all(c["n"] <= 1024 and c["m"] <= 5000 for c in C)
    # one lengthscale per feature: EI and UCB over ARD's whole box, a short last feature at
    # sf2 = 37, and a case that falls back to dense
    ard = [c for c in C if np.ndim(c["ell"]) == 1]
    assert {("ei", 64), ("ucb", 64), ("ei", 33)} <= {(c["acq"]["kind"], c["d"]) for c in ard}
    assert any(c["sf2"] == 37.0 and c["ell"][-1] == c["ell"].min() < c["ell"][0] for c in ard)
    assert any(c["regime"] == "dense" for c in ard)
    assert all(len(set(np.atleast_1d(c["ell"]).tolist())) > 1 for c in ard)


def test_posterior_is_the_oracles(case):
    """the split sum of squares is oracle.gp.GP.posterior up to its rounding: the
    mean within 4 n eps sum |k* alpha|, the variance within 4 n eps sf2 (two sums
    of n non-negative terms <= sf2, each within n eps of its value)"""
    z = po.case_data(case)
    g, r = z["gp"], po.case_restated(case)
    mu, var = g.posterior(z["U"])
    n, eps = case["n"], np.finfo(np.float64).eps
    Ks = g.sf2 * np.exp(-0.5 * ogp.sqdist(z["U"] * g.inv_ell, g.Xs))
    assert np.all(np.abs(r["mu"] - mu) <= 4 * n * eps * (Ks @ np.abs(g.alpha)))
    assert np.all(np.abs(r["var"] - var) <= 4 * n * eps * g.sf2)
    assert r["rows"] % 128 == 0 and 128 <= r["rows"] <= po.npad(n)


def test_bound_is_sound_and_selection_is_the_dense_one(case):
    r = po.case_restated(case)
    v = r["valid"]
    assert np.all(r["bound"][v] >= r["score"][v])
    assert np.all(r["bound"][~v] == -np.inf)
    want = sorted(np.flatnonzero(v).tolist(), key=lambda i: (-r["score"][i], i))[:case["k"]]
    assert r["sel"].tolist() == want
    assert r["dense"] == (2 * int(r["keep"].sum()) > case["m"])


def test_case_is_in_its_regime(case):
    r = po.case_restated(case)
    m, k, v = case["m"], case["k"], r["valid"]
    ns = int(r["keep"].sum())
    if case["regime"] == "prunes":
        assert 0 < ns <= m / 4 and not r["dense"] and int(v.sum()) >= k
    elif case["regime"] == "dense":
        assert ns > m / 2 and r["dense"] and int(v.sum()) >= k
    elif case["regime"] == "flat":
        s = r["score"][v]
        assert int(v.sum()) >= k and np.all(s == s[0]) and r["dense"]
    else:
        assert case["regime"] == "few_valid"
        assert int(v.sum()) < k and r["tau"] == -np.inf and ns == m
        # the valid candidates' ranking is decidable: their scores are all one
        # double, or pairwise further apart than the oracle band
        s = np.sort(r["score"][v])
        if s.size > 1 and not np.all(s == s[0]):
            assert np.all(np.diff(s) > 1e-5 * np.abs(s[1:]) + 1e-8)
        if case["acq"]["kind"] == "ucb":
            # a threshold of 0 in place of -inf would prune: fewer than half the
            # candidates have a bound >= 0, so the dense fallback does not hide it
            assert 2 * int((r["bound"] >= 0.0).sum()) < m


def test_selection_is_decidable(case):
    """prunes and dense cases: the k-th best score t is far above the absolute
    floor of the scores' tolerance, and next to nothing lies within the
    oracle band of it"""
    if case["regime"] not in ("prunes", "dense"):
        return
    r = po.case_restated(case)
    s = r["score"][r["valid"]]
    t = np.sort(s)[::-1][case["k"] - 1]
    assert t >= 1e-4
    assert int((np.abs(s - t) <= 1e-5 * abs(t) + 1e-8).sum()) - 1 <= 8


def test_mean_is_well_conditioned(case):
    """two summation orders of mu = sum_r alpha_r k*_r can differ by an ulp of
    every term, eps sum |alpha_r| k*_r; the path-to-path tolerance on the mean
    (rtol 1e-9, atol 1e-10) can only be asked where that stays below it (an
    almost noise-free fit of 128 points in one dimension has sum |alpha| ~ 1e7
    and does not).  Flat cases compare no scores but one double."""
    if case["regime"] == "flat":
        return
    z, r = po.case_data(case), po.case_restated(case)
    g = z["gp"]
    S = (g.sf2 * np.exp(-0.5 * ogp.sqdist(z["U"] * g.inv_ell, g.Xs))) @ np.abs(g.alpha)
    v = r["valid"]
    assert np.all(np.finfo(np.float64).eps * S[v] <= 1e-10 + 1e-9 * np.abs(r["mu"][v]))


def test_band_check_rejects_wrong_selections():
    """the shared band check fails on a missing, a repeated, an invalid and a
    misordered pick, and passes on the reference selection"""
    ref = np.array([0.5, 0.9, 0.1, 0.7, 0.3, 0.8])
    valid = np.array([1, 1, 1, 1, 1, 0], dtype=bool)
    ok = lambda idx, top: po.band_check(idx, top, ref, valid, 3, 10, 1e-9, 1e-12)   # noqa: E731
    ok([11, 13, 10], [0.9, 0.7, 0.5])
    for idx, top in [([11, 13, 14], [0.9, 0.7, 0.3]), ([11, 11, 13], [0.9, 0.9, 0.7]),
                     ([15, 11, 13], [0.8, 0.9, 0.7]), ([13, 11, 10], [0.7, 0.9, 0.5]),
                     ([11, 13, -1], [0.9, 0.7, 0.0])]:
        with pytest.raises(AssertionError):
            ok(idx, top)
    po.band_check([11, 13, 10, 14, 12, -1, -1], [0.9, 0.7, 0.5, 0.3, 0.1, 0.0, -np.inf], ref, valid, 7, 10, 1e-9, 1e-12)
    tie = np.array([0.5, 0.5, 0.5])
    po.band_check([0, 1], [0.5, 0.5], tie, np.ones(3, dtype=bool), 2, 0, 0.0, 0.0)
    with pytest.raises(AssertionError):
        po.band_check([1, 0], [0.5, 0.5], tie, np.ones(3, dtype=bool), 2, 0, 0.0, 0.0)
