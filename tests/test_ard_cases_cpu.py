"""The per-feature lengthscale table (tests/_ard_cases.py) is a fair judge, on
the reference alone, so that the GPU tests of the same table
(test_gpu_ard_scoring.py) can assert without conditions:

  - the oracle is self-consistent on every case: refitting with the features
    (and their lengthscales) in another order moves no mean and no variance by
    more than 1 % of the fp64 tier's tolerance;
  - every case notices a lengthscale taken from the wrong feature: candidates
    scaled by the rolled vector (training rows right) move more than half of
    the oracle's means by more than 100 tolerances, and so does the one-feature
    error at the end where a one_short case has its short feature (the error at
    the other end moves nothing there, which is why both ends are in the table);
  - every vector lies in ARD's box and every categorical vector is constant
    over the one-hot columns (the fit stays in categorical mode)."""
import numpy as np
import pytest

import _ard_cases as A
from oracle import gp as ogp
from oracle.space import BOOL, ENUM


def _data(c):
    return A.categorical_data(c) if "which" in c else A.numeric_data(c)


@pytest.fixture(params=A.NUMERIC + A.CATEGORICAL, ids=A.numeric_ids() + A.categorical_ids())
def case(request):
    return request.param


def _posterior_scaled(g, U, ell_cand):
    """the oracle's posterior with the candidates alone scaled by ell_cand"""
    return g.posterior(np.asarray(U) / np.asarray(ell_cand) / g.inv_ell)   # (posterior multiplies by inv_ell)


def _moved(c, z, ell_wrong):
    """the share of candidates whose oracle mean moves by more than 100 tolerances"""
    mu, _ = _posterior_scaled(z["gp"], z["U"], ell_wrong)
    return float(np.mean(np.abs(mu - z["mu"]) > 100.0 * (A.ATOL + A.RTOL * np.abs(z["mu"]))))


def test_table_keeps_its_shapes():
    assert {(c["n"], c["d"]) for c in A.NUMERIC} == A.SHAPES
    names = A.numeric_ids() + A.categorical_ids()
    assert len(set(names)) == len(names)
    rec = {(c["n"], c["d"], c["recipe"]) for c in A.NUMERIC if isinstance(c["recipe"], str)}
    assert {(1024, 64, "spread"), (1024, 64, "one_short_last"), (600, 33, "spread"), (600, 33, "one_short_first"),
            (600, 33, "one_short_last"), (500, 97, "spread"), (500, 97, "one_short_last"), (300, 16, "spread"),
            (200, 8, "narrow")} <= rec
    assert {37.0, 1e-3} <= {c["sf2"] for c in A.NUMERIC}
    assert {c["which"] for c in A.CATEGORICAL} == {"mixed", "hpl", "perm"}
    assert all(c["n"] == 700 and c["m"] == 5000 for c in A.CATEGORICAL)


def test_vector_is_in_the_box(case):
    z = _data(case)
    ell = z["ell"]
    assert ell.shape == (z["X"].shape[1],) and A.in_box(ell), (ell.min(), ell.max(), np.sqrt(len(ell)))
    if "which" not in case:
        if case["recipe"] in ("spread", "narrow") or not isinstance(case["recipe"], str):
            assert len(set(ell.tolist())) == len(ell)           # any permutation of indices changes the fit
        else:
            short = 0 if case["recipe"] == "one_short_first" else len(ell) - 1
            assert ell[short] == 0.05 * np.sqrt(len(ell)) and np.all(np.delete(ell, short) == case["common"])
        return
    # categorical: the groups are the product's, one value over all one-hot columns,
    # distinct values per numeric feature over a factor >= 40, PERM parameters apart
    gid, kinds, gv = z["gid"], z["kinds"], z["gvals"]
    assert np.array_equal(ell, gv[gid])
    col, cat_cols = 0, []
    for p in z["space"]:
        w = len(p.options) if p.options else 1
        if p.kind in (ENUM, BOOL):
            cat_cols += list(range(col, col + w))
        col += w
    assert col == len(ell) and cat_cols and len(set(ell[cat_cols].tolist())) == 1
    assert kinds.count("cat") == 1
    num = gv[[g for g, k in enumerate(kinds) if k == "num"]]
    assert len(set(num.tolist())) == len(num) >= 2 and num.max() / num.min() >= 40.0
    assert ell[cat_cols[0]] not in num.tolist()
    pv = gv[[g for g, k in enumerate(kinds) if k == "perm"]]
    assert np.all(np.diff(pv) != 0.0) and not set(pv.tolist()) & (set(num.tolist()) | {ell[cat_cols[0]]})
    for g in range(len(kinds)):
        assert len(set(ell[gid == g].tolist())) == 1


def test_oracle_is_self_consistent(case):
    z = _data(case)
    d = z["X"].shape[1]
    perm = np.random.default_rng(77 + d).permutation(d)
    g = ogp.GP(z["X"][:, perm], z["y"], lengthscale=z["ell"][perm], **A.hyper(case))
    mu, var = g.posterior(z["U"][:, perm])
    e_mu = A.worst(mu, z["mu"], A.RTOL, A.ATOL)
    e_var = A.worst(var, z["var"], A.RTOL, 1e-8)
    print("%s: permuted refit moves mu by %.3g, var by %.3g of the tolerance; cond(K) %.3g" %
          (case["name"], e_mu, e_var, np.linalg.cond(z["gp"].L) ** 2))
    assert e_mu <= 0.01 and e_var <= 0.01


def test_case_notices_a_wrong_lengthscale(case):
    z = _data(case)
    ell = z["ell"]
    if "which" in case:
        # roll among the numeric groups only (the one-hot columns keep their value)
        kinds, gv = z["kinds"], z["gvals"].copy()
        num = [g for g, k in enumerate(kinds) if k == "num"]
        gv[num] = np.roll(gv[num], 1)
        share = _moved(case, z, gv[z["gid"]])
        print("%s: roll over the numeric groups moves %.4f" % (case["name"], share))
        assert share > 0.5
        return
    first, last = ell.copy(), ell.copy()
    first[0], last[-1] = ell[1], ell[-2]
    s_roll, s_first, s_last = _moved(case, z, np.roll(ell, 1)), _moved(case, z, first), _moved(case, z, last)
    print("%s: roll moves %.4f, first %.4f, last %.4f" % (case["name"], s_roll, s_first, s_last))
    assert s_roll > 0.5
    if case["recipe"] == "one_short_first":
        assert s_first > 0.5
    if case["recipe"] == "one_short_last":
        assert s_last > 0.5
