"""The weighted pruned selection on the CPU: the restatement
(tests/_prune_weight_cases.py) is sound and selects what the dense weighted
ranking selects on every case of the shared table, each case sits in the
regime the table claims for it, its selection is decidable on the reference
alone, the constraint-weight bound dominates the weight wherever var <= var_ub,
and the cases that claim it prune only because of that bound -- so the GPU
tests of the same table (test_gpu_prune_weight.py) can assert without
conditions."""
import numpy as np
import pytest

import _prune_oracle as po
import _prune_weight_cases as pw
from _cons_oracle import cons_prob


@pytest.fixture(params=pw.CASES, ids=pw.case_ids())
def case(request):
    return request.param


def test_case_table_covers_the_issue():
    W = pw.CASES
    assert len({w["name"] for w in W}) == len(W)
    one = {w["thr"] for w in W if w["base"] == "d64_l2" and len(w["thr"]) == 1 and not w["nfail"]}
    assert {(1.0,), (0.6,), (0.35,), (-1.0,)} <= one
    assert {2, 4} <= {len(w["thr"]) for w in W if w["base"] == "d64_l2"}
    assert any(w["base"] == "d6_l008" and w["nfail"] == 64 for w in W)
    assert any(w["base"] == "d3_n129" and w["nfail"] == 30 for w in W)
    assert any(w["base"] == "m257" and w["nfail"] == 30 for w in W)
    assert any(w["base"] == "d16_k1" and w["nfail"] == 40 and pw.base_case(w)["cand_base"] == 2 ** 40 for w in W)
    assert any(w["base"].startswith("late_") and w["regime"] == "dense" for w in W)
    assert any(w["base"] == "flat_ei0" and w["regime"] == "flat" for w in W)
    assert any(w["base"].startswith("few_") and w["regime"] == "few_valid" for w in W)
    assert any(w["base"] == "ard_d64_ei" and w["nfail"] == 100 for w in W)
    assert any(w["vote"].get("power", 1.0) != 1.0 for w in W)
    assert any(w["vote"].get("prior") is not None for w in W)
    assert any(w["vote"].get("ell_scale", 1.0) != 1.0 for w in W)
    assert any(not w["thr"] and w["nfail"] for w in W)           # the vote alone
    assert any(pw.case_data(w)["cg"].n_feasible == 0 for w in W)  # the score is P alone
    assert all(pw.base_case(w)["n"] <= 1024 and pw.base_case(w)["m"] <= 5000 for w in W)
    assert all(w["nfail"] > 0 for w in W if w["vote"])


def test_bound_is_sound_and_selection_is_the_dense_one(case):
    c, r = pw.base_case(case), pw.case_restated(case)
    v = r["valid"]
    for tag in ("", "_e"):
        assert np.all(r["bound" + tag][v] >= r["score"][v])
        assert np.all(r["bound" + tag][~v] == -np.inf)
        want = sorted(np.flatnonzero(v).tolist(), key=lambda i: (-r["score"][i], i))[:c["k"]]
        assert r["sel" + tag].tolist() == want
    assert np.all(r["bound"] <= r["bound_e"])   # (each Pub_j <= 1)
    assert np.all(r["p"] > 0.0) and np.all(r["p"] <= 1.0)


def test_case_is_in_its_regime(case):
    c, r = pw.base_case(case), pw.case_restated(case)
    m, k, v = c["m"], c["k"], r["valid"]
    ns = int(r["keep"].sum())
    print("%s: feasible rows %d, survivors %d (EI-only bound %d) of %d" %
          (case["name"], pw.case_data(case)["cg"].n_feasible, ns, int(r["keep_e"].sum()), m))
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
        s = np.sort(r["score"][v])
        if s.size > 1 and not np.all(s == s[0]):
            assert np.all(np.diff(s) > 1e-5 * np.abs(s[1:]) + 1e-8)


def test_selection_is_decidable(case):
    """prunes and dense cases: the gap behind the k-th best score exceeds the band the
    GPU test compares selections in -- the oracle band, or for a declared tie the
    device-path band"""
    if case["regime"] not in ("prunes", "dense"):
        return
    c, r = pw.base_case(case), pw.case_restated(case)
    s = np.sort(r["score"][r["valid"]])[::-1]
    k = c["k"]
    t, gap = s[k - 1], s[k - 1] - s[k]
    assert t > 0.0
    if case["tie"]:
        assert gap <= 1e-5 * t + 1e-8, "not a tie at the oracle band: drop the declaration"
        assert gap > 1e-9 * t + 1e-12
    else:
        assert gap > 1e-5 * t + 1e-8


def test_constraints_help_where_the_table_says(case):
    """the EI-only bound on the same scores leaves the regime (dense, or more than m / 4
    survivors) where the weighted bound stays in it"""
    c, r = pw.base_case(case), pw.case_restated(case)
    m = c["m"]
    ns, ns_e = int(r["keep"].sum()), int(r["keep_e"].sum())
    assert ns <= ns_e
    if case["helps"]:
        assert case["regime"] == "prunes" and ns <= m / 4
        assert r["dense_e"] or ns_e > m / 4


def test_pub_dominates_p_on_random_inputs():
    """Pub >= P for every var <= var_ub, on random (mu_c, tau, var_ub) including var == 0,
    var_ub == 0 and mu_c == tau"""
    rng = np.random.default_rng(11)
    n, nc = 200000, 4
    tau = rng.standard_normal(nc) * 1.5
    mu_c = rng.standard_normal((nc, n)) * 2.0
    mu_c[:, :100] = tau[:, None]
    var_ub = 10.0 ** rng.uniform(-12, 1.5, n)
    var_ub[100:200] = 0.0
    var = var_ub * rng.uniform(0.0, 1.0, n)
    var[200:300] = 0.0
    var[300:400] = var_ub[300:400]
    for j in range(1, nc + 1):
        P = cons_prob(var, mu_c[:j], tau[:j])
        Pub = pw.P_ub(var_ub, mu_c[:j], tau[:j])
        assert np.all(Pub >= P)
        assert np.all(Pub <= 1.0) and np.all(Pub >= 0.0)


def test_envelope_brackets_the_score(case):
    """envelope_w's two sides bracket the restated score at both tolerances"""
    c, z, r = pw.base_case(case), pw.case_data(case), pw.case_restated(case)
    cg, v = z["cg"], r["valid"]
    power = pw.vote_params(case)[3]
    for tol in (po.PATH_TOL, po.ORACLE_TOL):
        a = (r["mu"], r["var"], r["mu_c"], r["p"], cg.tau, cg.f_best_c, cg.n_feasible, c["acq"], c["sf2"], power, tol)
        lo, hi = pw.envelope_w(*a), pw.envelope_w(*a, upper=True)
        assert np.all(lo[v] <= r["score"][v]) and np.all(r["score"][v] <= hi[v] * (1.0 + 1e-12) + 1e-300)
