"""The acquisition's gradient on the device (csrc/gp_polish.hip, ut_gp_acq_grad)
against the formulas restated over oracle/gp.py (tests/_polish_oracle.py, held
to finite differences and long double by tests/test_polish_oracle_cpu.py).

Tiers are the project's (test_gpu_lml.py, test_gpu_batch_select.py): rtol 1e-9
at sigma_n2 = 1e-2, 1e-5 at sigma_n2 = 1e-6.  mu and score are held to
rtol (|x| + max |x| over the case) (scores underflow, means cancel), var to
rtol (|var| + sigma_f2) (a difference of quantities of size sigma_f2 = 1), and
the gradient to rtol max |g_oracle| over the case, absolutely: the oracle's own
rounding there is 1.3e-12 and 3.9e-11 of it at the two tiers (long double),
well inside."""
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
from oracle.space import BOOL, ENUM, FLOAT, INT, LOGINT, PERM, POW2, Param  # noqa: E402

pytestmark = pytest.mark.gpu

CASES = P.CASES + [(200, 37, 300, "ard")]
UT_EINVAL = -1
MIXED = [Param("f", FLOAT, -3.0, 5.0), Param("i", INT, 1, 500), Param("l", LOGINT, 1, 4096),
         Param("p", POW2, 2, 256), Param("b", BOOL), Param("e", ENUM, options=list("vwxyz")),
         Param("q", PERM, options=list(range(6))), Param("g", FLOAT, 0.0, 1.0)]

_ENGINES = {}
_RUNS = {}


def ell_of(case):
    return O.ard_base(case[1]) if isinstance(case[3], str) else case[3]


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


def fit(e, case, sn2):
    n, d = case[:2]
    X, y = O.data(n, d)
    e.gp_fit(X, y, lengthscale=ell_of(case), sigma_n2=sn2)


def run(case, sn2, kind):
    """the device's and the oracle's results of a case; computed once, shared, never written"""
    key = (case, sn2, kind)
    if key not in _RUNS:
        n, d, p = case[:3]
        U = P.cands(n, d, p)
        e = engine(d)
        fit(e, case, sn2)
        got = host(*e.gp_acq_grad(dev(U.T), acq=e.acq(kind)))
        want = P.score_grad(P.gp_of(n, d, ell_of(case), sn2), U, kind)
        for a in got:
            a.setflags(write=False)
        _RUNS[key] = (got, want)
    return _RUNS[key]


@pytest.mark.parametrize("kind", P.KINDS)
@pytest.mark.parametrize("sn2,rtol", P.TIERS)
@pytest.mark.parametrize("case", CASES)
def test_against_the_oracle(case, sn2, rtol, kind):
    (score, mu, var, grad), w = run(case, sn2, kind)
    gm = np.abs(w["grad"]).max()
    e_g = np.abs(grad.T - w["grad"]).max()
    e_s = np.max(np.abs(score - w["score"]) / (np.abs(w["score"]) + np.abs(w["score"]).max()))
    e_m = np.max(np.abs(mu - w["mu"]) / (np.abs(w["mu"]) + np.abs(w["mu"]).max()))
    e_v = np.max(np.abs(var - w["var"]) / (np.abs(w["var"]) + 1.0))
    zero = np.abs(w["grad"]).max(axis=1) == 0.0
    print(f"{case} sn2={sn2:g} {kind}: grad err {e_g / gm:.3e} of max|g| = {gm:.3g}; score {e_s:.3e}, mu {e_m:.3e}, "
          f"var {e_v:.3e} (rtol {rtol:g}); rows with a zero oracle gradient: {zero.sum()}")
    assert np.isfinite(grad).all() and np.isfinite(score).all()
    assert e_s <= rtol and e_m <= rtol and e_v <= rtol
    assert e_g <= rtol * gm


def test_flat_ei_is_finite_and_small():
    """EI at (321, 3, 1024, 0.3), sigma_n2 = 1e-6 underflows for most candidates:
    the oracle's gradient is exactly zero there, the device's finite and inside the same bound"""
    (score, mu, var, grad), w = run(P.CASES[2], 1e-6, "ei")
    zero = np.abs(w["grad"]).max(axis=1) == 0.0
    assert zero.sum() >= 900
    assert np.isfinite(grad[:, zero]).all()
    assert np.abs(grad[:, zero]).max() <= 1e-5 * np.abs(w["grad"]).max()


@pytest.mark.parametrize("kind", P.KINDS)
def test_two_calls_return_equal_bits(kind):
    case = CASES[1]
    n, d, p = case[:3]
    e = engine(d)
    fit(e, case, 1e-2)
    U = dev(P.cands(n, d, p).T)
    a = host(*e.gp_acq_grad(U, acq=e.acq(kind)))
    b = host(*e.gp_acq_grad(U, acq=e.acq(kind)))
    for x, y in zip(a, b):
        assert x.tobytes() == y.tobytes()
    for x, y in zip(a, run(case, 1e-2, kind)[0]):        # ... and what an earlier engine state gave
        assert x.tobytes() == y.tobytes()
    # the score is the scoring path's within the tier, mu and var too
    mu, var, score = host(*e.gp_score_values(U, acq=e.acq(kind)))
    assert np.max(np.abs(a[0] - score) / (np.abs(score) + np.abs(score).max())) <= 1e-9
    assert np.max(np.abs(a[1] - mu) / (np.abs(mu) + np.abs(mu).max())) <= 1e-9
    assert np.max(np.abs(a[2] - var) / (np.abs(var) + 1.0)) <= 1e-9


def test_same_after_a_precision_8_refit():
    """a precision-8 refit leaves (L^-1)^T and alpha out: the call writes them itself"""
    case = CASES[0]
    n, d, p = case[:3]
    got, _ = run(case, 1e-2, "ei")
    e = engine(d)
    e.gp_set_precision(8)
    fit(e, case, 1e-2)
    again = host(*e.gp_acq_grad(dev(P.cands(n, d, p).T), acq=e.acq("ei")))
    e.gp_set_precision(64)
    gm = np.abs(got[3]).max()
    assert np.abs(again[3] - got[3]).max() <= 1e-9 * gm
    assert np.max(np.abs(again[0] - got[0])) <= 1e-9 * np.abs(got[0]).max()


@pytest.mark.parametrize("kind", P.KINDS)
def test_mixed_space_feature_columns(kind):
    """FLOAT, INT, LOGINT, POW2, BOOL, ENUM, PERM: the gradient row of a feature
    is its own column's, one-hot and PERM columns included"""
    import torch
    from uptune_amd.engine import BatchEngine
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    e = BatchEngine(to_manip(MIXED), device=0, seed=5)
    e.population_init(512, round_=0)
    vals = e.population_get().contiguous()
    tr, sl = vals[:, :150].contiguous(), vals[:, 150:450].contiguous()
    X = e.encode(tr).cpu().numpy().T
    F = X.shape[1]
    assert F == e.spec.n_features and F > len(MIXED)
    rng = np.random.default_rng(3)
    y = np.sum((X - 0.4) ** 2, axis=1) + 0.01 * rng.standard_normal(150)
    ell = 0.5 * O.ard_base(F)
    xi = -1.0 if kind == "ei" else 0.0     # (the plain EI underflows for most of this shortlist)
    e.gp_fit(X, y, lengthscale=ell, sigma_n2=1e-2)
    score, mu, var, grad = host(*e.gp_acq_grad(sl, acq=e.acq(kind, xi=xi)))
    U = e.encode(sl).cpu().numpy().T
    w = P.score_grad(ogp.GP(X, y, lengthscale=ell, sigma_n2=1e-2), U, kind, xi=xi)
    gm = np.abs(w["grad"]).max()
    err = np.abs(grad.T - w["grad"]).max(axis=0)          # per feature column
    print(f"mixed {kind}: grad err {err.max() / gm:.3e} of max|g| = {gm:.3g}; per-column max|g| "
          f"{np.abs(w['grad']).max(axis=0).min():.3g} .. {gm:.3g}")
    assert (np.abs(w["grad"]).max(axis=0) > 1e-6 * gm).all()   # every column has a derivative to get wrong
    assert (err <= 1e-9 * gm).all()
    assert np.max(np.abs(score - w["score"]) / (np.abs(w["score"]) + np.abs(w["score"]).max())) <= 1e-9
    e.close()


def test_failed_fit_gives_nan_scores():
    case = CASES[0]
    n, d, p = case[:3]
    X, y = O.data(n, d)
    e = engine(d, fresh=True)
    e.gp_fit(X, y, lengthscale=case[3], sigma_n2=-2.0, jitter=0.0, wait=False)   # not positive definite
    score = e.gp_acq_grad(dev(P.cands(n, d, p).T))[0].cpu().numpy()           # rc == 0: no exception
    assert np.isnan(score).all()
    assert not e.gp_fit_ok()
    e.close()


def test_bad_arguments_and_failed_allocation():
    import torch
    from uptune_amd import _lib as L
    case = CASES[0]
    n, d, p = case[:3]
    e = engine(d, fresh=True)
    U = dev(P.cands(n, d, p).T)
    acq = e.acq("ei")
    mu = torch.empty(p, dtype=torch.float64, device="cuda:0")
    g = torch.empty((d, p), dtype=torch.float64, device="cuda:0")

    def call(values=U.data_ptr(), ld=p, pp=p, a=ctypes.byref(acq), m=mu.data_ptr(), gr=g.data_ptr(), ldg=p):
        return e.lib.ut_gp_acq_grad(e.ctx, values, ld, pp, a, None, m, None, gr, ldg)
    assert call() == UT_EINVAL                           # no fit at all
    fit(e, case, 1e-2)
    assert call() == 0
    for bad in (dict(pp=0), dict(pp=4097, ld=4097, ldg=4097), dict(values=None), dict(a=None), dict(m=None),
                dict(gr=None), dict(ld=p - 1), dict(ldg=p - 1)):
        assert call(**bad) == UT_EINVAL, bad
    with pytest.raises(ValueError):                      # a column count that is not the space's
        e.gp_acq_grad(U[:d - 1])
    # constraint values or failed rows loaded: the weighted score's gradient is not built
    X, y = O.data(n, d)
    e.gp_cons_set(np.sum(X, axis=1), [2.5])
    assert call() == UT_EINVAL
    e.gp_cons_clear()
    assert call() == 0
    e.gp_feas_set(np.random.default_rng(1).uniform(size=(7, d)))
    assert call() == UT_EINVAL
    e.gp_feas_clear()
    assert call() == 0
    # the scratch goes through the counted allocations
    e2 = engine(d, fresh=True)
    fit(e2, case, 1e-2)
    assert e2.lib.ut_debug_fail_alloc(e2.ctx, 1) == 0
    with pytest.raises(L.UthotError, match="UT_ENOMEM"):
        e2.gp_acq_grad(U)
    assert np.isfinite(e2.gp_acq_grad(U)[3].cpu().numpy()).all()      # ... and the following call succeeds
    e.close()
    e2.close()
