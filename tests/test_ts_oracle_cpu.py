"""Thompson sampling without a GPU: cos2pi (the host build of ut_core.h
against its numpy restatement, bit for bit, and against long double), the
draws, the training-row identity, the paths' statistics, the pick rule's
exclusion, the case table of _ts_oracle.py (the fp64 and long-double
restatements must pick alike, or the GPU comparison would be vacuous), and the
technique's refusals and opt-in wiring."""
import ctypes
import inspect
import os
import re
import subprocess
import sys

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _ts_oracle as T  # noqa: E402
from oracle import mathx  # noqa: E402

LD = T.LD
HOSTLIB = os.path.join(ROOT, "uptune_amd", "libuthot_hostcheck.so")
needs_ld = pytest.mark.skipif(not T.have_longdouble(), reason="np.longdouble has fewer than 63 mantissa bits here")


@pytest.fixture(scope="module")
def hc():
    src = os.path.join(ROOT, "uptune_amd", "csrc", "hostcheck.cpp")
    core = os.path.join(ROOT, "uptune_amd", "csrc", "ut_core.h")
    if not os.path.exists(HOSTLIB) or os.path.getmtime(HOSTLIB) < max(os.path.getmtime(src), os.path.getmtime(core)):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", src, "-o",
                               HOSTLIB])
    lib = ctypes.CDLL(HOSTLIB)
    lib.uthc_cos2pi.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_longlong]
    lib.uthc_cos2pi.restype = None
    return lib


def cos_args():
    rng = np.random.default_rng(5)
    t = rng.uniform(-0.5, 0.5, size=1_000_000)
    sub = np.array([5e-324, 1e-310, 2.2250738585072014e-308])
    edge = np.array([0.0, 0.25, 0.5, 0.125, np.nextafter(0.125, 1), np.nextafter(0.25, 1), np.nextafter(0.25, 0),
                     np.nextafter(0.5, 0), 0.375])
    special = np.concatenate([edge, -edge, sub, -sub])
    t[:special.size] = special
    # ... and the phases' own shape: differences tau - rint(tau) of sums
    tau = rng.normal(scale=3.0, size=100_000)
    t[-tau.size:] = tau - np.rint(tau)
    return t


def test_cos2pi_host_equals_numpy_bit_for_bit(hc):
    t = cos_args()
    out = np.empty_like(t)
    hc.uthc_cos2pi(t.ctypes.data, out.ctypes.data, t.size)
    assert np.array_equal(out.view(np.uint64), T.cos2pi(t).view(np.uint64))
    # exact where the true value is representable
    for arg, want in ((0.0, 1.0), (0.25, 0.0), (-0.25, 0.0), (0.5, -1.0), (-0.5, -1.0), (5e-324, 1.0)):
        assert T.cos2pi(np.array([arg]))[0] == want


@needs_ld
def test_cos2pi_error_is_the_headers_cos_err():
    t = cos_args()
    err = float(np.max(np.abs(T.cos2pi(t).astype(LD) - T.cos_true(t))))
    print(f"max |cos2pi(t) - cos(2 pi t)| over {t.size} arguments: {err:.3e}")
    with open(os.path.join(ROOT, "uptune_amd", "csrc", "ut_core.h")) as fh:
        stated = float(re.search(r"UT_COS_ERR = ([0-9.e+-]+);", fh.read()).group(1))
    assert stated == T.COS_ERR
    assert err <= T.COS_ERR
    assert err >= T.COS_ERR / 4          # the stated bound is a measurement, not a guess


def test_inv_2pi_is_the_nearest_double():
    with open(os.path.join(ROOT, "uptune_amd", "csrc", "ut_core.h")) as fh:
        stated = float(re.search(r"UT_INV_2PI = ([0-9.e+-]+);", fh.read()).group(1))
    assert stated == T.INV_2PI
    if T.have_longdouble():
        assert T.INV_2PI == float(LD(1) / (LD(2) * T.LD_PI))


def test_normal_is_mathx_normal_draw():
    cand = np.arange(300, dtype=np.uint64)
    for stream in (0, 4, 63, 5 | (1 << 28), 255 | (2 << 28)):
        want = mathx.normal_draw(11, cand, stream, 3, T.OP_TS)
        got = T.normal(11, cand, np.uint64(stream), 3)
        assert np.array_equal(want.view(np.uint64), got.view(np.uint64))
    dr = T.draws(11, 7, 5, 3, 128, 3)
    assert np.array_equal(dr["Z"][:, 4], mathx.normal_draw(11, np.arange(128, dtype=np.uint64), 4, 3, T.OP_TS))
    assert np.array_equal(dr["Theta"][2], mathx.normal_draw(11, np.arange(128, dtype=np.uint64), 2 | (1 << 28), 3,
                                                             T.OP_TS))
    assert np.array_equal(dr["Eps"][1], mathx.normal_draw(11, np.arange(7, dtype=np.uint64), 1 | (2 << 28), 3,
                                                           T.OP_TS))
    assert ((dr["b"] >= 0.0) & (dr["b"] < 1.0)).all()
    # another round, another draw
    assert not np.array_equal(dr["Z"], T.draws(11, 7, 5, 3, 128, 4)["Z"])


def _fit_and_draws(c, dtype):
    z = T.data(c)
    fit = T.Fit(z["X"], z["y"], z["ell"], c["sf2"], c["sn2"], c["jitter"], dtype)
    dr = T.draws(T.seed_of(c), c["n"], z["d"], c["q"], c["D"], T.round_of(c))
    return z, fit, dr


def _identity_residual(fit, dr, A, X):
    """f_s(x_r) + sqrt(diag) Eps[s][r] + diag a_s[r] - ys[r], and the largest of the identity's terms: its
    summands as they are added, Theta[s][j] phi_j(x_r) and k(x_i, x_r) a_s[i] among them.  (f_s(x_r) is a sum
    of n + D such terms that cancel down to the size of ys; no arithmetic holds a sum to a fraction of an ulp
    of its result when its summands are larger, so the summands are what the error is measured in.)"""
    dt = fit.dtype
    Xs = fit.scaled(X)
    F = T.evaluate(fit, dr, A, X)
    noise = np.sqrt(dt(fit.diag)) * dr["Eps"].astype(dt)
    res = F + noise + dt(fit.diag) * A - fit.ys[None, :]
    Kf = np.abs(T.kernel(fit.Xs, Xs, fit.sf2)).astype(np.float64)
    ka = max(float(np.max(np.abs(np.asarray(A[s], dtype=np.float64))[:, None] * Kf)) for s in range(A.shape[0]))
    amp = np.sqrt(2.0 * fit.sf2 / dr["Z"].shape[0])
    terms = max(ka, amp * float(np.max(np.abs(dr["Theta"]))), float(np.max(np.abs(noise))),
                float(np.max(np.abs(dt(fit.diag) * A))), float(np.max(np.abs(fit.ys))))
    return res, terms


@needs_ld
@pytest.mark.parametrize("c", T.CASES, ids=T.ids())
def test_training_row_identity_long_double(c):
    z, fit, dr = _fit_and_draws(c, LD)
    res, terms = _identity_residual(fit, dr, T.weights(fit, dr), z["X"])
    worst = float(np.max(np.abs(res)))
    print(f"{c['name']}: identity residual {worst:.3e}, max |term| {terms:.3e}")
    assert worst <= 64 * 2.0 ** -64 * terms


@pytest.mark.parametrize("c", T.CASES, ids=T.ids())
def test_training_row_identity_fp64_at_the_tier(c):
    rtol = dict(T.TIERS)[c["sn2"]]
    z, fit, dr = _fit_and_draws(c, np.float64)
    res, terms = _identity_residual(fit, dr, T.weights(fit, dr), z["X"])
    worst = float(np.max(np.abs(res)))
    print(f"{c['name']}: identity residual {worst:.3e}, bound {rtol * terms:.3e}")
    assert worst <= rtol * terms


def test_path_statistics():
    """n = 100, d = 5, ell = 0.5, D = 1024, 2000 paths, 200 candidates"""
    n, d, D, q, m = 100, 5, 1024, 2000, 200
    rng = np.random.default_rng(77)
    X = rng.uniform(size=(n, d))
    y = np.sum((X - 0.4) ** 2, axis=1) + 0.01 * rng.standard_normal(n)
    U = rng.uniform(size=(m, d))
    fit = T.Fit(X, y, 0.5, 1.0, 1e-2, 1e-8)
    dr = T.draws(3, n, d, q, D, 9)
    F = T.evaluate(fit, dr, T.weights(fit, dr), U)
    Ks = T.kernel(fit.Xs, fit.scaled(U), fit.sf2)
    from scipy.linalg import solve_triangular
    V = solve_triangular(fit.L, Ks, lower=True)
    mu = Ks.T @ solve_triangular(fit.L.T, solve_triangular(fit.L, fit.ys, lower=True), lower=False)
    var = fit.sf2 - np.sum(V * V, axis=0)
    se = F.std(axis=0, ddof=1) / np.sqrt(q)
    zmax = float(np.max(np.abs(F.mean(axis=0) - mu) / se))
    ratio = float(np.median(F.var(axis=0, ddof=1) / var))
    print(f"path mean: max {zmax:.2f} standard errors; median variance ratio {ratio:.3f}")
    assert zmax <= 6.0
    assert 0.8 <= ratio <= 1.25
    # the minimisers collide: what the sequential exclusion is for
    print(f"distinct minimisers among {q} paths: {len(set(np.argmin(F, axis=1).tolist()))}")


def test_exclusion():
    n, d, D, q, m = 100, 5, 256, 17, 200
    rng = np.random.default_rng(78)
    X = rng.uniform(size=(n, d))
    y = np.sum((X - 0.4) ** 2, axis=1)
    U = rng.uniform(size=(m, d))
    fit = T.Fit(X, y, 0.5, 1.0, 1e-2, 1e-8)
    dr = T.draws(3, n, d, q, D, 2)
    F = T.evaluate(fit, dr, T.weights(fit, dr), U)
    assert len(set(np.argmin(F, axis=1).tolist())) < q         # the unexcluded minimisers do collide
    pos, f = T.select(F, None, q)
    assert len(set(pos.tolist())) == q and (pos >= 0).all()
    taken = np.zeros(m, dtype=bool)
    for s in range(q):
        rest = np.flatnonzero(~taken)
        assert pos[s] == rest[np.argmin(F[s, rest])] and f[s] == F[s, pos[s]]
        taken[pos[s]] = True
    dup = np.ones(m, dtype=np.uint8)
    dup[rng.permutation(m)[:10]] = 0
    pos, f = T.select(F, dup, q)
    assert (pos[:10] >= 0).all() and len(set(pos[:10].tolist())) == 10 and (dup[pos[:10]] == 0).all()
    assert (pos[10:] == -1).all() and np.isinf(f[10:]).all() and (f[10:] > 0).all()
    pos, f = T.select(F, np.ones(m, dtype=np.uint8), 3)
    assert (pos == -1).all()
    Fn = F.copy()
    Fn[1, 5] = np.nan
    pos, f = T.select(Fn, None, 4)
    assert pos[0] >= 0 and (pos[1:] == -1).all()               # a NaN minimum empties its slot and the rest
    Ft = np.zeros((2, 6))
    assert T.select(Ft, None, 2)[0].tolist() == [0, 1]         # ties: the smallest position


@needs_ld
@pytest.mark.parametrize("c", T.CASES, ids=T.ids())
def test_case_table_fp64_and_long_double_pick_alike(c):
    z, f64, dr = _fit_and_draws(c, np.float64)
    _, fld, _ = _fit_and_draws(c, LD)
    A64, Ald = T.weights(f64, dr), T.weights(fld, dr)
    F64, Fld = T.evaluate(f64, dr, A64, z["U"]), T.evaluate(fld, dr, Ald, z["U"])
    k = c["q"]
    p64, _ = T.select(F64, z["dup"], k)
    pld, _ = T.select(Fld, z["dup"], k)
    err = float(np.max(np.abs(F64.astype(LD) - Fld)))
    g = T.gap(Fld, z["dup"], k)
    print(f"{c['name']}: max |F64 - Fld| {err:.3e}, smallest gap {float(np.min(g)):.3e}, "
          f"picks {int(np.sum(pld >= 0))} of {k}")
    assert np.array_equal(p64, pld)
    assert float(np.min(g)) > 4 * err                          # ... and by a margin, not by luck
    if c["ell"] == "tiny":                                     # far from all data: the prior path alone
        far = T.prior(fld, dr, fld.scaled(z["U"][-1:]))
        assert np.array_equal(Fld[:, -1:], far)


def test_case_table_covers_the_issue():
    cs = T.CASES
    assert {c["n"] for c in cs} >= {1, 100, 129}
    assert {c["d"] for c in cs} >= {5, 64}
    assert {c["D"] for c in cs} >= {128, 256}
    assert {c["m"] for c in cs} >= {1, 127, 129, 1000}
    assert {c["q"] for c in cs} >= {1, 3, 33, 70}
    assert any(c["ell"] == "ard" for c in cs) and any(c["space"] for c in cs)
    assert {c["sn2"] for c in cs} == {sn2 for sn2, _ in T.TIERS}
    from oracle.space import BOOL, ENUM, FLOAT, INT, LOGINT, PERM, POW2
    assert {p.kind for p in T.mixed_space()} == {BOOL, ENUM, FLOAT, INT, LOGINT, PERM, POW2}


# --------------------------------------------------------------------------- the technique, without a device
def test_refusals():
    from uptune_amd.technique import GpuDifferentialEvolution, GpuTrustRegion, SharedModel
    for cls in (GpuDifferentialEvolution, GpuTrustRegion):
        for kw in (dict(prune_rows=128), dict(diversify=64), dict(polish=4), dict(feasibility=True),
                   dict(constraints=[("accuracy", ">=", 0.5)]), dict(surrogate="forest"), dict(surrogate=object()),
                   dict(ts_features=100), dict(ts_features=64), dict(ts_features=8192), dict(batch=300, pool=1024)):
            with pytest.raises(ValueError):
                cls(acq="ts", **kw)
            kw.pop("ts_features", None)
            if kw:
                cls(acq="ei", **kw)                             # ... and only with acq="ts"
    for sm in (SharedModel(feasibility=True), SharedModel(constraints=[("accuracy", ">=", 0.5)]),
               SharedModel(surrogate="forest")):
        with pytest.raises(ValueError):
            GpuDifferentialEvolution(acq="ts", shared=sm)
    t = GpuTrustRegion(acq="ts", ts_features=256)
    assert t.acq_kind == "ts" and t.ts_features == 256


def test_off_by_default_and_wired_through():
    from uptune_amd import technique as tq
    from uptune_amd.tuner import tune_bandit
    assert tq.GpuDifferentialEvolution().acq_kind == "ei"
    sig = inspect.signature(tune_bandit)
    assert sig.parameters["acq"].default == "ei" and sig.parameters["ts_features"].default == 1024
    for factory in (tq.bandit_a, tq.bandit_b, tq.pso_ga_de_bandit):
        assert all(t.acq_kind == "ei" for t in factory(trust_region=True).techniques)
        kids = factory(trust_region=True, acq="ts", ts_features=512).techniques
        assert all(t.acq_kind == "ts" and t.ts_features == 512 for t in kids)
        assert any(isinstance(t, tq.GpuTrustRegion) for t in kids)
        assert len({id(t.model) for t in kids}) == 1
    reg = tq.reference_registry(acq="ts", trust_region=True)
    assert all(t.acq_kind == "ts" for t in reg if isinstance(t, tq.GpuBatchTechnique))
    # the draws' key: a counter on the shared model, 24 bits
    m = tq.SharedModel()
    assert [m.next_ts_round() for _ in range(3)] == [0, 1, 2]
    m.ts_rounds = (1 << 24) + 5
    assert m.next_ts_round() == 5
