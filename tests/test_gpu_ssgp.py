"""The sparse-spectrum GP on the device (csrc/ssgp.hip: ut_ssgp_fit / _score /
_read) against the rule restated in tests/_ssgp_oracle.py, whose docstring
derives every bound used here.

Z, b bit for bit; A, c, w, mu, var within the derived bounds in long double (w, mu, var from
the device's own operands); L, L^-1 by their residuals on the device's own A, at most four times
numpy's fp64 ones (test_gpu_fit_factor.py's rule).  D = 2048 at n = 513 has two-step units: A is
held there on three tiles and the factor's residuals are not taken (long double at 2048^3)."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _ssgp_oracle as S  # noqa: E402
import _ts_oracle as T  # noqa: E402
from _spaces import to_manip  # noqa: E402
from oracle import gp as ogp  # noqa: E402

pytestmark = pytest.mark.gpu
LD = S.LD
SEED = 11


def _c(n, d, D, m, space=None, ell="iso", cols=None):
    return dict(name="n%d_d%s_D%d_m%d" % (n, "mix" if space else d, D, m), n=n, d=d, D=D, m=m, space=space, ell=ell,
                cols=cols)


# n = 129 is one row past a 128-row step, which at D <= 384 is also a unit of the Gram's split (S.split)
CASES = [_c(1, 1, 128, 1), _c(127, 5, 128, 127), _c(129, 65, 384, 130, ell="ard"), _c(129, 5, 128, 130),
         _c(300, 0, 384, 127, space="mixed"),
         _c(513, 5, 2048, 20, cols=np.r_[0:128, 1920:2048])]
IDS = [c["name"] for c in CASES]
_RUNS = {}


def dev(a):
    import torch
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")


def engine(c, monkeypatch=None, env=None):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)           # (read when the context is created)
    from uptune_amd.engine import BatchEngine
    return BatchEngine(to_manip(T.data(c)["space"]), device=0, seed=SEED)


def fit(e, c, sn2=1e-2, jitter=0.0):
    z = T.data(c)
    e.ssgp_fit(z["X"], z["y"], lengthscale=z["ell"], sigma_f2=1.0, sigma_n2=sn2, jitter=jitter, features=c["D"])


def run(c):
    if c["name"] not in _RUNS:
        assert T.have_longdouble()
        z, e = T.data(c), engine(c)
        fit(e, c)
        r = {k: e.ssgp_read(k) for k in ("Z", "b", "A", "c", "L", "Linv", "w")}
        r["info"] = e.ssgp_read(None)
        r["post"] = [t.cpu().numpy() for t in e.ssgp_score(dev(z["cand"]), dup=dev(z["dup"]))]
        r["e"] = e
        _RUNS[c["name"]] = r
    return _RUNS[c["name"]]


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_draws_gram_factor_and_weights(c):
    z, r = T.data(c), run(c)
    assert r["info"] == dict(n=c["n"], d=z["d"], D=c["D"], ok=True)
    assert c["cols"] is None or S.split(c["n"], c["D"]) == (2, 3)
    Z, b = S.draws(SEED, z["d"], c["D"])
    assert np.array_equal(r["Z"], Z) and np.array_equal(r["b"], b)
    A, cv, eA, ec = S.gram(z["X"], z["y"], z["ell"], Z, b, 1.0, 1e-2, c["cols"])
    Adev = r["A"] if c["cols"] is None else r["A"][np.ix_(c["cols"], c["cols"])]
    assert np.all(np.abs(Adev.astype(LD) - A) <= eA) and np.array_equal(r["A"], r["A"].T)
    assert np.all(np.abs(r["c"].astype(LD) - cv) <= ec)
    w, ew = S.weights(r["Linv"], r["c"])
    assert np.all(np.abs(r["w"].astype(LD) - w) <= ew)              # (n = 1: ys = 0, so c = w = 0 and the bound too)
    assert not np.triu(r["L"], 1).any() and not np.triu(r["Linv"], 1).any()
    if c["cols"] is not None:
        return
    Ad = r["A"].astype(LD)   # the factor and its inverse on the device's own A, beside numpy's fp64 on the same A

    def res(L, X):
        Ll, Xl = L.astype(LD), X.astype(LD)
        a = np.abs(Ll @ Ll.T - Ad) / (np.abs(Ll) @ np.abs(Ll).T)
        lo = np.tril_indices(len(L))                 # (above the diagonal both sides are exact zeros)
        i = np.abs(Xl @ Ll - np.eye(len(L), dtype=LD))[lo] / (np.abs(Xl) @ np.abs(Ll))[lo]
        return float(a.max()), float(i.max())
    Ln = np.linalg.cholesky(r["A"])
    (da, di), (na, ni) = res(r["L"], r["Linv"]), res(Ln, np.linalg.inv(Ln))
    assert da <= 4.0 * na and di <= 4.0 * ni


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_posterior_and_score(c):
    z, r = T.data(c), run(c)
    mu, var, sc = r["post"]
    want_mu, want_var, emu, evar = S.posterior(z["U"], z["ell"], r["Z"], r["b"], 1.0, 1e-2, r["Linv"], r["w"])
    assert np.all(np.abs(mu.astype(LD) - want_mu) <= emu) and np.all(np.abs(var.astype(LD) - want_var) <= evar)
    assert (var >= 0.0).all()
    ys, eys = S.ystd(z["y"])
    k = int(np.argmin(ys))
    sg = np.sqrt(var)
    tol = 64 * S.U * (np.abs(ys[k] - mu) + sg) + eys[k] + 1e-300
    dup = z["dup"] != 0
    assert np.all(np.abs(sc - ogp.acquisition(mu, var, ys[k]))[~dup] <= tol[~dup])
    assert np.all(sc[dup] == -np.inf)
    ucb = r["e"].ssgp_score(dev(z["cand"]), acq=r["e"].acq("ucb", kappa=1.5))[2].cpu().numpy()
    assert np.all(np.abs(ucb - (1.5 * sg - mu)) <= 4 * S.U * (1.5 * sg + np.abs(mu)))
    if c["ell"] == "ard":   # ... and at the default noise 1e-6 + 1e-8: finite, var >= 0, ok
        e = engine(c)
        fit(e, c, sn2=1e-6, jitter=1e-8)
        out = np.stack([t.cpu().numpy() for t in e.ssgp_score(dev(z["cand"]))])
        assert e.ssgp_read(None)["ok"] and np.isfinite(out).all() and (out[1] >= 0.0).all()


@pytest.mark.parametrize("D", [384, 1024])
def test_same_bits_however_the_launches_are_cut(monkeypatch, D):
    """the grid changes (two units per workgroup), the units and so every sum's order do not: another unit LENGTH
    would change the bits, which is why it is a function of (n, D) alone.  A pool whole, in two calls and in two
    Phi* chunks (capped at 256 candidates); D = 1024 is where the variance contraction could split its k loops"""
    c = _c(300, 5, D, 300)
    z, r = T.data(c), run(c)
    assert S.split(c["n"], D)[1] == 3
    e2 = engine(c, monkeypatch, {"UT_SSGP_UNITS_PER_WG": "2", "UT_SSGP_PHI_MIB": str(D // 384)})
    fit(e2, c)
    fit(r["e"], c)
    for k in ("A", "c", "Linv", "w"):
        assert np.array_equal(e2.ssgp_read(k), r[k]) and np.array_equal(r["e"].ssgp_read(k), r[k]), k
    cand = dev(z["cand"])
    for a, b in zip(e2.ssgp_score(cand, dup=dev(z["dup"])), r["post"]):
        assert np.array_equal(a.cpu().numpy(), b)            # two chunks, of 256 and of 44
    lo = r["e"].ssgp_score(cand[:, :130].contiguous(), dup=dev(z["dup"][:130]))
    hi = r["e"].ssgp_score(cand[:, 130:].contiguous(), dup=dev(z["dup"][130:]))
    for a, b, w in zip(lo, hi, r["post"]):
        assert np.array_equal(np.concatenate([a.cpu().numpy(), b.cpu().numpy()]), w)


def test_refusals():
    from uptune_amd._lib import UthotError
    c = CASES[1]
    z, e = T.data(c), engine(c)
    cand, acq, X, y = dev(z["cand"]), e.acq(), z["X"], z["y"]
    big = (np.zeros((65537, z["d"])), np.zeros(65537))
    calls = [(e.ssgp_score, (cand,), {}), (e.ssgp_read, ("A",), {})]                         # no fit
    calls += [(e.ssgp_fit, (X, y, 0.5), dict(features=D)) for D in (0, 64, 192, 2176)]
    calls += [(e.ssgp_fit, a, dict(features=128)) for a in ((X[:, :3], y, 0.5), (X[:0], y[:0], 0.5), big + (0.5,))]
    for k, (fn, a, kw) in enumerate(calls + [(e.ssgp_fit, (X, y, 0.5), dict(features=128))]):
        e.gp_set_precision(32 if k == len(calls) else 64)                                    # the last: not fp64
        with pytest.raises(UthotError, match="UT_EINVAL"):
            fn(*a, **kw)
    e.gp_set_precision(64)
    fit(e, c)
    for m in (0, cand.shape[1] + 1):                                                         # m < 1, ld < m
        with pytest.raises(UthotError, match="UT_EINVAL"):
            e.ssgp_score(cand, m=m)
    ptr, ld, out = ctypes.c_void_p(cand.data_ptr()), cand.stride(0), np.empty(128 * 128).ctypes.data_as(ctypes.c_void_p)
    L = e.lib
    assert [L.ut_ssgp_score(e.ctx, None, ld, 1, ctypes.byref(acq), None, None, None, None),
            L.ut_ssgp_score(e.ctx, ptr, ld, 1, None, None, None, None, None), L.ut_ssgp_read(e.ctx, -1, out, None),
            L.ut_ssgp_read(e.ctx, 7, out, None), L.ut_ssgp_read(e.ctx, 0, None, None),
            L.ut_ssgp_fit(e.ctx, None, y.ctypes.data, c["n"], z["d"], None, 128)] == [-1] * 6


def test_technique_rounds_request_distinct_configurations_and_refit():
    engine(CASES[0])                                            # (skips without a GPU)
    from uptune_amd import spaces, technique as Tq
    from uptune_amd.driver import SearchDriver
    manip = spaces.r64(4)                                       # Rosenbrock over [-1000, 1000]^4
    cost = lambda cfg: float(sum(100.0 * (cfg[i + 1] - cfg[i] ** 2) ** 2 + (1 - cfg[i]) ** 2 for i in range(3)))  # noqa: E731
    for root in (Tq.GpuDifferentialEvolution(surrogate="ssgp", ssgp_kw={"features": 128}, pool=2048, batch=4, seed=5),
                 Tq.bandit_a(bandit_seed=1, surrogate="ssgp", ssgp_kw={"features": 128}, pool=2048, batch=4, seed=5)):
        d = SearchDriver(manip, root, parallelism=4)
        d.main(cost, test_limit=24)
        req = [q.configuration.hash for q in d.requests_query()]          # every request, repeats included
        tech = d.root_technique
        model = (tech.techniques[0] if hasattr(tech, "techniques") else tech).model
        assert len(req) >= 24 and len(set(req)) == len(req)
        assert model.fits > 1 and model.engine.ssgp_read(None)["ok"]
