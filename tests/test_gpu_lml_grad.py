"""The LML gradient on the device (csrc/gp_lml_grad.hip, ut_gp_lml_grad) against
the analytic fp64 gradient of tests/_lml_grad_oracle.py, and
SharedModel(lengthscale="ard") over a real engine.

Errors are |device - oracle| / S, S the sum of the component's absolute terms
(the components cancel to 2e-9 .. 2e-3 of S, so g itself is no yardstick).
The oracle was checked against long double (test_lml_grad_oracle_cpu.py): ell
and sf2 to 6e-16, sn2 to 9e-14 at sigma_n2 = 1e-2 and to 8e-10 at 1e-6.  One
wrong element of M moves a component by about S / n^2 >= 1e-5 S at these n.
Bounds: 1e-9 at sigma_n2 = 1e-2; 1e-7 at 1e-6 (K^-1 carries cond(K) ~ 1e8
roundings there, in the oracle as on the device).

Measured on an MI355X (max over the shapes, precision 64 and 8 alike):
  sigma_n2 = 1e-2:  ell 4.8e-16, sf2 1.4e-17, sn2 1.4e-13
  sigma_n2 = 1e-6:  ell 1.5e-15, sf2 1.3e-17, sn2 5.0e-9   (the (128, 1) shape; 1.3e-9 elsewhere)"""
import ctypes
import gc
import os
import sys
import types

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _lml_grad_oracle as G  # noqa: E402
import _lml_oracle as O  # noqa: E402
from _spaces import to_manip  # noqa: E402
from oracle.space import BOOL, ENUM, FLOAT, Param  # noqa: E402

pytestmark = pytest.mark.gpu

# one padded block; no padding and d = 1; d not a multiple of 16; npad = 384 (three row
# tiles: the triangle's k-range start matters)
SHAPES = [(100, 5), (128, 1), (200, 37), (321, 3)]
TIERS = [(1e-2, 1e-9), (1e-6, 1e-7)]       # (sigma_n2, bound on |err| / S)
MIXED = [Param("a", FLOAT, 0.0, 1.0), Param("e1", ENUM, options=["p", "q", "r"]), Param("b", BOOL),
         Param("c", FLOAT, 0.0, 1.0), Param("e2", ENUM, options=["u", "v"])]

_ENGINES = {}


def engine(d, fresh=False, space=None):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from uptune_amd.engine import BatchEngine
    if fresh:
        return BatchEngine(to_manip(space or [Param(f"u{k}", FLOAT, 0.0, 1.0) for k in range(d)]), device=0, seed=0)
    if d not in _ENGINES:
        _ENGINES[d] = engine(d, fresh=True)
    _ENGINES[d].gp_set_precision(64)
    return _ENGINES[d]


@pytest.fixture(scope="module")
def want():
    """the oracle's gradient, computed once per (n, d, seed, lengthscale, noise)"""
    cache = {}

    def get(n, d, sn2, seed=0, ell=None, rows=None):
        key = (n, d, sn2, seed, None if ell is None else float(ell), rows)
        if key not in cache:
            X, y = O.data(n, d, seed=seed)
            r = slice(None) if rows is None else slice(0, rows)
            cache[key] = G.grad(X[r], y[r], O.ard_base(d) if ell is None else ell, sigma_n2=sn2)
        return cache[key]
    return get


def close(got, ref, bound, what):
    e = G.errors(got, ref)
    print(f"{what}: |err| / S  ell {e[0]:.3e}  sf2 {e[1]:.3e}  sn2 {e[2]:.3e}  (bound {bound:g})")
    assert max(e) <= bound, what


def bits(g):
    return np.concatenate([g[0], [g[1], g[2]]]).view(np.int64)


@pytest.mark.parametrize("sn2,bound", TIERS)
@pytest.mark.parametrize("prec", [64, 8])
@pytest.mark.parametrize("n,d", SHAPES)
def test_gradient_of_the_fit(n, d, prec, sn2, bound, want):
    X, y = O.data(n, d)
    ell = O.ard_base(d)
    e = engine(d)
    e.gp_set_precision(prec)
    e.gp_fit(X, y, lengthscale=ell, sigma_n2=sn2)
    got = e.gp_lml_grad()
    close(got, want(n, d, sn2), bound, f"sync fit n={n} d={d} prec={prec} sn2={sn2:g}")
    # two calls: the same bits
    assert np.array_equal(bits(got), bits(e.gp_lml_grad()))
    # a fit in flight (staged, never flushed by another call) is waited for
    X2, y2 = O.data(n, d, seed=1)
    e.gp_fit(X2, y2, lengthscale=ell, sigma_n2=sn2, wait=False)
    close(e.gp_lml_grad(), want(n, d, sn2, seed=1), bound, f"async fit n={n} d={d} prec={prec} sn2={sn2:g}")


@pytest.mark.parametrize("sn2,bound", TIERS)
@pytest.mark.parametrize("prec", [64, 8])
def test_gradient_after_append(prec, sn2, bound, want):
    d = 5
    X, y = O.data(140, d)
    e = engine(d)
    e.gp_set_precision(prec)
    e.gp_fit(X[:130], y[:130], lengthscale=1.5, sigma_n2=sn2)
    close(e.gp_lml_grad(), want(140, d, sn2, ell=1.5, rows=130), bound, f"before the append prec={prec}")
    e.gp_fit(X, y, lengthscale=1.5, sigma_n2=sn2)
    assert e.gp_last_fit_kind() == "append"
    close(e.gp_lml_grad(), want(140, d, sn2, ell=1.5), bound, f"append prec={prec} sn2={sn2:g}")


def test_scalar_outputs_may_be_null(want):
    n, d = 100, 5
    X, y = O.data(n, d)
    e = engine(d)
    e.gp_fit(X, y, lengthscale=O.ard_base(d), sigma_n2=1e-2)
    full = e.gp_lml_grad()
    g = np.empty(d)
    assert e.lib.ut_gp_lml_grad(e.ctx, d, g.ctypes.data, None, None) == 0
    assert np.array_equal(g.view(np.int64), full[0].view(np.int64))


def test_gradient_leaves_the_fit_alone():
    import torch
    n, d = 200, 37
    X, y = O.data(n, d)
    engine(d)
    U = torch.from_numpy(np.random.default_rng(5).uniform(size=(d, 512))).to("cuda:0")
    hyp = dict(lengthscale=2.0, sigma_n2=1e-6, jitter=1e-8)

    def score(e):
        return [t.cpu().numpy() for t in e.gp_score(U)]

    for prec in (64, 8):
        e = engine(d)
        e.gp_set_precision(prec)
        e.gp_fit(X, y, **hyp)
        before = score(e)
        e.gp_lml_grad()
        for a, b in zip(before, score(e)):
            assert np.array_equal(a, b)
    # a staged asynchronous fit fits what it was given: scoring after the
    # gradient call is that of an engine that was never asked for a gradient
    e = engine(d)
    e.gp_fit(X, y, **hyp)
    X3, y3 = O.data(n, d, seed=3)
    e.gp_fit(X3, y3, wait=False, **hyp)
    g3 = e.gp_lml_grad()
    got = score(e)
    ref = engine(d, fresh=True)
    ref.gp_fit(X, y, **hyp)
    ref.gp_fit(X3, y3, **hyp)
    want_s = score(ref)
    assert np.array_equal(bits(g3), bits(ref.gp_lml_grad()))
    ref.close()
    for a, b in zip(got, want_s):
        assert np.array_equal(a, b)


def mixed_rows(eng, n, seed):
    rng = np.random.default_rng(seed)
    cfgs = [{"a": float(rng.uniform()), "e1": "pqr"[rng.integers(3)], "b": bool(rng.integers(2)),
             "c": float(rng.uniform()), "e2": "uv"[rng.integers(2)]} for _ in range(n)]
    X = eng.features_host(cfgs)
    y = np.array([np.sin(3.0 * c["a"]) + (0.5 if c["e1"] == "q" else 0.0) + 0.3 * c["b"] for c in cfgs])
    return cfgs, X, y + 0.01 * rng.standard_normal(n)


def test_categorical_and_dense_kstar_give_the_same_gradient(monkeypatch):
    ell = np.array([0.7, 1.3, 1.3, 1.3, 1.3, 0.9, 1.3, 1.3])   # one value over the one-hot columns
    e = engine(8, fresh=True, space=MIXED)
    _, X, y = mixed_rows(e, 150, 3)
    ref = G.grad(X, y, ell, sigma_n2=1e-2)
    e.gp_fit(X, y, lengthscale=ell, sigma_n2=1e-2)
    assert e.gp_kstar_mode() == "categorical"
    close(e.gp_lml_grad(), ref, 1e-9, "categorical K*")
    e.close()
    monkeypatch.setenv("UT_CAT_KSTAR", "0")
    e2 = engine(8, fresh=True, space=MIXED)
    monkeypatch.delenv("UT_CAT_KSTAR")
    e2.gp_fit(X, y, lengthscale=ell, sigma_n2=1e-2)
    assert e2.gp_kstar_mode() == "dense"
    close(e2.gp_lml_grad(), ref, 1e-9, "dense K*")
    e2.close()


def test_errors_and_allocation_failure(want):
    from uptune_amd import _lib as L
    n, d = 100, 5
    X, y = O.data(n, d)
    g = np.empty(d + 1)
    sf, sn = ctypes.c_double(), ctypes.c_double()
    e = engine(d, fresh=True)
    with pytest.raises(L.UthotError, match="UT_ENOTPD"):
        e.gp_fit(X, y, lengthscale=1.0, sigma_n2=-2.0, jitter=0.0)
    assert e.lib.ut_gp_lml_grad(e.ctx, d, g.ctypes.data, ctypes.byref(sf), ctypes.byref(sn)) == -5   # UT_ENOTPD
    with pytest.raises(L.UthotError, match="UT_ENOTPD"):
        e.gp_lml_grad()
    e.gp_fit(X, y, lengthscale=O.ard_base(d), sigma_n2=1e-2)
    for bad_d in (d + 1, d - 1, 0):
        assert e.lib.ut_gp_lml_grad(e.ctx, bad_d, g.ctypes.data, ctypes.byref(sf), ctypes.byref(sn)) == -1   # UT_EINVAL
    assert e.lib.ut_gp_lml_grad(e.ctx, d, None, ctypes.byref(sf), ctypes.byref(sn)) == -1
    L.check(e.ctx, e.lib.ut_debug_fail_alloc(e.ctx, 1), "ut_debug_fail_alloc")
    with pytest.raises(L.UthotError, match="UT_ENOMEM"):
        e.gp_lml_grad()
    close(e.gp_lml_grad(), want(n, d, 1e-2), 1e-9, "after a failed allocation")
    e.close()


def test_close_returns_the_device_bytes():
    from uptune_amd import _lib as L
    lib = L.lib()

    def device_bytes():
        b = ctypes.c_int64(-1)
        assert lib.ut_device_bytes(0, ctypes.byref(b)) == 0
        return int(b.value)

    engine(5)      # the library and the device are up before the baseline is read
    gc.collect()
    base = device_bytes()
    e = engine(3, fresh=True)
    X, y = O.data(321, 3)
    e.gp_fit(X, y, lengthscale=1.0, sigma_n2=1e-2)
    fitted = device_bytes()
    e.gp_lml_grad()
    assert device_bytes() > fitted > base
    e.close()
    assert device_bytes() == base


# ---------------------------------------------------------------------------
# selection on the device
# ---------------------------------------------------------------------------
def rows_of(cfgs, y):
    return [types.SimpleNamespace(configuration=types.SimpleNamespace(data=c), time=float(t), state="OK", id=i)
            for i, (c, t) in enumerate(zip(cfgs, y))]


def test_shared_model_ard_on_the_device():
    from uptune_amd.technique import SharedModel
    rng = np.random.default_rng(7)
    X = rng.uniform(size=(80, 6))
    y = np.sin(3.0 * X[:, 0]) + (X[:, 1] - 0.3) ** 2 + 0.01 * rng.standard_normal(80)
    rows = rows_of([{f"u{k}": float(X[i, k]) for k in range(6)} for i in range(80)], y)
    drv = types.SimpleNamespace(results_query=lambda: rows)
    hyp = dict(sigma_n2=1e-4, jitter=0.0)
    auto = SharedModel(lengthscale="auto", **hyp)
    auto.engine = engine(6)
    assert auto.fit(drv)
    lml_auto = auto.engine.gp_lml()
    m = SharedModel(lengthscale="ard", **hyp)
    m.engine = engine(6)
    assert m.fit(drv)
    n, ell, val = m.ell_history[-1]
    print("ard on the device:", ell, "lml", val, "auto", auto.lengthscale_, lml_auto)
    assert n == 80 and ell is m.lengthscale_ and ell.shape == (6,)
    assert np.min(ell[2:]) > np.max(ell[:2])
    assert val > lml_auto
    # the fit that followed the selection is the selected point's
    assert abs(m.engine.gp_lml() - val) <= 1e-9 * abs(val)
    assert abs(val - O.lml(m._Xf[:80], m._yf[:80], ell, **m.hyper)) <= 1e-5 * abs(val)   # the project's fp64 tier


def test_shared_model_ard_keeps_the_categorical_kstar():
    from uptune_amd.technique import SharedModel
    e = engine(8, fresh=True, space=MIXED)
    cfgs, _, y = mixed_rows(e, 60, 11)
    m = SharedModel(lengthscale="ard", ard_maxiter=10, sigma_n2=1e-4)
    m.engine = e
    assert m.fit(types.SimpleNamespace(results_query=lambda: rows_of(cfgs, y)))
    ell = m.lengthscale_
    assert ell.shape == (8,) and len({float(v) for v in ell[[1, 2, 3, 4, 6, 7]]}) == 1
    assert e.gp_fit_ok() and e.gp_kstar_mode() == "categorical"
    assert len({float(v) for v in ell}) > 1       # the optimiser moved off the isotropic start
    e.close()
