"""Log marginal likelihood on the device (csrc/gp_lml.hip): ut_gp_lml of the
fit in place and ut_gp_lml_grid's batched factorisations, against the LML of
oracle/gp.py's own factor (the reference has no GP: SURVEY F2).

Tolerances.  The oracle's fp64 LML was checked against a long-double Cholesky
at these shapes: with sigma_n2 = 1e-2 it is good to 1.3e-13 relative, so those
cases hold the device to rtol 1e-9 (four orders above the reference's own
rounding, room for the MFMA's summation order; one wrong element moves the
LML by more than 1e-3); with sigma_n2 = 1e-6 the oracle itself is no better
than 8e-10, so those cases use the project's fp64 tier, rtol 1e-5."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _lml_oracle as O  # noqa: E402
from _spaces import to_manip  # noqa: E402
from oracle.space import FLOAT, Param  # noqa: E402

pytestmark = pytest.mark.gpu

SHAPES = [(100, 5), (200, 37), (321, 3)]   # one padded block; d not a multiple of 16; npad = 384
TIERS = [(1e-2, 1e-9), (1e-6, 1e-5)]       # (sigma_n2, rtol)
SCALES7 = np.geomspace(0.1, 4.0, 7)

_ENGINES = {}


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


def close(got, want, rtol, what):
    err = np.max(np.abs(np.asarray(got) - np.asarray(want)) / np.abs(np.asarray(want)))
    print(f"{what}: max relative error {err:.3e} (rtol {rtol:g})")
    np.testing.assert_allclose(got, want, rtol=rtol, atol=0.0, err_msg=what)


@pytest.mark.parametrize("sn2,rtol", TIERS)
@pytest.mark.parametrize("prec", [64, 8])
@pytest.mark.parametrize("n,d", SHAPES)
def test_lml_of_the_fit(n, d, prec, sn2, rtol):
    X, y = O.data(n, d)
    ell = O.ard_base(d)
    want = O.lml(X, y, ell, sigma_n2=sn2)
    e = engine(d)
    e.gp_set_precision(prec)
    e.gp_fit(X, y, lengthscale=ell, sigma_n2=sn2)
    close(e.gp_lml(), want, rtol, f"sync fit n={n} d={d} prec={prec}")
    # a fit in flight (staged, never flushed by another call) is waited for
    X2, y2 = O.data(n, d, seed=1)
    e.gp_fit(X2, y2, lengthscale=ell, sigma_n2=sn2, wait=False)
    close(e.gp_lml(), O.lml(X2, y2, ell, sigma_n2=sn2), rtol, f"async fit n={n} d={d} prec={prec}")


@pytest.mark.parametrize("sn2,rtol", TIERS)
@pytest.mark.parametrize("prec", [64, 8])
def test_lml_after_append(prec, sn2, rtol):
    d = 5
    X, y = O.data(140, d)
    e = engine(d)
    e.gp_set_precision(prec)
    e.gp_fit(X[:130], y[:130], lengthscale=1.5, sigma_n2=sn2)
    e.gp_fit(X, y, lengthscale=1.5, sigma_n2=sn2)
    assert e.gp_last_fit_kind() == "append"
    close(e.gp_lml(), O.lml(X, y, 1.5, sigma_n2=sn2), rtol, f"append prec={prec}")


def test_lml_of_a_failed_fit():
    from uptune_amd import _lib as L
    X, y = O.data(100, 5)
    e = engine(5, fresh=True)
    with pytest.raises(L.UthotError, match="UT_ENOTPD"):
        e.gp_fit(X, y, lengthscale=1.0, sigma_n2=-2.0, jitter=0.0)
    v = ctypes.c_double()
    assert e.lib.ut_gp_lml(e.ctx, ctypes.byref(v)) == -5   # UT_ENOTPD
    e.close()


@pytest.mark.parametrize("sn2,rtol", TIERS)
@pytest.mark.parametrize("per_point_noise", [False, True])
@pytest.mark.parametrize("g", [1, 7])
@pytest.mark.parametrize("n,d", SHAPES)
def test_grid_matches_oracle(n, d, g, per_point_noise, sn2, rtol):
    X, y = O.data(n, d)
    ell = O.ard_base(d)
    scales = SCALES7[2:3] if g == 1 else SCALES7
    noises = sn2 * np.linspace(1.0, 2.0, g) if per_point_noise else None
    want, want_best = O.lml_grid(X, y, ell, scales, noises, sigma_n2=sn2)
    assert np.isfinite(want).all()
    e = engine(d)
    got, best = e.gp_lml_grid(X, y, ell, scales, noises, sigma_n2=sn2)
    close(got, want, rtol, f"grid n={n} d={d} g={g}")
    # every point is also the LML of a fit at that point
    fits = []
    for j, s in enumerate(scales):
        e.gp_fit(X, y, lengthscale=s * ell, sigma_n2=sn2 if noises is None else noises[j])
        fits.append(e.gp_lml())
    close(got, fits, rtol, f"grid vs fit n={n} d={d} g={g}")
    # best index: only where the oracle's best and second best are far apart
    if g > 1:
        top = np.sort(want)[::-1]
        assert top[0] - top[1] > 1000.0 * rtol * abs(top[0]), "the grid does not separate its best point"
        assert best == want_best
    else:
        assert best == 0


def test_grid_chunks_give_the_same_bits(monkeypatch):
    n, d = 200, 37
    X, y = O.data(n, d)
    scales = np.geomspace(0.2, 3.0, 5)
    whole, b0 = engine(d).gp_lml_grid(X, y, O.ard_base(d), scales, sigma_n2=1e-2)
    monkeypatch.setenv("UT_LML_BATCH", "2")
    e2 = engine(d, fresh=True)   # chunks of 2, 2, 1
    monkeypatch.delenv("UT_LML_BATCH")
    parts, b1 = e2.gp_lml_grid(X, y, O.ard_base(d), scales, sigma_n2=1e-2)
    e2.close()
    assert np.isfinite(whole).all()
    assert np.array_equal(whole.view(np.int64), parts.view(np.int64)) and b0 == b1


def test_a_failed_point_poisons_nothing_else():
    n, d = 200, 37
    X, y = O.data(n, d)
    scales = np.geomspace(0.2, 3.0, 5)
    e = engine(d)
    good = np.full(5, 1e-2)
    clean, _ = e.gp_lml_grid(X, y, O.ard_base(d), scales, good, jitter=0.0)
    bad = good.copy()
    bad[2] = -2.0   # diagonal 1 - 2: the first pivot is negative
    got, best = e.gp_lml_grid(X, y, O.ard_base(d), scales, bad, jitter=0.0)
    assert np.isnan(got[2])
    keep = [0, 1, 3, 4]
    assert np.array_equal(got[keep].view(np.int64), clean[keep].view(np.int64))
    assert best == keep[int(np.argmax(clean[keep]))]
    got, best = e.gp_lml_grid(X, y, O.ard_base(d), scales, np.full(5, -2.0), jitter=0.0)
    assert np.isnan(got).all() and best == -1


def test_grid_leaves_the_fit_alone():
    n, d = 200, 37
    X, y = O.data(n, d)
    X2, y2 = O.data(100, d, seed=2)
    U = dev(np.random.default_rng(5).uniform(size=(d, 512)))
    hyp = dict(lengthscale=2.0, sigma_n2=1e-6, jitter=1e-8)

    def score(e):
        return [t.cpu().numpy() for t in e.gp_score(U)]

    e = engine(d)
    e.gp_fit(X, y, **hyp)
    before = score(e)
    e.gp_lml_grid(X2, y2, 1.0, SCALES7, sigma_n2=1e-2)
    after = score(e)
    for a, b in zip(before, after):
        assert np.array_equal(a, b)
    # a staged asynchronous fit stays staged, and fits what it was given
    X3, y3 = O.data(n, d, seed=3)
    e.gp_fit(X3, y3, wait=False, **hyp)
    e.gp_lml_grid(X2, y2, 1.0, SCALES7, sigma_n2=1e-2)
    got = score(e)
    ref = engine(d, fresh=True)
    ref.gp_fit(X, y, **hyp)
    ref.gp_fit(X3, y3, **hyp)
    want = score(ref)
    ref.close()
    for a, b in zip(got, want):
        assert np.array_equal(a, b)


def test_shared_model_auto_on_the_device():
    """SharedModel(lengthscale="auto") over a real engine: the default grid's
    argmax as the oracle has it, and the fit that follows uses it"""
    import types

    from uptune_amd.technique import SharedModel
    n, d = 60, 5
    X, y = O.data(n, d)
    rows = [types.SimpleNamespace(configuration=types.SimpleNamespace(data={f"u{k}": float(X[i, k]) for k in range(d)}),
                                  time=float(y[i]), state="OK", id=i) for i in range(n)]
    m = SharedModel(lengthscale="auto")
    m.engine = engine(d)
    assert m.fit(types.SimpleNamespace(results_query=lambda: rows))
    grid = np.sqrt(d) * np.geomspace(0.05, 4.0, 16)
    want, best = O.lml_grid(m._Xf[:n], m._yf[:n], 1.0, grid, **m.hyper)
    top = np.sort(want[np.isfinite(want)])[::-1]
    assert top[0] - top[1] > 1000.0 * 1e-5 * abs(top[0]), "the grid does not separate its best point"
    assert m.lengthscale_ == grid[best] and m.ell_history[0][:2] == (n, grid[best])
    close(m.ell_history[0][2], want[best], 1e-5, "auto: the selected point's LML")
    close(m.engine.gp_lml(), want[best], 1e-5, "auto: the LML of the fit that followed")


def test_grid_arguments_and_allocation_failure():
    from uptune_amd import _lib as L
    n, d = 100, 5
    X, y = O.data(n, d)
    e = engine(d, fresh=True)
    for scales in ([], [1.0, 0.0], [float("nan")], [float("inf")], [-1.0]):
        with pytest.raises(L.UthotError, match="UT_EINVAL"):
            e.gp_lml_grid(X, y, 1.0, scales)
    L.check(e.ctx, e.lib.ut_debug_fail_alloc(e.ctx, 1), "ut_debug_fail_alloc")
    with pytest.raises(L.UthotError, match="UT_ENOMEM"):
        e.gp_lml_grid(X, y, 1.0, SCALES7, sigma_n2=1e-2)
    got, best = e.gp_lml_grid(X, y, 1.0, SCALES7, sigma_n2=1e-2)
    want, want_best = O.lml_grid(X, y, 1.0, SCALES7, sigma_n2=1e-2)
    close(got, want, 1e-9, "after a failed allocation")
    assert best == want_best
    e.close()
