"""ut_ssgp_lml_grid on the device (csrc/ssgp.hip) against tests/_ssgp_lml_oracle.py, which derives every bound
on A_z and c_z used here.

The LML values (D <= 384) are held to the long-double evaluation of the formula on the device's own A_z, c_z, within
four times the error numpy's fp64 evaluation of the same formula shows on the same case (test_gpu_fit_factor.py's
rule), floored at 64 u |lml|.  The device's error over numpy's, the largest per case as measured on an MI355X:
n = 1: 0.38; 129 x 5, D = 128: 6.32 (z = 6, lml = -1985: inside the floor) and 3.89 (z = 3, lml = -80.75);
100 x 5, D = 384: 2.59; 300 x 37: 2.42; mixed: 2.37.  The error sits in |ys|^2 - |beta|^2, which is divided by 2 dg
with both norms near n: summed in plain fp64 and with beta_kb taken by the product with inv(L_kk), z = 3 stood at
7.2; as one signed sum in two doubles (k_ssgp_lml_points) at 4.11; with beta_kb by forward substitution on L_kk
(k_lml_diag<true>) at 3.89.  At D = 2048 (two-step units, 32 panels) the values are held to numpy's fp64 at
rtol 1e-9, the project's figure for dg = 1e-2 (test_gpu_lml.py), and A on the columns 0:128 and 1920:2048."""
import ctypes
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _lml_oracle as O  # noqa: E402
import _ssgp_lml_oracle as G  # noqa: E402
import _ssgp_oracle as S  # noqa: E402
import _ts_oracle as T  # noqa: E402
from _spaces import to_manip  # noqa: E402

pytestmark = pytest.mark.gpu
LD, SEED, DG = S.LD, 11, 1e-2


def _c(n, d, D, g, space=None, ell="iso", cols=None, noisy=False):
    return dict(name="n%d_d%s_D%d_g%d" % (n, "mix" if space else d, D, g), n=n, d=d, D=D, g=g, m=1, space=space,
                ell=ell, cols=cols, scales=np.geomspace(0.1, 4.0, g), noises=DG * np.linspace(1, 2, g) if noisy else None)


# ys = 0 and n < D; a row past a step, n - D = 1; n < D on three feature tiles; three units, d no multiple of 16, ARD,
# a noise per point; one-hot columns; two-step units and 32 panels
CASES = [_c(1, 1, 128, 1), _c(129, 5, 128, 7), _c(100, 5, 384, 3), _c(300, 37, 384, 7, ell="ard", noisy=True),
         _c(300, 0, 384, 3, space="mixed"), _c(513, 5, 2048, 2, cols=np.r_[0:128, 1920:2048])]
IDS = [c["name"] for c in CASES]
_RUNS = {}


def engine(c, monkeypatch=None, env=None):
    import torch
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)           # (read when the context is created)
    from uptune_amd.engine import BatchEngine
    return BatchEngine(to_manip(T.data(c)["space"]), device=0, seed=SEED)


def grid(e, c, scales=None, noises=None, parts=True):
    z = T.data(c)
    return e.ssgp_lml_grid(z["X"], z["y"], z["ell"], c["scales"] if scales is None else scales,
                           c["noises"] if noises is None else noises, features=c["D"], sigma_n2=DG, parts=parts)


def run(c):
    """the device's (lml, best, A, c) and the reference values with their tolerances, once per case"""
    if c["name"] not in _RUNS:
        assert T.have_longdouble()
        z = T.data(c)
        lml, best, A, cv = grid(engine(c), c)
        dgs = np.full(c["g"], DG) if c["noises"] is None else c["noises"]
        ref, tol = np.empty(c["g"], dtype=LD), np.empty(c["g"])
        for k in range(c["g"]):
            f64 = G.lml(A[k], cv[k], S.ystd(z["y"])[0] @ S.ystd(z["y"])[0], c["n"], dgs[k])
            if c["D"] > 384:
                ref[k], tol[k] = f64, 1e-9 * abs(f64)
                continue
            ys = S.ystd(z["y"], LD)[0]
            ref[k] = G.lml(A[k], cv[k], ys @ ys, c["n"], dgs[k], LD)
            tol[k] = max(4.0 * abs(float(f64 - ref[k])), 64 * S.U * abs(float(ref[k])))
            print("%s z %d: device error / numpy's = %.3g" % (c["name"], k, abs(float(lml[k] - ref[k])) /
                                                           max(abs(float(f64 - ref[k])), 1e-300)))
        _RUNS[c["name"]] = dict(lml=lml, best=best, A=A, c=cv, dg=dgs, ref=ref, tol=tol)
    return _RUNS[c["name"]]


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_gram_and_right_hand_side_of_every_point(c):
    z, r = T.data(c), run(c)
    Z, b = S.draws(SEED, z["d"], c["D"])
    for k, s in enumerate(c["scales"]):
        A, cv, eA, ec = G.gram(z["X"], z["y"], z["ell"], s, Z, b, 1.0, r["dg"][k], c["cols"])
        Adev = r["A"][k] if c["cols"] is None else r["A"][k][np.ix_(c["cols"], c["cols"])]
        assert np.all(np.abs(Adev.astype(LD) - A) <= eA) and np.array_equal(r["A"][k], r["A"][k].T)
        assert np.all(np.abs(r["c"][k].astype(LD) - cv) <= ec)


@pytest.mark.parametrize("c", CASES, ids=IDS)
def test_lml_values_and_best(c):
    r = run(c)
    assert np.all(np.abs(r["lml"].astype(LD) - r["ref"]) <= r["tol"])
    if c["g"] > 1:   # the inputs separate the two best points by more than the values may be off
        top = np.sort(r["ref"].astype(np.float64))[-2:]
        assert top[1] - top[0] > 2.0 * r["tol"].max()
    assert r["best"] == O.argmax_finite(r["ref"].astype(np.float64))


def test_same_bits_however_the_work_is_cut(monkeypatch):
    """the batches of points, the units per workgroup, the row chunks (1 MiB of P holds two of the three units) and
    the grid a point is part of change launches and buffers, never a sum's order"""
    c = _c(300, 5, 384, 7, noisy=True)
    assert S.split(c["n"], c["D"]) == (1, 3)
    want = grid(engine(c), c)
    for env in ({"UT_LML_BATCH": "1"}, {"UT_SSGP_UNITS_PER_WG": "2"}, {"UT_SSGP_PHI_MIB": "1"}):
        got = grid(engine(c, monkeypatch, env), c)
        assert all(np.array_equal(a, b) for a, b in zip(got, want)), env
        for k in env:
            monkeypatch.delenv(k)
    one = grid(engine(c), c, scales=c["scales"][4:5], noises=c["noises"][4:5])
    assert all(np.array_equal(one[k][0], want[k][4]) for k in (0, 2, 3))


def test_isolation_failure_and_refusals():
    import torch
    from uptune_amd._lib import UthotError
    c = CASES[1]
    z, e = T.data(c), engine(c)
    X, y, cand = z["X"], z["y"], torch.from_numpy(np.array(z["cand"], order="C")).to("cuda:0")
    e.ssgp_fit(X, y, lengthscale=z["ell"], sigma_n2=DG, features=128)
    e.gp_fit(X, y, lengthscale=z["ell"], sigma_n2=DG)
    before = [t.cpu().numpy() for t in e.ssgp_score(cand) + tuple(e.gp_score_values(cand))]
    noises = np.full(7, DG)
    noises[2] = -2.0
    lml, best = grid(e, c, noises=noises, parts=False)
    clean = run(c)["lml"]
    assert np.isnan(lml[2]) and np.array_equal(np.delete(lml, 2), np.delete(clean, 2))
    assert best == O.argmax_finite(lml) and best != 2
    lml, best = grid(e, c, noises=np.full(7, -2.0), parts=False)
    assert np.isnan(lml).all() and best == -1
    after = [t.cpu().numpy() for t in e.ssgp_score(cand) + tuple(e.gp_score_values(cand))]
    assert all(np.array_equal(a, b) for a, b in zip(before, after))
    big = (np.zeros((65537, z["d"])), np.zeros(65537))
    calls = [((X, y, 0.5, [1.0]), dict(features=D)) for D in (0, 64, 192, 2176)]
    calls += [(a + (0.5, [1.0]), dict(features=128)) for a in ((X[:, :3], y), (X[:0], y[:0]), big)]
    calls += [((X, y, 0.5, s), dict(features=128)) for s in ([], [1.0, 0.0], [-1.0], [np.inf], [np.nan])]
    for k, (a, kw) in enumerate(calls + [((X, y, 0.5, [1.0]), dict(features=128))]):
        e.gp_set_precision(32 if k == len(calls) else 64)                                    # the last: not fp64
        with pytest.raises(UthotError, match="UT_EINVAL"):
            e.ssgp_lml_grid(*a, **kw)
    e.gp_set_precision(64)
    from uptune_amd import _lib as L
    ell, out, one = np.full(z["d"], 0.5), np.empty(1), np.ones(1)
    h = L.GpHyper(sigma_f2=1.0, sigma_n2=DG, jitter=0.0, lengthscale_host=ell.ctypes.data)
    bi, P = ctypes.c_int32(0), lambda a: a.ctypes.data
    ok = [P(X), P(y), ctypes.byref(h), P(one), P(out), ctypes.byref(bi)]
    for drop in range(len(ok)):   # a NULL X, y, hyper, scales, lml or best
        a = [None if k == drop else v for k, v in enumerate(ok)]
        assert e.lib.ut_ssgp_lml_grid(e.ctx, a[0], a[1], c["n"], z["d"], a[2], 128, 1, a[3], None, a[4], a[5], None,
                                      None) == -1, drop


def test_technique_selects_its_lengthscale_on_its_own_likelihood():
    engine(CASES[0])                                            # (skips without a GPU)
    from uptune_amd import spaces, technique as Tq
    from uptune_amd.driver import SearchDriver
    manip = spaces.r64(4)                                       # Rosenbrock over [-1000, 1000]^4
    cost = lambda cfg: float(sum(100.0 * (cfg[i + 1] - cfg[i] ** 2) ** 2 + (1 - cfg[i]) ** 2 for i in range(3)))  # noqa: E731
    root = Tq.GpuDifferentialEvolution(surrogate="ssgp", ssgp_kw={"features": 128, "lml": "own"}, lengthscale="auto",
                                       pool=2048, batch=4, seed=5)
    d = SearchDriver(manip, root, parallelism=4)
    d.main(cost, test_limit=24)
    req = [q.configuration.hash for q in d.requests_query()]
    model = d.root_technique.model
    assert len(req) >= 24 and len(set(req)) == len(req)
    assert model.ell_history and model.lengthscale_ in model._grid(4)
    assert model.fits > 1 and model.engine.ssgp_read(None)["ok"]
