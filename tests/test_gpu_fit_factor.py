"""The fit's operands held to extended precision, element by element: every
case and append chain of tests/_fit_cases.py is fitted on the device, L, L^-1,
(L^-1)^T, beta, alpha and ys are read back (ut_gp_fit_read) and

  chol, inv, white   rho_dev <= 4 max(rho of the LAPACK route, rho of the numpy
                     restatement of gp_fit.hip) -- both fp64, measured by the same
                     functions on the same inputs -- and <= the cap n + d + 8
  beta, alpha, ys    within their derived bounds (<= 1); ut_gp_stats agrees
  bitwise            L^-1 exactly zero above the diagonal, padded rows and
                     columns exact identity rows, (L^-1)^T the transpose,
                     the f32 copy np.float32 of it
  precision 8        the stale flag after a refit (nothing copied, nothing
                     computed by the read), clear after an append or an fp64
                     recompute; the digit planes decode to rint(X_rk 2^(48 - ea_r))
                     exactly, zero past the diagonal and past n, so |dx| <=
                     2^(ea_r - 49) as I8_C assumes; rs, e2, E and Emu

under the refit's switches (UT_CHOL_FUSE, UT_CHOL_MERGED, UT_TRINV_BIG) where
the table says.  The measures, the yardstick and the derivations: _fit_cases.py.
The worst element's (i, j), its 64-block, rho_dev and both rho_ref are printed
and reported on failure."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

import _ard_cases as A  # noqa: E402
import _fit_cases as F  # noqa: E402
import _kstar_cases as KC  # noqa: E402
from _spaces import to_manip  # noqa: E402

LD = np.longdouble
ENV = ("UT_CHOL_FUSE", "UT_CHOL_MERGED", "UT_TRINV_BIG")
CHAIN_CASES = [F.chain_case(*ch) for ch in F.CHAINS]
REFITS = [(c, env) for env, ns in F.SWITCHES for c in F.CASES if ns is None or c["n"] in ns]


def _rid(c, env):
    return c["name"] + "".join("_%s%s" % (k[3:].lower(), v) for k, v in env.items())


def _engine(space, monkeypatch, env=None, prec=64):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in (env or {}).items():
        monkeypatch.setenv(k, v)           # (read when the context is created)
    from uptune_amd.engine import BatchEngine
    e = BatchEngine(to_manip(space), device=0, seed=0)
    e.gp_set_precision(prec)
    return e


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")


def _hyper(c):
    return dict(sigma_f2=c["sf2"], sigma_n2=c["sn2"], jitter=c["jitter"])


def _read(e, names=("L", "LINV", "LINVT", "ALPHA", "BETA", "YS")):
    out = {}
    for w in names:
        t, info = e.gp_fit_read(w)
        out[w] = None if t is None else t.cpu().numpy()
        out["info"] = info
    return out


def _exact(c, r):
    """the bitwise properties of one read-out"""
    n, npad = c["n"], F.npad_of(c["n"])
    X, L = r["LINV"], r["L"]
    assert X.shape == L.shape == (npad, npad)
    up = np.argwhere(np.triu(X, 1) != 0.0)
    assert up.size == 0, "%s: L^-1 not zero above the diagonal at %s ..." % (c["name"], up[:4].tolist())
    assert not np.triu(L, 1).any()
    eye = np.eye(npad)
    for nm, Mx in (("L^-1", X), ("L", L)):
        assert np.array_equal(Mx[n:], eye[n:]) and np.array_equal(Mx[:, n:], eye[:, n:]), \
            "%s: padded rows / columns of %s are not identity rows" % (c["name"], nm)
    assert not r["YS"][n:].any() and not r["BETA"][n:].any()
    if r["LINVT"] is not None:
        assert np.array_equal(r["LINVT"], X.T), "%s: (L^-1)^T is not the transpose of L^-1" % c["name"]
        assert not r["ALPHA"][n:].any()


def _held(c, z, r, stats):
    """the measures of one read-out against the lines of _fit_cases.py"""
    n = c["n"]
    ref, l_rows = F.references(c, z)
    assert r["info"]["l_rows"] == l_rows
    fit = dict(L=r["L"], X=r["LINV"])
    for m in F.measures_of(c):
        rho, (i, j) = F.measure(m, fit, z, n, l_rows if m == "chol" else None)
        ra, rb = ref[m]
        ln = F.line(c, ra, rb)
        msg = ("%s %s: rho_dev %.3g at %s, rho of the LAPACK route %.3g, of the restatement %.3g, line %.3g, cap %d"
               % (c["name"], m, rho, F.blk(i, j), ra, rb, ln, F.cap(c)))
        print(msg)
        assert rho <= ln and rho <= F.cap(c), msg
    rho, i = F.m_ys(r["YS"], z, n)
    print("%s ys: %.3g of its bound at row %d" % (c["name"], rho, i))
    assert rho <= 1.0, "%s: ys is %.3g of its bound at row %d" % (c["name"], rho, i)
    rho, i = F.m_beta(r["BETA"], r["LINV"], r["YS"], n)
    print("%s beta: %.3g of its bound at row %d" % (c["name"], rho, i))
    assert rho <= 1.0, "%s: beta is %.3g of its bound at row %d (64-block %d)" % (c["name"], rho, i, i // 64)
    if r["ALPHA"] is not None:
        rho, i = F.m_alpha(r["ALPHA"], r["LINV"], r["BETA"], n)
        print("%s alpha: %.3g of its bound at row %d" % (c["name"], rho, i))
        assert rho <= 1.0, "%s: alpha is %.3g of its bound at row %d (64-block %d)" % (c["name"], rho, i, i // 64)
    f_best, mean, sd = stats
    dm, ds = F.stats_bounds(z["y"], z["sd"])
    assert f_best == np.min(r["YS"][:n])
    assert abs(LD(mean) - z["mean"]) <= dm and abs(LD(sd) - z["sd"]) <= ds, (mean, sd)


def _i8_held(c, r, e):
    """precision 8: the digit planes, row scales and error sums against L^-1 and beta as read"""
    n, npad = c["n"], F.npad_of(c["n"])
    Nd = e.gp_fit_read("I8A")[0].cpu().numpy()
    rsv = e.gp_fit_read("I8RS")[0].cpu().numpy()
    assert Nd.shape == (npad, npad) and rsv.shape == (2 * npad + 2,)
    rs, e2, E, Emu = rsv[:npad], rsv[npad:2 * npad], rsv[2 * npad], rsv[2 * npad + 1]
    X = r["LINV"]
    ea, rs_w, N, e2_w = F.i8_expected(X, n, KC.i8_kstar_exp(c["sf2"]))
    assert np.array_equal(rs, rs_w), "%s: row scales differ at rows %s ..." % (
        c["name"], np.flatnonzero(rs != rs_w)[:4].tolist())
    bad = np.argwhere(Nd != N)
    assert bad.size == 0, "%s: decoded digits are not rint(X 2^(48 - ea)) at %s ..." % (c["name"], bad[:4].tolist())
    assert not np.triu(Nd, 1).any() and not Nd[n:].any()
    low = np.tril(np.ones((npad, npad), dtype=bool)) & (np.arange(npad) < n)[:, None]
    dx = np.abs(np.where(low, X, 0.0) - np.ldexp(Nd, (ea - 48)[:, None]))
    assert np.all(dx <= np.ldexp(1.0, ea - 49)[:, None])
    assert np.all(np.abs(e2 - e2_w) <= 2.0 * np.spacing(e2_w))
    E_w = np.sqrt(np.sum(e2.astype(LD)))
    Emu_w = np.sum(np.sqrt(e2.astype(LD)) * np.abs(r["BETA"].astype(LD)))
    slack = LD(1) + LD(2.0 ** -30)
    assert E_w <= LD(E) <= E_w * slack and Emu_w <= LD(Emu) <= Emu_w * slack, (E, float(E_w), Emu, float(Emu_w))
    assert e.gp_i8_bounds() == (E, Emu)


@pytest.mark.parametrize("c,env", REFITS, ids=[_rid(c, env) for c, env in REFITS])
def test_refit_operands(monkeypatch, c, env):
    z = F.data(c)
    e = _engine(z["space"], monkeypatch, env)
    e.gp_fit(z["X"], z["y"], lengthscale=z["ell"], **_hyper(c))
    r = _read(e)
    stats, kind, mode = e.gp_stats(), e.gp_last_fit_kind(), e.gp_kstar_mode()
    e.close()
    assert kind == "refit" and mode == ("categorical" if c["cat"] else "dense")
    assert r["info"] == dict(n=c["n"], npad=F.npad_of(c["n"]), precision=64, l_rows=F.npad_of(c["n"]), stale=0)
    _exact(c, r)
    _held(c, z, r, stats)


@pytest.mark.parametrize("prec", [64, 8])
@pytest.mark.parametrize("c", CHAIN_CASES, ids=[c["name"] for c in CHAIN_CASES])
def test_append_chain_operands(monkeypatch, c, prec):
    z = F.data(c)
    e = _engine(z["space"], monkeypatch, prec=prec)
    n = c["n0"]
    e.gp_fit(z["X"][:n], z["y"][:n], lengthscale=z["ell"], **_hyper(c))
    assert e.gp_last_fit_kind() == "refit"
    info = e.gp_fit_read("LINVT")[1]
    assert info["stale"] == (1 if prec == 8 else 0) and info["l_rows"] == info["npad"]
    for s in c["steps"]:
        n += s
        e.gp_fit(z["X"][:n], z["y"][:n], lengthscale=z["ell"], **_hyper(c))   # (precision 8: gp_ensure_linvt first)
        assert e.gp_last_fit_kind() == "append", (n, s)
    r = _read(e)
    stats = e.gp_stats()
    assert r["info"] == dict(n=c["n"], npad=F.npad_of(c["n"]), precision=prec, l_rows=F.CHAIN_L_ROWS[c["n0"]], stale=0)
    _exact(c, r)
    _held(c, z, r, stats)
    if prec == 8:
        _i8_held(c, r, e)
    e.close()


I8_REFITS = [c for c in F.CASES if c["n"] in (1, 65, 129, 300) and not c["cat"]]


@pytest.mark.parametrize("c", I8_REFITS, ids=[c["name"] for c in I8_REFITS])
def test_precision8_refit_planes_and_stale_transpose(monkeypatch, c):
    z = F.data(c)
    n, npad = c["n"], F.npad_of(c["n"])
    e = _engine(z["space"], monkeypatch, prec=8)
    e.gp_fit(z["X"], z["y"], lengthscale=z["ell"], **_hyper(c))
    r = _read(e)
    assert r["info"] == dict(n=n, npad=npad, precision=8, l_rows=npad, stale=1)
    assert r["LINVT"] is None and r["ALPHA"] is None
    assert e.gp_fit_read("ALPHA")[1]["stale"] == 1, "reading while stale computed the transpose"
    _exact(c, r)
    _i8_held(c, r, e)
    # an fp64 recompute is the transpose's first reader
    e.gp_set_i8_tol(0.0)
    e.gp_score(dev(np.random.default_rng(n).uniform(size=(c["d"], 64))))
    r2 = _read(e)
    assert r2["info"]["stale"] == 0 and np.array_equal(r2["LINV"], r["LINV"]) and np.array_equal(r2["BETA"], r["BETA"])
    _exact(c, r2)
    rho, i = F.m_alpha(r2["ALPHA"], r2["LINV"], r2["BETA"], n)
    assert rho <= 1.0, (rho, i)
    _i8_held(c, r2, e)
    e.close()


def test_precision32_transpose_copy(monkeypatch):
    """the f32 operand is np.float32 of (L^-1)^T, after a refit and after an append"""
    c = CHAIN_CASES[0]
    z = F.data(c)
    e = _engine(z["space"], monkeypatch, prec=32)
    for n in (c["n0"], c["n"]):
        e.gp_fit(z["X"][:n], z["y"][:n], lengthscale=z["ell"], **_hyper(c))
        f, info = e.gp_fit_read("LINVT_F32")
        X = e.gp_fit_read("LINV")[0].cpu().numpy()
        assert info["precision"] == 32 and info["stale"] == 0
        assert np.array_equal(f.cpu().numpy(), X.T.astype(np.float32).astype(np.float64))
    assert e.gp_last_fit_kind() == "append"
    e.close()


def test_fit_read_refusals(monkeypatch):
    """UT_EINVAL with no fit, the not-positive-definite error after a failed one,
    UT_EUNSUPPORTED for the f16x3 planes and for an operand of another precision"""
    from uptune_amd._lib import UthotError
    e = _engine(A.float_space(3), monkeypatch)
    rng = np.random.default_rng(3)
    X, y = rng.uniform(size=(40, 3)), rng.standard_normal(40)
    with pytest.raises(UthotError, match="no fit"):
        e.gp_fit_read("L")
    e.gp_fit(X, y, lengthscale=0.5)
    assert e.gp_fit_read("L")[0].shape == (128, 128) and e.gp_fit_read("YS")[0].shape == (128,)
    for w in ("H3", "LINVT_F32", "I8A", "I8RS"):
        with pytest.raises(UthotError, match="UT_EUNSUPPORTED|not read out|not a precision"):
            e.gp_fit_read(w)
    e.gp_fit(X, y, lengthscale=0.5, sigma_n2=-2.0, jitter=0.0, wait=False)     # not positive definite
    for _ in range(2):
        with pytest.raises(UthotError, match="not positive definite"):
            e.gp_fit_read("LINV")
    e.gp_set_precision(8)
    e.gp_fit(X, y, lengthscale=0.5)
    assert e.gp_fit_read("I8RS")[0].shape == (258,)
    with pytest.raises(UthotError, match="UT_EUNSUPPORTED|not a precision-32"):
        e.gp_fit_read("LINVT_F32")
    e.gp_set_precision(16)
    e.gp_fit(X, y, lengthscale=0.5)
    assert e.gp_fit_read("LINV")[1]["precision"] == 16
    with pytest.raises(UthotError, match="UT_EUNSUPPORTED|not read out"):
        e.gp_fit_read("H3")
    e.close()
