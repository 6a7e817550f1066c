"""The refit chain against the chain it replaced, bit for bit.

UT_FIT_LEGACY=1 selects the previous chain: k_gp_prep_train (a thread per
row), k_gp_kmat over every tile, k_trinv_level / k_trinv_big alone and the
Cholesky fused from 2048 padded rows.  The default chain (k_gp_prep_rows, the
lower-triangle k_gp_kmat and k_trinv_small at every level in fits of up to 2048
padded rows, the Cholesky fused from 1024 padded rows) keeps every element's
operations and their order, so every operand read back by ut_gp_fit_read must
be equal in every bit:

  the factor         its lower triangle only: the lower-triangle k_gp_kmat no
                     longer writes gp_K's blocks above the diagonal, and
                     UT_FIT_L (k_fit_read_lower) hands back zeros there on
                     both chains
  L^-1               whole
  beta, ys           whole
  precision 8        the int8 digit planes (decoded, UT_FIT_I8A) and
                     [rs | e2 | E | Emu] (UT_FIT_I8RS)

at sizes at and around every block (64), padding (128), tile (32 / 64 / 128) and
level edge, with the ragged last pair (300 -> 384, 700 -> 768, 1100 -> 1152) and
the padded identity block.  Inputs: the recipe of _fit_cases.data (same seeds,
lengthscales of _fit_cases.ell_of) without its extended-precision reference,
which these tests do not need.

The enqueue order of the round (the proposal before the fit's head kernels) is
unchanged, so there is no test of it here."""
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
from _spaces import to_manip  # noqa: E402

ENV = ("UT_FIT_LEGACY", "UT_CHOL_FUSE", "UT_CHOL_MERGED", "UT_TRINV_BIG", "UT_TRINV_SMALL_WG")
NS = (1, 63, 64, 65, 127, 128, 129, 255, 257, 300, 700, 1024, 1100, 2048)
DS = (1, 3, 64)
HYPER = dict(sigma_f2=1.0, sigma_n2=1e-6, jitter=1e-8)
EVERY = "1000000"

_INPUTS = {}


def _inputs(n, d):
    """X [n][d], y [n], ell [d] as _fit_cases.data draws them; read-only, computed once.
    (The seed, X and y lines restate _fit_cases.data, which cannot be called here: it also
    builds the longdouble K_ext, minutes at n = 2048.  Change the two together.)"""
    if (n, d) not in _INPUTS:
        rng = np.random.default_rng(7000 + 10 * n + d)
        X = rng.uniform(size=(n, d))
        y = np.sum((X - 0.4) ** 2, axis=1) + 0.01 * rng.standard_normal(n)
        ell = F.ell_of(dict(d=d, ell="lo"))
        for a in (X, y, ell):
            a.setflags(write=False)
        _INPUTS[(n, d)] = (X, y, ell)
    return _INPUTS[(n, d)]


def _engine(d, monkeypatch, env, prec=64):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    for k in ENV:
        monkeypatch.delenv(k, raising=False)
    for k, v in env.items():
        monkeypatch.setenv(k, v)           # (read when the context is created)
    from uptune_amd.engine import BatchEngine
    e = BatchEngine(to_manip(A.float_space(d)), device=0, seed=0)
    e.gp_set_precision(prec)
    return e


def _fit_read(n, d, monkeypatch, env, prec):
    X, y, ell = _inputs(n, d)
    e = _engine(d, monkeypatch, env, prec)
    e.gp_fit(X, y, lengthscale=ell, **HYPER)
    names = ("L", "LINV", "BETA", "YS") + (("I8A", "I8RS") if prec == 8 else ())
    out = {w: e.gp_fit_read(w)[0].cpu().numpy() for w in names}
    info = e.gp_fit_read("LINV")[1]
    kind = e.gp_last_fit_kind()
    e.close()
    assert kind == "refit" and info["npad"] == F.npad_of(n) and info["l_rows"] == info["npad"]
    return out


def _bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def _same(tag, ref, got):
    for w in ref:
        bad = np.argwhere(_bits(ref[w]) != _bits(got[w]))
        assert bad.size == 0, "%s: %s differs in %d elements, first at %s" % (tag, w, len(bad), bad[0].tolist())


@pytest.mark.parametrize("prec", [64, 8])
@pytest.mark.parametrize("d", DS)
@pytest.mark.parametrize("n", NS)
def test_chain_bitwise_against_legacy(monkeypatch, n, d, prec):
    ref = _fit_read(n, d, monkeypatch, {"UT_FIT_LEGACY": "1"}, prec)
    got = _fit_read(n, d, monkeypatch, {}, prec)
    assert np.all(np.isfinite(ref["LINV"])) and ref["LINV"].any()
    _same("n=%d d=%d precision %d" % (n, d, prec), ref, got)


# every L^-1 tile at every level it can tile: k_trinv_small everywhere; k_trinv_level
# everywhere on the new chain; k_trinv_big from TRB_MIN = 256 rows with k_trinv_level
# below; the default choice -- against k_trinv_level everywhere on the legacy chain
TILES = [("small", {"UT_TRINV_SMALL_WG": EVERY}),
         ("level", {"UT_TRINV_SMALL_WG": "0", "UT_TRINV_BIG": "0"}),
         ("big", {"UT_TRINV_SMALL_WG": "0", "UT_TRINV_BIG": "1"}),
         ("default", {})]


@pytest.mark.parametrize("n", [1024, 2048])
def test_each_trinv_tile_bitwise(monkeypatch, n):
    d = 3
    ref = _fit_read(n, d, monkeypatch, {"UT_FIT_LEGACY": "1", "UT_TRINV_BIG": "0"}, 64)
    for name, env in TILES:
        _same("n=%d tiles %s" % (n, name), ref, _fit_read(n, d, monkeypatch, env, 64))


@pytest.mark.parametrize("n", [300, 1024])
@pytest.mark.parametrize("legacy", ["1", "0"])
def test_not_positive_definite_flag(monkeypatch, legacy, n):
    """a duplicated training row with sigma_n2 = 0 and jitter 0: the waited fit
    returns UT_ENOTPD, and the device flag -- one bit, set by atomicOr -- is set
    (ut_gp_fit_status reads it back; k_gp_finalize reads it on the device and
    scores NaN) -- on both chains; n = 300 factors its diagonal blocks in
    k_chol_diag on both, n = 1024 in k_chol_update_diag on the default chain
    (fused from 1024 padded rows) and in k_chol_diag on the legacy one"""
    from uptune_amd._lib import UthotError
    d = 3
    X, y, ell = _inputs(n, d)
    X = X.copy()
    X[n - 100] = X[7]
    e = _engine(d, monkeypatch, {"UT_FIT_LEGACY": legacy})
    with pytest.raises(UthotError, match="not positive definite"):
        e.gp_fit(X, y, lengthscale=ell, sigma_f2=1.0, sigma_n2=0.0, jitter=0.0)
    e.gp_fit(X, y, lengthscale=ell, sigma_f2=1.0, sigma_n2=0.0, jitter=0.0, wait=False)
    U = torch.from_numpy(np.random.default_rng(5).uniform(size=(d, 256))).to("cuda:0")
    _, _, score = e.gp_score(U)            # enqueued behind the failing fit
    assert torch.isnan(score).all()
    assert not e.gp_fit_ok()
    e.gp_fit(X[:200], y[:200], lengthscale=ell, **HYPER)
    assert e.gp_fit_ok()
    e.close()
