"""ut_ssgp_lml_grid's value without a GPU: the D x D form of tests/_ssgp_lml_oracle.py against the log density of
ys ~ N(0, Phi Phi^T + dg I_n) taken directly from the n x n Cholesky factor, and ssgp_kw's "lml" key.

rtol 1e-11: at dg = 1e-2 the two forms differed by 5e-14 .. 4e-13 relative over n = 100 .. 300, D = 128 / 384 (the
cancellation in |ys|^2 - |beta|^2 is divided by dg); the tolerance is twenty-five times the largest."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _lml_oracle as O  # noqa: E402
import _ssgp_lml_oracle as G  # noqa: E402
import _ssgp_oracle as S  # noqa: E402
from uptune_amd import technique as T  # noqa: E402


@pytest.mark.parametrize("n,D", [(100, 128), (300, 384)])
def test_the_woodbury_form_is_the_direct_log_density(n, D):
    X, y = O.data(n, 5)
    dg = 1e-2
    Z, b = S.draws(11, 5, D)
    Phi, ys = S.features(X, 1.1, Z, b, 1.0), S.ystd(y)[0]
    L = np.linalg.cholesky(Phi @ Phi.T + dg * np.eye(n))
    a = np.linalg.solve(L, ys)
    direct = -0.5 * (a @ a) - np.log(np.diag(L)).sum() - 0.5 * n * np.log(2.0 * np.pi)
    got = G.lml(Phi.T @ Phi + dg * np.eye(D), Phi.T @ ys, ys @ ys, n, dg)
    print("n %d D %d: direct %.15g, D x D form %.15g, relative %.2e" % (n, D, direct, got, abs(got / direct - 1)))
    assert abs(got - direct) <= 1e-11 * abs(direct)


def test_ssgp_kw_lml_is_gp_or_own():
    for v in ("gp", "own"):
        assert T.SharedModel(surrogate="ssgp", lengthscale="auto", ssgp_kw={"lml": v}).ssgp_kw == {"lml": v}
    for v in ("ssgp", None, 1):
        with pytest.raises(ValueError, match="ssgp_kw lml"):
            T.SharedModel(surrogate="ssgp", ssgp_kw={"lml": v})
