"""ut_ssgp_lml_grid's rule (include/uthot.h) restated on tests/_ssgp_oracle.py: the long-double A_z, c_z of a grid
point with their elementwise bounds, and the LML formula in a chosen precision.  Nothing is measured on the device."""
import numpy as np

import _ssgp_oracle as S
import _ts_oracle as T

LD, U = S.LD, S.U

# S.features bounds tau's error by (d + 1) u (|us| |Zs|^T + |b|) for a device that sums the oracle's own us.  Here
# the oracle's rows are X * fl(1 / fl(ell * scale)) and the device's are fl(X * fl(1 / ell)), summed, times
# fl(1 / scale): against the exact X / (ell scale) the oracle's rows carry the roundings of (1) ell * scale, (2) its
# reciprocal, (3) the product with X; the device's those of (4) 1 / ell, (5) the product with X, (6) 1 / scale,
# (7) the product of the sum with it.  Seven more relative roundings, to first order: (d + 1) u -> (d + 8) u.
C_EXTRA = 7


def gram(X, y, ell, scale, Z, b, sf2, dg, cols=None):
    """S.gram at the lengthscales ell * scale, the phase term of its bounds widened by C_EXTRA roundings"""
    d = Z.shape[1]
    ez = np.broadcast_to(np.asarray(ell, dtype=np.float64), (d,)) * scale
    A, c, eA, ec = S.gram(X, y, ez, Z, b, sf2, dg, cols)
    amp = float(np.sqrt(2.0 * sf2 / Z.shape[0]))
    us = np.abs(np.asarray(X, dtype=np.float64) * (1.0 / ez)[None, :])
    de = amp * 2.0 * np.pi * C_EXTRA * U * (us @ np.abs(Z * T.INV_2PI).T + np.abs(b)[None, :])     # [n][D], on e_phi
    P = np.abs(S.features(X, ez, Z, b, sf2))
    Y = np.abs(S.ystd(y)[0])
    ec = ec + 1.01 * (de.T @ Y)                       # (1 %: the cross terms with e and eys, second order)
    if cols is not None:
        de, P = de[:, cols], P[:, cols]
    return A, c, eA + 1.01 * (P.T @ de + de.T @ P), ec


def lml(A, c, ys2, n, dg, dtype=np.float64):
    """-(|ys|^2 - |beta|^2) / (2 dg) - sum log L_ii - ((n - D) / 2) log dg - (n / 2) log 2 pi, beta = L^-1 c"""
    A, c = np.asarray(A).astype(dtype), np.asarray(c).astype(dtype)
    D = len(c)
    L = T.chol(A) if dtype is LD else np.linalg.cholesky(A)
    beta = np.zeros(D, dtype=dtype)
    for i in range(D):
        beta[i] = (c[i] - L[i, :i] @ beta[:i]) / L[i, i]
    two_pi = 2 * T.LD_PI if dtype is LD else dtype(2.0 * np.pi)
    return (-(dtype(ys2) - beta @ beta) / (2 * dtype(dg)) - np.sum(np.log(np.diag(L)))
            - dtype(n - D) / 2 * np.log(dtype(dg)) - dtype(n) / 2 * np.log(two_pi))
