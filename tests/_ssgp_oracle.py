"""The sparse-spectrum GP's rule (include/uthot.h "sparse-spectrum GP") restated
in numpy, in fp64 or long double, and the error bounds its tests hold the device
to.  Draws: tests/_ts_oracle.py's Philox restatement with OP_SSGP and round 0.

Bounds: u = 2^-53, gamma_k = k u, each stated where it is computed; none is measured on the device."""
import numpy as np

import _ts_oracle as T

LD = T.LD
OP_SSGP = 11
U = 2.0 ** -53


def draws(seed, d, D):
    from oracle import philox as ph
    j = np.arange(D, dtype=np.uint64)
    Z = T.normal(seed, j[:, None], np.arange(d, dtype=np.uint64)[None, :], 0, op=OP_SSGP)
    x, y, _, _ = ph.draw(seed, j, ph.STREAM_CAND, 0, OP_SSGP)
    return Z, ph.u01(x, y)


def split(n, D):   # ssgp.hip's ssgp_split: (steps per unit, units)
    nsteps, Tn = (n + 127) // 128, D // 128
    want = max(1, 512 // (Tn * (Tn + 1) // 2))
    steps = -(-nsteps // min(nsteps, want))
    return steps, -(-nsteps // steps)


def features(Uf, ell, Z, b, sf2, dtype=np.float64):
    """Phi [m][D] of the unit features Uf [m][d]; with long double also its error bound e_phi [m][D]"""
    D, d = Z.shape
    us = np.asarray(Uf, dtype=np.float64) * (1.0 / np.broadcast_to(np.asarray(ell, dtype=np.float64), (d,)))[None, :]
    Zs = Z * T.INV_2PI                                         # fp64: rounded once per entry
    tau = us.astype(dtype) @ Zs.T.astype(dtype) + b.astype(dtype)[None, :]
    fr = tau - np.rint(tau)
    amp = np.sqrt(dtype(2) * dtype(sf2) / dtype(D))
    if dtype is not LD:
        return amp * T.cos2pi(fr)
    # tau is a (d + 1)-term sum; phi's error: cos2pi's stated one, the phase's, the roundings of amp and the product
    dtau = (d + 1) * U * (np.abs(us) @ np.abs(Zs).T + np.abs(b)[None, :])
    return amp * T.cos_true(fr), float(amp) * (T.COS_ERR + 2.0 * np.pi * dtau + 3.0 * U)


def ystd(y, dtype=np.float64):
    """-> ys, its error bound (n + 8) u (|y| + |mean|) / sd"""
    y = np.asarray(y, dtype=np.float64)
    ys = T.standardise(y, dtype)
    sd = float(np.std(y)) or 1.0
    return ys, (len(y) + 8) * U * (np.abs(y) + abs(float(np.mean(y)))) / sd


def gram(X, y, ell, Z, b, sf2, diag, cols=None):
    """long double A (its rows and columns `cols`; None = all), c and their elementwise bounds (fp64 arrays)"""
    n, D = X.shape[0], Z.shape[0]
    Phi, e = features(X, ell, Z, b, sf2, LD)
    ys, eys = ystd(y, LD)
    c = Phi.T @ ys
    P, Y = np.abs(Phi).astype(np.float64), np.abs(ys).astype(np.float64)
    # n-term dot products of columns carrying e, summed in units and then over units
    g = (n + split(n, D)[1] + 2) * U
    ec = e.T @ Y + P.T @ eys + e.T @ eys + g * (P.T @ Y)
    if cols is not None:
        Phi, e, P = Phi[:, cols], e[:, cols], P[:, cols]
    A = Phi.T @ Phi + LD(diag) * np.eye(Phi.shape[1], dtype=LD)
    eA = P.T @ e + e.T @ P + e.T @ e + g * (P.T @ P) + U * np.abs(A).astype(np.float64)
    return A, c, eA, ec


def weights(Linv, c):
    """long double w = Linv^T (Linv c) from a given Linv and c, and its bound: two D-term mat-vecs,
    dbeta = gamma_(D+8) |Linv| |c|, dw = |Linv|^T dbeta + gamma_(D+8) |Linv|^T |beta|"""
    D = len(c)
    beta = Linv.astype(LD) @ c.astype(LD)
    aL, g = np.abs(Linv), (D + 8) * U
    db = g * (aL @ np.abs(c))
    return Linv.T.astype(LD) @ beta, aL.T @ db + g * (aL.T @ np.abs(beta).astype(np.float64))


def posterior(Uf, ell, Z, b, sf2, diag, Linv, w):   # long double mu, var from a given Linv and w, and their bounds
    D = Z.shape[0]
    phi, e = features(Uf, ell, Z, b, sf2, LD)                  # [m][D]
    mu = phi @ w.astype(LD)
    V = phi @ Linv.T.astype(LD)                                # [m][D]: v_i per candidate
    var = LD(diag) * np.sum(V * V, axis=1)
    P, aV, aL = np.abs(phi).astype(np.float64), np.abs(V).astype(np.float64), np.abs(Linv)
    # mu: a D-term dot product; v = Linv phi row by row, then var = diag sum v^2
    emu = e @ np.abs(w) + (D + 8) * U * (P @ np.abs(w))
    dv = e @ aL.T + (D + 2) * U * (P @ aL.T)
    evar = diag * (np.sum(2.0 * aV * dv + dv * dv, axis=1) + (D + 8) * U * np.sum(aV * aV, axis=1))
    return mu, var, emu, evar


def model(X, y, ell, sf2, diag, D, seed):   # the whole rule in fp64
    Z, b = draws(seed, X.shape[1], D)
    Phi = features(X, ell, Z, b, sf2)
    ys, _ = ystd(y)
    A = Phi.T @ Phi + diag * np.eye(D)
    Linv = np.linalg.inv(np.linalg.cholesky(A))
    return dict(Z=Z, b=b, w=Linv.T @ (Linv @ (Phi.T @ ys)), Linv=Linv, f_best=float(np.min(ys)), ys=ys)
