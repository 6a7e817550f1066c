"""Numpy restatement of ut_propose_cma (the rule is stated in include/uthot.h),
built from the oracle's Philox draws, its normal draw, its unit-value arithmetic
and its permutation operators; BOOL / ENUM / PERM as tests/_tr_oracle.py treats
them.  x is accumulated in np.longdouble.  Test infrastructure: imported by tests only."""
import numpy as np

from oracle import perm as pm
from oracle import philox as ph
from oracle.mathx import normal_draw
from oracle.space import BOOL, ENUM, PERM, columns, set_unit_value_vec, width

OP_CMA = 10   # ut_core.h
SUB = 1 << ph.STREAM_SUB_SHIFT


def moving(space):
    return [p for p, prm in enumerate(space) if prm.is_primitive() and prm.lo < prm.hi]


def fold(x):
    """mirroring at 0 and 1, on |x| (the fold is even; every step is then exact)"""
    a = np.abs(x)
    t = a - 2.0 * np.floor(a / 2.0)
    return np.where(t > 1.0, 2.0 - t, t)


def propose_cma_vec(space, centre, mean, A, sigma, cat_prob, seed, round_, cand_base, m):
    """-> (values [ncols][m], invalid [m] bool, u [dn][m], bound [dn][m]: the rule's
    forward-error bound (dn + 4) 2^-53 (|mean_j| + sigma sum_k |A_jk| |z_k|) on u)"""
    starts, _ = columns(space)
    centre = np.asarray(centre, dtype=np.float64)
    mv = moving(space)
    dn = len(mv)
    A = np.asarray(A, dtype=np.float64).reshape(dn, dn)
    mean = np.asarray(mean, dtype=np.float64)
    g = np.arange(cand_base, cand_base + m, dtype=np.uint64)
    Z = np.stack([normal_draw(seed, g, k | SUB, round_, OP_CMA) for k in range(dn)])          # [dn][m]
    LD = np.longdouble
    x = mean.astype(LD)[:, None] + LD(sigma) * (A.astype(LD) @ Z.astype(LD))
    u = fold(x).astype(np.float64)
    bound = (dn + 4) * 2.0 ** -53 * (np.abs(mean)[:, None] + sigma * (np.abs(A) @ np.abs(Z)))
    out = np.repeat(centre[:, None], m, axis=1)
    for j, p in enumerate(mv):
        out[starts[p]] = set_unit_value_vec(space[p], u[j], np.full(m, centre[starts[p]])) + 0.0
    for p, prm in enumerate(space):
        if prm.is_primitive():
            continue
        c0 = starts[p]
        _, _, az, _ = ph.draw(seed, g, p, round_, OP_CMA)
        pick = az.astype(np.float64) * (1.0 / 4294967296.0) < cat_prob
        if not pick.any():
            continue
        if prm.kind == PERM:
            S = width(prm)
            for i in np.nonzero(pick)[0]:
                cur = [int(a) for a in centre[c0:c0 + S]]
                pm.small_random_change(cur, pm.Words(seed, g[i], p | SUB, round_, OP_CMA))
                out[c0:c0 + S, i] = cur
        elif prm.kind == BOOL:
            out[c0, pick] = 1.0 - centre[c0]
        elif prm.kind == ENUM and len(prm.options) > 1:
            _, _, bz, bw = ph.draw(seed, g[pick], p | SUB, round_, OP_CMA)
            r = ph.below64(ph.u64(bz, bw), len(prm.options) - 1).astype(np.int64)
            out[c0, pick] = (r + (r >= int(centre[c0]))).astype(np.float64)
    invalid = ~np.any(out.view(np.uint64) != centre.view(np.uint64)[:, None], axis=0)
    return out, invalid, u, bound
