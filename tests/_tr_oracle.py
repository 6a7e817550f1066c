"""Numpy restatement of ut_propose_tr (the rule is stated in include/uthot.h),
built from the oracle's Philox draws, unit-value arithmetic and permutation
operators.  Test infrastructure: imported by tests only."""
import numpy as np

from oracle import perm as pm
from oracle import philox as ph
from oracle.space import BOOL, ENUM, PERM, columns, get_unit_value_vec, set_unit_value_vec, width

OP_TR = 6   # ut_core.h: the next op code after OP_GGA
assert OP_TR == ph.OP_GGA + 1


def box_faces(prm, c, h):
    """(uc, lo, hi) of a primitive parameter whose centre value is c"""
    uc = float(get_unit_value_vec(prm, np.array([c], dtype=np.float64))[0])
    return uc, max(uc - float(h), 0.0), min(uc + float(h), 1.0)


def propose_tr_vec(space, centre, half, prob, cat_prob, seed, round_, cand_base, m, must=1, with_selected=False):
    """-> (values [ncols][m], invalid [m] bool, u_pre [P][m]: the unit value before
    set_unit_value of each selected primitive, NaN elsewhere); with_selected adds
    the selection mask [P][m] as a fourth entry"""
    P = len(space)
    starts, _ = columns(space)
    centre = np.asarray(centre, dtype=np.float64)
    g = np.arange(cand_base, cand_base + m, dtype=np.uint64)
    out = np.repeat(centre[:, None], m, axis=1)
    u_pre = np.full((P, m), np.nan)
    picked = np.zeros((P, m), dtype=bool)
    sel = np.zeros(m, dtype=np.float64)
    for p, prm in enumerate(space):
        c0 = starts[p]
        ax, ay, az, _ = ph.draw(seed, g, p, round_, OP_TR)
        forced = (float(P - p) * ph.u01(ax, ay)) < (float(must) - sel)
        sel = sel + forced
        rate = az.astype(np.float64) * (1.0 / 4294967296.0) < (prob if prm.is_primitive() else cat_prob)
        pick = forced | rate
        picked[p] = pick
        if not pick.any():
            continue
        sb = p | (1 << ph.STREAM_SUB_SHIFT)
        gi = g[pick]
        if prm.kind == PERM:
            S = width(prm)
            for j in np.nonzero(pick)[0]:
                cur = [int(a) for a in centre[c0:c0 + S]]
                pm.small_random_change(cur, pm.Words(seed, g[j], sb, round_, OP_TR))
                out[c0:c0 + S, j] = cur
            continue
        c = centre[c0]
        if prm.is_primitive():
            bx, by, _, _ = ph.draw(seed, gi, sb, round_, OP_TR)
            _, lo, hi = box_faces(prm, c, half[p])
            u = lo + (hi - lo) * ph.u01(bx, by)
            u_pre[p, pick] = u
            out[c0, pick] = set_unit_value_vec(prm, u, np.full(u.shape, c)) + 0.0
        elif prm.kind == BOOL:
            out[c0, pick] = 1.0 - c
        elif prm.kind == ENUM:
            n = len(prm.options)
            if n > 1:
                _, _, bz, bw = ph.draw(seed, gi, sb, round_, OP_TR)
                r = ph.below64(ph.u64(bz, bw), n - 1).astype(np.int64)
                r = r + (r >= int(c))
                out[c0, pick] = r.astype(np.float64)
    invalid = ~np.any(out.view(np.uint64) != centre.view(np.uint64)[:, None], axis=0)
    return (out, invalid, u_pre, picked) if with_selected else (out, invalid, u_pre)
