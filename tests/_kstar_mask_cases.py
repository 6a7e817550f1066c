"""Test infrastructure: inputs with structured K* sparsity for the plane-occupancy
mask of k_gp_kstar_q (gp_kq.hip) and the masked variance contraction
k_gp_var_i8<true> (gp_i8.hip), and a numpy restatement of what the mask must be.
Shared by test_kstar_mask_cpu.py (the table checked on the CPU) and
test_gpu_kstar_mask.py.  The checker and never the product.

K* is stored as six balanced base-256 digits of rint(k* 2^(48 - eb)) under one
exponent eb = i8_kstar_exp(sf2), so with s0 = sf2 2^-eb in (0.245, 0.49] and
y = s0 exp(-|x' - u'|^2 / 2) an element has z leading zero digits for about
2^-(8z + 9) <= y < 2^-(8z + 1), and six zero digits below 2^-49.

Training rows: three tight clusters A, B, C (centres 20 apart on two axes, rows
a centre + 0.02 uniform noise), stored in cluster order with the boundaries on
multiples of 32 rows, so whole 32-row blocks (the variance contraction's k
stages) are far from a candidate.  n < 96 rows: cluster A alone.

Candidates: blocks of 32, one kind each, the kinds of PATTERN in turn:
  onA / onC   copies of training rows of A / C          mask 0x3f at that cluster
  z1 .. z5    at the distance from A's centre with y = 2^-(8z + 5) at the
              centre (random directions): z leading zero planes at A
  z2C         the same at C
  far         20 from every centre on a third axis      mask 0 everywhere
  lone        far, but candidate 7 of the block is a training row of A + 1e-3
  edge        around the distance from A's centre at which the exponent is
              -49 * 256 t units, where the last digit plane empties (+- 1 in the
              squared distance: about 185 t units either side)
PATTERN's strips of 128: [onA z1 z2 far] (four different masks), [z3 z4 z5
lone], [onA edge onC z2C] (live at A's and C's stages, dead at B's between
them), [far far far far] (no live stage), ...
"""
import math

import numpy as np

import _kstar_cases as KC

T_UNDER = -49.0 * 256.0          # exponents (t units) at or below it give six zero digits (sf2 2^-eb <= 0.49)
PATTERN = ("onA", "z1", "z2", "far", "z3", "z4", "z5", "lone", "onA", "edge", "onC", "z2C", "far", "far", "far", "far")
D_CLUSTER = 20.0
NOISE = 0.02


def _c(n, d, m, sf2, **kw):
    name = "n%d_d%d_m%d_sf%g" % (n, d, m, sf2)
    for k in sorted(kw):
        name += "_%s%s" % (k, "" if kw[k] is True else kw[k])
    return dict(dict(name=name, n=n, d=d, m=m, sf2=sf2, pre_m=0, fit_async=False), **kw)


# n -> npad, 64-row tiles RT, pairs P: 1 -> 128, 2, 1; 129 -> 256, 4, 2 (both tiles of a pair, the
# reversed order); 1000 -> 1024, 16, 8; 2000 -> 2048, 32, 16: I8_MASK_MAX_K, the masked kernel's limit
# (64 stages: lanes 32 .. 63 of the mask fetch, the high half of the live set, cluster C's stages
# 42 .. 62 behind B's dead ones); 2100 -> 2176, 34: past it the variance contraction keeps its
# unmasked kernel (K* writes the mask all the same).
# m -> 128-candidate strips CT: 1, 127 -> 1 (partial); 129 -> 2; 300 -> 3; 5000 -> 40 (several groups).
# d: 64 -> K32 2 (paired groups), 100 -> K32 4 (unpaired).
CASES = [
    _c(1, 64, 1, 1.0),
    _c(1, 100, 129, 1e-3),
    _c(129, 64, 127, 1.0),
    _c(129, 100, 300, 1e-3),
    _c(129, 64, 5000, 1.0),
    _c(129, 100, 5000, 1.0),
    _c(1000, 100, 1, 1.0),
    _c(1000, 100, 129, 1e-3),
    _c(1000, 64, 300, 1.0),
    _c(1000, 64, 5000, 1e-3),
    _c(2000, 64, 300, 1.0),
    _c(2000, 100, 129, 1e-3),
    _c(2100, 100, 127, 1e-3),
    _c(2100, 64, 300, 1.0),
    _c(129, 64, 127, 1.0, pre_m=5000),          # a small call after a large one: ldk (the mask's stride) shrinks
    _c(1000, 64, 300, 1.0, fit_async=True),     # scored right behind gp_fit(wait=False)
]


def ids():
    return [c["name"] for c in CASES]


def hyper(sf2):
    # (a large noise keeps the fit of near-identical rows positive definite)
    return dict(sigma_f2=sf2, sigma_n2=0.25 * sf2, jitter=0.0)


def segments(n):
    """-> (rA, rB): rows [0, rA) cluster A, [rA, rB) B, [rB, n) C; boundaries on multiples of 32"""
    nb = (n + 31) // 32
    if nb < 3:
        return n, n
    return 32 * ((nb + 2) // 3), 32 * ((2 * nb + 2) // 3)


def _centres(d):
    cA, cB, cC, cF = np.zeros(d), np.zeros(d), np.zeros(d), np.zeros(d)
    cB[0], cC[1], cF[2] = D_CLUSTER, D_CLUSTER, D_CLUSTER
    return cA, cB, cC, cF


def _radius(z, s0):
    """|u' - centre| with s0 exp(-r^2 / 2) = 2^-(8z + 5)"""
    return math.sqrt(2.0 * (math.log(s0) + (8 * z + 5) * math.log(2.0)))


_DATA = {}


def data(c):
    """-> dict X [n][d], y [n], U [m][d], ell [d] (ones), pre (the large call's candidates
    or None), kinds (per 32-candidate block); computed once, read-only"""
    if c["name"] not in _DATA:
        n, d, m, sf2 = c["n"], c["d"], c["m"], c["sf2"]
        rng = np.random.default_rng(7000 * n + 10 * d + m)
        cA, cB, cC, cF = _centres(d)
        rA, rB = segments(n)
        X = rng.uniform(size=(n, d)) * NOISE
        X[rA:rB] += cB
        X[rB:] += cC
        y = np.sum((X - 0.4) ** 2, axis=1) / 400.0 + 0.01 * rng.standard_normal(n)
        s0 = sf2 * 2.0 ** -KC.i8_kstar_exp(sf2)
        U = np.empty((m, d))
        kinds = []
        for b in range((m + 31) // 32):
            kind = PATTERN[b % len(PATTERN)]
            kinds.append(kind)
            j0, j1 = 32 * b, min(32 * b + 32, m)
            cnt = j1 - j0
            v = rng.standard_normal((cnt, d))
            v /= np.linalg.norm(v, axis=1)[:, None]
            if kind == "onA":
                blk = X[rng.integers(0, rA, size=cnt)]
            elif kind == "onC":
                blk = X[rng.integers(rB, n, size=cnt)] if rB < n else cC + v * 0.01
            elif kind == "far":
                blk = cF + v * 0.05
            elif kind == "lone":
                blk = cF + v * 0.05
                if cnt > 7:
                    blk[7] = X[0] + 1e-3
            elif kind == "edge":
                r2 = 2.0 * -T_UNDER / KC.T + rng.uniform(-1.0, 1.0, size=cnt)
                blk = cA + NOISE / 2 + v * np.sqrt(r2)[:, None]
            else:
                z = int(kind[1])
                blk = (cC if kind.endswith("C") else cA) + NOISE / 2 + v * _radius(z, s0)
            U[j0:j1] = blk
        pre = rng.uniform(size=(c["pre_m"], d)) * 0.5 if c["pre_m"] else None
        zz = dict(X=X, y=y, U=U, ell=np.ones(d), pre=pre, kinds=kinds)
        for a in zz.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _DATA[c["name"]] = zz
    return _DATA[c["name"]]


# --------------------------------------------------------------------------- the restatement
_REST = {}


def restate(c):
    """k_gp_kstar_q's arithmetic in numpy (as _kstar_cases.restate_q, which this is checked
    against) -> (t [n][m], the clamped exponent in t units; k [n][m], the stored k*)"""
    if c["name"] not in _REST:
        z = data(c)
        X, U, ell, sf2 = z["X"], z["U"], z["ell"], c["sf2"]
        o = KC.operands(X, U, ell)
        K = 32 * KC.k32_of(X.shape[1])
        ea, eb = o["ea"], o["eb"]
        Af = [a.astype(np.float64) for a in KC.digits(o["XT"], ea)]
        Bf = [b.astype(np.float64).T for b in KC.digits(o["Us"], eb[:, None])]
        acc = []
        for g in range(6):
            s = np.zeros((X.shape[0], U.shape[0]))
            for p in range(g + 1):
                s += Af[p] @ Bf[g - p]
            acc.append(s)
        if K <= KC.PAIR_MAX_K:
            u23, u45, u67 = acc[0] * 256.0 + acc[1], acc[2] * 256.0 + acc[3], acc[4] * 256.0 + acc[5]
            v = (u67 * 2.0 ** -16 + u45) * 2.0 ** -16 + u23
            sc = np.ldexp(1.0, ea + eb - 24)
        else:
            v = acc[5]
            for g in range(4, -1, -1):
                v = v * 2.0 ** -8 + acc[g]
            sc = np.ldexp(1.0, ea + eb - 16)
        hx, hc = (-0.5 * KC.T) * o["xn"], (-0.5 * KC.T) * o["cn"]
        t = np.maximum(np.minimum((v * sc[None, :] + hx[:, None]) + hc[None, :], 0.0), KC.T_MIN)
        ebk = KC.i8_kstar_exp(sf2)
        k = np.ldexp(np.rint(np.ldexp(KC.exp2t(t, sf2, 2.0 ** -ebk), 48)), ebk - 48)
        _REST[c["name"]] = (t, k)
    return _REST[c["name"]]


def mask_of(k, sf2):
    """the plane-occupancy mask of stored k* values k [rows][cols] (both multiples of 32):
    uint8 [rows / 32][cols / 32], bit p set iff digit plane p (0 = most significant) of the
    32 x 32 block holds a non-zero digit"""
    ebk = KC.i8_kstar_exp(sf2)
    dg = KC.digits(np.asarray(k, dtype=np.float64), ebk)
    R, Cc = k.shape[0] // 32, k.shape[1] // 32
    out = np.zeros((R, Cc), dtype=np.uint8)
    for p in range(6):
        nz = (dg[p] != 0).reshape(R, 32, Cc, 32).any(axis=(1, 3))
        out |= (nz.astype(np.uint8) << p)
    return out


def expected_mask(c):
    """the mask the restated planes give, padded with zeros to [npad / 32][ldk / 32]"""
    t, k = restate(c)
    npad, ldk = KC.npad_of(c["n"]), KC.ldk_of(c["m"])
    kp = np.zeros((npad, ldk))
    kp[:c["n"], :c["m"]] = k
    return mask_of(kp, c["sf2"])


def leading_zero_planes(mk):
    """of a non-zero mask byte"""
    return (int(mk) & -int(mk)).bit_length() - 1
