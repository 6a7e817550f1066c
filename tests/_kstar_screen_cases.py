"""Test infrastructure: a numpy restatement of the K* screen's certificate
(k_q_screen, gp_kq.hip) and borderline inputs for it.  Shared by
test_kstar_screen_cpu.py (the certificate checked on the CPU against the
restated digit planes) and test_gpu_kstar_screen.py.  The checker and never the
product.

The certificate.  k_gp_kstar_q forms an element's exponent in t units as
  t = s (U + 256 R) + hx_r + hc_c,  s = 2^(ea + eb_c - 24),  U = 256 T_2 + T_3,
  R = sum_{g=4..7} 2^(-8 (g - 2)) T_g  (in units of T_2),
with T_g the exact integer sums of the digit products a_p b_q, p + q = g.  T_2
and T_3 need the two top planes of each operand only (a_1 b_1; a_1 b_2 + a_2 b_1);
|a_p b_q| <= 2^14 and g - 1 pairs in group g give |R| <= K 2^14 (3 2^-16 +
4 2^-24 + 5 2^-32 + 6 2^-40) < 0.76 K, K = 32 ceil(dpad / 32).  So
  t <= t_up = s (U + 194.56 K) + hx_r + hc_c,
and the kernel stores six zero digits where rint(t) >> 8 <= -49, i.e. where
t < LINE = -12288.5 (sf2_exp2t_nonpos then returns y < 2^-49, whose 48-bit word
is 0).  A unit (64 training rows x 128 candidates, padding rows and columns at
-1e300) is certified when every element has t_up + slack < LINE, slack = 1 +
2^-40 (max_r |hx_r| + |hc_c| + 194.56 K s) for the fp64 roundings on both sides
(each below 2^-48 of that magnitude).

Effectiveness.  A unit whose largest extended-precision t (the difference form
in np.longdouble, live rows and columns only) is below LINE by more than the
certificate's own remainder bound BOUND = 194.56 K s plus 2 t units is
certified.  t_up exceeds the element's own t by s (194.56 K - 256 R): BOUND when
the true remainder R is 0, up to twice that in the worst case, so the rule is
not a theorem for every input; it holds where |256 R s| stays below what the 2
t units leave after the slack (1 + < 1e-3 at these scales), the kernel's own
contraction error against the extended-precision t (< 2^-46 K 2^(ea + eb),
_kstar_cases) and the operands' roundings.  The cases here are fixed and
seeded, and the rule is asserted on every one of them as stated.

Borderline cases (sweep): the training rows of 64-row tile k sit at c + a_k e on
one axis e (noise 1e-6), the candidates of strip j at c - r_j e (+ a small
perpendicular part), so every element of unit (k, j) has t = -T (r_j + a_k)^2 / 2
to within a fraction of a t unit, placed at LINE + off for a table of offsets off
on either side of the line.  The candidates lie across the origin from the rows
(a negative dot product: a scale too large then certifies wrongly) and near it
(small |u'|: a padding row taken as the data row 0 then fails to certify).
sf2 = 0.48: sf2 2^-eb = 0.48, so the first t whose word is not 0 is 16 t units
above the line.
"""
import numpy as np

import _kstar_cases as KC
import _kstar_mask_cases as MC

LINE = -12288.5
REM = 0.76 * 256.0
MUTANTS = ("no_remainder", "line_plus_256", "padding_live", "pair_scale")


def certificate(X, U, ell, n, m, mutant=None):
    """-> (cert [npad / 64][ldk / 128] bool, bound [ldk / 128]: the largest REM K s of the strip's live columns)"""
    assert mutant is None or mutant in MUTANTS
    d = X.shape[1]
    o = KC.operands(X, U, ell)
    K = 32 * KC.k32_of(d)
    npad, ldk = KC.npad_of(n), KC.ldk_of(m)
    ea, eb = o["ea"], o["eb"]
    A = [a.astype(np.float64) for a in KC.digits(o["XT"], ea)[:2]]
    B = [b.astype(np.float64) for b in KC.digits(o["Us"], eb[:, None])[:2]]
    Uv = 256.0 * (A[0] @ B[0].T) + (A[0] @ B[1].T + A[1] @ B[0].T)
    pair = K <= KC.PAIR_MAX_K
    s = np.ldexp(1.0, ea + eb - (24 if pair or mutant != "pair_scale" else 16))
    hx = (-0.5 * KC.T) * o["xn"]
    hc = (-0.5 * KC.T) * o["cn"]
    rem = 0.0 if mutant == "no_remainder" else REM * K
    line = LINE + (256.0 if mutant == "line_plus_256" else 0.0)
    rmx = float(np.max(np.abs(hx)))
    tu = np.full((npad, ldk), 0.0 if mutant == "padding_live" else -1e300)
    tu[:n, :m] = Uv * s[None, :] + hx[:, None]
    off = np.full(ldk, -1e300)
    off[:m] = (rem * s + hc) + (1.0 + 2.0 ** -40 * ((rmx + np.abs(hc)) + rem * s))
    if mutant == "padding_live":
        off[m:] = off[:m].max() if m else 0.0
    tu = tu + off[None, :]
    cert = tu.reshape(npad // 64, 64, ldk // 128, 128).max(axis=(1, 3)) < line
    w = np.zeros(ldk)
    w[:m] = REM * K * s
    return cert, w.reshape(ldk // 128, 128).max(axis=1)


def t_ext_unit_max(X, U, ell, n, m):
    """the largest extended-precision exponent (t units) of each unit's live elements; -inf where it has none"""
    ld = np.longdouble
    npad, ldk = KC.npad_of(n), KC.ldk_of(m)
    t = np.full((npad, ldk), -np.inf)
    Xl, Ul, el = X.astype(ld), U.astype(ld), np.asarray(ell).astype(ld)
    for r in range(n):
        q = (Xl[r][None, :] - Ul) / el[None, :]
        t[r, :m] = (-(ld(KC.T) / 2) * np.sum(q * q, axis=1)).astype(np.float64)
    return t.reshape(npad // 64, 64, ldk // 128, 128).max(axis=(1, 3))


def must_certify(X, U, ell, n, m):
    """the effectiveness rule: units below LINE by more than the certificate's remainder bound plus 2 t units"""
    _, w = certificate(X, U, ell, n, m)
    return t_ext_unit_max(X, U, ell, n, m) < (LINE - w - 2.0)[None, :]


def zero_units(k, n, m):
    """stored k* [n][m] -> [npad / 64][ldk / 128] bool: every element of the unit is 0"""
    npad, ldk = KC.npad_of(n), KC.ldk_of(m)
    kp = np.zeros((npad, ldk))
    kp[:n, :m] = k
    return ~(kp != 0).reshape(npad // 64, 64, ldk // 128, 128).any(axis=(1, 3))


# --------------------------------------------------------------------------- the borderline cases
SF2 = 0.48


def _s(name, n, d, m, centre, tile_off, strip_off, single=False):
    return dict(name=name, n=n, d=d, m=m, sf2=SF2, centre=centre, tile_off=tile_off, strip_off=strip_off,
                single=single, pre_m=0, fit_async=False)


# tile_off / strip_off: offsets in t units from the line of the row tiles and the strips; unit (k, j)
# sits at about LINE + tile_off[k] + strip_off[j].  centre: |c| (the operands' scale: s = 1 at 4, 2^10 at 128)
SWEEP = [
    _s("d8_c4_fine", 129, 8, 384, 4.0, (0.0, 3.0, -7.0), (-60.0, -1.0, 40.0)),
    _s("d8_c4_wide", 129, 8, 300, 4.0, (0.0, 30.0, -90.0), (-400.0, 60.0, 200.0)),
    _s("d8_c4_n1000", 1000, 8, 129, 4.0, tuple(12.0 * k - 90.0 for k in range(16)), (-20.0, 5.0)),
    _s("d64_c4", 129, 64, 384, 4.0, (0.0, 5.0, -300.0), (-250.0, -2.0, 120.0)),
    _s("d97_c4", 129, 97, 384, 4.0, (0.0, 4.0, -500.0), (-700.0, -150.0, 100.0)),
    _s("d97_c4_n1000", 1000, 97, 300, 4.0, tuple(40.0 * k - 600.0 for k in range(16)), (-300.0, 0.0, 300.0)),
    _s("d8_c128_single_a", 129, 8, 384, 128.0, (-1e5, -1e5, 0.0), (30.0, 60.0, 90.0), single=True),
    _s("d8_c128_single_b", 129, 8, 384, 128.0, (-1e5, -1e5, 0.0), (120.0, 150.0, 180.0), single=True),
    _s("d8_c128_single_c", 129, 8, 384, 128.0, (-1e5, -1e5, 0.0), (210.0, 240.0, 270.0), single=True),
]


def ids():
    return [c["name"] for c in SWEEP]


_DATA = {}


def data(c):
    """-> dict X [n][d], y [n], U [m][d], ell [d] (ones); computed once, read-only"""
    if c["name"] not in _DATA:
        n, d, m = c["n"], c["d"], c["m"]
        rng = np.random.default_rng(9000 * n + 10 * d + m + int(c["centre"]))
        e = np.zeros(d)
        e[0] = 1.0
        cen = c["centre"] * e
        r_line = np.sqrt(2.0 * -LINE / KC.T)
        # t = -T r^2 / 2 -> r at LINE + off: r = sqrt(2 (-LINE - off) / T); the tile's share is linear in its offset
        X = np.empty((n, d))
        for r in range(n):
            k = min(r // 64, len(c["tile_off"]) - 1)
            a = -c["tile_off"][k] / (KC.T * r_line)
            X[r] = cen + a * e + 1e-6 * rng.uniform(-1.0, 1.0, size=d)
        U = np.empty((m, d))
        for j0 in range(0, m, 128):
            off = c["strip_off"][min(j0 // 128, len(c["strip_off"]) - 1)]
            rj = np.sqrt(2.0 * (-LINE - off) / KC.T)
            cnt = min(128, m - j0)
            g = rng.standard_normal((cnt, d)) * (0.0 if c["single"] else 0.02)
            g[:, 0] = 0.0
            # the perpendicular part lengthens the distance by |g|^2 / (2 r): keep the radius exact
            par = np.sqrt(np.maximum(rj * rj - np.sum(g * g, axis=1), 0.0))
            U[j0:j0 + cnt] = cen - par[:, None] * e[None, :] + g
        y = np.sum((X - 0.4) ** 2, axis=1) / 400.0 + 0.01 * rng.standard_normal(n)
        z = dict(X=X, y=y, U=U, ell=np.ones(d))
        for a in z.values():
            a.setflags(write=False)
        _DATA[c["name"]] = z
    return _DATA[c["name"]]


_K = {}


def stored(c):
    """the stored k* [n][m] of a sweep case (_kstar_cases.restate_q) or a mask-table case (its restate)"""
    if c["name"] not in _K:
        if "centre" in c:
            z = data(c)
            _K[c["name"]] = KC.restate_q(z["X"], z["U"], z["ell"], c["sf2"])
        else:
            _K[c["name"]] = MC.restate(c)[1]
    return _K[c["name"]]


def inputs(c):
    return data(c) if "centre" in c else MC.data(c)


def all_cases():
    return list(MC.CASES) + list(SWEEP)
