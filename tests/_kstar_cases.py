"""Test infrastructure: the case table, the extended-precision reference, the
derived per-element tolerance and a numpy restatement of the digit scheme for
K*, k*_rc = sf2 exp(-|x'_r - u'_c|^2 / 2) with x' = x / ell, u' = u / ell.
Shared by test_kstar_cases_cpu.py (the table checked on the CPU) and
test_gpu_kstar_elements.py (every K* kernel held to it element by element
through ut_gp_kstar_read).  The checker and never the product.

Reference (k_ref): the difference form sum_k ((x_k - u_k) / ell_k)^2, which has
no cancellation, in np.longdouble (>= 63 mantissa bits asserted; else the stdlib
decimal at 40 digits on a fixed sample), from the raw X, U, ell and sf2 alone.
Its own error is (d + 3) 2^-64 of the exponent and 2^-63 relative: 2^-11 of
the smallest term of the tolerance below.

Tolerance (tolerance()): derived here, once, from what the kernels state about
themselves, and computed per element from the inputs; nothing in it was fitted
to a device's output.  With u = 2^-53, T = 256 / ln 2 (KSTAR_T_SCALE), xs =
|x'_r|, us = |u'_c|, df = |x'_r - u'_c|, the device forms the exponent in
t units (2^(1/256)), t = C + hx + hc with C = sum_k (T x'_rk) u'_kc, hx = -T/2
|x'_r|^2, hc = -T/2 |u'_c|^2.  Its absolute error, first order:

  inputs       x' = fl(x fl(1/ell)), u' likewise: the common 1/ell's rounding
               scales a difference (2u |t|); the two products' roundings do
               not cancel: T u df (xs + us)
  operand      fl(T x'): u T xs us (Cauchy-Schwarz over k)
  contraction  k_gp_kstar_q: 2^-46 K 2^(ea + eb_c), its documented bound, K =
               32 ceil(dpad / 32), ea = q_exp(max |T x'|) over the fit, eb_c =
               q_exp(max_k |u'_kc|); q_exp(v) = ilogb(v / 0.49) + 1.
               (Each operand's digit rounding is 2^-49 of its scale, |a|, |b|
               <= 0.49: 0.98 2^-49 per k; the dropped pairs p + q >= 8 are at
               most 5 2^14 2^-64 + 4 2^14 2^-72 + ... < 2.52 2^-49 per k; so
               < 3.5 2^-49 K 2^(ea + eb_c) < 2^-46 K 2^(ea + eb_c) / 2: the
               documented bound holds with a factor 2 to spare.)
               the fp64-MFMA kernels: gamma_K T xs us, gamma_K = K u, K = dpad
  half-norms   d sequential fused-or-not multiply-adds and the product with
               -T/2: (d + 2) u T (xs^2 + us^2) / 2
  three-term   fl(fl(C + hx) + hc), and C's own conversion: u (2 T xs us +
               T xs^2 / 2) + u |t|
  T            the constant's own rounding: u |t|

divided by T this is the error of the natural exponent, so of k* relatively;
the exp adds its documented 2 ulp (2^-51 relative; sf2_exp2t_nonpos); storing
as six digits adds 2^-49 2^i8_kstar_exp(sf2) absolutely (both precision-8
kernels; nothing for fp64 rows); 2^-1074 covers the flush to zero past
KSTAR_T_MIN, where k_ref < 1e-434 sf2.  The sum is multiplied by SLACK = 2, the
one slack factor: the bound is first order (second-order terms in u), and the
exp's 2 ulp is documented as "about" (its table entry sf2 exp2(j / 256) and the
product with the polynomial each round once more).

Categorical K* (k_gp_kstar's int8 code stages): the match count M is an exact
integer, c0 + c1 M one fused multiply-add whose terms are the one-hot blocks'
share of T (xs^2 + us^2) / 2 and T xs us; the formula above over the whole
one-hot feature vector (its norms are the numeric ones plus that share) bounds
it, so the same function is used with the features' d.

Restatement (restate_q): k_gp_kstar_q's arithmetic in numpy -- balanced base-256
digits of rint(v 2^(48 - e)), exact integer group sums (float64 matmuls of
integers below 2^31), the paired (K <= 96) and unpaired recombination, the table
exp, the six-digit store -- with three mutants that test_kstar_cases_cpu.py
requires to exceed the tolerance on every case marked tight:
  drop67    groups T_6 and T_7 (the pair U_67) dropped
  uplanes   the candidates' two least significant planes (4 and 5) zeroed
  eb_off    column MUTANT_COL's scale 2^(ea + eb_c) taken with eb_c + 1
"""
import decimal
import math

import numpy as np

import _ard_cases as A
from oracle.space import BOOL, ENUM

T = 369.3299304675746            # KSTAR_T_SCALE = 256 / ln 2
T_MIN = -1000.0 * T              # KSTAR_T_MIN
U53 = 2.0 ** -53
SLACK = 2.0
EXP_TAB = 256
PAIR_MAX_K = 96                  # Q_PAIR_MAX_K
MUTANT_COL = 0                   # an ordinary column (a training row + 1e-3) in every case
MUTANTS = ("drop67", "uplanes", "eb_off")
KERNELS = ("q", "i8", "f64")     # k_gp_kstar_q, k_gp_kstar<int8_t>, k_gp_kstar<double>
SAMPLE = 4096                    # decimal fallback: elements per case


def q_exp(mx):
    """ilogb(mx / 0.49) + 1 for mx > 0, else 0 (gp_kq.hip q_exp, ut_internal.h i8_kstar_exp)"""
    return math.frexp(mx / 0.49)[1] if mx > 0.0 else 0


def npad_of(n):
    return (n + 127) // 128 * 128


def ldk_of(m):
    return (m + 255) // 256 * 256


def dpad_of(d):
    return (d + 3) // 4 * 4


def k32_of(d):
    return (dpad_of(d) + 31) // 32


# --------------------------------------------------------------------------- the cases
def sqrt_ish(d):
    """the power of two nearest sqrt(d): with it 2 sqrt(d)-ish is a power of two and
    x / ell exact, so the columns built on digit boundaries land on them"""
    return 2.0 ** math.floor(math.log2(math.sqrt(d)) + 0.5)


def _c(n, d, m, sf2, ell, **kw):
    name = "n%d_d%d_m%d_sf%g_%s" % (n, d, m, sf2, ell)
    for k in sorted(kw):
        name += "_%s%s" % (k, "" if kw[k] is True else kw[k])
    return dict(dict(name=name, n=n, d=d, m=m, sf2=sf2, ell=ell, pre_m=0, fit_async=False, tight=True), **kw)


# ell: "lo" = 0.2 sqrt(d)-ish, "hi" = 2 sqrt(d)-ish (a power of two), or a recipe of
# _ard_cases.ell_vector.  d -> dpad, K32: 3 -> 4, 1; 4 -> 4, 1; 32 -> 32, 1; 33 -> 36, 2;
# 64 -> 64, 2; 96 -> 96, 3 (the last paired); 97 -> 100, 4 (the first unpaired); 112 -> 112, 4.
# n -> npad, 64-row tiles: 1, 127, 128 -> 128, 2; 129 -> 256, 4; 300 -> 384, 6;
# 1000 -> 1024, 16; 8200 -> 8320, 130.  m -> ldk, 64-column tiles: 1 .. 256 -> 256, 4;
# 257 -> 512, 8; 2049 -> 2304, 36.
CASES = [
    _c(1, 3, 1, 1.0, "lo"),
    _c(127, 3, 63, 37.0, "hi"),
    _c(128, 32, 64, 1.0, "lo"),
    _c(129, 33, 65, 1e-3, "hi"),
    _c(128, 96, 1, 1.0, "hi"),
    _c(300, 64, 256, 1.0, "hi"),
    _c(300, 96, 257, 1.0, "lo"),
    _c(300, 97, 257, 37.0, "hi"),
    _c(1000, 112, 256, 1e-3, "lo"),
    _c(8200, 4, 64, 1.0, "lo"),
    _c(129, 64, 2049, 1.0, "lo"),
    _c(1000, 33, 65, 1.0, "one_short_first"),
    _c(300, 97, 64, 37.0, "one_short_last"),
    _c(127, 64, 63, 1.0, "hi", pre_m=2049),        # a large-m call first on the same context
    _c(1000, 64, 257, 1.0, "lo", fit_async=True),   # scored right behind gp_fit(wait=False)
]


def ids():
    return [c["name"] for c in CASES]


def ell_of(c):
    d = c["d"]
    if c["ell"] == "lo":
        return np.full(d, 0.2 * sqrt_ish(d))
    if c["ell"] == "hi":
        return np.full(d, 2.0 * sqrt_ish(d))
    return A.ell_vector(c["ell"], d, 1.5)


def _unscale(target, il):
    """u with fl(u il) == target where one exists within 8 ulps of target / il, else the nearest"""
    u0 = target / il
    best, cand = u0, u0
    for step in range(-8, 9):
        cand = u0
        for _ in range(abs(step)):
            cand = np.nextafter(cand, np.inf if step > 0 else -np.inf)
        if cand * il == target:
            return cand
        if abs(cand * il - target) < abs(best * il - target):
            best = cand
    return best


def _from_word(word):
    """the value in [-0.49, 0.49] whose biased 48-bit word (i8_biased) is `word`"""
    return (word - 0x808080808080) / 2.0 ** 48


def special_columns(X, ell, rng):
    """the columns the kernels can go wrong at, side by side in one 64-column tile
    (name, u [d]); the first is an ordinary one"""
    n, d = X.shape
    il = 1.0 / ell
    cols = [("near", X[0] + 1e-3), ("copy", X[min(1, n - 1)].copy()), ("zero", np.zeros(d)),
            ("copy_last", X[n - 1].copy())]
    base = rng.uniform(size=d)
    for e in (-30, 0, 10):
        cols.append(("scale2^%d" % e, base * 2.0 ** e))
    far = X[0].copy()
    far[0] += 60.0 * ell[0]       # |x' - u'|^2 / 2 >= 1800: past KSTAR_T_MIN, k* exactly 0
    cols.append(("far", far))
    # max |u'| = 0.49 2^j and its two neighbours: q_exp's boundary (feature k0 holds the max)
    k0 = d - 1
    for j in (0, -3, 5):
        mid = 0.49 * 2.0 ** j
        for nm, tgt in (("below", np.nextafter(mid, 0.0)), ("at", mid), ("above", np.nextafter(mid, np.inf))):
            u = rng.uniform(size=d) * 0.3 * mid * ell
            u[k0] = _unscale(tgt, il[k0])
            cols.append(("q_exp2^%d_%s" % (j, nm), u))
    # scaled 48-bit words with the byte 0x00, 0x7f, 0x80, 0xff in every position
    # below the top one (whose range |x| <= 0.49 limits: 0xc4 / 0x3c keep x 2^-eb in
    # (0.245, 0.49), so eb = 1 whatever the other features hold), and 0x7f / 0x80 in
    # every position at eb = 0
    u = np.empty(d)
    for k in range(d):
        b = (0x00, 0x7f, 0x80, 0xff)[k % 4]
        top = 0xc4 if (k // 4) % 2 == 0 else 0x3c
        word = (top << 40) | sum(b << (8 * i) for i in range(5))
        u[k] = _unscale(2.0 * _from_word(word), il[k])
    cols.append(("bytes", u))
    u = np.empty(d)
    for k in range(d):
        b = (0x7f, 0x80)[k % 2]
        u[k] = _unscale(_from_word(sum(b << (8 * i) for i in range(6))), il[k])
    u[0] = _unscale(_from_word(0xc4 << 40 | 0x7f7f7f7f7f), il[0])   # 0.2676 in (0.245, 0.49]: eb = 0
    cols.append(("bytes_all", u))
    return cols


_DATA = {}


def data(c):
    """-> dict X [n][d], y [n], U [m][d], ell [d], names (of the special columns), pre
    (the large call's candidates or None), k_ref [n][m] longdouble; computed once, read-only"""
    if c["name"] not in _DATA:
        n, d, m = c["n"], c["d"], c["m"]
        rng = np.random.default_rng(1000 * n + 10 * d + m)
        X = rng.uniform(size=(n, d))
        y = np.sum((X - 0.4) ** 2, axis=1) + 0.01 * rng.standard_normal(n)
        ell = ell_of(c)
        U = rng.uniform(size=(m, d))
        sp = special_columns(X, ell, rng)[:m]
        for j, (_, u) in enumerate(sp):
            U[j] = u
        # the large call first: other columns at other scales, so a stale plane, column
        # scale or norm past the new ldk or under the new columns would show
        pre = rng.uniform(size=(c["pre_m"], d)) * 2.0 ** 7 if c["pre_m"] else None
        z = dict(X=X, y=y, U=U, ell=ell, names=[s[0] for s in sp], pre=pre, k_ref=reference(X, U, ell, c["sf2"]))
        for a in z.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _DATA[c["name"]] = z
    return _DATA[c["name"]]


# --------------------------------------------------------------------------- the reference
def have_longdouble():
    return np.finfo(np.longdouble).nmant >= 63


def reference(X, U, ell, sf2, extra=None):
    """k_ref [n][m] from the raw inputs in the difference form; extra [n][m]: a further
    exact squared distance (the one-hot blocks').  np.longdouble, or -- below 63
    mantissa bits -- decimal on SAMPLE elements, NaN elsewhere."""
    n, m = X.shape[0], U.shape[0]
    if have_longdouble():
        ld = np.longdouble
        Xl, Ul, el = X.astype(ld), U.astype(ld), np.asarray(ell).astype(ld)
        out = np.empty((n, m), dtype=ld)
        for r in range(n):
            q = (Xl[r][None, :] - Ul) / el[None, :]
            s = np.sum(q * q, axis=1)
            if extra is not None:
                s = s + extra[r].astype(ld)
            out[r] = ld(sf2) * np.exp(-s / ld(2))
        return out
    out = np.full((n, m), np.nan, dtype=np.longdouble)
    rng = np.random.default_rng(7)
    cnt = min(n * m, SAMPLE)
    pick = rng.choice(n * m, size=cnt, replace=False)
    with decimal.localcontext() as ctx:
        ctx.prec = 40
        D = decimal.Decimal
        for e in pick:
            r, c = divmod(int(e), m)
            s = sum(((D(float(X[r, k])) - D(float(U[c, k]))) / D(float(ell[k]))) ** 2 for k in range(X.shape[1]))
            if extra is not None:
                s += D(float(extra[r, c]))
            v = D(float(sf2)) * (-s / 2).exp()
            out[r, c] = np.longdouble(str(v)) if v > D("1e-4000") else 0
    return out


# --------------------------------------------------------------------------- what the device holds
def operands(X, U, ell):
    """the device's own operands, as its kernels round them (k_gp_prep_train,
    k_gp_xs_t, k_gp_prep_cand): x', T x', u', the norms; ea and eb_c of gp_kq.hip"""
    il = 1.0 / np.asarray(ell, dtype=np.float64)
    Xs, Us = X * il, U * il
    XT = Xs * T
    ea = q_exp(float(np.max(np.abs(XT)))) if XT.size else 0
    eb = np.array([q_exp(float(v)) for v in np.max(np.abs(Us), axis=1)], dtype=np.int64)
    return dict(Xs=Xs, Us=Us, XT=XT, xn=np.sum(Xs * Xs, axis=1), cn=np.sum(Us * Us, axis=1), ea=ea, eb=eb)


def i8_kstar_exp(sf2):
    return q_exp(sf2)


# --------------------------------------------------------------------------- the tolerance
def tolerance(X, U, ell, sf2, kernel, k_ref):
    """[n][m] float64: the largest |k - k_ref| the kernel's stated contracts allow
    (the module docstring derives it); k_ref enters as the magnitude the relative
    terms refer to"""
    assert kernel in KERNELS
    o = operands(X, U, ell)
    d = X.shape[1]
    dpad = dpad_of(d)
    xs, us = np.sqrt(o["xn"])[:, None], np.sqrt(o["cn"])[None, :]
    # df from the difference form (float64 suffices for a tolerance)
    df2 = np.empty((X.shape[0], U.shape[0]))
    for r in range(X.shape[0]):
        q = o["Xs"][r][None, :] - o["Us"]
        df2[r] = np.sum(q * q, axis=1)
    df, tabs = np.sqrt(df2), 0.5 * T * df2
    e_in = T * U53 * df * (xs + us) + 2.0 * U53 * tabs
    e_op = U53 * T * xs * us
    if kernel == "q":
        K = 32 * ((dpad + 31) // 32)
        e_con = 2.0 ** -46 * K * np.ldexp(1.0, o["ea"] + o["eb"])[None, :] * np.ones_like(df)
    else:
        e_con = dpad * U53 * T * xs * us
    e_norm = (d + 2) * U53 * T * (xs * xs + us * us) / 2.0
    e_sum = U53 * (2.0 * T * xs * us + T * xs * xs / 2.0) + U53 * tabs
    e_T = U53 * tabs
    rel = (e_in + e_op + e_con + e_norm + e_sum + e_T) / T + 2.0 ** -51
    tol = rel * np.abs(k_ref).astype(np.float64) + 2.0 ** -1074
    if kernel != "f64":
        tol = tol + 2.0 ** (-49 + i8_kstar_exp(sf2))
    return SLACK * tol


# --------------------------------------------------------------------------- the digit scheme restated
def digits(v, e):
    """six balanced base-256 digits of rint(v 2^(48 - e)), plane 0 the most
    significant (i8_biased / i8_planes); e broadcasts against v"""
    N = np.rint(np.ldexp(v, 48 - np.asarray(e))).astype(np.int64)
    out = []
    for _ in range(6):
        dg = ((N + 128) & 255) - 128
        out.append(dg)
        N = (N - dg) >> 8
    assert not N.any(), "a scaled value outside the six digits' range"
    return out[::-1]


def exp2t(t, sf2, kscale=1.0):
    """sf2_exp2t_nonpos with its table (times kscale, a power of two)"""
    L = 0.6931471805599453 / 256.0
    C2, C3, C4 = L * L / 2.0, L * L * L / 6.0, L * L * L * L / 24.0
    etab = (sf2 * np.exp2(np.arange(EXP_TAB) / EXP_TAB)) * kscale
    kf = np.rint(t)
    f = t - kf
    p = (((C4 * f + C3) * f + C2) * f + L) * f + 1.0
    k = kf.astype(np.int64)
    with np.errstate(under="ignore"):
        return np.ldexp(p * etab[k & (EXP_TAB - 1)], (k >> 8).astype(np.int64))


def restate_q(X, U, ell, sf2, mutant=None):
    """k_gp_kstar_q on the CPU -> the stored k* [n][m] (float64: a 48-bit integer
    times 2^(eb - 48)); mutant: None or one of MUTANTS"""
    assert mutant is None or mutant in MUTANTS
    o = operands(X, U, ell)
    d = X.shape[1]
    K = 32 * k32_of(d)
    ea, eb = o["ea"], o["eb"]
    Ad = digits(o["XT"], ea)                       # [6] of [n][d] (the padded k are zero digits)
    Bd = digits(o["Us"], eb[:, None])              # [6] of [m][d]
    if mutant == "uplanes":
        Bd[4], Bd[5] = np.zeros_like(Bd[4]), np.zeros_like(Bd[5])
    Af = [a.astype(np.float64) for a in Ad]
    Bf = [b.astype(np.float64).T for b in Bd]
    acc = []
    for g in range(6):                             # T_(g + 2): plane pairs p + q = g
        s = np.zeros((X.shape[0], U.shape[0]))
        for p in range(g + 1):
            s += Af[p] @ Bf[g - p]
        assert np.max(np.abs(s), initial=0.0) < 2.0 ** 31
        acc.append(s)
    if mutant == "drop67":
        acc[4], acc[5] = np.zeros_like(acc[4]), np.zeros_like(acc[5])
    ebs = eb + (np.arange(len(eb)) == MUTANT_COL) if mutant == "eb_off" else eb
    if K <= PAIR_MAX_K:
        u23, u45, u67 = acc[0] * 256.0 + acc[1], acc[2] * 256.0 + acc[3], acc[4] * 256.0 + acc[5]
        assert max(np.max(np.abs(u), initial=0.0) for u in (u23, u45, u67)) < 2.0 ** 31
        v = (u67 * 2.0 ** -16 + u45) * 2.0 ** -16 + u23
        sc = np.ldexp(1.0, ea + ebs - 24)
    else:
        v = acc[5]
        for g in range(4, -1, -1):
            v = v * 2.0 ** -8 + acc[g]
        sc = np.ldexp(1.0, ea + ebs - 16)
    hx, hc = (-0.5 * T) * o["xn"], (-0.5 * T) * o["cn"]
    t = np.maximum(np.minimum((v * sc[None, :] + hx[:, None]) + hc[None, :], 0.0), T_MIN)
    ebk = i8_kstar_exp(sf2)
    ks = exp2t(t, sf2, 2.0 ** -ebk)                # y = k* 2^-ebk <= 0.49
    N = np.rint(np.ldexp(ks, 48))
    return np.ldexp(N, ebk - 48)


def worst(k, k_ref, tol):
    """-> (max error / tolerance, (r, c) of it) over the elements with a reference"""
    err = np.abs(np.asarray(k).astype(np.longdouble) - k_ref).astype(np.float64)
    ratio = np.where(np.isnan(err), 0.0, err / tol)
    at = np.unravel_index(int(np.argmax(ratio)), ratio.shape)
    return float(ratio[at]), (int(at[0]), int(at[1]))


# --------------------------------------------------------------------------- the categorical case
def cat_space():
    """tests/test_gpu_kstar_q.py's small mixed space"""
    from oracle.space import FLOAT, INT, Param
    return [Param("x", FLOAT, -5.0, 5.0), Param("n", INT, 1, 64), Param("flag", BOOL),
            Param("mode", ENUM, options=["a", "b", "c", 4]), Param("y", FLOAT, 0.0, 1.0),
            Param("sel", ENUM, options=[str(i) for i in range(9)]), Param("big", INT, -100000, 2000000)]


CAT = dict(name="cat_mixed", n=300, m=257, sf2=1.0, ell=1.25)


def cat_data():
    """-> dict space, tr [ncols][n], cand [ncols][m] (values), X [n][F], U [m][F]
    (features), num / cat (feature column masks), y, k_ref: the numeric columns in the
    difference form, the ENUM / BOOL blocks as their exact one-hot distance"""
    if "cat" not in _DATA:
        from oracle import de as ode
        from oracle.space import features
        space = cat_space()
        tr = ode.population_init(space, CAT["n"], seed=8)
        cand = ode.population_init(space, CAT["m"], seed=7)
        cand[:, :8] = tr[:, :8]                    # candidates on training rows
        X, U = features(space, tr).T.copy(), features(space, cand).T.copy()
        cat = np.concatenate([np.full(len(p.options) if p.kind == ENUM else 1, p.kind in (ENUM, BOOL))
                              for p in space])
        assert cat.size == X.shape[1]
        assert np.all(np.isin(X[:, cat], (0.0, 1.0))) and np.all(np.isin(U[:, cat], (0.0, 1.0)))
        ell = np.full(X.shape[1], CAT["ell"])
        # the one-hot blocks' squared distance: an integer count of differing codes over ell^2
        cnt = np.array([[np.sum(X[r, cat] != U[c, cat]) for c in range(U.shape[0])] for r in range(X.shape[0])])
        extra = cnt.astype(np.longdouble) / (np.longdouble(CAT["ell"]) ** 2)
        k_ref = reference(X[:, ~cat], U[:, ~cat], ell[~cat], CAT["sf2"], extra=extra)
        y = np.sum((X - 0.35) ** 2, axis=1)
        z = dict(space=space, tr=tr, cand=cand, X=X, U=U, cat=cat, ell=ell, y=y, k_ref=k_ref)
        for a in z.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _DATA["cat"] = z
    return _DATA["cat"]
