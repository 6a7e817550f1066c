"""The case table of the device repr tests, and a branch classifier for it.

`classify(x)` names, from the bits of a double, the branches of
`ut::repr_double` / `ut::d2d` (uptune_amd/csrc/ut_core.h) that the value
takes, and returns the decimal digits and `decpt` those branches lead to.  It
is written with exact Python integers: the selection formulas are the
header's own (log10Pow2, log10Pow5, q <= 21, q <= 1, q < 63, mmShift, the
small-integer test), while vr / vp / vm come from exact big-integer division
instead of the 128-bit power-of-5 tables (Ryu's mulShift is proven to equal
that floor).  tests/test_repr_cases_cpu.py holds its digits and decpt to
CPython's repr, which is what keeps the tags honest.

`table()` is the list of doubles every float test of tests/test_gpu_repr.py
hashes: a fixed list of specials plus, for every tag, the first PER_TAG values
of a seeded pool that carry it; shuffled, so neighbouring lanes of a wave
format strings of different layouts and lengths.  `int_cases()` and
`logint_cases()` are the value lists of the wide INT and LOGINT tests.

(CPU only; no GPU, no torch.)
"""
import json
import math
import os
import random
import struct
from collections import namedtuple

SEED = 20240607
PER_TAG = 8
POOL_ROUNDS = 20000                # x 6 pool values per round

Classified = namedtuple("Classified", "tags digits decpt")

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")


def bits_of(x):
    return struct.unpack("<Q", struct.pack("<d", x))[0]


def from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


# --------------------------------------------------------------------------- tags
ENTRY_TAGS = ["zero", "nonfinite", "smallint", "subnormal", "mmShift0"]
POS_TAGS = ["pos_q21_mv5_0", "pos_q21_mv5_1", "pos_q21_even_0", "pos_q21_even_1", "pos_q21_odd_0", "pos_q21_odd_1",
            "pos_qbig"]
NEG_TAGS = ["neg_q1_even", "neg_q1_odd", "neg_qmid_0", "neg_qmid_1", "neg_qbig"]
GENERAL_TAGS = ["general", "general_vm_loop", "half_even", "general_vr_eq_vm"]
FAST_TAGS = ["fast_div100", "fast_nodiv100", "fast_vr_eq_vm", "fast_ru_0", "fast_ru_1"]
LAYOUT_TAGS = (["n%d" % n for n in range(1, 18)] + ["lay_exp", "lay_lead", "lay_inner", "lay_trail", "exp2", "exp3"] +
               ["decpt_%d" % k for k in range(-5, 19)])
ALL_TAGS = ENTRY_TAGS + POS_TAGS + NEG_TAGS + GENERAL_TAGS + FAST_TAGS + LAYOUT_TAGS
# tags of which the table needs only two values (there are no more distinct strings to have)
FEW_TAGS = {"zero": 2, "nonfinite": 2}


def _log10Pow2(e):
    return (e * 78913) >> 18


def _log10Pow5(e):
    return (e * 732923) >> 20


def _pow5factor(v):
    n = 0
    while v % 5 == 0:
        v //= 5
        n += 1
    return n


def _layout_tags(tags, n, decpt):
    tags.add("n%d" % n)
    if decpt <= -4 or decpt > 16:
        tags.add("lay_exp")
        tags.add("exp3" if abs(decpt - 1) >= 100 else "exp2")
    elif decpt <= 0:
        tags.add("lay_lead")
    elif decpt < n:
        tags.add("lay_inner")
    else:
        tags.add("lay_trail")
    if -5 <= decpt <= 18:
        tags.add("decpt_%d" % decpt)


def classify(x):
    """-> Classified(tags, digits, decpt); digits / decpt are None for inf and nan"""
    b = bits_of(x)
    mant = b & ((1 << 52) - 1)
    expo = (b >> 52) & 0x7FF
    tags = set()
    if expo == 0x7FF:
        tags.add("nonfinite")
        return Classified(tags, None, None)
    if expo == 0 and mant == 0:
        tags.add("zero")
        _layout_tags(tags, 1, 1)
        return Classified(tags, "0", 1)
    e2i = expo - 1023 - 52
    m2i = (1 << 52) | mant
    if expo != 0 and -52 <= e2i <= 0 and (m2i & ((1 << -e2i) - 1)) == 0:
        tags.add("smallint")
        v = m2i >> -e2i
        e10 = 0
        while v % 10 == 0:
            v //= 10
            e10 += 1
        digits = str(v)
        decpt = len(digits) + e10
        _layout_tags(tags, len(digits), decpt)
        return Classified(tags, digits, decpt)

    # ---- d2d
    if expo == 0:
        tags.add("subnormal")
        e2, m2 = 1 - 1023 - 52 - 2, mant
    else:
        e2, m2 = expo - 1023 - 52 - 2, m2i
    even = (m2 & 1) == 0
    mv = 4 * m2
    mm_shift = 1 if (mant != 0 or expo <= 1) else 0
    if mm_shift == 0:
        tags.add("mmShift0")
    lo_m = mv - 1 - mm_shift
    vm_tz = vr_tz = False
    if e2 >= 0:
        q = _log10Pow2(e2) - (1 if e2 > 3 else 0)
        e10 = q
        p10 = 10 ** q
        vr = (mv << e2) // p10
        vp = ((mv + 2) << e2) // p10
        vm = (lo_m << e2) // p10
        if q <= 21:
            if mv % 5 == 0:
                vr_tz = _pow5factor(mv) >= q
                tags.add("pos_q21_mv5_%d" % vr_tz)
            elif even:
                vm_tz = _pow5factor(lo_m) >= q
                tags.add("pos_q21_even_%d" % vm_tz)
            else:
                dec = _pow5factor(mv + 2) >= q
                vp -= 1 if dec else 0
                tags.add("pos_q21_odd_%d" % dec)
        else:
            tags.add("pos_qbig")
    else:
        q = _log10Pow5(-e2) - (1 if -e2 > 1 else 0)
        e10 = q + e2
        p5 = 5 ** (-e2 - q)
        vr = (mv * p5) >> q
        vp = ((mv + 2) * p5) >> q
        vm = (lo_m * p5) >> q
        if q <= 1:
            vr_tz = True
            if even:
                vm_tz = mm_shift == 1
                tags.add("neg_q1_even")
            else:
                vp -= 1
                tags.add("neg_q1_odd")
        elif q < 63:
            vr_tz = (mv & ((1 << q) - 1)) == 0
            tags.add("neg_qmid_%d" % vr_tz)
        else:
            tags.add("neg_qbig")

    removed = 0
    last = 0
    if vm_tz or vr_tz:
        tags.add("general")
        while vp // 10 > vm // 10:
            vm_tz = vm_tz and vm % 10 == 0
            vr_tz = vr_tz and last == 0
            last = vr % 10
            vr, vp, vm = vr // 10, vp // 10, vm // 10
            removed += 1
        if vm_tz:
            while vm % 10 == 0:
                tags.add("general_vm_loop")
                vr_tz = vr_tz and last == 0
                last = vr % 10
                vr, vp, vm = vr // 10, vp // 10, vm // 10
                removed += 1
        if vr_tz and last == 5 and vr % 2 == 0:
            tags.add("half_even")
            last = 4
        eq = vr == vm and (not even or not vm_tz)
        if eq:
            tags.add("general_vr_eq_vm")
        out = vr + (1 if (eq or last >= 5) else 0)
    else:
        round_up = False
        if vp // 100 > vm // 100:
            tags.add("fast_div100")
            round_up = vr % 100 >= 50
            vr, vp, vm = vr // 100, vp // 100, vm // 100
            removed += 2
        else:
            tags.add("fast_nodiv100")
        while vp // 10 > vm // 10:
            round_up = vr % 10 >= 5
            vr, vp, vm = vr // 10, vp // 10, vm // 10
            removed += 1
        if vr == vm:
            tags.add("fast_vr_eq_vm")
        tags.add("fast_ru_%d" % round_up)
        out = vr + (1 if (vr == vm or round_up) else 0)
    digits = str(out)
    decpt = len(digits) + e10 + removed
    _layout_tags(tags, len(digits), decpt)
    return Classified(tags, digits, decpt)


# --------------------------------------------------------------------------- the table
# (the SPECIAL list of tests/test_core_host.py is shared, not copied: importing that module
# builds nothing, its host library is a fixture)
def _host_special():
    from test_core_host import SPECIAL
    return list(SPECIAL)


NAN_A = from_bits(0x7FF8000000000000)        # the quiet NaN float("nan") gives
NAN_B = from_bits(0xFFF4000000BEEF01)        # another payload, sign set


def _neighbours(x):
    out = [x]
    if math.isfinite(x):
        out = [math.nextafter(x, -math.inf), x, math.nextafter(x, math.inf)]
    return out


def _specials():
    xs = _host_special()
    xs += [0.0, -0.0, math.inf, -math.inf, NAN_A, NAN_B]
    for k in range(-1074, 1024):
        xs += _neighbours(math.ldexp(1.0, k))
    for k in range(-323, 309):
        xs += _neighbours(float("1e%d" % k))
    xs += [float(2 ** 53 - 1), float(2 ** 53), float(2 ** 53 + 2), 1e15, 1e16, 1e17, 9999999999999998.0, 0.0001,
           0.00001]
    return xs


def _pool(rng):
    """the seeded pool, one value of each of its six sources per round"""
    for _ in range(POOL_ROUNDS):
        yield from_bits(rng.getrandbits(64))
        yield rng.uniform(-1000.0, 1000.0)
        yield float(rng.randrange(1 << 54, 1 << 90))
        yield float(rng.randrange(1, 1 << 20) * 5 ** rng.randrange(0, 22) * 2 ** rng.randrange(30, 60))
        yield math.ldexp(float(rng.randrange(1, 1 << 53)), -rng.randrange(0, 70))
        yield rng.randrange(1, 10 ** 6) / 10 ** rng.randrange(0, 12)


_TABLE = None


def table():
    """the case list (built once per process): specials + PER_TAG pool values per tag,
    one entry per bit pattern, shuffled with SEED"""
    global _TABLE
    if _TABLE is not None:
        return _TABLE
    rng = random.Random(SEED)
    need = {t: PER_TAG for t in ALL_TAGS}
    # the pool's only non-finite values are random NaNs, all one string, and it holds no zero:
    # the specials have +-0.0, +-inf and the two NaNs.  (Two more tags the pool does not reach,
    # mmShift0 -- a power of two outside [1, 2^53) -- and n1 outside the small integers, come
    # from the specials' 2^k and 1e+-k; tests/test_repr_cases_cpu.py counts every tag.)
    need["nonfinite"] = need["zero"] = 0
    picks = []
    open_tags = {t for t, n in need.items() if n > 0}
    for x in _pool(rng):
        if not open_tags:
            break
        if x != x or math.isinf(x):
            continue
        hit = classify(x).tags & open_tags
        if not hit:
            continue
        picks.append(x)
        for t in hit:
            need[t] -= 1
            if need[t] == 0:
                open_tags.discard(t)
    seen, out = set(), []
    for x in _specials() + picks:
        b = bits_of(x)
        if b not in seen:
            seen.add(b)
            out.append(x)
    rng.shuffle(out)
    _TABLE = out
    return out


def tag_counts(xs=None):
    counts = {t: 0 for t in ALL_TAGS}
    for x in (table() if xs is None else xs):
        for t in classify(x).tags:
            counts[t] += 1
    return counts


# --------------------------------------------------------------------------- integers
def int_cases():
    """values of a wide INT parameter, every digit count 1..16 and every power-of-ten edge"""
    rng = random.Random(SEED + 1)
    xs = [0, 1, -1]
    for k in range(1, 16):
        for v in (10 ** k - 1, 10 ** k, 10 ** k + 1):
            xs += [v, -v]
    xs += [2 ** 53 - 1, -(2 ** 53 - 1)]
    for nd in range(1, 17):
        lo = 10 ** (nd - 1) if nd > 1 else 0
        hi = min(10 ** nd - 1, 2 ** 53 - 1)
        for _ in range(200):
            v = rng.randint(lo, hi)
            xs.append(-v if rng.getrandbits(1) else v)
    return xs


def non_cr_log_ints():
    """integers x in [2^22, 2^31) where CPython's math.log(x) is not the correctly
    rounded log (tests/golden/libm_log_non_cr.json, made by tests/golden/make_libm_log_cases.py)"""
    with open(os.path.join(GOLDEN, "libm_log_non_cr.json")) as f:
        return json.load(f)["ints"]


def logint_cases():
    """stored values v of a LOGINT parameter over [0, 2^31 - 1]: x = v + 1 is 1 (log2 = 0.0,
    the zero path), every power of two (an integral log2 where the division is exact: the
    small-integer path), its two neighbours, and the golden arguments where libm's log is
    not correctly rounded"""
    xs = [1]
    for k in range(1, 32):
        xs += [2 ** k - 1, 2 ** k, 2 ** k + 1]
    xs = sorted({x for x in xs if 1 <= x <= 2 ** 31})
    xs += [int(x) for x in non_cr_log_ints()]
    return [x - 1 for x in xs]
