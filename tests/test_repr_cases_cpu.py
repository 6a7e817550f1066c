"""The case table of tests/test_gpu_repr.py, checked on the CPU: the branch
classifier of tests/_repr_cases.py against CPython's repr, the table's cover
of every branch tag, the host build of csrc/ut_core.h on the same values (so
a GPU failure says at once whether the device build or the shared text is
wrong), and the 24-byte bound SCR_WORDS = 7 of csrc/hash.hip rests on."""
import ctypes

import _repr_cases as rc
from test_core_host import hc  # noqa: F401  (the fixture that builds and binds the host library)


def _digits_decpt(s):
    """repr(float) of a finite value -> (digits without leading / trailing zeros, decpt)"""
    s = s.lstrip("-")
    if "e" in s:
        m, e = s.split("e")
        ip, _, fp = m.partition(".")
        allc, point = ip + fp, len(ip) + int(e)
    else:
        ip, _, fp = s.partition(".")
        allc, point = ip + fp, len(ip)
    lead = len(allc) - len(allc.lstrip("0"))
    d = allc.strip("0")
    if not d:
        return "0", 1          # repr(0.0): one digit, decpt 1 (the header's zero case)
    return d, point - lead


def test_digits_decpt_parser():
    assert _digits_decpt("1000.0") == ("1", 4)
    assert _digits_decpt("-0.00012") == ("12", -3)
    assert _digits_decpt("1.5e-07") == ("15", -6)
    assert _digits_decpt("1e+22") == ("1", 23)
    assert _digits_decpt("123.456") == ("123456", 3)
    assert _digits_decpt("-0.0") == ("0", 1)


def test_classifier_reproduces_cpython_repr():
    bad = []
    for x in rc.table():
        c = rc.classify(x)
        if c.digits is None:
            assert repr(x).lstrip("-") in ("inf", "nan") and c.tags == {"nonfinite"}
            continue
        d = c.digits.rstrip("0") or "0"
        if (d, c.decpt) != _digits_decpt(repr(x)):
            bad.append((x.hex(), repr(x), c.digits, c.decpt))
    assert not bad, bad[:5]


def test_classifier_layout_matches_repr_text():
    """the layout tags say what the string looks like"""
    for x in rc.table():
        t, s = rc.classify(x).tags, repr(x).lstrip("-")
        if "nonfinite" in t:
            continue
        assert ("lay_exp" in t) == ("e" in s), x.hex()
        if "lay_exp" in t:
            assert ("exp3" in t) == (len(s.split("e")[1]) == 4) and ("exp2" in t) == (len(s.split("e")[1]) == 3), x.hex()
        assert ("lay_lead" in t) == (s.startswith("0.") and "e" not in s and s != "0.0"), x.hex()
        assert ("lay_trail" in t) == (s.endswith(".0") and "e" not in s), x.hex()


def test_every_tag_occurs():
    """every tag at least PER_TAG times (zero and nonfinite: twice); the list of all counts
    is printed (pytest -s, or -rP, shows it)"""
    counts = rc.tag_counts()
    print("\ntable(): %d values; tag counts:" % len(rc.table()))
    for t in rc.ALL_TAGS:
        print("  %-18s %d" % (t, counts[t]))
    assert sorted(counts) == sorted(rc.ALL_TAGS)
    for t in rc.ALL_TAGS:
        assert counts[t] >= rc.FEW_TAGS.get(t, rc.PER_TAG), "tag %s occurs %d times in table()" % (t, counts[t])


def test_table_is_deterministic_and_distinct():
    xs = rc.table()
    assert xs is rc.table()
    assert len({rc.bits_of(x) for x in xs}) == len(xs)
    nans = [x for x in xs if x != x]
    assert len(nans) == 2 and rc.bits_of(nans[0]) != rc.bits_of(nans[1])


def test_repr_length_bound():
    """24 bytes of text at most: the pad byte of the inner SHA-256 block lands at byte
    <= 24, inside the SCR_WORDS = 7 words (bytes 0..27) of a lane's LDS column"""
    xs = rc.table()
    assert max(len(repr(x)) for x in xs) == 24
    assert all(len(repr(x)) <= 24 for x in xs)
    assert max(len(repr(v)) for v in rc.int_cases()) <= 24


def test_host_build_matches_cpython(hc):  # noqa: F811
    buf = ctypes.create_string_buffer(64)
    bad = []
    for x in rc.table():
        n = hc.uthc_repr_double(x, buf)
        if buf.raw[:n].decode() != repr(x):
            bad.append((x.hex(), repr(x), buf.raw[:n], sorted(rc.classify(x).tags)))
    assert not bad, (len(bad), bad[:5])
    for v in rc.int_cases():
        n = hc.uthc_repr_int64(v, buf)
        assert buf.raw[:n].decode() == repr(v), v


def test_int_and_logint_cases():
    ints = rc.int_cases()
    assert all(abs(v) <= 2 ** 53 - 1 and float(v) == v for v in ints)
    assert {len(str(abs(v))) for v in ints} == set(range(1, 17))
    for k in range(1, 16):
        for v in (10 ** k - 1, 10 ** k, 10 ** k + 1):
            assert v in ints and -v in ints
    lg = rc.logint_cases()
    assert all(0 <= v <= 2 ** 31 - 1 for v in lg)
    assert 0 in lg and all(2 ** k - 1 in lg for k in range(31))
    assert set(x - 1 for x in rc.non_cr_log_ints()) <= set(lg)
