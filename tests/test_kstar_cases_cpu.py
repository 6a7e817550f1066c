"""The K* case table (tests/_kstar_cases.py) checked on the CPU, so the device
tests (test_gpu_kstar_elements.py) can assert without conditions:
 a. the numpy restatement of k_gp_kstar_q's digit scheme meets the derived
    tolerance on every case (the largest error / tolerance is printed);
 b. the tolerance can fail: each mutant of the restatement (the U_67 pair
    dropped, the candidates' planes 4 and 5 zeroed, one column's eb_c off by
    one) exceeds it on every case marked tight;
 c. the reference agrees with oracle/gp.py's kernel to 1e-12 relative;
and the table reaches the shapes, scales and columns it is there for."""
import os
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _kstar_cases as KC  # noqa: E402
from oracle import gp as ogp  # noqa: E402


def test_reference_precision():
    """the longdouble the reference is computed in has at least 63 mantissa bits
    (else reference() takes the decimal sample, and the element checks cover it)"""
    if not KC.have_longdouble():
        z = KC.data(KC.CASES[2])
        assert np.count_nonzero(~np.isnan(z["k_ref"].astype(np.float64))) >= min(KC.SAMPLE, z["k_ref"].size)
        return
    assert np.finfo(np.longdouble).nmant >= 63


@pytest.mark.parametrize("c", KC.CASES, ids=KC.ids())
def test_restatement_meets_the_tolerance(c):
    z = KC.data(c)
    k = KC.restate_q(z["X"], z["U"], z["ell"], c["sf2"])
    tol = KC.tolerance(z["X"], z["U"], z["ell"], c["sf2"], "q", z["k_ref"])
    w, (r, col) = KC.worst(k, z["k_ref"], tol)
    print("%s: restatement %.3g of the tolerance at (%d, %d)" % (c["name"], w, r, col))
    assert w <= 1.0
    # the exponent is clamped at 0: k* <= sf2, up to the six digits' rounding of sf2 itself
    assert np.all(k <= c["sf2"] + 2.0 ** (-49 + KC.i8_kstar_exp(c["sf2"])))


@pytest.mark.parametrize("mutant", KC.MUTANTS)
@pytest.mark.parametrize("c", [c for c in KC.CASES if c["tight"]], ids=[c["name"] for c in KC.CASES if c["tight"]])
def test_mutants_exceed_the_tolerance(c, mutant):
    z = KC.data(c)
    k = KC.restate_q(z["X"], z["U"], z["ell"], c["sf2"], mutant=mutant)
    tol = KC.tolerance(z["X"], z["U"], z["ell"], c["sf2"], "q", z["k_ref"])
    w, (r, col) = KC.worst(k, z["k_ref"], tol)
    print("%s %s: %.3g of the tolerance at (%d, %d)" % (c["name"], mutant, w, r, col))
    assert w > 1.0


@pytest.mark.parametrize("c", KC.CASES, ids=KC.ids())
def test_reference_agrees_with_the_oracle(c):
    """oracle/gp.py's kernel, sf2 exp(-sqdist / 2) over the scaled inputs, in float64:
    1e-12 relative on every element (1e-300 absolutely, where exp underflows)"""
    z = KC.data(c)
    il = 1.0 / z["ell"]
    ko = c["sf2"] * np.exp(-0.5 * ogp.sqdist(z["X"] * il, z["U"] * il))
    kr = z["k_ref"].astype(np.float64)
    ok = ~np.isnan(kr)
    assert ok.sum() >= min(KC.SAMPLE, kr.size)
    err = np.abs(ko - kr)[ok] / (1e-300 + np.abs(kr[ok]))
    print("%s: oracle against the reference %.3g relative" % (c["name"], err.max()))
    assert err.max() <= 1e-12


def test_the_table_reaches_what_it_is_for():
    ds, ns, ms = {c["d"] for c in KC.CASES}, {c["n"] for c in KC.CASES}, {c["m"] for c in KC.CASES}
    assert {3, 32, 33, 64, 96, 97, 112} <= ds
    assert {1, 127, 128, 129, 300, 1000, 8200} <= ns
    assert {1, 63, 64, 65, 256, 257, 2049} <= ms
    assert {c["sf2"] for c in KC.CASES} == {1.0, 1e-3, 37.0}
    assert {"lo", "hi", "one_short_first", "one_short_last"} <= {c["ell"] for c in KC.CASES}
    assert any(c["pre_m"] > c["m"] for c in KC.CASES) and any(c["fit_async"] for c in KC.CASES)
    assert {KC.k32_of(d) for d in ds} >= {1, 2, 3, 4}
    assert 32 * KC.k32_of(96) <= KC.PAIR_MAX_K < 32 * KC.k32_of(97)
    assert any(KC.npad_of(c["n"]) // 64 > 64 for c in KC.CASES)          # more row tiles than an XCD's workgroups
    assert any((KC.ldk_of(c["m"]) // 64) % 8 for c in KC.CASES)


def test_special_columns_are_what_they_say():
    c = next(c for c in KC.CASES if c["d"] == 64 and c["ell"] == "hi" and c["m"] >= 64)
    z = KC.data(c)
    o = KC.operands(z["X"], z["U"], z["ell"])
    col = {nm: j for j, nm in enumerate(z["names"])}
    kr = z["k_ref"].astype(np.float64)
    assert col["near"] == KC.MUTANT_COL
    assert kr[1, col["copy"]] == c["sf2"] and np.all(z["U"][col["zero"]] == 0.0) and o["eb"][col["zero"]] == 0
    assert np.all(kr[:, col["far"]] < 1e-300)
    assert o["eb"][col["scale2^10"]] - o["eb"][col["scale2^-30"]] == 40
    # exact scaling (ell a power of two): the q_exp boundary and the byte patterns are hit exactly
    for j in (0, -3, 5):
        mx = [float(np.max(np.abs(o["Us"][col["q_exp2^%d_%s" % (j, s)]]))) for s in ("below", "at", "above")]
        assert mx[1] == 0.49 * 2.0 ** j and mx[0] == np.nextafter(mx[1], 0.0) and mx[2] == np.nextafter(mx[1], np.inf)
        assert [KC.q_exp(v) for v in mx][1:] == [j + 1, j + 1] and KC.q_exp(mx[0]) in (j, j + 1)
    for nm, eb in (("bytes", 1), ("bytes_all", 0)):
        j = col[nm]
        assert o["eb"][j] == eb
        dg = np.array([p[0] for p in KC.digits(o["Us"][j][None, :], eb)])      # [6][d], plane 0 the top
        low = dg[1:] if nm == "bytes" else dg[:, 1:]
        assert {int(v) for v in np.unique(low)} == ({-128, -1, 0, 127} if nm == "bytes" else {-1, 0})
        assert np.all(low == low[0][None, :])
