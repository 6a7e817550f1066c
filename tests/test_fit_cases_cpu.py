"""tests/_fit_cases.py checked on the CPU: the table's sizes reach the paths
they claim, the two fp64 references of the fit (LAPACK's route and the numpy
restatement of gp_fit.hip) stay under the derived cap and within a factor 4 of
each other -- what makes 4 rho_ref a meaningful line for the device -- every
mutant of the restatement exceeds that line, and the exact int8 expectations
agree with a bit-level restatement of i8_biased / k_split_i8 on crafted rows.
The host-side argument checks of ut_gp_fit_read that need no context are here
too."""
import ctypes
import os
import re
import sys

import numpy as np
import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _fit_cases as F  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = list(F.CASES) + [F.chain_case(*ch) for ch in F.CHAINS]


def test_longdouble_is_extended():
    assert F.have_longdouble()


def test_table_reaches_the_paths_claimed():
    assert sorted({c["n"] for c in F.CASES}) == sorted(F.PATHS)
    for n, (npad, ragged) in F.PATHS.items():
        assert F.npad_of(n) == npad and npad <= 768
        lv = F.levels(npad)
        assert [s for s, _, _, _ in lv] == [s for s in (64, 128, 256, 512) if s < npad]
        assert [k for _, _, _, k in lv] == ["big" if s >= 256 else "level" for s, _, _, _ in lv]
        rag = [(s, s2) for s, _, s2, _ in lv if s2 < s]
        assert rag == ([(lv[-1][0], ragged)] if ragged else [])
    assert F.levels(256) == [(64, 2, 64, "level"), (128, 1, 128, "level")]
    assert F.levels(384)[-1] == (256, 1, 128, "big") and F.levels(640)[-1] == (512, 1, 128, "big")
    assert F.levels(768)[-1] == (512, 1, 256, "big")
    assert sum(F.npad_of(c["n"]) == 768 for c in ALL) == 2
    assert {c["d"] for c in F.CASES} >= {3, 33, 64} and {c["sf2"] for c in F.CASES} == {1e-3, 1.0, 37.0}
    assert {c["sn2"] for c in F.CASES} == {1e-9, 1e-6, 1e-2}
    assert sum(c["dup"] for c in F.CASES) == 1 and sum(c["cat"] for c in F.CASES) == 1
    for env, ns in F.SWITCHES:
        assert ns is None or all(n in F.PATHS for n in ns)
    # the chains: every step an append (one padded size), l_rows the first appended block row
    for n0, steps, d in F.CHAINS:
        c = F.chain_case(n0, steps, d)
        assert F.npad_of(n0) == F.npad_of(c["n"])
        assert F.restate(c, F.data(c))["l_rows"] == F.CHAIN_L_ROWS[n0] == n0 // 64 * 64


@pytest.mark.parametrize("c", ALL, ids=[c["name"] for c in ALL])
def test_references_and_mutants(c):
    z = F.data(c)
    ref, l_rows = F.references(c, z)
    assert l_rows == (F.CHAIN_L_ROWS[c["n0"]] if "steps" in c else F.npad_of(c["n"]))
    for m, (ra, rb) in ref.items():
        print("%s %s: lapack %.3g, restatement %.3g, cap %d" % (c["name"], m, ra, rb, F.cap(c)))
        assert max(ra, rb) <= F.cap(c), (m, ra, rb)
        if m == "chol" and c["panel"]:
            continue
        # (the line the smaller one would set: 4x, and for a single block max(4x, 1))
        assert max(ra, rb) <= F.line(c, min(ra, rb), 0.0), "%s: the references differ by more than 4x: %g, %g" % (m, ra, rb)
    for mut in F.MUTANTS:
        if not F.applies(mut, c):
            continue
        m = F.mutant_measure(mut, c)
        fit = F.restate(c, z, mut)
        rho = F.measure(m, fit, z, c["n"], fit["l_rows"] if m == "chol" else None)[0]
        print("%s mutant %s: %s %.3g against the line %.3g" % (c["name"], mut, m, rho, F.line(c, *ref[m])))
        assert rho > F.line(c, *ref[m]), "mutant %s passes %s: %g <= %g" % (mut, m, rho, F.line(c, *ref[m]))


def test_every_mutant_applies_somewhere():
    for mut in F.MUTANTS:
        assert any(F.applies(mut, c) for c in ALL), mut
    tight_refits = [c for c in F.CASES if c["tight"]]
    for mut in ("l_tile_f32", "x_tile_f32", "no_jitter", "upd_chunk", "dbl_chunk"):
        assert all(F.applies(mut, c) for c in tight_refits), mut


def test_ys_reference_and_restated_vectors():
    """the restatement's beta and alpha pass their own bounds (<= 1), ys_bound holds for
    a plain fp64 standardisation"""
    c = F.CASES[5]
    z = F.data(c)
    n = c["n"]
    y = z["y"]
    mean = np.sum(y) / n
    sd = np.sqrt(np.sum((y - mean) ** 2) / n)
    ys = (y - mean) / sd
    assert F.m_ys(ys, z, n)[0] <= 1.0
    assert F.m_ys(ys * (1.0 + 2.0 ** -44), z, n)[0] > 1.0
    db, ds = F.stats_bounds(y, z["sd"])
    assert abs(mean - float(z["mean"])) <= db and abs(sd - float(z["sd"])) <= ds
    fit = F.restate(c, z)
    beta = np.tril(fit["X"][:n, :n]) @ ys
    assert F.m_beta(beta, fit["X"], ys, n)[0] <= 1.0
    alpha = fit["X"][:n, :n].T @ beta
    assert F.m_alpha(alpha, fit["X"], beta, n)[0] <= 1.0
    bad = beta.copy()
    bad[n - 1] *= 1.0 + 2.0 ** -36
    assert F.m_beta(bad, fit["X"], ys, n)[0] > 1.0


def test_i8_expectations_on_crafted_rows():
    """i8_expected (rint of the scaled value) against the bit-level restatement of
    i8_biased / k_split_i8: a value on a digit tie, max |x| exactly 0.49 2^e, an
    all-zero row, a 1-element row, rows past n"""
    eb = 3
    npad, n = 128, 100
    rng = np.random.default_rng(5)
    X = np.tril(rng.standard_normal((npad, npad)) * np.exp(4.0 * rng.standard_normal((npad, 1))))
    X[0, 0] = 0.7
    X[7, :8] = 0.0                                   # an all-zero row
    X[9, :10] = rng.uniform(-0.2, 0.2, 10) * 2.0 ** -6
    X[9, 3] = 0.49 * 2.0 ** -5                       # max |x| exactly 0.49 2^e
    ea9 = F.i8_row_exp(0.49 * 2.0 ** -5)
    X[11, :12] = rng.uniform(-0.1, 0.1, 12)
    X[11, 0] = 0.25                                  # ea = 0 here: x 2^48 on ties below
    X[11, 1] = (2 ** 20 + 0.5) * 2.0 ** -48          # a tie: to even, down
    X[11, 2] = (2 ** 20 + 1.5) * 2.0 ** -48          # a tie: to even, up
    X[11, 3] = -(127.5) * 2.0 ** -48                 # a tie across a digit boundary
    X[11, 4] = (0x7f7f7f7f7f80 - 0.5) * 2.0 ** -50   # every digit at its positive end
    X[:, :] = np.tril(X)
    ea, rs, N, e2 = F.i8_expected(X, n, eb)
    assert ea[11] == 0 and ea[9] == ea9 and rs[7] == 0.0 and np.all(rs[n:] == 0.0) and np.all(N[n:] == 0.0)
    assert np.all(N[np.triu_indices(npad, 1)] == 0.0)
    assert N[11, 1] == 2 ** 20 and N[11, 2] == 2 ** 20 + 2 and N[11, 3] == -128
    for r in (0, 7, 9, 11, 50, n - 1, n, npad - 1):
        kend = r + 1 if r < n else 0
        ea_r, rs_r, dg, Nr, e2_r = F.i8_split_restated(X[r], kend, eb)
        assert ea_r == ea[r] and rs_r == rs[r] and e2_r == e2[r], r
        assert np.array_equal(Nr.astype(np.float64), N[r]), r
        assert np.all(dg >= -128) and np.all(dg <= 127)
        if kend:
            assert np.max(np.abs(np.ldexp(X[r, :kend], -ea_r))) <= 0.49 * (1 + 2.0 ** -52)
            assert np.max(np.abs(X[r] * (np.arange(npad) < kend) - np.ldexp(Nr.astype(np.float64), ea_r - 48))) \
                <= 2.0 ** (ea_r - 49)
    assert rs[0] == 2.0 ** (F.i8_row_exp(0.7) + eb) and e2[0] == (F.I8_C * rs[0]) ** 2


def test_fit_read_host_side():
    """what ut_gp_fit_read answers without a context, and that the Python side mirrors
    the header: the operand codes and the info struct's layout"""
    from uptune_amd import _lib as L
    lib = L.lib()
    info = L.GpFitInfo()
    for w in list(L.FIT_OPERANDS.values()) + [-1, 99]:
        assert lib.ut_gp_fit_read(None, w, None, ctypes.byref(info)) == -1      # UT_EINVAL
    src = open(os.path.join(ROOT, "include", "uthot.h")).read()
    codes = {k: int(v) for k, v in re.findall(r"UT_FIT_(\w+) = (\d+)", src)}
    assert codes == L.FIT_OPERANDS and sorted(codes.values()) == list(range(len(codes)))
    hc = ctypes.CDLL(os.path.join(os.path.dirname(L.LIB_PATH), "libuthot_hostcheck.so"))
    hc.uthc_sizeof.restype = ctypes.c_longlong
    assert ctypes.sizeof(L.GpFitInfo) == hc.uthc_sizeof(9) == 20
    body = re.search(r"typedef struct ut_gp_fit_info \{(.*?)\}", src, re.S).group(1)
    names = re.findall(r"(\w+)\s*[,;]", re.sub(r"/\*.*?\*/", "", body, flags=re.S))
    assert names == [f for f, _ in L.GpFitInfo._fields_] == ["n", "npad", "precision", "l_rows", "stale"]
