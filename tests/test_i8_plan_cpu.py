"""Precision-8 dense scoring's host decisions (uptune_amd/csrc/gp_i8_plan.h: i8_plan, i8_hints_next and the
per-call read of the three overrides), compiled for the host with g++ and held to the Python restatement in
_i8_plan_model.py over the whole product of overrides, shapes and hints; the thresholds and the back-off at
their exact edges (CPU, no GPU)."""
import ctypes
import itertools
import os
import subprocess
import sys

import pytest

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

import _i8_plan_model as M  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "uptune_amd", "csrc")
HOSTLIB = os.path.join(ROOT, "uptune_amd", "libuthot_hostcheck.so")

TRI = (M.UNSET, 0, 1)
ENVS = [M.Env(*e) for e in itertools.product(TRI, TRI, TRI)]
HINTS = [M.Hints(*h) for h in itertools.product((False, True), (False, True), (False, True), (0, 1, 8))]
SHAPES = list(itertools.product((2048, 2176), (4, 5)))
B = 128   # blocks of the threshold cases


@pytest.fixture(scope="module")
def hc():
    deps = [os.path.join(CSRC, f) for f in ("hostcheck.cpp", "gp_i8_plan.h", "ut_core.h")]
    if not os.path.exists(HOSTLIB) or os.path.getmtime(HOSTLIB) < max(os.path.getmtime(p) for p in deps):
        subprocess.check_call(["g++", "-O2", "-std=c++17", "-shared", "-fPIC", "-ffp-contract=off", deps[0], "-o",
                               HOSTLIB])
    return ctypes.CDLL(HOSTLIB)


def _ints(v):
    return (ctypes.c_int * len(v))(*[int(x) for x in v])


def _plan_of(bits):
    return M.Plan(bool(bits & 1), bool(bits & 2), bool(bits & 4), bits >> 4)


def lib_plan(hc, npad, k32, env, hints):
    return _plan_of(hc.uthc_i8_plan(npad, k32, _ints(env), _ints(hints)))


def lib_next(hc, hints, p, n):
    out = (ctypes.c_int * 4)()
    bits = int(p.mask) | int(p.screen) << 1 | int(p.count) << 2 | p.var << 4
    hc.uthc_i8_hints_next(_ints(hints), bits, (ctypes.c_longlong * 4)(*n), out)
    return M.Hints(bool(out[0]), bool(out[1]), bool(out[2]), out[3])


def _all_plans(hc):
    return sorted({lib_plan(hc, npad, k32, e, h) for npad, k32 in SHAPES for e in ENVS for h in HINTS} | {M.NO_MASK})


def test_plan_over_the_product(hc):
    seen = set()
    for (npad, k32), e, h in itertools.product(SHAPES, ENVS, HINTS):
        p = lib_plan(hc, npad, k32, e, h)
        assert p == M.plan(npad, k32, e, h), (npad, k32, e, h)
        # a screened K* left planes unwritten: a masked kernel; the list is the screen's; the count is of an
        # unscreened mask
        assert p.mask and p.var in (M.UNMASKED, M.MASKED, M.LIST)
        assert not p.screen or p.var in (M.MASKED, M.LIST)
        assert p.var != M.LIST or p.screen
        assert not (p.count and p.screen)
        # the limits: no masked kernel past 2048 rows, no screen past 4 stages or with the masked kernel forbidden
        assert npad <= 2048 or p == M.Plan(True, False, False, M.UNMASKED)
        assert not p.screen or (k32 <= 4 and e.var_skip != 0)
        seen.add(p)
    assert {(p.screen, p.count, p.var) for p in seen} == {
        (False, False, M.UNMASKED), (False, False, M.MASKED), (False, True, M.UNMASKED), (False, True, M.MASKED),
        (True, False, M.MASKED), (True, False, M.LIST)}
    assert _plan_of(hc.uthc_i8_plan_no_mask()) == M.NO_MASK


def test_the_overrides_one_by_one(hc):
    """what each variable forces, at a shape where everything can run and with every hint against it"""
    off, on = M.Hints(False, False, False, 0), M.Hints(True, True, True, 0)
    P = lambda e, h: lib_plan(hc, 2048, 4, M.Env(*e), h)   # noqa: E731
    U = M.UNSET
    assert P((U, U, U), off) == M.Plan(True, False, True, M.UNMASKED)
    assert P((U, U, U), on) == M.Plan(True, True, False, M.LIST)
    assert P((1, U, U), off) == M.Plan(True, False, True, M.MASKED)       # UT_VAR_SKIP=1: the masked kernel
    assert P((0, U, U), on) == M.Plan(True, False, False, M.UNMASKED)     # =0: neither it nor the screen (nor a count)
    assert P((0, 1, 1), on) == M.Plan(True, False, False, M.UNMASKED)
    assert P((U, 1, U), off) == M.Plan(True, True, False, M.MASKED)       # UT_KSTAR_SCREEN=1: the list to its hint
    assert P((U, 1, U), M.Hints(False, False, True, 0)) == M.Plan(True, True, False, M.LIST)
    assert P((U, 0, U), on) == M.Plan(True, False, False, M.MASKED)       # =0: no screen and nothing counted
    assert P((U, U, 1), M.Hints(True, True, False, 0)) == M.Plan(True, True, False, M.LIST)
    assert P((U, U, 0), on) == M.Plan(True, True, False, M.MASKED)
    assert P((U, U, 1), off) == M.Plan(True, False, True, M.UNMASKED)     # UT_KSTAR_STRIPS=1 screens nothing itself


@pytest.mark.parametrize("text,var_skip,other", [(None, -1, -1), ("0", 0, 0), ("1", 1, 1), ("2", 1, 0), ("-1", 1, 0),
                                                 ("", 0, 0), ("on", 0, 0)])
def test_env_read_per_call(hc, monkeypatch, text, var_skip, other):
    """UT_VAR_SKIP is on with any non-zero number; UT_KSTAR_SCREEN and UT_KSTAR_STRIPS with 1 alone.  Each read
    sees the environment of that moment"""
    for name in ("UT_VAR_SKIP", "UT_KSTAR_SCREEN", "UT_KSTAR_STRIPS"):
        if text is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, text)
    out = (ctypes.c_int * 3)()
    hc.uthc_i8_env_read(out)
    assert list(out) == [var_skip, other, other]
    monkeypatch.setenv("UT_KSTAR_STRIPS", "1")
    monkeypatch.delenv("UT_VAR_SKIP", raising=False)
    hc.uthc_i8_env_read(out)
    assert list(out) == [-1, other, 1]


def test_initial_hints(hc):
    out = (ctypes.c_int * 4)()
    hc.uthc_i8_hints_initial(out)
    assert M.Hints(bool(out[0]), bool(out[1]), bool(out[2]), out[3]) == M.Hints() == M.Hints(True, False, False, 0)


def test_hints_over_the_product(hc):
    counts = [M.Counts(ns, ce, zb, B) for ns in (0, 7, 8, 128) for ce in (0, 1, 7, 8, 14, 16)
              for zb in (0, 63, 64, 111, 112, 128)]
    for p, h, n in itertools.product(_all_plans(hc), HINTS, counts):
        assert lib_next(hc, h, p, n) == M.hints_next(h, p, n), (p, h, n)


def test_thresholds_exactly(hc):
    counted, screened = M.Plan(True, False, True, M.MASKED), M.Plan(True, True, False, M.MASKED)
    h0 = M.Hints(False, False, False, 0)
    for zb, screen, lst in ((63, False, False), (64, True, False), (111, True, False), (112, True, True)):
        got = lib_next(hc, h0, counted, M.Counts(0, 0, zb, B))
        assert (got.screen, got.list) == (screen, lst), zb
    # screened: 8 blocks per certified unit (8 units = 64 blocks, 14 = 112)
    for ce, screen, lst in ((7, False, False), (8, True, False), (13, True, False), (14, True, True)):
        got = lib_next(hc, h0, screened, M.Counts(0, ce, 0, B))
        assert (got.screen, got.list) == (screen, lst), ce
    # var_skip: 1 block in 16, the certified units' blocks among them
    assert lib_next(hc, h0, counted, M.Counts(7, 0, 0, B)).var_skip is False
    assert lib_next(hc, h0, counted, M.Counts(8, 0, 0, B)).var_skip is True
    assert lib_next(hc, h0, screened, M.Counts(0, 1, 0, B)).var_skip is True       # nsparse + 8 cert = 8
    assert lib_next(hc, h0, counted, M.Counts(0, 1, 0, B)).var_skip is False       # (not screened: cert is not read)
    # a forced-off screen counted nothing: zero blocks 0 whatever ks_cnt held
    forced_off = M.Plan(True, False, False, M.MASKED)
    got = lib_next(hc, M.Hints(True, True, True, 0), forced_off, M.Counts(128, 16, 128, B))
    assert (got.screen, got.list, got.var_skip) == (False, False, True)


def test_back_off(hc):
    U = M.Env()
    h = M.Hints(True, True, False, 0)
    p = lib_plan(hc, 256, 1, U, h)
    assert p.screen
    h = lib_next(hc, h, p, M.Counts(60, 7, 0, B))           # certified 56 of 128 blocks: under half
    assert (h.screen, h.backoff) == (False, 8)
    for left in range(7, -1, -1):                           # eight unscreened calls whose counts alone would screen
        p = lib_plan(hc, 256, 1, U, h)
        assert not p.screen and p.count
        n = M.Counts(70, 0, 68, B)
        assert lib_next(hc, M.Hints(h.var_skip, h.screen, h.list, 0), p, n).screen is True
        h = lib_next(hc, h, p, n)
        assert (h.screen, h.backoff) == (False, left)
    p = lib_plan(hc, 256, 1, U, h)
    assert not p.screen
    h = lib_next(hc, h, p, M.Counts(70, 0, 68, B))          # the ninth
    assert (h.screen, h.backoff) == (True, 0)
    assert lib_plan(hc, 256, 1, U, h).screen
    # the count-down also runs under a forced-off screen, and a screened call that clears half leaves it alone
    h = M.Hints(True, False, False, 3)
    p = lib_plan(hc, 256, 1, M.Env(M.UNSET, 0, M.UNSET), h)
    assert not p.screen and not p.count
    assert lib_next(hc, h, p, M.Counts(70, 0, 0, B)).backoff == 2
    p = lib_plan(hc, 256, 1, M.Env(M.UNSET, 1, M.UNSET), h)
    assert p.screen
    assert lib_next(hc, h, p, M.Counts(0, 8, 0, B)) == M.Hints(True, True, False, 3)


def test_a_maskless_kstar_leaves_the_hints(hc):
    for h, n in itertools.product(HINTS, (M.Counts(0, 0, 0, B), M.Counts(128, 16, 128, B))):
        assert lib_next(hc, h, M.NO_MASK, n) == h
