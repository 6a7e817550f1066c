"""The device build of repr(float) / repr(int) (csrc/ut_core.h as hipcc
compiles it for gfx950, and the LDS byte emitter, column zeroing, 0x80 pad and
length word of repr_digest in csrc/hash.hip) against CPython, bit for bit.

Every digest is compared with oracle.hashing.hash_config (hashlib over
CPython's repr).  The float values are tests/_repr_cases.py's table(): every
branch of d2d and every layout of repr_double at least eight times
(tests/test_repr_cases_cpu.py counts them, and checks the host build of the
same source on the same values).  The cases reach every kernel that calls
repr_digest or reads what it wrote:

  a  k_inner_all + k_hash<true>     small m (<= HASH_SMALL_M), ragged m too
  b  k_hash<false>                  m > HASH_SMALL_M
  c  three strings per lane: the longest, then the shortest, then any
     (the zeroing of the lane's LDS column, W[15], the pad after len)
  d  capped grids: a workgroup's LDS columns reused across grid strides
  e  k_pop_digests (rebuild and patch), k_de_diff, k_inner_pairs; -0.0 / NaN bits
  f  ut_hash_parent
  g  repr_int64 under HM_INT        h  repr_double(py_log2) under HM_LOGINT
  i  k_inner_all past its grid cap (grid-stride reuse of its LDS columns)

No tolerances.  Needs a GPU."""
import hashlib
import os

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

import _repr_cases as rc  # noqa: E402
from oracle import hashing as oh  # noqa: E402
from oracle.space import FLOAT, INT, LOGINT, Param, from_f64  # noqa: E402

HASH_SMALL_M = 16384      # csrc/hash.hip: up to this m ut_hash takes the k_inner_all path
ROLL = 37                 # each repeat of a tiled table is rolled by this much more

S1 = [Param("x", FLOAT, 0.0, 1.0)]   # (ut_hash does not clamp: the range plays no part)
S3 = [Param("a", FLOAT, 0.0, 1.0), Param("b", FLOAT, 0.0, 1.0), Param("c", FLOAT, 0.0, 1.0)]
SINT = [Param("n", INT, -(2 ** 53 - 1), 2 ** 53 - 1), Param("f", FLOAT, 0.0, 1.0)]
SLOG = [Param("big_log", LOGINT, 0, (1 << 31) - 1), Param("f", FLOAT, 0.0, 1.0)]   # test_logint_large_range_bit_exact's
SWIDE = [Param("p%02d" % k, FLOAT, 0.0, 1.0) for k in range(20)]

_ENGINES = {}
_MEMO = {}


def _engine(key, space):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    if key not in _ENGINES:
        from _spaces import to_manip
        from uptune_amd.engine import BatchEngine
        _ENGINES[key] = BatchEngine(to_manip(space), device=0, seed=0)
    return _ENGINES[key]


def _hex(d):
    from uptune_amd.engine import digests_to_hex
    return digests_to_hex(d)


def _dev(a):
    # into a fresh device tensor: its stride(0) is the row length, which a numpy view with a
    # length-1 axis (t[None, :]) does not promise
    a = np.ascontiguousarray(a, dtype=np.float64)
    out = torch.empty(a.shape, dtype=torch.float64, device="cuda")
    out.copy_(torch.from_numpy(a))
    assert out.stride(0) == a.shape[1]
    return out


def _f64(xs):
    """doubles -> float64 array by their bit patterns (NaN payloads kept)"""
    return np.array([rc.bits_of(float(x)) for x in xs], dtype=np.uint64).view(np.float64)


def _oracle(space, vals):
    return [oh.hash_config(space, [from_f64(p, vals[i, j]) for i, p in enumerate(space)])
            for j in range(vals.shape[1])]


def _tile(vals, m):
    """[ncols][T] -> [ncols][m]: repeats of the candidates, repeat r rolled by ROLL * r, so a
    lane does not see the same value twice; returns the source candidate of each column too"""
    T = vals.shape[1]
    src = np.concatenate([np.roll(np.arange(T), ROLL * r) for r in range((m + T - 1) // T)])[:m]
    return np.ascontiguousarray(vals[:, src]), src


def _above_small_m(T):
    return (HASH_SMALL_M // T + 1) * T    # the next multiple of the table length above HASH_SMALL_M


# ---- shared values and references (each computed once) ------------------------------------
def _table():
    if "table" not in _MEMO:
        _MEMO["table"] = _f64(rc.table())
    return _MEMO["table"]


def _want1():
    """oracle digests of the one-parameter space over the table"""
    if "want1" not in _MEMO:
        _MEMO["want1"] = _oracle(S1, _table()[None, :])
    return _MEMO["want1"]


def _cols3():
    """case (c)'s candidates: column 0 the table by len(repr) descending, column 1 that order
    reversed, column 2 the shuffled table; and their oracle digests"""
    if "cols3" not in _MEMO:
        t = _table()
        order = np.array(sorted(range(t.size), key=lambda j: -len(repr(float(t[j])))))
        vals = np.stack([t[order], t[order][::-1], t])
        _MEMO["cols3"] = (vals, _oracle(S3, vals))
    return _MEMO["cols3"]


# ---- failure reports -----------------------------------------------------------------------
def _check_single(vals, got, want):
    """one FLOAT parameter: name the first differing values"""
    bad = [j for j in range(len(want)) if got[j] != want[j]]
    if bad:
        distinct = sorted({rc.bits_of(float(vals[j])) for j in bad})
        lines = ["%s  repr %s  tags %s" % (float(vals[j]).hex(), repr(float(vals[j])),
                                           sorted(rc.classify(float(vals[j])).tags)) for j in bad[:8]]
        pytest.fail("%d of %d digests differ (%d distinct values); first:\n  %s"
                    % (len(bad), len(want), len(distinct), "\n  ".join(lines)))


def _check_multi(vals, got, want):
    """several columns: a digest does not isolate one value; name the candidates"""
    bad = [j for j in range(len(want)) if got[j] != want[j]]
    if bad:
        lines = ["candidate %d: %s" % (j, [repr(float(v)) for v in vals[:, j]]) for j in bad[:8]]
        pytest.fail("%d of %d digests differ; first:\n  %s" % (len(bad), len(want), "\n  ".join(lines)))


# ---- a. small-m path -----------------------------------------------------------------------
def test_a_small_m_table():
    e = _engine("s1", S1)
    t = _table()
    assert t.size <= HASH_SMALL_M
    got = _hex(e.hash(_dev(t[None, :])))
    _MEMO["got1"] = got
    _check_single(t, got, _want1())


@pytest.mark.parametrize("m", [1, 127, 129])
def test_a_small_m_ragged(m):
    e = _engine("s1", S1)
    t = _table()[:m]
    _check_single(t, _hex(e.hash(_dev(t[None, :]))), _want1()[:m])


# ---- b. direct path ------------------------------------------------------------------------
def test_b_direct_path_table():
    e = _engine("s1", S1)
    t = _table()
    m = _above_small_m(t.size)
    assert m > HASH_SMALL_M and m % t.size == 0
    vals, src = _tile(t[None, :], m)
    got = _hex(e.hash(_dev(vals)))
    _check_single(vals[0], got, [_want1()[j] for j in src])
    small = _MEMO.get("got1") or _hex(e.hash(_dev(t[None, :])))
    assert got == [small[j] for j in src], "k_hash<false> and k_inner_all + k_hash<true> disagree"


# ---- c. one lane, several strings ----------------------------------------------------------
def test_c_three_strings_per_lane_small_m():
    e = _engine("s3", S3)
    vals, want = _cols3()
    lens = [len(repr(float(v))) for v in vals[:2, 0]]
    assert lens[0] == 24 and lens[1] == 3     # a lane formats the longest string, then the shortest
    assert vals.shape[1] <= HASH_SMALL_M
    _check_multi(vals, _hex(e.hash(_dev(vals))), want)


def test_c_three_strings_per_lane_direct():
    e = _engine("s3", S3)
    base, want = _cols3()
    m = _above_small_m(base.shape[1])
    assert m > HASH_SMALL_M
    vals, src = _tile(base, m)
    _check_multi(vals, _hex(e.hash(_dev(vals))), [want[j] for j in src])


# ---- d. grid-stride reuse of the LDS column ------------------------------------------------
def test_d_capped_grid_reuses_lds_columns():
    """one workgroup per CU (UT_HASH_WG_PER_CU=1) and three more blocks of candidates than
    CUs: some workgroups format a second block of strings over the first one's bytes.
    k_hash<false> through ut_hash, k_inner_pairs through ut_hash_de"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from _spaces import to_manip
    from uptune_amd.engine import BatchEngine
    base, want = _cols3()
    T = base.shape[1]
    m = 128 * (torch.cuda.get_device_properties(0).multi_processor_count + 3)
    assert m > HASH_SMALL_M
    vals, src = _tile(base, m)
    dv = _dev(vals)
    pop = _dev(np.ascontiguousarray(vals[:, ::-1][:, :1024]))    # unrelated targets: every pair is computed
    old = os.environ.get("UT_HASH_WG_PER_CU")
    try:
        os.environ["UT_HASH_WG_PER_CU"] = "1"
        e = BatchEngine(to_manip(S3), device=0, seed=0)
        capped = e.hash(dv).cpu()
        e.population_set(pop)
        capped_de = e.hash_de(dv, 0).cpu()
        e.close()
    finally:
        if old is None:
            os.environ.pop("UT_HASH_WG_PER_CU", None)
        else:
            os.environ["UT_HASH_WG_PER_CU"] = old
    full = _engine("s3", S3).hash(dv).cpu()
    n = min(T, m)
    _check_multi(vals[:, :n], _hex(capped[:n]), [want[j] for j in src[:n]])
    assert torch.equal(capped, full), "capped ut_hash differs from the full grid's"
    assert torch.equal(capped_de, full), "capped ut_hash_de differs from ut_hash"


# ---- e. population cache -------------------------------------------------------------------
def test_e_population_cache_paths():
    e = _engine("s3", S3)
    base, want = _cols3()
    T, npop = base.shape[1], 1024
    pop = np.ascontiguousarray(base[:, :npop])
    e.population_set(_dev(pop))

    def check(vals, ref):
        d = _dev(vals)
        _check_multi(vals, _hex(e.hash_de(d, 0)), ref)
        _check_multi(vals, _hex(e.hash(d)), ref)

    # 1. the population itself: every digest comes from the cache (k_pop_digests)
    check(pop, want[:npop])
    # 2. every odd candidate's column 1 is the column's next value: pairs and cache mixed
    mixed = pop.copy()
    odd = np.arange(1, npop, 2)
    mixed[1, odd] = base[1, odd + 1]
    assert (mixed[1, odd].view(np.uint64) != pop[1, odd].view(np.uint64)).all()
    check(mixed, _oracle(S3, mixed))
    # 3. four members replaced by candidates not in the population: the patch path
    rows = np.array([0, 5, 1000, 1023])
    new = np.ascontiguousarray(base[:, T - 4:T])
    e.population_replace(_dev(new), torch.from_numpy(rows).cuda())
    pop2 = pop.copy()
    pop2[:, rows] = new
    np.testing.assert_array_equal(e.population_get().cpu().numpy().view(np.uint64), pop2.view(np.uint64))
    ref2 = list(want[:npop])
    for k, r in enumerate(rows):
        ref2[r] = want[T - 4 + k]
    check(pop2, ref2)


def test_e_zero_sign_and_nan_payload_are_bits():
    """k_de_diff compares bits: -0.0 must not inherit the digest of a target's 0.0 ("-0.0" is
    another string), and a NaN of another payload is recomputed to the same "nan\""""
    e = _engine("s3", S3)
    base, _ = _cols3()
    n = 128
    pop = np.ascontiguousarray(base[:, :n])
    pop[0, :64] = 0.0
    pop[0, 64:] = _f64([rc.NAN_A])[0]
    trial = pop.copy()
    trial[0, :64] = -0.0
    trial[0, 64:] = _f64([rc.NAN_B])[0]
    assert (trial[0].view(np.uint64) != pop[0].view(np.uint64)).all()
    e.population_set(_dev(pop))
    want_pop, want_trial = _oracle(S3, pop), _oracle(S3, trial)
    assert want_pop[:64] != want_trial[:64] and want_pop[64:] == want_trial[64:]
    _check_multi(pop, _hex(e.hash_de(_dev(pop), 0)), want_pop)
    _check_multi(trial, _hex(e.hash_de(_dev(trial), 0)), want_trial)
    _check_multi(trial, _hex(e.hash(_dev(trial))), want_trial)


# ---- f. parent path ------------------------------------------------------------------------
def test_f_parent_path():
    e = _engine("s3", S3)
    base, _ = _cols3()
    t = _table()
    long24 = next(float(x) for x in t if len(repr(float(x))) == 24)
    subn = next(float(x) for x in t if "subnormal" in rc.classify(float(x)).tags)
    parent = np.array([long24, -0.0, subn])
    rng = np.random.default_rng(rc.SEED)
    m = 512
    children = np.ascontiguousarray(base[:, 2000:2000 + m])
    keep = rng.uniform(size=(3, m)) < 0.5
    children = np.where(keep, parent[:, None], children)
    assert keep.all(axis=0).any() and (~keep).all(axis=0).any()   # a copy of the parent; a child sharing nothing
    want = _oracle(S3, children)
    d = _dev(children)
    _check_multi(children, _hex(e.hash_parent(d, parent)), want)
    _check_multi(children, _hex(e.hash(d)), want)


# ---- g. wide INT ---------------------------------------------------------------------------
def test_g_wide_int():
    e = _engine("sint", SINT)
    assert not e.spec.params[0].lut     # the range exceeds INT_LUT_MAX: repr_int64 on the device
    ints = rc.int_cases()
    t = _table()
    vals = np.stack([np.array(ints, dtype=np.float64), np.resize(t, len(ints))])
    assert [int(v) for v in vals[0]] == ints
    want = _oracle(SINT, vals)
    d = _dev(vals)
    assert vals.shape[1] <= HASH_SMALL_M
    _check_multi(vals, _hex(e.hash(d)), want)
    e.population_set(_dev(np.ascontiguousarray(vals[:, :256])))
    _check_multi(vals, _hex(e.hash_de(d, 0)), want)
    # and k_hash<false>'s own HM_INT branch
    big, src = _tile(vals, _above_small_m(vals.shape[1]))
    assert big.shape[1] > HASH_SMALL_M
    _check_multi(big, _hex(e.hash(_dev(big))), [want[j] for j in src])


# ---- h. wide LOGINT ------------------------------------------------------------------------
def test_h_wide_logint():
    e = _engine("slog", SLOG)
    assert e.spec.params[0].vtab is None and not e.spec.params[0].lut
    vs = rc.logint_cases()
    vals = np.stack([np.array(vs, dtype=np.float64), np.resize(_table(), len(vs))])
    want = _oracle(SLOG, vals)
    _check_multi(vals, _hex(e.hash(_dev(vals))), want)
    big, src = _tile(vals, _above_small_m(vals.shape[1]))
    _check_multi(big, _hex(e.hash(_dev(big))), [want[j] for j in src])


# ---- i. k_inner_all past its grid cap ------------------------------------------------------
def test_i_inner_all_grid_stride():
    """20 FLOAT parameters at m = HASH_SMALL_M: 327 680 (parameter, candidate) pairs, more
    than k_inner_all's grid of 8 workgroups per CU covers in one pass on any part with fewer
    than 320 CUs, so its workgroups format further strings over their first ones"""
    e = _engine("swide", SWIDE)
    t = _table()
    m = HASH_SMALL_M
    assert 20 * m > 8 * 128 * torch.cuda.get_device_properties(0).multi_processor_count
    col, src = _tile(t[None, :], m)
    vals = np.stack([np.roll(col[0], 611 * k) for k in range(20)])
    srcs = np.stack([np.roll(src, 611 * k) for k in range(20)])
    # hash_config with each table value's inner string (oracle.hashing.hash_value) computed once
    inner = [str(oh.hash_value(S1[0], float(x))) for x in t]
    names = [p.name for p in SWIDE]          # already in hash_config's sorted order
    want = [hashlib.sha256("".join(names[i] + inner[srcs[i, j]] + str(i) + "|" for i in range(20)).encode())
            .hexdigest() for j in range(m)]
    for j in (0, 1, m - 1):                  # ... which is hash_config
        assert want[j] == oh.hash_config(SWIDE, [float(v) for v in vals[:, j]])
    _check_multi(vals, _hex(e.hash(_dev(vals))), want)
