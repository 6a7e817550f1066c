"""Top-k by threshold selection (topk.hip topk_select) against oracle.select:
the k largest scores, ties to the smallest global index, NaN and duplicates
never selected, -1 padding, best first.  Indices must match exactly and the
scores at the valid slots must be the input's bits.

Every input is one a selection step can go wrong on: a single key (the tie
class is everything), tie classes that straddle k and spread over every
workgroup, keys that differ only in the last digit or only in the sign, -0.0
against +0.0, infinities, denormals, NaN, masks that leave exactly k, k - 1 or
no candidates.  Each case runs on two contexts: the default one (the
tournament of sorts below the hand-over, the selection above it) and one with
UT_TOPK_SELECT=1 (the selection at every size).

The reference is computed once per input for k = 1024 and cut to each k (the
selection is a prefix of one sorted list by definition).
"""
import itertools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from _spaces import to_manip  # noqa: E402
from oracle import select as osel  # noqa: E402
from oracle.space import BOOL, ENUM, FLOAT, INT, Param  # noqa: E402

MS = [1, 255, 2047, 2048, 2049, 4097, 2 ** 16 + 3, 2 ** 17]
KS = [1, 2, 255, 256, 512, 1000, 1024]
BASES = [0, 1000, 2 ** 40]
KMAX = 1024

_ENG = {}


def engine(monkeypatch, forced):
    """one context per mode for the whole module (the mode is read at creation)"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    if forced not in _ENG:
        from uptune_amd.engine import BatchEngine
        if forced:
            monkeypatch.setenv("UT_TOPK_SELECT", "1")
        else:
            monkeypatch.delenv("UT_TOPK_SELECT", raising=False)
        _ENG[forced] = BatchEngine(to_manip([Param("x", FLOAT, 0.0, 1.0)]), device=0, seed=0)
    return _ENG[forced]


def dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).cuda()


# ---------------------------------------------------------------- the inputs
def _rng(m, salt):
    return np.random.default_rng(1000003 * salt + m)


def all_equal(m):
    return np.full(m, 0.25), None


def three_values(m):
    """the top value at 100 spread positions, the middle one at every third
    position: whatever k is, the k-th score's tie class straddles k and has
    members in every workgroup"""
    s = np.zeros(m)
    s[::3] = 1.0
    s[_rng(m, 1).permutation(m)[:100]] = 2.0
    return s, None


def sparse_ties(m):
    """the threshold value at every 50th position, everything else below it
    but for ten larger scores: at m = 2^17 the tie class (2622) does not fit
    the sort's chunk and the ties wanted (up to 1014) lie in 13 workgroups'
    segments, so a later workgroup's rank must count the earlier ones' ties"""
    r = _rng(m, 11)
    s = -1.0 - r.random(m)
    s[::50] = 0.5
    s[r.permutation(m)[:10]] = 3.0
    return s, None


def rounded_normals(m):
    return np.round(_rng(m, 2).standard_normal(m), 2), None


def increasing(m):
    return np.arange(m, dtype=np.float64) * 0.5 - 7.0, None


def decreasing(m):
    return -np.arange(m, dtype=np.float64) * 0.5 + 7.0, None


def infinities(m):
    s = _rng(m, 3).standard_normal(m)
    s[::5] = np.inf
    s[1::7] = -np.inf
    return s, None


def signed_zeros(m):
    s = np.where(_rng(m, 4).integers(0, 2, m) == 1, -0.0, 0.0)
    s[2::11] = -1.0
    return s, None


def denormals_and_negatives(m):
    r = _rng(m, 5)
    s = -np.abs(r.standard_normal(m))
    d = r.integers(1, 50, m).astype(np.uint64).view(np.float64)   # denormals, many equal
    s[::2] = np.where(r.integers(0, 2, m) == 1, d, -d)[::2]
    return s, None


def nan_every_97(m):
    s = np.round(_rng(m, 6).standard_normal(m), 1)
    s[::97] = np.nan
    return s, None


def all_nan(m):
    return np.full(m, np.nan), None


def lowest_bit(m):
    """keys that differ only in the lowest mantissa bit: the last digit pass decides"""
    b = np.full(m, np.float64(1.5).view(np.uint64), dtype=np.uint64) + _rng(m, 7).integers(0, 2, m).astype(np.uint64)
    return b.view(np.float64), None


def sign_bit(m):
    s = np.where(_rng(m, 8).integers(0, 2, m) == 1, -3.0, 3.0)
    return s, None


def dup_random(m):
    r = _rng(m, 9)
    return np.round(r.standard_normal(m), 1), (r.integers(0, 3, m) == 0).astype(np.uint8)


KINDS = {f.__name__: f for f in (all_equal, three_values, sparse_ties, rounded_normals, increasing, decreasing, infinities,
                                 signed_zeros, denormals_and_negatives, nan_every_97, all_nan, lowest_bit, sign_bit,
                                 dup_random)}


def check(e, s_d, dup_d, s, want, k, base):
    idx, top = e.topk(s_d, k, dup=dup_d, cand_base=base)
    idx2, top2 = e.topk(s_d, k, dup=dup_d, cand_base=base)
    idx, top, idx2, top2 = (t.cpu().numpy() for t in (idx, top, idx2, top2))
    assert idx.tolist() == want, (k, base)
    ok = idx >= 0
    np.testing.assert_array_equal(top[ok].view(np.uint64), s[idx[ok] - base].view(np.uint64))
    # the same call twice: identical tensors
    assert idx.tobytes() == idx2.tobytes() and top.tobytes() == top2.tobytes()


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("kind", list(KINDS))
def test_topk_matches_oracle(monkeypatch, kind, m):
    s, dup = KINDS[kind](m)
    s = np.ascontiguousarray(s, dtype=np.float64)
    ref = osel.topk(s.tolist(), KMAX, dup=None if dup is None else dup.tolist())
    s_d, dup_d = dev(s), None if dup is None else dev(dup)
    for forced in (False, True):
        e = engine(monkeypatch, forced)
        for k, base in itertools.product(KS, BASES):
            want = [base + i if i >= 0 else -1 for i in ref[:k]]
            check(e, s_d, dup_d, s, want, k, base)
    if kind == "all_equal":     # the headline's case, spelled out
        assert ref[:min(m, KMAX)] == list(range(min(m, KMAX)))


@pytest.mark.parametrize("m", MS)
@pytest.mark.parametrize("left", ["k", "k-1", "0"])
def test_dup_mask_leaves_few(monkeypatch, left, m):
    """the mask leaves exactly k, k - 1 or no candidates (m < k: as many as there are)"""
    r = _rng(m, 10)
    s = np.round(r.standard_normal(m), 1)
    s_d = dev(s)
    perm = r.permutation(m)
    for k in KS:
        n = {"k": k, "k-1": k - 1, "0": 0}[left]
        dup = np.ones(m, np.uint8)
        dup[perm[:n]] = 0
        want0 = osel.topk(s.tolist(), k, dup=dup.tolist())
        assert sum(i >= 0 for i in want0) == min(n, m)
        dup_d = dev(dup)
        for forced in (False, True):
            e = engine(monkeypatch, forced)
            for base in BASES:
                check(e, s_d, dup_d, s, [base + i if i >= 0 else -1 for i in want0], k, base)


# ---------------------------------------------------------------- whole rounds
def r64_space():
    return [Param("x%d" % i, FLOAT, -1000.0, 1000.0) for i in range(64)]


def disc_space():
    """8 * 8 * 2 * 3 = 384 configurations: in-batch duplicates are the rule"""
    return [Param("a", INT, 0, 7), Param("b", INT, 0, 7), Param("f", BOOL), Param("e", ENUM, options=["p", "q", "r"])]


def round_engine(monkeypatch, space, ell, forced, n=130):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from uptune_amd.engine import BatchEngine
    if forced:
        monkeypatch.setenv("UT_TOPK_SELECT", "1")
    else:
        monkeypatch.delenv("UT_TOPK_SELECT", raising=False)
    e = BatchEngine(to_manip(space), device=0, seed=11)
    e.population_init(512)
    X = np.unique(e.encode(e.population_get()).T.contiguous().cpu().numpy(), axis=0)
    X = X[np.random.default_rng(3).permutation(X.shape[0])[:n]]
    y = np.random.default_rng(5).standard_normal(n)
    e.gp_set_precision(8)
    e.gp_fit(X, y, lengthscale=ell, sigma_f2=1.0, sigma_n2=1e-6, jitter=1e-8)
    e.history_reset(0)
    return e


def one_round(e, monkeypatch, lazy, m, k):
    if lazy:
        monkeypatch.delenv("UT_LAZY_HASH", raising=False)
    else:
        monkeypatch.setenv("UT_LAZY_HASH", "0")
    lz0, fb0 = e.round_lazy_stats()
    out = [t.cpu().numpy() for t in e.score_round_de(m, k, round_=1, cr=0.2)]
    lz1, fb1 = e.round_lazy_stats()
    return out, lz1 - lz0, fb1 - fb0


@pytest.mark.parametrize("forced", [False, True])
def test_round_lazy_equals_eager(monkeypatch, forced):
    """m = 4096, k = 256: (indices, scores, digests) with UT_LAZY_HASH=0 and with the default"""
    e = round_engine(monkeypatch, r64_space(), 2.0, forced)
    eager, lz, _ = one_round(e, monkeypatch, False, 4096, 256)
    assert lz == 0
    lazy, lz, fb = one_round(e, monkeypatch, True, 4096, 256)
    assert (lz, fb) == (1, 0)
    for g, w, name in zip(lazy, eager, ("idx", "top", "dig", "vals")):
        np.testing.assert_array_equal(g, w, err_msg=name)
    e.close()


def test_round_fallback_prefix_mostly_in_history(monkeypatch):
    """k = 256 against 384 configurations, 300 of them in the history, m =
    10000: the prefix's top-512 comes from the selection (the tournament would
    need three launches there), the round falls back (the gated remainder
    keeps the tournament, as the eager round's top-256 of five chunks does)
    and pads with -1 exactly as the eager round does"""
    e = round_engine(monkeypatch, disc_space(), 0.7, False)
    allv = np.array(list(itertools.product(range(8), range(8), range(2), range(3))), dtype=np.float64).T
    dig = e.hash(dev(allv))
    e.history_add(dig[:300].contiguous())
    eager, _, _ = one_round(e, monkeypatch, False, 10000, 256)
    assert (eager[0] == -1).any() and (eager[0] >= 0).sum() <= 84
    lazy, lz, fb = one_round(e, monkeypatch, True, 10000, 256)
    assert (lz, fb) == (1, 1)
    for g, w, name in zip(lazy, eager, ("idx", "top", "dig", "vals")):
        np.testing.assert_array_equal(g, w, err_msg=name)
    e.close()
