"""Lazy dense DE rounds (UT_LAZY_HASH, api.hip score_round_de_impl): hashing and
deduplicating only the score-sorted prefix of K' >= 2k candidates must select
exactly what the eager round -- every candidate hashed, duplicates masked
before the top-k -- selects: indices, scores, digests and value rows, bit for
bit, with and without history hits inside the prefix, through the on-device
fallback, and at the edges of the policy.

The premise is that equal configurations get bitwise-equal scores wherever
they sit in the batch; test_scores_do_not_depend_on_position checks it for
every precision.

Shapes: m = 6000 (no multiple of 2048 or 128), n = 130 training rows, k = 64
(K' = 128) unless a case says otherwise.
"""
import itertools

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from _spaces import to_manip  # noqa: E402
from oracle.space import BOOL, ENUM, FLOAT, INT, Param  # noqa: E402

M, N, K = 6000, 130, 64


def r64_space():
    return [Param("x%d" % i, FLOAT, -1000.0, 1000.0) for i in range(64)]


def disc_space():
    """8 * 8 * 2 * 3 = 384 configurations: in-batch duplicates are the rule"""
    return [Param("a", INT, 0, 7), Param("b", INT, 0, 7), Param("f", BOOL), Param("e", ENUM, options=["p", "q", "r"])]


SPACES = {"r64": (r64_space, 2.0), "disc": (disc_space, 0.7)}


def make_engine(space_name, prec, seed=11, npop=512):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from uptune_amd.engine import BatchEngine
    mk, ell = SPACES[space_name]
    e = BatchEngine(to_manip(mk()), device=0, seed=seed)
    e.population_init(npop)
    pop = e.population_get()
    # distinct training rows (the discrete population repeats configurations)
    X = np.unique(e.encode(pop).T.contiguous().cpu().numpy(), axis=0)
    X = X[np.random.default_rng(3).permutation(X.shape[0])[:N]]
    assert X.shape[0] == N
    y = np.random.default_rng(5).standard_normal(N)
    e.gp_set_precision(prec)
    e.gp_fit(X, y, lengthscale=ell, sigma_f2=1.0, sigma_n2=1e-6, jitter=1e-8)
    e.history_reset(0)
    return e


def run(e, monkeypatch, lazy, m=M, k=K, round_=1):
    """one round under UT_LAZY_HASH = lazy -> (host arrays, lazy rounds, fallbacks it added)"""
    monkeypatch.setenv("UT_LAZY_HASH", "1" if lazy else "0")
    lz0, fb0 = e.round_lazy_stats()
    out = e.score_round_de(m, k, round_=round_, cr=0.2)
    lz1, fb1 = e.round_lazy_stats()
    return [t.cpu().numpy() for t in out], lz1 - lz0, fb1 - fb0


def assert_same(got, want):
    for g, w, name in zip(got, want, ("idx", "top", "dig", "vals")):
        np.testing.assert_array_equal(g, w, err_msg=name)


@pytest.mark.parametrize("prec", [64, 8])
@pytest.mark.parametrize("space_name", ["r64", "disc"])
def test_lazy_equals_eager(monkeypatch, space_name, prec):
    e = make_engine(space_name, prec)
    eager, lz, fb = run(e, monkeypatch, False)
    assert (lz, fb) == (0, 0)
    lazy, lz, fb = run(e, monkeypatch, True)
    print(f"{space_name} prec {prec}: lazy rounds +{lz}, fallbacks +{fb}, selected {(eager[0] >= 0).sum()}")
    assert lz == 1
    if space_name == "r64":
        assert fb == 0 and (eager[0] >= 0).all()
    assert_same(lazy, eager)
    # history hits inside the prefix: the eager run's first 40 selections
    e.history_add(torch.from_numpy(eager[2][:40].copy()))
    eager2, _, _ = run(e, monkeypatch, False)
    assert not set(eager2[0][eager2[0] >= 0].tolist()) & set(eager[0][:40].tolist())
    lazy2, lz, fb = run(e, monkeypatch, True)
    assert lz == 1
    if space_name == "r64":
        assert fb == 0
    assert_same(lazy2, eager2)
    e.close()


@pytest.mark.parametrize("prec", [64, 8])
def test_fallback_discrete_mostly_in_history(monkeypatch, prec):
    """k = 256 against 384 configurations, 300 of them in the history: at most
    84 selections exist, the prefix of 512 is full of candidates, so the round
    falls back and pads with -1 exactly as the eager round does"""
    e = make_engine("disc", prec)
    allv = np.array(list(itertools.product(range(8), range(8), range(2), range(3))), dtype=np.float64).T
    dig = e.hash(torch.from_numpy(np.ascontiguousarray(allv)).cuda())
    e.history_add(dig[:300].contiguous())
    eager, _, _ = run(e, monkeypatch, False, k=256)
    assert (eager[0] == -1).any() and (eager[0] >= 0).sum() <= 84
    lazy, lz, fb = run(e, monkeypatch, True, k=256)
    assert (lz, fb) == (1, 1)
    assert_same(lazy, eager)
    # the next lazy round decides for itself (few candidates: fewer copies in its prefix)
    e.history_reset(0)
    eager3, _, _ = run(e, monkeypatch, False, m=200, k=4, round_=2)
    lazy3, lz, fb = run(e, monkeypatch, True, m=200, k=4, round_=2)
    assert lz == 1 and fb in (0, 1)
    assert_same(lazy3, eager3)
    e.close()


@pytest.mark.parametrize("prec", [64, 8])
def test_fallback_whole_prefix_in_history(monkeypatch, prec):
    """R64 with the eager top-128 in the history: the whole prefix is
    duplicates.  The round after it, on a fresh history, must not fall back:
    the gate is reset by every lazy round."""
    e = make_engine("r64", prec)
    top128, _, _ = run(e, monkeypatch, False, k=128)
    e.history_add(torch.from_numpy(top128[2].copy()))
    eager, _, _ = run(e, monkeypatch, False)
    assert (eager[0] >= 0).all() and not set(eager[0].tolist()) & set(top128[0].tolist())
    lazy, lz, fb = run(e, monkeypatch, True)
    assert (lz, fb) == (1, 1)
    assert_same(lazy, eager)
    e.history_reset(0)
    eager2, _, _ = run(e, monkeypatch, False, round_=2)
    lazy2, lz, fb = run(e, monkeypatch, True, round_=2)
    assert (lz, fb) == (1, 0)
    assert_same(lazy2, eager2)
    e.close()


@pytest.mark.parametrize("m,k,is_lazy", [(M, 512, True),     # K' = 1024: the top-k kernel's limit
                                         (M, 600, False),    # K' = 2048: eager by policy
                                         (100, 64, False)])  # K' = 128 >= m: eager
def test_policy_edges(monkeypatch, m, k, is_lazy):
    e = make_engine("r64", 64)
    eager, _, _ = run(e, monkeypatch, False, m=m, k=k)
    lazy, lz, fb = run(e, monkeypatch, True, m=m, k=k)
    assert lz == (1 if is_lazy else 0) and fb == 0
    assert_same(lazy, eager)
    e.close()


# ---------------------------------------------------------------- the premise
M4 = 3 * 2048 + 77


def copy_pairs():
    """50 (source, copy) column pairs: crafted ones across the 64-, 128- and
    2048-wide tiles and into the last partial tile, the rest scattered"""
    pairs = [(5, 5 + 64), (7, 7 + 128), (9, 9 + 2048), (6143, M4 - 1), (6200, 3), (2047, 2048), (127, 4096 + 200)]
    used = {p for pr in pairs for p in pr}
    rng = np.random.default_rng(17)
    rest = [int(p) for p in rng.permutation(M4) if int(p) not in used][:2 * (50 - len(pairs))]
    pairs += list(zip(rest[0::2], rest[1::2]))
    assert len(pairs) == 50 and len({p for pr in pairs for p in pr}) == 100
    return pairs


@pytest.fixture(scope="module")
def candidates():
    vals = np.random.default_rng(23).uniform(-1000.0, 1000.0, size=(64, M4))
    pairs = copy_pairs()
    for src, dst in pairs:
        vals[:, dst] = vals[:, src]
    return vals, pairs


@pytest.mark.parametrize("prec", [64, 32, 16, 8])
@pytest.mark.parametrize("n", [130, 1000])
def test_scores_do_not_depend_on_position(candidates, n, prec):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from uptune_amd.engine import BatchEngine
    vals, pairs = candidates
    e = BatchEngine(to_manip(r64_space()), device=0, seed=1)
    rng = np.random.default_rng(n)
    X = rng.uniform(size=(n, 64))
    y = rng.standard_normal(n)
    e.gp_set_precision(prec)
    e.gp_fit(X, y, lengthscale=2.0, sigma_f2=1.0, sigma_n2=1e-6, jitter=1e-8)
    mu, var, score = (t.cpu().numpy() for t in e.gp_score_values(torch.from_numpy(vals).cuda()))
    assert np.isfinite(score).all()
    src = np.array([p[0] for p in pairs])
    dst = np.array([p[1] for p in pairs])
    for name, a in (("mu", mu), ("var", var), ("score", score)):
        np.testing.assert_array_equal(a[dst].view(np.uint64), a[src].view(np.uint64), err_msg=f"{name} n={n} prec={prec}")
    e.close()
