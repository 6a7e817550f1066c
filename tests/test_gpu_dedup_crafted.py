"""Dedup and the history table (csrc/dedup.hip, the history calls of
csrc/api.hip) on digests that SHA-256 never gives them: digests that differ in
one bit of one word, hundreds of digests with one home slot, probe chains that
wrap from the last slot to slot 0, digests both in the history and repeated in
the batch, a history grown twice, a small batch after a large one, and device
allocations that fail.  Every mask is compared with oracle.select.dedup for
equality.  Needs a GPU.

The only fact about the tables used here: capacities are powers of two >= 1024
and the home slot is word 0 & (capacity - 1), so word 0 = 0xFFFFFFFF lands in
the last slot of any table and word 0 = 0 in slot 0."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from oracle import select as osel  # noqa: E402

ONES = 0xFFFFFFFF


def _engine():
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from uptune_amd.engine import BatchEngine
    from uptune_amd.manipulator import ConfigurationManipulator, IntegerParameter
    return BatchEngine(ConfigurationManipulator([IntegerParameter("x", 0, 9)]))


def _rand(rng, n):
    return rng.integers(0, 1 << 32, size=(n, 8), dtype=np.uint32)


def _dev(a):
    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.uint32).view(np.int32)).cuda()


def _hex(a):
    from uptune_amd.engine import digests_to_hex
    return digests_to_hex(np.ascontiguousarray(a, dtype=np.uint32).reshape(-1, 8))


def _got(e, batch):
    return e.dedup(_dev(batch)).cpu().numpy().tolist()


def _want(batch, history=()):
    hist = set()
    for h in history:
        hist |= set(_hex(h))
    return osel.dedup(_hex(batch), hist)


def _scatter(rng, groups, m):
    """batch [m][8]: every (digest, copies) of `groups` at random places, random digests elsewhere;
    -> batch, {group index: sorted positions}"""
    batch = _rand(rng, m)
    total = sum(c for _, c in groups)
    pos = rng.permutation(m)[:total]
    where, k = {}, 0
    for g, (d, copies) in enumerate(groups):
        where[g] = sorted(int(p) for p in pos[k:k + copies])
        batch[where[g]] = d
        k += copies
    return batch, where


# --------------------------------------------------------------------------- A. crafted digests
def _one_bit_neighbours(rng):
    base = _rand(rng, 1)[0]
    out = [base]
    for w in range(8):
        for bit in (0, 31):
            d = base.copy()
            d[w] ^= np.uint32(1 << bit)
            out.append(d)
    out.append(np.zeros(8, np.uint32))
    out.append(np.full(8, ONES, np.uint32))
    return out


def test_every_word_is_compared():
    rng = np.random.default_rng(1)
    digs = _one_bit_neighbours(rng)
    assert len({d.tobytes() for d in digs}) == 19
    groups = [(d, 2 + (g % 2)) for g, d in enumerate(digs)]
    batch, where = _scatter(rng, groups, 3000)
    # the repeats span workgroups of 256, and some first occurrence is outside block 0
    assert any(p[0] // 256 != p[-1] // 256 for p in where.values())
    assert any(p[0] >= 256 for p in where.values())
    e = _engine()
    e.history_reset(0)
    want = _want(batch)
    assert sum(want) == sum(c - 1 for _, c in groups)
    assert _got(e, batch) == want
    # only the base digest is in the history: its one-bit neighbours are not seen
    e.history_add(digs[0].reshape(1, 8))
    want_h = _want(batch, [digs[0]])
    assert sum(want_h) == sum(want) + 1
    assert _got(e, batch) == want_h
    # and every neighbour in the history, the base not
    e.history_reset(0)
    e.history_add(_dev(np.stack(digs[1:])))
    assert _got(e, batch) == _want(batch, [np.stack(digs[1:])])


def test_one_home_slot():
    """600 digests that differ only in word 7: one probe chain of 600 slots"""
    rng = np.random.default_rng(2)
    base = _rand(rng, 1)[0]
    base[0] = 0x5A5A0100
    chain = np.tile(base, (600, 1))
    chain[:, 7] = rng.permutation(1 << 16)[:600].astype(np.uint32) * np.uint32(65537)
    assert len({r.tobytes() for r in chain}) == 600
    batch = np.concatenate([chain, chain[rng.integers(0, 600, size=200)]])
    batch = batch[rng.permutation(800)]
    e = _engine()
    e.history_reset(0)
    want = _want(batch)
    assert sum(want) == 200
    assert _got(e, batch) == want
    # the same chain in the history table: every third digest added, all probed
    e.history_add(chain[::3])
    assert _got(e, batch) == _want(batch, [chain[::3]])


def _wrap_digests(rng):
    last = _rand(rng, 64)
    last[:, 0] = ONES                                   # home = the last slot of any table
    low = _rand(rng, 32)
    low[:, 0] = np.repeat(np.arange(16, dtype=np.uint32), 2)   # home slots 0..15, displaced by the wrapped chain
    return last, low


def test_probe_chain_wraps_in_the_batch_table():
    rng = np.random.default_rng(3)
    last, low = _wrap_digests(rng)
    batch = np.concatenate([last, low, last[rng.integers(0, 64, size=24)], low[rng.integers(0, 32, size=16)]])
    batch = batch[rng.permutation(batch.shape[0])]
    e = _engine()
    e.history_reset(0)
    want = _want(batch)
    assert sum(want) == 40
    assert _got(e, batch) == want


def test_probe_chain_wraps_in_the_history_table():
    rng = np.random.default_rng(4)
    last, low = _wrap_digests(rng)
    hist = np.concatenate([last[::2], low[::2]])
    probe = np.concatenate([last, low, last[:5], low[:5]])
    probe = probe[rng.permutation(probe.shape[0])]
    want = _want(probe, [hist])
    assert sum(want) == 48 + 10         # the history's 48 wherever they stand, and one of each repeated pair
    for form in (_dev, np.ascontiguousarray):
        e = _engine()
        e.history_reset(0)
        e.history_add(form(hist))
        assert _got(e, probe) == want
        # grown (and so rehashed) with digests of the same two kinds, the chain wraps in the bigger table too
        more = np.concatenate([last[1::2], low[1::4], _rand(rng, 600)])
        e.history_add(form(more))
        assert _got(e, probe) == _want(probe, [hist, more])


def test_in_history_and_repeated_in_batch():
    rng = np.random.default_rng(5)
    a, b = _rand(rng, 2)
    a7, b7 = a.copy(), b.copy()         # neighbours in word 7 only: never seen, never repeated
    a7[7] ^= np.uint32(1)
    b7[7] ^= np.uint32(0x80000000)
    batch, where = _scatter(rng, [(a, 3), (b, 3), (a7, 1), (b7, 1)], 700)
    e = _engine()
    e.history_reset(0)
    e.history_add(a.reshape(1, 8))
    got = _got(e, batch)
    assert [i for i, v in enumerate(got) if v] == sorted(where[0] + where[1][1:])
    assert got == _want(batch, [a])


def test_history_growth_is_exact():
    rng = np.random.default_rng(6)
    pool = _rand(rng, 300 + 150 + 50 + 1500 + 6000)
    a1 = pool[:300]
    twice = pool[450:500]
    a2 = np.concatenate([pool[300:450], a1[100:150], twice, twice])[rng.permutation(300)]
    a3 = pool[500:2000]
    a4 = pool[2000:]
    near = pool[::3].copy()                      # a third of the added digests get a near-miss that is never
    near[:, 5] ^= np.uint32(1) << rng.integers(0, 32, size=near.shape[0]).astype(np.uint32)   # added: word 5 differs
    e = _engine()
    e.history_reset(0)
    added = []
    for k, part in enumerate((a1, a2, a3, a4)):
        assert part.shape[0] == (300, 300, 1500, 6000)[k]
        e.history_add(_dev(part) if k % 2 == 0 else np.ascontiguousarray(part))
        added.append(part)
        probe = np.concatenate(added + [near, near[:20]])
        probe = probe[rng.permutation(probe.shape[0])]
        want = _want(probe, added)
        assert _got(e, probe) == want, "after add %d" % k
    assert sum(want) == 300 + 300 + 1500 + 6000 + 20
    e.history_reset(10)
    assert _got(e, probe) == _want(probe)


def test_small_batch_after_a_large_one():
    rng = np.random.default_rng(7)
    hist = _rand(rng, 40)
    e = _engine()
    e.history_reset(0)
    e.history_add(hist)
    for m in (5000, 10, 1100):
        fresh = _rand(rng, m)
        batch = fresh.copy()
        batch[m // 2:m // 2 + m // 5] = fresh[:m // 5]      # in-batch repeats
        batch[m - 3:] = hist[:3]                              # and three from the history
        want = _want(batch, [hist])
        assert sum(want) == m // 5 + 3
        assert _got(e, batch) == want, "m = %d" % m


# --------------------------------------------------------------------------- B. failed allocations
INJECTED = "injected failure"


def _inject(e, skip, count):
    """the next `skip` counted allocations succeed, the `count` after them fail; count 0 clears"""
    from uptune_amd import _lib as L
    L.check(e.ctx, e.lib.ut_debug_fail_alloc_after(e.ctx, skip, count), "ut_debug_fail_alloc_after")


def _fails_injected(e, skip, call):
    """`call` raises with the injected allocation failure after `skip` allocations of its own succeeded"""
    from uptune_amd import _lib as L
    _inject(e, skip, 1)
    try:
        with pytest.raises(L.UthotError, match=INJECTED):
            call()
    finally:
        _inject(e, 0, 0)


def _held(e):
    """device bytes the library holds now; engines of earlier tests are collected first"""
    import gc
    gc.collect()
    return e.device_bytes()


def _history_case(seed):
    rng = np.random.default_rng(seed)
    h0, h1 = _rand(rng, 400), _rand(rng, 300)     # 400 fit a 1024-slot table, 700 do not
    near = h0[::4].copy()
    near[:, 7] ^= np.uint32(0x80000000)
    probe = np.concatenate([h0, h1, near, h1[:10], near[:10]])
    return h0, h1, probe[rng.permutation(probe.shape[0])]


# a history call allocates two arrays, the keys and then the slot states: skip = 0 fails
# the first, skip = 1 lets the keys through and fails the second (the keys are given back)
ARRAYS = pytest.mark.parametrize("skip", [0, 1], ids=["keys", "state"])


@pytest.mark.parametrize("form", ["device", "host"])
@ARRAYS
def test_failed_history_growth_keeps_the_old_history(skip, form):
    h0, h1, probe = _history_case(10 + skip)
    conv = _dev if form == "device" else np.ascontiguousarray
    e = _engine()
    e.history_reset(0)
    e.history_add(conv(h0))
    assert _got(e, probe) == _want(probe, [h0])
    held = _held(e)
    _fails_injected(e, skip, lambda: e.history_add(conv(h1)))
    assert e.device_bytes() == held                # nothing obtained by the failed call is kept
    assert _got(e, probe) == _want(probe, [h0])
    e.history_add(conv(h1))
    assert e.device_bytes() > held
    assert _got(e, probe) == _want(probe, [h0, h1])


def test_injection_skip_counts_allocations_not_calls():
    """skip = 2 is more than one growth allocates: the growth succeeds, and the injection
    stays armed for the next counted allocation (the batch table's first)"""
    h0, h1, probe = _history_case(15)
    e = _engine()
    e.history_reset(0)
    e.history_add(h0)
    _inject(e, 2, 1)
    try:
        e.history_add(h1)                          # keys and states: the two skipped
        from uptune_amd import _lib as L
        with pytest.raises(L.UthotError, match=INJECTED):
            e.dedup(_dev(probe))
    finally:
        _inject(e, 0, 0)
    assert _got(e, probe) == _want(probe, [h0, h1])


@ARRAYS
def test_failed_history_reset_leaves_an_empty_history(skip):
    h0, h1, probe = _history_case(20 + skip)
    e = _engine()
    held = _held(e)                               # no history and no batch table yet
    e.history_reset(0)
    e.history_add(h0)
    assert e.device_bytes() > held
    _fails_injected(e, skip, lambda: e.history_reset(5000))
    assert e.device_bytes() == held                # the old table is gone, nothing of the new one is kept
    assert _got(e, probe) == _want(probe)          # in-batch repeats only
    e.history_add(_dev(h1))
    assert _got(e, probe) == _want(probe, [h1])


def test_failed_batch_table_growth():
    rng = np.random.default_rng(30)
    hist = _rand(rng, 50)
    small = np.concatenate([_rand(rng, 90), hist[:10]])
    small[40:50] = small[:10]
    big = _rand(rng, 3000)
    big[2000:2500] = big[:500]
    big[2990:] = hist[10:20]
    e = _engine()
    e.history_reset(0)
    e.history_add(hist)
    held = _held(e)                                   # no batch table yet
    assert _got(e, small) == _want(small, [hist])      # the batch table has its smallest size now
    assert e.device_bytes() > held
    _fails_injected(e, 0, lambda: e.dedup(_dev(big)))  # needs a bigger one
    assert e.device_bytes() == held                    # the small one is gone, no other in its place
    assert _got(e, small) == _want(small, [hist])
    assert _got(e, big) == _want(big, [hist])
