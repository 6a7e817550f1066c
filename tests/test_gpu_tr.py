"""ut_propose_tr on the device against its numpy restatement (tests/_tr_oracle.py;
the rule is stated in include/uthot.h): values and the invalid mask bit for bit.
hpl64 and perm_mixed together hold all seven kinds, the single-point ranges
ndiv and pow2_3, the two-value pow2_2, 0..1 integers, a LOGINT beyond the host
table and permutations of 3, 10 and 40 items."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import _tr_oracle as tro  # noqa: E402
from _spaces import oracle_space, to_manip  # noqa: E402
from oracle import de as ode  # noqa: E402
from oracle.space import ENUM, FLOAT, INT, Param, columns  # noqa: E402

M, PADDING = 1000, 24           # m: not a multiple of the 256-lane block; ld = m + PADDING > m
BIG = 2 ** 32 + 5               # a candidate base whose high counter word is not zero
SEED = 23
SENTINEL = -7.25


def _engine(space, seed=SEED):
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from uptune_amd.engine import BatchEngine
    return BatchEngine(to_manip(space), device=0, seed=seed)


@pytest.fixture(scope="module")
def setups():
    from uptune_amd import spaces
    out = {}
    for name, manip in (("hpl64", spaces.hpl64()), ("perm_mixed", spaces.perm_mixed())):
        space = oracle_space(manip)
        out[name] = (space, _engine(space), ode.population_init(space, 4, seed=5)[:, 1].copy())
    return out


def call(e, centre, half, prob, cat_prob, round_, base, m, must=1, ld=None, raw=False):
    """ut_propose_tr through the C ABI with ld > m -> (rc, values [ncols][m], invalid [m], whole out buffer)"""
    from uptune_amd import _lib as L
    ld = m + PADDING if ld is None else ld
    out = torch.full((e.spec.ncols, max(ld, 1)), SENTINEL, dtype=torch.float64, device=e.device)
    inv = torch.full((max(m, 1),), 9, dtype=torch.uint8, device=e.device)
    c = None if centre is None else torch.from_numpy(np.ascontiguousarray(centre, dtype=np.float64)).to(e.device)
    h = np.ascontiguousarray(half, dtype=np.float64)
    a = L.TrParams(prob=prob, cat_prob=cat_prob, must=must)
    rc = e.lib.ut_propose_tr(e.ctx, C.byref(a), None if c is None else C.c_void_p(c.data_ptr()),
                             C.c_void_p(h.ctypes.data), round_, base, m, C.c_void_p(out.data_ptr()), ld,
                             C.c_void_p(inv.data_ptr()))
    e.sync()
    o, i = out.cpu().numpy(), inv.cpu().numpy()
    if raw:
        return rc, o, i
    assert rc == 0, e.lib.ut_last_error(e.ctx)
    assert (o[:, m:] == SENTINEL).all()          # nothing is written past column m
    return o[:, :m], i[:m].astype(bool)


def check(space, e, centre, half, prob, cat_prob, round_, base, m=M, must=1):
    got, ginv = call(e, centre, half, prob, cat_prob, round_, base, m, must=must)
    want, winv, _ = tro.propose_tr_vec(space, centre, half, prob, cat_prob, e.seed, round_, base, m, must=must)
    np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))
    np.testing.assert_array_equal(ginv, winv)
    return got, ginv


@pytest.mark.parametrize("name", ["hpl64", "perm_mixed"])
@pytest.mark.parametrize("L", [1.6, 0.8, 2.0 ** -7])
@pytest.mark.parametrize("prob,cat_prob", [(0.0, 0.0), (0.3, 1.0), (1.0, 0.0), (1.0, 1.0)])
def test_matches_the_restatement(setups, name, L, prob, cat_prob):
    space, e, centre = setups[name]
    got, inv = check(space, e, centre, np.full(len(space), L / 2.0), prob, cat_prob, 3, 11)
    if prob == 1.0 and L >= 0.8:
        assert not inv.any() and len({r.tobytes() for r in got.T}) > 0.99 * M


@pytest.mark.parametrize("name", ["hpl64", "perm_mixed"])
def test_high_counter_word(setups, name):
    space, e, centre = setups[name]
    h = np.full(len(space), 0.4)
    a, _ = check(space, e, centre, h, 0.3, 0.3, 1, BIG)
    b, _ = call(e, centre, h, 0.3, 0.3, 1, 5, M)
    assert (a != b).any()


@pytest.mark.parametrize("name", ["hpl64", "perm_mixed"])
@pytest.mark.parametrize("face", ["lo", "hi"])
def test_centre_on_a_face_of_the_space(setups, name, face):
    """every primitive at its lower / upper bound: a FLOAT's unit value is exactly 0 / 1, the box is clipped there"""
    space, e, centre = setups[name]
    starts, _ = columns(space)
    c = centre.copy()
    for p, prm in enumerate(space):
        if prm.is_primitive():
            c[starts[p]] = float(prm.lo if face == "lo" else prm.hi)
    fl = [p for p, prm in enumerate(space) if prm.kind == FLOAT]
    assert all(tro.box_faces(space[p], c[starts[p]], 0.0)[0] == (0.0 if face == "lo" else 1.0) for p in fl)
    for L in (1.6, 2.0 ** -7):
        check(space, e, c, np.full(len(space), L / 2.0), 1.0, 0.5, 2, 11)


@pytest.mark.parametrize("name", ["hpl64", "perm_mixed"])
def test_anisotropic_half_widths(setups, name):
    space, e, centre = setups[name]
    h = np.array([[0.0, 2.5, 0.01, 1.0, 1e-9, 0.3][p % 6] for p in range(len(space))])
    check(space, e, centre, h, 0.7, 0.2, 4, 11, must=3)
    check(space, e, centre, h, 0.0, 0.0, 4, 11, must=len(space))    # every parameter forced
    _, inv = check(space, e, centre, h, 0.0, 0.0, 4, 11, must=0)    # nothing moves
    assert inv.all()


def test_collapsed_integer_boxes_are_all_invalid():
    space = [Param("i%d" % k, INT, 0, 1000) for k in range(6)]
    e = _engine(space, seed=1)
    c = np.array([0.0, 1000.0, 500.0, 1.0, 999.0, 37.0])
    got, inv = check(space, e, c, np.full(6, 1e-9), 1.0, 1.0, 0, 0)
    assert inv.all() and (got.view(np.uint64) == c.view(np.uint64)[:, None]).all()


def test_single_point_space_is_all_invalid():
    space = [Param("k", INT, 5, 5), Param("e", ENUM, options=["x"])]
    e = _engine(space, seed=1)
    _, inv = check(space, e, np.array([5.0, 0.0]), np.array([0.4, 0.4]), 1.0, 1.0, 0, 0, must=2)
    assert inv.all()


@pytest.mark.parametrize("name", ["hpl64", "perm_mixed"])
def test_deterministic_and_split_invariant(setups, name):
    space, e, centre = setups[name]
    h = np.full(len(space), 0.4)
    for base in (11, BIG):
        a, ai = call(e, centre, h, 0.3, 0.6, 5, base, M)
        b, bi = call(e, centre, h, 0.3, 0.6, 5, base, M)
        assert a.tobytes() == b.tobytes() and ai.tobytes() == bi.tobytes()
        k = 437
        l, li = call(e, centre, h, 0.3, 0.6, 5, base, k)
        r, ri = call(e, centre, h, 0.3, 0.6, 5, base + k, M - k)
        assert np.concatenate([l, r], axis=1).tobytes() == a.tobytes()
        assert np.concatenate([li, ri]).tobytes() == ai.tobytes()


def test_engine_method(setups):
    space, e, centre = setups["hpl64"]
    h = np.full(len(space), 0.4)
    vals, inv = e.propose_tr(M, centre, h, 0.3, round_=2, cand_base=11)
    want, winv, _ = tro.propose_tr_vec(space, centre, h, 0.3, 0.3, e.seed, 2, 11, M)
    np.testing.assert_array_equal(vals.cpu().numpy(), want)
    np.testing.assert_array_equal(inv.cpu().numpy().astype(bool), winv)
    with pytest.raises(ValueError):
        e.propose_tr(M, centre, h[:-1], 0.3)


def test_refusals_launch_nothing(setups):
    from uptune_amd import _lib as L
    space, e, centre = setups["perm_mixed"]
    P = len(space)
    h = np.full(P, 0.4)
    bad = h.copy()
    bad[2] = -0.1
    nan, inf = h.copy(), h.copy()
    nan[1], inf[0] = np.nan, np.inf
    for kw in (dict(centre=None, half=h, prob=0.3, cat_prob=0.3), dict(centre=centre, half=h, prob=1.5, cat_prob=0.3),
               dict(centre=centre, half=h, prob=0.3, cat_prob=-0.1), dict(centre=centre, half=bad, prob=0.3, cat_prob=0.3),
               dict(centre=centre, half=nan, prob=0.3, cat_prob=0.3), dict(centre=centre, half=inf, prob=0.3, cat_prob=0.3),
               dict(centre=centre, half=h, prob=0.3, cat_prob=0.3, ld=M - 1),
               dict(centre=centre, half=h, prob=0.3, cat_prob=0.3, must=P + 1),
               dict(centre=centre, half=h, prob=0.3, cat_prob=0.3, must=-1)):
        rc, out, inv = call(e, round_=0, base=0, m=M, raw=True, **kw)
        assert rc == -1, kw                                   # UT_EINVAL
        assert (out == SENTINEL).all() and (inv == 9).all()   # no kernel wrote anything
    # before ut_space_define
    ctx = C.c_void_p()
    assert e.lib.ut_ctx_create(0, 1, C.byref(ctx)) == 0
    a = L.TrParams(prob=0.3, cat_prob=0.3, must=1)
    rc = e.lib.ut_propose_tr(ctx, C.byref(a), None, None, 0, 0, 10, None, 10, None)
    e.lib.ut_ctx_destroy(ctx)
    assert rc == -3                                           # UT_ENOSPACE
