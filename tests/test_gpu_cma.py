"""ut_propose_cma on the device against its numpy restatement (tests/_cma_oracle.py;
the rule is stated in include/uthot.h).  The unit points are held by the rule's
forward-error bound, element by element; the values are set_unit_value of the
device's own unit points, and the BOOL / ENUM / PERM columns and the invalid
mask are the restatement's, all bit for bit."""
import ctypes as C

import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

import _cma_oracle as co  # noqa: E402
from _spaces import oracle_space, to_manip  # noqa: E402
from oracle import de as ode  # noqa: E402
from oracle.space import FLOAT, INT, POW2, Param, columns, get_unit_value_vec, set_unit_value_vec  # noqa: E402

M, PADDING, SEED, SENTINEL = 1000, 24, 23, -7.25
BASE = 2 ** 32 - 300            # the range of M candidates crosses the counter's high word
DNS = [1, 3, 16, 17, 64, 65, 128]


def _space(name):
    if name != "mixed":
        return [Param("x%d" % k, FLOAT, -5.0, 10.0) for k in range(int(name))]
    from uptune_amd import spaces          # every kind, a single-point POW2 and a single-point INT
    return oracle_space(spaces.perm_mixed()) + [Param("p2", POW2, 1, 1024), Param("p2fix", POW2, 256, 256),
                                                Param("ifix", INT, 2, 2)]


def _factor(dn, kind, rng):
    if kind == "dense":
        return rng.normal(size=(dn, dn)) / np.sqrt(dn)
    q, _ = np.linalg.qr(rng.normal(size=(dn, dn)))      # lower-triangular factor of an SPD matrix, cond ~ 1e6
    return np.linalg.cholesky((q * np.logspace(-6.0, 0.0, dn)) @ q.T)


@pytest.fixture(scope="module")
def setup():
    """name, factor kind -> (space, engine, centre, mean, A, the restatement at M candidates from BASE)"""
    if not torch.cuda.is_available():
        pytest.skip("no GPU")
    from uptune_amd.engine import BatchEngine
    made, engines = {}, {}

    def get(name, kind="chol", sigma=0.3, cat_prob=0.3):
        key = (name, kind, sigma, cat_prob)
        if key not in made:
            space = _space(name)
            if name not in engines:
                engines[name] = BatchEngine(to_manip(space), device=0, seed=SEED)
            e = engines[name]
            rng = np.random.default_rng(len(space))
            centre = ode.population_init(space, 4, seed=5)[:, 1].copy()
            dn = len(co.moving(space))
            mean, A = rng.uniform(0.2, 0.8, dn), _factor(dn, kind, rng)
            ref = co.propose_cma_vec(space, centre, mean, A, sigma, cat_prob, SEED, 3, BASE, M)
            made[key] = (space, e, centre, mean, A, ref)
        return made[key]
    return get


def call(e, centre, mean, A, sigma, cat_prob, m, base=BASE, round_=3, dn=None, ld=None, unit=True, null=None):
    """ut_propose_cma through the C ABI with ld > m -> (rc, whole values buffer, invalid, whole unit buffer)"""
    from uptune_amd import _lib as L
    dn = len(mean) if dn is None else dn
    ld = m + PADDING if ld is None else ld
    out = torch.full((e.spec.ncols, max(ld, 1)), SENTINEL, dtype=torch.float64, device=e.device)
    un = torch.full((max(len(mean), 1), max(ld, 1)), SENTINEL, dtype=torch.float64, device=e.device)
    inv = torch.full((max(m, 1),), 9, dtype=torch.uint8, device=e.device)
    c = torch.from_numpy(np.ascontiguousarray(centre, dtype=np.float64)).to(e.device)
    mu, A = np.ascontiguousarray(mean, dtype=np.float64), np.ascontiguousarray(A, dtype=np.float64)
    ptr = dict(centre=C.c_void_p(c.data_ptr()), mean=C.c_void_p(mu.ctypes.data), factor=C.c_void_p(A.ctypes.data),
               out=C.c_void_p(out.data_ptr()), inv=C.c_void_p(inv.data_ptr()),
               unit=C.c_void_p(un.data_ptr()) if unit else None)
    a = L.CmaParams(sigma=sigma, cat_prob=cat_prob, dn=dn)
    ptr["params"] = C.byref(a)
    if null:
        ptr[null] = None
    rc = e.lib.ut_propose_cma(e.ctx, ptr["params"], ptr["centre"], ptr["mean"], ptr["factor"], round_, base, m,
                              ptr["out"], ld, ptr["inv"], ptr["unit"])
    e.sync()
    return rc, out.cpu().numpy(), inv.cpu().numpy(), un.cpu().numpy()


def check(space, e, centre, mean, A, ref, sigma, cat_prob, m, base=BASE):
    """one call held to the first m candidates of the restatement `ref` -> (values, invalid, unit)"""
    rc, out, inv, un = call(e, centre, mean, A, sigma, cat_prob, m, base=base)
    assert rc == 0, e.lib.ut_last_error(e.ctx)
    assert (out[:, m:] == SENTINEL).all() and (un[:, m:] == SENTINEL).all()     # nothing past column m
    got, u = out[:, :m], un[:, :m]
    want, _, u_ref, bound = (r[..., :m] for r in ref)
    assert (u >= 0.0).all() and (u <= 1.0).all()
    err = np.abs(u - u_ref)
    print("dn %d m %d: max |u - u_ref| / bound = %.3g" % (len(mean), m, float((err / bound).max())))
    assert (err <= bound).all()
    # primitive columns from the device's own u; every other column is the restatement's
    want = want.copy()
    starts, _ = columns(space)
    for j, p in enumerate(co.moving(space)):
        want[starts[p]] = set_unit_value_vec(space[p], u[j], np.full(m, centre[starts[p]])) + 0.0
    np.testing.assert_array_equal(got.view(np.uint64), want.view(np.uint64))
    same = (want.view(np.uint64) == centre.view(np.uint64)[:, None]).all(axis=0)
    np.testing.assert_array_equal(inv[:m].astype(bool), same)
    return got, same, u


@pytest.mark.parametrize("kind", ["chol", "dense"])
@pytest.mark.parametrize("m", [1, 63, 65, 1000])
@pytest.mark.parametrize("dn", DNS)
def test_unit_points_and_values(setup, dn, m, kind):
    space, e, centre, mean, A, ref = setup(str(dn), kind)
    _, same, _ = check(space, e, centre, mean, A, ref, 0.3, 0.3, m)
    assert not same.any()


@pytest.mark.parametrize("cat_prob", [0.0, 0.3, 1.0])
def test_mixed_space(setup, cat_prob):
    space, e, centre, mean, A, ref = setup("mixed", "dense", 0.3, cat_prob)
    assert len(mean) == 4 and e.spec.P - 4 == 7
    got, _, _ = check(space, e, centre, mean, A, ref, 0.3, cat_prob, M)
    assert len({r.tobytes() for r in got.T}) > 0.99 * M


def test_mirroring_folds_wide_samples_into_the_unit_box(setup):
    """sigma = 50: a sample lies tens of folds outside [0, 1]"""
    space, e, centre, mean, A, _ = setup("17", "dense")
    wide = co.propose_cma_vec(space, centre, mean, A, 50.0, 0.0, SEED, 3, BASE, M)
    _, _, u = check(space, e, centre, mean, A, wide, 50.0, 0.0, M)
    assert u.min() < 0.01 and u.max() > 0.99


@pytest.mark.parametrize("cat_prob", [0.0, 0.3])
def test_collapsed_step_on_an_integer_space_is_invalid(cat_prob):
    """sigma = 1e-13 around the centre's own unit point: every integer rounds back, so a row
    differs from the centre only where the BOOL or the ENUM moved"""
    from oracle.space import BOOL, ENUM
    from uptune_amd.engine import BatchEngine
    space = [Param("i%d" % k, INT, 0, 1000) for k in range(6)] + [Param("b", BOOL), Param("e", ENUM, options=list("xyz"))]
    e = BatchEngine(to_manip(space), device=0, seed=1)
    c = np.array([0.0, 1000.0, 500.0, 1.0, 999.0, 37.0, 1.0, 2.0])
    uc = np.array([get_unit_value_vec(space[p], c[p:p + 1])[0] for p in range(6)])
    A = np.random.default_rng(2).normal(size=(6, 6))
    ref = co.propose_cma_vec(space, c, uc, A, 1e-13, cat_prob, 1, 3, BASE, M)
    got, same, _ = check(space, e, c, uc, A, ref, 1e-13, cat_prob, M)
    assert (got[:6].view(np.uint64) == c[:6].view(np.uint64)[:, None]).all()
    assert same.all() if cat_prob == 0.0 else 0 < same.sum() < M


@pytest.mark.parametrize("name", ["65", "mixed"])
def test_split_invariant_across_the_high_counter_word(setup, name):
    space, e, centre, mean, A, _ = setup(name, "dense")
    _, out, inv, un = call(e, centre, mean, A, 0.3, 0.3, M)
    parts = [call(e, centre, mean, A, 0.3, 0.3, n, base=BASE + b) for b, n in ((0, 437), (437, 128), (565, 435))]
    assert all(p[0] == 0 for p in parts)
    for whole, k in ((out, 1), (un, 3)):
        assert np.concatenate([p[k][:, :n] for p, n in zip(parts, (437, 128, 435))], axis=1).tobytes() == \
            np.ascontiguousarray(whole[:, :M]).tobytes()
    assert np.concatenate([p[2][:n] for p, n in zip(parts, (437, 128, 435))]).tobytes() == inv[:M].tobytes()
    again = call(e, centre, mean, A, 0.3, 0.3, M, base=5)
    assert (again[1] != out).any()


def test_refusals_launch_nothing(setup):
    from uptune_amd import _lib as L
    space, e, centre, mean, A, _ = setup("mixed", "dense")
    nan_mean, inf_fac = mean.copy(), A.copy()
    nan_mean[1], inf_fac[2, 3] = np.nan, np.inf
    ok = dict(centre=centre, mean=mean, A=A, sigma=0.3, cat_prob=0.3, m=M)
    for kw in ([dict(null=k) for k in ("params", "centre", "mean", "factor", "out", "inv")] +
               [dict(sigma=s) for s in (0.0, -1.0, np.inf, np.nan)] + [dict(cat_prob=p) for p in (-0.1, 1.5, np.nan)] +
               [dict(dn=d) for d in (0, 3, 5, 129)] + [dict(mean=nan_mean), dict(A=inf_fac), dict(m=-1),
                                                        dict(base=-1), dict(ld=M - 1)]):
        rc, out, inv, un = call(e, **{**ok, **kw})
        assert rc == -1, kw                                                            # UT_EINVAL
        assert (out == SENTINEL).all() and (inv == 9).all() and (un == SENTINEL).all()   # no kernel wrote
    ctx = C.c_void_p()                                                                 # before ut_space_define
    assert e.lib.ut_ctx_create(0, 1, C.byref(ctx)) == 0
    a = L.CmaParams(sigma=0.3, cat_prob=0.3, dn=4)
    rc = e.lib.ut_propose_cma(ctx, C.byref(a), None, None, None, 0, 0, 10, None, 10, None, None)
    e.lib.ut_ctx_destroy(ctx)
    assert rc == -3                                                                    # UT_ENOSPACE
