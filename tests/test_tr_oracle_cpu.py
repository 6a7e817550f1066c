"""Trust-region proposals without a GPU: the numpy restatement of ut_propose_tr
(tests/_tr_oracle.py) keeps the invariants of the rule in include/uthot.h, the
TrustRegion state machine follows TuRBO-1's schedule, and the opt-in wiring
changes nothing unless asked."""
import ctypes as C
import math

import numpy as np
import pytest

import _tr_oracle as tro
from _spaces import oracle_space
from oracle import de as ode
from oracle.space import BOOL, ENUM, INT, LOGINT, PERM, POW2, columns, get_unit_value_vec, width


def _space(name):
    from uptune_amd import spaces
    return oracle_space(spaces.hpl64() if name == "hpl64" else spaces.perm_mixed())


def _centre(space, seed=5):
    return ode.population_init(space, 4, seed=seed)[:, 1].copy()


def _half(space, L):
    return np.full(len(space), L / 2.0)


@pytest.mark.parametrize("name", ["hpl64", "perm_mixed"])
@pytest.mark.parametrize("L", [1.6, 0.8, 2.0 ** -7])
def test_restatement_invariants(name, L):
    space = _space(name)
    starts, nc = columns(space)
    c = _centre(space)
    h = _half(space, L)
    m = 600
    vals, inv, u_pre, picked = tro.propose_tr_vec(space, c, h, 0.3, 0.5, 7, 2, 11, m, must=1, with_selected=True)
    assert vals.shape == (nc, m) and inv.shape == (m,)
    assert picked.sum(axis=0).min() >= 1
    for p, prm in enumerate(space):
        c0, col = starts[p], vals[starts[p]]
        # an unselected parameter keeps the centre's bits
        keep = ~picked[p]
        w = width(prm)
        assert (vals[c0:c0 + w][:, keep].view(np.uint64) == c[c0:c0 + w].view(np.uint64)[:, None]).all()
        if prm.is_primitive():
            _, lo, hi = tro.box_faces(prm, c[c0], h[p])
            u = u_pre[p, picked[p]]
            assert np.isfinite(u).all() and (u >= lo).all() and (u <= hi).all()
            assert np.isnan(u_pre[p, keep]).all()
            lo_v, hi_v = float(prm.lo), float(prm.hi)
            assert (col >= lo_v).all() and (col <= hi_v).all()
            if prm.kind in (INT, LOGINT, POW2):
                assert (col == np.rint(col)).all()
            if prm.kind == POW2:
                assert (np.frexp(col)[0] == 0.5).all()
            if prm.lo == prm.hi:
                assert (col == c[c0]).all()
        elif prm.kind == BOOL:
            assert set(np.unique(col)) <= {0.0, 1.0}
            assert (col[picked[p]] == 1.0 - c[c0]).all()
        elif prm.kind == ENUM:
            n = len(prm.options)
            assert (col >= 0).all() and (col < n).all() and (col == np.rint(col)).all()
            if n > 1:
                assert (col[picked[p]] != c[c0]).all()
        elif prm.kind == PERM:
            assert (np.sort(vals[c0:c0 + w], axis=0) == np.arange(w)[:, None]).all()
    same = (vals.view(np.uint64) == c.view(np.uint64)[:, None]).all(axis=0)
    np.testing.assert_array_equal(inv, same)


def test_enum_moves_are_uniform_over_the_other_options():
    space = _space("hpl64")
    starts, _ = columns(space)
    c = _centre(space)
    vals, _, _ = tro.propose_tr_vec(space, c, _half(space, 0.8), 0.0, 1.0, 3, 0, 0, 3000, must=0)
    p = next(i for i, q in enumerate(space) if q.kind == ENUM and len(q.options) == 6)
    cnt = np.bincount(vals[starts[p]].astype(int), minlength=6)
    assert cnt[int(c[starts[p]])] == 0
    assert (np.delete(cnt, int(c[starts[p]])) > 3000 / 5 * 0.8).all()


@pytest.mark.parametrize("name", ["hpl64", "perm_mixed"])
@pytest.mark.parametrize("must", [0, 1, 5])
def test_exactly_must_parameters_at_zero_rates(name, must):
    space = _space(name)
    out = tro.propose_tr_vec(space, _centre(space), _half(space, 0.8), 0.0, 0.0, 9, 1, 2 ** 32 + 5, 400, must=must,
                             with_selected=True)
    assert (out[3].sum(axis=0) == must).all()
    if must == 0:
        assert out[1].all()


def test_rows_are_a_function_of_the_global_index():
    space = _space("perm_mixed")
    c, h = _centre(space), _half(space, 0.8)
    a = tro.propose_tr_vec(space, c, h, 0.3, 0.3, 4, 1, 100, 200)
    b = tro.propose_tr_vec(space, c, h, 0.3, 0.3, 4, 1, 100, 80)
    d = tro.propose_tr_vec(space, c, h, 0.3, 0.3, 4, 1, 180, 120)
    np.testing.assert_array_equal(a[0], np.concatenate([b[0], d[0]], axis=1))
    np.testing.assert_array_equal(a[1], np.concatenate([b[1], d[1]]))
    assert (tro.propose_tr_vec(space, c, h, 0.3, 0.3, 4, 2, 100, 200)[0] != a[0]).any()


def test_collapsed_integer_box_is_all_invalid():
    from oracle.space import Param
    space = [Param("i%d" % k, INT, 0, 1000) for k in range(6)]
    c = np.array([0.0, 1000.0, 500.0, 1.0, 999.0, 37.0])
    vals, inv, _ = tro.propose_tr_vec(space, c, np.full(6, 1e-9), 1.0, 1.0, 1, 0, 0, 300)
    assert inv.all() and (vals == c[:, None]).all()
    space = [Param("k", INT, 5, 5), Param("e", ENUM, options=["x"])]
    vals, inv, _ = tro.propose_tr_vec(space, np.array([5.0, 0.0]), np.array([0.4, 0.4]), 1.0, 1.0, 1, 0, 0, 100)
    assert inv.all()


# --------------------------------------------------------------------------- the state machine
def test_trust_region_schedule():
    from uptune_amd.trust_region import TrustRegion
    t = TrustRegion(n_move=64, batch=8)
    assert t.fail_tol == 8 and TrustRegion(n_move=4, batch=8).fail_tol == 4 and t.L == 0.8
    assert TrustRegion(n_move=64, batch=8, fail_tol=2).fail_tol == 2
    for _ in range(2):
        assert t.judge(True) is False
    assert t.L == 0.8
    t.judge(True)
    assert t.L == 1.6                       # doubled after succ_tol = 3 successes in a row
    for _ in range(3):
        t.judge(True)
    assert t.L == 1.6                       # capped at L_max
    t.judge(True), t.judge(True), t.judge(False), t.judge(True), t.judge(True)
    assert t.L == 1.6 and t.succ == 2       # a failure breaks the streak
    for _ in range(7):
        t.judge(False)
    assert t.L == 1.6
    t.judge(False)
    assert t.L == 0.8 and t.fail == 0       # halved after fail_tol = 8 failures in a row
    assert t.probs() == (20 / 64, 20 / 64)
    t.judge(False), t.judge(True)
    assert t.fail == 0 and t.succ == 1      # a success breaks the failure streak


def test_trust_region_restarts_below_l_min():
    from uptune_amd.trust_region import TrustRegion
    t = TrustRegion(n_move=8, batch=8, fail_tol=1)
    halvings = 0
    while not t.judge(False):
        halvings += 1
        assert t.L >= t.L_min
        prob, cat = t.probs()
        assert prob == 1.0 and cat == min(1.0, t.L / t.L_init)
    # 0.8 -> ... -> 0.8 / 2^6 = 2^-7 * 1.6 >= L_min; the seventh halving falls below it
    assert halvings == 6 and t.restarts == 1 and t.L == t.L_init and t.succ == t.fail == 0
    t.L = t.L_min
    assert t.judge(False) is True and t.restarts == 2


def test_half_widths():
    from uptune_amd import spaces
    from uptune_amd._lib import UT_FLOAT, UT_INT, UT_LOGINT, UT_POW2
    from uptune_amd.manipulator import compile_space
    from uptune_amd.trust_region import TrustRegion
    spec = compile_space(spaces.hpl64())
    t = TrustRegion(n_move=60, batch=8)
    prim = [i for i, p in enumerate(spec.params) if p.kind in (UT_FLOAT, UT_INT, UT_LOGINT, UT_POW2)]
    mov = [i for i in prim if spec.params[i].lo < spec.params[i].hi]
    fixed = [i for i in prim if i not in mov]
    assert sorted(spec.params[i].name for i in fixed) == ["ndiv", "pow2_3"]
    floor = np.array([0.0 if spec.params[i].kind == UT_FLOAT else 1.0 / spec.params[i].u_span for i in mov])
    # a scalar lengthscale: w = 1 (a two-value integer's floor, 1 / 1.9998, is above L / 2 = 0.4)
    h = t.half_widths(spec, 0.2)
    assert h.shape == (spec.P,) and (h[fixed] == 0.0).all() and (np.delete(h, prim) == 0.0).all()
    np.testing.assert_array_equal(h[mov], np.maximum(0.4, floor))
    assert (h[mov] == 0.4).sum() > 30 and floor.max() > 0.5
    # per-feature lengthscales: w = ell / geomean(ell) over the movable primitives
    rng = np.random.default_rng(3)
    ell = np.exp(rng.normal(size=spec.n_features))
    e = np.array([ell[spec.params[i].feat_col] for i in mov])
    w = e / math.exp(np.mean(np.log(e)))
    assert abs(float(np.mean(np.log(w)))) < 1e-12 and w.max() / w.min() > 10
    for t.L in (1.6, 0.8, 2.0 ** -12):     # the last: all but the widest integer ranges sit on their floor
        h = t.half_widths(spec, ell)
        np.testing.assert_allclose(h[mov], np.maximum(t.L * w / 2.0, floor), rtol=1e-12)
        assert (h[fixed] == 0.0).all() and (np.delete(h, prim) == 0.0).all()
    assert (h[mov] >= floor).all() and (h[mov][floor > 0] == floor[floor > 0]).sum() > 20
    # ... and on a space without integer kinds the geometric mean of h / (L / 2) is 1
    spec = compile_space(spaces.r64())
    ell = np.exp(rng.normal(size=spec.n_features))
    w = t.half_widths(spec, ell) / (t.L / 2.0)
    assert abs(float(np.mean(np.log(w)))) < 1e-12 and w.max() / w.min() > 10


def test_integer_floor_reaches_a_neighbour():
    """with h = 1 / u_span the box of an INT centre covers the unit interval of a neighbouring integer"""
    from oracle.space import Param
    prm = Param("n", INT, 0, 1000)
    c = np.array([500.0])
    uc = float(get_unit_value_vec(prm, c)[0])
    span = 1000.9998
    vals, inv, _ = tro.propose_tr_vec([prm], c, np.array([1.0 / span]), 1.0, 1.0, 2, 0, 0, 400)
    assert set(np.unique(vals[0])) == {499.0, 500.0, 501.0} and 0 < inv.sum() < 400
    assert 0.0 < uc < 1.0


# --------------------------------------------------------------------------- wiring
def test_registry_and_bandits_are_unchanged_without_the_flag():
    from uptune_amd import technique as T
    kw = dict(pool=256, batch=4)
    reg = T.reference_registry(**kw)
    assert len(reg) == 24 and not any(isinstance(t, T.GpuTrustRegion) for t in reg)
    reg = T.reference_registry(trust_region=True, **kw)
    assert len(reg) == 25 and isinstance(reg[-1], T.GpuTrustRegion) and reg[-1].name == "GpuTrustRegion"
    assert [t.name for t in reg[:24]] == [t.name for t in T.reference_registry(**kw)]
    for make, n in ((T.bandit_a, 3), (T.bandit_b, 2), (T.pso_ga_de_bandit, 4)):
        a, b, c = make(**kw), make(trust_region=True, **kw), make(trust_region=False, **kw)
        assert len(a.techniques) == len(c.techniques) == n and len(b.techniques) == n + 1
        assert [type(t) for t in a.techniques] == [type(t) for t in b.techniques[:n]]
        arm = b.techniques[-1]
        assert isinstance(arm, T.GpuTrustRegion) and arm.name == "gpu-trust-region"
        assert arm.model is b.techniques[0].model and arm.sharded and arm.centre_mode == "best"
        assert not hasattr(a.techniques[0], "trust_region")
    with pytest.raises(ValueError):
        T.GpuTrustRegion(centre="nearest", **kw)
    assert T.GpuTrustRegion(centre="own", **kw).centre_mode == "own"
    import inspect
    from uptune_amd.tuner import tune_bandit
    assert inspect.signature(tune_bandit).parameters["trust_region"].default is False


def test_c_abi_refuses_without_a_context():
    from uptune_amd import _lib as L
    lib = L.lib()
    assert C.sizeof(L.TrParams) == 24
    hc = C.CDLL(L.LIB_PATH.replace("libuthot.so", "libuthot_hostcheck.so"))
    hc.uthc_sizeof.restype = C.c_longlong
    assert hc.uthc_sizeof(10) == C.sizeof(L.TrParams)
    assert hc.uthc_sizeof(9) > 0 and hc.uthc_sizeof(11) == -1     # the earlier indices stay, none is added past it
    a = L.TrParams(prob=0.3, cat_prob=0.3, must=1)
    h = (C.c_double * 2)(0.1, 0.1)
    assert lib.ut_propose_tr(None, C.byref(a), None, h, 0, 0, 10, None, 10, None) == -1   # UT_EINVAL
