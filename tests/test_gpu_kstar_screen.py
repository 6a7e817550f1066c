"""The K* screen (k_q_screen, gp_kq.hip): before k_gp_kstar_q it certifies the units
(64 training rows x 128 candidates) whose every element is stored as six zero
digits, from the products of the operands' two top digit planes; their planes are
not computed, k_gp_kstar_q walks the list of the other items and the masked
variance kernel the list of the strips with a live unit.  Held here to the
unscreened library bit for bit (UT_KSTAR_SCREEN=1 against 0) on the mask table
and the borderline sweeps of _kstar_screen_cases.py, across calls on one context
(stale planes behind cleared mask dwords), under the library's own choice, on the
paths where it must not run, and against oracle/gp.py."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

import _ard_cases as A  # noqa: E402
import _i8_plan_model as PM  # noqa: E402
import _kstar_cases as KC  # noqa: E402
import _kstar_mask_cases as MC  # noqa: E402
import _kstar_screen_cases as SC  # noqa: E402
from _spaces import to_manip  # noqa: E402
from oracle import de as ode  # noqa: E402
from oracle import gp as ogp  # noqa: E402
from oracle.space import features  # noqa: E402

CASES = SC.all_cases()
KEYS = ("mu", "var", "score", "k", "mask", "var_part", "mu_part")


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")


def _engine(space, monkeypatch, screen, var_skip=None, tol=None, seed=0, strips="with_screen"):
    """screen True / False / None: UT_KSTAR_SCREEN=1 / 0 / unset (the library's own choice);
    var_skip likewise for UT_VAR_SKIP and strips for UT_KSTAR_STRIPS (all read per call).  strips
    "with_screen": 1 where the screen is forced (the variance kernel then walks the strip list in
    every screened call), unset otherwise"""
    if strips == "with_screen":
        strips = True if screen is True else None
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    monkeypatch.setenv("UT_KSTAR_Q", "1")
    for name, v in (("UT_KSTAR_SCREEN", screen), ("UT_VAR_SKIP", var_skip), ("UT_KSTAR_STRIPS", strips)):
        if v is None:
            monkeypatch.delenv(name, raising=False)
        else:
            monkeypatch.setenv(name, "1" if v else "0")
    from uptune_amd.engine import BatchEngine
    e = BatchEngine(to_manip(space), device=0, seed=seed)
    e.gp_set_precision(8)
    if tol is not None:
        e.gp_set_i8_tol(tol)
    return e


def _read(e, m):
    """everything the last dense call left, as host arrays"""
    out = dict(stats=e.gp_i8_stats(), screen=e.gp_kstar_screen_stats())
    kd, npad, ldk, fmt = e.gp_kstar_read()
    out.update(k=kd.cpu().numpy(), npad=npad, ldk=ldk, fmt=fmt)
    mk = e.gp_kstar_mask_read()
    out["mask"] = None if mk is None else mk.cpu().numpy()
    if fmt == 8:
        vp, mp = e.gp_i8_parts_read()
        out["var_part"], out["mu_part"] = vp.cpu().numpy()[:, :m], mp.cpu().numpy()[:, :m]
    return out


def _score(e, U):
    mu, var, sc = e.gp_score(dev(U.T))
    out = dict(mu=mu.cpu().numpy(), var=var.cpu().numpy(), score=sc.cpu().numpy())
    out.update(_read(e, U.shape[0]))
    return out


def _same(a, b, what):
    assert a["stats"] == b["stats"] and a["fmt"] == b["fmt"], what
    for key in KEYS:
        if key in a or key in b:
            if a.get(key) is None or b.get(key) is None:
                assert a.get(key) is None and b.get(key) is None, "%s: %s" % (what, key)
            else:
                assert np.array_equal(a[key], b[key]), "%s: %s differs" % (what, key)


_RUNS = {}


def _run(monkeypatch, c, screen):
    key = (c["name"], screen)
    if key not in _RUNS:
        z = SC.inputs(c)
        e = _engine(A.float_space(c["d"]), monkeypatch, screen, tol=0.999)   # (no whole-round fp64 fallback)
        e.gp_fit(z["X"], z["y"], lengthscale=z["ell"], wait=not c["fit_async"], **MC.hyper(c["sf2"]))
        if z.get("pre") is not None:
            e.gp_score(dev(z["pre"].T))
        _RUNS[key] = _score(e, z["U"])
        e.close()
    return _RUNS[key]


@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_screen_changes_no_bit(monkeypatch, c):
    """the mask table (wait=False fit and a shrinking ldk among its cases) and the borderline sweeps"""
    a, b = _run(monkeypatch, c, True), _run(monkeypatch, c, False)
    _same(a, b, c["name"])
    assert b["screen"][0] is False and b["screen"][1] == 0
    npad, ldk = KC.npad_of(c["n"]), KC.ldk_of(c["m"])
    screened, ncert, units = a["screen"]
    assert units == (npad // 64) * (ldk // 128)
    assert screened is (npad <= 2048)          # (past I8_MASK_MAX_K rows there is no masked variance kernel)
    if not screened:
        return
    # every unit the CPU effectiveness rule names is certified, and nothing with a digit in it
    z = SC.inputs(c)
    zero = SC.zero_units(a["k"][:c["n"], :c["m"]], c["n"], c["m"])
    cpu = SC.certificate(z["X"], z["U"], z["ell"], c["n"], c["m"])[0]
    must = SC.must_certify(z["X"], z["U"], z["ell"], c["n"], c["m"]) if KC.have_longdouble() else cpu
    print("%s: %d units, certified %d (the restatement: %d), named by the rule %d, all-zero %d" %
          (c["name"], units, ncert, int(cpu.sum()), int(must.sum()), int(zero.sum())))
    assert int(must.sum()) <= ncert <= int(zero.sum())
    # unit by unit: a certified unit has both its mask dwords 0 (rows 2 rt, 2 rt + 1; bytes 4 ct .. 4 ct + 3)
    dead = ~a["mask"].reshape(npad // 64, 2, ldk // 128, 4).any(axis=(1, 3))
    assert not (must & ~dead).any(), "a unit the rule names has a mask byte set: %s" % np.argwhere(must & ~dead)[:4].tolist()


def _table():
    c = MC.CASES[8]     # n 1000, d 64, m 300
    return c, MC.data(c)


def test_stats_far_and_near(monkeypatch):
    c, z = _table()
    far = np.tile(z["U"][96:128], (9, 1))           # the 'far' block: 288 candidates
    e = _engine(A.float_space(c["d"]), monkeypatch, True, tol=0.999)
    e.gp_fit(z["X"], z["y"], lengthscale=z["ell"], **MC.hyper(c["sf2"]))
    r = _score(e, far)
    assert r["screen"] == (True, r["screen"][2], (1024 // 64) * (512 // 128)) and not r["mask"].any()
    assert np.all(r["var"] == c["sf2"]) and np.all(r["mu"] == 0.0)
    e.gp_fit(z["X"], z["y"], lengthscale=25.0, **MC.hyper(c["sf2"]))   # every k* near sf2
    r = _score(e, z["U"])
    # (the padding's units -- columns 384 .. 511 -- are certified whatever the lengthscale; rows 1000 .. 1023
    # share the last tile with live rows)
    assert r["screen"][0] is True and r["screen"][1] == (1024 // 64) * 1
    e.close()


def _two_clusters():
    """n = 129, d = 8: rows 0 .. 63 and 128 at P (the origin), 64 .. 127 at Q = P + 9 e_0 (exp(-40.5) sf2: zero
    digits across, every plane with a digit within a cluster); four candidate sets of m = 384"""
    rng = np.random.default_rng(77)
    n, d, m = 129, 8, 384
    X = rng.uniform(size=(n, d)) * 0.3
    X[64:128, 0] += 9.0
    y = np.sum((X - 0.4) ** 2, axis=1) / 40.0
    nearP = rng.uniform(size=(m, d)) * 0.3
    nearQ = nearP.copy()
    nearQ[:, 0] += 9.0
    far = nearP.copy()
    far[:, 1] += 30.0
    alt = (np.arange(m) % 2 == 0)[:, None]
    sets = dict(dense=np.where(alt, nearP, nearQ), far=far, half=np.where(alt, nearQ, far), rows=nearP)
    return X, y, sets


def test_stale_planes(monkeypatch):
    """a dense call leaves digits in every plane; the calls after it on the same context do not write the
    planes of the units they certify, and equal a fresh unscreened context all the same"""
    X, y, sets = _two_clusters()
    hy = dict(lengthscale=1.0, sigma_f2=1.0, sigma_n2=0.25, jitter=0.0)
    e = _engine(A.float_space(8), monkeypatch, True, tol=0.999)
    e.gp_fit(X, y, **hy)
    got = {name: _score(e, sets[name]) for name in ("dense", "far", "half", "rows", "dense")}
    e.close()
    assert np.all(got["dense"]["mask"][:4, :12] == 0x3f)      # rows 0 .. 127 x every candidate: all planes
    want_cert = dict(far=16, half=16 - 3, rows=16 - 3 * 2, dense=4 + 3)   # of 4 x 4 units (one padded strip)
    for name in ("far", "half", "rows", "dense"):
        f = _engine(A.float_space(8), monkeypatch, False, tol=0.999)
        f.gp_fit(X, y, **hy)
        _same(got[name], _score(f, sets[name]), name)
        f.close()
        assert got[name]["screen"] == (True, want_cert[name], 16), (name, got[name]["screen"])


def test_the_library_choice(monkeypatch):
    """both variables unset: dense, far, far, dense, far on one context equals UT_VAR_SKIP=0 (which never
    screens); the screen runs on the far call that follows a far call and not on the first call"""
    X, y, sets = _two_clusters()
    hy = dict(lengthscale=1.0, sigma_f2=1.0, sigma_n2=0.25, jitter=0.0)
    res = []
    for var_skip in (None, False):
        e = _engine(A.float_space(8), monkeypatch, None, var_skip=var_skip, tol=0.999)
        e.gp_fit(X, y, **hy)
        res.append([_score(e, sets[name]) for name in ("dense", "far", "far", "dense", "far")])
        e.close()
    for i, (a, b) in enumerate(zip(*res)):
        _same(a, b, "call %d" % i)
        assert b["screen"][0] is False
    ran = [r["screen"][0] for r in res[0]]
    print("screened calls:", ran)
    assert ran[0] is False and ran[2] is True


# far: unscreened, every block zero -> the hint; far: screened; dense: screened, 7 units of 16 (under half) ->
# held off; eight unscreened calls whose zero blocks (68 of 128 and more) alone would screen; dense: the hint
# returns; four screened calls
POLICY_SEQUENCE = ("far", "far", "dense", "dense", "half", "rows", "far", "dense", "half", "rows", "far", "dense",
                   "far", "half", "rows", "dense")
POLICY_SCREENED = "USSUUUUUUUUUSSSS"


def test_the_hint_policy_across_calls(monkeypatch):
    """all three variables unset, sixteen calls on one context: each call screens exactly when the policy model
    (_i8_plan_model.py), stepped with the counts read from the call before it (its mask and statistics), says
    so -- through a back-off episode: a screen that cleared under half, the eight held-off calls, the return"""
    X, y, sets = _two_clusters()
    e = _engine(A.float_space(8), monkeypatch, None, tol=0.999)
    e.gp_fit(X, y, lengthscale=1.0, sigma_f2=1.0, sigma_n2=0.25, jitter=0.0)
    hints, trace, held = PM.Hints(), "", []
    for i, name in enumerate(POLICY_SEQUENCE):
        plan = PM.plan(256, 1, PM.Env(), hints)
        e.gp_score(dev(sets[name].T))
        screened, ncert, units = e.gp_kstar_screen_stats()
        mask = e.gp_kstar_mask_read().cpu().numpy()
        assert mask.shape == (8, 16) and units == 16
        assert screened is plan.screen, "call %d (%s): the library %s, the model %s after %s" % (
            i, name, screened, plan.screen, hints)
        trace += "S" if screened else "U"
        # (a certified unit's 8 bytes are 0 and were not visited to be counted)
        cert = ncert if screened else 0
        n = PM.Counts(int((mask != 0x3f).sum()) - 8 * cert, cert, 0 if screened else int((mask == 0).sum()), mask.size)
        # held off: the counts alone (no back-off pending) would turn the hint on, the model leaves it off
        alone = PM.hints_next(hints._replace(backoff=0), plan, n).screen
        hints = PM.hints_next(hints, plan, n)
        held.append(alone and not hints.screen and not plan.screen)
        print("call %2d %-5s %s cert %2d zero %3d -> %s" % (i, name, trace[-1], ncert, int((mask == 0).sum()), hints))
    e.close()
    print("screened calls:", trace)
    # the episode, in the model's own trace: a screened call that set the back-off, held-off calls, the return
    assert trace == POLICY_SCREENED
    start = trace.index("SU")
    assert POLICY_SEQUENCE[start] == "dense" and sum(held) == 8 and all(held[start + 1:start + 9])
    assert "S" in trace[start + 9:]


def test_paths_without_the_screen(monkeypatch):
    X, y, sets = _two_clusters()
    hy = dict(lengthscale=1.0, sigma_f2=1.0, sigma_n2=0.25, jitter=0.0)
    e = _engine(A.float_space(8), monkeypatch, True, var_skip=False, tol=0.999)   # the unmasked variance kernel
    e.gp_fit(X, y, **hy)
    a = _score(e, sets["far"])
    e.close()
    assert a["screen"][0] is False and np.all(a["var"] == 1.0)
    # npad 2176 > 2048
    rng = np.random.default_rng(5)
    X2 = rng.uniform(size=(2049, 8))
    y2 = np.sum((X2 - 0.4) ** 2, axis=1)
    U2 = rng.uniform(size=(129, 8)) + 30.0
    e = _engine(A.float_space(8), monkeypatch, True, tol=0.999)
    e.gp_fit(X2, y2, **hy)
    b = _score(e, U2)
    e.close()
    assert b["screen"][0] is False and np.all(b["var"] == 1.0) and not b["mask"].any()
    # d = 132 (K32 = 5): the strip's planes do not fit the screen's LDS image
    X3 = rng.uniform(size=(129, 132))
    y3 = np.sum((X3 - 0.4) ** 2, axis=1)
    U3 = rng.uniform(size=(129, 132)) + 30.0
    e = _engine(A.float_space(132), monkeypatch, True, tol=0.999)
    e.gp_fit(X3, y3, **hy)
    d3 = _score(e, U3)
    e.close()
    assert d3["screen"][0] is False and np.all(d3["var"] == 1.0) and not d3["mask"].any()


def test_forced_screen_leaves_the_strip_list_to_its_hint(monkeypatch):
    """UT_KSTAR_SCREEN=1 with UT_KSTAR_STRIPS unset: the list after an all-far call, every strip otherwise;
    and UT_KSTAR_STRIPS=0: never the list.  The same bits as a fresh unscreened context either way"""
    X, y, sets = _two_clusters()
    hy = dict(lengthscale=1.0, sigma_f2=1.0, sigma_n2=0.25, jitter=0.0)
    for strips in (None, False):
        e = _engine(A.float_space(8), monkeypatch, True, tol=0.999, strips=strips)
        e.gp_fit(X, y, **hy)
        got = [(name, _score(e, sets[name])) for name in ("dense", "far", "half", "rows")]
        e.close()
        for name, r in got[1:]:
            f = _engine(A.float_space(8), monkeypatch, False, tol=0.999)
            f.gp_fit(X, y, **hy)
            _same(r, _score(f, sets[name]), "%s, strips %s" % (name, strips))
            f.close()
            assert r["screen"][0] is True


def test_whole_round_fallback_after_a_screened_call(monkeypatch):
    c, z = _table()
    far = np.tile(z["U"][96:128], (9, 1))
    res = []
    for screen in (True, False):
        e = _engine(A.float_space(c["d"]), monkeypatch, screen, tol=0.999)
        e.gp_fit(z["X"], z["y"], lengthscale=z["ell"], **MC.hyper(c["sf2"]))
        first = _score(e, far)
        assert first["screen"][0] is screen
        e.gp_set_i8_tol(0.0)                        # every candidate recomputed: kst rewritten as fp64 rows
        r = _score(e, z["U"])
        assert r["stats"][0] == -1 and r["fmt"] == 64 and r["mask"] is None
        e.gp_set_i8_tol(0.999)
        res.append((r, _score(e, z["U"])))
        e.close()
    for a, b in zip(*res):
        _same(a, b, "fallback")


def _de_round(monkeypatch, screen, ell):
    space = A.float_space(64)
    e = _engine(space, monkeypatch, screen, seed=5)
    npop, m, k, n = 512, 3000, 16, 300
    pop = ode.population_init(space, npop, seed=5)
    e.population_set(dev(pop))
    X = features(space, pop[:, :n]).T
    y = np.sum((X - 0.45) ** 2, axis=1)
    e.history_reset(0)
    e.gp_fit(X, y, lengthscale=ell, sigma_f2=1.0, sigma_n2=1e-6, jitter=1e-8, wait=False)
    idx, top, dig, vals = e.score_round_de(m, k, round_=1, cand_base=0, cr=0.3)
    e.sync()
    mk = e.gp_kstar_mask_read()
    assert mk is not None, "the round fell back to fp64 as a whole"
    out = (idx.cpu().numpy(), top.cpu().numpy(), dig.cpu().numpy(), vals.cpu().numpy(), mk.cpu().numpy())
    st = e.gp_kstar_screen_stats()
    e.close()
    return out, st


def test_same_topk_of_a_de_round(monkeypatch):
    """a dense DE round at ell = 0.05 behind gp_fit(wait=False): same top-k, digests and values"""
    (a, sa), (b, sb) = _de_round(monkeypatch, True, 0.05), _de_round(monkeypatch, False, 0.05)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    print("ell 0.05: certified %d of %d units" % sa[1:])
    assert sa[0] is True and sb[0] is False and sa[1] > 0


@pytest.mark.parametrize("which", ["far", "mixed"])
def test_posterior_against_the_oracle(monkeypatch, which):
    c, z = _table()
    U = np.tile(z["U"][96:128], (9, 1)) if which == "far" else z["U"]
    e = _engine(A.float_space(c["d"]), monkeypatch, True)
    e.gp_fit(z["X"], z["y"], lengthscale=z["ell"], **MC.hyper(c["sf2"]))
    r = _score(e, U)
    e.close()
    assert r["screen"][0] is True and r["screen"][1] > 0
    h = MC.hyper(c["sf2"])
    g = ogp.GP(z["X"], z["y"], lengthscale=1.0, sigma_f2=h["sigma_f2"], sigma_n2=h["sigma_n2"], jitter=h["jitter"])
    mu_o, var_o = g.posterior(U)
    np.testing.assert_allclose(r["mu"], mu_o, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(r["var"], var_o, rtol=1e-5, atol=1e-8 * c["sf2"])
