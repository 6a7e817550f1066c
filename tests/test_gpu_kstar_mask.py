"""K*'s plane-occupancy mask (k_gp_kstar_q, gp_kq.hip) and the variance contraction
that skips all-zero digit planes by it (k_gp_var_i8<true>, gp_i8.hip), on the
structured-sparsity table of tests/_kstar_mask_cases.py
(test_kstar_mask_cpu.py shows that the table holds every mask class):

  the mask read back (ut_gp_kstar_mask_read) equals, byte for byte and padding
  included, the mask recomputed from the planes read back (ut_gp_kstar_read);
  the planes meet the extended-precision reference at the element tolerance, and
  every element the restatement puts below 2^-49 of the scale is exactly 0;
  with and without the variance skip (UT_VAR_SKIP=0) every output is the same
  bits: mean, variance, EI, the per-tile partials, the recompute count, and the
  top-k of a dense DE round;
  an all-zero K* gives var == sf2 and the prior mean exactly, nothing recomputed;
  planes without a mask (UT_KSTAR_Q=0, a categorical fit, the whole-round fp64
  fallback) report none and score as UT_VAR_SKIP=0 does;
  one case per n against oracle/gp.py at 1e-5."""
import os
import sys

import numpy as np
import pytest
import torch

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

pytestmark = pytest.mark.gpu

import _ard_cases as A  # noqa: E402
import _kstar_cases as KC  # noqa: E402
import _kstar_mask_cases as MC  # noqa: E402
from _spaces import to_manip  # noqa: E402
from oracle import de as ode  # noqa: E402
from oracle import gp as ogp  # noqa: E402
from oracle.space import features  # noqa: E402


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")


def _engine(space, monkeypatch, var_skip=True, kstar_q=True, tol=None, seed=0):
    """var_skip True / False: UT_VAR_SKIP=1 / 0, the masked / the unmasked variance kernel whatever the
    last call's K* looked like; None: unset, the library's own choice between the two"""
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    monkeypatch.setenv("UT_KSTAR_Q", "1" if kstar_q else "0")     # (read when the context is created)
    if var_skip is None:
        monkeypatch.delenv("UT_VAR_SKIP", raising=False)
    else:
        monkeypatch.setenv("UT_VAR_SKIP", "1" if var_skip else "0")   # (read per call)
    from uptune_amd.engine import BatchEngine
    e = BatchEngine(to_manip(space), device=0, seed=seed)
    e.gp_set_precision(8)
    if tol is not None:
        e.gp_set_i8_tol(tol)
    return e


_RUNS = {}


def _run(monkeypatch, c, var_skip=True, tol=None):
    """one scoring of case c -> dict of host arrays; computed once per configuration"""
    key = (c["name"], var_skip, tol)
    if key not in _RUNS:
        z = MC.data(c)
        e = _engine(A.float_space(c["d"]), monkeypatch, var_skip, tol=tol)
        e.gp_fit(z["X"], z["y"], lengthscale=z["ell"], wait=not c["fit_async"], **MC.hyper(c["sf2"]))
        if z["pre"] is not None:
            e.gp_score(dev(z["pre"].T))
        mu, var, sc = e.gp_score(dev(z["U"].T))
        out = dict(mu=mu.cpu().numpy(), var=var.cpu().numpy(), score=sc.cpu().numpy(), stats=e.gp_i8_stats())
        kd, npad, ldk, fmt = e.gp_kstar_read()
        out.update(k=kd.cpu().numpy(), npad=npad, ldk=ldk, fmt=fmt)
        mk = e.gp_kstar_mask_read()
        out["mask"] = None if mk is None else mk.cpu().numpy()
        if fmt == 8:
            vp, mp = e.gp_i8_parts_read()
            out["var_part"], out["mu_part"] = vp.cpu().numpy()[:, :c["m"]], mp.cpu().numpy()[:, :c["m"]]
        e.close()
        _RUNS[key] = out
    return _RUNS[key]


@pytest.mark.parametrize("c", MC.CASES, ids=MC.ids())
def test_mask_equals_the_planes(monkeypatch, c):
    r = _run(monkeypatch, c, tol=0.999)    # (0.999: no whole-round fp64 fallback rewrites K*)
    assert r["fmt"] == 8 and r["stats"][0] != -1
    assert (r["npad"], r["ldk"]) == (KC.npad_of(c["n"]), KC.ldk_of(c["m"]))
    assert r["mask"] is not None and r["mask"].shape == (r["npad"] // 32, r["ldk"] // 32)
    want = MC.mask_of(r["k"], c["sf2"])
    bad = np.argwhere(r["mask"] != want)
    assert bad.size == 0, "%s: mask differs from the planes at blocks %s ..." % (c["name"], bad[:4].tolist())
    nrb, ncb = (c["n"] + 31) // 32, (c["m"] + 31) // 32
    assert not r["mask"][nrb:].any() and not r["mask"][:, ncb:].any()
    # (against the restatement's mask, whose classes test_kstar_mask_cpu.py counts: a block whose
    # largest element sits at a digit boundary may differ by a rounding; printed, not asserted --
    # test_planes_against_the_restatement holds the planes themselves to the restatement)
    differ = np.count_nonzero(r["mask"] != MC.expected_mask(c))
    print("%s: %d blocks, %d with a plane, %d differ from the restatement's" %
          (c["name"], want.size, np.count_nonzero(want), differ))


@pytest.mark.parametrize("c", MC.CASES, ids=MC.ids())
def test_planes_against_the_restatement(monkeypatch, c):
    a = _run(monkeypatch, c, tol=0.999)
    t, k = MC.restate(c)
    n, m = c["n"], c["m"]
    s0 = c["sf2"] * 2.0 ** -KC.i8_kstar_exp(c["sf2"])
    below = t < 256.0 * (-49.0 - np.log2(s0)) - 1.0    # below 2^-49 of the scale (1 t unit: 0.3 %, clear of any rounding)
    assert not np.any(a["k"][:n, :m][below] != 0.0)
    # the planes against the extended-precision reference at the element tolerance, as
    # test_gpu_kstar_elements.py holds them
    z = MC.data(c)
    k_ref = KC.reference(z["X"], z["U"], z["ell"], c["sf2"])
    tol = KC.tolerance(z["X"], z["U"], z["ell"], c["sf2"], "q", k_ref)
    w, (r, col) = KC.worst(a["k"][:n, :m], k_ref, tol)
    print("%s: worst element %.3g of the tolerance at (%d, %d)" % (c["name"], w, r, col))
    assert w <= 1.0


@pytest.mark.parametrize("tol", [None, 0.999], ids=["default_tol", "tol0.999"])
@pytest.mark.parametrize("c", MC.CASES, ids=MC.ids())
def test_var_skip_changes_no_bit(monkeypatch, c, tol):
    a = _run(monkeypatch, c, tol=tol)
    b = _run(monkeypatch, c, var_skip=False, tol=tol)
    assert a["stats"] == b["stats"] and a["fmt"] == b["fmt"]
    for key in ("mu", "var", "score", "k") + (("var_part", "mu_part") if a["fmt"] == 8 else ()):
        assert np.array_equal(a[key], b[key]), "%s: %s differs with the variance skip" % (c["name"], key)
    assert np.all(np.isfinite(a["mu"])) and np.all(a["var"] >= 0.0)


def _de_round(monkeypatch, var_skip, ell):
    space = A.float_space(64)
    e = _engine(space, monkeypatch, var_skip, seed=5)
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
    e.close()
    return out


@pytest.mark.parametrize("ell", [0.05, 0.4], ids=["ell0.05", "ell0.4"])
def test_var_skip_same_topk_of_a_de_round(monkeypatch, ell):
    """a dense DE round at a lengthscale where most (0.05: nearly all) of K* underflows"""
    a = _de_round(monkeypatch, True, ell)
    b = _de_round(monkeypatch, False, ell)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    print("ell %g: %d of %d blocks with a plane" % (ell, np.count_nonzero(a[4]), a[4].size))
    assert np.count_nonzero(a[4] != 0x3f) > 0


@pytest.mark.parametrize("n,m", [(129, 300), (1000, 129)])
def test_all_zero_kstar(monkeypatch, n, m):
    """ell = 0.01: every k* underflows; var == sf2 and the mean the prior's, exactly"""
    rng = np.random.default_rng(11)
    X, U = rng.uniform(size=(n, 8)), rng.uniform(size=(m, 8))
    y = rng.standard_normal(n)
    sf2 = 37.0
    res = []
    for var_skip in (True, False):
        e = _engine(A.float_space(8), monkeypatch, var_skip)
        e.gp_fit(X, y, lengthscale=0.01, sigma_f2=sf2, sigma_n2=1e-6 * sf2, jitter=0.0)
        mu, var, sc = e.gp_score(dev(U.T))
        res.append((mu.cpu().numpy(), var.cpu().numpy(), sc.cpu().numpy(), e.gp_i8_stats()[0],
                    e.gp_kstar_mask_read().cpu().numpy(), e.gp_kstar_read()[0].cpu().numpy()))
        e.close()
    (mu, var, sc, rec, mk, k), b = res
    assert not mk.any() and not k.any() and rec == 0
    assert np.all(var == sf2) and np.all(mu == 0.0)
    g = ogp.GP(X, y, lengthscale=0.01, sigma_f2=sf2, sigma_n2=1e-6 * sf2, jitter=0.0)
    mu_o, var_o = g.posterior(U)
    np.testing.assert_allclose(var, var_o, rtol=1e-12)
    np.testing.assert_allclose(mu, mu_o, rtol=1e-12, atol=1e-12)
    for x, y2 in zip(res[0], b):
        assert np.array_equal(x, y2)


def test_planes_without_a_mask(monkeypatch):
    """one context: a masked call, then the writers that leave no mask, then a masked
    call again whose mask is its own and not a stale one"""
    from uptune_amd._lib import UthotError
    c = MC.CASES[3]
    z = MC.data(c)
    far = np.tile(z["U"][96:128], (4, 1))          # the 'far' block: an all-zero mask
    e = _engine(A.float_space(c["d"]), monkeypatch)
    with pytest.raises(UthotError, match="no precision-8 dense scoring call"):
        e.gp_kstar_mask_read()
    e.gp_fit(z["X"], z["y"], lengthscale=z["ell"], **MC.hyper(c["sf2"]))
    e.gp_score(dev(far.T))
    assert not e.gp_kstar_mask_read().cpu().numpy().any()
    e.gp_set_i8_tol(0.0)                            # the whole round falls back to fp64: kst rewritten
    mu64, var64, _ = e.gp_score(dev(z["U"].T))
    assert e.gp_i8_stats()[0] == -1 and e.gp_kstar_read()[3] == 64 and e.gp_kstar_mask_read() is None
    e.gp_set_i8_tol(0.999)
    mu, var, _ = e.gp_score(dev(z["U"].T))
    k, mk = e.gp_kstar_read()[0].cpu().numpy(), e.gp_kstar_mask_read().cpu().numpy()
    e.close()
    assert np.array_equal(mk, MC.mask_of(k, c["sf2"])) and mk.any()
    np.testing.assert_allclose(mu.cpu().numpy(), mu64.cpu().numpy(), rtol=1e-5, atol=1e-6)
    np.testing.assert_allclose(var.cpu().numpy(), var64.cpu().numpy(), rtol=1e-5, atol=1e-8 * c["sf2"])


def test_the_library_choice_changes_no_bit(monkeypatch):
    """UT_VAR_SKIP unset: the variance kernel follows the last call's K* (masked after a
    sparse one, unmasked after a dense one); a dense, a sparse, a dense and a sparse call
    on one context give what UT_VAR_SKIP=0 gives"""
    c = MC.CASES[8]
    z = MC.data(c)
    # m = 256 = ldk: no padded column; at ell 25 every k* is 0.7 .. 1 of sf2 (blocks 1 .. 7 of the
    # table: none of copies of one training row), so only the mask's last, partly padded row has zero planes
    near = np.concatenate([z["U"][32:256], z["U"][32:64]])
    res = []
    for var_skip in (None, False):
        e = _engine(A.float_space(c["d"]), monkeypatch, var_skip, tol=0.999)   # (no whole-round fp64 fallback)
        e.gp_fit(z["X"], z["y"], lengthscale=25.0, **MC.hyper(c["sf2"]))   # ell 25: every k* near sf2, no zero plane
        out = []
        for U in (near, z["U"], near, near):
            out += [x.cpu().numpy() for x in e.gp_score(dev(U.T))]
            out.append(e.gp_kstar_mask_read().cpu().numpy())
        e.gp_fit(z["X"], z["y"], lengthscale=z["ell"], **MC.hyper(c["sf2"]))  # ell 1: the table's sparsity
        for U in (z["U"], near, z["U"]):
            out += [x.cpu().numpy() for x in e.gp_score(dev(U.T))]
            out.append(e.gp_kstar_mask_read().cpu().numpy())
        res.append(out)
        e.close()
    for x, y in zip(*res):
        assert np.array_equal(x, y)
    npad_blocks = 1024 // 32
    # the first call's K* is dense by the library's own measure, the last one sparse
    assert np.count_nonzero(res[0][3] != 0x3f) * 16 < res[0][3].size and np.any(res[0][-1][:npad_blocks] == 0)


@pytest.mark.parametrize("which", ["kstar_q0", "categorical"])
def test_other_plane_writers_keep_the_dense_path(monkeypatch, which):
    """k_gp_kstar<int8_t> (UT_KSTAR_Q=0, categorical fits) writes planes and no mask:
    the mask read reports none and the results are UT_VAR_SKIP=0's"""
    res = []
    for var_skip in (True, False):
        if which == "categorical":
            z, c = KC.cat_data(), KC.CAT
            e = _engine(z["space"], monkeypatch, var_skip, tol=0.999)
            e.gp_fit(z["X"], z["y"], lengthscale=z["ell"], **MC.hyper(c["sf2"]))
            out = e.gp_score_values(dev(z["cand"]))
        else:
            c = MC.CASES[3]
            z = MC.data(c)
            e = _engine(A.float_space(c["d"]), monkeypatch, var_skip, kstar_q=False, tol=0.999)
            e.gp_fit(z["X"], z["y"], lengthscale=z["ell"], **MC.hyper(c["sf2"]))
            out = e.gp_score(dev(z["U"].T))
        assert e.gp_kstar_read()[3] == 8 and e.gp_kstar_mask_read() is None
        res.append([x.cpu().numpy() for x in out])
        e.close()
    for x, y in zip(*res):
        assert np.array_equal(x, y)


@pytest.mark.parametrize("c", [MC.CASES[1], MC.CASES[3], MC.CASES[8], MC.CASES[11]],
                         ids=lambda c: c["name"])
def test_posterior_against_the_oracle(monkeypatch, c):
    """one case per n against oracle/gp.py at 1e-5, as the neighbouring tests do"""
    r = _run(monkeypatch, c)
    z = MC.data(c)
    h = MC.hyper(c["sf2"])
    g = ogp.GP(z["X"], z["y"], lengthscale=1.0, sigma_f2=h["sigma_f2"], sigma_n2=h["sigma_n2"], jitter=h["jitter"])
    mu_o, var_o = g.posterior(z["U"])
    np.testing.assert_allclose(r["mu"], mu_o, rtol=1e-5, atol=1e-5)
    np.testing.assert_allclose(r["var"], var_o, rtol=1e-5, atol=1e-8 * c["sf2"])
