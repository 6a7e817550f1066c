"""Every K* kernel of the fp64 tier held to an extended-precision K*, element
by element: k_gp_kstar_q (precision 8, the default), k_gp_kstar<int8_t>
(precision 8, UT_KSTAR_Q=0) and k_gp_kstar<double> (precision 64) score each
case of tests/_kstar_cases.py, the K* they left behind is read back
(ut_gp_kstar_read) and

  |k - k_ref| <= tol   for every r < n, c < m   (the tolerance derived in
                                                 _kstar_cases.py, per element)
  k == 0 exactly       for every r >= n or c >= m, up to npad and ldk
                       (the int8 variance contraction reads these without a mask)

The worst element's (r, c), error / tolerance and eb_c are printed, and
reported on failure.  One categorical case takes the int8 code-product stages
of k_gp_kstar through gp_score_values.  The posterior stays with
test_gp_vs_oracle / test_gpu_i8.py / test_gpu_ard_scoring.py (1e-5) and the two
precision-8 kernels against each other with test_gpu_kstar_q.py (1e-9)."""
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
from _spaces import to_manip  # noqa: E402

PREC = {"q": 8, "i8": 8, "f64": 64}


def _engine(space, kernel, monkeypatch, tol=0.999):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    monkeypatch.setenv("UT_KSTAR_Q", "1" if kernel == "q" else "0")   # (read when the context is created)
    from uptune_amd.engine import BatchEngine
    e = BatchEngine(to_manip(space), device=0, seed=0)
    e.gp_set_precision(PREC[kernel])
    if PREC[kernel] == 8:
        e.gp_set_i8_tol(tol)     # (0.999: no whole-round fp64 fallback rewrites K*)
    return e


def dev(a):
    return torch.from_numpy(np.array(a, order="C")).to("cuda:0")


def _hyper(sf2):
    # (K* does not see the noise; a large one keeps every fit positive definite and the
    # precision-8 bound test from flagging the candidates that sit on training rows)
    return dict(sigma_f2=sf2, sigma_n2=0.25 * sf2, jitter=0.0)


def _held(name, kernel, k, n, m, sf2, k_ref, tol, eb):
    """the element checks of one read-out k [npad][ldk]"""
    w, (r, c) = KC.worst(k[:n, :m], k_ref, tol)
    print("%s %s: worst element %.3g of the tolerance at (%d, %d), k %.17g, reference %.17g, eb_c %d"
          % (name, kernel, w, r, c, k[r, c], float(k_ref[r, c]), eb[c]))
    assert w <= 1.0, ("%s %s: |k - k_ref| is %.3g of the tolerance at row %d, column %d (eb_c %d)"
                      % (name, kernel, w, r, c, eb[c]))
    store = 0.0 if kernel == "f64" else 2.0 ** (-49 + KC.i8_kstar_exp(sf2))
    assert np.all(k[:n, :m] <= sf2 + store) and np.all(k[:n, :m] >= 0.0)
    bad = np.argwhere((k != 0.0) & ((np.arange(k.shape[0]) >= n)[:, None] | (np.arange(k.shape[1]) >= m)[None, :]))
    assert bad.size == 0, "%s %s: padding not zero at %s ..." % (name, kernel, bad[:4].tolist())
    return w


@pytest.mark.parametrize("kernel", KC.KERNELS)
@pytest.mark.parametrize("c", KC.CASES, ids=KC.ids())
def test_kstar_elements(monkeypatch, c, kernel):
    z = KC.data(c)
    n, m, sf2 = c["n"], c["m"], c["sf2"]
    e = _engine(A.float_space(c["d"]), kernel, monkeypatch)
    e.gp_fit(z["X"], z["y"], lengthscale=z["ell"], wait=not c["fit_async"], **_hyper(sf2))
    if z["pre"] is not None:
        e.gp_score(dev(z["pre"].T))
    e.gp_score(dev(z["U"].T))
    kd, npad, ldk, fmt = e.gp_kstar_read()
    k = kd.cpu().numpy()
    rec = e.gp_i8_stats()[0]
    mode = e.gp_kstar_mode()
    e.close()
    assert mode == "dense" and (npad, ldk) == (KC.npad_of(n), KC.ldk_of(m)) and k.shape == (npad, ldk)
    assert fmt == PREC[kernel] and rec != -1, "the whole-round fallback rewrote K* (recomputed %d)" % rec
    tol = KC.tolerance(z["X"], z["U"], z["ell"], sf2, kernel, z["k_ref"])
    _held(c["name"], kernel, k, n, m, sf2, z["k_ref"], tol, KC.operands(z["X"], z["U"], z["ell"])["eb"])


def test_kstar_read_after_the_fp64_fallback(monkeypatch):
    """precision 8 with nothing accepted (tolerance 0): the whole round is redone in
    fp64 and K* rewritten as fp64 rows; the read-out says so (format 64) and returns
    them, held to k_gp_kstar<double>'s tolerance"""
    c = KC.CASES[2]
    z = KC.data(c)
    e = _engine(A.float_space(c["d"]), "q", monkeypatch, tol=0.0)
    e.gp_fit(z["X"], z["y"], lengthscale=z["ell"], **_hyper(c["sf2"]))
    e.gp_score(dev(z["U"].T))
    kd, npad, ldk, fmt = e.gp_kstar_read()
    k, rec = kd.cpu().numpy(), e.gp_i8_stats()[0]
    e.close()
    assert rec == -1 and fmt == 64
    tol = KC.tolerance(z["X"], z["U"], z["ell"], c["sf2"], "f64", z["k_ref"])
    _held(c["name"], "f64", k, c["n"], c["m"], c["sf2"], z["k_ref"], tol,
          KC.operands(z["X"], z["U"], z["ell"])["eb"])


@pytest.mark.parametrize("kernel", ["f64", "i8"])
def test_kstar_elements_categorical(monkeypatch, kernel):
    """the int8 code-product stages of k_gp_kstar (ENUM / BOOL one-hot blocks as a
    match count) through gp_score_values, at precisions 64 and 8"""
    z, c = KC.cat_data(), KC.CAT
    e = _engine(z["space"], kernel, monkeypatch)
    e.gp_fit(z["X"], z["y"], lengthscale=z["ell"], **_hyper(c["sf2"]))
    e.gp_score_values(dev(z["cand"]))
    kd, npad, ldk, fmt = e.gp_kstar_read()
    k, mode = kd.cpu().numpy(), e.gp_kstar_mode()
    e.close()
    assert mode == "categorical" and fmt == PREC[kernel]
    tol = KC.tolerance(z["X"], z["U"], z["ell"], c["sf2"], kernel, z["k_ref"])
    _held(c["name"], kernel, k, c["n"], c["m"], c["sf2"], z["k_ref"], tol,
          np.zeros(c["m"], dtype=np.int64))


def test_kstar_read_argument_errors(monkeypatch):
    """UT_EINVAL with nothing to read (no dense call since the last fit, a pruned call
    since) or a bad range, UT_EUNSUPPORTED for the fp32 and f16x3 formats; a column
    range returns that part of the whole"""
    from uptune_amd._lib import UthotError
    e = _engine(A.float_space(3), "f64", monkeypatch)
    rng = np.random.default_rng(3)
    X, y, feat = rng.uniform(size=(40, 3)), rng.standard_normal(40), dev(rng.uniform(size=(3, 300)))
    with pytest.raises(UthotError, match="no dense scoring call"):
        e.gp_kstar_read()
    e.gp_fit(X, y, lengthscale=0.5)
    with pytest.raises(UthotError, match="no dense scoring call"):
        e.gp_kstar_read()
    e.gp_score(feat)
    k, npad, ldk, fmt = e.gp_kstar_read()
    assert (npad, ldk, fmt) == (128, 512, 64) and k.shape == (128, 512)
    part = e.gp_kstar_read(c0=250, nc=70)[0]
    assert part.shape == (128, 70) and torch.equal(part, k[:, 250:320])
    for c0, nc in ((-1, 4), (500, 13), (0, 513)):
        with pytest.raises(UthotError, match="columns outside"):
            e.gp_kstar_read(c0=c0, nc=nc)
    e.gp_topk_pruned(feat, 4, bound_rows=128)
    with pytest.raises(UthotError, match="no dense scoring call"):
        e.gp_kstar_read()
    e.gp_score(feat)
    e.gp_kstar_read()
    e.gp_fit(X, y, lengthscale=0.7)
    with pytest.raises(UthotError, match="no dense scoring call"):
        e.gp_kstar_read()
    for bits in (32, 16):
        e.gp_set_precision(bits)
        e.gp_fit(X, y, lengthscale=0.5)
        e.gp_score(feat)
        with pytest.raises(UthotError, match="UT_EUNSUPPORTED|not read out"):
            e.gp_kstar_read()
    e.close()
