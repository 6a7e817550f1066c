"""Every instance of the column-sum K* kernel (gp_kstar_sums.hip) through the
public entry points: the constraint means at nc = 1, 2, 3, 4 (one to four
weighted sums per column) and the failure vote with ell_scale != 1 (one plain
sum, the scaled exponent, two row sets), each on a numeric fit (the dense
contraction) and on a categorical one (the int8 code product) -- ten kernels.

The shape is the smallest at which the item arithmetic can go wrong: n = 129
training rows (two row tiles, the second with one live row), 130 failed rows
(two more tiles of the same launch), m = 130 candidates (two column tiles);
d = 5, or the mixed space of test_categorical_operands.

Restatements and tolerances are the ones tests/test_gpu_cons.py and
tests/test_gpu_feas.py hold the same quantities to: mu_c at rtol 1e-5 / atol
1e-9, P from the device's own var and mu_c at rtol 1e-10, the vote's p, S_ok
and S_fail at rtol 1e-5 / atol 1e-12."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from _cons_oracle import ConsGP, cons_prob  # noqa: E402
from _feas_oracle import feas_prob  # noqa: E402
from _spaces import to_manip  # noqa: E402
from oracle.space import features  # noqa: E402
from test_gpu_cons import HYPER, MIXED, close as cons_close, cons_values, fspace, tail_close  # noqa: E402
from test_gpu_feas import close as feas_close  # noqa: E402

N, NF, M, D = 129, 130, 130, 5


@pytest.mark.parametrize("kind", ["numeric", "categorical"])
def test_every_instance(monkeypatch, kind):
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from uptune_amd.engine import BatchEngine
    monkeypatch.setenv("UT_CAT_KSTAR", "1")
    space = MIXED if kind == "categorical" else fspace(D)
    e = BatchEngine(to_manip(space), device=0, seed=3)
    try:
        e.population_init(1024, round_=0)
        vals = e.population_get().contiguous()
        feat = features(space, vals.cpu().numpy()).T
        X, F, U = feat[:N], feat[N:N + NF], feat[N + NF:N + NF + M]
        V = vals[:, N + NF:N + NF + M].contiguous()
        Ud = torch.from_numpy(np.ascontiguousarray(U.T)).to("cuda:0")
        rng = np.random.default_rng(17)
        y, C = rng.standard_normal(N), cons_values(X, 4, rng)
        ell = 1.2 if kind == "categorical" else 0.5
        e.gp_fit(X, y, lengthscale=ell, wait=True, **HYPER)
        assert e.gp_kstar_mode() == ("categorical" if kind == "categorical" else "dense")
        var = e.gp_score_values(V)[1].cpu().numpy()

        # the means: nc weighted sums per column, one row set
        for nc in (1, 2, 3, 4):
            thr = np.median(C[:, :nc], axis=0)
            e.gp_cons_set(np.ascontiguousarray(C[:, :nc]), thr)
            g = ConsGP(X, y, C[:, :nc], thr, ell, **HYPER)
            w_mc = g.mu_c(U)
            P, mu_c = [t.cpu().numpy() for t in e.gp_cons_prob(values=V)]
            Pf, mu_cf = [t.cpu().numpy() for t in e.gp_cons_prob(features=Ud)]
            print("%s nc %d: max |mu_c diff| %.3g / %.3g (|mu_c| <= %.3g)" % (
                kind, nc, np.abs(mu_c - w_mc).max(), np.abs(mu_cf - w_mc).max(), np.abs(w_mc).max()))
            assert mu_c.shape == (nc, M)
            cons_close(mu_c, w_mc, "mu_c, values, nc %d" % nc)
            cons_close(mu_cf, w_mc, "mu_c, features, nc %d" % nc)
            tail_close(P, cons_prob(var, mu_c, g.tau), "P, nc %d" % nc)
        e.gp_cons_clear()

        # the vote: one plain sum per column, the exponent scaled, the failed rows as the second row set
        for s in (0.5, 2.0):
            e.gp_feas_set(F, strength=0.01, ell_scale=s)
            want = feas_prob(X, F, U, ell, strength=0.01, ell_scale=s)
            a = [t.cpu().numpy() for t in e.gp_feas_prob(values=V)]
            b = [t.cpu().numpy() for t in e.gp_feas_prob(features=Ud)]
            for g1, g2, w, name in zip(a, b, want, ("p", "S_ok", "S_fail")):
                print("%s ell_scale %g %s: max rel diff %.3g / %.3g" % (
                    kind, s, name, np.max(np.abs(g1 - w) / np.maximum(np.abs(w), 1e-300)),
                    np.max(np.abs(g2 - w) / np.maximum(np.abs(w), 1e-300))))
                feas_close(g1, w, "%s, values, ell_scale %g" % (name, s))
                feas_close(g2, w, "%s, features, ell_scale %g" % (name, s))
    finally:
        e.close()
