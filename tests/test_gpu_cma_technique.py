"""GpuCMAES: rounds drawn from N(mean, sigma^2 C) (ut_propose_cma) with the state of
cma.CMAState told from the rounds' own evaluated results.  The driver setting of
test_gpu_tr_technique.py: 2-D Rosenbrock on [-2, 2]^2, batch 8, 12 seeded results."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

from test_gpu_tr_technique import _driver, _rosen, _space  # noqa: E402

KW = dict(pool=1024, batch=8, population=64, seed=3, lengthscale=0.3)


def test_runs_to_its_first_restart():
    from uptune_amd import technique as T
    # sigma_min = 2^-4: on this space the step falls below it within a few dozen generations
    d = _driver(T.GpuCMAES(name="cma", sigma_min=2.0 ** -4, **KW))
    t = d.root_technique
    for k in range(12):                    # (max_generations counts from the driver's start)
        d.main(_rosen, test_limit=10 ** 6, max_generations=5 * (k + 1))
        if t.cma is not None and t.cma.restarts:
            break
    assert t.cma.restarts >= 1 and t.cma.generation >= 2
    assert len(d.results) == len(d.seen_hashes()) > 12 + 16
    assert d.best_result.time < min(d.results[k].time for k in d.seen_hashes()[:12])
    vals = np.array([[r.configuration.data["x0"], r.configuration.data["x1"]] for r in d.results.values()])
    assert (vals >= -2.0).all() and (vals <= 2.0).all()


def test_without_preselection_every_request_is_a_row_of_the_pool():
    from uptune_amd import technique as T

    class Recording(T.GpuCMAES):
        def propose(self, m):
            vals, inv = super().propose(m)
            self.pools = getattr(self, "pools", []) + [vals.cpu().numpy()]
            return vals, inv

    d = _driver(Recording(name="cma", preselect=False, **KW))
    d.main(_rosen, test_limit=10 ** 6, max_generations=4)
    t = d.root_technique
    assert t.pool == 8 and all(p.shape == (2, 8) for p in t.pools) and not t.last_uniform
    rows = {tuple(c) for p in t.pools for c in p.T}
    asked = [r for r in d.results.values() if r.requestor == "cma"]
    assert len(asked) == 32 and all((r.configuration.data["x0"], r.configuration.data["x1"]) in rows for r in asked)
    assert t.cma.generation >= 2          # a round is told when the next one starts


def test_bandit_a_with_the_arm_runs_on_one_model():
    from uptune_amd import technique as T
    meta = T.bandit_a(bandit_seed=1, cma=True, pool=1024, batch=4, population=64, seed=2)
    d = _driver(meta)
    d.parallelism = 4
    d.main(_rosen, test_limit=10 ** 6, max_generations=4)
    arms = d.root_technique.techniques
    assert len(arms) == 4 and isinstance(arms[-1], T.GpuCMAES)
    assert all(t.model is arms[0].model for t in arms)
    assert len(d.results) == len(d.seen_hashes()) > 12 + 4
    assert any(r.requestor == "gpu-cma-es" for r in d.results.values())
