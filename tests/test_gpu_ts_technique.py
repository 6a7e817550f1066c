"""acq="ts" on the techniques: a dense GP round draws `batch` posterior sample
paths (ut_gp_ts_draw) and takes one pick per path (ut_gp_ts_select).  The
driver setting of test_gpu_tr_technique.py: 2-D Rosenbrock on [-2, 2]^2, pool
4096, batch 8, 12 seeded results."""
import numpy as np
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

KW = dict(pool=4096, batch=8, population=256, seed=3, lengthscale=0.3)


def _space():
    from uptune_amd.manipulator import ConfigurationManipulator, FloatParameter
    return ConfigurationManipulator([FloatParameter("x0", -2.0, 2.0), FloatParameter("x1", -2.0, 2.0)])


def _rosen(cfg):
    return 100.0 * (cfg["x1"] - cfg["x0"] ** 2) ** 2 + (cfg["x0"] - 1.0) ** 2


def _drive(tech, rounds=5, seeded=12, parallelism=8):
    from uptune_amd.driver import SearchDriver
    from uptune_amd.tuner import random_configs
    m = _space()
    d = SearchDriver(m, tech, parallelism=parallelism)
    cfgs, keys = random_configs(m, seeded, 101, 0, with_keys=True)
    d.seed_results(cfgs, _rosen, keys=keys)
    d.main(_rosen, test_limit=10 ** 6, max_generations=rounds)
    return d


def _recording(base):
    class Recording(base):
        def after_round(self, idx, hexes):
            super().after_round(idx, hexes)
            self.seen = getattr(self, "seen", []) + [list(hexes)]

        def _ts_picks(self, *a):
            self.ts_calls = getattr(self, "ts_calls", 0) + 1
            return super()._ts_picks(*a)
    return Recording


def _classes():
    from uptune_amd import technique as T
    return {"de": T.GpuDifferentialEvolution, "tr": T.GpuTrustRegion}


@pytest.mark.parametrize("which", ["de", "tr"])
def test_rounds_hand_on_distinct_new_configurations(which):
    cls = _recording(_classes()[which])
    d = _drive(cls(acq="ts", ts_features=256, name="ts", **KW))
    t = d.root_technique
    assert len(t.seen) == 5 and t.ts_calls == 5 and t.model.ts_rounds == 5
    known = set(d.seen_hashes()[:12])
    for hx in t.seen:
        assert len(hx) == 8 and len(set(hx)) == 8 and not (set(hx) & known)    # batch distinct, none seen before
        known |= set(hx)
    assert len(d.results) == len(d.seen_hashes()) == 12 + 40
    # the same seeds, the same sequence
    d2 = _drive(cls(acq="ts", ts_features=256, name="ts", **KW))
    assert list(d2.results.keys()) == list(d.results.keys())
    # ... and not EI's
    d3 = _drive(cls(acq="ei", name="ts", **KW))
    assert getattr(d3.root_technique, "ts_calls", 0) == 0 and d3.root_technique.model.ts_rounds == 0
    assert list(d3.results.keys()) != list(d.results.keys())


def test_ei_runs_are_unchanged():
    """acq="ei" spelled out, or with a ts_features it never reads: the sequence of the default"""
    from uptune_amd import technique as T
    a = _drive(T.GpuDifferentialEvolution(name="de", **KW), rounds=3)
    b = _drive(T.GpuDifferentialEvolution(name="de", acq="ei", ts_features=512, **KW), rounds=3)
    assert list(a.results.keys()) == list(b.results.keys())
    assert [r.time for r in a.results.values()] == [r.time for r in b.results.values()]


def test_bandit_with_the_arm_draws_on_one_counter():
    from uptune_amd import technique as T
    meta = T.bandit_a(bandit_seed=1, trust_region=True, acq="ts", ts_features=128, pool=1024, batch=4,
                      population=64, seed=2)
    d = _drive(meta, rounds=5, parallelism=4)
    arms = d.root_technique.techniques
    assert len(arms) == 4 and isinstance(arms[-1], T.GpuTrustRegion)
    assert all(t.model is arms[0].model and t.acq_kind == "ts" for t in arms)
    assert arms[0].model.ts_rounds == sum(t.round for t in arms) > 0     # every GP round drew, each under its own key
    assert len(d.results) == len(d.seen_hashes()) > 12 + 4
    assert any(r.requestor == "gpu-trust-region" for r in d.results.values())


def test_tune_bandit_passes_the_acquisition():
    from uptune_amd.tuner import tune_bandit
    kw = dict(generations=3, parallelism=4, n_init=8, pool=1024, batch=4, population=64)
    a = tune_bandit(_space(), _rosen, **kw)
    b = tune_bandit(_space(), _rosen, acq="ei", **kw)
    assert list(a.results.keys()) == list(b.results.keys()) and len(a.results) > 8
    c = tune_bandit(_space(), _rosen, acq="ts", ts_features=128, trust_region=True, **kw)
    assert all(t.acq_kind == "ts" and t.ts_features == 128 for t in c.root_technique.techniques)
    assert c.root_technique.techniques[0].model.ts_rounds > 0
    assert len(c.results) == len(c.seen_hashes()) and len(c.results) > 8
