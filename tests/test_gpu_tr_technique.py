"""GpuTrustRegion: rounds proposed inside a box around a centre (ut_propose_tr),
sized by trust_region.TrustRegion from the outcome of the rounds before.  The
driver setting of test_gpu_polish_technique.py: 2-D Rosenbrock on [-2, 2]^2,
pool 4096, batch 8, 12 seeded results."""
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


def _driver(tech, seeded=12):
    from uptune_amd.driver import SearchDriver
    from uptune_amd.tuner import random_configs
    m = _space()
    d = SearchDriver(m, tech, parallelism=8)
    if seeded:
        cfgs, keys = random_configs(m, seeded, 101, 0, with_keys=True)
        d.seed_results(cfgs, _rosen, keys=keys)
    return d


def _drive(tech, rounds=6, seeded=12):
    d = _driver(tech, seeded)
    d.main(_rosen, test_limit=10 ** 6, max_generations=rounds)
    return d


def _recording():
    from uptune_amd import technique as T

    class Recording(T.GpuTrustRegion):
        def propose(self, m):
            vals, inv = super().propose(m)
            self.seen = getattr(self, "seen", []) + [dict(
                round=self.round, uniform=self.last_uniform, L=self.tr.L, vals=vals.cpu().numpy(),
                inv=None if inv is None else inv.cpu().numpy(),
                centre=None if self.last_uniform else self.last_centre.copy(),
                half=None if self.last_uniform else self.last_half.copy())]
            return vals, inv

        def after_round(self, idx, hexes):
            super().after_round(idx, hexes)
            self.seen[-1]["hexes"] = list(hexes)
    return Recording


def _unit(v):
    return (v + 2.0) / 4.0


@pytest.mark.parametrize("centre", ["best", "own"])
def test_rounds_hand_on_distinct_new_configurations_inside_the_box(centre):
    d = _drive(_recording()(centre=centre, name="tr", **KW))
    t = d.root_technique
    seen = t.seen
    assert len(seen) == 6
    known = set(d.seen_hashes()[:12])
    for r in seen:
        hx = r["hexes"]
        assert len(hx) == 8 and len(set(hx)) == 8 and not (set(hx) & known)   # 8 distinct, none seen before
        known |= set(hx)
        assert (r["vals"] >= -2.0).all() and (r["vals"] <= 2.0).all()
        if not r["uniform"]:
            # every proposed row lies within the half-widths of the centre in unit space (ulps of rounding
            # from the unit value back to the stored one: 4 * 2^-52 on [-2, 2])
            du = np.abs(_unit(r["vals"]) - _unit(r["centre"])[:, None])
            assert (du <= r["half"][:, None] + 1e-15).all()
            assert (r["half"] == r["L"] / 2.0).all()
    assert len(d.results) == len(d.seen_hashes()) == 12 + 48
    # "best" has a centre from the seeded results on; "own" starts with one uniform round
    assert [r["uniform"] for r in seen] == [centre == "own"] + [False] * 5
    if centre == "best":
        best = d.results[d.seen_hashes()[0]]
        for k in d.seen_hashes()[:12]:
            if d.results[k].time < best.time:
                best = d.results[k]
        np.testing.assert_array_equal(seen[0]["centre"], [best.configuration.data["x0"], best.configuration.data["x1"]])
    # the box moved with the results: a later centre is a row this technique proposed
    assert any((seen[k]["centre"] != seen[1]["centre"]).any() for k in range(2, 6))
    if centre == "best":    # (an own centre starts from a uniform round's best, not from the seeded results)
        assert d.best_result.time < min(d.results[k].time for k in d.seen_hashes()[:12])


def test_without_results_the_first_round_is_uniform():
    d = _drive(_recording()(name="tr", **KW), rounds=2, seeded=0)
    seen = d.root_technique.seen
    assert [r["uniform"] for r in seen] == [True, False]
    # uniform rows fill the space, box rows do not
    assert np.ptp(seen[0]["vals"], axis=1).min() > 3.9
    assert len(d.results) == len(d.seen_hashes()) == 16


def test_collapse_restarts_and_own_centre_goes_uniform():
    tech = _recording()(centre="own", name="tr", fail_tol=1, **KW)
    d = _driver(tech)
    t = d.root_technique

    def worse(cfg):
        return 1e9 + _rosen(cfg)

    d.main(_rosen, test_limit=10 ** 6, max_generations=2)     # a uniform round, then a box round
    assert [r["uniform"] for r in t.seen] == [True, False] and t.tr.restarts == 0
    t.tr.L = t.tr.L_min                                         # one failed round from collapse
    d.main(worse, test_limit=10 ** 6, max_generations=4)      # round 2 fails ...
    seen = t.seen
    assert len(seen) == 4
    # round 1 or round 2 is the first to fail (everything measured from now on is worse): the failure halves
    # L below L_min, the region restarts at L_init, and the round that follows is a uniform one
    k = next(i for i in (2, 3) if seen[i]["uniform"])
    assert t.tr.restarts == 1 and seen[k]["L"] == t.tr.L_init
    assert all(not seen[i]["uniform"] and seen[i]["L"] == t.tr.L_min for i in range(2, k))
    assert np.ptp(seen[k]["vals"], axis=1).min() > 3.9
    if k == 2:      # ... and its best result is the next centre, however bad
        assert not seen[3]["uniform"] and seen[3]["L"] == t.tr.L_init
        own = min((d.results[h] for h in seen[2]["hexes"]), key=lambda r: r.time)
        np.testing.assert_array_equal(seen[3]["centre"], [own.configuration.data["x0"], own.configuration.data["x1"]])
    assert len(d.results) == len(d.seen_hashes())


def test_best_centre_restart_keeps_the_box():
    tech = _recording()(centre="best", name="tr", fail_tol=1, **KW)
    d = _driver(tech)
    t = d.root_technique
    d.main(_rosen, test_limit=10 ** 6, max_generations=1)
    t.tr.L = t.tr.L_min
    d.main(lambda cfg: 1e9 + _rosen(cfg), test_limit=10 ** 6, max_generations=4)
    # rounds 1 .. 3 all fail; the first failure collapses the region, the later ones halve it again
    assert len(t.seen) == 4 and t.tr.restarts == 1 and not any(r["uniform"] for r in t.seen)
    assert t.seen[-1]["L"] in (t.tr.L_init / 2, t.tr.L_init / 4)


def test_bandit_a_with_the_arm_runs_on_one_model():
    from uptune_amd import technique as T
    meta = T.bandit_a(bandit_seed=1, trust_region=True, pool=1024, batch=4, population=64, seed=2)
    d = _driver(meta)
    d.parallelism = 4
    d.main(_rosen, test_limit=10 ** 6, max_generations=3)
    arms = d.root_technique.techniques
    assert len(arms) == 4 and isinstance(arms[-1], T.GpuTrustRegion)
    assert all(t.model is arms[0].model for t in arms)
    assert len(d.results) == len(d.seen_hashes()) > 12 + 4
    assert any(r.requestor == "gpu-trust-region" for r in d.results.values())


def test_tune_bandit_arm_is_opt_in():
    from uptune_amd import technique as T
    from uptune_amd.tuner import tune_bandit
    kw = dict(generations=3, parallelism=4, n_init=8, pool=1024, batch=4, population=64)
    a = tune_bandit(_space(), _rosen, **kw)
    b = tune_bandit(_space(), _rosen, trust_region=False, **kw)
    assert list(a.results.keys()) == list(b.results.keys()) and len(a.results) > 8
    assert [type(t) for t in a.root_technique.techniques] == [T.GpuPSO, T.GpuGA, T.GpuDifferentialEvolution, T.GpuGGA]
    c = tune_bandit(_space(), _rosen, trust_region=True, **kw)
    arms = c.root_technique.techniques
    assert len(arms) == 5 and isinstance(arms[-1], T.GpuTrustRegion) and arms[-1].name == "gpu-trust-region"
    assert all(t.model is arms[0].model for t in arms)
    assert len(c.results) == len(c.seen_hashes()) and len(c.results) > 8
    # the arm was asked (the bandit tries every arm once) and its requests were evaluated
    assert any(r.requestor == "gpu-trust-region" for r in c.results.values())
