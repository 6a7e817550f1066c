"""GpuBatchTechnique(diversify=D): a round with a GP picks its batch from the D
best-scoring candidates with ut_gp_select_batch (each pick conditioned on the
picks before it) instead of taking the plain top-k.  2-D Rosenbrock, pool 4096,
batch 8, a few seeded results so that the first round already has a model."""
import pytest

torch = pytest.importorskip("torch")

pytestmark = pytest.mark.gpu

KW = dict(pool=4096, batch=8, population=256, seed=3, lengthscale=0.3)


def _space():
    from uptune_amd.manipulator import ConfigurationManipulator, FloatParameter
    return ConfigurationManipulator([FloatParameter("x0", -2.0, 2.0), FloatParameter("x1", -2.0, 2.0)])


def _rosen(cfg):
    return 100.0 * (cfg["x1"] - cfg["x0"] ** 2) ** 2 + (cfg["x0"] - 1.0) ** 2


def _drive(tech, rounds=3):
    from uptune_amd.driver import SearchDriver
    from uptune_amd.tuner import random_configs
    m = _space()
    d = SearchDriver(m, tech, parallelism=8)
    cfgs, keys = random_configs(m, 12, 101, 0, with_keys=True)
    d.seed_results(cfgs, _rosen, keys=keys)
    d.main(_rosen, test_limit=10 ** 6, max_generations=rounds)
    return d


def test_diversified_rounds_pick_from_the_plain_top():
    from uptune_amd import technique as T

    class Recording(T.GpuDifferentialEvolution):
        def _diverse_picks(self, vals, score, dup, dig, base):
            out = super()._diverse_picks(vals, score, dup, dig, base)
            plain = self.engine.topk(score, 64, dup=dup, cand_base=base)[0]
            self.seen = getattr(self, "seen", []) + [(out[1].cpu().tolist(), plain.cpu().tolist(),
                                                      out[4].cpu().numpy(), vals.cpu().numpy(), base)]
            return out

    d = _drive(Recording(diversify=64, name="de", **KW))
    seen = d.root_technique.seen
    assert len(seen) >= 3                      # every round had a model
    for idx, plain, rows, vals, base in seen:
        assert len(idx) == 8 and len(set(idx)) == 8 and min(idx) >= 0
        assert set(idx) <= set(plain)
        assert idx[0] == plain[0]
        for j, g in enumerate(idx):            # the rows returned are the picks' own
            assert (rows[:, j] == vals[:, g - base]).all()
    assert len(d.results) == len(d.seen_hashes())


def test_diversify_0_is_the_default_path():
    from uptune_amd import technique as T
    a = _drive(T.GpuDifferentialEvolution(name="de", **KW))
    b = _drive(T.GpuDifferentialEvolution(diversify=0, name="de", **KW))
    assert list(a.results.keys()) == list(b.results.keys()) and len(a.results) > 12
    c = _drive(T.GpuDifferentialEvolution(diversify=64, name="de", **KW))
    assert list(c.results.keys()) != list(a.results.keys())


def test_invalid_combinations_raise():
    from uptune_amd import technique as T
    with pytest.raises(ValueError):
        T.GpuDifferentialEvolution(diversify=64, prune_rows=128, **KW)
    with pytest.raises(ValueError):
        T.GpuDifferentialEvolution(diversify=64, surrogate=object(), **KW)
    with pytest.raises(ValueError):
        T.GpuDifferentialEvolution(diversify=4, **KW)          # < batch
    with pytest.raises(ValueError):
        T.GpuDifferentialEvolution(diversify=4097, **KW)

    class TwoRanks(T.GpuDifferentialEvolution):
        def _dist(self):
            return 0, 2

    with pytest.raises(ValueError):
        TwoRanks(diversify=64, name="de", **KW)._round()       # before any collective
    assert T.GpuPSO(diversify=64, name="pso", **KW).diversify == 64
    # the factories and tune_bandit pass it through
    assert all(t.diversify == 16 for t in T.pso_ga_de_bandit(diversify=16, **KW).techniques)
