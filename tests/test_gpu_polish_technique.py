"""GpuBatchTechnique(polish=T): a dense GP round refines its polish_pool
best-scoring candidates with T ascent steps on the acquisition (ut_gp_polish)
and takes its batch from the refined rows.  2-D Rosenbrock, pool 4096, batch 8,
a few seeded results so that the first round already has a model (the setting
of test_gpu_diversify.py)."""
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


def _drive(tech, rounds=3):
    from uptune_amd.driver import SearchDriver
    from uptune_amd.tuner import random_configs
    m = _space()
    d = SearchDriver(m, tech, parallelism=8)
    cfgs, keys = random_configs(m, 12, 101, 0, with_keys=True)
    d.seed_results(cfgs, _rosen, keys=keys)
    d.main(_rosen, test_limit=10 ** 6, max_generations=rounds)
    return d


def _recording():
    from uptune_amd import technique as T

    class Recording(T.GpuDifferentialEvolution):
        def _polished_picks(self, vals, score, dup, dig, base):
            out = super()._polished_picks(vals, score, dup, dig, base)
            eng = self.engine
            rows = out[4].contiguous()
            self.seen = getattr(self, "seen", []) + [dict(
                idx=out[1].cpu().numpy(), top=out[2].cpu().numpy(), dig=out[3].cpu().numpy(), rows=rows.cpu().numpy(),
                vals=vals.cpu().numpy(), score=score.cpu().numpy(), base=base,
                rescored=eng.gp_acq_grad(rows, acq=eng.acq(self.acq_kind))[0].cpu().numpy(),
                rehashed=eng.hash(rows).cpu().numpy(), isdup=eng.dedup(out[3]).cpu().numpy())]
            return out
    return Recording


def test_polished_rounds_hand_on_the_final_rows():
    d = _drive(_recording()(polish=8, name="de", **KW))
    seen = d.root_technique.seen
    assert len(seen) >= 3                      # every round had a model
    moved = 0
    for r in seen:
        idx, loc = r["idx"], r["idx"] - r["base"]
        assert len(idx) == 8 and len(set(idx.tolist())) == 8 and idx.min() >= 0
        # a pick is no worse than the shortlist entry it descends from (the pool's score is the scoring
        # path's, the pick's the polish's own: the tier's 1e-9 apart)
        s_from = r["score"][loc]
        assert (r["top"] >= s_from - 1e-9 * (np.abs(s_from) + np.abs(r["score"][np.isfinite(r["score"])]).max())).all()
        # the rows, scores and digests handed on are the final rows' own; none is a configuration seen before
        assert r["rescored"].tobytes() == r["top"].tobytes()
        assert (r["rehashed"] == r["dig"]).all()
        assert not r["isdup"].any()
        assert (r["rows"] >= -2.0).all() and (r["rows"] <= 2.0).all()
        moved += int((r["rows"] != r["vals"][:, loc]).any(axis=0).sum())
    print("picks whose row moved:", moved, "of", 8 * len(seen))
    assert moved >= 8
    assert len(d.results) == len(d.seen_hashes())


def test_polish_0_is_the_default_path():
    from uptune_amd import technique as T
    a = _drive(T.GpuDifferentialEvolution(name="de", **KW))
    b = _drive(T.GpuDifferentialEvolution(polish=0, name="de", **KW))
    assert list(a.results.keys()) == list(b.results.keys()) and len(a.results) > 12
    c = _drive(T.GpuDifferentialEvolution(polish=8, name="de", **KW))
    assert list(c.results.keys()) != list(a.results.keys())
    assert len(c.results) == len(c.seen_hashes()) and len(c.results) > 12


def test_polish_composes_with_diversify():
    d = _drive(_recording()(polish=8, diversify=64, name="de", **KW))
    seen = d.root_technique.seen
    assert len(seen) >= 3
    for r in seen:
        assert len(set(r["idx"].tolist())) == 8 and r["idx"].min() >= 0
        assert len({bytes(x) for x in r["dig"]}) == 8
        assert (r["rehashed"] == r["dig"]).all()
    assert len(d.results) == len(d.seen_hashes())


def test_sharded_rounds_over_several_ranks_raise():
    from uptune_amd import technique as T

    class TwoRanks(T.GpuDifferentialEvolution):
        def _dist(self):
            return 0, 2

    with pytest.raises(ValueError):
        TwoRanks(polish=8, name="de", **KW)._round()       # before any collective
    # tune_bandit passes the pair through
    from uptune_amd.tuner import tune_bandit
    drv = tune_bandit(_space(), _rosen, generations=2, parallelism=4, n_init=8, pool=1024, batch=4, population=64,
                      polish=2, polish_pool=32)
    assert all(t.polish == 2 and t.polish_pool == 32 for t in drv.root_technique.techniques)
