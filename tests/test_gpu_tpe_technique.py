"""surrogate="tpe" through the driver: a stand-alone technique on a small mixed
space (new configurations, refits as results arrive, the same history for the
same seed) and one bandit run sharing the estimator across arms.  Needs a GPU."""
import pytest

torch = pytest.importorskip("torch")
pytestmark = [pytest.mark.gpu, pytest.mark.skipif(not torch.cuda.is_available(), reason="no GPU")]


def _space():
    from uptune_amd import manipulator as M
    return M.ConfigurationManipulator([M.FloatParameter("x", -2.0, 2.0), M.IntegerParameter("k", 1, 64),
                                       M.BooleanParameter("flag"), M.EnumParameter("mode", ["a", "b", "c"]),
                                       M.PermutationParameter("order", [0, 1, 2, 3])])


def _cost(c):
    return ((c["x"] - 0.5) ** 2 + abs(c["k"] - 20) / 64.0 + (0.0 if c["flag"] else 0.3)
            + {"a": 0.2, "b": 0.0, "c": 0.4}[c["mode"]] + 0.05 * c["order"].index(0))


def _history(seed):
    from uptune_amd import technique as T
    from uptune_amd.driver import SearchDriver
    de = T.GpuDifferentialEvolution(surrogate="tpe", tpe_kw={"gamma": 0.25}, pool=2048, batch=4, seed=seed)
    d = SearchDriver(_space(), de, parallelism=4)
    d.main(_cost, test_limit=32)
    return d, [(r.configuration.hash, r.time) for r in d.results.values()]


def test_technique_selects_new_configurations_and_refits():
    d, hist = _history(5)
    model = d.root_technique.model
    assert len(hist) >= 32 and len({h for h, _ in hist}) == len(hist)
    assert model.fits > 1 and model.fit_seconds > 0
    info = model.engine.tpe_info()
    assert info["gamma"] == 0.25 and info["n_l"] + info["n_g"] >= 4 and info["d"] == model.engine.spec.n_features
    assert _history(5)[1] == hist


def test_bandit_shares_one_estimator():
    from uptune_amd.tuner import tune_bandit
    d = tune_bandit(_space(), _cost, generations=6, parallelism=4, n_init=8, pool=2048, batch=4, seed=1,
                    surrogate="tpe")
    models = {id(t.model) for t in d.root_technique.techniques}
    assert len(models) == 1 and d.root_technique.techniques[0].model.fits >= 1
    assert d.best_result.time <= min(r.time for r in list(d.results.values())[:8])
