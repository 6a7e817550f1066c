"""The forest mean / variance restatement (tests/_forest_stat_oracle.py) pinned
without a device: its leaves against sklearn's own trees, its fp64 variance
against the long-double one within the per-candidate tolerance on every case,
the unshifted textbook formula outside that tolerance on the offset cases (why
the shift by the first leaf exists), from_sklearn(leaf_var=True), and the
refitting model's host logic against a CPU stand-in engine."""
import numpy as np
import pytest

import _forest_stat_cases as SC
import _forest_stat_oracle as O
from _oracle_engine import OracleEngine

LD = np.longdouble


@pytest.mark.parametrize("kind,offset", [("rf", False), ("rf", True), ("et", False), ("et", True)])
def test_leaves_and_leaf_variances_match_sklearn(kind, offset):
    from uptune_amd.forest import from_sklearn
    model = SC.sk_model(kind, offset)
    f = from_sklearn(model, leaf_var=True)
    X = np.random.default_rng(3).uniform(size=(200, 6))
    lf = O.leaves(f.nodes, f.roots, f.rule, X)
    imp = np.concatenate([e.tree_.impurity for e in model.estimators_])
    assert f.leaf_var.shape == (f.nodes.size,) and (f.leaf_var >= 0).all()
    np.testing.assert_array_equal(f.leaf_var, np.maximum(imp, 0.0))
    for t, est in enumerate(model.estimators_):
        np.testing.assert_array_equal(f.nodes["value"][lf[:, t]], est.predict(X))
        np.testing.assert_array_equal(f.leaf_var[lf[:, t]], np.maximum(est.tree_.impurity[est.apply(X)], 0.0))
    st = O.stats(f.nodes, f.roots, f.rule, f.div, X, leaf_var=f.leaf_var)
    np.testing.assert_array_equal(st["mu"], model.predict(X))
    # plain from_sklearn is unchanged: no leaf variances, the same records
    g = from_sklearn(model)
    assert g.leaf_var is None and g.nodes.tobytes() == f.nodes.tobytes()


def test_leaf_var_refused_for_other_criteria():
    from sklearn.ensemble import RandomForestRegressor
    from uptune_amd.forest import from_sklearn
    X, y = SC._train()
    model = RandomForestRegressor(n_estimators=3, criterion="absolute_error", random_state=0).fit(X[:60], y[:60])
    with pytest.raises(TypeError, match="squared-error"):
        from_sklearn(model, leaf_var=True)
    assert from_sklearn(model).leaf_var is None


@pytest.mark.parametrize("name", sorted(SC.CASES))
def test_fp64_variance_within_tolerance_of_extended(name):
    st = SC.reference(name)
    err = np.abs(st["var"].astype(LD) - st["var_ext_ld"])
    print(name, "max err / tol", float(np.max(err / np.maximum(st["tol"], 1e-300))))
    assert (st["var"] >= 0).all() and np.isfinite(st["var"]).all()
    assert (err <= st["tol"]).all()


@pytest.mark.parametrize("name", SC.OFFSET_CASES)
def test_unshifted_formula_misses_the_tolerance(name):
    st = SC.reference(name)
    err = np.abs(st["var_unshifted"].astype(LD) - st["var_ext_ld"])
    print(name, "unshifted max err / tol", float(np.max(err / st["tol"])))
    assert (err > st["tol"]).mean() > 0.9 and np.max(err / st["tol"]) > 1e4


def test_single_tree_has_only_its_leaf_variance():
    f, X, _, _ = SC.case("le_T1_F3_m64")
    st = SC.reference("le_T1_F3_m64")
    np.testing.assert_array_equal(st["var"], f.leaf_var[st["leaf"][:, 0]])


# --------------------------------------------------------------------------- the refitting model, host side
class ForestOracleEngine(OracleEngine):
    """the CPU stand-in with the two forest calls the refitting model makes"""

    def forest_set(self, model):
        from uptune_amd.forest import as_forest
        self.forest = as_forest(model)
        self.sets = getattr(self, "sets", 0) + 1

    def forest_score(self, feat, acq=None, f_best=0.0, dup=None, m=None):
        import torch
        from oracle import gp as ogp
        f = self.forest
        st = O.stats(f.nodes, f.roots, f.rule, f.div, feat.numpy().T, leaf_var=f.leaf_var)
        kind, xi, kappa = acq or self.acq()
        s = ogp.acquisition(st["mu"], st["var"], f_best, kind=kind, xi=xi, kappa=kappa)
        if dup is not None:
            s = np.where(dup.numpy() != 0, -np.inf, s)
        return torch.from_numpy(st["mu"]), torch.from_numpy(st["var"]), torch.from_numpy(np.ascontiguousarray(s))


def _sphere(c):
    return float(sum((c["u%d" % k] - 0.7) ** 2 for k in range(4)))


def _run(seed, limit=40):
    from uptune_amd import technique as T
    from uptune_amd.driver import SearchDriver
    from uptune_amd.manipulator import ConfigurationManipulator, FloatParameter
    man = ConfigurationManipulator([FloatParameter("u%d" % k, 0.0, 1.0) for k in range(4)])
    de = T.GpuDifferentialEvolution(surrogate="forest", pool=256, batch=4, population=32, seed=seed,
                                    engine_factory=lambda mm, dev, sd: ForestOracleEngine(mm, dev, sd),
                                    forest_kw={"n_estimators": 8}, name="de-forest")
    d = SearchDriver(man, de, parallelism=4)
    d.main(_sphere, test_limit=limit)
    return d


def test_refitting_model_host_logic():
    d = _run(2)
    model = d.root_technique.model
    res = d.results_query()
    assert model.surrogate == "forest" and model.fits > 1 and model.engine.sets == model.fits
    f = model.engine.forest
    assert f.n_trees == 8 and f.leaf_var is not None and f.div == 8.0
    assert model.fit_seconds > 0.0
    # fit() refits iff the usable results changed (the last generation's arrived after the last round)
    fits = model.fits
    assert model.fit(d) is True and model.fits == fits + 1
    assert model.fit(d) is True and model.fits == fits + 1 and model._n == len(res)
    # f_best is min(y) of the rows the last fit saw, in the units it fitted
    assert model.f_best == min(r.time for r in res[:model._n]) and model._n >= model.min_train
    assert d.best_result.time <= next(iter(d.results.values())).time
    # deterministic for a seed: a second run requests the same configurations
    d2 = _run(2)
    assert [r.configuration.hash for r in d2.results_query()] == [r.configuration.hash for r in res]


def test_tree_surrogate_refusals_and_sharing():
    from uptune_amd import technique as T
    for kw, msg in ((dict(diversify=8), "diversify conditions a GP posterior: not with a tree surrogate"),
                    (dict(feasibility=True), "feasibility weights the GP's EI: not with a tree surrogate"),
                    (dict(constraints=[("acc", ">=", 0.5)]), "constraints weight the GP's EI: not with a tree"),
                    (dict(prune_rows=64), "not with a tree surrogate")):
        with pytest.raises(ValueError, match=msg):
            T.GpuDifferentialEvolution(surrogate="forest", **kw)
    with pytest.raises(ValueError):
        T.SharedModel(surrogate="boosted")
    with pytest.raises(ValueError, match="shared model that fits a GP"):
        T.GpuDifferentialEvolution(surrogate="forest", shared=T.SharedModel())
    for make in (T.bandit_a, T.bandit_b, T.pso_ga_de_bandit):
        meta = make(surrogate="forest", forest_kw={"n_estimators": 5}, pool=64, batch=2)
        models = {id(t.model) for t in meta.techniques}
        assert len(models) == 1 and meta.techniques[0].model.surrogate == "forest"
        assert meta.techniques[0].model.forest_kw == {"n_estimators": 5}
        assert all(t.surrogate == "forest" and not t._static for t in meta.techniques)
    # the GP remains the default, and a model object is still a static surrogate
    assert T.GpuDifferentialEvolution().model.surrogate is None
    t = T.GpuDifferentialEvolution(surrogate=SC.sk_model("rf", False))
    assert t._static and t.model.surrogate is None
