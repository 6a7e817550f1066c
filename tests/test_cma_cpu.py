"""CMA-ES without a GPU: the CMAState update (uptune_amd/cma.py) keeps its
invariants, shows the step-size rule's defining behaviour on a linear function
and converges on a sphere, fed from the numpy restatement of ut_propose_cma
(tests/_cma_oracle.py); the opt-in wiring changes nothing unless asked."""
import types

import numpy as np
import pytest

import _cma_oracle as co
from oracle.space import FLOAT, Param
from uptune_amd.cma import CMAState


def _generation(st, space, f, lam, gen, seed=11):
    """one ask / sample / rank / tell -> (the generation's best f, restarted)"""
    mean, sigma, A = st.ask()
    centre = np.zeros(len(space))
    _, _, U, _ = co.propose_cma_vec(space, centre, mean, A, sigma, 0.0, seed, gen, gen * lam, lam)
    y = f(U)
    restarted = st.tell(U, np.argsort(y, kind="stable"))
    if not restarted:
        C = st.C
        assert (C == C.T).all()
        assert np.abs(st.A @ st.A.T - C).max() <= 1e-12 * np.abs(C).max()
    return float(y.min()), restarted


def test_linear_function_grows_the_step():
    space = [Param("x%d" % k, FLOAT, 0.0, 1.0) for k in range(5)]
    # the rule is scale-invariant; a small sigma0 keeps 20 generations of a growing step inside the
    # unit box, where f(u) = u_0 is linear in x (at the mirror it is |x_0|, which any ES contracts on)
    st = CMAState(5, 12, sigma0=1e-4)
    m0 = st.mean[0]
    for gen in range(20):
        _generation(st, space, lambda U: U[0], 12, gen)
    assert st.sigma > st.sigma0 and st.mean[0] < m0 and st.restarts == 0


def test_sphere_converges():
    space = [Param("x%d" % k, FLOAT, 0.0, 1.0) for k in range(8)]
    st = CMAState(8, 16)
    st.mean = np.full(8, 0.2)
    best = [_generation(st, space, lambda U: ((U - 0.5) ** 2).sum(axis=0), 16, gen)[0] for gen in range(150)]
    assert min(best) < 1e-3 * best[0]


def test_restart_triggers():
    st = CMAState(4, 8)
    assert st.tell(np.full((4, 1), 0.7), [0]) is False and st.generation == 0 and st.mean[0] == 0.5   # < 2 rows: no-op
    st.mean = np.array([0.1, 0.2, 0.3, 0.4])
    st.sigma, st.p_c = 0.01, np.ones(4)
    sing = np.ones((4, 4))                         # rank one: no Cholesky factor
    assert st._refactor(sing) is True and st.restarts == 1
    assert st.sigma == st.sigma0 and (st.C == np.eye(4)).all() and not st.p_c.any() and st.mean[3] == 0.4
    assert st._refactor(np.diag([1.0, 1.0, 1.0, 1e-15])) is True and st.restarts == 2     # cond(A) > 1e7
    st.sigma = st.sigma_min                        # sigma underflow, through a tell of eight results at the mean:
    U = np.repeat(st.mean[:, None], 8, axis=1)     # a zero step shortens the path and the step size with it
    assert st.tell(U, np.arange(8)) is True and st.restarts == 3 and st.sigma == st.sigma0
    with pytest.raises(ValueError):
        CMAState(0, 8)
    with pytest.raises(ValueError):
        CMAState(129, 8)


def test_opt_in_wiring_and_the_dn_refusals():
    import inspect
    from uptune_amd import spaces
    from uptune_amd import technique as T
    from uptune_amd.manipulator import BooleanParameter, ConfigurationManipulator, compile_space
    from uptune_amd.tuner import tune_bandit
    kw = dict(pool=256, batch=4)
    reg = T.reference_registry(cma=True, **kw)
    assert len(reg) == 25 and isinstance(reg[-1], T.GpuCMAES) and reg[-1].name == "GpuCMAES"
    assert [t.name for t in reg[:24]] == [t.name for t in T.reference_registry(**kw)]
    for make, n in ((T.bandit_a, 3), (T.bandit_b, 2), (T.pso_ga_de_bandit, 4)):
        a, b = make(**kw), make(cma=True, **kw)
        assert len(a.techniques) == n and [type(t) for t in a.techniques] == [type(t) for t in b.techniques[:n]]
        arm = b.techniques[-1]
        assert len(b.techniques) == n + 1 and isinstance(arm, T.GpuCMAES) and arm.name == "gpu-cma-es"
        assert arm.model is b.techniques[0].model and arm.preselect and arm.pool == 256
    assert inspect.signature(tune_bandit).parameters["cma"].default is False
    assert T.GpuCMAES(preselect=False, **kw).pool == 4
    # a stand-in engine: init_population reads the compiled space alone
    for manip, ok in ((spaces.r64(128), True), (spaces.r64(129), False),
                      (ConfigurationManipulator([BooleanParameter("b")]), False)):
        t = T.GpuCMAES(**kw)
        t.model.engine = types.SimpleNamespace(spec=compile_space(manip))
        if ok:
            t.init_population()
            assert len(t._moving) == 128
        else:
            with pytest.raises(ValueError, match="GpuCMAES"):
                t.init_population()
