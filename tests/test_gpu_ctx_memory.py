"""Device memory of a context: every allocating family of libuthot is driven
once at the smallest shapes that reach it, and closing the engine must return
the library's device bytes (ut_device_bytes, read without a context) to what
they were before the engine existed.

Shapes: 130 training rows (two 128-row tiles after padding), 300 candidates
(two 256-column strips), k = 4; the space has one parameter of every kind the
device tables distinguish (Float, Integer, Enum, Boolean, a size-4
Permutation).

A failed regrow of the GP buffers is not tested here: gp_alloc's allocations
are outside the fault injection's count by design (ut_debug_fail_alloc counts
ensure() and dalloc() only), so it cannot be made to fail without a new debug
entry point."""
import ctypes
import gc

import numpy as np
import pytest

torch = pytest.importorskip("torch")
pytestmark = pytest.mark.gpu

from _forest_cases import le_forest  # noqa: E402
from _spaces import to_manip  # noqa: E402
from oracle.space import BOOL, ENUM, FLOAT, INT, PERM, Param  # noqa: E402

N, M, K = 130, 300, 4
SPACE = [Param("x", FLOAT, -1.0, 1.0), Param("i", INT, 0, 9), Param("e", ENUM, options=["a", "b", "c"]),
         Param("b", BOOL), Param("p", PERM, options=[0, 1, 2, 3])]


def device_bytes(lib):
    b = ctypes.c_int64(-1)
    assert lib.ut_device_bytes(0, ctypes.byref(b)) == 0
    return int(b.value)


def test_close_returns_every_device_byte():
    if not torch.cuda.is_available():
        pytest.skip("needs a GPU")
    from uptune_amd import _lib as L
    from uptune_amd.engine import BatchEngine
    lib = L.lib()
    gc.collect()
    base = device_bytes(lib)
    e = BatchEngine(to_manip(SPACE), device=0, seed=3)
    # 1. two population slots, the second with PSO state (parked while slot 0 is selected)
    e.population_init(160)
    e.population_select(1)
    e.population_init(64)
    e.pso_reset()
    e.population_select(0)
    pop = e.population_get()
    X = e.encode(pop).T.contiguous().cpu().numpy()
    y = np.random.default_rng(7).normal(size=X.shape[0])
    hyp = dict(lengthscale=1.5, sigma_n2=1e-2)
    # 2. history from the host
    e.history_add(np.arange(5 * 8, dtype=np.uint32).reshape(5, 8))
    # 3. fp64 fit, a scored DE round
    e.gp_fit(X[:N], y[:N], **hyp)
    e.score_round_de(M, K, round_=1)
    # 4. a pruned DE round, the bound pass in f32 (the default)
    st = e.score_round_de_pruned(M, K, round_=2, bound_rows=128)[4]
    assert st["bound_rows"] == 128
    # 5. a GA round
    e.score_round_ga(M, K, parent1=pop[:, 0].cpu().numpy(), round_=3)
    # 6. the other precisions
    for prec in (32, 16, 8):
        e.gp_set_precision(prec)
        e.gp_fit(X[:N], y[:N], **hyp)
        e.score_round_de(M, K, round_=4)
    # 7. an appended fit
    e.gp_set_precision(64)
    e.gp_fit(X[:N], y[:N], **hyp)
    e.gp_fit(X[:N + 2], y[:N + 2], **hyp)
    assert e.gp_last_fit_kind() == "append"
    e.score_round_de(M, K, round_=5)
    # 8. the likelihood grid
    lml, best = e.gp_lml_grid(X[:N], y[:N], 1.5, [0.5, 1.0, 2.0], sigma_n2=1e-2)
    assert np.isfinite(lml).all() and 0 <= best < 3
    # 9. a forest
    e.forest_set(le_forest(n_feat=3))
    pred, _ = e.forest_predict(e.encode(pop))
    assert torch.isfinite(pred).all()
    e.sync()
    held = device_bytes(lib)
    print(f"device bytes: baseline {base}, with the engine {held}")
    assert held > base
    e.close()
    left = device_bytes(lib) - base
    print(f"device bytes left after close(): {left}")
    assert left == 0
