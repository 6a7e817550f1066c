"""The edge shapes of tests/_rf_fit_cases.py reach the paths of
csrc/forest_fit.hip they are there for: every case's condition, asserted on the
restatement's own output, so that a case which stops reaching its path fails
here and does not pass vacuously on the device.  The restatement's route /
predict / level_widths against its own growth.  No GPU."""
import time

import numpy as np
import pytest

import _rf_fit_cases as RC
import _rf_fit_oracle as RF


@pytest.mark.parametrize("name", sorted(RC.CASES))
def test_case_reaches_its_path(name):
    t0 = time.perf_counter()
    ref = RC.reference(name)
    print(name, "widest level %d, %d nodes, largest split feature %d" % RC.shape_of(ref["roots"], ref["nodes"]),
          "%.2f s" % (time.perf_counter() - t0))
    RC.check(name)


@pytest.mark.parametrize("name", ["wide_levels_bootstrap", "blocks_65_frac", "no_eligible_feature"])
def test_route_sends_training_rows_where_the_fit_put_them(name):
    ref = RC.reference(name)
    roots, nodes, node_rows = ref["roots"], ref["nodes"], ref["node_rows"]
    assert len(node_rows) == nodes.size
    leaf = RF.route(nodes, roots, RF.codes_of(ref["X"]))
    assert (nodes["feature"][leaf] == -1).all()
    ends = np.append(roots, nodes.size)
    for t in range(len(roots)):
        assert ((leaf[:, t] >= ends[t]) & (leaf[:, t] < ends[t + 1])).all()
        in_bag = node_rows[roots[t]]
        assert all(i in node_rows[leaf[i, t]] for i in in_bag)
    # level_widths counts every node once
    assert [sum(w) for w in RF.level_widths(nodes, roots)] == np.diff(ends).tolist()
    # predict is the tree-order mean of the routed leaves' values
    mu = RF.predict(nodes, roots, RF.codes_of(ref["X"]))
    i = len(mu) // 2
    acc = 0.0
    for t in range(len(roots)):
        acc += float(nodes["value"][leaf[i, t]])
    assert mu[i] == acc / len(roots)


def test_candidates_hold_the_values_a_double_comparison_misroutes():
    for d in (3, 17):
        C = RC.candidates(d)
        assert C.shape == (2000, d)
        for v in RC.SPECIALS:
            assert any(np.array_equal(c, v, equal_nan=True) and np.signbit(c) == np.signbit(v) for c in C[:, d - 1])
    # route on codes agrees with a float32 comparison of x with the threshold, as uthot.h states LT
    ref = RC.reference("no_eligible_feature")
    nodes, roots = ref["nodes"], ref["roots"]
    C = RC.candidates(2)
    leaf = RF.route(nodes, roots, RF.codes_of(C))
    for i in range(0, len(C), 37):
        for t, r in enumerate(roots):
            nd = int(r)
            while nodes["feature"][nd] >= 0:
                x = np.float32(C[i, nodes["feature"][nd]])
                left = True if np.isnan(x) else bool(x < np.float32(nodes["threshold"][nd]))
                nd = int(nodes["left"][nd] if left else nodes["right"][nd])
            assert nd == leaf[i, t]
