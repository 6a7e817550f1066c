"""Device time of the forest surrogate's scoring kernels and host time of its
refit (profiles/forest_ei.json).

    python scripts/forest_ei_bench.py --out profiles/forest_ei.json

One process, two shapes:

  c2   m = 2^20 candidates, d = 64 features, a 64-tree RandomForestRegressor
       (min_samples_leaf=3) fitted on 1,024 rows of the bench's Rosenbrock data
  c4   the gcc flag space (707 features), m = 2^22 GA children of the best
       recorded run, the forest fitted on every successful run recorded in
       tests/golden/gcc_history.npz

and at each of them three calls on the same features and the same loaded
ensemble: ut_forest_predict (the mean alone: the yardstick), and
ut_forest_score (mean + variance + EI) with the one-lane kernel and with the
staged kernel (UT_FOREST_STATS=lane / staged).  707 features exceed the staged
kernel's LDS budget, so at c4 the staged request runs the one-lane kernel; the
record says so.

A time is the host clock around `inner` back-to-back calls and a device
synchronise, divided by `inner`; the variants alternate inside every repeat,
after warm-up calls of each; median, min and max over the repeats are
recorded, so the spread is there to hold a difference against.  Before timing,
the three calls' outputs are compared: mu bitwise the prediction, and both
kernels the same bits.  The host refit (RandomForestRegressor.fit) is timed
with n_jobs=1 and n_jobs=16, median of three.  Fails without a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RF = dict(n_estimators=64, min_samples_leaf=3, random_state=0)


def c2_setup():
    import torch
    from uptune_amd.engine import BatchEngine
    from uptune_amd.manipulator import ConfigurationManipulator, FloatParameter
    d, n, m = 64, 1024, 1 << 20
    e = BatchEngine(ConfigurationManipulator([FloatParameter(i, -1000.0, 1000.0) for i in range(d)]), device=0, seed=1)
    rng = np.random.default_rng(101)
    X = rng.uniform(size=(n, d))
    y = np.sum(100.0 * (X[:, 1:] - X[:, :-1] ** 2) ** 2 + (1.0 - X[:, :-1]) ** 2, axis=1)
    e.population_init(m)
    feat = e.encode(e.population_get())
    torch.cuda.synchronize()
    return e, X, y, feat


def c4_setup():
    import torch
    from uptune_amd import spaces
    from uptune_amd.engine import BatchEngine
    e = BatchEngine(spaces.gcc(), device=0, seed=1)
    z = np.load(os.path.join(ROOT, "tests", "golden", "gcc_history.npz"))
    hist, qor = z["values"], z["qor"]
    ok = np.flatnonzero(np.isfinite(qor))
    hv = torch.from_numpy(np.ascontiguousarray(hist[:, ok])).to(e.device)
    X = e.encode(hv).T.contiguous().cpu().numpy()
    parent = hist[:, int(ok[np.argmin(qor[ok])])].copy()
    vals = e.propose_ga(1 << 22, parent, None, round_=1, mutation_rate=0.1)[0]
    feat = e.encode(vals)
    del vals
    torch.cuda.synchronize()
    return e, X, qor[ok].astype(np.float64), feat


def fit_times(X, y):
    from sklearn.ensemble import RandomForestRegressor
    out, model = {}, None
    for jobs in (1, 16):
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            model = RandomForestRegressor(n_jobs=jobs, **RF).fit(X, y)
            ts.append(time.perf_counter() - t0)
        out["n_jobs_%d" % jobs] = dict(median_s=float(np.median(ts)), min_s=float(min(ts)), max_s=float(max(ts)))
    return out, model     # the fit does not depend on n_jobs (one seed per tree)


def shape_step(name, repeats, inner):
    import torch
    from uptune_amd.forest import from_sklearn
    e, X, y, feat = (c2_setup if name == "c2" else c4_setup)()
    host, model = fit_times(X, y)
    f = from_sklearn(model, leaf_var=True)
    e.forest_set(f)
    f_best, acq = float(y.min()), e.acq("ei")
    F, m = int(feat.shape[0]), int(feat.shape[1])

    def score(kernel):
        os.environ["UT_FOREST_STATS"] = kernel
        return e.forest_score(feat, acq, f_best)

    calls = {"predict": lambda: e.forest_predict(feat), "stats_lane": lambda: score("lane"),
             "stats_staged": lambda: score("staged")}
    # the same answers first
    pred = calls["predict"]()[0]
    lane, staged = calls["stats_lane"](), calls["stats_staged"]()
    torch.cuda.synchronize()
    same = bool(torch.equal(pred.view(torch.int64), lane[0].view(torch.int64)) and
                all(torch.equal(a.view(torch.int64), b.view(torch.int64)) for a, b in zip(lane, staged)))
    assert same, "the kernels disagree"
    var = lane[1]
    summary = dict(var_min=float(var.min()), var_median=float(var.median()), var_max=float(var.max()),
                   ei_positive=int((lane[2] > 0).sum()))
    del pred, lane, staged, var
    for c in calls.values():
        for _ in range(2):
            c()
    torch.cuda.synchronize()
    ts = {k: [] for k in calls}
    for _ in range(repeats):
        for k, c in calls.items():
            torch.cuda.synchronize()
            t0 = time.perf_counter()
            for _ in range(inner):
                c()
            torch.cuda.synchronize()
            ts[k].append((time.perf_counter() - t0) * 1e3 / inner)
    os.environ.pop("UT_FOREST_STATS", None)
    depth = float(np.mean([est.tree_.max_depth for est in model.estimators_]))
    rec = dict(shape=name, m=m, n_features=F, n_train=int(X.shape[0]), n_trees=f.n_trees, n_nodes=int(f.nodes.size),
               mean_max_depth=depth, repeats=repeats, inner=inner, outputs_agree=same,
               staged_kernel_ran=bool(F <= 128), host_fit=host, scores=summary,
               ms={k: dict(median=float(np.median(v)), min=float(min(v)), max=float(max(v))) for k, v in ts.items()})
    rec["stats_lane_over_predict"] = rec["ms"]["stats_lane"]["median"] / rec["ms"]["predict"]["median"]
    rec["stats_staged_over_lane"] = rec["ms"]["stats_staged"]["median"] / rec["ms"]["stats_lane"]["median"]
    del feat
    e.close()
    torch.cuda.empty_cache()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "forest_ei.json"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--inner", type=int, default=5)
    ap.add_argument("--shapes", default="c2,c4")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "forest_ei_bench needs a GPU"
    recs = []
    for name in a.shapes.split(","):
        recs.append(shape_step(name, a.repeats, a.inner))
        print(json.dumps(recs[-1]), flush=True)
    res = dict(what="ut_forest_predict (mean alone) against ut_forest_score (mean + variance + EI) with the "
                    "one-lane and the staged kernel, same features and ensemble, host clock around `inner` calls "
                    "+ synchronise, variants alternating per repeat (ms per call: median, min, max); host_fit: "
                    "RandomForestRegressor(n_estimators=64, min_samples_leaf=3).fit, seconds",
               device=torch.cuda.get_device_name(0), shapes=recs)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
