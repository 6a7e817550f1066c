"""The boosted-tree surrogate fitted on the device (ut_gbt_fit): time, held-out
error beside sklearn's HistGradientBoostingRegressor, and one search comparison
(profiles/gbt_fit.json).

    python scripts/gbt_fit_bench.py --out profiles/gbt_fit.json

  time    c2: 1,024 rows x 64 features of the bench's Rosenbrock data; c4: the
          gcc flag space's successful runs in tests/golden/gcc_history.npz x 707
          features.  Four fits alternate inside every repeat, after a warm-up of
          each: ut_gbt_fit with the reference's parameters (300 rounds, eta 0.015,
          depth 10, subsample 0.4, colsample_bylevel 0.5, lambda 1); ut_gbt_fit
          with subsample = colsample_bylevel = 1; HistGradientBoostingRegressor
          with the same rounds, rate, depth, l2 and min_samples_leaf, 255 bins,
          no early stopping (it has no row subsampling, hence the pair without);
          ut_forest_fit (64 trees) on the same rows for context.  The host clock
          around a call that ends in a device synchronise; median, min, max.
  rmse    five 80/20 splits of the c2 and of the c4 rows: the
          held-out RMSE of the device ensemble (subsample = colsample = 1)
          beside the sklearn model on the same split.
  search  tune_bandit on spaces.r64() with the 64-D Rosenbrock objective, 400
          tests, five seeds: surrogate="gbt" against the GP default.

The file is rewritten after every step.  Kernel times are not taken here: they
come from a kernel-trace run of this script with --only time.  Fails without a
GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

from forest_fit_bench import _engine, _rosen64, c2_data, c4_data, stat  # noqa: E402

FULL = dict(subsample=1.0, colsample_bylevel=1.0)
HGB = dict(max_iter=300, learning_rate=0.015, max_depth=10, l2_regularization=1.0, min_samples_leaf=1, max_bins=255,
           early_stopping=False, max_leaf_nodes=None)


def time_step(name, X, y, repeats):
    import torch
    from sklearn.ensemble import HistGradientBoostingRegressor
    e = _engine(X.shape[1])

    def dev(**kw):
        e.gbt_fit(X, y, **kw)
        torch.cuda.synchronize()

    def forest():
        e.forest_fit(X, y)
        torch.cuda.synchronize()

    calls = {"device_reference_params": dev, "device_no_sampling": lambda: dev(**FULL),
             "sklearn_hist_gb": lambda: HistGradientBoostingRegressor(random_state=0, **HGB).fit(X, y),
             "device_forest_fit": forest}
    for c in calls.values():
        c()
    ts = {k: [] for k in calls}
    nodes = {}
    for _ in range(repeats):
        for k, c in calls.items():
            t0 = time.perf_counter()
            c()
            ts[k].append(time.perf_counter() - t0)
            if k.startswith("device_"):
                nodes[k] = int(e.forest_get()[1].size)
    e.close()
    rec = dict(shape=name, n=int(X.shape[0]), d=int(X.shape[1]), repeats=repeats, nodes=nodes,
               **{k: stat(v) for k, v in ts.items()})
    rec["device_no_sampling_over_sklearn"] = rec["device_no_sampling"]["median_s"] / rec["sklearn_hist_gb"]["median_s"]
    return rec


def rmse_step(name, X, y):
    import torch
    from sklearn.ensemble import HistGradientBoostingRegressor
    e = _engine(X.shape[1])
    dev, sk = [], []
    for split in range(5):
        perm = np.random.default_rng(7 + split).permutation(len(y))
        cut = int(0.8 * len(y))
        tr, te = perm[:cut], perm[cut:]
        e.gbt_fit(X[tr], y[tr], **FULL)
        pred, _ = e.forest_predict(torch.from_numpy(np.ascontiguousarray(X[te].T)).cuda())
        dev.append(float(np.sqrt(np.mean((pred.cpu().numpy() - y[te]) ** 2))))
        m = HistGradientBoostingRegressor(random_state=0, **HGB).fit(X[tr], y[tr])
        sk.append(float(np.sqrt(np.mean((m.predict(X[te]) - y[te]) ** 2))))
    e.close()
    return dict(data=name, n=int(len(y)), y_std=float(np.std(y)), device_rmse=dev, sklearn_rmse=sk,
                device_range_within_sklearn_range=bool(min(sk) <= min(dev) and max(dev) <= max(sk)))


def search_step(seeds, generations, out):
    from uptune_amd import spaces
    from uptune_amd.tuner import tune_bandit
    runs = []
    for seed in seeds:
        for surrogate in ("gbt", None):
            t0 = time.perf_counter()
            d = tune_bandit(spaces.r64(), _rosen64, generations=generations, seed=seed, surrogate=surrogate)
            model = d.root_technique.techniques[0].model
            runs.append(dict(seed=seed, surrogate=surrogate or "gp", best=float(d.best_result.time),
                             tests=int(d.test_count), wall_s=time.perf_counter() - t0, fits=int(model.fits),
                             fit_seconds=float(model.fit_seconds)))
            print(json.dumps(runs[-1]), flush=True)
            out(runs)
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "gbt_fit.json"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--generations", type=int, default=100)
    ap.add_argument("--only", default="time,rmse,search")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "gbt_fit_bench needs a GPU"
    only = a.only.split(",")
    res = dict(what="ut_gbt_fit (300 rounds, eta 0.015, depth 10, lambda 1; subsample 0.4 / colsample_bylevel 0.5, or "
                    "both 1) beside HistGradientBoostingRegressor.fit with the same settings and ut_forest_fit (64 "
                    "trees): seconds per fit (host clock, the device call ends in a synchronise, variants alternating "
                    "per repeat); held-out RMSE on five 80/20 splits; tune_bandit on the 64-D Rosenbrock space, "
                    "surrogate='gbt' against the GP",
               device=torch.cuda.get_device_name(0))
    if os.path.exists(a.out):   # steps taken in separate runs join one file
        with open(a.out) as fh:
            res.update({k: v for k, v in json.load(fh).items() if k not in res})

    def write():
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            json.dump(res, fh, indent=1)
            fh.write("\n")

    data = {"c2": c2_data(), "c4": c4_data()} if "time" in only or "rmse" in only else {}
    if "time" in only:
        res["time"] = []
        for name, (X, y) in data.items():
            res["time"].append(time_step(name, X, y, a.repeats))
            print(json.dumps(res["time"][-1]), flush=True)
            write()
    if "rmse" in only:
        res["rmse"] = []
        for name, (X, y) in data.items():
            res["rmse"].append(rmse_step(name, X, y))
            print(json.dumps(res["rmse"][-1]), flush=True)
            write()
    if "search" in only:
        res["search_generations"] = a.generations

        def out(runs):
            res["search"] = runs
            write()
        search_step(range(5), a.generations, out)
    write()
    return 0


if __name__ == "__main__":
    sys.exit(main())
