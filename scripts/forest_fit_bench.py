"""The forest surrogate's refit on the device (ut_forest_fit) beside the host
refit it replaces (RandomForestRegressor.fit): time, held-out error, and one
search run (profiles/forest_fit.json).

    python scripts/forest_fit_bench.py --out profiles/forest_fit.json

  time    c2: 1,024 rows x 64 features of the bench's Rosenbrock data; c4: the
          gcc flag space's successful runs in tests/golden/gcc_history.npz x 707
          features.  64 trees, min_samples_leaf = 3 everywhere.  The three fits
          (device, sklearn n_jobs=1, sklearn n_jobs=16) alternate inside every
          repeat, after a warm-up of each; the host clock around a call that ends
          in a device synchronise; median, min and max over the repeats.
  rmse    80/20 split of the c4 rows and of a synthetic 64-D function: the
          held-out RMSE of the device forest's ut_forest_predict beside five
          sklearn forests (random_state 0..4) on the same split.
  search  tune_bandit on spaces.r64() with the 64-D Rosenbrock objective,
          surrogate="forest", forest_fit="device" against "host", five seeds:
          the best objective, the wall time and the seconds spent refitting.

Kernel times are not taken here: they come from a kernel-trace run of this
script with --only time.  Fails without a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

RF = dict(n_estimators=64, min_samples_leaf=3)


def _engine(d):
    from uptune_amd.engine import BatchEngine
    from uptune_amd.manipulator import ConfigurationManipulator, FloatParameter
    return BatchEngine(ConfigurationManipulator([FloatParameter(i, 0.0, 1.0) for i in range(d)]), device=0, seed=1)


def c2_data():
    rng = np.random.default_rng(101)
    X = rng.uniform(size=(1024, 64))
    return X, np.sum(100.0 * (X[:, 1:] - X[:, :-1] ** 2) ** 2 + (1.0 - X[:, :-1]) ** 2, axis=1)


def c4_data():
    import torch
    from uptune_amd import spaces
    from uptune_amd.engine import BatchEngine
    e = BatchEngine(spaces.gcc(), device=0, seed=1)
    z = np.load(os.path.join(ROOT, "tests", "golden", "gcc_history.npz"))
    ok = np.flatnonzero(np.isfinite(z["qor"]))
    hv = torch.from_numpy(np.ascontiguousarray(z["values"][:, ok])).to(e.device)
    X = e.encode(hv).T.contiguous().cpu().numpy()
    e.close()
    return X, z["qor"][ok].astype(np.float64)


def stat(ts):
    return dict(median_s=float(np.median(ts)), min_s=float(min(ts)), max_s=float(max(ts)))


def time_step(name, X, y, repeats):
    import torch
    from sklearn.ensemble import RandomForestRegressor
    e = _engine(X.shape[1])

    def device():
        e.forest_fit(X, y)
        torch.cuda.synchronize()

    calls = {"device": device,
             "sklearn_n_jobs_1": lambda: RandomForestRegressor(n_jobs=1, random_state=0, **RF).fit(X, y),
             "sklearn_n_jobs_16": lambda: RandomForestRegressor(n_jobs=16, random_state=0, **RF).fit(X, y)}
    for c in calls.values():
        c()
    ts = {k: [] for k in calls}
    for _ in range(repeats):
        for k, c in calls.items():
            t0 = time.perf_counter()
            c()
            ts[k].append(time.perf_counter() - t0)
    roots, nodes = e.forest_get()
    e.close()
    rec = dict(shape=name, n=int(X.shape[0]), d=int(X.shape[1]), repeats=repeats, device_nodes=int(nodes.size),
               **{k: stat(v) for k, v in ts.items()})
    rec["device_over_n_jobs_16"] = rec["device"]["median_s"] / rec["sklearn_n_jobs_16"]["median_s"]
    return rec


def rmse_step(name, X, y):
    import torch
    from sklearn.ensemble import RandomForestRegressor
    perm = np.random.default_rng(7).permutation(len(y))
    cut = int(0.8 * len(y))
    tr, te = perm[:cut], perm[cut:]
    e = _engine(X.shape[1])
    e.forest_fit(X[tr], y[tr])
    pred, _ = e.forest_predict(torch.from_numpy(np.ascontiguousarray(X[te].T)).cuda())
    dev = float(np.sqrt(np.mean((pred.cpu().numpy() - y[te]) ** 2)))
    e.close()
    sk = [float(np.sqrt(np.mean((RandomForestRegressor(n_jobs=16, random_state=s, **RF).fit(X[tr], y[tr])
                                 .predict(X[te]) - y[te]) ** 2))) for s in range(5)]
    spread = max(sk) - min(sk)
    return dict(data=name, n_train=int(cut), n_test=int(len(y) - cut), y_std=float(np.std(y[te])), device_rmse=dev,
                sklearn_rmse=sk, device_within_one_spread=bool(min(sk) - spread <= dev <= max(sk) + spread))


def _rosen64(cfg):
    x = np.array([cfg[i] for i in range(64)])
    return float(np.sum(100.0 * (x[1:] - x[:-1] ** 2) ** 2 + (x[:-1] - 1.0) ** 2))


def search_step(seeds, generations):
    from uptune_amd import spaces
    from uptune_amd.tuner import tune_bandit
    runs = []
    for seed in seeds:
        for where in ("host", "device"):
            t0 = time.perf_counter()
            d = tune_bandit(spaces.r64(), _rosen64, generations=generations, seed=seed, surrogate="forest",
                            forest_fit=where)
            model = d.root_technique.techniques[0].model
            runs.append(dict(seed=seed, forest_fit=where, best=float(d.best_result.time), tests=int(d.test_count),
                             wall_s=time.perf_counter() - t0, fits=int(model.fits),
                             fit_seconds=float(model.fit_seconds)))
            print(json.dumps(runs[-1]), flush=True)
    return runs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "forest_fit.json"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--generations", type=int, default=50)
    ap.add_argument("--only", default="time,rmse,search")
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "forest_fit_bench needs a GPU"
    only = a.only.split(",")
    res = dict(what="ut_forest_fit beside RandomForestRegressor.fit (64 trees, min_samples_leaf 3): seconds per fit "
                    "(host clock, the device call ends in a synchronise, variants alternating per repeat); held-out "
                    "RMSE on an 80/20 split; tune_bandit(surrogate='forest') on the 64-D Rosenbrock space",
               device=torch.cuda.get_device_name(0))
    data = {"c2": c2_data(), "c4": c4_data()}
    if "time" in only:
        res["time"] = []
        for name, (X, y) in data.items():
            res["time"].append(time_step(name, X, y, a.repeats))
            print(json.dumps(res["time"][-1]), flush=True)
    if "rmse" in only:
        rng = np.random.default_rng(3)
        Xs = rng.uniform(size=(2000, 64))
        ys = np.sin(6.0 * Xs[:, 0]) + 2.0 * Xs[:, 1] * Xs[:, 2] + (Xs[:, 3] > 0.5) + 0.1 * rng.normal(size=2000)
        res["rmse"] = [rmse_step("gcc", *data["c4"]), rmse_step("synthetic64", Xs, ys)]
        print(json.dumps(res["rmse"]), flush=True)
    if "search" in only:
        res["search_generations"] = a.generations
        res["search"] = search_step(range(5), a.generations)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as fh:
        json.dump(res, fh, indent=1)
        fh.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
