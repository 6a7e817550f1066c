"""Wall time of ut_gp_lml_grid against g synchronous fits (profiles/lml_grid.json).

The grid factorises its g kernel matrices in one batched chain and forms no
inverse, so it has to come in below g times one ut_gp_fit of the same shape.
Three modes, so the fit can be timed on another build of the library (the
parent commit's, through UTHOT_LIB) in the same session:

    python scripts/lml_bench.py fit  --out fit.json      # one synchronous fit per shape
    python scripts/lml_bench.py grid --out grid.json     # the grid per shape
    python scripts/lml_bench.py merge --fit fit.json --grid grid.json --out profiles/lml_grid.json

Every timed call ends in a device synchronisation (both entry points are
synchronous), so the host clock around it is the call's wall time; the median
of the repeats after two warm-up calls is recorded, with the spread.
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [dict(n=1024, d=64, g=16), dict(n=4096, d=64, g=8)]
HYP = dict(sigma_f2=1.0, sigma_n2=1e-6, jitter=1e-8)


def data(n, d):
    rng = np.random.default_rng(n + d)
    X = rng.uniform(size=(n, d))
    return X, np.sum((X - 0.4) ** 2, axis=1) + 0.01 * rng.standard_normal(n)


def timed(fn, repeats, warmup=2):
    for _ in range(warmup):
        fn()
    ts = []
    for _ in range(repeats):
        t0 = time.perf_counter()
        fn()
        ts.append((time.perf_counter() - t0) * 1e3)
    return dict(median_ms=float(np.median(ts)), min_ms=float(np.min(ts)), max_ms=float(np.max(ts)), repeats=repeats)


def engine(d):
    from uptune_amd.engine import BatchEngine
    from uptune_amd.manipulator import ConfigurationManipulator, FloatParameter
    return BatchEngine(ConfigurationManipulator([FloatParameter(f"u{k}", 0.0, 1.0) for k in range(d)]), device=0)


def run(mode, repeats, label):
    out = dict(mode=mode, library=label, shapes=[])
    for s in SHAPES:
        n, d, g = s["n"], s["d"], s["g"]
        X, y = data(n, d)
        e = engine(d)
        rec = dict(s)
        if mode == "fit":
            # the same rows again are no append (n does not grow): every call refactors
            rec.update(timed(lambda: e.gp_fit(X, y, lengthscale=2.0, **HYP), repeats))
            assert e.gp_last_fit_kind() == "refit"
        else:
            scales = np.sqrt(d) * np.geomspace(0.05, 4.0, g)
            res = {}
            rec.update(timed(lambda: res.update(v=e.gp_lml_grid(X, y, 1.0, scales, **HYP)), repeats))
            lml, best = res["v"]
            rec.update(lml=[None if not np.isfinite(v) else float(v) for v in lml], best=int(best))
        e.close()
        out["shapes"].append(rec)
        print(json.dumps(rec), flush=True)
    return out


def merge(fit, grid):
    rows = []
    for f, q in zip(fit["shapes"], grid["shapes"]):
        assert (f["n"], f["d"], f["g"]) == (q["n"], q["d"], q["g"])
        g_fits = q["g"] * f["median_ms"]
        rows.append(dict(n=q["n"], d=q["d"], g=q["g"], grid_ms=q["median_ms"], grid_min_ms=q["min_ms"],
                         grid_max_ms=q["max_ms"], fit_ms=f["median_ms"], fit_min_ms=f["min_ms"],
                         fit_max_ms=f["max_ms"], g_fits_ms=g_fits, ratio=q["median_ms"] / g_fits,
                         repeats=q["repeats"], best=q["best"], lml=q["lml"]))
    return dict(what="ut_gp_lml_grid wall time against g synchronous ut_gp_fit calls of the same shape "
                     "(median of the repeats, host clock around synchronous calls)",
                fit_library=fit["library"], grid_library=grid["library"], shapes=rows)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("mode", choices=["fit", "grid", "merge"])
    ap.add_argument("--out", default=os.path.join("profiles", "lml_grid.json"))
    ap.add_argument("--fit")
    ap.add_argument("--grid")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--label", default="this commit", help="which build of the library is timed (UTHOT_LIB)")
    a = ap.parse_args()
    if a.mode == "merge":
        res = merge(json.load(open(a.fit)), json.load(open(a.grid)))
    else:
        res = run(a.mode, a.repeats, a.label)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
