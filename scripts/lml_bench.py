"""Wall time of ut_gp_lml_grid against g synchronous fits (profiles/lml_grid.json).

The grid factorises its g kernel matrices in one batched chain and forms no
inverse, so it has to come in below g times one ut_gp_fit of the same shape.
Three modes, so the fit can be timed on another build of the library (the
parent commit's, through UTHOT_LIB) in the same session:

    python scripts/lml_bench.py fit  --out fit.json      # one synchronous fit per shape
    python scripts/lml_bench.py grid --out grid.json     # the grid per shape
    python scripts/lml_bench.py merge --fit fit.json --grid grid.json --out profiles/lml_grid.json

and the gradient's leg (profiles/lml_grad.json): ut_gp_lml_grad alone on a fit
in place per shape, and one whole SharedModel(lengthscale="ard") selection at
n = 1024, against the same fit times:

    python scripts/lml_bench.py grad --out grad.json
    python scripts/lml_bench.py merge-grad --fit fit.json --grad grad.json --out profiles/lml_grad.json

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
        if mode == "grad":
            e.gp_fit(X, y, lengthscale=2.0, **HYP)
            res = {}
            rec.update(timed(lambda: res.update(v=e.gp_lml_grad()), repeats))
            rec.update(max_abs_dlog_ell=float(np.max(np.abs(res["v"][0]))), dlog_sf2=res["v"][1], dlog_sn2=res["v"][2])
            if n == 1024:
                rec.update(ard=ard_selection(e, X, y, max(2, repeats // 3)))
        elif mode == "fit":
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


def ard_selection(e, X, y, repeats):
    """one whole "ard" selection (the grid, then L-BFGS-B: a fit, its LML and its
    gradient per evaluation) on the engine, as SharedModel.fit runs it"""
    from uptune_amd.technique import SharedModel
    m = SharedModel(lengthscale="ard", **HYP)
    m.engine = e
    evals = []
    inner = e.gp_lml_grad

    def counted():
        evals[-1] += 1
        return inner()
    e.gp_lml_grad = counted

    def once():
        evals.append(0)
        m._select_ard(X, y)
    rec = timed(once, repeats, warmup=1)
    e.gp_lml_grad = inner
    n, ell, lml = m.ell_history[-1]
    grid = np.sqrt(X.shape[1]) * np.geomspace(0.05, 4.0, 16)   # the selection's own default grid
    rec.update(evaluations=evals[-1], maxiter=m.ard_maxiter, lml=float(lml),
               lml_start=float(np.nanmax(e.gp_lml_grid(X, y, 1.0, grid, **HYP)[0])),
               ell_min=float(np.min(ell)), ell_max=float(np.max(ell)))
    return rec


def merge_grad(fit, grad):
    rows = []
    for f, q in zip(fit["shapes"], grad["shapes"]):
        assert (f["n"], f["d"]) == (q["n"], q["d"])
        row = dict(n=q["n"], d=q["d"], grad_ms=q["median_ms"], grad_min_ms=q["min_ms"], grad_max_ms=q["max_ms"],
                   fit_ms=f["median_ms"], fit_min_ms=f["min_ms"], fit_max_ms=f["max_ms"],
                   ratio=q["median_ms"] / f["median_ms"], repeats=q["repeats"])
        if "ard" in q:
            a = q["ard"]
            row["ard_selection"] = dict(a, selection_ms=a["median_ms"], fits_equivalent=a["median_ms"] / f["median_ms"])
        rows.append(row)
    return dict(what="ut_gp_lml_grad wall time on a fit in place against one synchronous ut_gp_fit of the same "
                     "shape, and one whole SharedModel(lengthscale='ard') selection (median of the repeats, host "
                     "clock around synchronous calls)",
                fit_library=fit["library"], grad_library=grad["library"], shapes=rows)


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
    ap.add_argument("mode", choices=["fit", "grid", "merge", "grad", "merge-grad"])
    ap.add_argument("--out", default=os.path.join("profiles", "lml_grid.json"))
    ap.add_argument("--fit")
    ap.add_argument("--grid")
    ap.add_argument("--grad")
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--label", default="this commit", help="which build of the library is timed (UTHOT_LIB)")
    a = ap.parse_args()
    if a.mode == "merge":
        res = merge(json.load(open(a.fit)), json.load(open(a.grid)))
    elif a.mode == "merge-grad":
        res = merge_grad(json.load(open(a.fit)), json.load(open(a.grad)))
    else:
        res = run(a.mode, a.repeats, a.label)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
