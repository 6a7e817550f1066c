"""Fit and scoring time of the sparse-spectrum GP beside the exact GP, in one
process: nine repeats per configuration, the configurations alternating inside
every repeat, medians and ranges into profiles/ssgp.json.

    python scripts/ssgp_bench.py fit      # ut_ssgp_fit at (n, 64, 1024) and the gcc history, ut_gp_fit at n = 1024, 4096
    python scripts/ssgp_bench.py score    # ut_ssgp_score at 2^20 candidates, d = 64, D = 512 / 1024, beside
                                          # ut_gp_score_values (fp64) at n = 1024
    python scripts/ssgp_bench.py search   # tune_bandit, 64-D Rosenbrock, 400 tests, five seeds, GP and ssgp
    python scripts/ssgp_bench.py lml      # ut_ssgp_lml_grid, 16 points, D = 1024: beside 16 ut_ssgp_fit calls and (n <=
                                          # 4096) ut_gp_lml_grid; held-out RMSE / NLPD at the selected lengthscale
                                          # -> profiles/ssgp_lml.json

The Gram's share of the fp64 MFMA peak is taken from its own flops,
n_pad D (D + 128) (the lower tile pairs) plus the two feature contractions per
pair and step, against the time of the whole fit: a lower bound on the kernel's."""
import json
import os
import sys
import time

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from uptune_amd import spaces  # noqa: E402
from uptune_amd.engine import BatchEngine  # noqa: E402

REPEATS, PEAK_TF = 9, 78.6      # fp64 matrix peak of the MI355X, TFLOP/s
OUT = os.path.join(ROOT, "profiles", "ssgp.json")


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def alternate(jobs):
    """jobs: name -> callable; -> name -> dict(median_ms, min_ms, max_ms) over REPEATS alternating passes"""
    for fn in jobs.values():
        fn()                                                   # warm-up: allocations, code objects
    ms = {k: [] for k in jobs}
    for _ in range(REPEATS):
        for k, fn in jobs.items():
            ms[k].append(timed(fn))
    return {k: dict(median_ms=float(np.median(v)), min_ms=min(v), max_ms=max(v)) for k, v in ms.items()}


def gram_flops(n, d, D):
    npad, T = -(-n // 128) * 128, D // 128
    pairs, dpad = T * (T + 1) // 2, -(-d // 4) * 4
    return 2.0 * npad * 128 * 128 * pairs + 2.0 * npad * 128 * dpad * T * T


def bench_fit():
    rng = np.random.default_rng(0)
    eng = BatchEngine(spaces.r64(), device=0, seed=1)
    data = {n: (rng.uniform(size=(n, 64)), rng.standard_normal(n)) for n in (1024, 4096, 16384)}
    jobs = {}
    for n, (X, y) in data.items():
        jobs["ssgp_n%d_D1024" % n] = lambda X=X, y=y: eng.ssgp_fit(X, y, 2.0, features=1024)
    for n in (1024, 4096):
        jobs["gp_n%d" % n] = lambda X=data[n][0], y=data[n][1]: (eng.gp_fit(X, y, 2.0), eng.gp_fit_ok())
    out = alternate(jobs)
    for n in data:
        r = out["ssgp_n%d_D1024" % n]
        r["gram_peak_fraction_lower_bound"] = gram_flops(n, 64, 1024) / (r["median_ms"] * 1e-3) / (PEAK_TF * 1e12)
    # the gcc flag space's recorded history: its successful runs, encoded through the space (707 features)
    z = np.load(os.path.join(ROOT, "tests", "golden", "gcc_history.npz"))
    ok = np.flatnonzero(np.isfinite(z["qor"]))
    geng = BatchEngine(spaces.gcc(), device=0, seed=1)
    hv = torch.from_numpy(np.ascontiguousarray(z["values"][:, ok])).to(geng.device)
    X, y = geng.encode(hv).T.contiguous().cpu().numpy(), np.asarray(z["qor"][ok], dtype=np.float64)
    out.update(alternate({"ssgp_gcc_n%d_d%d_D1024" % X.shape: lambda: geng.ssgp_fit(X, y, 4.0, features=1024)}))
    return out


def bench_score():
    rng = np.random.default_rng(0)
    eng = BatchEngine(spaces.r64(), device=0, seed=1)
    X, y = rng.uniform(-1000, 1000, size=(1024, 64)), rng.standard_normal(1024)
    Xf = (X + 1000.0) / 2000.0
    cand = torch.from_numpy(rng.uniform(-1000, 1000, size=(64, 1 << 20))).to("cuda:0")
    eng.gp_fit(Xf, y, 2.0)
    jobs = {"gp_n1024_fp64": lambda: eng.gp_score_values(cand)}
    out = {}
    for D in (512, 1024):
        eng.ssgp_fit(Xf, y, 2.0, features=D)
        out.update(alternate({**jobs, "ssgp_D%d" % D: lambda: eng.ssgp_score(cand)}))
    return out


def bench_search():
    """tune_bandit on 64-D Rosenbrock, 100 generations of 4 (400 tests), the GP's default lengthscale, five
    seeds: best objective at the end with the default GP and with surrogate="ssgp" (D = 1024)"""
    from uptune_amd.tuner import tune_bandit

    def cost(cfg):
        x = np.array([cfg[i] for i in range(64)])
        return float(np.sum(100.0 * (x[1:] - x[:-1] ** 2) ** 2 + (1.0 - x[:-1]) ** 2))
    out = {}
    for name, kw in (("gp", {}), ("ssgp_D1024", {"surrogate": "ssgp"})):
        best = [float(tune_bandit(spaces.r64(), cost, generations=100, parallelism=4, seed=sd, **kw).best_result.time)
                for sd in range(5)]
        out[name] = dict(best=best, median=float(np.median(best)), min=min(best), max=max(best))
    return out


def gcc_history():
    z = np.load(os.path.join(ROOT, "tests", "golden", "gcc_history.npz"))
    ok = np.flatnonzero(np.isfinite(z["qor"]))
    eng = BatchEngine(spaces.gcc(), device=0, seed=1)
    V = np.ascontiguousarray(z["values"][:, ok])
    X = eng.encode(torch.from_numpy(V).to(eng.device)).T.contiguous().cpu().numpy()
    return eng, V, X, np.asarray(z["qor"][ok], dtype=np.float64)


def bench_lml():
    """the grid of SharedModel (sqrt(d) geomspace(0.05, 4, 16) on a unit base), sigma_n2 = 1e-2.  The Gram's share of
    the peak from its own MFMA flops (the lower tile pairs of every point) against the whole call: a lower bound"""
    rng, sn2, D, g = np.random.default_rng(0), 1e-2, 1024, 16
    eng = BatchEngine(spaces.r64(), device=0, seed=1)
    grid = lambda d: np.sqrt(d) * np.geomspace(0.05, 4.0, g)   # noqa: E731
    sets = {}
    for n in (1024, 4096, 16384, 65536):
        V = rng.uniform(-1000, 1000, size=(64, n))
        X = (V.T + 1000.0) / 2000.0
        sets["n%d_d64" % n] = (eng, V, X, np.sum((X - 0.4) ** 2, axis=1) + 0.05 * rng.standard_normal(n))
    sets["gcc"] = gcc_history()
    out = {}
    for name, (e, V, X, y) in sets.items():
        n, d = X.shape
        sc = grid(d)
        jobs = {"ssgp_grid": lambda: e.ssgp_lml_grid(X, y, 1.0, sc, features=D, sigma_n2=sn2),
                "ssgp_16_fits": lambda: [e.ssgp_fit(X, y, s, sigma_n2=sn2, features=D) for s in sc]}
        if n <= 4096:
            jobs["gp_grid"] = lambda: e.gp_lml_grid(X, y, 1.0, sc, sigma_n2=sn2)
        r = alternate(jobs)
        npad, T = -(-n // 128) * 128, D // 128
        r["gram_peak_fraction_lower_bound"] = (g * 2.0 * npad * 128 * 128 * T * (T + 1) / 2 /
                                               (r["ssgp_grid"]["median_ms"] * 1e-3) / (PEAK_TF * 1e12))
        out[name] = r
        if name not in ("n16384_d64", "gcc"):
            continue
        # quality: a 20 % hold-out; the posterior in standardised units, s^2 = var + sigma_n2
        perm = rng.permutation(n)
        te, tr = perm[:n // 5], perm[n // 5:]
        lml, best = e.ssgp_lml_grid(X[tr], y[tr], 1.0, sc, features=D, sigma_n2=sn2)
        ells = {"selected": float(sc[best]), "default_0.3": 0.3}
        if len(tr) <= 4096:
            ells["gp_selected"] = float(sc[e.gp_lml_grid(X[tr], y[tr], 1.0, sc, sigma_n2=sn2)[1]])
        mean, sd = float(np.mean(y[tr])), float(np.std(y[tr])) or 1.0
        cand = torch.from_numpy(np.ascontiguousarray(V[:, te])).to(e.device)
        q = dict(lml=[float(v) for v in lml])
        for k, ell in ells.items():
            e.ssgp_fit(X[tr], y[tr], ell, sigma_n2=sn2, features=D)
            mu, var, _ = (t.cpu().numpy() for t in e.ssgp_score(cand))
            res, s2 = (y[te] - mean) / sd - mu, var + sn2
            q[k] = dict(lengthscale=ell, rmse=float(np.sqrt(np.mean(res ** 2))),
                        nlpd=float(np.mean(0.5 * np.log(2.0 * np.pi * s2) + res ** 2 / (2.0 * s2))))
        out[name]["held_out"] = q
    return out


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "fit"
    if what == "lml":
        OUT = os.path.join(ROOT, "profiles", "ssgp_lml.json")
    res = json.load(open(OUT)) if os.path.exists(OUT) else {}
    res[what] = {"fit": bench_fit, "score": bench_score, "search": bench_search, "lml": bench_lml}[what]()
    res["repeats"] = REPEATS
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res[what], indent=1, sort_keys=True))
