"""Fit and scoring time of the sparse-spectrum GP beside the exact GP, in one
process: nine repeats per configuration, the configurations alternating inside
every repeat, medians and ranges into profiles/ssgp.json.

    python scripts/ssgp_bench.py fit      # ut_ssgp_fit at (n, 64, 1024) and the gcc history, ut_gp_fit at n = 1024, 4096
    python scripts/ssgp_bench.py score    # ut_ssgp_score at 2^20 candidates, d = 64, D = 512 / 1024, beside
                                          # ut_gp_score_values (fp64) at n = 1024
    python scripts/ssgp_bench.py search   # tune_bandit, 64-D Rosenbrock, 400 tests, five seeds, GP and ssgp

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


if __name__ == "__main__":
    what = sys.argv[1] if len(sys.argv) > 1 else "fit"
    res = json.load(open(OUT)) if os.path.exists(OUT) else {}
    res[what] = {"fit": bench_fit, "score": bench_score, "search": bench_search}[what]()
    res["repeats"] = REPEATS
    with open(OUT, "w") as f:
        json.dump(res, f, indent=1, sort_keys=True)
    print(json.dumps(res[what], indent=1, sort_keys=True))
