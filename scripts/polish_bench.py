"""Device time of ut_gp_acq_grad and ut_gp_polish (T = 8), and the polish's
effect on the C1 search (profiles/polish.json).

    python scripts/polish_bench.py --out profiles/polish.json            # the timings
    python scripts/polish_bench.py --out profiles/polish.json --c1 0 1 2 3 4   # the search effect

Timings.  Per shape (n training rows, d features, p candidates) on a fit in
place, after one warm-up call: nine calls, each a timing round of its own with
the library's stage events on (ut_set_timing / ut_stage_time: HIP events
recorded on the stream between the stages, so nothing of the host is in them).
A stage's time in a call is its mean over its occurrences times their count
(ut_gp_acq_grad runs every stage once; ut_gp_polish with T steps runs K*, V and
the tail 2 T + 1 times, W and the gradient T times); the call's time is the sum
of its stages.  Reported: the median over the nine calls, with the smallest and
largest.  Stages:
  kstar  encode + K*^T (the fp64 K* kernel over every feature)
  v      V = L^-1 K*^T (k_bs_v)
  tail   mu, var, score, the gradient's two coefficients per candidate
  w      W = L^-T V
  grad   the two gradient products and their epilogue
  step   (polish) mask / project / trial and accept / reject
  final  (polish) decode, re-encode; its K*, V and tail are in those stages
ut_gp_select_batch's bs_v stage (k_bs_v and the mean) at the same shape, in the
same process, is the yardstick for the two triangular products.

Search effect (--c1 SEEDS).  C1 as tests/test_gpu_c1.py sets it up
(Rosenbrock on [-1000, 1000]^2, technique.bandit_a, pool 4096, batch 8,
population 30, lengthscale 0.3, rank-transformed targets, parallelism 4, 5000
tests), once with polish=0 and once with polish=8 per bandit seed; the best
objective after 5000 tests of each run is recorded, nothing else is claimed."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [dict(n=1024, d=64, p=1024), dict(n=4096, d=64, p=4096)]
HYP = dict(sigma_f2=1.0, sigma_n2=1e-2, jitter=1e-8)
T = 8
REPEATS = 9
GRAD_STAGES = [("kstar", "pl_kstar", 1), ("v", "pl_v", 1), ("tail", "pl_tail", 1), ("w", "pl_w", 1),
               ("grad", "pl_grad", 1)]
POLISH_STAGES = [("kstar", "pl_kstar", 2 * T + 1), ("v", "pl_v", 2 * T + 1), ("tail", "pl_tail", 2 * T + 1),
                 ("w", "pl_w", T), ("grad", "pl_grad", T), ("step", "pl_step", T), ("final", "pl_final", 1)]


def data(n, d):
    rng = np.random.default_rng(n + d)
    X = rng.uniform(size=(n, d))
    return X, np.sum((X - 0.4) ** 2, axis=1) + 0.01 * rng.standard_normal(n)


def timed(e, call, stages):
    """nine calls, each its own timing round: -> {stage: [ms per call]}, 'total' among them"""
    import torch
    call()
    torch.cuda.synchronize()
    per = {name: [] for name, _, _ in stages}
    per["total"] = []
    for _ in range(REPEATS):
        e.set_timing(True)
        call()
        one = {name: e.stage_time(key) * count for name, key, count in stages}
        e.set_timing(False)
        for name, v in one.items():
            per[name].append(v)
        per["total"].append(sum(one.values()))
    return per


def summary(per):
    return {name: dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)))
            for name, v in per.items()}


def timings():
    import torch
    from uptune_amd.engine import BatchEngine
    from uptune_amd.manipulator import ConfigurationManipulator, FloatParameter
    assert torch.cuda.is_available(), "polish_bench needs a GPU"
    out = []
    for s in SHAPES:
        n, d, p = s["n"], s["d"], s["p"]
        X, y = data(n, d)
        e = BatchEngine(ConfigurationManipulator([FloatParameter(f"u{j}", 0.0, 1.0) for j in range(d)]), device=0)
        e.gp_fit(X, y, lengthscale=2.0, **HYP)
        U = torch.from_numpy(np.random.default_rng(7000 + n).uniform(size=(d, p))).to("cuda:0")
        acq = e.acq("ei")
        grad = summary(timed(e, lambda: e.gp_acq_grad(U, acq=acq), GRAD_STAGES))
        pol = summary(timed(e, lambda: e.gp_polish(U, T, acq=acq), POLISH_STAGES))
        sel = summary(timed(e, lambda: e.gp_select_batch(U, 8, acq=acq), [("bs_v", "bs_v", 1)]))
        vals, score, score0, moved = e.gp_polish(U, T, acq=acq)
        # the triangular products need n^2 p flops each, the two gradient products 2 n d p each
        gf_tri, gf_grad = 1e-9 * n * n * p, 4e-9 * n * d * p
        rec = dict(s, steps=T, repeats=REPEATS, acq_grad=grad, polish=pol, select_batch_bs_v=sel["bs_v"],
                   gflop_v=gf_tri, gflop_w=gf_tri, gflop_grad=gf_grad,
                   tflops_v=gf_tri / grad["v"]["median_ms"], tflops_w=gf_tri / grad["w"]["median_ms"],
                   tflops_grad=gf_grad / grad["grad"]["median_ms"],
                   moved=int(moved.sum().item()), best_score0=float(score0.max().item()),
                   best_score=float(score.max().item()))
        out.append(rec)
        print(json.dumps(rec), flush=True)
        e.close()
    return dict(what="ut_gp_acq_grad and ut_gp_polish (T = 8) on a fit in place: device time by the library's stage "
                     "events, median of nine calls after a warm-up; ut_gp_select_batch's bs_v stage as the yardstick",
                shapes=out)


def _rosen(cfg):
    x0, x1 = cfg[0], cfg[1]
    return 100.0 * (x1 - x0 * x0) ** 2 + (x0 - 1.0) ** 2


def c1(seeds, polish, log):
    from uptune_amd import technique as T_
    from uptune_amd.driver import SearchDriver
    from uptune_amd.manipulator import ConfigurationManipulator, FloatParameter
    runs = []
    for seed in seeds:
        m = ConfigurationManipulator([FloatParameter(0, -1000.0, 1000.0), FloatParameter(1, -1000.0, 1000.0)])
        meta = T_.bandit_a(bandit_seed=seed, pool=4096, batch=8, population=30, seed=11, lengthscale=0.3,
                           y_transform="rank", polish=polish)
        d = SearchDriver(m, meta, parallelism=4)
        t0 = time.perf_counter()
        best = d.main(_rosen, test_limit=5000)
        rec = dict(bandit_seed=seed, polish=polish, best=float(best.time), tests=int(d.test_count),
                   unique=len(d.results) == len(d.seen_hashes()), wall_s=time.perf_counter() - t0)
        runs.append(rec)
        print(json.dumps(rec), flush=True)
        if log:
            with open(log, "a") as f:
                f.write(json.dumps(rec) + "\n")
    return runs


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "polish.json"))
    ap.add_argument("--c1", type=int, nargs="*", default=None, help="bandit seeds of the C1 search-effect runs")
    ap.add_argument("--polish", type=int, nargs="*", default=[0, T], help="polish settings of the C1 runs")
    ap.add_argument("--log", default=None, help="append every finished C1 run to this file as well")
    a = ap.parse_args()
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    if a.c1 is None:
        res.update(timings())
    else:
        runs = [r for r in res.get("c1_runs", [])]
        for pol in a.polish:
            runs += c1(a.c1, pol, a.log)
        res["c1"] = ("C1 (tests/test_gpu_c1.py's setting) with polish=0 and polish=8: the best objective after 5000 "
                     "tests per bandit seed")
        res["c1_runs"] = sorted(runs, key=lambda r: (r["polish"], r["bandit_seed"]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
