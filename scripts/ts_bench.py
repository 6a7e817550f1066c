"""Times of Thompson sampling's three calls (profiles/ts.json).

    python scripts/ts_bench.py times --out profiles/ts.json
    python scripts/ts_bench.py search --out profiles/ts.json

times.  Per shape (m candidates, d features, n training rows, D random features, q
paths) on a fit in place: ut_gp_ts_draw, ut_gp_ts_eval (every path at every
candidate, F [q][m]) and ut_gp_ts_select (k = q picks) by device events around
each call, the median of the repeats after two warm-up calls, with the
spread; and, from the same process on the same fit and candidates, a dense EI
round's ut_gp_score_values + ut_topk (k = q) for scale.

The eval's arithmetic, from the shapes: both contractions of k_ts_paths over
the n + D rows of both row sets, the first repeated for every group of 32
paths, 2 m (npad + D) (dpad groups + 32 groups) flop (padded paths and rows
included: they are computed).  Its share of the fp64 matrix peak is that over
the eval's time over 78.6 TF (spec).  The shader clock is read from the
driver's pp_dpm_sclk before and after where the file is readable.

search.  The search effect of acq="ts" against acq="ei", both with
trust_region=True, five seeds each, in the two settings of scripts/tr_bench.py:
C1 (bandit_a, 5000 tests, the polish table's setting: best objective at the
end) and tune_bandit on spaces.r64() with the 64-D Rosenbrock objective
(generations=100, lengthscale="auto": best objective among the requests of
generations < 25 / 50 / 100).  Each mode keeps the other's record in --out."""
import argparse
import glob
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [dict(m=1 << 20, d=64, n=1024, D=1024, q=16), dict(m=1 << 20, d=64, n=1024, D=1024, q=256),
          dict(m=1 << 20, d=64, n=4096, D=1024, q=16)]
HYP = dict(sigma_f2=1.0, sigma_n2=1e-2, jitter=1e-8)
PEAK_FP64_TF = 78.6


def sclk():
    """the active shader clock level of every card, as the driver prints it; None when not readable"""
    out = []
    for p in sorted(glob.glob("/sys/class/drm/card*/device/pp_dpm_sclk")):
        try:
            with open(p) as f:
                out += [ln.strip() for ln in f if "*" in ln]
        except OSError:
            pass
    return out or None


def data(n, d):
    rng = np.random.default_rng(n + d)
    X = rng.uniform(size=(n, d))
    return X, np.sum((X - 0.4) ** 2, axis=1) + 0.01 * rng.standard_normal(n)


def timed(fn, repeats):
    import torch
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(repeats):
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        fn()
        b.record()
        b.synchronize()
        ts.append(a.elapsed_time(b))
    return dict(median_ms=float(np.median(ts)), min_ms=float(np.min(ts)), max_ms=float(np.max(ts)), repeats=repeats)


def run(repeats, shapes):
    import torch
    from uptune_amd.engine import BatchEngine
    from uptune_amd.manipulator import ConfigurationManipulator, FloatParameter
    assert torch.cuda.is_available(), "ts_bench needs a GPU"
    out = []
    clk0 = sclk()
    for s in shapes:
        m, d, n, D, q = s["m"], s["d"], s["n"], s["D"], s["q"]
        X, y = data(n, d)
        e = BatchEngine(ConfigurationManipulator([FloatParameter(f"u{j}", 0.0, 1.0) for j in range(d)]), device=0)
        e.gp_fit(X, y, lengthscale=2.0, **HYP)
        U = torch.rand((d, m), dtype=torch.float64, device="cuda:0", generator=torch.Generator("cuda:0").manual_seed(7))
        acq = e.acq("ei")
        rnd = [0]

        def draw():
            rnd[0] += 1
            e.gp_ts_draw(q, D, round_=rnd[0])
        t_draw = timed(draw, repeats)
        t_eval = timed(lambda: e.gp_ts_eval(U), repeats)
        t_sel = timed(lambda: e.gp_ts_select(U, q), repeats)
        pos = e.gp_ts_select(U, q)[0]

        def ei():
            _, _, sc = e.gp_score_values(U, acq=acq)
            return e.topk(sc, q)
        t_ei = timed(ei, repeats)
        groups = (q + 31) // 32
        npad, dpad = (n + 127) // 128 * 128, (d + 3) // 4 * 4
        flop = 2.0 * m * (npad + D) * (dpad * groups + 32 * groups)
        rec = dict(s, ts_draw=t_draw, ts_eval=t_eval, ts_select=t_sel, ei_score_values_topk=t_ei,
                   eval_gflop=1e-9 * flop, eval_tflops=1e-9 * flop / t_eval["median_ms"],
                   eval_share_of_fp64_matrix_peak=1e-9 * flop / t_eval["median_ms"] / PEAK_FP64_TF,
                   picks=int((pos >= 0).sum().item()), distinct=int(torch.unique(pos).numel()))
        out.append(rec)
        print(json.dumps(rec), flush=True)
        e.close()
        del U
        torch.cuda.empty_cache()
    return dict(what="ut_gp_ts_draw / _eval / _select on a fit in place by device events around each call (median, "
                     "min, max of the repeats after two warm-up calls); a dense EI round's ut_gp_score_values + "
                     "ut_topk from the same process for scale; the eval's flop from the shapes over the fp64 "
                     "matrix spec peak", peak_fp64_tf=PEAK_FP64_TF, sclk_before=clk0, sclk_after=sclk(), shapes=out)


def _rosen2(cfg):
    x0, x1 = cfg[0], cfg[1]
    return 100.0 * (x1 - x0 * x0) ** 2 + (x0 - 1.0) ** 2


def _rosen64(cfg):
    x = np.array([cfg[i] for i in range(64)])
    return float(np.sum(100.0 * (x[1:] - x[:-1] ** 2) ** 2 + (x[:-1] - 1.0) ** 2))


def _arm_stats(d):
    arm = d.root_technique.techniques[-1]
    return dict(arm_requests=arm.request_count, arm_restarts=arm.tr.restarts if arm.tr else 0,
                ts_draws=d.root_technique.techniques[0].model.ts_rounds)


def search(seeds, generations=100):
    from uptune_amd import spaces
    from uptune_amd import technique as T
    from uptune_amd.driver import SearchDriver
    from uptune_amd.manipulator import ConfigurationManipulator, FloatParameter
    from uptune_amd.tuner import tune_bandit
    c1, r64 = [], []
    for acq in ("ei", "ts"):
        for seed in seeds:
            m = ConfigurationManipulator([FloatParameter(0, -1000.0, 1000.0), FloatParameter(1, -1000.0, 1000.0)])
            meta = T.bandit_a(bandit_seed=seed, pool=4096, batch=8, population=30, seed=11, lengthscale=0.3,
                              y_transform="rank", trust_region=True, acq=acq)
            d = SearchDriver(m, meta, parallelism=4)
            t0 = time.perf_counter()
            best = d.main(_rosen2, test_limit=5000)
            rec = dict(bandit_seed=seed, acq=acq, best=float(best.time), tests=int(d.test_count),
                       unique=len(d.results) == len(d.seen_hashes()), wall_s=time.perf_counter() - t0, **_arm_stats(d))
            c1.append(rec)
            print(json.dumps(rec), flush=True)
    for acq in ("ei", "ts"):
        for seed in seeds:
            t0 = time.perf_counter()
            d = tune_bandit(spaces.r64(), _rosen64, generations=generations, lengthscale="auto", seed=seed,
                            trust_region=True, acq=acq)
            by_gen = {}
            for g in (25, 50, 100):
                ts = [q.result.time for q in d.requests_query() if q.result is not None and q.generation < g]
                by_gen[str(g)] = float(min(ts)) if ts else None
            rec = dict(seed=seed, acq=acq, best_by_generation=by_gen, tests=int(d.test_count),
                       wall_s=time.perf_counter() - t0, **_arm_stats(d))
            r64.append(rec)
            print(json.dumps(rec), flush=True)
    return dict(search_what="acq='ts' against acq='ei', trust_region=True on both: C1 (bandit_a, 5000 tests, best "
                            "objective at the end, per bandit seed) and tune_bandit on spaces.r64() with the 64-D "
                            "Rosenbrock objective (generations=100, lengthscale='auto', best objective among the "
                            "requests of generations < 25 / 50 / 100, per seed)", c1_runs=c1, r64_runs=r64)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("times", "search"), nargs="?", default="times")
    ap.add_argument("--seeds", type=int, nargs="*", default=[0, 1, 2, 3, 4])
    ap.add_argument("--out", default=os.path.join("profiles", "ts.json"))
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--small", action="store_true", help="the shapes at m = 2^14 (a rehearsal of the script)")
    a = ap.parse_args()
    shapes = [dict(s, m=1 << 14) for s in SHAPES] if a.small else SHAPES
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    res.update(run(a.repeats, shapes) if a.what == "times" else search(a.seeds))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
