"""Trust-region proposals: kernel time, whether the GP has anything to say
inside the box, and the effect of the arm on two searches (profiles/tr.json).

    python scripts/tr_bench.py kernel                 # ut_propose_tr beside ut_propose_ga
    python scripts/tr_bench.py informative            # a C2-shaped dense round on a DE pool and on a box pool
    python scripts/tr_bench.py c1 --seeds 0 1 2 3 4   # bandit_a on C1 with and without the arm
    python scripts/tr_bench.py r64 --seeds 0 1 2 3 4  # tune_bandit on 64-D Rosenbrock with and without it

kernel.  ut_propose_tr at C2 (R64, m = 2^20, prob = 20 / 64) and C3 (hpl64,
m = 2^21), alternating in one process with ut_propose_ga(normal=1,
mutation_rate=prob, parent1=centre) at the same shape.  A stand-alone proposal
call records no stage events of the library (they belong to the scoring
rounds), so each call is bracketed by two events on the library's stream --
the same measurement, taken by the script.  Median of nine after a warm-up,
with min and max; write bandwidth = 8 * ncols * m bytes over the time.

informative.  n = 1024 random R64 results, lengthscale 0.2, precision 8: one
dense scoring call on 2^20 DE trials and one on 2^20 box candidates (L = 0.8
around the best row); ut_gp_kstar_screen_stats' certified share and the number
of distinct scores among the top 256 of each.

c1 / r64.  C1 as scripts/polish_bench.py runs it (bandit_a, 5000 tests), and
tune_bandit on spaces.r64() with the 64-D Rosenbrock objective, generations =
100, lengthscale="auto"; each with and without trust_region=True per bandit
seed.  Recorded as measured, nothing else is claimed."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

REPEATS = 9
HBM_BYTES_PER_S = 6.3e12


def _summary(ms, nbytes):
    med = float(np.median(ms))
    return dict(median_ms=med, min_ms=float(np.min(ms)), max_ms=float(np.max(ms)),
                write_gb_s=nbytes / med * 1e-6, share_of_hbm=nbytes / (med * 1e-3) / HBM_BYTES_PER_S)


def kernel():
    import torch
    from uptune_amd import spaces
    from uptune_amd.engine import BatchEngine
    from uptune_amd.trust_region import TrustRegion
    out = []
    for name, manip, m in (("c2_r64", spaces.r64(), 1 << 20), ("c3_hpl64", spaces.hpl64(), 1 << 21)):
        e = BatchEngine(manip, device=0, seed=5)
        e.population_init(4, round_=0)
        centre = e.population_get()[:, 1].cpu().numpy().copy()      # a random configuration
        tr = TrustRegion(e.spec.P, 8)
        prob, cat = tr.probs()
        half = tr.half_widths(e.spec, 0.2)
        stream = torch.cuda.current_stream(e.device)

        def timed(call):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            call()
            b.record(stream)
            b.synchronize()
            return a.elapsed_time(b)

        def tr_call():
            return e.propose_tr(m, centre, half, prob, cat, round_=1, cand_base=0)

        def ga_call():
            return e.propose_ga(m, parent1=centre, round_=1, cand_base=0, mutation_rate=prob, normal=True)

        tr_call(), ga_call()
        torch.cuda.synchronize()
        t_tr, t_ga = [], []
        for _ in range(REPEATS):
            t_tr.append(timed(tr_call))
            t_ga.append(timed(ga_call))
        vals, inv = tr_call()
        nbytes = 8 * e.spec.ncols * m
        rec = dict(shape=name, m=m, ncols=e.spec.ncols, prob=prob, cat_prob=cat, L=tr.L, repeats=REPEATS,
                   propose_tr=_summary(t_tr, nbytes), propose_ga=_summary(t_ga, nbytes),
                   tr_over_ga=float(np.median(t_tr) / np.median(t_ga)), invalid=int(inv.sum().item()))
        out.append(rec)
        print(json.dumps(rec), flush=True)
        e.close()
    return dict(kernel_what="ut_propose_tr and ut_propose_ga(normal=1, mutation_rate=prob, parent1=centre) alternating "
                            "in one process: device time between two events on the library's stream, median of nine "
                            "after a warm-up", kernel=out)


def informative():
    import torch
    from uptune_amd import spaces
    from uptune_amd.engine import BatchEngine
    from uptune_amd.trust_region import TrustRegion
    m, n, k = 1 << 20, 1024, 256
    e = BatchEngine(spaces.r64(), device=0, seed=9)
    e.population_init(n, round_=7)
    rows = e.population_get()
    X = e.encode(rows).T.contiguous().cpu().numpy()
    r = rows.cpu().numpy()
    y = np.sum(100.0 * (r[1:] - r[:-1] ** 2) ** 2 + (r[:-1] - 1.0) ** 2, axis=0)
    best = r[:, int(np.argmin(y))].copy()
    e.gp_set_precision(8)
    e.gp_fit(X, y, lengthscale=0.2, sigma_f2=1.0, sigma_n2=1e-6, jitter=1e-8)
    e.population_init(4096, round_=0)
    tr = TrustRegion(e.spec.P, 8)
    prob, cat = tr.probs()
    pools = dict(de=e.propose_de(m, round_=1, cr=0.2, best=best),
                 trust_region=e.propose_tr(m, best, tr.half_widths(e.spec, 0.2), prob, cat, round_=1)[0])
    out = {}
    for name, vals in pools.items():
        for _ in range(2):      # the second call runs with the hints the first one left
            mu, var, score = e.gp_score_values(vals, acq=e.acq("ei"))
            screened, cert, units = e.gp_kstar_screen_stats()
        _, top = e.topk(score, k)
        s = score.cpu().numpy()
        out[name] = dict(screened=screened, certified=cert, units=units, certified_share=cert / units if units else None,
                         distinct_top256=int(len(np.unique(top.cpu().numpy()))), distinct_scores=int(len(np.unique(s))),
                         var_min=float(var.min().item()), var_max=float(var.max().item()))
        print(name, json.dumps(out[name]), flush=True)
    e.close()
    return dict(informative_what="n = 1024 random R64 results, lengthscale 0.2, precision 8, 2^20 candidates: the K* "
                                 "screen's certified units and the distinct scores among the top 256, on a DE pool and "
                                 "on a trust-region pool (L = 0.8 around the best row)", informative=out)


def _rosen2(cfg):
    x0, x1 = cfg[0], cfg[1]
    return 100.0 * (x1 - x0 * x0) ** 2 + (x0 - 1.0) ** 2


def _rosen64(cfg):
    x = np.array([cfg[i] for i in range(64)])
    return float(np.sum(100.0 * (x[1:] - x[:-1] ** 2) ** 2 + (x[:-1] - 1.0) ** 2))


def c1(seeds):
    from uptune_amd import technique as T
    from uptune_amd.driver import SearchDriver
    from uptune_amd.manipulator import ConfigurationManipulator, FloatParameter
    runs = []
    for arm in (False, True):
        for seed in seeds:
            m = ConfigurationManipulator([FloatParameter(0, -1000.0, 1000.0), FloatParameter(1, -1000.0, 1000.0)])
            kw = dict(trust_region=True) if arm else {}
            meta = T.bandit_a(bandit_seed=seed, pool=4096, batch=8, population=30, seed=11, lengthscale=0.3,
                              y_transform="rank", **kw)
            d = SearchDriver(m, meta, parallelism=4)
            t0 = time.perf_counter()
            best = d.main(_rosen2, test_limit=5000)
            rec = dict(bandit_seed=seed, trust_region=arm, best=float(best.time), tests=int(d.test_count),
                       unique=len(d.results) == len(d.seen_hashes()), wall_s=time.perf_counter() - t0)
            if arm:
                t = d.root_technique.techniques[-1]
                rec.update(arm_requests=t.request_count, arm_restarts=t.tr.restarts if t.tr else 0)
            runs.append(rec)
            print(json.dumps(rec), flush=True)
    return dict(c1_what="C1 (bandit_a, 5000 tests, the polish table's setting) with and without trust_region=True: the "
                        "best objective after 5004 tests per bandit seed", c1_runs=runs)


def r64(seeds, generations=100):
    from uptune_amd import spaces
    from uptune_amd.tuner import tune_bandit
    runs = []
    for arm in (False, True):
        for seed in seeds:
            t0 = time.perf_counter()
            d = tune_bandit(spaces.r64(), _rosen64, generations=generations, lengthscale="auto", seed=seed,
                            trust_region=arm)
            by_gen = {}
            for g in (25, 50, 100):
                ts = [q.result.time for q in d.requests_query() if q.result is not None and q.generation < g]
                by_gen[str(g)] = float(min(ts)) if ts else None
            rec = dict(seed=seed, trust_region=arm, best_by_generation=by_gen, tests=int(d.test_count),
                       wall_s=time.perf_counter() - t0)
            if arm:
                t = d.root_technique.techniques[-1]
                rec.update(arm_requests=t.request_count, arm_restarts=t.tr.restarts if t.tr else 0,
                           arm_L=t.tr.L if t.tr else None)
            runs.append(rec)
            print(json.dumps(rec), flush=True)
    return dict(r64_what="tune_bandit on spaces.r64() with the 64-D Rosenbrock objective, generations=100, "
                         "lengthscale='auto', with and without trust_region=True: the best objective among the "
                         "requests of generations < 25 / 50 / 100", r64_runs=runs)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("kernel", "informative", "c1", "r64"))
    ap.add_argument("--out", default=os.path.join("profiles", "tr.json"))
    ap.add_argument("--seeds", type=int, nargs="*", default=[0, 1, 2, 3, 4])
    a = ap.parse_args()
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    res.update(dict(kernel=kernel, informative=informative, c1=lambda: c1(a.seeds), r64=lambda: r64(a.seeds))[a.what]())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
