"""CMA-ES proposals: kernel time beside its comparators, and the effect of the
arm on the 64-D Rosenbrock search (profiles/cma.json).

    python scripts/cma_bench.py kernel
    python scripts/cma_bench.py r64 --seeds 0 1 2 3 4

kernel.  ut_propose_cma at m = 2^20 on R64 (dn = 64) and on the same space with
128 parameters (dn = 128), a dense lower-triangular factor, sigma = 0.3, with
and without out_unit, alternating in one process with
  * ut_propose_tr (prob = 20 / P) and ut_propose_ga(normal=1) on the same space,
  * the same samples composed from torch ops on the device
    (torch.randn(m, dn) @ A.T, mirror, scale to the range, transposed store),
  * a bare store of ncols x m doubles (the HBM floor).
A stand-alone proposal call records no stage events of the library, so each
call is bracketed by two events on the library's stream.  Median of nine after
a warm-up, with min and max.  No target time is fixed: the ratios are reported,
and whether the stores bound the kernel is read off the floor and off what the
second output (out_unit, as many bytes again) adds.

r64.  spaces.r64() with the 64-D Rosenbrock objective, 400 tests (generations =
100, parallelism 4), lengthscale="auto", per seed: tune_bandit as it is, with
cma=True, and GpuCMAES stand-alone with preselect on and off.  Median and range
of the best objective, and the requests the bandit gave the arm.  Recorded as
measured, nothing else is claimed."""
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
    m = 1 << 20
    for dn in (64, 128):
        e = BatchEngine(spaces.r64(dn), device=0, seed=5)
        e.population_init(4, round_=0)
        centre = e.population_get()[:, 1].cpu().numpy().copy()
        rng = np.random.default_rng(dn)
        B = rng.normal(size=(dn, dn)) / np.sqrt(dn)
        A = np.linalg.cholesky(B @ B.T + 1e-3 * np.eye(dn))
        mean = rng.uniform(0.3, 0.7, dn)
        tr = TrustRegion(e.spec.P, 8)
        prob, cat = tr.probs()
        half = tr.half_widths(e.spec, 0.2)
        stream = torch.cuda.current_stream(e.device)
        At = torch.from_numpy(A.T.copy()).to(e.device)
        mean_t = torch.from_numpy(mean).to(e.device)
        buf = torch.empty(e.spec.ncols, m, dtype=torch.float64, device=e.device)

        def timed(call):
            a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            a.record(stream)
            call()
            b.record(stream)
            b.synchronize()
            return a.elapsed_time(b)

        def torch_call():
            x = mean_t + 0.3 * (torch.randn(m, dn, dtype=torch.float64, device=e.device) @ At)
            a = x.abs()
            t = a - 2.0 * torch.floor(a * 0.5)
            u = torch.where(t > 1.0, 2.0 - t, t)
            buf.copy_((u * 2000.0 - 1000.0).T)

        calls = dict(
            propose_cma=lambda: e.propose_cma(m, centre, mean, A, 0.3, 0.0, round_=1, with_unit=False),
            propose_cma_unit=lambda: e.propose_cma(m, centre, mean, A, 0.3, 0.0, round_=1, with_unit=True),
            propose_tr=lambda: e.propose_tr(m, centre, half, prob, cat, round_=1, cand_base=0),
            propose_ga=lambda: e.propose_ga(m, parent1=centre, round_=1, cand_base=0, mutation_rate=prob, normal=True),
            torch_ops=torch_call,
            bare_store=lambda: buf.fill_(1.0))
        for c in calls.values():
            c()
        torch.cuda.synchronize()
        ts = {k: [] for k in calls}
        for _ in range(REPEATS):
            for k, c in calls.items():
                ts[k].append(timed(c))
        nbytes = 8 * e.spec.ncols * m
        rec = dict(dn=dn, m=m, ncols=e.spec.ncols, repeats=REPEATS,
                   **{k: _summary(v, nbytes * (2 if k == "propose_cma_unit" else 1)) for k, v in ts.items()})
        cm = rec["propose_cma"]["median_ms"]
        rec["cma_over"] = {k: cm / rec[k]["median_ms"] for k in calls if k != "propose_cma"}
        out.append(rec)
        print(json.dumps(rec), flush=True)
        e.close()
    return dict(kernel_what="ut_propose_cma (without / with out_unit) alternating in one process with ut_propose_tr, "
                            "ut_propose_ga(normal=1), the same samples from torch ops and a bare store of ncols x m "
                            "doubles: device time between two events on the library's stream, median of nine after a "
                            "warm-up; cma_over = propose_cma's median over each comparator's", kernel=out)


def _rosen64(cfg):
    x = np.array([cfg[i] for i in range(64)])
    return float(np.sum(100.0 * (x[1:] - x[:-1] ** 2) ** 2 + (x[:-1] - 1.0) ** 2))


def r64(seeds, generations=100):
    from uptune_amd import spaces
    from uptune_amd import technique as T
    from uptune_amd.driver import SearchDriver
    from uptune_amd.tuner import tune_bandit
    runs = []
    for variant in ("default", "cma_arm", "cma_alone_preselect", "cma_alone_plain"):
        for seed in seeds:
            t0 = time.perf_counter()
            if variant in ("default", "cma_arm"):
                d = tune_bandit(spaces.r64(), _rosen64, generations=generations, lengthscale="auto", seed=seed,
                                cma=variant == "cma_arm")
                t = d.root_technique.techniques[-1] if variant == "cma_arm" else None
            else:
                t = T.GpuCMAES(name="gpu-cma-es", pool=1 << 16, batch=8, seed=seed, lengthscale="auto",
                               preselect=variant == "cma_alone_preselect")
                d = SearchDriver(spaces.r64(), t, parallelism=4)
                d.main(_rosen64, test_limit=generations * 4, max_generations=generations)
                t = d.root_technique
            rec = dict(variant=variant, seed=seed, best=float(d.best_result.time), tests=int(d.test_count),
                       wall_s=time.perf_counter() - t0)
            if t is not None:
                rec.update(arm_requests=t.request_count, arm_generations=t.cma.generation if t.cma else 0,
                           arm_restarts=t.cma.restarts if t.cma else 0, arm_sigma=t.cma.sigma if t.cma else None)
            runs.append(rec)
            print(json.dumps(rec), flush=True)
    table = {}
    for variant in ("default", "cma_arm", "cma_alone_preselect", "cma_alone_plain"):
        b = [r["best"] for r in runs if r["variant"] == variant]
        table[variant] = dict(median=float(np.median(b)), min=float(np.min(b)), max=float(np.max(b)))
    print(json.dumps(table), flush=True)
    return dict(r64_what="spaces.r64() with the 64-D Rosenbrock objective, 400 tests, lengthscale='auto': tune_bandit as "
                         "it is (default), with cma=True (cma_arm), and GpuCMAES stand-alone with preselect on / off; "
                         "the best objective per seed, its median and range per variant", r64_runs=runs, r64_table=table)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("what", choices=("kernel", "r64"))
    ap.add_argument("--out", default=os.path.join("profiles", "cma.json"))
    ap.add_argument("--seeds", type=int, nargs="*", default=[0, 1, 2, 3, 4])
    a = ap.parse_args()
    res = {}
    if os.path.exists(a.out):
        with open(a.out) as f:
            res = json.load(f)
    res.update(dict(kernel=kernel, r64=lambda: r64(a.seeds))[a.what]())
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
