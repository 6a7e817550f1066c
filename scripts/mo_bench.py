"""Device time of two-objective scoring and its search effect (profiles/mo.json).

    python scripts/mo_bench.py --out profiles/mo.json [--parent-tree DIR]

Every step runs in a child process of its own under `timeout`, in a fixed
order, and the first one that fails ends the script (nothing more is started
on the device after a fault or a hang).  The steps:

  c2_tail      at the C2 shape (m = 2^20 candidates, d = 64, n = 1024, the bench's
               data and lengthscale), fronts of 16, 64 and 256 rows: the EHVI tail
               by device events inside ut_gp_mo_score (stage `mo_means`, the
               column-sum K* with alpha_2, and stage `mo_ehvi`, k_mo_ehvi) and the
               whole call by the host clock around call + synchronise; in the same
               process the constrained tail with one constraint (stage `cons` of
               ut_gp_cons_prob) and the plain EI score of the same pool
               (ut_gp_score_values, host clock)
  front        k_mo_mark + k_mo_place (stage `mo_front`) at n = 1024 and n = 4096,
               for a front of every row (Y2 = -y) and a generic one
  c2_round     the bench's DE round (precision 8, an asynchronous refit per round)
               with nothing loaded, by the host clock around round + synchronise;
               five runs (processes) of this tree and, with --parent-tree (a built
               checkout of the parent commit), five of that, alternating
  zdt1         ZDT1 in 8 dimensions through tune_bandit, 400 tests, seeds 0 .. 4,
               objectives= on and off (off: plain EI on the first objective), both
               under ParetoMinimize: the final hypervolume against the fixed
               reference point (1.1, 11)

A stage time is the median over nine repeats of the library's device-event
difference for that stage (ut_stage_time, timing restarted per call), after
warm-up calls of the same shape."""
import argparse
import json
import math
import os
import subprocess
import sys
import time

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
HYP = dict(sigma_f2=1.0, sigma_n2=1e-6, jitter=1e-8)
ZDT_REF = (1.1, 11.0)


def use_tree(tree):
    sys.path.insert(0, tree)
    sys.path.insert(0, os.path.join(tree, "scripts"))


def front_values(y, P):
    """Y2 that puts exactly the P rows of smallest y on the front"""
    rank = np.empty(len(y), dtype=np.int64)
    rank[np.argsort(y, kind="stable")] = np.arange(len(y))
    return np.where(rank < P, float(P) - rank, float(P) + 1.0 + rank)


def wall_ms(call, repeats, warm=2):
    import torch
    for _ in range(warm):
        call()
    ts = []
    for _ in range(repeats):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        call()
        torch.cuda.synchronize()
        ts.append((time.perf_counter() - t0) * 1e3)
    return float(np.median(ts)), [float(np.min(ts)), float(np.max(ts))]


def tail_step(repeats):
    from cons_bench import cons_values, stage_medians
    from feas_bench import c2_setup
    from uptune_amd.pareto import default_ref
    m = 1 << 20
    e, X, y, ell = c2_setup(m)
    vals = e.population_get()
    e.gp_fit(X, y, lengthscale=ell, **HYP)
    plain, plain_mm = wall_ms(lambda: e.gp_score_values(vals), repeats)
    fronts = []
    for P in (16, 64, 256):
        Y2 = front_values(y, P)
        e.gp_mo_set(Y2, default_ref(np.column_stack([y, Y2])))
        assert e.gp_mo_info()["P"] == P
        st, mm = stage_medians(e, lambda: e.gp_mo_score(values=vals), ["kstar", "var", "mo_means", "mo_ehvi"], repeats)
        whole, whole_mm = wall_ms(lambda: e.gp_mo_score(values=vals), repeats)
        scored, scored_mm = wall_ms(lambda: e.gp_score_values(vals), repeats)
        fronts.append(dict(P=P, mo_means_ms=st["mo_means"], mo_ehvi_ms=st["mo_ehvi"], mo_ehvi_ms_minmax=mm["mo_ehvi"],
                           tail_ms=st["mo_means"] + st["mo_ehvi"], mo_score_ms=whole, mo_score_ms_minmax=whole_mm,
                           score_values_ehvi_ms=scored, score_values_ehvi_ms_minmax=scored_mm,
                           tail_over_plain_ei_score=(st["mo_means"] + st["mo_ehvi"]) / plain,
                           mo_score_over_plain_ei_score=whole / plain))
    e.gp_mo_clear()
    C, thr = cons_values(X, 1)
    e.gp_cons_set(C, thr)
    cs, cmm = stage_medians(e, lambda: e.gp_cons_prob(values=vals), ["cons"], repeats)
    e.gp_cons_clear()
    rec = dict(step="c2_tail", config="c2", m=m, d=int(X.shape[1]), n=int(X.shape[0]), repeats=repeats,
               plain_ei_score_ms=plain, plain_ei_score_ms_minmax=plain_mm, cons_tail_nc1_ms=cs["cons"],
               cons_tail_nc1_ms_minmax=cmm["cons"], fronts=fronts)
    e.close()
    return rec


def front_step(repeats):
    from cons_bench import stage_medians
    from feas_bench import c2_setup
    from uptune_amd.pareto import default_ref
    m = 4096
    out = []
    for n in (1024, 4096):
        e, X, y, ell = c2_setup(m, n=n)
        vals = e.population_get()
        e.gp_fit(X, y, lengthscale=ell, **HYP)
        for name, Y2 in (("every_row", -y), ("generic", np.random.default_rng(9).standard_normal(n) - 0.5 * y / y.std())):
            ref = default_ref(np.column_stack([y, Y2]))

            def call():
                e.gp_mo_set(Y2, ref)          # the operands are rebuilt by the scoring call that follows
                e.gp_mo_score(values=vals)

            st, mm = stage_medians(e, call, ["mo_ops", "mo_front"], repeats)
            out.append(dict(n=n, front=name, P=e.gp_mo_info()["P"], mo_front_ms=st["mo_front"],
                            mo_front_ms_minmax=mm["mo_front"], mo_ops_ms=st["mo_ops"]))
        e.close()
    return dict(step="front", d=64, repeats=repeats, cases=out)


def round_step(repeats):
    """cons_bench.py's C2 round with nothing loaded"""
    import torch
    from feas_bench import c2_setup
    k, m = 256, 1 << 20
    e, X, y, ell = c2_setup(m)
    e.gp_set_precision(8)
    acq = e.acq("ei")
    r = [0]

    def rnd():
        r[0] += 1
        e.gp_fit(X, y, lengthscale=ell, wait=False, **HYP)
        e.score_round_de(m, k, round_=r[0], cr=0.2, n_cross=1, acq=acq, want_values=False)

    med, mm = wall_ms(rnd, repeats, warm=4)
    torch.cuda.synchronize()
    e.close()
    return dict(step="c2_round", m=m, n=1024, k=k, precision=8, repeats=repeats, round_ms=med, round_ms_minmax=mm)


def zdt1(cfg):
    x = [cfg["x%d" % j] for j in range(8)]
    g = 1.0 + 9.0 * sum(x[1:]) / 7.0
    return {"time": x[0], "size": g * (1.0 - math.sqrt(x[0] / g))}


def zdt_step(seed, on):
    from uptune_amd.driver import ParetoMinimize
    from uptune_amd.manipulator import ConfigurationManipulator, FloatParameter
    from uptune_amd.pareto import hypervolume2d
    from uptune_amd.tuner import tune_bandit
    space = ConfigurationManipulator([FloatParameter("x%d" % j, 0.0, 1.0) for j in range(8)])
    kw = dict(objectives=[("time", "min"), ("size", "min")], ref_point=ZDT_REF) if on else {}
    t0 = time.perf_counter()
    d = tune_bandit(space, zdt1, generations=100, parallelism=4, n_init=16, pool=8192, batch=4, population=256,
                    seed=seed, lengthscale=0.5, driver_objective=ParetoMinimize("size"), **kw)
    pts = [(r.time, r.size) for r in d.pareto_front()]
    return dict(step="zdt1", seed=seed, objectives=bool(on), tests=int(d.test_count), results=len(d.results),
                front=len(pts), hypervolume=hypervolume2d(pts, ZDT_REF), seconds=time.perf_counter() - t0)


def child(step, limit, repeats, tree=ROOT):
    cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", step,
           "--repeats", str(repeats), "--tree", tree]
    p = subprocess.run(cmd, capture_output=True, text=True, cwd=tree)
    line = [ln for ln in p.stdout.splitlines() if ln.startswith("MO_REC ")]
    if p.returncode != 0 or not line:
        print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
        print("step %s ended with status %d: stopping here" % (step, p.returncode), file=sys.stderr)
        return None
    rec = json.loads(line[-1][len("MO_REC "):])
    print(json.dumps(rec), flush=True)
    return rec


def spread(v):
    return dict(median=float(np.median(v)), min=float(np.min(v)), max=float(np.max(v)))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "mo.json"))
    ap.add_argument("--repeats", type=int, default=9)
    ap.add_argument("--parent-tree", default=None, help="a built checkout of the parent commit (c2_round on both)")
    ap.add_argument("--only", default=None, help="comma-separated steps (c2_tail, front, c2_round, zdt1)")
    ap.add_argument("--step", default=None, help="(internal) run one step in this process and print its record")
    ap.add_argument("--tree", default=ROOT, help="(internal) the tree the step imports from")
    a = ap.parse_args()
    if a.step:
        use_tree(a.tree)
        import torch
        assert torch.cuda.is_available(), "mo_bench needs a GPU"
        if a.step.startswith("zdt1:"):
            _, seed, on = a.step.split(":")
            rec = zdt_step(int(seed), on == "1")
        else:
            rec = {"c2_tail": tail_step, "front": front_step, "c2_round": round_step}[a.step](a.repeats)
        print("MO_REC " + json.dumps(rec), flush=True)
        return 0
    only = a.only.split(",") if a.only else ["c2_tail", "front", "c2_round", "zdt1"]
    res = dict(what="two-objective scoring: the EHVI tail (k_kstar_sums with alpha_2 + k_mo_ehvi) by device events "
                    "inside ut_gp_mo_score and the call by the host clock, against the constrained tail with one "
                    "constraint and the plain EI score of the same pool; the front kernels; the bench's C2 round with "
                    "nothing loaded on this tree and the parent's; ZDT1 (8 inputs, 400 tests) with objectives= on and off")
    for step, limit in (("c2_tail", 420), ("front", 300)):
        if step in only:
            rec = child(step, limit, a.repeats)
            if rec is None:
                return 1
            res[step] = rec
    if "c2_round" in only:
        runs = {"this": [], "parent": []}
        for _ in range(5):                                  # alternating: the same machine state for both
            for which, tree in (("this", ROOT), ("parent", a.parent_tree)):
                if tree is None:
                    continue
                rec = child("c2_round", 300, a.repeats, tree=os.path.abspath(tree))
                if rec is None:
                    return 1
                runs[which].append(rec["round_ms"])
        res["c2_round_nothing_loaded"] = {k: dict(runs_ms=v, **spread(v)) for k, v in runs.items() if v}
    if "zdt1" in only:
        runs = []
        for seed in range(5):
            for on in (1, 0):
                rec = child("zdt1:%d:%d" % (seed, on), 420, a.repeats)
                if rec is None:
                    return 1
                runs.append(rec)
        res["zdt1"] = dict(reference_point=list(ZDT_REF), runs=runs,
                           hypervolume_on=spread([r["hypervolume"] for r in runs if r["objectives"]]),
                           hypervolume_off=spread([r["hypervolume"] for r in runs if not r["objectives"]]))
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
