"""Weighted pruning at the C3 shape (profiles/prune_weight.json).

    python scripts/prune_weight_bench.py --out profiles/prune_weight.json [--parent DIR]

The workload is the bench's C3 pruned round: HPL-64, m = 2^21 candidates,
n = 4096 training rows, k = 256, bound_rows = 256, an asynchronous refit per
round, the selections appended to the history.  Every step runs in a child
process of its own under `timeout`, in a fixed order, and the first one that
fails ends the script (nothing more is started on the device after a fault or
a hang).  The steps, at bound passes 32 and 64:

  plain_pNN_rK        the pruned round with nothing loaded, run K of --runs, on this
  parent_pNN_rK       tree and (--parent DIR: a built checkout of the parent commit)
                      on the parent, alternating; ms per round = the median over the
                      run's rounds of the host clock around round + synchronise.  The
                      regression check: this tree's runs inside the parent's spread
  cons_pNN_qQ         one constraint c = x . w + 0.05 N <= its Q-quantile over the
                      training rows (Q = 0.5, 0.05), reloaded after every fit: the
                      weighted pruned round, its stage `cons` (k_kstar_sums over every
                      candidate), survivors and dense flag; the survivors of the same
                      round with the constraint-weight bound switched off
                      (UT_PRUNE_WEIGHT_BOUND=0: the EI bound at f_best_c alone, for
                      this comparison only); and the dense constrained fp64 round
                      (ut_score_round_de) in the same process
"""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HYP = dict(sigma_f2=1.0, sigma_n2=1e-6)
M, N, K, ROWS, ELL = 1 << 21, 4096, 256, 256, 1.0


def c3_setup(rounds):
    from uptune_amd import spaces
    from uptune_amd.engine import BatchEngine
    manip = spaces.hpl64()
    e = BatchEngine(manip, device=0, seed=1)
    e.gp_set_precision(64)
    e.population_init(M)
    e.history_reset(4 * (N + 3680 + (rounds + 8) * 4 * K))
    tr = BatchEngine(manip, device=0, seed=101)
    tr.population_init(N)
    tv = tr.population_get()
    X = tr.encode(tv).T.contiguous().cpu().numpy()
    e.history_add(e.hash(tv))
    y = np.sum((X - 0.3) ** 2, axis=1)
    tr.close()
    return e, X, y


def walls(fn, rounds, warm=2):
    import torch
    for _ in range(warm):
        fn()
    out = []
    for _ in range(rounds):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def plain_step(name, prune_pass, rounds):
    e, X, y = c3_setup(rounds)
    e.gp_set_prune_pass(prune_pass)
    acq = e.acq("ei")
    r, stats = [0], []

    def rnd():
        r[0] += 1
        e.gp_fit(X, y, lengthscale=ELL, wait=False, **HYP)
        idx, top, dig, _, st = e.score_round_de_pruned(M, K, round_=r[0], cr=0.2, n_cross=1, acq=acq,
                                                       want_values=False, bound_rows=ROWS)
        e.history_add(dig)
        stats.append(st)

    ts = walls(rnd, rounds)
    rec = dict(step=name, prune_pass=prune_pass, rounds=rounds, round_ms=float(np.median(ts)),
               round_ms_minmax=[float(np.min(ts)), float(np.max(ts))],
               survivors=int(np.median([s["survivors"] for s in stats])), dense=int(sum(s["dense"] for s in stats)))
    e.close()
    return rec


def cons_step(name, prune_pass, q, rounds):
    import torch
    e, X, y = c3_setup(3 * rounds)
    e.gp_set_prune_pass(prune_pass)
    e.gp_set_prune_weighted(True)
    acq = e.acq("ei")
    w = np.random.default_rng(5).standard_normal(X.shape[1]) / np.sqrt(X.shape[1])
    C = (X @ w + 0.05 * np.random.default_rng(6).standard_normal(N)).reshape(N, 1)
    thr = [float(np.quantile(C, q))]
    r, stats = [0], []

    def rnd(pruned=True, keep=True):
        r[0] += 1
        e.gp_fit(X, y, lengthscale=ELL, wait=False, **HYP)
        e.gp_cons_set(C, thr)
        if pruned:
            out = e.score_round_de_pruned(M, K, round_=r[0], cr=0.2, n_cross=1, acq=acq, want_values=False,
                                          bound_rows=ROWS)
            if keep:
                stats.append(out[4])
        else:
            out = e.score_round_de(M, K, round_=r[0], cr=0.2, n_cross=1, acq=acq, want_values=False)
        e.history_add(out[2])
        return out

    ts = walls(rnd, rounds)
    n_feasible = e.gp_cons_info()["n_feasible"]
    e.set_timing(True)
    stage = []
    for _ in range(5):
        rnd(keep=False)
        torch.cuda.synchronize()
        stage.append(e.stage_time("cons"))
    e.set_timing(False)
    # the same rounds with the constraint-weight bound off: what the EI bound alone keeps
    os.environ["UT_PRUNE_WEIGHT_BOUND"] = "0"
    ei_only = [rnd(keep=False)[4] for _ in range(3)]
    del os.environ["UT_PRUNE_WEIGHT_BOUND"]
    td = walls(lambda: rnd(pruned=False), max(3, rounds // 2), warm=1)
    rec = dict(step=name, prune_pass=prune_pass, quantile=q, n_feasible=int(n_feasible), rounds=rounds,
               round_ms=float(np.median(ts)), round_ms_minmax=[float(np.min(ts)), float(np.max(ts))],
               cons_means_ms=float(np.median(stage)),
               survivors=int(np.median([s["survivors"] for s in stats])), dense=int(sum(s["dense"] for s in stats)),
               ei_only_survivors=int(np.median([s["survivors"] for s in ei_only])),
               ei_only_dense=int(sum(s["dense"] for s in ei_only)),
               dense_round_ms=float(np.median(td)), dense_round_ms_minmax=[float(np.min(td)), float(np.max(td))])
    e.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "prune_weight.json"))
    ap.add_argument("--runs", type=int, default=5, help="runs (processes) of the regression check per tree and pass")
    ap.add_argument("--rounds", type=int, default=10, help="timed rounds per run")
    ap.add_argument("--parent", default=None, help="a built checkout of the parent commit (regression check)")
    ap.add_argument("--skip-cons", action="store_true")
    ap.add_argument("--step", default=None, help="(internal) run one step in this process and print its record")
    ap.add_argument("--tree", default=ROOT, help="(internal) the checkout whose uptune_amd the step imports")
    a = ap.parse_args()
    if a.step:
        sys.path.insert(0, os.path.abspath(a.tree))
        import torch
        assert torch.cuda.is_available(), "prune_weight_bench needs a GPU"
        kind, pp = a.step.split("_")[0], int(a.step.split("_p")[1].split("_")[0])
        if kind == "cons":
            rec = cons_step(a.step, pp, float(a.step.rsplit("_q", 1)[1]), a.rounds)
        else:
            rec = plain_step(a.step, pp, a.rounds)
        print("PW_REC " + json.dumps(rec), flush=True)
        return 0
    if a.parent:
        a.parent = os.path.abspath(a.parent)
    steps = []
    for pp in (32, 64):
        for run in range(a.runs):
            steps.append(("plain_p%d_r%d" % (pp, run), ROOT, 240))
            if a.parent:
                steps.append(("parent_p%d_r%d" % (pp, run), a.parent, 240))
    if not a.skip_cons:
        steps += [("cons_p%d_q%s" % (pp, q), ROOT, 300) for pp in (32, 64) for q in ("0.5", "0.05")]
    recs = []
    for name, tree, limit in steps:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name,
               "--rounds", str(a.rounds), "--tree", tree]
        p = subprocess.run(cmd, capture_output=True, text=True, cwd=tree)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("PW_REC ")]
        if p.returncode != 0 or not line:
            print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
            print("step %s ended with status %d: stopping here" % (name, p.returncode), file=sys.stderr)
            return 1
        recs.append(json.loads(line[-1][len("PW_REC "):]))
        print(json.dumps(recs[-1]), flush=True)
    reg = {}
    for pp in (32, 64):
        new = [r["round_ms"] for r in recs if r["step"].startswith("plain_p%d_" % pp)]
        old = [r["round_ms"] for r in recs if r["step"].startswith("parent_p%d_" % pp)]
        reg["pass%d" % pp] = dict(this_ms=new, parent_ms=old,
                                  this_minmax=[min(new), max(new)] if new else None,
                                  parent_minmax=[min(old), max(old)] if old else None,
                                  inside_parent_spread=bool(old and min(old) <= float(np.median(new)) <= max(old)))
    res = dict(what="the bench's C3 pruned round (HPL-64, m = 2^21, n = 4096, k = 256, bound_rows = 256) by the host "
                    "clock around round + synchronise: with nothing loaded on this tree and on the parent commit "
                    "(one process per run, alternating), and with one constraint loaded under "
                    "ut_gp_set_prune_weighted (stage `cons` = k_kstar_sums over every candidate, by device events), "
                    "against the dense constrained fp64 round in the same process",
               regression=reg, steps=recs)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
