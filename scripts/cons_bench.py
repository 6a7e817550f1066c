"""Device time of constrained EI's tail (profiles/cons.json).

    python scripts/cons_bench.py --out profiles/cons.json

Every step runs in a child process of its own under `timeout`, in a fixed
order, and the first one that fails ends the script (nothing more is started
on the device after a fault or a hang).  The steps:

  c2_n1024_nc1, c2_n1024_nc4   stage `cons` (k_kstar_sums + k_cons_apply) of
  c2_n4096_nc1, c2_n4096_nc4   ut_gp_cons_prob at the C2 shape (m = 2^20 candidates,
                               d = 64, the bench's data and lengthscale) with 1,024
                               and 4,096 training rows; and, in the same process, the
                               yardstick: stage `feas` of ut_gp_feas_prob with ONE
                               failed row loaded -- the same kernel without weights,
                               over the same training row tiles
                               plus one tile of 128
  c2_round                     the bench's DE round (precision 8, an asynchronous
                               refit per round, no history growth) with and without
                               one constraint loaded (reloaded after every fit, so
                               its per-fit operands are rebuilt every round),
                               alternating, by the host clock around round +
                               synchronise; and its stages by device events

A stage time is the median over the repeats of the library's device-event
difference for that stage (ut_stage_time, timing restarted per call), after
warm-up calls of the same shape."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "scripts"))

STEPS = [("c2_n1024_nc1", 240), ("c2_n1024_nc4", 240), ("c2_n4096_nc1", 300), ("c2_n4096_nc4", 300), ("c2_round", 300)]
HYP = dict(sigma_f2=1.0, sigma_n2=1e-6, jitter=1e-8)


def stage_medians(e, call, stages, repeats, warm=2):
    import torch
    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    samples = {s: [] for s in stages}
    for _ in range(repeats):
        e.set_timing(True)
        call()
        torch.cuda.synchronize()
        for s in stages:
            try:
                samples[s].append(e.stage_time(s))
            except Exception:   # the stage did not run
                samples[s].append(0.0)
    e.set_timing(False)
    return {s: float(np.median(v)) for s, v in samples.items()}, {s: [float(np.min(v)), float(np.max(v))]
                                                                   for s, v in samples.items()}


def cons_values(X, nc):
    W = np.random.default_rng(5).standard_normal((X.shape[1], nc)) / np.sqrt(X.shape[1])
    C = np.sin(3.0 * X @ W) + 0.1 * np.random.default_rng(6).standard_normal((X.shape[0], nc))
    return C, np.median(C, axis=0)


def prob_step(name, repeats):
    import torch
    from feas_bench import c2_setup
    n, nc = int(name.split("_n")[1].split("_")[0]), int(name.rsplit("nc", 1)[1])
    m = 1 << 20
    e, X, y, ell = c2_setup(m, n=n)
    vals = e.population_get()
    e.gp_fit(X, y, lengthscale=ell, **HYP)
    C, thr = cons_values(X, nc)
    e.gp_cons_set(C, thr)
    st, mm = stage_medians(e, lambda: e.gp_cons_prob(values=vals), ["kstar", "var", "cons"], repeats)
    e.gp_cons_clear()
    e.gp_feas_set(np.random.default_rng(7).uniform(size=(1, X.shape[1])))
    vote, vmm = stage_medians(e, lambda: e.gp_feas_prob(values=vals), ["feas"], repeats)
    tiles = n // 128
    rec = dict(step=name, config="c2", m=m, d=int(X.shape[1]), n=n, nc=nc, repeats=repeats, cons_ms=st["cons"],
               cons_ms_minmax=mm["cons"], kstar_f64_ms=st["kstar"], var_f64_ms=st["var"], vote_ms=vote["feas"],
               vote_ms_minmax=vmm["feas"], vote_row_tiles=tiles + 1, cons_row_tiles=tiles,
               ratio_per_row_tile=(st["cons"] / tiles) / (vote["feas"] / (tiles + 1)),
               cons_ms_per_1024_rows=st["cons"] * 1024.0 / n)
    torch.cuda.synchronize()
    e.close()
    return rec


def round_step(name, repeats):
    import torch
    from feas_bench import c2_setup
    k, m = 256, 1 << 20
    e, X, y, ell = c2_setup(m)
    C, thr = cons_values(X, 1)
    e.gp_set_precision(8)
    acq = e.acq("ei")
    r = [0]

    def rnd(loaded):
        r[0] += 1
        e.gp_fit(X, y, lengthscale=ell, wait=False, **HYP)
        if loaded:
            e.gp_cons_set(C, thr)
        e.score_round_de(m, k, round_=r[0], cr=0.2, n_cross=1, acq=acq, want_values=False)

    def wall(loaded):
        if not loaded:
            e.gp_cons_clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rnd(loaded)
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for loaded in (False, True, False, True):    # warm-up of both forms
        wall(loaded)
    ts = {False: [], True: []}
    for _ in range(repeats):                      # alternating: the same machine state for both
        for loaded in (False, True):
            ts[loaded].append(wall(loaded))
    st, _ = stage_medians(e, lambda: rnd(True), ["kstar", "var", "cons"], repeats, warm=1)
    rec = dict(step=name, m=m, n=1024, nc=1, k=k, precision=8, repeats=repeats,
               round_ms=float(np.median(ts[False])), round_loaded_ms=float(np.median(ts[True])),
               round_ms_minmax=[float(np.min(ts[False])), float(np.max(ts[False]))],
               round_loaded_ms_minmax=[float(np.min(ts[True])), float(np.max(ts[True]))], stage_ms=st)
    e.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "cons.json"))
    ap.add_argument("--repeats", type=int, default=20)
    ap.add_argument("--step", default=None, help="(internal) run one step in this process and print its record")
    a = ap.parse_args()
    if a.step:
        import torch
        assert torch.cuda.is_available(), "cons_bench needs a GPU"
        rec = (round_step if a.step.endswith("_round") else prob_step)(a.step, a.repeats)
        print("CONS_REC " + json.dumps(rec), flush=True)
        return 0
    recs = []
    for name, limit in STEPS:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name,
               "--repeats", str(a.repeats)]
        p = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("CONS_REC ")]
        if p.returncode != 0 or not line:
            print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
            print("step %s ended with status %d: stopping here" % (name, p.returncode), file=sys.stderr)
            return 1
        recs.append(json.loads(line[-1][len("CONS_REC "):]))
        print(json.dumps(recs[-1]), flush=True)
    res = dict(what="constrained EI's tail (k_kstar_sums + k_cons_apply, stage `cons`) by device events inside "
                    "ut_gp_cons_prob, against the feasibility vote with one failed row (the same kernel over the same "
                    "training row tiles + 1) in the same process; the bench's C2 round by the host clock around "
                    "round + synchronise, alternating one constraint loaded / nothing loaded (medians)",
               steps=recs)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
