"""Device time of the feasibility vote (profiles/feas.json).

    python scripts/feas_bench.py --out profiles/feas.json

Every step runs in a child process of its own under `timeout`, in a fixed
order, and the first one that fails ends the script (nothing more is started
on the device after a fault or a hang).  The steps:

  c2_prob_nf128, c2_prob_nf1024   ut_gp_feas_prob alone at the C2 shape (m = 2^20
                                   candidates, d = 64, n = 1024, the bench's data
                                   and lengthscale) with 128 and 1,024 failed rows
  c4_prob                          ... at the C4 shape: the gcc space (707 features,
                                   552 of them one-hot: the int8 code product), the
                                   first 1,024 successful recorded runs, the 117
                                   failed ones among the first 3,000, m = 2^22 GA children
  c2_round, c4_round               the bench's DE / GA round (precision 8, an
                                   asynchronous refit per round) with and without
                                   the rows loaded, alternating, by the host clock
                                   around round + synchronise; and its stages
                                   `kstar` and `feas` by device events

A stage time is the mean of the library's device-event differences over the
repeats (ut_stage_time), after warm-up calls of the same shape.  The vote
contracts n + n_f rows where K* contracts n, so `ms_per_1024_rows` is the
figure to hold against K* alone at the same shape (fp64, stage `kstar` of
ut_gp_score, measured here in the same process: `kstar_f64_ms`)."""
import argparse
import json
import os
import subprocess
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

STEPS = [("c2_prob_nf128", 240), ("c2_prob_nf1024", 240), ("c4_prob", 300), ("c2_round", 300), ("c4_round", 420)]
HYP = dict(sigma_f2=1.0, sigma_n2=1e-6, jitter=1e-8)


def c2_setup(m, n=1024, d=64):
    import torch
    from uptune_amd.engine import BatchEngine
    from uptune_amd.manipulator import ConfigurationManipulator, FloatParameter
    e = BatchEngine(ConfigurationManipulator([FloatParameter(i, -1000.0, 1000.0) for i in range(d)]), device=0, seed=1)
    rng = np.random.default_rng(101)
    X = rng.uniform(size=(n, d))
    y = np.sum(100.0 * (X[:, 1:] - X[:, :-1] ** 2) ** 2 + (1.0 - X[:, :-1]) ** 2, axis=1)
    e.population_init(m)
    e.history_reset(4 * (n + 64 * 256))
    e.history_add(e.hash(torch.from_numpy(np.ascontiguousarray((X * 2000.0 - 1000.0).T)).to(e.device)))
    return e, X, y, 0.2


def c4_setup():
    import torch
    from uptune_amd import spaces
    from uptune_amd.engine import BatchEngine
    e = BatchEngine(spaces.gcc(), device=0, seed=1)
    z = np.load(os.path.join(ROOT, "tests", "golden", "gcc_history.npz"))
    hist, qor = z["values"], z["qor"]
    hv = torch.from_numpy(np.ascontiguousarray(hist)).to(e.device)
    e.history_reset(4 * (3680 + 64 * 256))
    e.history_add(e.hash(hv))
    fin = np.isfinite(qor)
    ok = np.flatnonzero(fin)[:1024]
    bad = np.flatnonzero(~fin[:3000])
    feat = lambda rows: e.encode(hv[:, torch.from_numpy(rows).to(e.device)].contiguous()).T.contiguous().cpu().numpy()  # noqa: E731
    return e, feat(ok), qor[ok].astype(np.float64), 2.0, feat(bad), hist[:, int(np.argmin(qor))].copy()


def stage_means(e, call, stages, repeats, warm=2):
    import torch
    for _ in range(warm):
        call()
    torch.cuda.synchronize()
    e.set_timing(True)
    for _ in range(repeats):
        call()
    torch.cuda.synchronize()
    out = {}
    for s in stages:
        try:
            out[s] = e.stage_time(s)
        except Exception:   # the stage did not run (nothing loaded: no `feas`)
            out[s] = 0.0
    e.set_timing(False)
    return out


def prob_step(name, repeats):
    import torch
    if name == "c4_prob":
        e, X, y, ell, F, parent = c4_setup()
        m = 1 << 22
        vals = e.propose_ga(m, parent, None, round_=1, mutation_rate=0.1)[0]
        shape = dict(config="c4", m=m, d=int(X.shape[1]), n=1024, nf=int(F.shape[0]))
    else:
        nf = int(name.rsplit("nf", 1)[1])
        m = 1 << 20
        e, X, y, ell = c2_setup(m)
        F = np.random.default_rng(7).uniform(size=(nf, X.shape[1]))
        vals = e.population_get()
        shape = dict(config="c2", m=m, d=int(X.shape[1]), n=1024, nf=nf)
    e.gp_fit(X, y, lengthscale=ell, **HYP)
    e.gp_feas_set(F)
    st = stage_means(e, lambda: e.gp_feas_prob(values=vals), ["encode", "feas"], repeats)
    # the yardstick in the same process: fp64 K* alone (ut_gp_score's stage kstar)
    feat = e.encode(vals) if name != "c4_prob" else None
    ks = None
    if feat is not None:
        e.gp_feas_clear()
        ks = stage_means(e, lambda: e.gp_score(feat), ["kstar"], repeats)["kstar"]
    rows = shape["n"] + shape["nf"]
    rec = dict(shape, step=name, kstar_mode=e.gp_kstar_mode(), repeats=repeats, feas_ms=st["feas"],
               encode_ms=st["encode"], ms_per_1024_rows=st["feas"] * 1024.0 / rows, kstar_f64_ms=ks,
               gflop_dense=2e-9 * rows * shape["d"] * shape["m"])   # 2 (n + nf) d m: what the dense contraction needs
    torch.cuda.synchronize()
    e.close()
    return rec


def round_step(name, repeats):
    import torch
    k = 256
    if name == "c4_round":
        e, X, y, ell, F, parent = c4_setup()
        m = 1 << 22
    else:
        m = 1 << 20
        e, X, y, ell = c2_setup(m)
        F = np.random.default_rng(7).uniform(size=(128, X.shape[1]))
    e.gp_set_precision(8)
    acq = e.acq("ei")
    r = [0]

    def rnd():
        r[0] += 1
        e.gp_fit(X, y, lengthscale=ell, wait=False, **HYP)
        if name == "c4_round":
            e.score_round_ga(m, k, parent1=parent, round_=r[0], mutation_rate=0.1, acq=acq, want_values=False)
        else:
            e.score_round_de(m, k, round_=r[0], cr=0.2, n_cross=1, acq=acq, want_values=False)

    def wall(loaded):
        e.gp_feas_set(F) if loaded else e.gp_feas_clear()
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        rnd()
        torch.cuda.synchronize()
        return (time.perf_counter() - t0) * 1e3

    for loaded in (False, True, False, True):    # warm-up of both forms
        wall(loaded)
    ts = {False: [], True: []}
    for _ in range(repeats):                      # alternating: the same machine state for both
        for loaded in (False, True):
            ts[loaded].append(wall(loaded))
    e.gp_feas_set(F)
    st = stage_means(e, rnd, ["kstar", "var", "feas"], repeats, warm=1)
    rec = dict(step=name, m=m, n=1024, nf=int(F.shape[0]), k=k, precision=8, repeats=repeats,
               round_ms=float(np.median(ts[False])), round_loaded_ms=float(np.median(ts[True])),
               round_ms_minmax=[float(np.min(ts[False])), float(np.max(ts[False]))],
               round_loaded_ms_minmax=[float(np.min(ts[True])), float(np.max(ts[True]))],
               stage_ms=st, kstar_mode=e.gp_kstar_mode())
    e.close()
    return rec


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "feas.json"))
    ap.add_argument("--repeats", type=int, default=10)
    ap.add_argument("--step", default=None, help="(internal) run one step in this process and print its record")
    a = ap.parse_args()
    if a.step:
        import torch
        assert torch.cuda.is_available(), "feas_bench needs a GPU"
        rec = (round_step if a.step.endswith("_round") else prob_step)(a.step, a.repeats)
        print("FEAS_REC " + json.dumps(rec), flush=True)
        return 0
    recs = []
    for name, limit in STEPS:
        cmd = ["timeout", "-k", "10", str(limit), sys.executable, os.path.abspath(__file__), "--step", name,
               "--repeats", str(a.repeats)]
        p = subprocess.run(cmd, capture_output=True, text=True, cwd=ROOT)
        line = [ln for ln in p.stdout.splitlines() if ln.startswith("FEAS_REC ")]
        if p.returncode != 0 or not line:
            print(p.stdout[-2000:], p.stderr[-4000:], file=sys.stderr)
            print("step %s ended with status %d: stopping here" % (name, p.returncode), file=sys.stderr)
            return 1
        recs.append(json.loads(line[-1][len("FEAS_REC "):]))
        print(json.dumps(recs[-1]), flush=True)
    res = dict(what="the feasibility vote (k_kstar_sums + k_feas_apply, stage `feas`) by device events: alone "
                    "(ut_gp_feas_prob) and inside the bench's rounds; rounds by the host clock around round + "
                    "synchronise, alternating loaded / not loaded (medians)",
               steps=recs)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
