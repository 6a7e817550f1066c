"""Wall time of ut_gp_select_batch alone (profiles/batch_select.json).

    python scripts/batch_select_bench.py --out profiles/batch_select.json

Per shape (n training rows, d features, a shortlist of p, k picks) on a fit in
place: the whole call by the host clock around call + device synchronisation
(the call itself never waits: its k + 1 loop launches are issued back to back),
the median of the repeats after two warm-up calls with the spread; then, in a
second set of calls with the library's stage events on, the split into
  kstar  encode + K*^T (the existing fp64 K* kernel over every feature),
  v      V = L^-1 K*^T written out, and the mean V^T beta,
  sigma  Sigma = Kss - V^T V, full symmetric,
  loop   the k + 1 chained pick launches,
as device-event differences on the stream (so the loop's figure includes the
gaps between its launches, which is what it costs).  The FLOP counts are those
the algorithm needs (lower-triangular L^-1: n^2 p; the lower tiles of Sigma
mirrored: n p^2), from the shapes.  The parent's C2 round time from README is
recorded beside them for scale."""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

SHAPES = [dict(n=1024, d=64, p=1024, k=256), dict(n=1024, d=64, p=4096, k=256), dict(n=4096, d=64, p=4096, k=256)]
HYP = dict(sigma_f2=1.0, sigma_n2=1e-2, jitter=1e-8)
STAGES = [("kstar", "bs_kstar"), ("v", "bs_v"), ("sigma", "bs_sigma"), ("loop", "bs_loop")]
C2_ROUND_MS = 16.18   # README: the C2 headline round (2^20 candidates, n = 1024) on the parent commit


def data(n, d):
    rng = np.random.default_rng(n + d)
    X = rng.uniform(size=(n, d))
    return X, np.sum((X - 0.4) ** 2, axis=1) + 0.01 * rng.standard_normal(n)


def run(repeats):
    import torch
    from uptune_amd.engine import BatchEngine
    from uptune_amd.manipulator import ConfigurationManipulator, FloatParameter
    assert torch.cuda.is_available(), "batch_select_bench needs a GPU"
    out = []
    for s in SHAPES:
        n, d, p, k = s["n"], s["d"], s["p"], s["k"]
        X, y = data(n, d)
        e = BatchEngine(ConfigurationManipulator([FloatParameter(f"u{j}", 0.0, 1.0) for j in range(d)]), device=0)
        e.gp_fit(X, y, lengthscale=2.0, **HYP)
        U = torch.from_numpy(np.random.default_rng(7000 + n).uniform(size=(d, p))).to("cuda:0")
        acq = e.acq("ei")

        def once():
            r = e.gp_select_batch(U, k, acq=acq)
            torch.cuda.synchronize()
            return r
        for _ in range(2):
            pos = once()[0]
        ts = []
        for _ in range(repeats):
            t0 = time.perf_counter()
            once()
            ts.append((time.perf_counter() - t0) * 1e3)
        e.set_timing(True)
        for _ in range(repeats):
            once()
        stages = {name: e.stage_time(key) for name, key in STAGES}
        e.set_timing(False)
        gf_v, gf_s = 1e-9 * n * n * p, 1e-9 * n * p * p
        rec = dict(s, median_ms=float(np.median(ts)), min_ms=float(np.min(ts)), max_ms=float(np.max(ts)),
                   repeats=repeats, stage_ms=stages, stage_sum_ms=float(sum(stages.values())),
                   loop_us_per_launch=1e3 * stages["loop"] / (k + 1), gflop_v=gf_v, gflop_sigma=gf_s,
                   tflops_v=gf_v / stages["v"], tflops_sigma=gf_s / stages["sigma"],
                   picks=int((pos >= 0).sum().item()), distinct=int(torch.unique(pos).numel()))
        out.append(rec)
        print(json.dumps(rec), flush=True)
        e.close()
    return dict(what="ut_gp_select_batch alone on a fit in place: host clock around call + synchronise (median of "
                     "the repeats), and its stages by device events",
                c2_round_ms_parent=C2_ROUND_MS, shapes=out)


if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join("profiles", "batch_select.json"))
    ap.add_argument("--repeats", type=int, default=10)
    a = ap.parse_args()
    res = run(a.repeats)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(res, f, indent=1)
        f.write("\n")
