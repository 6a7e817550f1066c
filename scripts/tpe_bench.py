"""The TPE surrogate (csrc/tpe.hip) timed: the fit, the scoring kernel at both
precisions, the same formula composed from torch ops on the same device, and
the GP's EI score of the same pool for context (profiles/tpe.json).

    python scripts/tpe_bench.py --out profiles/tpe.json

  c2   2^20 candidates x 64 numeric features, 1,024 results (the bench's shape).
  gcc  the gcc flag space (tests/golden/gcc_rows.npz, mostly one-hot): its first
       300 rows as results, the fixture's rows tiled to 2^16 candidates.

Nine repeats in one process; inside a repeat the variants alternate, after a
warm-up of each; the host clock around a call that ends in a device
synchronise; median, min and max.  The torch composition is chunked over
candidates (f32, the f32 tier's formula: exp2(A (x - mu)^2 + B) summed per set,
log of the two sums) and is checked against the kernel's score before it is
timed.

  exp2    the bare issue rate of the hardware exp2: a stand-alone kernel (its
          source below, compiled when the script starts and launched in this
          process) in which every lane runs 16 independent chains v = exp2(-v)
          and nothing else; 2,048 workgroups x 256 lanes x 4,096 steps, nine
          repeats after a warm-up.  The f32 kernel's time at each shape is then
          given as a multiple of m * d_num * (n + 2) exp2 at that rate.
  search  tune_bandit on spaces.r64() with the 64-D Rosenbrock objective, 100
          generations x 4 = 400 tests, seeds 0..4: surrogate="tpe" against the
          GP default (lengthscale="auto", tr_bench's setting); best objective
          per run, median and range.

Fails without a GPU."""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

REPEATS = 9

EXP2_SRC = r"""
#include <hip/hip_runtime.h>
constexpr int CHAINS = 16;
__global__ __launch_bounds__(256) void k_exp2_issue(int steps, float* out) {
  float v[CHAINS];
#pragma unroll
  for (int c = 0; c < CHAINS; ++c) v[c] = 1.0f + 0.01f * (float)((threadIdx.x + c) & 15);
  for (int s = 0; s < steps; ++s) {
#pragma unroll
    for (int c = 0; c < CHAINS; ++c) v[c] = __builtin_amdgcn_exp2f(-v[c]);   // stays in (0.4, 1)
  }
  float sum = 0.0f;
#pragma unroll
  for (int c = 0; c < CHAINS; ++c) sum += v[c];
  out[(size_t)blockIdx.x * 256 + threadIdx.x] = sum;
}
extern "C" int exp2_issue(int blocks, int steps, float* out) {
  hipLaunchKernelGGL(k_exp2_issue, dim3(blocks), dim3(256), 0, 0, steps, out);
  return (int)hipGetLastError();
}
"""
EXP2_BLOCKS, EXP2_STEPS, EXP2_CHAINS = 2048, 4096, 16


def exp2_rate():
    """exp2 per second of the bare loop: median, min, max over the repeats"""
    import ctypes
    import subprocess
    import tempfile
    import torch
    with tempfile.TemporaryDirectory() as tmp:
        src, lib = os.path.join(tmp, "exp2_issue.hip"), os.path.join(tmp, "libexp2_issue.so")
        with open(src, "w") as fh:
            fh.write(EXP2_SRC)
        subprocess.check_call([os.environ.get("HIPCC", "/opt/rocm/bin/hipcc"), "-O3", "-shared", "-fPIC",
                               "--offload-arch=" + os.environ.get("UT_OFFLOAD_ARCH", "gfx950"), "-Xclang",
                               "-target-feature", "-Xclang", "-packed-fp32-ops", src, "-o", lib])
        fn = ctypes.CDLL(lib).exp2_issue
        fn.argtypes = [ctypes.c_int, ctypes.c_int, ctypes.c_void_p]
        out = torch.zeros(EXP2_BLOCKS * 256, dtype=torch.float32, device="cuda")

        def call():
            assert fn(EXP2_BLOCKS, EXP2_STEPS, out.data_ptr()) == 0

        ms = [_timed(call, torch.cuda.synchronize) for _ in range(REPEATS + 1)][1:]
        assert bool(((out > 6.0) & (out < 16.0)).all())   # 16 chains, each in (0.4, 1)
    n = EXP2_BLOCKS * 256 * EXP2_STEPS * EXP2_CHAINS
    return dict(exp2_per_launch=n, **_stats(ms), per_s_median=n / (float(np.median(ms)) * 1e-3),
                per_s_best=n / (float(np.min(ms)) * 1e-3))


def _rosen64(cfg):
    x = np.array([cfg[i] for i in range(64)])
    return float(np.sum(100.0 * (x[1:] - x[:-1] ** 2) ** 2 + (x[:-1] - 1.0) ** 2))


def search(seeds=(0, 1, 2, 3, 4), generations=100):
    from uptune_amd import spaces
    from uptune_amd.tuner import tune_bandit
    out = {"what": "tune_bandit on spaces.r64(), 64-D Rosenbrock, %d generations x 4 tests: the best objective"
                   % generations, "runs": []}
    for name, kw in (("gp", dict(lengthscale="auto")), ("tpe", dict(surrogate="tpe"))):
        for seed in seeds:
            t0 = time.perf_counter()
            d = tune_bandit(spaces.r64(), _rosen64, generations=generations, seed=seed, **kw)
            model = d.root_technique.techniques[0].model
            rec = dict(surrogate=name, seed=seed, best=float(d.best_result.time), tests=int(d.test_count),
                       fits=int(model.fits), wall_s=time.perf_counter() - t0)
            out["runs"].append(rec)
            print(json.dumps(rec), flush=True)
        best = [r["best"] for r in out["runs"] if r["surrogate"] == name]
        out[name] = dict(median=float(np.median(best)), min=float(np.min(best)), max=float(np.max(best)))
    return out


def _timed(fn, sync):
    sync()
    t0 = time.perf_counter()
    fn()
    sync()
    return (time.perf_counter() - t0) * 1e3


def _stats(v):
    return dict(median_ms=float(np.median(v)), min_ms=float(np.min(v)), max_ms=float(np.max(v)))


def torch_tables(fit, d, device):
    """the oracle's components as f32 tensors per numeric column, and the categorical weights"""
    import torch
    import _tpe_oracle as TO
    num, cat = [], torch.zeros(d, dtype=torch.float64, device=device)
    bias = 0.0
    for j in range(d):
        if j in fit.num:
            rec = []
            for mu, sig, w, Z in fit.num[j]:
                A = -1.4426950408889634 / (2.0 * sig * sig)
                B = np.log2((w / (sig.astype(TO.LD) * np.sqrt(2 * TO.LD(np.pi)) * Z)).astype(np.float64))
                rec.append([torch.tensor(a, dtype=torch.float32, device=device) for a in (mu, A, B)])
            num.append((j, rec))
        elif fit.kinds[j] == 1:
            l, g = fit.cat[j]
            bias += float(l[0] - g[0])
            cat[j] = float((l[1] - g[1]) - (l[0] - g[0]))
        elif fit.kinds[j] >= 2:
            l, g = fit.cat[j]
            cat[j:j + fit.kinds[j]] = torch.tensor((l - g).astype(np.float64), device=device)
    return num, cat, bias


def torch_score(feat, tables, chunk=16384):
    import torch
    num, cat, bias = tables
    m = feat.shape[1]
    out = torch.empty(m, dtype=torch.float64, device=feat.device)
    for c0 in range(0, m, chunk):
        f = feat[:, c0:c0 + chunk]
        acc = (cat[:, None] * f).sum(dim=0) + bias
        for j, rec in num:
            x = f[j].to(torch.float32)[:, None]
            sums = [torch.exp2(A * (x - mu) ** 2 + B).sum(dim=1) for mu, A, B in rec]
            acc += torch.log(sums[0].double()) - torch.log(sums[1].double())
        out[c0:c0 + chunk] = acc
    return out


def shape(name, e, X, y, feat, kinds, out):
    import torch
    import _tpe_oracle as TO
    sync = torch.cuda.synchronize
    fit = TO.Fit(X, y, kinds)
    tables = torch_tables(fit, X.shape[1], feat.device)
    e.tpe_fit(X, y, kinds=kinds, precision=32)
    got = e.tpe_score(feat)
    ref = torch_score(feat, tables)
    gap = float((got - ref).abs().max())
    assert gap < 1e-2, gap
    if kinds is None:   # the EI score of the same pool, for context (the numeric shape only)
        e.gp_fit(X, y, lengthscale=0.3 * np.sqrt(X.shape[1]))
    runs = {"fit": lambda: e.tpe_fit(X, y, kinds=kinds, precision=32), "torch_f32": lambda: torch_score(feat, tables),
            "gp_ei_score": lambda: e.gp_score(feat)}
    order = ("fit", "score_f32", "score_f64", "torch_f32") + (("gp_ei_score",) if kinds is None else ())
    t = {k: [] for k in order}
    for rep in range(REPEATS + 1):   # the first pass warms every variant up
        for k in order:
            if k.startswith("score"):
                e.tpe_fit(X, y, kinds=kinds, precision=int(k[-2:]))
                ms = _timed(lambda: e.tpe_score(feat), sync)
            else:
                ms = _timed(runs[k], sync)
            if rep:
                t[k].append(ms)
    terms = feat.shape[1] * len(fit.num) * (len(y) + 2)
    out[name] = dict(m=int(feat.shape[1]), d=int(X.shape[1]), d_num=len(fit.num), n=int(len(y)), exp2_terms=int(terms),
                     torch_vs_kernel_max_abs=gap, **{k: _stats(v) for k, v in t.items()})
    out[name]["f32_exp2_per_s"] = terms / (out[name]["score_f32"]["median_ms"] * 1e-3) if terms else None
    print(name, json.dumps(out[name]), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tpe.json"))
    a = ap.parse_args()
    import torch
    assert torch.cuda.is_available(), "tpe_bench needs a GPU"
    from uptune_amd import spaces
    from uptune_amd.engine import BatchEngine
    out = {"repeats": REPEATS, "device": torch.cuda.get_device_name(0)}

    e = BatchEngine(spaces.r64(), device=0, seed=1)
    rng = np.random.default_rng(101)
    X = rng.uniform(size=(1024, 64))
    y = np.sum(100.0 * (X[:, 1:] - X[:, :-1] ** 2) ** 2 + (1.0 - X[:, :-1]) ** 2, axis=1)
    feat = torch.rand(64, 1 << 20, dtype=torch.float64, device="cuda",
                      generator=torch.Generator("cuda").manual_seed(3))
    shape("c2", e, X, y, feat, None, out)
    e.close()

    e = BatchEngine(spaces.gcc(), device=0, seed=1)
    rows = np.load(os.path.join(ROOT, "tests", "golden", "gcc_rows.npz"))["values"]
    f = e.encode(torch.from_numpy(np.ascontiguousarray(rows)).cuda())
    X = f[:, :300].T.contiguous().cpu().numpy()
    y = np.random.default_rng(300).normal(size=300) + X[:, 0]
    feat = f[:, torch.arange(1 << 16, device="cuda") % f.shape[1]].contiguous()
    shape("gcc", e, X, y, feat, e.tpe_kinds(), out)
    e.close()

    out["exp2_issue"] = exp2_rate()
    for name in ("c2", "gcc"):
        bare_ms = out[name]["exp2_terms"] / out["exp2_issue"]["per_s_median"] * 1e3
        out[name]["bare_exp2_ms"] = bare_ms
        out[name]["f32_time_over_bare_exp2"] = out[name]["score_f32"]["median_ms"] / bare_ms
    print("exp2", json.dumps(out["exp2_issue"]), flush=True)
    out["search"] = search()
    with open(a.out, "w") as fh:
        json.dump(out, fh, indent=1)
        fh.write("\n")


if __name__ == "__main__":
    main()
