#!/usr/bin/env python
"""The fit's operands against extended precision, per case: fits every case and
append chain of tests/_fit_cases.py on the device, reads L and L^-1 back
(ut_gp_fit_read) and prints rho of the chol, inv and white measures for the
device, the LAPACK route and the numpy restatement of gp_fit.hip; writes
profiles/fit_factor.json (DESIGN.md's table).

  python scripts/fit_factor_report.py [--out profiles/fit_factor.json]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))

import _fit_cases as F  # noqa: E402
from _spaces import to_manip  # noqa: E402


def fit(c, z):
    from uptune_amd.engine import BatchEngine
    e = BatchEngine(to_manip(z["space"]), device=0, seed=0)
    hy = dict(sigma_f2=c["sf2"], sigma_n2=c["sn2"], jitter=c["jitter"])
    n = c.get("n0", c["n"])
    e.gp_fit(z["X"][:n], z["y"][:n], lengthscale=z["ell"], **hy)
    for s in c.get("steps", ()):
        n += s
        e.gp_fit(z["X"][:n], z["y"][:n], lengthscale=z["ell"], **hy)
    L, info = e.gp_fit_read("L")
    out = dict(L=L.cpu().numpy(), X=e.gp_fit_read("LINV")[0].cpu().numpy(), l_rows=info["l_rows"])
    e.close()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "fit_factor.json"))
    a = ap.parse_args()
    rows = []
    print("%-38s %-6s %10s %10s %12s %8s" % ("case", "", "device", "LAPACK", "restatement", "line"))
    for c in list(F.CASES) + [F.chain_case(*ch) for ch in F.CHAINS]:
        z = F.data(c)
        ref, l_rows = F.references(c, z)
        dv = fit(c, z)
        assert dv["l_rows"] == l_rows
        for m in F.measures_of(c):
            rho, (i, j) = F.measure(m, dv, z, c["n"], l_rows if m == "chol" else None)
            ra, rb = ref[m]
            rows.append(dict(case=c["name"], n=c["n"], npad=F.npad_of(c["n"]), measure=m, device=rho, lapack=ra,
                             restatement=rb, line=F.line(c, ra, rb), cap=F.cap(c), at=[i, j]))
            print("%-38s %-6s %10.3g %10.3g %12.3g %8.3g" % (c["name"], m, rho, ra, rb, F.line(c, ra, rb)), flush=True)
    with open(a.out, "w") as f:
        json.dump(dict(unit="max |error| / first-order bound (tests/_fit_cases.py)", rows=rows), f, indent=1)
        f.write("\n")
    print("wrote", a.out)
    return 0 if all(np.isfinite(r["device"]) and r["device"] <= r["line"] for r in rows) else 1


if __name__ == "__main__":
    sys.exit(main())
