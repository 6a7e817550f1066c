"""Test infrastructure: the case table of per-feature ("ard") lengthscales that
the CPU test of the table (test_ard_cases_cpu.py) and the GPU tests of the
scoring paths (test_gpu_ard_scoring.py) share.  The checker and never the
product.

SharedModel._select_ard hands ut_gp_fit one lengthscale per feature, each
anywhere in ARD's box sqrt(d) * [0.05, 16]; a scalar lengthscale cannot tell a
kernel that indexes 1/ell through the wrong map from one that does not.

Numeric cases (test_gp_vs_oracle's recipe): X uniform in the unit cube,
y = sum (x - 0.4)^2 + 0.01 N, 3000 uniform candidates of which the first ten
are X[:10] + 1e-3; sn2 = 1e-6 sf2, jitter = 1e-8 sf2.  Lengthscale recipes:

  spread           sqrt(d) geomspace(0.05, 16, d), permuted: the whole box
  narrow           sqrt(d) geomspace(0.05, 1, d), permuted (small d)
  one_short_first  a common value, feature 0 at the floor 0.05 sqrt(d)
  one_short_last   a common value, feature d - 1 at the floor (the last real
                   row before K*'s padding)
  a tuple          taken as it is (d = 3)

Categorical cases (test_categorical_kstar_equals_dense's recipe: n = 700,
m = 5000, twenty candidates on training points): one lengthscale per group of
SharedModel._ell_groups -- every ENUM / BOOL column the same one, a numeric
feature its own (spread over a factor of at least 40), a PERM parameter's
columns one."""
import types

import numpy as np

from _spaces import oracle_space, to_manip
from oracle import de as ode
from oracle import gp as ogp
from oracle.space import BOOL, ENUM, FLOAT, INT, PERM, Param, features

M = 3000          # candidates of a numeric case
BOX = (0.05, 16.0)


def in_box(ell):
    d = len(ell)
    lo, hi = np.sqrt(d) * BOX[0], np.sqrt(d) * BOX[1]
    return bool(np.all(ell >= lo * (1.0 - 1e-12)) and np.all(ell <= hi * (1.0 + 1e-12)))


def ell_vector(recipe, d, common=1.5):
    if not isinstance(recipe, str):
        return np.array(recipe, dtype=np.float64)
    perm = np.random.default_rng(4000 + d).permutation(d)
    if recipe == "spread":
        return (np.sqrt(d) * np.geomspace(BOX[0], BOX[1], d))[perm]
    if recipe == "narrow":
        return (np.sqrt(d) * np.geomspace(BOX[0], 1.0, d))[perm]
    ell = np.full(d, float(common))
    ell[{"one_short_first": 0, "one_short_last": d - 1}[recipe]] = BOX[0] * np.sqrt(d)
    return ell


def _n(n, d, recipe, sf2=1.0, common=1.5):
    name = "n%d_d%d_%s" % (n, d, recipe if isinstance(recipe, str) else "hand")
    return dict(name=name, n=n, d=d, recipe=recipe, sf2=sf2, sn2=1e-6 * sf2, jitter=1e-8 * sf2, common=common)


NUMERIC = [
    _n(1024, 64, "spread"),
    _n(1024, 64, "one_short_last", common=2.0),
    _n(600, 33, "spread"),                          # K32 = 2 with 31 padded columns
    _n(600, 33, "one_short_first"),
    _n(600, 33, "one_short_last", sf2=37.0, common=2.0),
    _n(500, 97, "spread", sf2=1e-3),                # just past the paired groups' K = 96; K32 = 4
    _n(500, 97, "one_short_last"),
    _n(300, 16, "spread"),
    _n(200, 8, "narrow"),
    _n(77, 3, (0.15, 0.3, 0.6)),                    # n no multiple of 128
    # (the floor itself: 0.0866 is 3e-6 below 0.05 sqrt(3), outside the box)
    _n(129, 3, (0.05 * 3.0 ** 0.5, 0.25, 0.5)),     # one row into the second tile
]
SHAPES = {(1024, 64), (600, 33), (500, 97), (300, 16), (200, 8), (77, 3), (129, 3)}


def numeric_ids():
    return [c["name"] for c in NUMERIC]


def by_name(name):
    return next(c for c in NUMERIC + CATEGORICAL if c["name"] == name)


def float_space(d):
    return [Param("u%d" % k, FLOAT, 0.0, 1.0) for k in range(d)]


def hyper(c):
    return dict(sigma_f2=c["sf2"], sigma_n2=c["sn2"], jitter=c["jitter"])


_DATA = {}


def _frozen(z):
    for a in z.values():
        if isinstance(a, np.ndarray):
            a.setflags(write=False)
    return z


def numeric_data(c):
    """-> dict X [n][d], y [n], U [M][d], ell [d], gp (oracle GP), mu, var, ei [M]
    (the oracle's); computed once, shared by the tests, never written to"""
    if c["name"] not in _DATA:
        n, d = c["n"], c["d"]
        rng = np.random.default_rng(n + d)
        X = rng.uniform(size=(n, d))
        y = np.sum((X - 0.4) ** 2, axis=1) + 0.01 * rng.standard_normal(n)
        U = rng.uniform(size=(M, d))
        U[:10] = X[:10] + 1e-3
        ell = ell_vector(c["recipe"], d, c["common"])
        g = ogp.GP(X, y, lengthscale=ell, **hyper(c))
        mu, var = g.posterior(U)
        _DATA[c["name"]] = _frozen(dict(X=X, y=y, U=U, ell=ell, gp=g, mu=mu, var=var,
                                        ei=ogp.acquisition(mu, var, g.f_best)))
    return _DATA[c["name"]]


# --------------------------------------------------------------------------- categorical
def mixed_space():
    return [Param("x", FLOAT, -5.0, 5.0), Param("n", INT, 1, 64), Param("flag", BOOL),
            Param("mode", ENUM, options=["a", "b", "c", 4]), Param("y", FLOAT, 0.0, 1.0),
            Param("big", INT, -100000, 2000000)]


def hpl_space():
    from uptune_amd import spaces
    return oracle_space(spaces.hpl64())


def perm_space():
    from uptune_amd import spaces
    return oracle_space(spaces.perm_mixed())


SPACES = {"mixed": mixed_space, "hpl": hpl_space, "perm": perm_space}


def ell_groups(space):
    """feature column -> lengthscale group, by the product's own rule
    (SharedModel._ell_groups over the compiled space; no device)"""
    from uptune_amd.manipulator import compile_space
    from uptune_amd.technique import SharedModel
    spec = compile_space(to_manip(space))
    model = types.SimpleNamespace(engine=types.SimpleNamespace(spec=spec))
    return SharedModel._ell_groups(model, spec.n_features)


def group_kinds(space):
    """per group: "cat" (the ENUM / BOOL columns), "perm" or "num" """
    gid = ell_groups(space)
    kinds, col = {}, 0
    for p in space:
        w = len(p.options) if p.kind in (ENUM, PERM) else 1
        kinds[int(gid[col])] = "cat" if p.kind in (ENUM, BOOL) else "perm" if p.kind == PERM else "num"
        col += w
    assert col == len(gid)
    return [kinds[g] for g in range(len(kinds))]


def _k(which, cat, num_lo, num_hi, perm_vals=(), num_order=None):
    return dict(name="cat_" + which, which=which, cat=cat, num_lo=num_lo, num_hi=num_hi, perm_vals=tuple(perm_vals),
                num_order=num_order, n=700, m=5000, sf2=1.0, sn2=1e-6, jitter=1e-8)


CATEGORICAL = [
    # 700 rows under four numeric lengthscales from the floor 0.15 to 6 (the factor 40) have
    # cond(K) ~ 1e7 whichever feature takes which; this order keeps the oracle's own
    # rounding below 1 % of the tolerance (test_ard_cases_cpu.py), most others do not
    _k("mixed", 0.45, 0.15, 6.0, num_order=(3, 2, 0, 1)),
    _k("hpl", 3.0, 0.7, 28.0),
    _k("perm", 1.2, 0.4, 16.0, perm_vals=(0.6, 1.7, 4.0)),
]


def categorical_ids():
    return [c["name"] for c in CATEGORICAL]


def group_values(c, space):
    """one lengthscale per group: the cat value, geomspace(num_lo, num_hi) over the
    numeric groups in num_order (None: a fixed random one), perm_vals in order over
    the PERM parameters"""
    kinds = group_kinds(space)
    num = [g for g, k in enumerate(kinds) if k == "num"]
    order = c["num_order"] or np.random.default_rng(4100 + len(num)).permutation(len(num))
    vals = np.geomspace(c["num_lo"], c["num_hi"], len(num))[list(order)]
    out = np.empty(len(kinds))
    pv = iter(c["perm_vals"])
    for g, k in enumerate(kinds):
        out[g] = c["cat"] if k == "cat" else next(pv) if k == "perm" else vals[num.index(g)]
    return out


def categorical_data(c):
    """-> dict space, tr [ncols][n] and cand [ncols][m] values, X [n][F], y, U [m][F],
    gid [F], gvals [groups], kinds, ell [F], gp, mu, var, ei (the oracle's); cached"""
    if c["name"] not in _DATA:
        space = SPACES[c["which"]]()
        tr = ode.population_init(space, c["n"], seed=8)
        cand = ode.population_init(space, c["m"], seed=7)
        cand[:, :20] = tr[:, :20]                  # candidates on training points (var ~ 0)
        X = features(space, tr).T.copy()
        y = np.sum((X - 0.35) ** 2, axis=1)
        U = features(space, cand).T.copy()
        gid = ell_groups(space)
        gvals = group_values(c, space)
        ell = np.ascontiguousarray(gvals[gid])
        g = ogp.GP(X, y, lengthscale=ell, **hyper(c))
        mu, var = g.posterior(U)
        _DATA[c["name"]] = _frozen(dict(space=space, tr=tr, cand=cand, X=X, y=y, U=U, gid=gid, gvals=gvals,
                                        kinds=group_kinds(space), ell=ell, gp=g, mu=mu, var=var,
                                        ei=ogp.acquisition(mu, var, g.f_best)))
    return _DATA[c["name"]]


# --------------------------------------------------------------------------- shared tolerances
# test_gp_vs_oracle's: the fp64 tier (precisions 64 and 8) and the fp32 tier (32 and 16)
RTOL, ATOL = 1e-5, 1e-9


def tiers(prec):
    """-> (mu, var, ei) tolerances as (rtol, atol) each, test_gp_vs_oracle's"""
    if prec in (64, 8):
        return (RTOL, ATOL), (RTOL, 1e-8), (RTOL, 1e-8)
    return (RTOL, ATOL), (1e-3, 1e-5), (1e-3, 1e-5)


def worst(got, want, rtol, atol):
    """the largest error as a fraction of its tolerance (<= 1 passes assert_allclose)"""
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    return float(np.max(np.abs(got - want) / (atol + rtol * np.abs(want)))) if got.size else 0.0
