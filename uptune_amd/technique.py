"""Search-technique plugin interface, AUC bandit and the GPU batch techniques.

Mirrors the reference's plugin API so the GPU path drops in where the
per-candidate CPU techniques sit:

  SearchTechnique.desired_result / desired_configuration   opentuner/search/technique.py:70-121
  register / all_techniques / get_enabled                   technique.py:287, 331-355
  MetaSearchTechnique.desired_result                        opentuner/search/metatechniques.py:14-57
  BanditQueue / AUCBanditQueue                              opentuner/search/bandittechniques.py:20-146
  AUCBanditMetaTechnique                                    bandittechniques.py:150-165

`desired_configuration()` returns a config dict, None (nothing to propose ->
the bandit credits 0 and moves on) or False (waiting for results) exactly as
in the reference.  The GPU techniques (GpuDifferentialEvolution, GpuPSO,
GpuGA, GpuGGA, and the opt-in GpuTrustRegion) score a whole candidate pool
per round on the device
(proposal -> hash_config -> dedup -> GP-EI -> top-k) and hand the top-k out one
per call.  Device contexts are created lazily in set_driver and are never
deep-copied (technique instances are deepcopied per driver, driver.py:75).
Device errors never propagate into the driver (the reference's controller
retries forever on exceptions, api.py:433-435): the technique logs and
returns None so the bandit moves on.
"""
from __future__ import annotations

import copy
import logging
import math
import random
from collections import deque
from typing import Any, Dict, List, Optional, Union

import numpy as np

log = logging.getLogger(__name__)


# ---------------------------------------------------------------------------
# plugin interface + registry
# ---------------------------------------------------------------------------
class SearchTechniqueBase:
    def __init__(self, name: Optional[str] = None):
        self.name = name or self.default_name()

    def is_ready(self) -> bool:
        return True

    def default_name(self) -> str:
        return self.__class__.__name__

    def handle_requested_result(self, result) -> None:
        pass

    def set_driver(self, driver) -> None:
        raise NotImplementedError

    def desired_result(self):
        raise NotImplementedError


class SearchTechnique(SearchTechniqueBase):
    """technique.py:70-175: subclasses implement desired_configuration()."""

    def __init__(self, *pargs, **kwargs):
        super().__init__(*pargs, **kwargs)
        self.driver = None
        self.manipulator = None
        self.objective = None
        self.request_count = 0

    def set_driver(self, driver):
        self.driver = driver
        self.manipulator = driver.manipulator
        self.objective = driver.objective

    def desired_result(self):
        """technique.py:88-111: wrap desired_configuration() into a DesiredResult
        (None = nothing to propose, False = waiting for results)"""
        from .driver import Configuration, DesiredResult
        cfg = self.desired_configuration()
        if cfg is None:
            return None
        if cfg is False:
            return False
        config = cfg if isinstance(cfg, Configuration) else self.driver.get_configuration(cfg)
        desired = DesiredResult(configuration=config, requestor=self.name, generation=self.driver.generation,
                                tuning_run=getattr(self.driver, "tuning_run", None))
        if hasattr(self, "limit"):
            desired.limit = self.limit
        self.driver.register_result_callback(desired, self.handle_requested_result)
        self.request_count += 1
        return desired

    def desired_configuration(self):
        raise NotImplementedError


the_registry: List[SearchTechniqueBase] = []


def register(t: SearchTechniqueBase) -> None:
    the_registry.append(t)


def all_techniques() -> List[SearchTechniqueBase]:
    return the_registry


def get_enabled(names: List[str]) -> List[SearchTechniqueBase]:
    known = {t.name for t in the_registry}
    for n in names:
        if n not in known:
            raise Exception("Unknown technique: --technique={}".format(n))
    return [t for t in the_registry if t.name in names]


# ---------------------------------------------------------------------------
# meta techniques / bandit (stay on the CPU: O(#techniques) per request)
# ---------------------------------------------------------------------------
class MetaSearchTechnique(SearchTechniqueBase):
    """metatechniques.py:14-76"""

    def __init__(self, techniques, log_freq=500, *pargs, **kwargs):
        super().__init__(*pargs, **kwargs)
        self.techniques = techniques
        self.request_count = 0
        self.log_freq = log_freq
        self.unique_names()

    def unique_names(self):
        names = set()
        for t in self.techniques:
            while t.name in names:
                t.name += "~"
            names.add(t.name)

    def set_driver(self, driver):
        for t in self.techniques:
            t.set_driver(driver)
        self.driver = driver

    def desired_result(self):
        for technique in self.select_technique_order():
            dr = technique.desired_result()
            if dr is not None:
                if dr is False:
                    continue  # waiting for results
                self.driver.register_result_callback(
                    dr, lambda result, technique=technique: self.on_technique_result(technique, result))
                self.request_count += 1
                return dr
            self.on_technique_no_desired_result(technique)
        return None

    def on_technique_no_desired_result(self, technique):
        pass

    def on_technique_result(self, technique, result):
        pass

    def select_technique_order(self):
        return list(self.techniques)


class BanditQueue:
    """bandittechniques.py:20-79"""

    def __init__(self, keys, C=0.05, window=500, **kwargs):
        self.C = C
        self.history = deque()
        self.keys = keys
        self.use_counts = dict((k, 0) for k in keys)
        self.window = window
        self.request_count = 0

    def exploitation_term(self, key):
        return 0.0

    def exploration_term(self, key):
        if self.use_counts[key] > 0:
            return math.sqrt((2.0 * math.log(len(self.history), 2.0)) / self.use_counts[key])
        return float("inf")

    def bandit_score(self, key):
        return self.exploitation_term(key) + self.C * self.exploration_term(key)

    def ordered_keys(self, rng=random):
        keys = list(self.keys)
        rng.shuffle(keys)  # break ties randomly
        keys.sort(key=self.bandit_score)
        self.request_count += 1
        return reversed(keys)

    def on_result(self, key, value):
        self.history.append((key, value))
        self.on_push_history(key, value)
        if len(self.history) > self.window:
            self.on_pop_history(*self.history.popleft())

    def on_push_history(self, key, value):
        self.use_counts[key] += 1

    def on_pop_history(self, key, value):
        self.use_counts[key] -= 1


class AUCBanditQueue(BanditQueue):
    """Area-under-curve credit assignment (Fialho et al.): a restatement of
    bandittechniques.py:82-146 with the same scores and tie-break sequence.
    The exploitation term is the reference's O(1) incremental form: with the
    uses of `key` in the window numbered 1..pos, AUC = 2 * (sum of the
    numbers of the credited uses) / (pos * (pos + 1)).  auc_sum holds that
    sum; popping the oldest use renumbers the rest down by one, i.e. subtracts
    the number of credited uses left (auc_decay)."""

    def __init__(self, *args, **kwargs):
        super().__init__(*args, **kwargs)
        self.auc_sum = dict((t, 0) for t in self.keys)
        self.auc_decay = dict((t, 0) for t in self.keys)

    def exploitation_term(self, key):
        pos = self.use_counts[key]
        if pos:
            return self.auc_sum[key] * 2.0 / (pos * (pos + 1.0))
        return 0.0

    def on_push_history(self, key, value):
        super().on_push_history(key, value)
        if value:
            self.auc_sum[key] += self.use_counts[key]
            self.auc_decay[key] += 1

    def on_pop_history(self, key, value):
        super().on_pop_history(key, value)
        self.auc_sum[key] -= self.auc_decay[key]
        if value:
            self.auc_decay[key] -= 1


class AUCBanditMetaTechnique(MetaSearchTechnique):
    """bandittechniques.py:150-165"""

    def __init__(self, techniques, bandit_kwargs=None, seed: Optional[int] = None, **kwargs):
        super().__init__(techniques, **kwargs)
        self.bandit = AUCBanditQueue([t.name for t in techniques], **(bandit_kwargs or {}))
        self.name_to_technique = dict((t.name, t) for t in self.techniques)
        self._rng = random.Random(seed) if seed is not None else None  # None: the global `random`

    def select_technique_order(self):
        return [self.name_to_technique[k] for k in self.bandit.ordered_keys(self._rng or random)]

    def on_technique_result(self, technique, result):
        self.bandit.on_result(technique.name, result.was_new_best)

    def on_technique_no_desired_result(self, technique):
        self.bandit.on_result(technique.name, 0)


# ---------------------------------------------------------------------------
# GPU batch techniques
# ---------------------------------------------------------------------------
class SharedModel:
    """Device state the GPU techniques of one bandit share: ONE context, hence
    one history digest set and one GP fit per change of the training set (the
    reference composes DE, PSO and GA under one bandit, bandittechniques.py:311-320,
    and north_star C5 asks for a shared surrogate).  Each technique keeps its
    own population in a slot of that context (ut_population_select).

    A technique built without `shared=` makes a private SharedModel, so a
    stand-alone technique and a bandit member run the same code.  Everything
    here reads the driver only through the reference SearchDriver surface:
    requests_query() (every requested configuration's hash -> the dedup set),
    results_query() (Configuration.data + time -> the training set)."""

    def __init__(self, device: int = 0, seed: int = 0, lengthscale: Union[float, str] = 0.3, min_train: int = 4,
                 precision: int = 64, sigma_f2: float = 1.0, sigma_n2: float = 1e-6, jitter: float = 1e-8,
                 engine_factory=None, y_transform: Optional[str] = None, ell_grid=None, ard_maxiter: int = 40,
                 feasibility: Union[bool, Dict[str, Any]] = False, constraints=None, prune_weighted: bool = False,
                 surrogate: Optional[str] = None, forest_kw: Optional[Dict[str, Any]] = None,
                 objectives=None, ref_point=None):
        if isinstance(lengthscale, str) and lengthscale not in ("auto", "ard"):
            raise ValueError("lengthscale: a number (or one per feature), 'auto' or 'ard'")
        self.device, self.seed, self.lengthscale, self.min_train = device, seed, lengthscale, min_train
        self.precision = precision
        # lengthscale="ard": one lengthscale per feature group, by L-BFGS-B on the
        # log marginal likelihood over log ell (engine.gp_lml_grad: the gradient
        # of the fit in place), started at "auto"'s isotropic choice, at most
        # ard_maxiter iterations, every ell within [grid min, 4 grid max]; at the
        # same moments as "auto".  A group is one numeric feature, one PERM
        # parameter's columns, or all ENUM / BOOL one-hot columns together (the
        # categorical K* needs one lengthscale over those).  Never worse than
        # "auto": a result whose LML does not exceed the start's is dropped for
        # the start.  lengthscale_ is then the per-feature array.
        self.ard_maxiter = int(ard_maxiter)
        # lengthscale="auto": the lengthscale is the candidate of ell_grid
        # (isotropic; default sqrt(n_features) * geomspace(0.05, 4, 16)) with the
        # largest log marginal likelihood on the fit's own rows and targets
        # (engine.gp_lml_grid: one batched factorisation chain).  Chosen at the
        # first fit and wherever the padded size changes -- where the device
        # refactors anyway -- so the incremental fits in between keep identical
        # hyperparameters.  lengthscale_ is the value in use, ell_history one
        # (n, ell, lml) per selection.
        self.ell_grid = None if ell_grid is None else np.asarray(ell_grid, dtype=np.float64).ravel()
        self.lengthscale_ = None if isinstance(lengthscale, str) else lengthscale
        self.ell_history: List[Any] = []
        # y_transform: what the GP is fitted on.  None = the objective as
        # measured; "rank" = its normal scores, Phi^-1((rank + 1/2) / n) (order
        # preserving, so the incumbent stays the minimum): an objective spanning
        # many decades (Rosenbrock over [-1000, 1000]^2: 0 .. 1e14) otherwise
        # standardises to a flat landscape where EI only explores
        if y_transform not in (None, "rank"):
            raise ValueError("y_transform: None or 'rank'")
        self.y_transform = y_transform
        # engine_factory(manipulator, device, seed) -> a BatchEngine-compatible
        # object; None = uptune_amd.engine.BatchEngine (the device path).  Tests
        # substitute a CPU stand-in to exercise the plugin plumbing without a GPU.
        self.engine_factory = engine_factory
        self.hyper = dict(sigma_f2=sigma_f2, sigma_n2=sigma_n2, jitter=jitter)
        # feasibility: False, True or a dict of prior / strength / ell_scale /
        # power (engine.gp_feas_set).  When on, fit() also loads the features of
        # the driver's results that FAILED (not usable, but with a configuration),
        # in arrival order, and every EI score is weighted by the kernel vote of
        # the training rows against them.  n_failed is how many are loaded.
        self.feasibility = _feas_setting(feasibility)
        # constraints: [(attr, op, threshold), ...], op "<=" or ">=", at most 4:
        # measurements every result carries as an attribute (accuracy, energy,
        # size, ...; the reference's ThresholdAccuracyMinimizeTime, objective.py:246-298,
        # is [("accuracy", ">=", target)]).  fit() gathers them for the training
        # rows, in the fit's row order, and loads them after every gp_fit
        # (engine.gp_cons_set; ">=" negated): EI then counts only improvement on
        # the best FEASIBLE result, times the probability that every constraint
        # holds under a GP on the fit's own factor.  A result whose attribute is
        # missing, None or not finite is not usable (neither trained on nor
        # failed).  n_feasible_ is the feasible training rows of the last fit.
        self.constraints = _cons_setting(constraints)
        # prune_weighted: the engine's pruned rounds accept the loaded failed
        # rows / constraint values and select by the weighted score
        # (engine.gp_set_prune_weighted); False: they refuse, and a technique
        # with prune_rows > 0 cannot use this model's feasibility / constraints
        self.prune_weighted = bool(prune_weighted)
        # surrogate: None = the GP; "forest" = a random forest refitted on the
        # host from the same usable rows, features and y_transform whenever the
        # GP would refit: RandomForestRegressor(n_estimators=64, min_samples_leaf=3,
        # random_state=seed, **forest_kw), deterministic for a seed and data (SPMD
        # replicas agree), loaded with its leaf variances and scored by EI / UCB
        # on the mean and variance over trees (engine.forest_score; SMAC's
        # model).  f_best is min(y) in the units fitted, fit_seconds the host
        # time spent in RandomForestRegressor.fit.  The GP's weights
        # (feasibility, constraints) and its pruned rounds do not apply.
        if surrogate not in (None, "forest"):
            raise ValueError("SharedModel surrogate: None (the GP) or 'forest'")
        if surrogate is not None and (self.feasibility is not None or self.constraints):
            raise ValueError("feasibility and constraints weight the GP's EI: not with a tree surrogate")
        self.surrogate = surrogate
        self.forest_kw = dict(forest_kw or {})
        # objectives: [("time", "min"), (attr, "min" or "max")] -- a second
        # measurement every result carries (accuracy, energy, size, confidence)
        # is minimised (or maximised) beside the time, with no trade-off fixed
        # beforehand.  time stays the GP's y (with its y_transform); the second
        # one's values of the training rows ride beside it as constraint values
        # do, are loaded after every gp_fit (engine.gp_mo_set; "max" negated),
        # and every EI score becomes the expected hypervolume improvement against
        # the rows' Pareto front.  ref_point: the reference point in raw units
        # (time, second), its first coordinate passed through y_transform; None =
        # pareto.default_ref of the usable rows at the first fit, held from then
        # on so that hypervolumes within a run compare.  ref_point_ is the point
        # in use, in the units fitted (time, signed second).
        self.objectives = _mo_setting(objectives)
        if self.objectives:
            if self.constraints:
                raise ValueError("objectives: constrained EHVI is not built: no constraints with two objectives")
            if self.feasibility is not None:
                raise ValueError("objectives: EHVI under the failure vote is not built: no feasibility with two "
                                 "objectives")
            if surrogate is not None:
                raise ValueError("objectives: EHVI needs the GP's joint posterior: not with a tree surrogate")
        if ref_point is not None:
            if not self.objectives:
                raise ValueError("ref_point belongs to objectives=")
            ref_point = tuple(float(v) for v in ref_point)
            if len(ref_point) != 2 or not all(math.isfinite(v) for v in ref_point):
                raise ValueError("ref_point: two finite coordinates (time, second), raw units")
        self.ref_point = ref_point
        self._reset()
        self.slots: Dict[str, int] = {}

    def _reset(self):
        self.engine = None
        self._req_seen = 0          # requests_query() rows pushed to the device set (list drivers)
        self._hist = set()          # digests pushed (any driver)
        self._res_ids: List[Any] = []
        # training rows in arrival order (features, objective): the first _n
        # rows of capacity-grown buffers, so a fit that appends a few results
        # copies only those
        self._n = 0
        self._Xa = np.zeros((0, 0))
        self._ya = np.zeros(0)
        # the same rows in the fit's order (what gp_fit receives): best y first
        # as of the last refit, the results since appended in arrival order
        self._Xf = np.zeros((0, 0))
        self._yf = np.zeros(0)
        self._nf = 0
        self._perm_npad = 0
        self._ell_npad = 0          # padded size of the fit the lengthscale was last selected at ("auto")
        # features of the rounds' selections, encoded on the device beside
        # them (GpuBatchTechnique._round), by hash_config digest: a result of a
        # selected configuration needs no second encode round trip
        self._feat_cache: Dict[str, np.ndarray] = {}
        self._fit_key = None
        self._fit_unverified = False
        self.fits = 0
        self.ts_rounds = 0          # Thompson-sampling draws made on this model (next_ts_round)
        self.f_best = None          # surrogate="forest": min(y) of the last fit, in the units fitted
        self.fit_seconds = 0.0      # ... and the host time of its RandomForestRegressor.fit calls
        # list drivers (append-only results table): the usable rows found so
        # far and how far the table has been scanned
        self._scan_n = 0
        self._scan_last = None
        self._scan_rows: List[Any] = []
        self._scan_ids: List[Any] = []
        # feasibility: the failed results found so far (list drivers: by the
        # same scan), their features in arrival order and how many of them the
        # engine holds (-1: what it holds is stale)
        self._scan_failed: List[Any] = []
        self._fail_X = np.zeros((0, 0))
        self._fail_k = 0
        self._fail_sent = 0
        self.n_failed = 0
        # constraints: the training rows' signed values (c <= t form), arrival
        # order and the fit's order, beside _ya / _yf
        self._Ca = np.zeros((0, 0))
        self._Cf = np.zeros((0, 0))
        self.n_feasible_ = None
        self.ref_point_ = None      # objectives: the reference point in use, units fitted

    def _side_columns(self) -> List[Any]:
        """what rides beside y as (attr, op, _): the constraints, or the second
        objective as one column ("max" = ">=": negated)"""
        if self.objectives:
            attr, sense = self.objectives[1]
            return [(attr, ">=" if sense == "max" else "<=", None)]
        return self.constraints

    def __deepcopy__(self, memo):
        # techniques (and so their shared model) are deep-copied per driver
        # (driver.py:75): the copy starts without a device context
        new = self.__class__.__new__(self.__class__)
        memo[id(self)] = new
        new.__dict__.update({k: copy.deepcopy(v, memo) for k, v in self.__dict__.items() if k != "engine"})
        new._reset()
        return new

    def next_ts_round(self) -> int:
        """the 24-bit key of the next Thompson-sampling draw: a counter, so that
        no two draws on one model (whichever technique makes them) share a key"""
        r = self.ts_rounds & 0xFFFFFF
        self.ts_rounds += 1
        return r

    def slot(self, tech) -> int:
        return self.slots.setdefault(tech.name, len(self.slots))

    def engine_for(self, tech):
        """the shared engine with `tech`'s population slot selected"""
        if self.engine is None:
            if self.engine_factory is None:
                from .engine import BatchEngine
                self.engine = BatchEngine(tech.manipulator, device=self.device, seed=self.seed)
            else:
                self.engine = self.engine_factory(tech.manipulator, self.device, self.seed)
            self.engine.gp_set_precision(self.precision)
            if self.prune_weighted:
                self.engine.gp_set_prune_weighted(True)
            self.engine.history_reset(1024)
        self.engine.population_select(self.slot(tech))
        return self.engine

    def sync_history(self, driver) -> None:
        """every configuration the driver has requested joins the device dedup
        set (driver.py:157-158,177-200: history + in-flight requests)"""
        reqs = driver.requests_query()
        if isinstance(reqs, list):             # append-only table: only the new rows
            rows, self._req_seen = reqs[self._req_seen:], len(reqs)
        else:                                  # a SQL query (reference driver): all rows, filtered
            rows = reqs
        new = []
        for dr in rows:
            h = dr.configuration.hash
            if h not in self._hist:
                self._hist.add(h)
                new.append(h)
        if new:
            self.engine.history_add(new)

    def _scan(self, driver):
        """the driver's results as (usable rows, their ids, failed results), in
        arrival order: what either surrogate trains on"""
        cons = self._side_columns()

        def measured(r):   # (constraints) every constrained measurement is there and finite
            for attr, _, _ in cons:
                v = getattr(r, attr, None)
                if v is None or not math.isfinite(v):
                    return False
            return True

        def usable(r):
            return (getattr(r, "state", "OK") == "OK" and r.time is not None and math.isfinite(r.time)
                    and (not cons or measured(r)))

        def failed(r):   # (feasibility) a result that is not usable but says where it failed
            if cons and getattr(r, "state", "OK") == "OK" and r.time is not None and math.isfinite(r.time):
                return False   # it ran: only a constrained measurement is missing
            return self.feasibility is not None and getattr(r, "configuration", None) is not None

        res = driver.results_query()
        if isinstance(res, list):
            # an in-memory table only grows: scan the rows added since the last
            # call (a table that shrank or changed under us is rescanned)
            if len(res) < self._scan_n or (self._scan_n and res[self._scan_n - 1] is not self._scan_last):
                self._scan_n, self._scan_rows, self._scan_ids, self._scan_failed = 0, [], [], []
                self._fail_k = 0
            for r in res[self._scan_n:]:
                if usable(r):
                    self._scan_ids.append(getattr(r, "id", len(self._scan_rows)))
                    self._scan_rows.append(r)
                elif failed(r):
                    self._scan_failed.append(r)
            self._scan_n = len(res)
            self._scan_last = res[-1] if res else None
            rows, ids, bad = self._scan_rows, self._scan_ids, self._scan_failed
        else:   # a SQL query (reference driver): every row, filtered
            res = list(res)
            rows = [r for r in res if usable(r)]
            ids = [getattr(r, "id", i) for i, r in enumerate(rows)]
            bad = [r for r in res if not usable(r) and failed(r)]
            self._fail_k = 0
        return rows, ids, bad

    def _gather(self, rows, ids) -> None:
        """_Xa / _ya (and _Ca) := the features, objectives (and signed constraint
        values) of `rows`, arrival order; only the rows appended since the last
        call are encoded"""
        cons = self._side_columns()
        k = self._n
        if k == 0 or ids[:k] != self._res_ids:      # not an append: re-encode everything
            k = self._n = self._nf = 0
            self._fail_k = 0
            if self._fail_sent > 0:
                self._fail_sent = -1
        new = rows[k:]
        if new:
            n = k + len(new)
            self._Xa, self._ya = _rows_room(self._Xa, self._ya, k, n, self.engine.spec.n_features)
            self._Xa[k:n] = self._features(new)
            self._ya[k:n] = [float(r.time) for r in new]
            if cons:
                self._Ca = _cols_room(self._Ca, k, n, len(cons))
                self._Ca[k:n] = [[(-1.0 if op == ">=" else 1.0) * float(getattr(r, attr)) for attr, op, _ in cons]
                                 for r in new]
            self._n = n
            self._res_ids = list(ids)   # a copy: the scan list keeps growing

    def _transform(self, y):
        """what the surrogate is fitted on (y_transform)"""
        if self.y_transform == "rank":
            from scipy.special import ndtri
            from scipy.stats import rankdata
            # average ranks: tied (repeated) measurements get one normal score,
            # whatever their row order
            r = rankdata(y, method="average") - 1.0
            y = ndtri((r + 0.5) / len(y))
        return y

    def _transform_point(self, t: float, y) -> float:
        """one raw objective value in the units _transform(y) is in: under
        "rank" the normal score of its rank among y (average rank on ties),
        which moves with the data, so it is taken again at every fit"""
        if self.y_transform == "rank":
            from scipy.special import ndtri
            y = np.asarray(y)
            r = float(np.sum(y < t)) + 0.5 * float(np.sum(y == t))
            return float(ndtri((r + 0.5) / (len(y) + 1)))
        return float(t)

    def _fit_forest(self, rows, ids) -> bool:
        """surrogate="forest": refit the random forest iff the usable results changed"""
        import time

        from sklearn.ensemble import RandomForestRegressor

        from .forest import from_sklearn
        key = (len(rows), ids[-1])
        if key == self._fit_key:
            return True
        self._gather(rows, ids)
        n = self._n
        y = self._transform(self._ya[:n])
        kw = dict(n_estimators=64, min_samples_leaf=3, random_state=self.seed)
        kw.update(self.forest_kw)
        t0 = time.perf_counter()
        rf = RandomForestRegressor(**kw).fit(self._Xa[:n], y)
        self.fit_seconds += time.perf_counter() - t0
        self.engine.forest_set(from_sklearn(rf, leaf_var=True))
        self.f_best = float(np.min(y))
        self._fit_key = key
        self.fits += 1
        return True

    def fit(self, driver) -> bool:
        """(re)fit the surrogate iff the driver's results changed since the last
        fit.  The GP: the new training rows are encoded on the device
        (ut_encode_features) and the fit is enqueued without a host wait
        (ut_gp_fit_async)"""
        cons = self._side_columns()
        rows, ids, bad = self._scan(driver)
        if len(rows) < self.min_train:
            return False
        if self.surrogate == "forest":
            return self._fit_forest(rows, ids)
        if self._fit_unverified and self._fit_key is not None:
            # the previous fit ran asynchronously (no host wait when it was
            # enqueued): a kernel matrix that was not positive definite would
            # leave every score NaN, so check it once, before reusing it
            self._fit_unverified = False
            if not self.engine.gp_fit_ok():
                self.hyper["jitter"] = max(10.0 * self.hyper.get("jitter", 0.0), 1e-8)
                log.warning("GP fit on %d results was not positive definite: refitting with jitter %g",
                            self._fit_key[0], self.hyper["jitter"])
                self._fit_key = None
        key = (len(rows), ids[-1])
        if key == self._fit_key:
            self._load_failed(bad)      # failures alone do not refit, but they count
            return True
        self._gather(rows, ids)
        # Row order.  The GP posterior does not depend on it, but the EI bound of
        # pruned scoring (ut_gp_topk_pruned) comes from the first rows of L^-1:
        # with the best results first it sees the neighbourhood that GA / GGA
        # children (mutations of the best configuration) live in (the C5 GGA
        # round: 262,144 survivors -> 8, 75 -> 5 ms; a GA round: 2,459 -> 8,
        # scripts/exp/gga_prune_probe.py).  The rows are re-sorted only where
        # the device refits anyway (a new padded size, ut_internal.h NPAD = 128, or a
        # re-encode); in between the new results are appended, so the
        # incremental fit still applies.
        n = self._n
        npad = -(-n // 128) * 128
        self._Xf, self._yf = _rows_room(self._Xf, self._yf, self._nf, n, self._Xa.shape[1])
        if cons:
            self._Cf = _cols_room(self._Cf, self._nf, n, len(cons))
        if self._nf == 0 or npad != self._perm_npad or self._nf > n:
            perm = np.argsort(self._ya[:n], kind="stable")
            self._Xf[:n] = self._Xa[perm]
            self._yf[:n] = self._ya[perm]
            if cons:   # (re-gathered with the rows)
                self._Cf[:n] = self._Ca[perm]
            self._perm_npad = npad
        else:
            self._Xf[self._nf:n] = self._Xa[self._nf:n]
            self._yf[self._nf:n] = self._ya[self._nf:n]
            if cons:
                self._Cf[self._nf:n] = self._Ca[self._nf:n]
        self._nf = n
        y = self._transform(self._yf[:n])
        ell = self.lengthscale
        if isinstance(ell, str):   # "auto" / "ard"
            if npad != self._ell_npad:
                if ell == "ard":
                    self._select_ard(self._Xf[:n], y)
                else:
                    self._select_lengthscale(self._Xf[:n], y)
                self._ell_npad = npad
            ell = self.lengthscale_
        self.engine.gp_fit(self._Xf[:n], y, lengthscale=ell, wait=False, **self.hyper)
        if self.objectives:
            # the second objective's values belong to this fit, as constraint
            # values do; the reference point is chosen once
            if self.ref_point is not None:
                sign = -1.0 if self.objectives[1][1] == "max" else 1.0
                self.ref_point_ = (self._transform_point(self.ref_point[0], self._yf[:n]), sign * self.ref_point[1])
            elif self.ref_point_ is None:
                from .pareto import default_ref
                self.ref_point_ = tuple(float(v) for v in default_ref(np.column_stack([y, self._Cf[:n, 0]])))
            self.engine.gp_mo_set(self._Cf[:n, 0], self.ref_point_)
        elif cons:
            # the values belong to this fit (the last one, after any of the
            # lengthscale selection's own); no host wait in between
            thr = [(-1.0 if op == ">=" else 1.0) * float(t) for _, op, t in cons]
            self.engine.gp_cons_set(self._Cf[:n], thr)
            self.n_feasible_ = int(np.all(self._Cf[:n] <= np.asarray(thr), axis=1).sum())
        self._fit_key = key
        self._fit_unverified = True
        self.fits += 1
        self._load_failed(bad)
        return True

    def _load_failed(self, bad) -> None:
        """(feasibility) the failed results' features to the engine, whenever
        their number changed or the model was re-encoded: the new ones encoded
        through _features (the round's cached encodings), rows in arrival order"""
        if self.feasibility is None:
            return
        k, n = min(self._fail_k, len(bad)), len(bad)
        if n > k:
            X, _ = _rows_room(self._fail_X, np.zeros(self._fail_X.shape[0]), k, n, self.engine.spec.n_features)
            X[k:n] = self._features(bad[k:])
            self._fail_X, self._fail_k = X, n
        if n == self._fail_sent:
            return
        self.engine.gp_feas_set(self._fail_X[:n], **self.feasibility)
        self._fail_sent = self.n_failed = n

    def _grid(self, d: int) -> np.ndarray:
        return math.sqrt(d) * np.geomspace(0.05, 4.0, 16) if self.ell_grid is None else self.ell_grid

    def _select_lengthscale(self, X, y) -> None:
        """lengthscale_ := the grid candidate with the largest log marginal
        likelihood of (X, y); when no candidate is positive definite the previous
        choice stays (the grid's median on the first fit) and the fit's jitter
        retry takes it from there"""
        grid = self._grid(X.shape[1])
        lml, best = self.engine.gp_lml_grid(X, y, 1.0, grid, **self.hyper)
        if best >= 0:
            self.lengthscale_ = float(grid[best])
        elif self.lengthscale_ is None:
            self.lengthscale_ = float(np.median(grid))
        self.ell_history.append((len(y), self.lengthscale_, float(lml[best]) if best >= 0 else float("nan")))

    def _ell_groups(self, d: int) -> np.ndarray:
        """feature column -> its lengthscale group ("ard"): numeric features one
        each, a PERM parameter's columns one, every ENUM / BOOL column the same one"""
        from . import _lib as L
        gid = np.zeros(d, dtype=np.int64)
        ng, cat = 0, -1
        for p in self.engine.spec.params:
            if p.kind in (L.UT_ENUM, L.UT_BOOL):
                if cat < 0:
                    cat, ng = ng, ng + 1
                g = cat
            else:
                g, ng = ng, ng + 1
            gid[p.feat_col:p.feat_col + p.n_feat] = g
        return gid

    def _select_ard(self, X, y) -> None:
        """lengthscale_ := one lengthscale per feature (per group, _ell_groups)
        by L-BFGS-B on the log marginal likelihood of (X, y) from the grid's
        isotropic best; each evaluation is a fit at the point, its LML and its
        gradient on the device.  A point that is not positive definite is
        rejected, and a result no better than the start keeps the start."""
        from scipy.optimize import minimize

        from ._lib import UthotError
        d = X.shape[1]
        grid = self._grid(d)
        lml, best = self.engine.gp_lml_grid(X, y, 1.0, grid, **self.hyper)
        if best < 0:   # as "auto": the previous choice stays (the grid's median on the first fit)
            if self.lengthscale_ is None:
                self.lengthscale_ = np.full(d, float(np.median(grid)))
            self.ell_history.append((len(y), self.lengthscale_, float("nan")))
            return
        ell0, lml0 = float(grid[best]), float(lml[best])
        gid = self._ell_groups(d)
        ng = int(gid.max()) + 1
        top = {"lml": lml0, "theta": None}
        reject = -lml0 + 1e3 * (1.0 + abs(lml0))   # a rejected point: far worse than the start, flat

        def neg_lml(theta):
            ell = np.exp(theta)[gid]
            try:
                self.engine.gp_fit(X, y, lengthscale=ell, wait=True, **self.hyper)
                ok = self.engine.gp_fit_ok()
            except UthotError as e:
                if "UT_ENOTPD" not in str(e):
                    raise
                ok = False
            if not ok:
                return reject, np.zeros(ng)
            v = float(self.engine.gp_lml())
            g = self.engine.gp_lml_grad()[0]
            if v > top["lml"] and not np.array_equal(theta, theta0):   # (the start is the grid's own point)
                top["lml"], top["theta"] = v, np.array(theta, dtype=np.float64)
            return -v, -np.bincount(gid, weights=g, minlength=ng)

        lo, hi = math.log(float(np.min(grid))), math.log(4.0 * float(np.max(grid)))
        theta0 = np.full(ng, math.log(ell0))
        minimize(neg_lml, theta0, jac=True, method="L-BFGS-B", bounds=[(lo, hi)] * ng,
                 options={"maxiter": self.ard_maxiter})
        if top["theta"] is None:   # nothing beat the isotropic start
            ell = np.full(d, ell0)
        else:
            ell = np.ascontiguousarray(np.exp(top["theta"])[gid])
        self.lengthscale_ = ell
        self.ell_history.append((len(y), ell, top["lml"]))

    def note_selections(self, hexes) -> None:
        """a round's selections are requests the driver has not made yet: they
        join the dedup set now, so no technique sharing this model selects one
        of them again while it waits in a queue (a bandit runs other techniques'
        rounds between the requests of one round's batch)"""
        new = [h for h in hexes if h not in self._hist]
        if new:
            self._hist.update(new)
            self.engine.history_add(new)

    def remember_features(self, hexes, feat) -> None:
        """features [k][F] of configurations selected this round, by digest"""
        if len(self._feat_cache) > (1 << 16):   # selections never evaluated: bounded
            self._feat_cache.clear()
        for hx, f in zip(hexes, feat):
            self._feat_cache[hx] = f

    def _features(self, results) -> np.ndarray:
        """GP features of results: the round's device encoding where the result's
        configuration is one of the selections, else encoded now"""
        out = np.empty((len(results), self.engine.spec.n_features))
        miss = []
        for i, r in enumerate(results):
            f = self._feat_cache.pop(getattr(r.configuration, "hash", None), None)
            if f is None:
                miss.append(i)
            else:
                out[i] = f
        if miss:
            out[miss] = self.engine.features_host([results[i].configuration.data for i in miss])
        return out


def _feas_setting(feasibility) -> Optional[Dict[str, Any]]:
    """feasibility= as gp_feas_set's keyword arguments; None = off"""
    if feasibility is False or feasibility is None:
        return None
    if feasibility is True:
        return {}
    if not isinstance(feasibility, dict) or set(feasibility) - {"prior", "strength", "ell_scale", "power"}:
        raise ValueError("feasibility: False, True or a dict of prior, strength, ell_scale, power")
    return dict(feasibility)


def _cons_setting(constraints) -> List[Any]:
    """constraints= as a list of (attr, op, threshold); [] = off"""
    if not constraints:
        return []
    out = []
    for c in constraints:
        if not isinstance(c, (tuple, list)) or len(c) != 3 or not isinstance(c[0], str) or c[1] not in ("<=", ">="):
            raise ValueError("constraints: a list of (attribute, '<=' or '>=', threshold)")
        t = float(c[2])
        if math.isnan(t):
            raise ValueError("constraints: a threshold is NaN")
        out.append((c[0], c[1], t))
    if len(out) > 4:
        raise ValueError("constraints: at most 4 (UT_CONS_MAX)")
    return out


def _mo_setting(objectives) -> List[Any]:
    """objectives= as [("time", sense), (attr, sense)]; [] = off (one objective)"""
    if not objectives:
        return []
    out = [tuple(o) if isinstance(o, (tuple, list)) else o for o in objectives]
    if len(out) != 2 or any(not isinstance(o, tuple) or len(o) != 2 or o[1] not in ("min", "max") for o in out):
        raise ValueError("objectives: exactly two of (attribute, 'min' or 'max'); more than two are not built")
    if out[0] != ("time", "min"):
        raise ValueError("objectives: the first is ('time', 'min'), the GP's own target")
    if out[1][0] not in ("accuracy", "energy", "size", "confidence"):
        raise ValueError("objectives: the second is one of accuracy, energy, size, confidence")
    return out


def _cols_room(Cm, used, n, nc):
    """Cm with room for n rows of nc constraint values, the first `used` rows kept"""
    if Cm.shape[0] >= n and Cm.shape[1] == nc:
        return Cm
    C2 = np.empty((max(n + n // 2, 256), nc))
    used = min(used, n, Cm.shape[0])
    if used and Cm.shape[1] == nc:
        C2[:used] = Cm[:used]
    return C2


def _rows_room(X, y, used, n, d):
    """(X, y) with room for n rows of d features, the first `used` rows kept"""
    if X.shape[0] >= n and X.shape[1] == d:
        return X, y
    cap = max(n + n // 2, 256)
    X2, y2 = np.empty((cap, d)), np.empty(cap)
    used = min(used, n, X.shape[0])
    if used and X.shape[1] == d:
        X2[:used], y2[:used] = X[:used], y[:used]
    return X2, y2


class GpuBatchTechnique(SearchTechnique):
    """Base of the device-scored population techniques.

    One round = propose `pool` candidates with the technique's operator,
    hash_config + dedup against every configuration the driver has seen,
    score with the shared GP (EI/UCB) fitted on the driver's results, keep
    the top `batch`; desired_configuration() then returns them one per call.
    """

    # DE / GA pools shard over the ranks of a process group by GLOBAL candidate
    # index; PSO moves its (small) swarm on every rank (replicas)
    sharded = True

    def __init__(self, pool: int = 1 << 14, batch: int = 8, population: int = 1024, device: int = 0,
                 seed: int = 0, lengthscale: Union[float, str] = 0.3, min_train: int = 4, acq: str = "ei",
                 group=None, surrogate=None, shared: Optional[SharedModel] = None, engine_factory=None,
                 prune_rows: int = 0, precision: int = 64, y_transform: Optional[str] = None, diversify: int = 0,
                 feasibility: Union[bool, Dict[str, Any]] = False, constraints=None, prune_weighted: bool = False,
                 forest_kw: Optional[Dict[str, Any]] = None, polish: int = 0, polish_pool: Optional[int] = None,
                 ts_features: int = 1024, objectives=None, ref_point=None, *pargs, **kwargs):
        super().__init__(*pargs, **kwargs)
        # surrogate="forest" (SharedModel): a random forest refitted from the
        # driver's results, scored by EI / UCB on its mean and variance over
        # trees.  A shared model carries its own setting (and forest_kw)
        refit = isinstance(surrogate, str) and surrogate == "forest"
        if shared is not None:
            if refit and shared.surrogate != "forest":
                raise ValueError("surrogate='forest' with a shared model that fits a GP")
            if surrogate is not None and not refit and shared.surrogate == "forest":
                raise ValueError("a model object as surrogate with a shared model that refits a forest")
            refit = shared.surrogate == "forest"
        tree = refit or surrogate is not None
        # prune_weighted (SharedModel): pruned rounds under constraints / feasibility,
        # by the weighted bound of ut_gp_set_prune_weighted.  A shared model carries its own
        weighted = shared.prune_weighted if shared is not None else bool(prune_weighted)
        # constraints (SharedModel): EI over the best feasible result times the
        # probability that every measured constraint holds.  A shared model
        # carries its own setting; the rule is defined for the dense EI score only
        if shared.constraints if shared is not None else _cons_setting(constraints):
            if int(prune_rows) > 0 and not weighted:
                raise ValueError("constraints weight every candidate's score: not with prune_rows")
            if int(diversify) > 0:
                raise ValueError("constraints are not known to the per-pick acquisition: not with diversify")
            if acq == "ucb":
                raise ValueError("constraints multiply a score that is >= 0: EI, not acq='ucb'")
            if tree:
                raise ValueError("constraints weight the GP's EI: not with a tree surrogate")
        # feasibility (SharedModel): EI times the estimated probability that the
        # candidate does not fail.  A shared model carries its own setting; the
        # weight is defined for the dense EI score only
        if (shared.feasibility if shared is not None else _feas_setting(feasibility)) is not None:
            if int(prune_rows) > 0 and not weighted:
                raise ValueError("feasibility weights every candidate's score: not with prune_rows")
            if int(diversify) > 0:
                raise ValueError("feasibility is not known to the per-pick acquisition: not with diversify")
            if acq == "ucb":
                raise ValueError("feasibility multiplies a score that is >= 0: EI, not acq='ucb'")
            if tree:
                raise ValueError("feasibility weights the GP's EI: not with a tree surrogate")
        # objectives (SharedModel): every EI score becomes the expected hypervolume
        # improvement over time and a second measurement.  A shared model carries
        # its own setting; EHVI is built for the dense EI score alone
        if shared.objectives if shared is not None else _mo_setting(objectives):
            if int(prune_rows) > 0:
                raise ValueError("objectives: the pruning bound does not know EHVI: not with prune_rows")
            if int(diversify) > 0:
                raise ValueError("objectives: EHVI is not known to the per-pick acquisition: not with diversify")
            if acq == "ucb":
                raise ValueError("objectives: EHVI stands in for EI, there is no two-objective UCB: not acq='ucb'")
            if acq == "ts":
                raise ValueError("objectives: paths of two objectives are not built: not acq='ts'")
            if int(polish) > 0:
                raise ValueError("objectives: EHVI's gradient is not built: no polish with two objectives")
            if tree:
                raise ValueError("objectives: EHVI needs the GP's joint posterior: not with a tree surrogate")
            if shared is None and _cons_setting(constraints):
                raise ValueError("objectives: constrained EHVI is not built: no constraints with two objectives")
            if shared is None and _feas_setting(feasibility) is not None:
                raise ValueError("objectives: EHVI under the failure vote is not built: no feasibility with two "
                                 "objectives")
        # diversify = D > 0: a round with a GP takes the D best-scoring candidates
        # as a shortlist and picks its `batch` from them with ut_gp_select_batch,
        # each pick conditioned on the picks before it, so that a batch drawn
        # around one population is not `batch` neighbours; 0 = the plain top-k
        self.diversify = int(diversify)
        if self.diversify:
            if not int(batch) <= self.diversify <= 4096:
                raise ValueError("diversify must be 0 or in [batch, 4096]")
            if int(prune_rows) > 0:
                raise ValueError("diversify needs every candidate's score: not with prune_rows")
            if tree:
                raise ValueError("diversify conditions a GP posterior: not with a tree surrogate")
        # polish = T > 0: a dense GP round refines its polish_pool best-scoring
        # candidates with T steps of projected gradient ascent on the acquisition
        # (ut_gp_polish) before it takes its batch from them -- the local search
        # that the reference's default bandit has in its RandomNelderMead arm
        # (bandittechniques.py:273-278); 0 = today's path, untouched
        self.polish = int(polish)
        self.polish_pool = max(4 * int(batch), 64) if polish_pool is None else int(polish_pool)
        if self.polish < 0:
            raise ValueError("polish must be >= 0")
        if self.polish:
            if not int(batch) <= self.polish_pool <= 4096:
                raise ValueError("polish_pool must be in [batch, 4096]")
            if int(prune_rows) > 0:
                raise ValueError("polish needs every candidate's score: not with prune_rows")
            if tree:
                raise ValueError("polish climbs a GP's acquisition: not with a tree surrogate")
            if shared.constraints if shared is not None else _cons_setting(constraints):
                raise ValueError("the gradient of the constrained score is not built: no polish with constraints")
            if (shared.feasibility if shared is not None else _feas_setting(feasibility)) is not None:
                raise ValueError("the gradient of the weighted score is not built: no polish with feasibility")
        # acq="ts": Thompson sampling.  A dense GP round draws `batch` sample paths
        # of the posterior over the whole pool (ut_gp_ts_draw, ts_features random
        # Fourier features, keyed by a counter on the shared model so that no two
        # draws on one model share a key) and slot s takes path s's minimiser among
        # the candidates no earlier slot took (ut_gp_ts_select): TuRBO's
        # acquisition, whose batches are diverse without a second mechanism.  The
        # reported score of a pick is -f_s there.  Off by default
        self.ts_features = int(ts_features)
        if acq == "ts":
            if not (128 <= self.ts_features <= 4096 and self.ts_features % 128 == 0):
                raise ValueError("ts_features must be a multiple of 128 in [128, 4096]")
            if not 1 <= int(batch) <= 256:
                raise ValueError("acq='ts' draws one path per batch slot: batch must be in [1, 256]")
            if int(prune_rows) > 0:
                raise ValueError("acq='ts' evaluates its paths at every candidate: not with prune_rows")
            if self.diversify:
                raise ValueError("acq='ts' spreads its batch by its own paths: not with diversify")
            if self.polish:
                raise ValueError("a sample path has no acquisition gradient built: no polish with acq='ts'")
            if shared.constraints if shared is not None else _cons_setting(constraints):
                raise ValueError("paths under constraints are not built: no constraints with acq='ts'")
            if (shared.feasibility if shared is not None else _feas_setting(feasibility)) is not None:
                raise ValueError("paths under the failure vote are not built: no feasibility with acq='ts'")
            if tree:
                raise ValueError("acq='ts' samples a GP posterior: not with a tree surrogate")
        # prune_rows > 0: score rounds with ut_gp_topk_pruned (selection-exact EI
        # bound from the first prune_rows rows of L^-1 k*; fp64 fits, EI / UCB):
        # the same selections as the dense variance at a fraction of its cost
        # when the bounds are tight (or the GP is flat: exact ties by index)
        self.prune_rows = int(prune_rows)
        if refit and self.prune_rows > 0:
            raise ValueError("prune_rows bounds a GP posterior: not with a tree surrogate")
        # surrogate: None = the GP fitted on the driver's results (EI / UCB); or a
        # tree ensemble over the same features (sklearn regressor, XGBoost JSON,
        # forest.Forest) ranking candidates by predicted objective (minimised),
        # the multi-stage tuner's model scoring (multi_stage.py:8-22, :109-123);
        # or "forest": the model's own refitted random forest (above)
        self.surrogate = "forest" if refit else surrogate
        self._static = tree and not refit    # a fixed model object: no fit, mean ranking
        # precision: the GP contractions of a private model (64 / 32 / 16 = f16x3);
        # a shared model (the bandit's) carries its own
        self.model = shared if shared is not None else SharedModel(device=device, seed=seed,
                                                                   lengthscale=lengthscale, min_train=min_train,
                                                                   precision=precision,
                                                                   engine_factory=engine_factory,
                                                                   y_transform=y_transform,
                                                                   feasibility=feasibility,
                                                                   constraints=constraints,
                                                                   prune_weighted=prune_weighted,
                                                                   surrogate="forest" if refit else None,
                                                                   forest_kw=forest_kw, objectives=objectives,
                                                                   ref_point=ref_point)
        # multi-GPU: with torch.distributed initialised and
        # world > 1, rank r scores candidates [base + r*pool, base + (r+1)*pool)
        # of every round and the local top-k lists are all-gathered and merged
        self.group = group
        self.pool, self.batch, self.population = int(pool), int(batch), int(population)
        self.acq_kind = acq
        self.queue: List[Any] = []      # (config dict, hash hex) of the last round's selections
        self.round = 0
        self.cand_base = 0
        self._initialised = False

    def __deepcopy__(self, memo):
        # the process group is shared, never copied; the model drops its device state
        cls = self.__class__
        new = cls.__new__(cls)
        memo[id(self)] = new
        for k, v in self.__dict__.items():
            setattr(new, k, v if k == "group" else copy.deepcopy(v, memo))
        new._initialised = False
        return new

    @property
    def engine(self):
        return self.model.engine

    def _dist(self):
        """(rank, world) of the sharded round (world 1 without torch.distributed)"""
        try:
            import torch.distributed as dist
        except Exception:  # pragma: no cover
            return 0, 1
        if not dist.is_available() or not dist.is_initialized():
            return 0, 1
        return dist.get_rank(self.group), dist.get_world_size(self.group)

    def round_base(self) -> int:
        """global index of this rank's first candidate of the current round"""
        rank, _ = self._dist()
        return self.cand_base + (rank * self.pool if self.sharded else 0)

    # -- device state ------------------------------------------------------
    def _ensure_engine(self):
        eng = self.model.engine_for(self)
        if not self._initialised:
            self.init_population()
            self._initialised = True
        return eng

    def init_population(self):
        self.engine.population_init(max(self.population, 4), round_=0)

    def propose(self, m: int):
        """-> (values [P][m] device tensor, invalid mask or None)"""
        raise NotImplementedError

    def hash_proposals(self, vals, base):
        """hash_config of this round's proposals"""
        return self.engine.hash(vals)

    def best_row(self):
        """driver.best_result's configuration as a SoA value row, or None"""
        b = self.driver.best_result
        return None if b is None else self.engine.spec.encode_configs([b.configuration.data])[:, 0]

    def _local_round(self):
        """this rank's shard: propose -> hash -> dedup -> score -> local top-k"""
        import torch
        eng = self._ensure_engine()
        self.model.sync_history(self.driver)
        # the fit first: its new training rows are encoded through the device
        # (one host round trip) while the queue is still empty.  Pruned scoring
        # needs the whole fit before its K*, so the round's stages queue behind
        # it (ut_gp_join_fit): the fit's chain of small kernels runs alone
        # instead of starving beside the hash, and no host wait sits between the
        # hash and the fit (the proposals never read the GP).  Dense fp64 rounds
        # keep the fit beside their K* (only the variance GEMM waits for it).
        have_model = not self._static and self.model.fit(self.driver)
        if have_model and self.prune_rows > 0 and self.model.precision == 64:
            eng.gp_join_fit()
        base = self.round_base()
        vals, invalid = self.propose(self.pool)
        dig = self.hash_proposals(vals, base)
        dup = eng.dedup(dig)
        if invalid is not None:
            dup = torch.maximum(dup, invalid)
        if self._static:
            if getattr(eng, "forest", None) is None:
                eng.forest_set(self.surrogate)
            _, score = eng.forest_predict(eng.encode(vals), dup=dup)
        elif have_model and self.model.surrogate == "forest":
            _, _, score = eng.forest_score(eng.encode(vals), eng.acq(self.acq_kind), self.model.f_best, dup=dup)
        elif have_model:
            if self.prune_rows > 0 and self.model.precision == 64:
                idx, top, _ = eng.gp_topk_pruned(eng.encode(vals), self.batch, acq=eng.acq(self.acq_kind), dup=dup,
                                                 cand_base=base, bound_rows=self.prune_rows)
                loc = torch.where(idx >= 0, idx - base, torch.zeros_like(idx))
                return vals, idx, top, dig[loc], vals[:, loc]
            if self.acq_kind == "ts":
                return self._ts_picks(vals, dup, dig, base)
            # encoding fused into the K* operand pass (no feature matrix)
            _, _, score = eng.gp_score_values(vals, acq=eng.acq(self.acq_kind), dup=dup)
            if self.polish > 0:
                return self._polished_picks(vals, score, dup, dig, base)
            if self.diversify > 0:
                return self._diverse_picks(vals, score, dup, dig, base)
        else:  # no model yet: every non-duplicate candidate is equally good (lowest index first)
            score = torch.zeros(vals.shape[1], dtype=torch.float64, device=vals.device)
        idx, top = eng.topk(score, self.batch, dup=dup, cand_base=base)   # GLOBAL candidate indices
        loc = torch.where(idx >= 0, idx - base, torch.zeros_like(idx))
        return vals, idx, top, dig[loc], vals[:, loc]

    def _ts_picks(self, vals, dup, dig, base):
        """the round's selections by Thompson sampling: one posterior sample path
        per batch slot, each slot its path's minimiser among the candidates that
        are new and that no earlier slot took (BatchEngine.gp_ts_draw /
        gp_ts_select); what _local_round returns, in pick order"""
        import torch
        eng = self.engine
        k = min(self.batch, vals.shape[1])
        eng.gp_ts_draw(k, self.ts_features, round_=self.model.next_ts_round())
        pos, f = eng.gp_ts_select(vals, k, dup=dup)
        loc = torch.where(pos >= 0, pos, torch.zeros_like(pos))
        idx = torch.where(pos >= 0, loc + base, torch.full_like(pos, -1))
        return vals, idx, -f, dig[loc], vals[:, loc]

    def _diverse_picks(self, vals, score, dup, dig, base):
        """the round's selections from the `diversify` best-scoring candidates,
        each conditioned on the picks before it (BatchEngine.gp_select_batch);
        what _local_round returns, in pick order"""
        import torch
        eng = self.engine
        D = min(self.diversify, vals.shape[1])
        sidx, _ = eng.topk(score, D, dup=dup, cand_base=0)       # local positions, -1 = none
        none = sidx < 0
        sloc = torch.where(none, torch.zeros_like(sidx), sidx)
        pos, top, _ = eng.gp_select_batch(vals[:, sloc].contiguous(), min(self.batch, D), acq=eng.acq(self.acq_kind),
                                          dup=none.to(torch.uint8))
        loc = sloc[torch.where(pos >= 0, pos, torch.zeros_like(pos))]
        idx = torch.where(pos >= 0, loc + base, torch.full_like(pos, -1))
        return vals, idx, top, dig[loc], vals[:, loc]

    def _polished_picks(self, vals, score, dup, dig, base):
        """the round's selections from the polish_pool best-scoring candidates
        after `polish` ascent steps on each (BatchEngine.gp_polish); what
        _local_round returns.  A pick keeps the global index of the shortlist
        entry it descends from; its row, digest and score are the final ones."""
        import torch
        eng = self.engine
        acq = eng.acq(self.acq_kind)
        D = min(self.polish_pool, vals.shape[1])
        sidx, _ = eng.topk(score, D, dup=dup, cand_base=0)       # local positions, -1 = none
        none = sidx < 0
        sloc = torch.where(none, torch.zeros_like(sidx), sidx)
        short, sdig = vals[:, sloc].contiguous(), dig[sloc]
        rows, fscore, score0, moved = eng.gp_polish(short, self.polish, acq=acq, dup=none.to(torch.uint8))
        pdig = eng.hash(rows)
        # a moved entry that landed on a configuration already seen (or on an
        # earlier entry's row) goes back to where it came from
        back = (moved != 0) & (eng.dedup(pdig) != 0)
        rows = torch.where(back[None, :], short, rows)
        fscore = torch.where(back, score0, fscore)
        fdig = torch.where(back[:, None], sdig, pdig)
        out = torch.maximum(eng.dedup(fdig), none.to(torch.uint8))   # what is still a repeat is left out
        k = min(self.batch, D)
        if self.diversify > 0:   # polishing pulls neighbours onto one hill; conditioning spreads them again
            pos, top, _ = eng.gp_select_batch(rows, k, acq=acq, dup=out)
        else:
            pos, top = eng.topk(fscore, k, dup=out, cand_base=0)
        at = torch.where(pos >= 0, pos, torch.zeros_like(pos))
        idx = torch.where(pos >= 0, sloc[at] + base, torch.full_like(pos, -1))
        return vals, idx, top, fdig[at], rows[:, at]

    def _round(self):
        from .engine import digests_to_hex
        rank, world = self._dist()
        if self.polish > 0 and world > 1 and self.sharded:
            raise ValueError("polish is not built for sharded rounds over several ranks")
        if self.acq_kind == "ts" and world > 1 and self.sharded:
            raise ValueError("acq='ts' is not built for sharded rounds over several ranks")
        if self.diversify > 0 and world > 1 and self.sharded:
            # (every rank holds the same setting: all raise together, before any collective)
            raise ValueError("diversify is not built for sharded rounds over several ranks")
        if world > 1 and self.sharded:
            # a failure on any rank must not leave the others inside the
            # all-gather: agree first, then all proceed or all give up
            from .driver import agree
            err = None
            try:
                vals, idx, top, dig, rows = self._local_round()
            except Exception as ex:   # noqa: BLE001 -- re-raised below on every rank
                err = ex
            # the vote travels on the technique's GPU whether or not the round
            # failed (a failed rank must use the same communicator as the others)
            import torch
            dev = idx.device if err is None else torch.device("cuda", self.model.device)
            if not agree(err is None, self.group, dev):
                raise RuntimeError(f"{self.name}: scoring round failed on "
                                   f"{'this rank: ' + repr(err) if err is not None else 'another rank'}")
            from .dist import allgather_selection
            idx, top, rows, dig = allgather_selection(idx, top, dig, rows, self.batch, group=self.group,
                                                      with_digests=True)
        else:
            vals, idx, top, dig, rows = self._local_round()
        import torch
        eng = self.engine
        # the selections (and, for the GP's next fit, their features) reach the
        # host in ONE copy: global indices, value rows, digests, features
        feat = None if self._static else eng.encode(rows)
        parts = [idx.contiguous().view(torch.float64), rows.contiguous().reshape(-1),
                 dig.to(torch.int32).contiguous().view(torch.float64).reshape(-1)]
        if feat is not None:
            parts.append(feat.contiguous().reshape(-1))
        host = torch.cat(parts).cpu().numpy()
        k, ncol = idx.numel(), rows.shape[0]
        o1, o2 = k + ncol * k, k + ncol * k + 4 * k
        keep = host[:k].view(np.int64) >= 0
        idx_h = host[:k].view(np.int64)[keep]
        rows_h = host[k:o1].reshape(ncol, k)[:, keep]
        hexes = digests_to_hex(host[o1:o2].view(np.int32).reshape(k, 8)[keep])
        cfgs = eng.spec.decode_values(rows_h)
        self.queue.extend(zip(cfgs, hexes))
        self.model.note_selections(hexes)
        if feat is not None:
            # a result's features are what features_host(config) encodes: keep
            # those of selections whose config re-encodes to the same value
            # bits (always, unless a value has two encodings, e.g. an enum
            # option listed twice)
            same = (eng.spec.encode_configs(cfgs).view(np.int64) == rows_h.view(np.int64)).all(axis=0)
            ft = host[o2:].reshape(-1, k)[:, keep].T
            self.model.remember_features([h for h, s in zip(hexes, same) if s], ft[same])
        self.after_round(idx_h, hexes)
        self.round += 1
        self.cand_base += (world if self.sharded else 1) * self.pool

    def after_round(self, idx, hexes):
        pass

    def desired_configuration(self):
        try:
            if not self.queue:
                self._round()
            if not self.queue:
                return None
            cfg, hx = self.queue.pop(0)
            # the digest is already known: an in-memory driver interns it as is
            # (no second hash); the reference driver hashes the dict itself
            intern = getattr(self.driver, "configuration_from_digest", None)
            return intern(cfg, hx) if intern is not None else cfg
        except Exception as ex:  # never raise into the driver loop
            log.warning("%s: device round failed: %s", self.name, ex)
            return None


class GpuDifferentialEvolution(GpuBatchTechnique):
    """Batched DifferentialEvolution(Alt) (differentialevolution.py:29-151):
    every round proposes DE/rand/1/bin trials for the population, with the
    driver's best config in the donor pool (information sharing, :112-116);
    an evaluated trial replaces its target when better (handle_requested_result,
    :131-139)."""

    def __init__(self, cr: float = 0.2, n_cross: int = 1, information_sharing: int = 1, *pargs, **kwargs):
        super().__init__(*pargs, **kwargs)
        self.cr, self.n_cross, self.information_sharing = cr, n_cross, information_sharing
        self._pending: Dict[str, int] = {}       # trial digest -> target member
        self._pop_results: Dict[int, Any] = {}   # member -> its Result (PopulationMember.config)

    def propose(self, m):
        return self.engine.propose_de(m, round_=self.round, cand_base=self.round_base(), cr=self.cr,
                                      n_cross=self.n_cross, best=self.best_row(),
                                      information_sharing=self.information_sharing), None

    def hash_proposals(self, vals, base):
        # trials keep most of their target's values: reuse its inner digests
        return self.engine.hash_de(vals, base)

    def after_round(self, idx, hexes):
        npop = self.engine.npop
        for g, hx in zip(np.asarray(idx).tolist(), hexes):   # global index g targets member g % npop
            self._pending[hx] = g % npop

    def handle_requested_result(self, result):
        import torch
        tgt = self._pending.pop(result.configuration.hash, None)
        if tgt is None or self.engine is None:
            return
        parent = self._pop_results.get(tgt)
        if parent is None or self.objective.lt(result, parent):
            eng = self.model.engine_for(self)
            vals = torch.from_numpy(eng.spec.encode_configs([result.configuration.data])).to(eng.device)
            eng.population_replace(vals, torch.tensor([tgt], device=eng.device))
            self._pop_results[tgt] = result


class GpuPSO(GpuBatchTechnique):
    """Batched PSO (pso.py:11-77); particles move toward the driver's best."""

    sharded = False   # the swarm moves on every rank: same particles, same result

    def __init__(self, omega=0.5, phi_l=0.5, phi_g=0.5, enum_mode=0, crossover="op3_cross_OX1", *pargs, **kwargs):
        super().__init__(*pargs, **kwargs)
        self.omega, self.phi_l, self.phi_g, self.enum_mode = omega, phi_l, phi_g, enum_mode
        self.crossover = crossover   # PSO(crossover=...) for permutation params (pso.py:80-84)

    def init_population(self):
        super().init_population()
        self.engine.pso_reset()

    def propose(self, m):
        gb = self.best_row()
        if gb is None:  # no result yet: particle 0 stands in for the global best
            gb = self.engine.population_get()[:, 0]
        npop = self.engine.npop
        x, v = self.engine.propose_pso(gb, min(m, npop), round_=self.round, cand_base=0, omega=self.omega,
                                       phi_l=self.phi_l, phi_g=self.phi_g, enum_mode=self.enum_mode,
                                       crossover=self.crossover)
        self.engine.pso_commit(x, v, cand_base=0)   # HybridParticle.move mutates the particle in place
        return x, None


class GpuGA(GpuBatchTechnique):
    """Batched UniformGreedyMutation / NormalGreedyMutation / GA
    (evolutionarytechniques.py:13-158)."""

    def __init__(self, mutation_rate=0.1, crossover_rate=0.0, must_mutate_count=1, normal=False, sigma=0.1,
                 crossover_strength=0.0, op=4, crossover=None, *pargs, **kwargs):
        super().__init__(*pargs, **kwargs)
        # crossover: GA(crossover='op3_cross_OX3', ...) -- applied to permutation
        # params of size > 6 when two parents are selected (:117-134, :144-148)
        self.ga = dict(mutation_rate=mutation_rate, crossover_rate=crossover_rate,
                       must_mutate_count=must_mutate_count, normal=normal, sigma=sigma,
                       crossover_strength=crossover_strength, op=op, crossover=crossover)

    def propose(self, m):
        # GreedySelectionMixin.select: the global best config (random() before any result)
        self._parent = self.best_row()
        return self.engine.propose_ga(m, self._parent, None, round_=self.round, cand_base=self.round_base(), **self.ga)

    def hash_proposals(self, vals, base):
        # children keep most of the parent's values: reuse its inner digests
        parent = getattr(self, "_parent", None)
        hp = getattr(self.engine, "hash_parent", None)
        if parent is None or hp is None:
            return self.engine.hash(vals)
        return hp(vals, parent)


class GpuGGA(GpuGA):
    """globalGA.NormalGreedyMutation(crossover_rate=0.5, crossover_strength=0.2) (globalGA.py:129)"""

    def __init__(self, *pargs, **kwargs):
        kwargs.setdefault("mutation_rate", 0.1)
        super().__init__(*pargs, crossover_rate=0.5, crossover_strength=0.2, normal=True, op=5, **kwargs)


class GpuTrustRegion(GpuBatchTechnique):
    """Trust-region proposals (TuRBO-1, Eriksson et al. 2019): every round draws
    its pool inside a box around one centre (ut_propose_tr), sized by the outcome
    of the rounds before it (trust_region.TrustRegion) and shaped by the GP's
    per-feature lengthscales; the shared surrogate scores the pool as it does
    any other.  Off by default everywhere: trust_region=True on the bandits adds
    it as an arm.

    centre="best": the box sits on the driver's best result; a round succeeds
    when one of its own evaluated requests beat the best at proposal time.
    centre="own": the centre is the best result of this technique's own
    requests since its last restart; with none yet (the first round, the round
    after a restart) the round is uniform random rows scored by the model, and
    its best result becomes the centre.  Before any result exists both modes
    take that uniform round.  A round is judged when the next one starts, from
    the results that have arrived by then."""

    def __init__(self, centre: str = "best", L_init: float = 0.8, L_min: float = 2.0 ** -7, L_max: float = 1.6,
                 succ_tol: int = 3, fail_tol: Optional[int] = None, must: int = 1, *pargs, **kwargs):
        super().__init__(*pargs, **kwargs)
        if centre not in ("best", "own"):
            raise ValueError("centre must be 'best' or 'own'")
        self.centre_mode = centre
        self.must = int(must)
        self._tr_kw = dict(L_init=L_init, L_min=L_min, L_max=L_max, succ_tol=succ_tol, fail_tol=fail_tol)
        self.tr = None                           # TrustRegion, once the space is known (init_population)
        self._pending: Dict[str, int] = {}       # request digest -> the round that proposed it
        self._open: Dict[int, Dict[str, Any]] = {}   # rounds not yet judged: ref, improved, uniform
        self._own_best = None                    # centre="own": best Result of the own requests since the restart
        self._since = 0                          # ... the first round after it
        self._parent = None
        self.last_centre = self.last_half = None   # the last box round's centre row and half-widths
        self.last_uniform = False                # the last round was a uniform one

    def init_population(self):
        # no standing population: a uniform round draws its own rows
        from .trust_region import TrustRegion
        from . import _lib as L
        n_move = 0
        for p in self.engine.spec.params:
            if p.kind <= L.UT_POW2:
                n_move += p.lo < p.hi
            elif p.kind == L.UT_BOOL:
                n_move += 1
            else:
                n_move += (p.width if p.kind == L.UT_PERM else len(p.options)) > 1
        if self.tr is None:
            self.tr = TrustRegion(n_move, self.batch, **self._tr_kw)

    def _judge_open_rounds(self):
        for rnd in sorted(self._open):
            st = self._open.pop(rnd)
            if st["uniform"]:
                continue
            if self.tr.judge(st["improved"]) and self.centre_mode == "own":
                self._own_best, self._since = None, self.round   # restart: the next round is uniform

    def _centre_result(self):
        return self._own_best if self.centre_mode == "own" else self.driver.best_result

    def propose(self, m):
        eng = self.engine
        self._judge_open_rounds()
        ref = self._centre_result()
        self._open[self.round] = dict(ref=ref, improved=False, uniform=ref is None)
        self.last_uniform = ref is None
        if ref is None:
            # rows [rank * m, (rank + 1) * m) of one population keyed by (seed, member, round)
            rank, world = self._dist()
            eng.population_init(max(world * m, 4), round_=self.round)
            self._parent = None
            return eng.population_get()[:, rank * m:(rank + 1) * m].contiguous(), None
        centre = eng.spec.encode_configs([ref.configuration.data])[:, 0]
        ell = self.model.lengthscale_
        half = self.tr.half_widths(eng.spec, 1.0 if ell is None else ell)
        prob, cat_prob = self.tr.probs()
        self.last_centre, self.last_half = centre, half
        self._parent = centre
        return eng.propose_tr(m, centre, half, prob, cat_prob, must=min(self.must, eng.spec.P), round_=self.round,
                              cand_base=self.round_base())

    def hash_proposals(self, vals, base):
        # most columns keep the centre's value: reuse its inner digests
        hp = getattr(self.engine, "hash_parent", None)
        if self._parent is None or hp is None:
            return self.engine.hash(vals)
        return hp(vals, self._parent)

    def after_round(self, idx, hexes):
        for hx in hexes:
            self._pending[hx] = self.round

    def handle_requested_result(self, result):
        rnd = self._pending.pop(result.configuration.hash, None)
        if rnd is None:
            return
        st = self._open.get(rnd)
        if st is not None and (st["ref"] is None or self.objective.lt(result, st["ref"])):
            st["improved"] = True
        if self.centre_mode == "own" and rnd >= self._since and (
                self._own_best is None or self.objective.lt(result, self._own_best)):
            self._own_best = result


def _shared_model(kw) -> SharedModel:
    return SharedModel(device=kw.get("device", 0), seed=kw.get("seed", 0), lengthscale=kw.get("lengthscale", 0.3),
                       min_train=kw.get("min_train", 4), precision=kw.get("precision", 64),
                       engine_factory=kw.pop("engine_factory", None), y_transform=kw.get("y_transform"),
                       feasibility=kw.get("feasibility", False), constraints=kw.get("constraints"),
                       prune_weighted=kw.get("prune_weighted", False),
                       surrogate="forest" if isinstance(kw.get("surrogate"), str) and kw["surrogate"] == "forest"
                       else None, forest_kw=kw.get("forest_kw"), objectives=kw.get("objectives"),
                       ref_point=kw.get("ref_point"))


def _tr_arm(on: bool, shared: SharedModel, kw) -> List[SearchTechniqueBase]:
    """the bandits' opt-in trust-region arm (trust_region=True)"""
    return [GpuTrustRegion(name="gpu-trust-region", shared=shared, **kw)] if on else []


def pso_ga_de_bandit(bandit_seed: Optional[int] = None, **kw) -> AUCBanditMetaTechnique:
    """GPU counterpart of the reference's "PSO_GA_DE" bandit (bandittechniques.py:311-320):
    the four techniques share ONE SharedModel (one device context: one GP fit
    per generation, one dedup set) with a population slot each.  bandit_seed
    fixes the bandit's tie-break shuffles (required for SPMD runs: every rank
    must order the techniques the same way).  trust_region=True adds a
    GpuTrustRegion arm on the same model."""
    kw = dict(kw)
    tr = bool(kw.pop("trust_region", False))
    shared = kw.pop("shared", None) or _shared_model(kw)
    return AUCBanditMetaTechnique([
        GpuPSO(name="gpu-pso", shared=shared, **kw),
        GpuGA(name="gpu-ga", crossover_rate=0.5, shared=shared, **kw),
        GpuDifferentialEvolution(name="gpu-de", shared=shared, **kw),
        GpuGGA(name="gpu-gga", shared=shared, **kw),
    ] + _tr_arm(tr, shared, kw), name="GPU_PSO_GA_DE", seed=bandit_seed)


def bandit_a(bandit_seed: Optional[int] = None, **kw) -> AUCBanditMetaTechnique:
    """GPU counterpart of the reference's default root technique,
    "AUCBanditMetaTechniqueA" (bandittechniques.py:273-278; technique.py:349):
    DifferentialEvolutionAlt (cr 0.2), UniformGreedyMutation (mutation rate
    0.1, evolutionarytechniques.py:13-24) and NormalGreedyMutation(mutation_rate
    =0.3) on one shared model.  The fourth child, RandomNelderMead, is a
    sequential simplex technique outside the scoring path (DESIGN.md "Out of
    scope") and is not built; polish=T (GpuBatchTechnique) is the local search
    that stands in for it.  trust_region=True adds a GpuTrustRegion arm, a local
    search that stays batch-parallel, in that fourth slot."""
    kw = dict(kw)
    tr = bool(kw.pop("trust_region", False))
    shared = kw.pop("shared", None) or _shared_model(kw)
    return AUCBanditMetaTechnique([
        GpuDifferentialEvolution(name="gpu-de-alt", cr=0.2, shared=shared, **kw),
        GpuGA(name="gpu-uniform-greedy-mutation", mutation_rate=0.1, shared=shared, **kw),
        GpuGA(name="gpu-normal-greedy-mutation", mutation_rate=0.3, normal=True, shared=shared, **kw),
    ] + _tr_arm(tr, shared, kw), name="GpuAUCBanditMetaTechniqueA", seed=bandit_seed)


def bandit_b(bandit_seed: Optional[int] = None, **kw) -> AUCBanditMetaTechnique:
    """"AUCBanditMetaTechniqueB" (bandittechniques.py:279-282): DifferentialEvolutionAlt
    and UniformGreedyMutation on one shared model (trust_region=True: and a
    GpuTrustRegion arm)"""
    kw = dict(kw)
    tr = bool(kw.pop("trust_region", False))
    shared = kw.pop("shared", None) or _shared_model(kw)
    return AUCBanditMetaTechnique([
        GpuDifferentialEvolution(name="gpu-de-alt", cr=0.2, shared=shared, **kw),
        GpuGA(name="gpu-uniform-greedy-mutation", mutation_rate=0.1, shared=shared, **kw),
    ] + _tr_arm(tr, shared, kw), name="GpuAUCBanditMetaTechniqueB", seed=bandit_seed)


_XO = ("op3_cross_OX3", "op3_cross_OX1", "op3_cross_PMX", "op3_cross_PX", "op3_cross_CX")


def reference_registry(wrap=None, bandit_cls=None, **kw) -> List[SearchTechniqueBase]:
    """GPU counterparts of the population techniques the reference registers,
    same parameters, names prefixed "Gpu" (crossover variants suffixed, since
    the reference registers all five PSO / GA variants under one class name):

      DifferentialEvolution (cr 0.9), DifferentialEvolutionAlt (cr 0.2),
      DifferentialEvolution_20_100      differentialevolution.py:148-151
      PSO(crossover=OX3|OX1|PMX|PX|CX)  pso.py:80-84
      GA(crossover=..., mutation 0.1, crossover rate 0.8)
                                        evolutionarytechniques.py:146-150
      ga-base, UniformGreedyMutation05/10/20, NormalGreedyMutation05/10/20
                                        evolutionarytechniques.py:151-158
      GGA                               globalGA.py:129
      PSO_GA_DE bandit                  bandittechniques.py:311-320
      AUCBanditMetaTechniqueA / B       bandittechniques.py:273-282 (A without
                                        RandomNelderMead: see bandit_a)

    `wrap(cls)` maps each GPU technique class before construction (the
    reference-side binding rebases them onto its SearchTechnique)
    and `bandit_cls` replaces this module's AUCBanditMetaTechnique for the
    bandit.  `kw` goes to every technique (pool, batch, device, seed, ...).  The
    DE population size is the device population (`population=`), not 30 / 100:
    every member is scored each round.  trust_region=True appends a stand-alone
    GpuTrustRegion (an addition of this library: the reference has none)."""
    W = wrap or (lambda c: c)
    kw = dict(kw)
    tr = bool(kw.pop("trust_region", False))
    ef = kw.get("engine_factory")
    sm = _shared_model(kw)          # the bandit's children share one model (pops engine_factory; every
    #                                 technique, stand-alone or not, gets the requested precision)
    if ef is not None:
        kw["engine_factory"] = ef   # ... while each stand-alone technique builds its own
    DE, PSO, GA, GGA = W(GpuDifferentialEvolution), W(GpuPSO), W(GpuGA), W(GpuGGA)
    out: List[SearchTechniqueBase] = [
        DE(name="GpuDifferentialEvolution", cr=0.9, **kw),
        DE(name="GpuDifferentialEvolutionAlt", cr=0.2, **kw),
        DE(name="GpuDifferentialEvolution_20_100", cr=0.2, **kw),
    ]
    for xo in _XO:
        out.append(PSO(name="GpuPSO-" + xo[len("op3_cross_"):], crossover=xo, **kw))
    for xo in _XO:
        out.append(GA(name="GpuGA-" + xo[len("op3_cross_"):], crossover=xo, mutation_rate=0.10, crossover_rate=0.8,
                      **kw))
    out.append(GA(name="Gpuga-base", mutation_rate=0.10, **kw))
    for r in (5, 10, 20):
        out.append(GA(name="GpuUniformGreedyMutation%02d" % r, mutation_rate=r / 100.0, **kw))
    for r in (5, 10, 20):
        out.append(GA(name="GpuNormalGreedyMutation%02d" % r, mutation_rate=r / 100.0, normal=True, **kw))
    out.append(GGA(name="GpuGGA", **kw))
    children = [PSO(name="gpu-pso", shared=sm, **kw), GA(name="gpu-ga", crossover_rate=0.5, shared=sm, **kw),
                DE(name="gpu-de", shared=sm, **kw), GGA(name="gpu-gga", shared=sm, **kw)]
    out.append((bandit_cls or AUCBanditMetaTechnique)(children, name="GPU_PSO_GA_DE"))
    # AUCBanditMetaTechniqueA / B, each with a model of its own
    sa, sb = _shared_model(dict(kw)), _shared_model(dict(kw))
    for nm, kids in (("GpuAUCBanditMetaTechniqueA",
                      [DE(name="gpu-de-alt", cr=0.2, shared=sa, **kw),
                       GA(name="gpu-uniform-greedy-mutation", mutation_rate=0.1, shared=sa, **kw),
                       GA(name="gpu-normal-greedy-mutation", mutation_rate=0.3, normal=True, shared=sa, **kw)]),
                     ("GpuAUCBanditMetaTechniqueB",
                      [DE(name="gpu-de-alt", cr=0.2, shared=sb, **kw),
                       GA(name="gpu-uniform-greedy-mutation", mutation_rate=0.1, shared=sb, **kw)])):
        out.append((bandit_cls or AUCBanditMetaTechnique)(kids, name=nm))
    if tr:
        out.append(W(GpuTrustRegion)(name="GpuTrustRegion", **kw))
    return out
