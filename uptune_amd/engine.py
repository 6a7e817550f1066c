"""BatchEngine: the Python face of libuthot.so.

Owns one ut_ctx (one GPU, one HIP stream = torch's current stream on that
device, so library kernels and torch.distributed collectives are ordered on
the same queue).  All large arrays are torch tensors resident in HBM; only
their data pointers cross the C ABI.
"""
from __future__ import annotations

import ctypes as C
from typing import Any, Dict, List, Optional, Sequence, Tuple

import numpy as np
import torch

from . import _lib as L
from .manipulator import SpaceSpec, compile_space, to_descs


def _ptr(t: Optional[torch.Tensor]):
    return None if t is None else C.c_void_p(t.data_ptr())


def digests_to_hex(d: torch.Tensor | np.ndarray) -> List[str]:
    """[n][8] big-endian uint32 words (as int32/uint32) -> hexdigest strings"""
    a = d.cpu().numpy() if isinstance(d, torch.Tensor) else np.asarray(d)
    a = a.view(np.uint32).astype(">u4")
    return [row.tobytes().hex() for row in a]


def hex_to_digests(hexes: Sequence[str]) -> np.ndarray:
    """hexdigest strings -> [n][8] uint32 (big-endian word values)"""
    if not hexes:
        return np.zeros((0, 8), dtype=np.uint32)
    raw = np.frombuffer(b"".join(bytes.fromhex(h) for h in hexes), dtype=">u4").reshape(-1, 8)
    return raw.astype(np.uint32)


def _xop(name) -> int:
    if name is None:
        return L.UT_X_NONE
    if isinstance(name, int):
        return name
    if name not in L.CROSSOVERS:
        raise ValueError(f"unknown permutation crossover {name!r} (one of {sorted(L.CROSSOVERS)})")
    return L.CROSSOVERS[name]


class BatchEngine:
    """One device context over one search space."""

    def __init__(self, space, device: int = 0, seed: int = 0, py2_layout: bool = False):
        self.lib = L.lib()
        if not torch.cuda.is_available():
            raise L.UthotError("uptune_amd.BatchEngine needs a ROCm GPU (torch.cuda.is_available() is False)")
        self.device = torch.device("cuda", device)
        self.seed = int(seed)
        self.spec: SpaceSpec = space if isinstance(space, SpaceSpec) else compile_space(space)
        ctx = C.c_void_p()
        torch.cuda.set_device(self.device)
        L.check(None, self.lib.ut_ctx_create(device, self.seed, C.byref(ctx)), "ut_ctx_create")
        self.ctx = ctx
        self._bind_stream()
        descs, keep = to_descs(self.spec)
        L.check(self.ctx, self.lib.ut_space_define(self.ctx, self.spec.P, descs, 1 if py2_layout else 0),
                "ut_space_define")
        del keep
        self.npop = 0
        self.slot = 0
        self._slot_npop: Dict[int, int] = {}
        self.forest = None

    # -- plumbing ----------------------------------------------------------
    def _bind_stream(self):
        s = torch.cuda.current_stream(self.device)
        self._stream = s
        L.check(self.ctx, self.lib.ut_set_stream(self.ctx, C.c_void_p(s.cuda_stream)), "ut_set_stream")

    def close(self):
        if getattr(self, "ctx", None):
            self.lib.ut_ctx_destroy(self.ctx)
            self.ctx = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass

    def __deepcopy__(self, memo):
        # techniques are deepcopied per SearchDriver (driver.py:75); a device
        # context is never copied -- the copy re-creates it lazily
        return None

    def sync(self):
        L.check(self.ctx, self.lib.ut_sync(self.ctx), "ut_sync")

    def device_bytes(self) -> int:
        """ut_device_bytes: device memory libuthot holds on this engine's GPU in
        this process (every context; one rank per GPU makes it the rank's footprint)"""
        b = C.c_int64()
        L.check(self.ctx, self.lib.ut_device_bytes(self.device.index, C.byref(b)), "ut_device_bytes")
        return int(b.value)

    def space_info(self) -> Tuple[int, int, int]:
        a, b, c = C.c_int64(), C.c_int64(), C.c_int32()
        L.check(self.ctx, self.lib.ut_space_info(self.ctx, C.byref(a), C.byref(b), C.byref(c)), "ut_space_info")
        return a.value, b.value, c.value

    def _empty(self, *shape, dtype=torch.float64) -> torch.Tensor:
        return torch.empty(*shape, dtype=dtype, device=self.device)

    # -- population --------------------------------------------------------
    def population_init(self, npop: int, round_: int = 0):
        L.check(self.ctx, self.lib.ut_population_init(self.ctx, int(npop), int(round_)), "ut_population_init")
        self.npop = int(npop)

    def population_set(self, values: torch.Tensor):
        values = values.to(self.device, torch.float64).contiguous()
        n = values.shape[1]
        L.check(self.ctx, self.lib.ut_population_set(self.ctx, n, _ptr(values), n), "ut_population_set")
        self.npop = n

    def population_select(self, slot: int):
        """ut_population_select: later population / PSO calls use slot `slot`"""
        if slot == self.slot:
            return
        L.check(self.ctx, self.lib.ut_population_select(self.ctx, int(slot)), "ut_population_select")
        self._slot_npop[self.slot] = self.npop
        self.slot = int(slot)
        self.npop = self._slot_npop.get(self.slot, 0)

    def population_get(self) -> torch.Tensor:
        out = self._empty(self.spec.ncols, self.npop)
        L.check(self.ctx, self.lib.ut_population_get(self.ctx, _ptr(out), self.npop), "ut_population_get")
        return out

    def population_replace(self, trial: torch.Tensor, idx: torch.Tensor):
        trial = trial.contiguous()
        idx = idx.to(self.device, torch.int64).contiguous()
        L.check(self.ctx, self.lib.ut_population_replace(self.ctx, _ptr(trial), trial.shape[1], _ptr(idx),
                                                         idx.numel()), "ut_population_replace")

    # -- proposal ----------------------------------------------------------
    def _de_params(self, cr, n_cross, best, information_sharing):
        """ut_de_params + the device best row it points to (kept alive by the caller)"""
        b = self._row(best)
        p = L.DeParams(cr=float(cr), n_cross=int(n_cross), information_sharing=int(information_sharing),
                       best=None if b is None else b.data_ptr())
        return p, b

    def propose_de(self, m: int, round_: int = 0, cand_base: int = 0, cr: float = 0.2, n_cross: int = 1,
                   out: Optional[torch.Tensor] = None, best=None, information_sharing: int = 1) -> torch.Tensor:
        """DE trials (differentialevolution.py:105-129); `best` = the driver's
        best config as a value row [ncols] (added `information_sharing` times to
        the donor pool, :112-116), None before the first result."""
        if out is None:
            out = self._empty(self.spec.ncols, m)
        p, keep = self._de_params(cr, n_cross, best, information_sharing)
        L.check(self.ctx, self.lib.ut_propose_de(self.ctx, C.byref(p), int(round_), int(cand_base), int(m),
                                                 _ptr(out), out.stride(0)), "ut_propose_de")
        del keep
        return out

    def pso_reset(self):
        L.check(self.ctx, self.lib.ut_pso_reset(self.ctx), "ut_pso_reset")

    def _row(self, r):
        if r is None:
            return None
        if isinstance(r, torch.Tensor):
            return r.to(self.device, torch.float64).contiguous()
        # through pinned memory, asynchronously on the engine's stream (the
        # library's stream, _bind_stream): a pageable copy would wait for every
        # kernel already queued (the fit, the previous stages) before returning
        h = torch.from_numpy(np.ascontiguousarray(r, dtype=np.float64)).pin_memory()
        with torch.cuda.stream(self._stream):
            return h.to(self.device, non_blocking=True)

    def propose_pso(self, gbest, m: int, round_: int = 0, cand_base: int = 0, omega: float = 0.5,
                    phi_l: float = 0.5, phi_g: float = 0.5, sigma: float = 0.2, alias_pbest: bool = True,
                    enum_mode: int = 0, crossover: str = "op3_cross_OX1"):
        """HybridParticle.move for particles (cand_base + i) % npop (pso.py:70-77);
        `crossover` is PSO(crossover=...) for permutation params (pso.py:80-84)."""
        gb = self._row(gbest)
        x = self._empty(self.spec.ncols, m)
        v = self._empty(self.spec.ncols, m)
        a = L.PsoParams(omega=omega, phi_l=phi_l, phi_g=phi_g, sigma=sigma, alias_pbest=1 if alias_pbest else 0,
                        enum_mode=int(enum_mode), crossover=_xop(crossover))
        L.check(self.ctx, self.lib.ut_propose_pso(self.ctx, C.byref(a), _ptr(gb), int(round_), int(cand_base), int(m),
                                                  _ptr(x), _ptr(v), m), "ut_propose_pso")
        return x, v

    def pso_commit(self, values: torch.Tensor, vel: Optional[torch.Tensor], cand_base: int = 0):
        L.check(self.ctx, self.lib.ut_pso_commit(self.ctx, _ptr(values), _ptr(vel), values.stride(0), int(cand_base),
                                                 values.shape[1]), "ut_pso_commit")

    def propose_ga(self, m: int, parent1=None, parent2=None, round_: int = 0, cand_base: int = 0,
                   mutation_rate: float = 0.1, sigma: float = 0.1, crossover_rate: float = 0.0,
                   crossover_strength: float = 0.0, must_mutate_count: int = 1, normal: bool = False,
                   max_retries: int = 10, op: int = 4, crossover: Optional[str] = None):
        """EvolutionaryTechnique / GGA proposals (evolutionarytechniques.py:29-61,
        globalGA.py:28-48 and :68-76); `crossover` = GA(crossover=...) for permutation
        params (CrossoverMixin, :117-134).  Returns (values [ncols][m], invalid [m])."""
        p1, p2 = self._row(parent1), self._row(parent2)
        out = self._empty(self.spec.ncols, m)
        inv = self._empty(m, dtype=torch.uint8)
        a = L.GaParams(mutation_rate=mutation_rate, sigma=sigma, crossover_rate=crossover_rate,
                       crossover_strength=crossover_strength, must_mutate_count=must_mutate_count,
                       normal=1 if normal else 0, max_retries=max_retries, op=op, crossover=_xop(crossover))
        L.check(self.ctx, self.lib.ut_propose_ga(self.ctx, C.byref(a), _ptr(p1), _ptr(p2), int(round_),
                                                 int(cand_base), int(m), _ptr(out), m, _ptr(inv)), "ut_propose_ga")
        return out, inv

    def propose_tr(self, m: int, centre, half_width, prob: float, cat_prob: Optional[float] = None, must: int = 1,
                   round_: int = 0, cand_base: int = 0):
        """Trust-region proposals (ut_propose_tr): candidates in the box centre +- half_width
        (unit space, one entry per parameter) that move each primitive parameter with
        probability `prob`, each BOOL / ENUM / PERM with `cat_prob` (default: prob), and
        `must` parameters always.  Returns (values [ncols][m], invalid [m])."""
        c = self._row(centre)
        h = np.ascontiguousarray(half_width, dtype=np.float64).reshape(-1)
        if h.size != self.spec.P:
            raise ValueError(f"half_width has {h.size} entries for {self.spec.P} parameters")
        out = self._empty(self.spec.ncols, m)
        inv = self._empty(m, dtype=torch.uint8)
        a = L.TrParams(prob=float(prob), cat_prob=float(prob if cat_prob is None else cat_prob), must=int(must))
        L.check(self.ctx, self.lib.ut_propose_tr(self.ctx, C.byref(a), _ptr(c), C.c_void_p(h.ctypes.data), int(round_),
                                                 int(cand_base), int(m), _ptr(out), m, _ptr(inv)), "ut_propose_tr")
        return out, inv

    def encode(self, values: torch.Tensor, m: Optional[int] = None) -> torch.Tensor:
        m = values.shape[1] if m is None else m
        feat = self._empty(self.spec.n_features, m)
        L.check(self.ctx, self.lib.ut_encode_features(self.ctx, _ptr(values), values.stride(0), m, _ptr(feat), m),
                "ut_encode_features")
        return feat

    def features_host(self, cfgs: Sequence[Dict[Any, Any]]) -> np.ndarray:
        """configs -> GP features [n][F] (host f64), encoded on the device"""
        if not len(cfgs):
            return np.zeros((0, self.spec.n_features))
        vals = torch.from_numpy(self.spec.encode_configs(cfgs)).to(self.device)
        return self.encode(vals).T.contiguous().cpu().numpy()

    # -- identity / dedup --------------------------------------------------
    def hash(self, values: torch.Tensor, m: Optional[int] = None) -> torch.Tensor:
        m = values.shape[1] if m is None else m
        out = self._empty(m, 8, dtype=torch.int32)
        L.check(self.ctx, self.lib.ut_hash(self.ctx, _ptr(values), values.stride(0), m, _ptr(out)), "ut_hash")
        return out

    def hash_de(self, values: torch.Tensor, cand_base: int = 0, m: Optional[int] = None) -> torch.Tensor:
        """ut_hash_de: hash_config of DE trials proposed from the selected
        population with this cand_base, reusing the targets' inner digests"""
        m = values.shape[1] if m is None else m
        out = self._empty(m, 8, dtype=torch.int32)
        L.check(self.ctx, self.lib.ut_hash_de(self.ctx, _ptr(values), values.stride(0), m, int(cand_base), _ptr(out)),
                "ut_hash_de")
        return out

    def hash_parent(self, values: torch.Tensor, parent, m: Optional[int] = None) -> torch.Tensor:
        """ut_hash_parent: hash_config of GA / GGA children of `parent` (a value
        row), reusing the parent's inner digests for the unchanged params"""
        m = values.shape[1] if m is None else m
        p = self._row(parent)
        out = self._empty(m, 8, dtype=torch.int32)
        L.check(self.ctx, self.lib.ut_hash_parent(self.ctx, _ptr(values), values.stride(0), m, _ptr(p), _ptr(out)),
                "ut_hash_parent")
        return out

    def hash_configs(self, cfgs: Sequence[Dict[Any, Any]]) -> List[str]:
        vals = torch.from_numpy(self.spec.encode_configs(cfgs)).to(self.device)
        d = self.hash(vals)
        return digests_to_hex(d)

    def history_reset(self, capacity: int = 0):
        L.check(self.ctx, self.lib.ut_history_reset(self.ctx, int(capacity)), "ut_history_reset")

    def history_add(self, digests):
        if isinstance(digests, torch.Tensor):
            d = digests.to(self.device, torch.int32).contiguous()
            L.check(self.ctx, self.lib.ut_history_add(self.ctx, _ptr(d), d.shape[0]), "ut_history_add")
        else:
            arr = np.ascontiguousarray(hex_to_digests(digests) if len(digests) and isinstance(digests[0], str)
                                       else np.asarray(digests, dtype=np.uint32).reshape(-1, 8))
            L.check(self.ctx, self.lib.ut_history_add_host(self.ctx, arr.ctypes.data, arr.shape[0]),
                    "ut_history_add_host")

    def dedup(self, digests: torch.Tensor) -> torch.Tensor:
        m = digests.shape[0]
        out = self._empty(m, dtype=torch.uint8)
        L.check(self.ctx, self.lib.ut_dedup(self.ctx, _ptr(digests), m, _ptr(out)), "ut_dedup")
        return out

    # -- GP ----------------------------------------------------------------
    def gp_set_precision(self, bits):
        """64 (fp64 MFMA, 1e-5 tier), 32 (fp32 MFMA, 1e-3 tier), 16 / "f16x3"
        (variance contraction as three fp16 MFMA products of hi/lo splits, f32
        accumulate: the 1e-3 tier at the fp16 MFMA rate) or 8 / "i8" (the fp64
        tier on the int8 MFMA: six-digit slices, a per-candidate error bound,
        fp64 recompute of the candidates it does not clear); applies to later fits"""
        bits = {"f16x3": 16, "i8": 8}.get(bits, bits)
        L.check(self.ctx, self.lib.ut_gp_set_precision(self.ctx, int(bits)), "ut_gp_set_precision")

    def gp_set_prune_pass(self, bits: int):
        """gp_topk_pruned's bound pass: 32 (default, f32 k* with bounded rounding) or 64 (fp64)"""
        L.check(self.ctx, self.lib.ut_gp_set_prune_pass(self.ctx, int(bits)), "ut_gp_set_prune_pass")

    def gp_set_prune_weighted(self, on: bool):
        """ut_gp_set_prune_weighted: with True, gp_topk_pruned and
        score_round_de_pruned accept loaded failed rows / constraint values (EI
        only) and select by the dense weighted score; False (default): they
        raise UT_EUNSUPPORTED meanwhile"""
        L.check(self.ctx, self.lib.ut_gp_set_prune_weighted(self.ctx, 1 if on else 0), "ut_gp_set_prune_weighted")

    def gp_set_i8_tol(self, tol: float):
        """precision 8: largest accepted relative variance error (0: recompute all in fp64)"""
        L.check(self.ctx, self.lib.ut_gp_set_i8_tol(self.ctx, float(tol)), "ut_gp_set_i8_tol")

    def gp_i8_stats(self) -> Tuple[int, float]:
        """precision 8: (candidates of the last score recomputed in fp64, -1 = all;
        the fit's error bound E on |L^-1 k* - v^|)"""
        n, e = C.c_int64(), C.c_double()
        L.check(self.ctx, self.lib.ut_gp_i8_stats(self.ctx, C.byref(n), C.byref(e)), "ut_gp_i8_stats")
        return int(n.value), float(e.value)

    def gp_i8_bounds(self) -> Tuple[float, float]:
        """precision 8: the fit's bounds (E on the variance's |L^-1 k* - v^|,
        Emu on the mean from the int8 variance epilogue); 0, 0 otherwise"""
        e, em = C.c_double(), C.c_double()
        L.check(self.ctx, self.lib.ut_gp_i8_bounds(self.ctx, C.byref(e), C.byref(em)), "ut_gp_i8_bounds")
        return float(e.value), float(em.value)

    def gp_fit(self, X: np.ndarray, y: np.ndarray, lengthscale, sigma_f2: float = 1.0, sigma_n2: float = 1e-6,
               jitter: float = 0.0, wait: bool = True):
        """ut_gp_fit (wait=True) or ut_gp_fit_async (wait=False: the fit runs on the
        device beside the next round's proposal/hash stages)"""
        X = np.ascontiguousarray(X, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        n, d = X.shape
        ell = np.ascontiguousarray(np.broadcast_to(np.asarray(lengthscale, dtype=np.float64), (d,)))
        h = L.GpHyper(sigma_f2=float(sigma_f2), sigma_n2=float(sigma_n2), jitter=float(jitter),
                      lengthscale_host=ell.ctypes.data)
        fn = self.lib.ut_gp_fit if wait else self.lib.ut_gp_fit_async
        self._gp_d = d
        L.check(self.ctx, fn(self.ctx, X.ctypes.data, y.ctypes.data, n, d, C.byref(h)), "ut_gp_fit")

    def gp_join_fit(self):
        """ut_gp_join_fit: later work on the engine's stream waits for the
        in-flight fit on the device (no host wait)"""
        L.check(self.ctx, self.lib.ut_gp_join_fit(self.ctx), "ut_gp_join_fit")

    def gp_fit_ok(self) -> bool:
        """ut_gp_fit_status: waits for the last fit; False = its kernel matrix
        was not positive definite (scores are NaN until a fit succeeds)"""
        ok = C.c_int32()
        L.check(self.ctx, self.lib.ut_gp_fit_status(self.ctx, C.byref(ok)), "ut_gp_fit_status")
        return bool(ok.value)

    def gp_set_fit_append(self, enable: bool):
        """incremental fits when the training set only grows (on by default)"""
        L.check(self.ctx, self.lib.ut_gp_set_fit_append(self.ctx, int(bool(enable))), "ut_gp_set_fit_append")

    def gp_last_fit_kind(self) -> str:
        k = C.c_int32()
        L.check(self.ctx, self.lib.ut_gp_last_fit_kind(self.ctx, C.byref(k)), "ut_gp_last_fit_kind")
        return "append" if k.value == 1 else "refit"

    def gp_kstar_mode(self) -> str:
        """ut_gp_kstar_mode: "categorical" (ENUM / BOOL one-hot blocks as an
        int8 code product beside the fp64 contraction) or "dense" """
        v = C.c_int32()
        L.check(self.ctx, self.lib.ut_gp_kstar_mode(self.ctx, C.byref(v)), "ut_gp_kstar_mode")
        return "categorical" if v.value else "dense"

    def gp_lml(self) -> float:
        """ut_gp_lml: log marginal likelihood of the current fit (standardised y);
        waits for an in-flight fit, raises UT_ENOTPD if it was not positive definite"""
        v = C.c_double()
        L.check(self.ctx, self.lib.ut_gp_lml(self.ctx, C.byref(v)), "ut_gp_lml")
        return float(v.value)

    def gp_lml_grad(self) -> Tuple[np.ndarray, float, float]:
        """ut_gp_lml_grad: the gradient of the current fit's log marginal
        likelihood in (log lengthscale [d], log sigma_f2, log sigma_n2); fp64,
        deterministic, waits for an in-flight fit and raises as gp_lml does"""
        d = int(getattr(self, "_gp_d", self.spec.n_features))   # the last gp_fit's feature count
        g = np.empty(d, dtype=np.float64)
        sf, sn = C.c_double(), C.c_double()
        L.check(self.ctx, self.lib.ut_gp_lml_grad(self.ctx, d, g.ctypes.data, C.byref(sf), C.byref(sn)),
                "ut_gp_lml_grad")
        return g, float(sf.value), float(sn.value)

    def gp_lml_grid(self, X: np.ndarray, y: np.ndarray, lengthscale, scales, noises=None, sigma_f2: float = 1.0,
                    sigma_n2: float = 1e-6, jitter: float = 0.0) -> Tuple[np.ndarray, int]:
        """ut_gp_lml_grid: the log marginal likelihood of (X, y) at the points
        (scales[j] * lengthscale, noises[j] or sigma_n2), all factorised in one
        batched chain on the device.  Returns (lml [g], NaN where not positive
        definite; the argmax over the finite values, -1 if none).  The current
        fit and a fit in flight are left as they are."""
        X = np.ascontiguousarray(X, dtype=np.float64)
        y = np.ascontiguousarray(y, dtype=np.float64)
        n, d = X.shape
        ell = np.ascontiguousarray(np.broadcast_to(np.asarray(lengthscale, dtype=np.float64), (d,)))
        sc = np.ascontiguousarray(np.atleast_1d(np.asarray(scales, dtype=np.float64)))
        g = int(sc.shape[0])
        nz = None
        if noises is not None:
            nz = np.ascontiguousarray(np.atleast_1d(np.asarray(noises, dtype=np.float64)))
            if nz.shape != sc.shape:
                raise ValueError("gp_lml_grid: noises must have one entry per scale")
        h = L.GpHyper(sigma_f2=float(sigma_f2), sigma_n2=float(sigma_n2), jitter=float(jitter),
                      lengthscale_host=ell.ctypes.data)
        out = np.empty(max(g, 1), dtype=np.float64)
        best = C.c_int32(-1)
        L.check(self.ctx, self.lib.ut_gp_lml_grid(self.ctx, X.ctypes.data, y.ctypes.data, n, d, C.byref(h), g,
                                                  sc.ctypes.data, None if nz is None else nz.ctypes.data,
                                                  out.ctypes.data, C.byref(best)), "ut_gp_lml_grid")
        return out[:g], int(best.value)

    def gp_stats(self) -> Tuple[float, float, float]:
        a, b, c = C.c_double(), C.c_double(), C.c_double()
        L.check(self.ctx, self.lib.ut_gp_stats(self.ctx, C.byref(a), C.byref(b), C.byref(c)), "ut_gp_stats")
        return a.value, b.value, c.value

    @staticmethod
    def acq(kind: str = "ei", xi: float = 0.0, kappa: float = 2.0) -> L.Acq:
        return L.Acq(kind=L.UT_ACQ_EI if kind == "ei" else L.UT_ACQ_UCB, xi=float(xi), kappa=float(kappa))

    def gp_score(self, feat: torch.Tensor, m: Optional[int] = None, acq: Optional[L.Acq] = None,
                 dup: Optional[torch.Tensor] = None):
        m = feat.shape[1] if m is None else m
        acq = acq or self.acq()
        mu, var, score = self._empty(m), self._empty(m), self._empty(m)
        L.check(self.ctx, self.lib.ut_gp_score(self.ctx, _ptr(feat), feat.stride(0), m, C.byref(acq), _ptr(dup),
                                               _ptr(mu), _ptr(var), _ptr(score)), "ut_gp_score")
        return mu, var, score

    def gp_score_values(self, values: torch.Tensor, m: Optional[int] = None, acq: Optional[L.Acq] = None,
                        dup: Optional[torch.Tensor] = None):
        """ut_gp_score_values: gp_score(encode(values)) with the encoding fused
        into the K* operand pass (no feature matrix)"""
        m = values.shape[1] if m is None else m
        acq = acq or self.acq()
        mu, var, score = self._empty(m), self._empty(m), self._empty(m)
        L.check(self.ctx, self.lib.ut_gp_score_values(self.ctx, _ptr(values), values.stride(0), m, C.byref(acq),
                                                      _ptr(dup), _ptr(mu), _ptr(var), _ptr(score)),
                "ut_gp_score_values")
        return mu, var, score

    def gp_select_batch(self, values: torch.Tensor, k: int, acq: Optional[L.Acq] = None,
                        dup: Optional[torch.Tensor] = None, p: Optional[int] = None):
        """ut_gp_select_batch: k picks from the shortlist values[:, :p], each
        conditioned on the picks before it (the posterior variance shrinks
        around a pick; the mean and f_best stay).  -> (pos [k] positions in
        [0, p) in pick order, score [k] and var [k] at pick time); an empty
        slot holds -1, -inf, NaN.  Always fp64; stream-ordered, no host wait."""
        if values.dim() != 2 or values.shape[0] != self.spec.ncols:
            raise ValueError(f"gp_select_batch: values must be [{self.spec.ncols}][p]")
        if values.stride(1) != 1:
            values = values.contiguous()
        p = values.shape[1] if p is None else int(p)
        k = int(k)
        acq = acq or self.acq()
        n = max(k, 1)
        pos, score, var = self._empty(n, dtype=torch.int64), self._empty(n), self._empty(n)
        L.check(self.ctx, self.lib.ut_gp_select_batch(self.ctx, _ptr(values), values.stride(0), p, C.byref(acq),
                                                      _ptr(dup), k, _ptr(pos), _ptr(score), _ptr(var)),
                "ut_gp_select_batch")
        return pos, score, var

    # ---- Thompson sampling: posterior sample paths (csrc/gp_ts.hip) ----
    def gp_ts_draw(self, q: int, features: int = 1024, round_: int = 0) -> None:
        """ut_gp_ts_draw: q sample paths of the current fit's posterior with
        `features` random Fourier features, keyed by (seed, round_).  The paths
        belong to that fit: draw again after every fit."""
        L.check(self.ctx, self.lib.ut_gp_ts_draw(self.ctx, int(q), int(features), int(round_)), "ut_gp_ts_draw")

    def _pool(self, values: torch.Tensor, m: Optional[int], who: str):
        if values.dim() != 2 or values.shape[0] != self.spec.ncols:
            raise ValueError(f"{who}: values must be [{self.spec.ncols}][m]")
        if values.stride(1) != 1:
            values = values.contiguous()
        return values, (values.shape[1] if m is None else int(m))

    def gp_ts_eval(self, values: torch.Tensor, m: Optional[int] = None) -> torch.Tensor:
        """ut_gp_ts_eval: -> F [q][m], every drawn path at every candidate of
        values[:, :m].  Always fp64; stream-ordered."""
        values, m = self._pool(values, m, "gp_ts_eval")
        info = self.gp_ts_read(None)
        F = torch.empty((info["q"], max(m, 1)), dtype=torch.float64, device=self.device)
        L.check(self.ctx, self.lib.ut_gp_ts_eval(self.ctx, _ptr(values), values.stride(0), m, _ptr(F), F.stride(0)),
                "ut_gp_ts_eval")
        return F

    def gp_ts_select(self, values: torch.Tensor, k: int, dup: Optional[torch.Tensor] = None,
                     m: Optional[int] = None):
        """ut_gp_ts_select: path s < k picks its minimiser over the candidates
        of values[:, :m] that are no duplicates and that no earlier path
        picked.  -> (pos [k], f [k]) in pick order; an empty slot holds -1,
        +inf.  Always fp64; stream-ordered, no host wait."""
        values, m = self._pool(values, m, "gp_ts_select")
        k = int(k)
        n = max(k, 1)
        pos, f = self._empty(n, dtype=torch.int64), self._empty(n)
        L.check(self.ctx, self.lib.ut_gp_ts_select(self.ctx, _ptr(values), values.stride(0), m, _ptr(dup), k,
                                                   _ptr(pos), _ptr(f)), "ut_gp_ts_select")
        return pos, f

    def gp_ts_read(self, what: Optional[str]):
        """ut_gp_ts_read (tests): what in "Z" [D][d], "b" [D], "Theta" [q][D],
        "Eps" [q][n], "A" [q][n] -> a numpy array; None -> the sizes alone."""
        info = (C.c_int32 * 4)()
        L.check(self.ctx, self.lib.ut_gp_ts_read(self.ctx, 0, None, info), "ut_gp_ts_read")
        q, D, n, d = (int(v) for v in info)
        if what is None:
            return dict(q=q, D=D, n=n, d=d)
        code, shape = {"Z": (0, (D, d)), "b": (1, (D,)), "Theta": (2, (q, D)), "Eps": (3, (q, n)),
                       "A": (4, (q, n))}[what]
        out = np.empty(shape, dtype=np.float64)
        L.check(self.ctx, self.lib.ut_gp_ts_read(self.ctx, code, out.ctypes.data_as(C.c_void_p), None),
                "ut_gp_ts_read")
        return out

    def _shortlist(self, values: torch.Tensor, who: str) -> torch.Tensor:
        if values.dim() != 2 or values.shape[0] != self.spec.ncols:
            raise ValueError(f"{who}: values must be [{self.spec.ncols}][p]")
        return values if values.stride(1) == 1 else values.contiguous()

    def gp_acq_grad(self, values: torch.Tensor, acq: Optional[L.Acq] = None):
        """ut_gp_acq_grad: -> (score [p], mu [p], var [p], grad [n_features][p]),
        the acquisition of values[:, :p] under the current fit and its
        derivative in every unit feature.  Always fp64; stream-ordered."""
        values = self._shortlist(values, "gp_acq_grad")
        p = values.shape[1]
        acq = acq or self.acq()
        score, mu, var = self._empty(p), self._empty(p), self._empty(p)
        grad = torch.empty((self.spec.n_features, max(p, 1)), dtype=torch.float64, device=self.device)
        L.check(self.ctx, self.lib.ut_gp_acq_grad(self.ctx, _ptr(values), values.stride(0), p, C.byref(acq),
                                                  _ptr(score), _ptr(mu), _ptr(var), _ptr(grad), grad.stride(0)),
                "ut_gp_acq_grad")
        return score, mu, var, grad

    def gp_polish(self, values: torch.Tensor, steps: int, acq: Optional[L.Acq] = None,
                  dup: Optional[torch.Tensor] = None, step0: float = 0.0, step_max: float = 0.0,
                  grow: float = 0.0, shrink: float = 0.0):
        """ut_gp_polish: `steps` projected gradient-ascent steps on the
        acquisition for each candidate of values[:, :p]; only FLOAT / INT /
        LOGINT / POW2 values move.  -> (values [ncols][p], score [p], score0
        [p], moved [p] uint8); score >= score0, and an unmoved row is the
        input's bits.  A 0 parameter takes the library's default (step0 0.25,
        step_max 1.0, grow 2.0, shrink 0.5)."""
        values = self._shortlist(values, "gp_polish")
        p = values.shape[1]
        acq = acq or self.acq()
        prm = L.PolishParams(steps=int(steps), pad=0, step0=float(step0), step_max=float(step_max),
                             grow=float(grow), shrink=float(shrink))
        out = torch.empty((self.spec.ncols, max(p, 1)), dtype=torch.float64, device=self.device)
        score, score0 = self._empty(p), self._empty(p)
        moved = self._empty(p, dtype=torch.uint8)
        L.check(self.ctx, self.lib.ut_gp_polish(self.ctx, _ptr(values), values.stride(0), p, C.byref(acq), _ptr(dup),
                                                C.byref(prm), _ptr(out), out.stride(0), _ptr(score), _ptr(score0),
                                                _ptr(moved)), "ut_gp_polish")
        return out, score, score0, moved

    # -- failure-aware scoring ----------------------------------------------
    def gp_feas_set(self, X_fail, prior: Optional[float] = None, strength: float = 1.0, ell_scale: float = 1.0,
                    power: float = 1.0):
        """ut_gp_feas_set: load (replace) the features [nf][F] of the configurations
        that FAILED.  While rows are loaded every dense EI score is multiplied by
        p^power, p = (S_ok + strength p0) / (S_ok + S_fail + strength) the kernel
        vote of the fit's rows against these (the GP's kernel, lengthscales times
        ell_scale); prior=None: p0 = n / (n + nf) of the fit in use.  UCB scoring,
        gp_select_batch and, unless gp_set_prune_weighted(True), pruned scoring
        raise UT_EUNSUPPORTED meanwhile."""
        X = np.ascontiguousarray(X_fail, dtype=np.float64)
        if X.ndim != 2:
            raise ValueError("gp_feas_set: X_fail must be [nf][n_features]")
        nf, d = X.shape
        par = L.FeasParams(prior=0.0 if prior is None else float(prior), strength=float(strength),
                           ell_scale=float(ell_scale), power=float(power))
        L.check(self.ctx, self.lib.ut_gp_feas_set(self.ctx, X.ctypes.data if nf else None, nf, d, C.byref(par)),
                "ut_gp_feas_set")

    def gp_feas_clear(self):
        """no failed rows: every call scores as it did before any were loaded"""
        L.check(self.ctx, self.lib.ut_gp_feas_set(self.ctx, None, 0, 0, None), "ut_gp_feas_set")

    def gp_feas_prob(self, values: Optional[torch.Tensor] = None, features: Optional[torch.Tensor] = None,
                     m: Optional[int] = None):
        """ut_gp_feas_prob: (p, S_ok, S_fail), each [m], of candidates given as raw
        values [ncols][m] (the K* the fit scores with) or as features [F][m] (the
        dense contraction); stream-ordered, no host wait"""
        if (values is None) == (features is None):
            raise ValueError("gp_feas_prob: exactly one of values and features")
        x = values if values is not None else features
        if x.stride(1) != 1:
            x = x.contiguous()
        m = x.shape[1] if m is None else int(m)
        p, s_ok, s_fail = self._empty(m), self._empty(m), self._empty(m)
        L.check(self.ctx, self.lib.ut_gp_feas_prob(self.ctx, _ptr(x) if values is not None else None,
                                                   _ptr(x) if values is None else None, x.stride(0), m, _ptr(p),
                                                   _ptr(s_ok), _ptr(s_fail)), "ut_gp_feas_prob")
        return p, s_ok, s_fail

    def gp_feas_info(self) -> Dict[str, Any]:
        """what is loaded: {"nf": rows (0: nothing), "prior" (None: from the fit),
        "strength", "ell_scale", "power"}"""
        nf, par = C.c_int32(), L.FeasParams()
        L.check(self.ctx, self.lib.ut_gp_feas_info(self.ctx, C.byref(nf), C.byref(par)), "ut_gp_feas_info")
        return {"nf": int(nf.value), "prior": float(par.prior) if par.prior > 0.0 else None,
                "strength": float(par.strength), "ell_scale": float(par.ell_scale), "power": float(par.power)}

    # -- constrained EI -------------------------------------------------------
    def gp_cons_set(self, C_values, thresholds):
        """ut_gp_cons_set: load (replace) the measured constraint values
        C [n][nc] of the current fit's rows, in the fit's row order, and the
        thresholds [nc] of c_j <= t_j (a >= constraint: negate both).  While
        loaded every dense EI score becomes EI(f_best over the feasible rows) *
        prod_j P(c_j <= t_j) under GPs on the fit's own factor.  The values
        belong to that fit: call again after every gp_fit (scoring raises
        UT_EINVAL until then).  Does not wait for a fit in flight."""
        Cv = np.ascontiguousarray(C_values, dtype=np.float64)
        if Cv.ndim == 1:
            Cv = Cv.reshape(-1, 1)
        if Cv.ndim != 2:
            raise ValueError("gp_cons_set: C must be [n][nc]")
        thr = np.ascontiguousarray(np.atleast_1d(np.asarray(thresholds, dtype=np.float64)))
        n, nc = Cv.shape
        if thr.shape != (nc,):
            raise ValueError("gp_cons_set: one threshold per constraint column")
        L.check(self.ctx, self.lib.ut_gp_cons_set(self.ctx, Cv.ctypes.data if nc else None, n, nc,
                                                  thr.ctypes.data if nc else None), "ut_gp_cons_set")

    def gp_cons_clear(self):
        """no constraints: every call scores as it did before any were loaded"""
        L.check(self.ctx, self.lib.ut_gp_cons_set(self.ctx, None, 0, 0, None), "ut_gp_cons_set")

    def gp_cons_prob(self, values: Optional[torch.Tensor] = None, features: Optional[torch.Tensor] = None,
                     m: Optional[int] = None):
        """ut_gp_cons_prob: (P [m], mu_c [nc][m]) of candidates given as raw values
        [ncols][m] (the K* the fit scores with) or as features [F][m] (the dense
        contraction): the probability that every constraint holds and the
        standardised constraint means; stream-ordered, no host wait"""
        if (values is None) == (features is None):
            raise ValueError("gp_cons_prob: exactly one of values and features")
        x = values if values is not None else features
        if x.stride(1) != 1:
            x = x.contiguous()
        m = x.shape[1] if m is None else int(m)
        nc = self._cons_counts()[1]
        ld = x.stride(0)
        p = self._empty(m)
        mu_c = torch.empty((max(nc, 1), ld), dtype=torch.float64, device=p.device)
        L.check(self.ctx, self.lib.ut_gp_cons_prob(self.ctx, _ptr(x) if values is not None else None,
                                                   _ptr(x) if values is None else None, ld, m, _ptr(p),
                                                   _ptr(mu_c) if nc else None), "ut_gp_cons_prob")
        return p, mu_c[:nc, :m]

    def _cons_counts(self) -> Tuple[int, int]:
        n, nc = C.c_int32(), C.c_int32()
        L.check(self.ctx, self.lib.ut_gp_cons_info(self.ctx, C.byref(n), C.byref(nc), None, None), "ut_gp_cons_info")
        return int(n.value), int(nc.value)

    def gp_cons_info(self) -> Dict[str, Any]:
        """what is loaded: {"n": rows, "nc": constraints (0: nothing), "n_feasible":
        rows with every value within its threshold, "f_best_c": the smallest
        standardised objective among them (NaN: none)}; waits for the fit"""
        n, nc, nf, fb = C.c_int32(), C.c_int32(), C.c_int32(), C.c_double()
        L.check(self.ctx, self.lib.ut_gp_cons_info(self.ctx, C.byref(n), C.byref(nc), C.byref(nf), C.byref(fb)),
                "ut_gp_cons_info")
        return {"n": int(n.value), "nc": int(nc.value), "n_feasible": int(nf.value), "f_best_c": float(fb.value)}

    # -- two objectives ---------------------------------------------------------
    def gp_mo_set(self, Y2, ref):
        """ut_gp_mo_set: load (replace) the second objective's values Y2 [n] of
        the current fit's rows, in the fit's row order, and the reference point
        (R1 in the units of gp_fit's y, R2 in Y2's); both objectives are
        minimised (a maximised one: negate it).  While loaded every dense EI
        score becomes the expected hypervolume improvement against the rows'
        Pareto front inside the reference box.  The values belong to that fit:
        call again after every gp_fit (scoring raises UT_EINVAL until then).
        Does not wait for a fit in flight."""
        y2 = np.ascontiguousarray(Y2, dtype=np.float64).ravel()
        r = np.ascontiguousarray(ref, dtype=np.float64).ravel()
        if r.shape != (2,):
            raise ValueError("gp_mo_set: the reference point has two coordinates")
        n = y2.shape[0]
        L.check(self.ctx, self.lib.ut_gp_mo_set(self.ctx, y2.ctypes.data if n else None, n, r.ctypes.data),
                "ut_gp_mo_set")

    def gp_mo_clear(self):
        """no second objective: every call scores as it did before one was loaded"""
        L.check(self.ctx, self.lib.ut_gp_mo_set(self.ctx, None, 0, None), "ut_gp_mo_set")

    def gp_mo_score(self, values: Optional[torch.Tensor] = None, features: Optional[torch.Tensor] = None,
                    m: Optional[int] = None):
        """ut_gp_mo_score: (EHVI [m], mu_2 [m]) of candidates given as raw values
        [ncols][m] (the K* the fit scores with) or as features [F][m] (the dense
        contraction); stream-ordered, no host wait"""
        if (values is None) == (features is None):
            raise ValueError("gp_mo_score: exactly one of values and features")
        x = values if values is not None else features
        if x.stride(1) != 1:
            x = x.contiguous()
        m = x.shape[1] if m is None else int(m)
        ehvi, mu2 = self._empty(m), self._empty(m)
        L.check(self.ctx, self.lib.ut_gp_mo_score(self.ctx, _ptr(x) if values is not None else None,
                                                  _ptr(x) if values is None else None, x.stride(0), m, _ptr(ehvi),
                                                  _ptr(mu2)), "ut_gp_mo_score")
        return ehvi, mu2

    def gp_mo_info(self) -> Dict[str, Any]:
        """what is loaded: {"n": rows (0: nothing), "P": the front's size, "ref_std":
        the standardised reference point, "hv": the front's hypervolume inside
        it, standardised units}; waits for the fit"""
        n, P, hv = C.c_int32(), C.c_int32(), C.c_double()
        ref = (C.c_double * 2)()
        L.check(self.ctx, self.lib.ut_gp_mo_info(self.ctx, C.byref(n), C.byref(P), ref, C.byref(hv)), "ut_gp_mo_info")
        return {"n": int(n.value), "P": int(P.value), "ref_std": (float(ref[0]), float(ref[1])), "hv": float(hv.value)}

    def gp_mo_front(self):
        """ut_gp_mo_front: (rows int32 [P], a [P], b [P]) of the front, ordered by
        the standardised first objective ascending; waits for the fit"""
        n = C.c_int32()
        L.check(self.ctx, self.lib.ut_gp_mo_info(self.ctx, C.byref(n), None, None, None), "ut_gp_mo_info")
        cap = int(n.value)
        rows = np.zeros(max(cap, 1), dtype=np.int32)
        a, b = np.zeros(max(cap, 1)), np.zeros(max(cap, 1))
        P = C.c_int32()
        L.check(self.ctx, self.lib.ut_gp_mo_front(self.ctx, rows.ctypes.data, a.ctypes.data, b.ctypes.data, cap,
                                                  C.byref(P)), "ut_gp_mo_front")
        k = int(P.value)
        return rows[:k].copy(), a[:k].copy(), b[:k].copy()

    def gp_mo_read(self, what: int) -> np.ndarray:
        """(for tests) ut_gp_mo_read: 0 = y2s [n], 1 = alpha_2 [n], 2 = (m_2, s_2)"""
        n = C.c_int32()
        L.check(self.ctx, self.lib.ut_gp_mo_info(self.ctx, C.byref(n), None, None, None), "ut_gp_mo_info")
        out = np.zeros(2 if what == 2 else max(int(n.value), 1))
        L.check(self.ctx, self.lib.ut_gp_mo_read(self.ctx, int(what), out.ctypes.data), "ut_gp_mo_read")
        return out if what == 2 else out[:int(n.value)]

    def gp_topk_pruned(self, feat: torch.Tensor, k: int, m: Optional[int] = None, acq: Optional[L.Acq] = None,
                       dup: Optional[torch.Tensor] = None, cand_base: int = 0, bound_rows: int = 256):
        """ut_gp_topk_pruned: the top-k of the GP score, selection-exact, with the
        full variance GEMM only for candidates whose score bound (first
        `bound_rows` rows of L^-1 k*) reaches the threshold.  -> (idx, score, stats dict)"""
        m = feat.shape[1] if m is None else m
        acq = acq or self.acq()
        idx = self._empty(k, dtype=torch.int64)
        top = self._empty(k)
        st = L.PruneStats()
        L.check(self.ctx, self.lib.ut_gp_topk_pruned(self.ctx, _ptr(feat), feat.stride(0), m, C.byref(acq), _ptr(dup),
                                                     int(cand_base), int(k), int(bound_rows), _ptr(idx), _ptr(top),
                                                     C.byref(st)), "ut_gp_topk_pruned")
        return idx, top, {"survivors": st.survivors, "bound_rows": st.bound_rows, "dense": bool(st.dense),
                          "threshold": st.threshold, "m": m}

    # -- tree-ensemble surrogate ---------------------------------------------
    def forest_set(self, model):
        """load a tree ensemble (sklearn regressor, XGBoost JSON or forest.Forest)"""
        from .forest import as_forest
        f = as_forest(model)
        nodes = np.ascontiguousarray(f.nodes)
        roots = np.ascontiguousarray(f.roots, dtype=np.int32)
        L.check(self.ctx, self.lib.ut_forest_set(self.ctx, f.n_trees, roots.ctypes.data, nodes.size,
                                                 nodes.ctypes.data, int(f.rule), float(f.base), float(f.scale),
                                                 float(f.div)), "ut_forest_set")
        self.forest = f
        if f.leaf_var is not None:
            lv = np.ascontiguousarray(f.leaf_var, dtype=np.float64)
            L.check(self.ctx, self.lib.ut_forest_leaf_var(self.ctx, lv.ctypes.data, lv.size), "ut_forest_leaf_var")

    def forest_predict(self, feat: torch.Tensor, m: Optional[int] = None, dup: Optional[torch.Tensor] = None,
                       sign: float = -1.0):
        """-> (pred [m], score [m] = sign * pred, -inf on duplicates)"""
        m = feat.shape[1] if m is None else m
        pred, score = self._empty(m), self._empty(m)
        L.check(self.ctx, self.lib.ut_forest_predict(self.ctx, _ptr(feat), feat.stride(0), m, feat.shape[0],
                                                     _ptr(dup), float(sign), _ptr(pred), _ptr(score)),
                "ut_forest_predict")
        return pred, score

    def forest_score(self, feat: torch.Tensor, acq: Optional[L.Acq] = None, f_best: float = 0.0,
                     dup: Optional[torch.Tensor] = None, m: Optional[int] = None):
        """ut_forest_score of the loaded averaged ensemble: -> (mu, var, score), each [m];
        mu is forest_predict's pred, var the variance over trees plus the mean leaf
        variance, score the GP's acquisition at (mu, var, f_best), -inf on duplicates"""
        m = feat.shape[1] if m is None else m
        acq = acq or self.acq()
        mu, var, score = self._empty(m), self._empty(m), self._empty(m)
        L.check(self.ctx, self.lib.ut_forest_score(self.ctx, _ptr(feat), feat.stride(0), m, feat.shape[0],
                                                   _ptr(dup), C.byref(acq), float(f_best), _ptr(mu), _ptr(var),
                                                   _ptr(score)), "ut_forest_score")
        return mu, var, score

    # -- selection ---------------------------------------------------------
    def topk(self, score: torch.Tensor, k: int, dup: Optional[torch.Tensor] = None, cand_base: int = 0):
        idx = self._empty(k, dtype=torch.int64)
        top = self._empty(k)
        L.check(self.ctx, self.lib.ut_topk(self.ctx, _ptr(score), _ptr(dup), score.numel(), int(cand_base), int(k),
                                           _ptr(idx), _ptr(top)), "ut_topk")
        return idx, top

    # -- whole round -------------------------------------------------------
    def score_round_de(self, m: int, k: int, round_: int = 0, cand_base: int = 0, cr: float = 0.2,
                       n_cross: int = 1, acq: Optional[L.Acq] = None, want_values: bool = True, best=None,
                       information_sharing: int = 1):
        de, keep = self._de_params(cr, n_cross, best, information_sharing)  # noqa: F841 (keeps best alive)
        acq = acq or self.acq()
        idx = self._empty(k, dtype=torch.int64)
        top = self._empty(k)
        dig = self._empty(k, 8, dtype=torch.int32)
        vals = self._empty(self.spec.ncols, k) if want_values else None
        out = L.RoundOut(topk_idx=idx.data_ptr(), topk_score=top.data_ptr(), topk_digest=dig.data_ptr(),
                         topk_values=vals.data_ptr() if vals is not None else None)
        L.check(self.ctx, self.lib.ut_score_round_de(self.ctx, C.byref(de), C.byref(acq), int(round_),
                                                     int(cand_base), int(m), int(k), C.byref(out)),
                "ut_score_round_de")
        return idx, top, dig, vals

    def score_round_ga(self, m: int, k: int, parent1=None, parent2=None, round_: int = 0, cand_base: int = 0,
                       mutation_rate: float = 0.1, sigma: float = 0.1, crossover_rate: float = 0.0,
                       crossover_strength: float = 0.0, must_mutate_count: int = 1, normal: bool = False,
                       max_retries: int = 10, op: int = 4, crossover: Optional[str] = None,
                       acq: Optional[L.Acq] = None, want_values: bool = True):
        """ut_score_round_ga: propose_ga -> hash_parent + dedup (side stream) beside
        encode + GP posterior -> top-k; -> (idx, top, digests, values)"""
        p1, p2 = self._row(parent1), self._row(parent2)
        a = L.GaParams(mutation_rate=mutation_rate, sigma=sigma, crossover_rate=crossover_rate,
                       crossover_strength=crossover_strength, must_mutate_count=must_mutate_count,
                       normal=1 if normal else 0, max_retries=max_retries, op=op, crossover=_xop(crossover))
        acq = acq or self.acq()
        idx = self._empty(k, dtype=torch.int64)
        top = self._empty(k)
        dig = self._empty(k, 8, dtype=torch.int32)
        vals = self._empty(self.spec.ncols, k) if want_values else None
        out = L.RoundOut(topk_idx=idx.data_ptr(), topk_score=top.data_ptr(), topk_digest=dig.data_ptr(),
                         topk_values=vals.data_ptr() if vals is not None else None)
        L.check(self.ctx, self.lib.ut_score_round_ga(self.ctx, C.byref(a), _ptr(p1), _ptr(p2), C.byref(acq),
                                                     int(round_), int(cand_base), int(m), int(k), C.byref(out)),
                "ut_score_round_ga")
        return idx, top, dig, vals

    def score_round_de_pruned(self, m: int, k: int, round_: int = 0, cand_base: int = 0, cr: float = 0.2,
                              n_cross: int = 1, acq: Optional[L.Acq] = None, want_values: bool = True, best=None,
                              information_sharing: int = 1, bound_rows: int = 256):
        """score_round_de with ut_gp_topk_pruned's selection-exact pruning;
        -> (idx, top, digests, values, stats dict)"""
        de, keep = self._de_params(cr, n_cross, best, information_sharing)  # noqa: F841
        acq = acq or self.acq()
        idx = self._empty(k, dtype=torch.int64)
        top = self._empty(k)
        dig = self._empty(k, 8, dtype=torch.int32)
        vals = self._empty(self.spec.ncols, k) if want_values else None
        out = L.RoundOut(topk_idx=idx.data_ptr(), topk_score=top.data_ptr(), topk_digest=dig.data_ptr(),
                         topk_values=vals.data_ptr() if vals is not None else None)
        st = L.PruneStats()
        L.check(self.ctx, self.lib.ut_score_round_de_pruned(self.ctx, C.byref(de), C.byref(acq), int(round_),
                                                            int(cand_base), int(m), int(k), int(bound_rows),
                                                            C.byref(out), C.byref(st)), "ut_score_round_de_pruned")
        return idx, top, dig, vals, {"survivors": st.survivors, "bound_rows": st.bound_rows, "dense": bool(st.dense),
                                     "threshold": st.threshold, "m": m}

    def gp_prune_bounds(self, m: int):
        """ut_gp_prune_bounds (for tests): the last pruned call's per-candidate
        score bounds [m] (float64) and exact flags [m] (uint8) -> (ub, exact)"""
        ub = self._empty(int(m))
        exact = self._empty(int(m), dtype=torch.uint8)
        L.check(self.ctx, self.lib.ut_gp_prune_bounds(self.ctx, _ptr(ub), _ptr(exact), int(m)), "ut_gp_prune_bounds")
        return ub, exact

    def gp_kstar_read(self, c0: int = 0, nc: Optional[int] = None):
        """ut_gp_kstar_read (for tests): the K* the last dense scoring call left
        behind, k*[r][c] for every padded training row r < npad and the columns
        c0 <= c < c0 + nc (nc None: up to ldk), padding included
        -> (k [npad][nc] float64 on the device, npad, ldk, format 64 | 8)"""
        npad, ldk, fmt = C.c_int32(), C.c_int64(), C.c_int32()
        L.check(self.ctx, self.lib.ut_gp_kstar_read(self.ctx, None, int(c0), 0, C.byref(npad), C.byref(ldk),
                                                    C.byref(fmt)), "ut_gp_kstar_read")
        nc = ldk.value - int(c0) if nc is None else int(nc)
        k = self._empty(npad.value, max(nc, 0))
        L.check(self.ctx, self.lib.ut_gp_kstar_read(self.ctx, _ptr(k), int(c0), nc, None, None, None),
                "ut_gp_kstar_read")
        return k, int(npad.value), int(ldk.value), int(fmt.value)

    def gp_kstar_mask_read(self):
        """ut_gp_kstar_mask_read (for tests): the plane-occupancy mask of the digit
        planes the last dense precision-8 call left, bit p of byte [r][c] set iff
        plane p of the 32-row x 32-candidate block (r, c) of K* holds a non-zero digit
        -> uint8 tensor [npad / 32][ldk / 32] on the device, or None when those
        planes have no mask (UT_NOMASK)"""
        rows, cols = C.c_int32(), C.c_int64()
        rc = self.lib.ut_gp_kstar_mask_read(self.ctx, None, C.byref(rows), C.byref(cols))
        if rc == L.NOMASK:
            return None
        L.check(self.ctx, rc, "ut_gp_kstar_mask_read")
        mk = self._empty(rows.value, cols.value, dtype=torch.uint8)
        L.check(self.ctx, self.lib.ut_gp_kstar_mask_read(self.ctx, _ptr(mk), None, None), "ut_gp_kstar_mask_read")
        return mk

    def gp_kstar_screen_stats(self) -> Tuple[bool, int, int]:
        """ut_gp_kstar_screen_stats (for tests): the K* screen of the last
        precision-8 dense call -> (screened, certified units, units of 64
        training rows x 128 candidates)"""
        s, nc, nu = C.c_int32(), C.c_int64(), C.c_int64()
        L.check(self.ctx, self.lib.ut_gp_kstar_screen_stats(self.ctx, C.byref(s), C.byref(nc), C.byref(nu)),
                "ut_gp_kstar_screen_stats")
        return bool(s.value), int(nc.value), int(nu.value)

    def gp_i8_parts_read(self):
        """ut_gp_i8_parts_read (for tests): the precision-8 variance contraction's
        per-64-row-tile column sums of the last dense call that kept its planes
        -> (var_part, mu_part), float64 [npad / 64][ldk] on the device (columns at
        and past that call's m hold no meaning)"""
        rows, ldk = C.c_int32(), C.c_int64()
        L.check(self.ctx, self.lib.ut_gp_i8_parts_read(self.ctx, None, None, C.byref(rows), C.byref(ldk)),
                "ut_gp_i8_parts_read")
        vp, mp = self._empty(rows.value, ldk.value), self._empty(rows.value, ldk.value)
        L.check(self.ctx, self.lib.ut_gp_i8_parts_read(self.ctx, _ptr(vp), _ptr(mp), None, None),
                "ut_gp_i8_parts_read")
        return vp, mp

    def gp_fit_read(self, what: str):
        """ut_gp_fit_read (for tests): one operand of the last fit, after waiting
        for it.  what: a key of _lib.FIT_OPERANDS ("L", "LINV", "LINVT", "ALPHA",
        "BETA", "YS", "LINVT_F32", "I8A", "I8RS", "H3")
        -> (float64 tensor on the device, [npad][npad], [npad] or [2 npad + 2];
        None while info["stale"] is set for LINVT / ALPHA, info: n, npad,
        precision, l_rows, stale)"""
        w = L.FIT_OPERANDS[what]
        fi = L.GpFitInfo()
        L.check(self.ctx, self.lib.ut_gp_fit_read(self.ctx, w, None, C.byref(fi)), "ut_gp_fit_read")
        info = {k: int(getattr(fi, k)) for k, _ in L.GpFitInfo._fields_}
        if what in ("LINVT", "ALPHA") and info["stale"]:
            return None, info
        npad = info["npad"]
        out = self._empty(*{"ALPHA": (npad,), "BETA": (npad,), "YS": (npad,), "I8RS": (2 * npad + 2,)}.get(
            what, (npad, npad)))
        L.check(self.ctx, self.lib.ut_gp_fit_read(self.ctx, w, _ptr(out), None), "ut_gp_fit_read")
        return out, info

    def round_lazy_stats(self) -> Tuple[int, int]:
        """(lazy dense DE rounds, those of them that fell back to hashing every
        candidate) since the context was created; waits for the stream"""
        lz, fb = C.c_int64(), C.c_int64()
        L.check(self.ctx, self.lib.ut_round_lazy_stats(self.ctx, C.byref(lz), C.byref(fb)), "ut_round_lazy_stats")
        return int(lz.value), int(fb.value)

    def round_buffers(self):
        """device pointers (values, features, digests, dup, mu, var, score) of the
        last round and their leading dimension.  features is None; after a lazy
        round that did not fall back (round_lazy_stats) digests and dup are None
        too -- only its score-sorted prefix was hashed -- and score holds the
        unmasked scores."""
        ptrs = [C.c_void_p() for _ in range(7)]
        ld = C.c_int64()
        L.check(self.ctx, self.lib.ut_round_buffers(self.ctx, *[C.byref(p) for p in ptrs], C.byref(ld)),
                "ut_round_buffers")
        return [p.value for p in ptrs], ld.value

    def set_timing(self, on: bool):
        L.check(self.ctx, self.lib.ut_set_timing(self.ctx, 1 if on else 0), "ut_set_timing")

    def stage_time(self, stage: str) -> float:
        v = C.c_double()
        L.check(self.ctx, self.lib.ut_stage_time(self.ctx, stage.encode(), C.byref(v)), "ut_stage_time")
        return v.value

    def decode(self, values: torch.Tensor) -> List[Dict[Any, Any]]:
        return self.spec.decode_values(values.detach().cpu().numpy())


_DEFAULT: Dict[int, BatchEngine] = {}


def default_engine(manipulator) -> BatchEngine:
    dev = torch.cuda.current_device() if torch.cuda.is_available() else 0   # this rank's GPU
    key = (id(manipulator), dev)
    eng = _DEFAULT.get(key)
    if eng is None:
        eng = BatchEngine(manipulator, device=dev)
        _DEFAULT[key] = eng
    return eng
