/*
 * uthot.h -- C ABI of libuthot.so, the gfx950 (MI355X) batch candidate
 * proposal + scoring library behind uptune_amd.
 *
 * Drop-in boundary.  The reference runs this path one configuration at a
 * time inside the Python search loop:
 *   SearchTechnique.desired_configuration()   opentuner/search/technique.py:113-121
 *   DifferentialEvolution.create_new_configuration
 *                                             opentuner/search/differentialevolution.py:105-129
 *   HybridParticle.move / op3_swarm           opentuner/search/pso.py:70-77
 *   EvolutionaryTechnique.mutation            opentuner/search/evolutionarytechniques.py:51-61
 *   ConfigurationManipulator.hash_config      opentuner/search/manipulator.py:233-243
 *   SearchDriver.get_configuration/has_results opentuner/search/driver.py:157-158,253-258
 *   ParallelTuning.unique / hash_cfg          python/uptune/api.py:254-288
 * Each entry point below replaces one of those per-candidate Python calls
 * with one batched, stream-ordered call over m candidates.
 *
 * Conventions
 *   - every function returns 0 on success or a negative UT_E* code; the
 *     message is available from ut_last_error(ctx);
 *   - pointer arguments are DEVICE pointers unless the name ends in _host;
 *   - work is enqueued on the context's HIP stream (ut_set_stream); results
 *     are valid once that stream is synchronised;
 *   - SoA value arrays are column-per-parameter: value of param p for
 *     candidate i lives at values[col(p) * ld + i] (f64 for every kind: FLOAT
 *     raw value, INT/LOGINT raw integer, POW2 raw power of two, BOOL 0/1,
 *     ENUM option index); a PERM of size S takes S consecutive columns
 *     holding its item indices in order.  col(p) = p + the sum of (size - 1)
 *     over the PERM params before p (ut_space_columns);
 *   - digests are 8 big-endian uint32 words (= sha256().digest()) per
 *     candidate, candidate-major ([m][8]);
 *   - candidate indices are GLOBAL (cand_base + i), so random streams and
 *     tie-breaks do not depend on how a pool is sharded over GPUs.
 *   - one context per host thread.
 */
#ifndef UTHOT_H
#define UTHOT_H
#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct ut_ctx ut_ctx;

enum {
  UT_OK = 0,
  UT_EINVAL = -1,      /* bad argument */
  UT_EHIP = -2,        /* HIP runtime error */
  UT_ENOSPACE = -3,    /* ut_space_define not called */
  UT_EUNSUPPORTED = -4,
  UT_ENOTPD = -5,      /* GP kernel matrix not positive definite */
  UT_ENOMEM = -6,
  UT_ECOMM = -7        /* RCCL error (multi-GPU exchange) */
};

/* parameter kinds: manipulator.py:651-1356 (the kinds create_params builds,
 * python/uptune/api.py:179-199) */
enum {
  UT_FLOAT = 0,  /* FloatParameter        manipulator.py:703-744 */
  UT_INT = 1,    /* IntegerParameter      manipulator.py:651-700 */
  UT_LOGINT = 2, /* LogIntegerParameter   manipulator.py:778-797 (stored int, searched log2) */
  UT_POW2 = 3,   /* PowerOfTwoParameter   manipulator.py:811-836 (stored 2^e, searched e) */
  UT_BOOL = 4,   /* BooleanParameter      manipulator.py:930-996 */
  UT_ENUM = 5,   /* EnumParameter         manipulator.py:1024-1045 */
  UT_PERM = 6    /* PermutationParameter  manipulator.py:1048-1356 (n_options = size) */
};

typedef struct ut_param_desc {
  int32_t kind;        /* UT_* kind */
  int32_t sort_rank;   /* position in sorted(params, key=name)  (manipulator.py:237) */
  double lo, hi;       /* min_value, max_value of the STORED value (POW2: powers of two) */
  double u_lo, u_hi;   /* unit-encoding bounds of the SEARCHED value (get_value) as Python
                          computes them: ints widened by 0.4999 (manipulator.py:476-479);
                          LOGINT: its scaled legal_range (:792-795); POW2: exponents -+0.4999 */
  double u_span;       /* float(u_hi - u_lo) as Python computes it */
  int64_t n_options;   /* ENUM option count (BOOL: 2) */
  const char* name;    /* str(p.name) bytes, not NUL-terminated */
  int32_t name_len;
  int32_t lut_count;   /* >0: inner digests of repr(get_value) supplied in lut */
  const uint8_t* lut_host; /* lut_count * 32 bytes: sha256(repr(get_value)).digest(),
                              indexed by (value - lo) for INT and LOGINT, by
                              (exponent - log2 lo) for POW2, by option index for
                              ENUM, 0=False/1=True for BOOL */
  int32_t vtab_count;  /* LOGINT: >0 = get_value(v) = math.log(v + 1.0 - min, 2.0) for
                          v = lo .. lo+vtab_count-1, computed by the host's CPython;
                          0 = computed on the device (ut_core.h libm_log: glibc's
                          log restated bit for bit, so the same values) */
  int32_t pad;
  const double* vtab_host;
  /* PERM: repr(item) bytes of the n_options items, concatenated, and their
   * n_options + 1 offsets; the inner digest is sha256(repr(list of items)),
   * "[" + ", ".join(repr(item)) + "]" (ComplexParameter.hash_value :855-858) */
  const uint8_t* perm_repr_host;
  const int32_t* perm_repr_off_host;
} ut_param_desc;

/* permutation crossover operators (op3_cross_*, manipulator.py:1179-1353) */
enum { UT_X_NONE = 0, UT_X_OX1 = 1, UT_X_OX3 = 2, UT_X_PX = 3, UT_X_CX = 4, UT_X_PMX = 5 };

typedef struct ut_de_params {   /* differentialevolution.py:34-40,142-151 */
  double cr;                    /* crossover rate (0.9 DE, 0.2 DE-Alt) */
  int32_t n_cross;              /* forced crossovers (1), <= 4 */
  int32_t information_sharing;  /* copies of the driver's best config added to the donor pool (1);
                                   used only when best != NULL (differentialevolution.py:112-116) */
  const double* best;           /* device row [ncols]: driver.best_result's values, NULL = no result yet */
} ut_de_params;

typedef struct ut_gp_hyper {
  double sigma_f2;    /* signal variance */
  double sigma_n2;    /* noise variance added to the diagonal */
  double jitter;      /* extra diagonal jitter */
  const double* lengthscale_host; /* d entries (ARD) */
} ut_gp_hyper;

enum { UT_ACQ_EI = 0, UT_ACQ_UCB = 1 };

typedef struct ut_acq {
  int32_t kind;       /* UT_ACQ_EI or UT_ACQ_UCB */
  int32_t pad;
  double xi;          /* EI exploration offset */
  double kappa;       /* UCB: score = kappa*sigma - mu */
} ut_acq;

/* ---- context ------------------------------------------------------------ */
int ut_ctx_create(int device, uint64_t seed, ut_ctx** out);
int ut_ctx_destroy(ut_ctx* ctx);
const char* ut_last_error(ut_ctx* ctx);
/* hipStream_t to enqueue on; NULL = the device's default (null) stream.  A new
 * context starts on its own non-blocking stream. */
int ut_set_stream(ut_ctx* ctx, void* hip_stream);
int ut_sync(ut_ctx* ctx);
int ut_version(void);
/* device memory (bytes) the library currently holds on `device` in this
 * process, over all its contexts (RCCL's own buffers not included): one rank
 * per process and GPU makes this the rank's HBM footprint */
int ut_device_bytes(int32_t device, int64_t* bytes_host);

/* ---- search space (ConfigurationManipulator, manipulator.py:129-272) ---- */
/* py2_layout: 1 = OpenTuner/Python-2 hash layout (no b'' around primitive
 * inner digests; pins samples/tutorials/tuneup.opentuner.db), 0 = uptune's
 * Python-3 port (manipulator.py:240 str() of a bytes object). */
int ut_space_define(ut_ctx* ctx, int32_t n_params, const ut_param_desc* params, int32_t py2_layout);
/* outer hash message length in bytes, SHA-256 block count, GP feature width */
int ut_space_info(ut_ctx* ctx, int64_t* outer_len, int64_t* outer_blocks, int32_t* n_features);
/* number of SoA value columns (= n_params unless the space has PERMs) */
int ut_space_columns(ut_ctx* ctx, int32_t* n_columns);

/* ---- population (DifferentialEvolution.population, PSO particles) ------- */
/* op1_randomize every member on the device (manipulator.py:171-176,596-606) */
int ut_population_init(ut_ctx* ctx, int64_t npop, uint32_t round_);
int ut_population_set(ut_ctx* ctx, int64_t npop, const double* values, int64_t ld);
int ut_population_get(ut_ctx* ctx, double* values, int64_t ld);
/* population slots: every population / PSO call acts on the selected slot
 * (initially 0).  The techniques of one bandit share one context -- one GP
 * fit, one history set -- with a population each (bandittechniques.py:311-320
 * composes DE, PSO and GA over one surrogate).  slot in [0, 1024). */
int ut_population_select(ut_ctx* ctx, int32_t slot);
/* copy trial rows back into the population: pop[:, idx[j]] = trial[:, j] */
int ut_population_replace(ut_ctx* ctx, const double* trial, int64_t ld, const int64_t* idx, int64_t n);

/* ---- proposal ----------------------------------------------------------- */
/* DE/rand/1/bin: one trial per candidate; candidate g targets population
 * member g % npop (differentialevolution.py:105-129).  Donors x1, x2, x3 are
 * the first three of a shuffle of population - {target} plus
 * information_sharing copies of `best` (:109-118): three distinct pool
 * positions, so x1..x3 may all be copies of the best config.  Needs
 * npop - 1 + (best ? information_sharing : 0) >= 3. */
int ut_propose_de(ut_ctx* ctx, const ut_de_params* p, uint32_t round_, int64_t cand_base, int64_t m,
                  double* out_values, int64_t ld);

/* PSO (pso.py:11-77, HybridParticle + op3_swarm per kind).  Candidate g
 * moves particle g % npop towards gbest (device row [P]) and its own best. */
typedef struct ut_pso_params {
  double omega, phi_l, phi_g;   /* 0.5, 0.5, 0.5 (pso.py:49) */
  double sigma;                 /* Int/Pow2 gaussian noise, unit scale 0.2 (manipulator.py:661) */
  int32_t alias_pbest;          /* 1 = reference: particle.best IS the position (pso.py:46, :60) */
  int32_t enum_mode;            /* 0 = reference: enum never moves (manipulator.py:442); 1 = corrected */
  int32_t crossover;            /* PERM: UT_X_* of PSO(crossover=...) (pso.py:80-84; op3_swarm :1115-1140) */
  int32_t pad;
} ut_pso_params;
/* velocities := 0 and particle bests := positions (pso.py:59-68) */
int ut_pso_reset(ut_ctx* ctx);
int ut_propose_pso(ut_ctx* ctx, const ut_pso_params* p, const double* gbest, uint32_t round_, int64_t cand_base,
                   int64_t m, double* out_values, double* out_velocity, int64_t ld);
/* particles [cand_base, cand_base+m) take the moved positions / velocities */
int ut_pso_commit(ut_ctx* ctx, const double* values, const double* velocity, int64_t ld, int64_t cand_base,
                  int64_t m);
/* particle bests for selected particles: best[:, idx[j]] = values[:, j] */
int ut_pso_update_best(ut_ctx* ctx, const double* values, int64_t ld, const int64_t* idx, int64_t n);

/* GA family (evolutionarytechniques.py:13-158, globalGA.py:11-129). */
typedef struct ut_ga_params {
  double mutation_rate;       /* per-param mutation probability */
  double sigma;               /* NormalMutationMixin sigma (0.1) */
  double crossover_rate;      /* probability of selecting two parents */
  double crossover_strength;  /* GGA: fraction of params copied from parent 2 (0.2); 0 = GA family */
  int32_t must_mutate_count;  /* 1; <= P */
  int32_t normal;             /* 1 = NormalGreedyMutation / GGA, 0 = UniformGreedyMutation / GA */
  int32_t max_retries;        /* 10 (hash equal to a parent -> mutate again); <= 15 */
  int32_t op;                 /* RNG stream family: 4 = GA, 5 = GGA */
  int32_t crossover;          /* GA(crossover=...): UT_X_* applied to PERM params of size > 6 when two
                                 parents are selected (CrossoverMixin.crossover :123-134); UT_X_NONE else */
  int32_t pad;
} ut_ga_params;
/* parent1/parent2: device rows [P] (the global best), NULL = random parent
 * (select() without a best result).  out_invalid[i] = 1 when all retries
 * reproduced a parent (the reference returns None). */
int ut_propose_ga(ut_ctx* ctx, const ut_ga_params* p, const double* parent1, const double* parent2,
                  uint32_t round_, int64_t cand_base, int64_t m, double* out_values, int64_t ld,
                  uint8_t* out_invalid);

/* Trust-region proposals: candidates inside a box around one centre row,
 * each moving a random subset of the parameters (TuRBO's perturbation rule,
 * Eriksson et al. 2019; uptune_amd/trust_region.py keeps the box's size).
 *
 * Inputs: centre c (device row of ncols SoA values, as ut_propose_ga's
 * parent1), half_width_host h[P] (host, unit space, finite and >= 0; read by
 * primitive kinds only), prob / cat_prob the perturbation probability of the
 * primitive kinds (FLOAT, INT, LOGINT, POW2) / of BOOL, ENUM and PERM, and
 * must: that many parameters are always perturbed.
 *
 * Candidate g = cand_base + i is a function of (seed, g, round_) alone, so
 * any split of [cand_base, cand_base + m) over calls or ranks gives the same
 * rows.  Draws use op code OP_TR = 6 (ut_core.h).  For p = 0 .. P - 1 in order,
 * with sel = 0 at p = 0:
 *   A = draw(seed, g, p, round_, OP_TR)
 *   forced: (double)(P - p) * u01(A.x, A.y) < (double)must - sel; then sel += 1
 *           (selection sampling, as ut_propose_ga's must_mutate_count)
 *   rate:   (double)A.z * 2^-32 < prob        (cat_prob for BOOL / ENUM / PERM)
 *   A.w is unused.  p is selected iff forced or rate; an unselected parameter
 *   keeps the centre's value(s), bit for bit.
 * For a selected p, B = draw(seed, g, p | 1 << 28, round_, OP_TR) and
 *   FLOAT / INT / LOGINT / POW2:
 *       uc = get_unit_value(c_p);  lo = max(uc - h_p, 0);  hi = min(uc + h_p, 1)
 *       u  = lo + (hi - lo) * u01(B.x, B.y)     (each operation rounded, this order)
 *       v  = set_unit_value(u) + 0.0, or c_p when the range is a single point
 *            (+ 0.0: an integer kind whose value rounds to zero from below
 *            stores +0.0 as the centre does, not -0.0, which int() does not have)
 *     (lo and hi are computed once per call and parameter, not per candidate)
 *   BOOL:  v = 1 - c_p
 *   ENUM:  n_opt = 1 keeps c_p; else r = floor(u64(B.z, B.w) * (n_opt - 1) / 2^64),
 *          r += (r >= c_p), v = r: uniform over the other options
 *   PERM:  op1_small_random_change (manipulator.py:1066-1079, p = 0.25) on a copy
 *          of the centre's permutation, from the perm draw site
 *          (seed, g, p | 1 << 28, round_, OP_TR); B itself is not drawn.
 * out_invalid[i] = 1 when row i equals the centre bit for bit in every column
 * (integer rounding can bring a value back; there are no retries).
 *
 * UT_EINVAL: a NULL params, centre or half_width_host, prob or cat_prob outside
 * [0, 1], a half-width that is negative or not finite, must outside [0, P],
 * m < 0, cand_base < 0, ld < m, a NULL out_values or out_invalid with m > 0.
 * UT_ENOSPACE before ut_space_define.  No kernel runs on a refused call. */
typedef struct ut_tr_params {
  double prob;
  double cat_prob;
  int32_t must;
  int32_t pad;
} ut_tr_params;
int ut_propose_tr(ut_ctx* ctx, const ut_tr_params* p, const double* centre, const double* half_width_host,
                  uint32_t round_, int64_t cand_base, int64_t m, double* out_values, int64_t ld,
                  uint8_t* out_invalid);

/* GP features of configurations: unit values (get_unit_value), BOOL 0/1,
 * ENUM one-hot, PERM position of each item / (size - 1).  out_features[f * ld_out + i]. */
int ut_encode_features(ut_ctx* ctx, const double* values, int64_t ld, int64_t m, double* out_features,
                       int64_t ld_out);

/* ---- identity + dedup (hash_config, driver.get_configuration) ----------- */
int ut_hash(ut_ctx* ctx, const double* values, int64_t ld, int64_t m, uint32_t* out_digest);
/* The same digests for DE trials of the selected population: candidate i's
 * target is member (cand_base + i) % npop (ut_propose_de).  Inner digests of
 * values bitwise equal to the target's are taken from a per-population cache
 * (built on first use, patched by ut_population_replace); only the changed
 * values are formatted and hashed.  Correct for any values (a value that does
 * not match its "target" is simply recomputed); fast when most match. */
int ut_hash_de(ut_ctx* ctx, const double* values, int64_t ld, int64_t m, int64_t cand_base, uint32_t* out_digest);
/* The same digests for GA / GGA children of one parent config (ut_propose_ga:
 * parent1, a device row of ncols values; mutation and crossover change a few
 * params, the rest are the parent's): inner digests of values bitwise equal
 * to the parent's come from the parent's own digests (computed once per call);
 * only the changed values are formatted and hashed.  Correct for any values.
 * Replaces the per-child hash_config of evolutionarytechniques.py:38-49. */
int ut_hash_parent(ut_ctx* ctx, const double* values, int64_t ld, int64_t m, const double* parent,
                   uint32_t* out_digest);
/* Empty history sized for `capacity` digests.  If the new table cannot be
 * allocated (UT_ENOMEM) the history is left empty and valid: ut_dedup then
 * reports in-batch repeats only, and ut_history_add may be called again. */
int ut_history_reset(ut_ctx* ctx, int64_t capacity);
/* Add n digests (a digest may be given more than once, in one call or over
 * several).  The table grows as needed; if a growth fails (UT_ENOMEM, UT_EHIP)
 * the history is exactly what it was before the call: none of the call's
 * digests is added and every earlier one is still found. */
int ut_history_add(ut_ctx* ctx, const uint32_t* digests, int64_t n);   /* device [n][8] */
int ut_history_add_host(ut_ctx* ctx, const uint32_t* digests_host, int64_t n);
/* out_dup[i] = 1 if digest i is in the history or repeats an earlier
 * (smaller index) candidate of the same batch. */
int ut_dedup(ut_ctx* ctx, const uint32_t* digests, int64_t m, uint8_t* out_dup);

/* ---- GP surrogate ------------------------------------------------------- */
/* X_host: [n][d] features, y_host: [n] objective (minimised).  Fits
 * L = chol(K + (sigma_n2 + jitter) I), L^-1, alpha on the device. */
int ut_gp_fit(ut_ctx* ctx, const double* X_host, const double* y_host, int32_t n, int32_t d,
              const ut_gp_hyper* hyper);
/* The same fit, enqueued on the context's internal fit stream without a host
 * wait: it runs beside whatever is enqueued next (e.g. the proposal and hash
 * stages of the next round), and every later scoring call waits for it on the
 * device.  X_host / y_host may be reused on return (they are staged in
 * pinned memory); the fit's launches are issued by the next call that needs
 * them -- after the proposal of ut_score_round_* / ut_propose_* (ordered
 * before it on the device), or on entry to any call that reads GP state.
 * A failed fit (not positive definite) is reported by ut_gp_stats /
 * ut_gp_fit_status, and makes every score NaN (nothing is selected). */
int ut_gp_fit_async(ut_ctx* ctx, const double* X_host, const double* y_host, int32_t n, int32_t d,
                    const ut_gp_hyper* hyper);
/* Incremental fits (default on; UT_FIT_APPEND=0 or enable=0 turns them off):
 * when a fit's training set extends the previous fit's -- its first n_old
 * rows bitwise equal to the previous X, the same hyperparameters, the same
 * padded size (n rounded up to 128) and a positive-definite previous factor --
 * the factor is extended by block rows (B = K21 L^-T, D = chol(K22 - B B^T),
 * new L^-1 rows -D^-1 B L^-1) instead of refactored: O(n^2 k) instead of
 * O(n^3).  The posterior equals the refit's to rounding.  The tuning loop's
 * per-generation refit (SharedModel.fit: the results table only grows) is
 * exactly this case.  ut_gp_last_fit_kind: 0 = the last fit refactored,
 * 1 = it appended. */
int ut_gp_set_fit_append(ut_ctx* ctx, int32_t enable);
int ut_gp_last_fit_kind(ut_ctx* ctx, int32_t* kind);
/* posterior of standardised y and the acquisition score for m candidates
 * (features [d][ld]).  mu/var/score may be NULL.  dup (may be NULL) marks
 * candidates excluded from selection (score forced to -inf). */
int ut_gp_score(ut_ctx* ctx, const double* features, int64_t ld, int64_t m, const ut_acq* acq,
                const uint8_t* dup, double* mu, double* var, double* score);
/* ut_gp_score on raw values [ncols][ld] instead of features: the encoding
 * (ut_encode_features), the 1/lengthscale scaling and |u|^2 run as one pass
 * that writes only what the K* GEMM reads, so no [d][m] feature matrix is
 * written and read back.  Same results as ut_gp_score(ut_encode_features(values))
 * for values in their parameters' domains: ENUM values are option indices in
 * [0, n_options) and BOOL values 0 or 1, as every proposal kernel writes them
 * (the reference has no other values: an out-of-range index raises in
 * EnumParameter, manipulator.py).  In categorical mode (ut_gp_kstar_mode) an
 * out-of-range ENUM value matches no option (2 / ell^2 against every training
 * row, where the dense encoding's all-zero block gives 1 / ell^2) and a BOOL
 * value other than 0 counts as 1. */
int ut_gp_score_values(ut_ctx* ctx, const double* values, int64_t ld, int64_t m, const ut_acq* acq,
                       const uint8_t* dup, double* mu, double* var, double* score);
/* Selection-exact pruned scoring + top-k (fp64 fits only; EI, or UCB with
 * kappa >= 0: scores that increase with sigma).  sigma^2 = sf2 - |L^-1 k*|^2
 * and every row of L^-1 k* adds a square, so the first `bound_rows` rows give
 * an upper bound on sigma^2, hence on the score, at a (bound_rows / n)^2
 * fraction of the variance GEMM.  The exact scores of the 1024 best bounds
 * give a threshold tau (their k-th best); only candidates whose bound reaches
 * tau get the full variance GEMM, and the top-k of those is the top-k of the
 * dense evaluation (every pruned candidate's exact score < tau <= the k-th
 * best).  out_idx/out_score [k] as ut_topk (global indices cand_base + i).
 * The mean is k* . alpha (K* epilogue), so the whole fit is waited for.  One
 * host synchronisation (the survivor count).  stats (host, may be NULL):
 * survivors, the bound rows used, tau. */
typedef struct ut_prune_stats {
  int64_t survivors;     /* candidates that got the full variance (m if the round fell back to dense) */
  int32_t bound_rows;    /* rows of L^-1 k* in the bound (a multiple of 128) */
  int32_t dense;         /* 1: too many survivors, the round ran the dense variance instead */
  double threshold;      /* tau; -inf when the threshold set holds fewer than k valid candidates
                            (m < k, or nearly all duplicates): then nothing is pruned */
} ut_prune_stats;
int ut_gp_topk_pruned(ut_ctx* ctx, const double* features, int64_t ld, int64_t m, const ut_acq* acq,
                      const uint8_t* dup, int64_t cand_base, int32_t k, int32_t bound_rows, int64_t* out_idx,
                      double* out_score, ut_prune_stats* stats_host);
/* arithmetic of the two scoring contractions (K* and L^-1 K*^T) for fits made
 * after this call: 64 = fp64 MFMA (default; 1e-5 parity), 32 = fp32 MFMA
 * (1e-3 parity), 16 = "f16x3": K* in fp64, the variance contraction as three
 * fp16 MFMA products (hi*hi + hi*lo + lo*hi) of scaled hi/lo splits of L^-1 and
 * K*, f32 accumulate (fp32-class, the same 1e-3 parity tier), 8 = the fp64
 * tier on the int8 MFMA: K* in fp64 (mean k* . alpha in fp64), the variance
 * contraction over six 8-bit digit planes of L^-1 and K* with exact int32
 * sums, each candidate's variance error bounded from the digits' truncation;
 * candidates whose bound exceeds ut_gp_set_i8_tol (relative) are recomputed
 * on the fp64 path (1e-5 parity, the fp64 tier's).  The fit itself is always
 * fp64.  Replaces the variance half of the per-candidate GP posterior the
 * reference has none of; precision 8 scores need n <= 16384. */
int ut_gp_set_precision(ut_ctx* ctx, int32_t bits);
/* ut_gp_topk_pruned's bound pass over every candidate: 32 (default) runs the
 * distance contraction past the bound rows on the f32 MFMA and k* = sf2 2^t
 * by v_exp_f32, and widens each candidate's score bound by every rounding of
 * it (|k*^ - k*| <= rho k*^ + 2^-125 sf2 with rho from the contraction length
 * and the norms; the mean within (rho + 2^-19) sum |alpha| k*^; the bound rows
 * stay fp64); the threshold set and the survivors are then scored in fp64
 * (mean k* . alpha), so the selection is the dense one.  64: the bound pass in
 * fp64 (its mean exact and reused for the survivors). */
int ut_gp_set_prune_pass(ut_ctx* ctx, int32_t bits);
/* Weighted pruning (off by default).  With enable = 0, ut_gp_topk_pruned and
 * ut_score_round_de_pruned return UT_EUNSUPPORTED while failed rows
 * (ut_gp_feas_set) or constraint values (ut_gp_cons_set) are loaded.  With
 * enable = 1 both accept them with UT_ACQ_EI and return the k best
 * (S, -index) pairs among the valid candidates of the dense weighted score
 *   S(u) = (E(u) P(u)) p(u)^gamma,
 * E the EI at f_best_c (1 when values are loaded and no row is feasible), P the
 * constraint weight (1 with no values), p the feasibility vote (p^gamma = 1
 * with no rows): the dense path's factors in its order.  Every factor lies in
 * [0, 1], so the bound of the first bound_rows rows stays a bound; the
 * constraint weight is bounded per candidate as well,
 *   ub(u)  = ub_E(u) prod_j Pub_j(u),
 *   Pub_j  = 1 where tau_j - mu_cj(u) >= 0, else Phi((tau_j - mu_cj(u)) / sqrt(var_ub(u)))
 * (Phi of a negative ratio rises with sigma, and var <= var_ub), with ub_E at
 * f_best_c (1 with no feasible row) and mu_cj exact for every candidate (one
 * fp64 pass of the constraint means per call, at either bound pass).  The vote
 * gets no bound.  A bound is flagged exact (ut_gp_prune_bounds) only when the
 * pass pins the variance and the EI argument and no failed rows are loaded:
 * with failed rows no bound is exact, and a flat posterior then runs the dense
 * branch.  ut_gp_prune_bounds returns the weighted bounds; ut_prune_stats is
 * unchanged.  Still refused with enable = 1: UT_ACQ_UCB while anything is
 * loaded (UT_EUNSUPPORTED, the dense path's message), constraint values of an
 * earlier fit (UT_EINVAL), failed rows the categorical K* cannot read
 * (UT_EINVAL).  With nothing loaded the switch changes no bit of any result. */
int ut_gp_set_prune_weighted(ut_ctx* ctx, int32_t enable);
/* precision 8: the largest accepted relative error of a candidate's variance
 * (default 2^-20); 0 recomputes every candidate in fp64 */
int ut_gp_set_i8_tol(ut_ctx* ctx, double tol);
/* precision 8: candidates of the last ut_gp_score / round recomputed in fp64
 * (-1: most were, and the whole round ran the fp64 contraction), and the
 * current fit's bound E on |L^-1 k* - v^| */
int ut_gp_i8_stats(ut_ctx* ctx, int64_t* recomputed_host, double* bound_host);
/* precision 8: the fit's error bounds -- E on |L^-1 k* - v^| (the variance)
 * and Emu = sum_r e_r |(L^-1 y)_r| on the mean mu^ = v^ . L^-1 y, which the
 * int8 variance epilogue computes (gp_i8.hip); 0 for other fits.  A candidate
 * is recomputed in fp64 unless its variance bound is <= tol * var and
 * Emu <= tol * sqrt(var). */
int ut_gp_i8_bounds(ut_ctx* ctx, double* E, double* Emu);
/* order everything enqueued on ctx's stream after this call behind the
 * in-flight fit (a stream wait on its event; no host wait).  Scoring that
 * needs the whole fit (pruned, fp32, f16x3) then starts with the fit done, and
 * the proposal / hash stages before it no longer share the CUs with the fit's
 * chain of small kernels. */
int ut_gp_join_fit(ut_ctx* ctx);
/* wait for the last (possibly asynchronous) fit and report whether its kernel
 * matrix was positive definite (*ok = 1) or not (*ok = 0: later scoring
 * yields NaN scores until a new fit succeeds); not an error either way */
int ut_gp_fit_status(ut_ctx* ctx, int32_t* ok);
/* the K* contraction the current fit scores with: *categorical = 1 when its
 * ENUM / BOOL one-hot blocks go through the int8 code product (one lengthscale
 * over those features, every training row one-hot there; candidates encoded
 * by the library), 0 = the dense fp64 contraction over every feature.  Both
 * give the same posterior (the categorical part of |x - u|^2 is exactly
 * 2 / ell^2 per mismatching ENUM, 1 / ell^2 per BOOL); UT_CAT_KSTAR=0 turns
 * the categorical form off. */
int ut_gp_kstar_mode(ut_ctx* ctx, int32_t* categorical);
/* f_best (min standardised y), y mean/std used for standardisation */
int ut_gp_stats(ut_ctx* ctx, double* f_best, double* y_mean, double* y_std);
/* Log marginal likelihood of the standardised targets,
 *   lml = -1/2 |L^-1 ys|^2 - sum_{i<n} log L_ii - (n/2) log 2 pi,  L = chol(K + (sigma_n2 + jitter) I):
 * the measure by which a lengthscale is chosen (the reference has no GP and so
 * none to choose).
 * LML of the current fit (standardised y); waits for an in-flight fit like
 * ut_gp_fit_status; UT_ENOTPD if that fit was not positive definite */
int ut_gp_lml(ut_ctx* ctx, double* lml_host);
/* LML at g hyperparameter points for the training set (X_host [n][d], y_host [n]):
 * point j uses lengthscale scale_host[j] * hyper->lengthscale_host[k] (the ARD
 * shape is kept), hyper->sigma_f2, and noise noise_host[j] (NULL: hyper->sigma_n2)
 * + hyper->jitter.  lml_host[j] = NaN where K is not positive definite.
 * *best_host = argmax over the finite values (ties: smallest j), -1 if none.
 * Synchronous.  Leaves the context's current fit, a staged asynchronous fit
 * and every scoring result untouched.  The g factorisations run batched, in
 * chunks of as many points as fit 1 GiB of kernel matrices (UT_LML_BATCH
 * overrides the chunk size; the results do not depend on it), in scratch
 * buffers of their own.  n < 1, d < 1, g < 1, a NULL pointer (noise_host
 * excepted) or a scale that is not finite and > 0 is UT_EINVAL. */
int ut_gp_lml_grid(ut_ctx* ctx, const double* X_host, const double* y_host, int32_t n, int32_t d,
                   const ut_gp_hyper* hyper, int32_t g, const double* scale_host,
                   const double* noise_host, double* lml_host, int32_t* best_host);
/* Gradient of the LML of the current fit in the log hyperparameters.  With
 *   W = alpha alpha^T - K^-1,  Kf_ij = sigma_f2 exp(-1/2 |xs_i - xs_j|^2)  (K, xs as in ut_gp_lml):
 *   dlog_ell_host[k] = dLML / dlog ell_k     = 1/2 sum_ij W_ij Kf_ij (xs_ik - xs_jk)^2   (d values)
 *   *dlog_sf2_host   = dLML / dlog sigma_f2  = 1/2 sum_ij W_ij Kf_ij
 *   *dlog_sn2_host   = dLML / dlog sigma_n2  = 1/2 sigma_n2 tr W   (the jitter is a constant)
 * over the n training rows.  Waits for an in-flight fit like ut_gp_lml;
 * UT_ENOTPD if that fit was not positive definite; UT_EINVAL if d is not the
 * fit's feature count or dlog_ell_host is NULL (the two scalar outputs may be
 * NULL).  Always fp64, whatever ut_gp_set_precision says, and over every
 * feature, whichever K* the fit scores with.  Reads the fit, writes scratch of
 * its own: the fit and every scoring result stay as they are.  Sums in a fixed
 * order: two calls on one fit return the same bits. */
int ut_gp_lml_grad(ut_ctx* ctx, int32_t d, double* dlog_ell_host, double* dlog_sf2_host,
                   double* dlog_sn2_host);
/* Batch-aware selection: k picks from a shortlist of p candidates (values
 * [ncols][ld], raw values as for ut_gp_score_values), each conditioned on the
 * picks before it, so that one round's batch is not k neighbours.  With U the
 * shortlist's features and the current fit:
 *   mu_i = k*_i . alpha,  V = L^-1 K*^T  (n x p),
 *   Sigma = Kss - V^T V,  Kss_ij = sigma_f2 exp(-1/2 |us_i - us_j|^2)  (every scaled feature),
 *   var_i = max(Sigma_ii, 0)           (the sigma_f2 - |v|^2 of ut_gp_score)
 * and for t = 0 .. k-1:
 *   1. s_i = acq(mu_i, var_i) with the fit's f_best (the acquisition of
 *      ut_gp_score, the same ut_acq); -inf where dup[i] != 0 (dup may be NULL)
 *      and for a candidate already picked;
 *   2. j = argmax s, ties to the smallest position; if the maximum is -inf or
 *      NaN this slot and every later one is empty;
 *   3. c_i = Sigma_ij - sum_{s<t} G_is G_js,  q = c_j + sigma_n2 + jitter (the
 *      believed observation is as noisy as a training point),
 *      G_it = c_i / sqrt(q),  var_i <- max(var_i - G_it^2, 0).
 * mu and f_best never change: conditioning on an observation equal to its own
 * posterior mean moves no other mean, and a lowered f_best would penalise a
 * pick's neighbours twice (GP-BUCB's variance-only update, for EI as for UCB).
 * So the first pick is the plain top-1, and for EI, and UCB with kappa >= 0,
 * the scores at pick time never increase.
 * Device outputs, in pick order: out_pos [k] positions in [0, p), out_score [k]
 * the score at pick time, out_var [k] the conditioned variance at pick time;
 * an empty slot holds -1, -inf, NaN.  out_score and out_var may be NULL.
 * Stream-ordered, no host wait: an in-flight fit is waited for on the device,
 * and a failed fit makes every score NaN, so every slot is empty.  Always
 * fp64, whatever ut_gp_set_precision says, and over every feature, whichever
 * K* the fit scores with.  Reads the fit, writes scratch of its own: the fit,
 * every scoring result and the round buffers stay as they are.  Sums in a
 * fixed order: two calls on one fit return the same bits.  The loop is one
 * small launch per pick (k + 1 in all).
 * UT_EINVAL: p < 1, k < 1, k > p, p > 4096, ld < p, a NULL values, acq or
 * out_pos, a fit whose feature count is not the space's, no fit (as
 * ut_gp_score_values).  UT_ENOMEM: the scratch could not be allocated. */
int ut_gp_select_batch(ut_ctx* ctx, const double* values, int64_t ld, int32_t p, const ut_acq* acq,
                       const uint8_t* dup, int32_t k, int64_t* out_pos, double* out_score, double* out_var);

/* ---- Thompson sampling: posterior sample paths over the pool --------------- */
/* The reference has no GP.  Its model-based selection is randomised all the
 * same: multi_stage.py:109-123 samples its picks from a rank window of the
 * model's ordering, and bandittechniques.py breaks the ties of its arm
 * ordering at random (bandittechniques.py:58).  Here the randomisation is the GP's own: one sample path of the
 * posterior per batch slot over the whole pool, each slot taking its path's
 * minimiser (TuRBO's acquisition inside the trust-region box).  The joint
 * posterior is not sampled exactly (cubic in the pool); the paths are built by
 * pathwise conditioning (Matheron's rule), linear in the pool.
 *
 * Inputs: the current fit's training features X (n x d), 1/ell per feature,
 * sigma_f2, diag = sigma_n2 + jitter, the standardised targets ys, the factor
 * L with its explicit L^-1; the call's q paths, D features, 24-bit round_.
 *
 * Draws (the counter generator of ut_core.h with OP_TS = 7; indices < 2^20;
 * normal_draw's attempts take stream bits 24-27, the sub-blocks bits 28-29):
 *   Z[j][k]     = normal_draw(seed, cand = j, stream = k, round_, OP_TS)       j < D, k < d
 *   b[j]        = u01(x, y) of draw(seed, j, STREAM_CAND, round_, OP_TS)       a phase in turns, [0, 1)
 *   Theta[s][j] = normal_draw(seed, j, s | (1 << STREAM_SUB_SHIFT), round_, OP_TS)   s < q
 *   Eps[s][r]   = normal_draw(seed, r, s | (2 << STREAM_SUB_SHIFT), round_, OP_TS)   r < n
 *
 * Paths, with us = u * (1/ell) per feature and Zs[j][k] = Z[j][k] * INV_2PI,
 * INV_2PI = 0.15915494309189535 the fp64 nearest of 1 / (2 pi), the product
 * rounded once per entry of Z (that is where the 1 / (2 pi) rounding sits):
 *   tau_j(u) = sum_k Zs[j][k] us_k + b_j                      (turns)
 *   phi_j(u) = sqrt(2 sigma_f2 / D) cos2pi(tau_j - rint(tau_j))
 *   g_s(u)   = sum_j Theta[s][j] phi_j(u)                     (the prior path)
 *   r_s      = ys - g_s(X) - sqrt(diag) Eps[s]                (length n)
 *   a_s      = L^-T (L^-1 r_s)
 *   f_s(u)   = g_s(u) + sum_r k(x_r, u) a_s[r],   k = sigma_f2 exp(-1/2 |xs_r - us|^2) over every feature
 * cos2pi is ut_core.h's (IEEE + - * only; its error bound COS_ERR is stated
 * there).  At every training row r, whatever D:
 *   f_s(x_r) + sqrt(diag) Eps[s][r] + diag a_s[r] = ys[r].
 *
 * Picks, for s = 0 .. k-1 (k <= q): pos_s = the position of the smallest
 * f_s(u_i) over the candidates with dup[i] == 0 (dup may be NULL) that no
 * earlier path picked; ties to the smallest position; if none is left or the
 * minimum is NaN (any remaining value NaN), slot s and every later slot are
 * empty: -1, +inf.
 *
 * ut_gp_ts_draw: Z, b, Theta, Eps and A = [a_s] ([q][npad], 0 on padding rows)
 *   on the device for the current fit; g_s(X) by the path kernel itself on the
 *   training rows, a_s for all q columns by two products with the explicit
 *   inverse on the fp64 MFMA.
 * ut_gp_ts_eval: device out_F [q][ldf] = f_s(u_i) for the m candidates values
 *   [ncols][ld] (raw values as for ut_gp_score_values).
 * ut_gp_ts_select: the pick rule; device out_pos [k], out_f [k] (may be NULL).
 *   Paths are evaluated in groups of 32 (the F workspace is 32 x m doubles:
 *   256 MiB at m = 2^20); a group's picks finish before the next group is
 *   evaluated, a taken mask on the device carries across groups, a pick is two
 *   small launches, and nothing is read by the host in between.
 * ut_gp_ts_read: (for tests) what = 0 Z [D][d], 1 b [D], 2 Theta [q][D],
 *   3 Eps [q][n], 4 A [q][n] into out_host; info (may be NULL) = {q, D, n, d}.
 *   out_host NULL: info alone.  Waits for the stream.
 * Always fp64 and over every feature, whatever ut_gp_set_precision says and
 * whichever K* the fit scores with.  Stream-ordered, no host wait (ut_gp_ts_read
 * apart): an in-flight fit is waited for on the device, and a failed fit makes
 * every path NaN, so every slot is empty.  Reads the fit, writes scratch of its
 * own.  Sums run in a fixed order with no atomics into results: two calls on
 * one fit and one draw return the same bits.
 * UT_EINVAL: no fit; draws made for an earlier fit (stale: draw again after
 * every fit) or none; q < 1 or q > 256; D < 128, not a multiple of 128, or
 * > 4096; round_ >= 2^24; k < 1 or k > q; a NULL values, out_F or out_pos;
 * m < 1; ld or ldf < m; a fit whose feature count is not the space's.
 * UT_ENOMEM: the scratch could not be allocated. */
int ut_gp_ts_draw(ut_ctx* ctx, int32_t q, int32_t D, uint32_t round_);
int ut_gp_ts_eval(ut_ctx* ctx, const double* values, int64_t ld, int64_t m, double* out_F, int64_t ldf);
int ut_gp_ts_select(ut_ctx* ctx, const double* values, int64_t ld, int64_t m, const uint8_t* dup, int32_t k,
                    int64_t* out_pos, double* out_f);
int ut_gp_ts_read(ut_ctx* ctx, int32_t what, double* out_host, int32_t* info);

/* ---- acquisition gradient and projected-ascent polish --------------------- */
/* The reference's default bandit carries a local-search arm, RandomNelderMead
 * (bandittechniques.py:273-278; the simplex walk itself is
 * simplextechniques.py:180-320).  Here the shortlist of a GP round is refined
 * by the acquisition's own gradient instead: the polish below stands in for
 * that arm, it is not a Nelder-Mead.
 *
 * ut_gp_acq_grad: score, mean, variance and d score / d u of p candidates
 * (values [ncols][ld], raw values as for ut_gp_score_values; 1 <= p <= 4096).
 * With u the candidate's unit features, us = u / ell, xs_i the fit's scaled
 * training rows (the dense RBF over every feature, as ut_gp_select_batch):
 *   k_i = sigma_f2 exp(-1/2 |us - xs_i|^2),  v = L^-1 k,  w = L^-T v,
 *   mu = v . beta,  var = max(sigma_f2 - |v|^2, 0),  sigma = sqrt(var),
 *   dmu/du_j  = -(1/ell_j) (us_j sum_i alpha_i k_i - sum_i alpha_i k_i xs_ij)
 *   dvar/du_j = +(2/ell_j) (us_j sum_i w_i k_i     - sum_i w_i k_i xs_ij)
 *   dsigma/du_j = dvar/du_j / (2 sigma) where sigma > 0, else 0
 *   EI:  ds = -Phi(z) dmu + phi(z) dsigma,  I = f_best - mu - xi, z = I / sigma;
 *        where sigma is not > 0: ds = -[I > 0] dmu
 *   UCB: ds = kappa dsigma - dmu
 * f_best and xi as in ut_gp_score (the same ut_acq); score is that call's
 * acquisition of (mu, var).  Device outputs: out_score [p] (may be NULL),
 * out_mu [p], out_var [p] (may be NULL), out_grad [n_feat][ld_g]: the
 * derivative in EVERY unit feature, one-hot and PERM columns included.
 * Stream-ordered, no host wait: an in-flight fit is waited for on the device; a
 * failed fit makes every score NaN (the return code is still 0).  Always fp64,
 * whatever ut_gp_set_precision says.  Reads the fit, writes scratch of its
 * own.  Sums in a fixed order: two calls on one fit return the same bits.
 * UT_EINVAL: p < 1, p > 4096, ld < p, ld_g < p, a NULL values, acq, out_mu or
 * out_grad, no fit, a fit whose feature count is not the space's, and while
 * constraint values (ut_gp_cons_set) or failed rows (ut_gp_feas_set) are
 * loaded: the gradient of the weighted score is not built.
 * UT_ENOMEM: the scratch could not be allocated. */
int ut_gp_acq_grad(ut_ctx* ctx, const double* values, int64_t ld, int32_t p, const ut_acq* acq,
                   double* out_score, double* out_mu, double* out_var, double* out_grad, int64_t ld_g);

typedef struct ut_polish_params {
  int32_t steps;   /* T >= 0 ascent steps */
  int32_t pad;
  double step0;    /* first step length, in lengthscale units; 0: 0.25 */
  double step_max; /* its cap; 0: 1.0 */
  double grow;     /* factor after an accepted step; 0: 2.0 */
  double shrink;   /* factor after a rejected step; 0: 0.5 */
} ut_polish_params;

/* ut_gp_polish: T steps of projected gradient ascent on the acquisition for
 * each of p candidates, all on the device.  Per candidate i:
 *   1. u = the encoder's unit features of the input values, eta = step0,
 *      s = s0 = score(u) (ut_gp_acq_grad's score).  A candidate with
 *      dup[i] != 0 (dup may be NULL) never moves: its out_score and out_score0
 *      are -inf and its out_values the input.  A failed fit makes every score
 *      NaN, so nothing moves.
 *   2. T times: g = ds/du; g_j = 0 on every feature that is not a FREE column
 *      (the unit value of a FLOAT, INT, LOGINT or POW2 parameter with
 *      u_lo < u_hi; BOOL, ENUM and PERM columns are never free) and where
 *      (u_j <= 0 and g_j < 0) or (u_j >= 1 and g_j > 0);
 *      N = sqrt(sum_j (ell_j g_j)^2), j ascending.  N == 0 or not finite: the
 *      candidate stays and eta is unchanged.  Otherwise the trial is
 *      u'_j = clip(u_j + eta ell_j^2 g_j / N, 0, 1) on the free columns, and
 *      s' = score(u').  s' > s (strictly): u <- u', s <- s',
 *      eta <- min(grow eta, step_max); otherwise eta <- shrink eta.
 *   3. A candidate that accepted no step is returned as it came.  Otherwise
 *      v' = set_unit_value(u) on the free parameters (manipulator.py:490-503;
 *      integer kinds round there), every other column the input's bits; v' is
 *      encoded again by the same encoder and scored: s_v.  If s_v > s0:
 *      out_values = v', out_score = s_v, moved = 1; otherwise out_values are
 *      the input's bits, out_score = s0, moved = 0.
 * So out_score >= out_score0 for every candidate, out_score is bitwise what
 * ut_gp_acq_grad returns as score on out_values (same p), and steps = 0
 * returns the input bitwise.
 * Device outputs: out_values [ncols][ld_o], out_score [p], out_score0 [p] (may
 * be NULL), out_moved [p] (may be NULL).  Stream-ordered, no host wait; always
 * fp64; fixed summation order (two calls return the same bits); 2 T + 1
 * evaluations of K* and V = L^-1 K*^T (T = 0: 2), T of W = L^-T V.
 * UT_EINVAL: as ut_gp_acq_grad (p, ld, NULL values / acq / out_values /
 * out_score / prm, no fit, feature count, loaded constraint values or failed
 * rows), ld_o < p, steps < 0, a negative or non-finite step0, step_max, grow
 * or shrink.  UT_ENOMEM: the scratch could not be allocated. */
int ut_gp_polish(ut_ctx* ctx, const double* values, int64_t ld, int32_t p, const ut_acq* acq,
                 const uint8_t* dup, const ut_polish_params* prm, double* out_values, int64_t ld_o,
                 double* out_score, double* out_score0, uint8_t* out_moved);

/* ---- failure-aware scoring ---------------------------------------------- */
/* The surrogate is fitted on results that succeeded; a configuration that
 * failed (compile error, crash, timeout) only joins the dedup set.  These calls
 * load the FAILED configurations' features, and every dense EI score is then
 * weighted by an estimate p(u) of the probability that candidate u succeeds
 * (constrained EI: score = EI * p).  The reference has no counterpart: a
 * failed result is only ever "worst" there.
 *
 * p is a kernel vote (Nadaraya-Watson) over the current fit's training rows
 * x_r (r < n, the results that succeeded) and the loaded failed rows f_q
 * (q < nf), with the GP's own kernel and lengthscales ell, sigma_f2 left out:
 *   k(a, u)   = exp(-1/2 |(a - u) / ell|^2 / s^2)          (k(a, a) = 1)
 *   S_ok(u)   = sum_{r < n}  k(x_r, u)
 *   S_fail(u) = sum_{q < nf} k(f_q, u)
 *   p(u)      = (S_ok + lambda p0) / (S_ok + S_fail + lambda)
 * p lies in [0, 1]; far from all data p -> p0, on a lone failed row
 * p ~ lambda p0 / (1 + lambda).  A finite score becomes score * p^gamma (no pow
 * when gamma == 1); -inf (a duplicate) and NaN (a failed fit) pass through, and
 * mu and var are never changed.  The sums run in a fixed order: two calls return
 * the same bits. */
typedef struct ut_feas_params {
  double prior;      /* p0 in (0, 1]; <= 0: n / (n + nf) of the fit in use, taken at scoring time */
  double strength;   /* lambda > 0: the prior's weight in pseudo-observations */
  double ell_scale;  /* s > 0: the vote's kernel is the GP's with every lengthscale times s */
  double power;      /* gamma >= 0 */
} ut_feas_params;
/* Load (replace) the failed rows: Xfail_host [nf][d], features as ut_gp_fit takes
 * them; nf = 0 clears (Xfail_host and p may then be NULL).  p == NULL: prior
 * from the fit, lambda = s = gamma = 1.  May be called before any fit;
 * synchronous on the host side (the caller's buffer is free on return).  The
 * rows' scaled K* operands are rebuilt for every new fit, so a refit with
 * other lengthscales needs no second call.
 * While rows are loaded the weight applies to ut_gp_score, ut_gp_score_values,
 * ut_score_round_de and ut_score_round_ga at every precision, and, as it is
 * defined for EI only (a UCB score can be negative), a scoring call with
 * UT_ACQ_UCB returns UT_EUNSUPPORTED; so do ut_gp_topk_pruned and
 * ut_score_round_de_pruned unless ut_gp_set_prune_weighted is on (their
 * weighted bound is opt-in) and ut_gp_select_batch (its per-pick acquisition
 * does not know the weight).  A fit that
 * scores with the categorical K* needs failed rows that are one-hot in the
 * ENUM blocks and 0 / 1 in the BOOL columns: otherwise the scoring call returns
 * UT_EINVAL naming the first row that is not.
 * UT_EINVAL (what was loaded before stays loaded): Xfail_host NULL with nf > 0,
 * nf < 0, d not the space's feature count, a non-finite row entry, strength or
 * ell_scale not finite and > 0 (or 1 / ell_scale^2 not a normal number), power
 * not finite or < 0, prior > 1 or NaN. */
int ut_gp_feas_set(ut_ctx* ctx, const double* Xfail_host, int32_t nf, int32_t d, const ut_feas_params* p);
/* p (and optionally S_ok, S_fail) of m candidates, by the formulae above, for
 * the fit in use and the rows loaded (none: S_fail = 0, p0 = 1).  Exactly one
 * of values ([ncols][ld], raw values as for ut_gp_score_values: the K* the fit
 * scores with) and features ([d][ld], as for ut_gp_score: the dense contraction
 * over every feature) is non-NULL.  Device outputs [m]; p_out is required,
 * s_ok_out and s_fail_out may be NULL.  Needs a fit (UT_EINVAL without one);
 * stream-ordered, no host wait: it waits on the device for an in-flight fit's
 * scaled training inputs only, as K* does. */
int ut_gp_feas_prob(ut_ctx* ctx, const double* values, const double* features, int64_t ld, int64_t m,
                    double* p_out, double* s_ok_out, double* s_fail_out);
/* what is loaded: the row count (0: nothing) and the parameters as given (either may be NULL) */
int ut_gp_feas_info(ut_ctx* ctx, int32_t* nf, ut_feas_params* p);

/* ---- constrained EI ------------------------------------------------------ */
/* The reference's ThresholdAccuracyMinimizeTime (objective.py:246-298) minimises
 * time among the results whose accuracy reaches a target.  A constraint that is
 * MEASURED on every run is a GP target like the objective, on the same inputs,
 * kernel and hyperparameters, so it shares the fit's factor L and needs only a
 * weight vector of its own (Gardner et al. 2014, constrained EI).
 *
 * Up to UT_CONS_MAX constraints c_j(x) <= t_j (a >= constraint: negate both on
 * the host).  For the current fit -- n rows X, lengthscales, sigma_f2,
 * sigma_n2 + jitter, L, the standardised objective ys -- and values C [n][nc]
 * row-aligned with the fit's rows:
 *   m_j, s_j   = mean, std (ddof 0; std 0 -> 1) of column j  (the fit's own rule for y)
 *   chat_j     = (C[:, j] - m_j) / s_j        tau_j = (t_j - m_j) / s_j
 *   alpha_j    = K^-1 chat_j = L^-T (L^-1 chat_j)
 *   mu_cj(u)   = k*(u) . alpha_j              (k* with sigma_f2, the K* the fit scores with)
 *   P_j(u)     = Phi((tau_j - mu_cj(u)) / sqrt(var(u)));  var(u) == 0: mu_cj(u) <= tau_j ? 1 : 0
 *   P(u)       = prod_j P_j(u)                (j ascending)
 *   F          = { r : C[r, j] <= t_j for every j }   (compared on the raw values)
 *   f_best_c   = min_{r in F} ys[r]
 *   score(u)   = EI(mu(u), var(u); f_best_c, xi) P(u)   if F is not empty
 *              = P(u)                                    if F is empty
 * var(u) is the objective's own posterior variance (the latent constraint: no
 * sigma_n2 is added), EI the acquisition of ut_gp_score with f_best_c in place
 * of the fit's f_best.  -inf (a duplicate) and NaN (a failed fit) pass through;
 * mu and var are never changed.  With every row feasible and P = 1 the result
 * is bitwise the unconstrained score.  All sums run in a fixed order: two calls
 * return the same bits. */
#define UT_CONS_MAX 4
/* Load (replace) the constraint values of the fit that is current at the call
 * (objective.py:246-298): C_host [n][nc], threshold_host [nc]; nc = 0 clears
 * (both pointers may then be NULL).  A fit staged by ut_gp_fit_async counts as
 * current and is not waited for.  Synchronous on the host side (the caller's
 * buffers are free on return).  The values belong to that fit: after any later
 * fit every scoring call that would apply them returns UT_EINVAL, naming the
 * stale fit, until ut_gp_cons_set is called again or the constraints are
 * cleared.
 * While constraints are loaded the rule above applies to ut_gp_score,
 * ut_gp_score_values, ut_score_round_de and ut_score_round_ga at every
 * precision, after the dense posterior and before the feasibility weight
 * (score = EI(f_best_c) P p^gamma when both are loaded); a scoring call with
 * UT_ACQ_UCB returns UT_EUNSUPPORTED, and so do ut_gp_select_batch and, unless
 * ut_gp_set_prune_weighted is on, ut_gp_topk_pruned and
 * ut_score_round_de_pruned.
 * UT_EINVAL (what was loaded before stays loaded): no fit, n not the fit's n,
 * nc < 0 or nc > UT_CONS_MAX, a NULL pointer with nc > 0, a non-finite value,
 * a NaN threshold (+-inf thresholds are allowed). */
int ut_gp_cons_set(ut_ctx* ctx, const double* C_host, int32_t n, int32_t nc, const double* threshold_host);
/* P (p_out [m], required) and optionally the standardised constraint means
 * mu_cj (mu_c_out [nc][ld], may be NULL) of m candidates under the loaded
 * constraints (objective.py:246-298); none loaded: P = 1.  Exactly one of values
 * ([ncols][ld], raw values: the K* the fit scores with) and features ([d][ld]:
 * the dense contraction over every feature) is non-NULL.  Runs the objective's
 * posterior for var(u) first.  Device outputs; stream-ordered, no host wait. */
int ut_gp_cons_prob(ut_ctx* ctx, const double* values, const double* features, int64_t ld, int64_t m,
                    double* p_out, double* mu_c_out);
/* What is loaded (objective.py:246-298): the row count, the constraint count
 * (0: nothing), the size of F and f_best_c (NaN when F is empty or nothing is
 * loaded).  Any pointer may be NULL.  Waits for the fit when either of the
 * last two is asked for; UT_EINVAL then if the values belong to an earlier fit. */
int ut_gp_cons_info(ut_ctx* ctx, int32_t* n, int32_t* nc, int32_t* n_feasible, double* f_best_c);

/* ---- two objectives ------------------------------------------------------ */
/* The reference orders results by a pair in MaximizeAccuracyMinimizeSize
 * (objective.py:218-230), lexicographically: one point comes back.  Here a
 * second measured quantity is a GP target like the objective -- same inputs,
 * kernel and hyperparameters, so the fit's factor L and, in standardised
 * units, its posterior variance are shared -- and the score of a candidate is
 * the exact expected hypervolume improvement (EHVI) against the Pareto front
 * of the fit's rows.
 *
 * Both objectives are minimised (a maximised one: negate it on the host).  For
 * the current fit -- n rows, the standardised objective ys with its mean m_1
 * and std s_1, sigma_f2, L -- values Y2 [n] row-aligned with the fit's rows and
 * a reference point (R1, R2), R1 in the units of the y given to ut_gp_fit, R2
 * in Y2's:
 *   m_2, s_2   = mean, std (ddof 0; std 0 -> 1) of Y2      (the fit's own rule for y)
 *   y2s        = (Y2 - m_2) / s_2        r_j = (R_j - m_j) / s_j
 *   alpha_2    = L^-T (L^-1 y2s)
 *   mu_1(u), var(u) = the objective's posterior as ut_gp_score gives it at the
 *                     fit's precision tier
 *   mu_2(u)    = sigma_f2 (k*(u) . alpha_2)   (fp64, row-tile partials summed tile 0 upward)
 *   sigma      = sqrt(var(u))
 * The front F of the rows (a, b) = (ys[r], y2s[r]): row r is in F iff
 *   a_r < r_1 and b_r < r_2, and
 *   no row s has a_s <= a_r, b_s <= b_r and one of a_s < a_r, b_s < b_r, s < r
 * (of identical points the smallest row stays).  F is ordered by (a, r)
 * ascending, so a_1 < ... < a_P and b_1 > ... > b_P; the sentinels are
 * a_0 = -inf, a_{P+1} = r_1, b_0 = r_2.
 *   psi(t; mu) = 0                                        t = -inf
 *              = max(t - mu, 0)                           var == 0
 *              = (t - mu) Phi(z) + sigma phi(z),  z = (t - mu) / sigma   otherwise
 *   w_i        = max(psi(a_{i+1}; mu_1) - psi(a_i; mu_1), 0)             i = 0 .. P
 *   EHVI(u)    = sum_{i = 0 .. P} w_i psi(b_i; mu_2)                     i ascending, fp64
 * (Phi and phi as in the EI of ut_gp_score.)  This is the exact expectation of
 * the hypervolume gain of (Y1, Y2) ~ N(mu_1, var) x N(mu_2, var): the region
 * inside the reference box that F does not dominate is the union of the strips
 * [a_i, a_{i+1}) x (-inf, b_i), and E[(a' - max(Y, a))+] = psi(a') - psi(a).
 * EHVI >= 0; P = 0 gives psi(r_1; mu_1) psi(r_2; mu_2).  -inf (a duplicate)
 * and NaN (a failed fit) scores pass through; mu and var are never changed;
 * two calls return the same bits. */
/* Load (replace) the second objective of the fit that is current at the call
 * (objective.py:218-230): Y2_host [n], ref_host [2]; n = 0 clears (both
 * pointers may then be NULL).  A fit staged by ut_gp_fit_async counts as
 * current and is not waited for.  Synchronous on the host side.  The values
 * belong to that fit: after any later fit every scoring call that would apply
 * them returns UT_EINVAL, naming the stale fit, until ut_gp_mo_set is called
 * again or the values are cleared.
 * While a second objective is loaded ut_gp_score, ut_gp_score_values,
 * ut_score_round_de and ut_score_round_ga with UT_ACQ_EI return score = EHVI
 * at every precision, applied after the dense posterior (xi is ignored);
 * UT_ACQ_UCB returns UT_EUNSUPPORTED, and so do ut_gp_topk_pruned and
 * ut_score_round_de_pruned (whatever ut_gp_set_prune_weighted says),
 * ut_gp_select_batch, ut_gp_acq_grad, ut_gp_polish and ut_gp_ts_select, and
 * ut_gp_cons_set and ut_gp_feas_set with values or rows to load.  No kernel
 * runs on a refused call.
 * UT_EINVAL (what was loaded before stays loaded): no fit, n < 0 or not the
 * fit's n, a NULL pointer with n > 0, a non-finite value or reference
 * coordinate.  UT_EUNSUPPORTED (likewise): constraint values or failed rows
 * are loaded. */
int ut_gp_mo_set(ut_ctx* ctx, const double* Y2_host, int32_t n, const double* ref_host);
/* EHVI (ehvi_out [m], required) and optionally mu_2 (mu2_out [m], may be NULL)
 * of m candidates under the loaded second objective (objective.py:218-230).
 * Exactly one of values ([ncols][ld], raw values: the K* the fit scores with)
 * and features ([d][ld]: the dense contraction over every feature) is
 * non-NULL.  Runs the objective's posterior first.  Device outputs;
 * stream-ordered, no host wait.  UT_EINVAL: nothing loaded, values of an
 * earlier fit, no fit, bad arguments. */
int ut_gp_mo_score(ut_ctx* ctx, const double* values, const double* features, int64_t ld, int64_t m,
                   double* ehvi_out, double* mu2_out);
/* What is loaded (objective.py:218-230): the row count (0: nothing), the size
 * P of F, the standardised reference point (r_1, r_2) and the hypervolume of F
 * inside it, sum_i (a_{i+1} - a_i) (r_2 - b_i), in standardised units (NaN
 * when nothing is loaded).  Any pointer may be NULL.  Waits for the fit when
 * any of the last three is asked for; UT_EINVAL then if the values belong to
 * an earlier fit. */
int ut_gp_mo_info(ut_ctx* ctx, int32_t* n, int32_t* P, double* ref_std, double* hv);
/* The ordered front (objective.py:218-230): *P its size, and its first
 * min(P, cap) members' rows, a and b into the host arrays (each may be NULL).
 * Waits for the fit.  UT_EINVAL: nothing loaded, values of an earlier fit,
 * cap < 0, P NULL. */
int ut_gp_mo_front(ut_ctx* ctx, int32_t* rows_host, double* a_host, double* b_host, int32_t cap, int32_t* P);
/* (for tests) what = 0: y2s [n], 1: alpha_2 [n], 2: m_2, s_2 into out_host.  Waits for the fit. */
int ut_gp_mo_read(ut_ctx* ctx, int32_t what, double* out_host);

/* ---- selection ---------------------------------------------------------- */
/* k largest scores, ties -> smallest global index; entries with dup[i]!=0 or
 * NaN score are never selected; missing slots get index -1.  out_score of a
 * missing slot is unspecified (it depends on the route the call takes: the
 * score of some unselectable entry, or 0.0); read out_score only where
 * out_idx >= 0.  The same holds for the padded slots of a round's topk_score. */
int ut_topk(ut_ctx* ctx, const double* score, const uint8_t* dup, int64_t m, int64_t cand_base, int32_t k,
            int64_t* out_idx, double* out_score);

/* ---- one whole round: propose(DE) -> hash -> dedup -> encode -> GP score
 *      -> top-k.  Buffers are owned by the context; results copied to the
 *      given device pointers (any may be NULL). ------------------------- */
typedef struct ut_round_out {
  int64_t* topk_idx;      /* [k] global candidate index */
  double* topk_score;     /* [k] */
  uint32_t* topk_digest;  /* [k][8] */
  double* topk_values;    /* [P][k] */
} ut_round_out;
int ut_score_round_de(ut_ctx* ctx, const ut_de_params* de, const ut_acq* acq, uint32_t round_, int64_t cand_base,
                      int64_t m, int32_t k, const ut_round_out* out);
/* A GA / GGA scoring round (UniformGreedyMutation / NormalGreedyMutation / GA /
 * GGA proposals, evolutionarytechniques.py:29-61, globalGA.py:28-48 and :68-76): the
 * children of parent1 (ut_propose_ga's parameters), hash_config of the children
 * (ut_hash_parent with parent1; ut_hash without) and dedup against the history
 * + the batch on a second stream beside the encode and the GP posterior,
 * invalid children (every retry reproduced a parent) counted as duplicates,
 * then the top-k.  The fit must be current (ut_gp_fit / _async). */
int ut_score_round_ga(ut_ctx* ctx, const ut_ga_params* ga, const double* parent1, const double* parent2,
                      const ut_acq* acq, uint32_t round_, int64_t cand_base, int64_t m, int32_t k,
                      const ut_round_out* out);
/* the same round with ut_gp_topk_pruned's selection-exact pruning in place of
 * the dense variance (fp64 fits; the round's mu/var/score buffers are not
 * filled) */
int ut_score_round_de_pruned(ut_ctx* ctx, const ut_de_params* de, const ut_acq* acq, uint32_t round_,
                             int64_t cand_base, int64_t m, int32_t k, int32_t bound_rows, const ut_round_out* out,
                             ut_prune_stats* stats_host);
/* device pointers to the last round's internal buffers (for tests/bench);
 * features is NULL: the rounds (dense and pruned) encode straight into the K*
 * operands (features / ell, norms, one-hot codes) and keep no feature matrix.
 * After a lazy round that did not fall back (ut_round_lazy_stats) digests and
 * dup are NULL -- only the round's score-sorted prefix was hashed -- and score
 * holds the unmasked scores (no -inf on duplicates); asking for either of the
 * two waits for the round. */
int ut_round_buffers(ut_ctx* ctx, double** values, double** features, uint32_t** digests, uint8_t** dup,
                     double** mu, double** var, double** score, int64_t* ld);
/* for tests: copy, on ctx's stream, the per-candidate score bounds [m] (device
 * doubles: +inf where the f32 pass had no usable bound, -inf on duplicates,
 * NaN after a failed fit) and exact flags [m] (device bytes: 1 = the bound is
 * the candidate's exact score) of the last ut_gp_topk_pruned /
 * ut_score_round_de_pruned call into caller-provided device arrays (either
 * may be NULL).  They are kept when that call fell back to the dense variance.
 * UT_EINVAL while no pruned call has computed bounds, or if m is not that
 * call's m. */
int ut_gp_prune_bounds(ut_ctx* ctx, double* ub_out, uint8_t* exact_out, int64_t m);
/* for tests: the K* that the last dense scoring call (ut_gp_score,
 * ut_gp_score_values, a dense round) on ctx left in its scratch, element by
 * element: k_out [npad][nc] (device doubles, written on ctx's stream) gets
 * k*[r][c] for every training row 0 <= r < npad and candidate column
 * c0 <= c < c0 + nc <= ldk, the padding (r >= n, c >= m: exact zeros)
 * included.  *npad, *ldk: that call's padded sizes; *format: 64 when the
 * scratch holds fp64 rows (copied: an fp64 fit, or a precision-8 call whose
 * whole round fell back to fp64 and rewrote K*), 8 when it holds precision 8's
 * six digit planes (decoded exactly: a 48-bit integer times 2^(eb - 48)).
 * Where those planes have a plane-occupancy mask (ut_gp_kstar_mask_read), a
 * digit of a plane whose mask bit is clear is decoded as 0: true by the mask's
 * definition, and necessary after a screened call (ut_gp_kstar_screen_stats),
 * which does not write the planes of the units it certified as all-zero.
 * k_out may be NULL (the sizes and the format only); so may the other three.
 * Nothing is launched or recorded on the scoring paths for this.
 * UT_EUNSUPPORTED after a dense call of an fp32 or f16x3 fit; UT_EINVAL when no
 * dense call has completed since the last fit (a fit, a pruned call and a failed
 * dense call each leave nothing to read) or for columns outside [0, ldk]. */
int ut_gp_kstar_read(ut_ctx* ctx, double* k_out, int64_t c0, int64_t nc, int32_t* npad, int64_t* ldk,
                     int32_t* format);
/* for tests: the plane-occupancy mask of the digit planes ut_gp_kstar_read
 * decodes, as k_gp_kstar_q wrote it beside them: mask_out [npad / 32][ldk / 32]
 * (device bytes, copied on ctx's stream) has bit p of byte [r][c] set iff digit
 * plane p (0 = most significant) of the 32 training rows x 32 candidates block
 * (r, c) of K* holds a non-zero digit; the padding's bytes are 0.  The
 * precision-8 variance contraction skips the zero planes' loads and products
 * by it while the last call's K* had a zero plane in at least 1 block of 16
 * (UT_VAR_SKIP, read per call: 0 never, 1 always; both kernels give the same bits).
 * *rows, *cols (may be NULL): npad / 32 and ldk / 32; mask_out may be NULL (the
 * sizes only).  Nothing is launched or recorded on the scoring paths for this.
 * Returns UT_NOMASK (a status, not an error: no message is set) when the planes the last dense call left
 * have no mask: written by k_gp_kstar<int8_t> (UT_KSTAR_Q=0, categorical fits)
 * or rewritten as fp64 rows by the whole-round fallback; UT_EINVAL when there
 * are no precision-8 planes to describe (ut_gp_kstar_read's conditions). */
#define UT_NOMASK 1
int ut_gp_kstar_mask_read(ut_ctx* ctx, uint8_t* mask_out, int32_t* rows, int64_t* cols);
/* for tests: the K* screen of the last precision-8 dense call.  Before
 * k_gp_kstar_q a screened call bounds every element's exponent from the
 * products of the operands' two top digit planes and certifies the units (64
 * training rows x 128 candidates) whose every element is stored as six zero
 * digits: their planes are not computed, their mask bytes are 0.  A call
 * screens when k_gp_kstar_q runs, npad <= 2048, d <= 128, UT_VAR_SKIP is not 0,
 * and UT_KSTAR_SCREEN (read per call) is 1, or unset while at least half of the
 * last call's blocks were all-zero.  *screened: 1 / 0; *certified: the certified
 * units (0 when not screened); *units: (npad / 64) (ldk / 128), 0 when the last
 * dense call left no masked planes.  UT_KSTAR_STRIPS (read per call): 1 / 0
 * makes a screened call's variance kernel walk / not walk the screen's list of
 * strips with a live unit, unset it does when at least 7 blocks in 8 of the
 * last call were all-zero; the same bits either way.  Host values of the last call's one sync:
 * nothing is launched or recorded on the scoring paths for this. */
int ut_gp_kstar_screen_stats(ut_ctx* ctx, int32_t* screened, int64_t* certified, int64_t* units);
/* for tests: the precision-8 variance contraction's per-tile partials of the
 * last dense precision-8 call that kept its digit planes (ut_gp_kstar_read's
 * format 8), copied on ctx's stream: var_part_out and mu_part_out (device
 * doubles, either may be NULL) get [npad / 64][ldk], row rt the column sums of
 * v^2 and of v beta over the 64 training rows of tile rt; columns at and past
 * that call's m are not written by the contraction and hold no meaning.
 * *rows, *ldk (may be NULL): npad / 64 and ldk.  Nothing is launched or
 * recorded on the scoring paths for this.  UT_EINVAL otherwise. */
int ut_gp_i8_parts_read(ut_ctx* ctx, double* var_part_out, double* mu_part_out, int32_t* rows, int64_t* ldk);
/* for tests: one operand of the last fit, as doubles.  Waits for that fit
 * (a staged one is enqueued first), then copies, on ctx's stream, into out
 * (caller-provided device doubles; may be NULL: the info only).  *info (may be
 * NULL) is always filled once the fit is known to be positive definite.
 *   UT_FIT_L         [npad][npad]: the lower triangle of the factor, zeros above
 *                    the diagonal.  info->l_rows: the leading rows whose
 *                    off-diagonal entries are L's -- npad after a refit; after
 *                    appends the first appended block row times 64 (their B
 *                    lives in scratch; the diagonal blocks beyond stay valid).
 *   UT_FIT_LINV      [npad][npad]: L^-1 as stored, upper triangle included.
 *   UT_FIT_LINVT     [npad][npad]: (L^-1)^T;  UT_FIT_ALPHA [npad].  While
 *                    info->stale is set (a precision-8 refit leaves both to
 *                    their first reader) nothing is copied and nothing computed.
 *   UT_FIT_BETA, UT_FIT_YS   [npad]: L^-1 ys and the standardised targets.
 *   UT_FIT_LINVT_F32 [npad][npad]: the f32 copy of (L^-1)^T, widened
 *                    (precision-32 fits; UT_EUNSUPPORTED otherwise).
 *   UT_FIT_I8A       [npad][npad] in (row, k) order: the six digit planes of
 *                    L^-1 decoded exactly to sum_p a_p 256^(5-p);
 *   UT_FIT_I8RS      [2 npad + 2]: [rs | e2 | E | Emu]  (precision-8 fits;
 *                    UT_EUNSUPPORTED otherwise).
 *   UT_FIT_H3        the f16x3 planes: always UT_EUNSUPPORTED.
 * Nothing is launched or recorded on the fit or scoring paths for this.
 * UT_EINVAL with no fit or an unknown operand; UT_ENOTPD after a fit that was
 * not positive definite. */
enum {
  UT_FIT_L = 0, UT_FIT_LINV = 1, UT_FIT_LINVT = 2, UT_FIT_ALPHA = 3, UT_FIT_BETA = 4, UT_FIT_YS = 5,
  UT_FIT_LINVT_F32 = 6, UT_FIT_I8A = 7, UT_FIT_I8RS = 8, UT_FIT_H3 = 9
};
typedef struct ut_gp_fit_info {
  int32_t n, npad;     /* training rows and their padded count */
  int32_t precision;   /* 64, 32, 16 or 8: the fit's */
  int32_t l_rows;      /* see UT_FIT_L */
  int32_t stale;       /* 1: (L^-1)^T and alpha are not written for this factor yet */
} ut_gp_fit_info;
int ut_gp_fit_read(ut_ctx* ctx, int32_t what, double* out, ut_gp_fit_info* info);
/* Dense DE rounds (ut_score_round_de) are lazy when K', the smallest power of
 * two >= 2k, is at most 1024 and less than m: only the K' best-scoring
 * candidates are hashed and deduplicated, which selects what hashing all m
 * would.  A round whose prefix holds fewer than k distinct new configurations
 * falls back, on the device, to hashing all m.  UT_LAZY_HASH=0 (read per
 * round) keeps every round eager.  The counts since ut_ctx_create; reading
 * fallback_rounds waits for the stream. */
int ut_round_lazy_stats(ut_ctx* ctx, int64_t* lazy_rounds, int64_t* fallback_rounds);

/* ---- tree-ensemble surrogate (the reference's own model family:
 *      plugins/xgbregressor.py:50-63, src/multi_stage.py:8-22) ------------- */
/* pred = (base + sum over trees of scale * leaf) / div, trees in order;
 * LE: go left iff (float)x <= threshold (sklearn), LT: iff (float)x < (float)threshold
 * (XGBoost); NaN features take default_left.  Leaves have feature < 0. */
enum { UT_SPLIT_LE = 0, UT_SPLIT_LT = 1 };
typedef struct ut_tree_node {
  int32_t feature;       /* GP feature column tested; < 0 = leaf */
  int32_t left, right;   /* child node indices (global in the node array) */
  int32_t default_left;  /* NaN goes left */
  double threshold;
  double value;          /* leaf value */
} ut_tree_node;
/* An ensemble with no tree, a root or child index outside [0, n_nodes), an
 * unknown rule or div == 0 is UT_EINVAL, and the ensemble loaded before stays
 * loaded.  The largest feature index of the splits is recorded. */
int ut_forest_set(ut_ctx* ctx, int32_t n_trees, const int32_t* roots_host, int64_t n_nodes,
                  const ut_tree_node* nodes_host, int32_t rule, double base, double scale, double div);
/* features [n_features][ld] (the layout ut_encode_features writes); pred and
 * score [m] may be NULL; score = sign * pred (sign -1: minimise), -inf where dup[i].
 * n_features must exceed the largest feature index the loaded ensemble splits
 * on: fewer columns than the model was trained on is UT_EINVAL (the message
 * names both numbers), never an answer read from another column. */
int ut_forest_predict(ut_ctx* ctx, const double* features, int64_t ld, int64_t m, int32_t n_features,
                      const uint8_t* dup, double sign, double* pred, double* score);
/* Predictive variance and acquisition of an AVERAGED ensemble (base 0, scale 1,
 * div = n_trees: a random forest, whose trees are samples of one function; the
 * reference scores its models by their mean alone, src/multi_stage.py:8-22,
 * plugins/xgbregressor.py:50-63 -- the variance over trees is SMAC's, Hutter,
 * Hoos & Leyton-Brown 2011).
 *
 * ut_forest_leaf_var, after ut_forest_set: the variance of the training
 * targets in every leaf (var_host[k] for node k; read at leaves only, where it
 * must be finite and >= 0, else UT_EINVAL and nothing changes; n_nodes must be
 * the loaded count).  ut_forest_set clears it.  Without it every leaf variance
 * is 0.  It lives in the leaf records' threshold field on the device, which
 * ut_forest_predict never reads. */
int ut_forest_leaf_var(ut_ctx* ctx, const double* var_host, int64_t n_nodes);
/* Tree t = 0..T-1 of candidate i ends in a leaf of value m_t and variance s_t;
 * every sum in tree order, in fp64, nothing fused:
 *   mu    = (base + sum m_t) / div            bitwise ut_forest_predict's pred
 *   a_t   = m_t - m_0                         shifted by the candidate's own first leaf
 *   D1 = sum a_t, D2 = sum a_t^2, SV = sum s_t
 *   var   = max((D2 + SV) / T - (D1 / T)^2, 0)     law of total variance over trees
 *   score = the acquisition of ut_gp_score at (mu, var, f_best) for the same
 *           ut_acq (EI: improvement below f_best; UCB: kappa sigma - mu);
 *           -inf where dup[i] != 0 (dup may be NULL)
 * mu, var, score [m] device outputs, each may be NULL; features, ld, n_features
 * and their UT_EINVAL cases as ut_forest_predict (the n_features message names
 * both numbers); a NULL acq or unknown kind is UT_EINVAL.  UT_EUNSUPPORTED
 * unless the loaded ensemble is an average (a boosted ensemble's stages are not
 * samples of one function).  m == 0 returns 0 and launches nothing.  Enqueued
 * on the context's stream with no host wait; the outputs do not depend on
 * which of the two kernels runs (UT_FOREST_STATS=lane|staged forces one, read
 * per call, for measurements). */
int ut_forest_score(ut_ctx* ctx, const double* features, int64_t ld, int64_t m, int32_t n_features,
                    const uint8_t* dup, const ut_acq* acq, double f_best, double* mu, double* var, double* score);

/* ---- multi-GPU exchange over RCCL -------------
 * One process per GPU, one communicator per context.  Rank r scores the
 * global candidate indices [r*m, (r+1)*m) of a round; population, training
 * set, GP factor and history set are replicated.  These calls replace the
 * reference's result exchange between its parallel_factor search instances
 * (python/uptune/api.py:400-401 creates them, :547-553 api.sync injects every
 * instance's results into the others; opentuner/api.py:87-104 TuningRunManager.sync).
 * Collectives are enqueued on the context's stream (ut_set_stream) with no
 * host wait, except ut_comm_bcast_results (it returns the broadcast count)
 * and ut_comm_barrier. */
#define UT_COMM_ID_BYTES 128
/* a fresh communicator id (rank 0 creates it; the caller hands the 128 bytes
 * to every rank, e.g. over torch.distributed's store) */
int ut_comm_unique_id(uint8_t* id_host);
/* join the communicator (blocks until all nranks ranks have joined); the
 * context's device is this rank's GPU */
int ut_comm_init(ut_ctx* ctx, int32_t rank, int32_t nranks, const uint8_t* id_host);
int ut_comm_destroy(ut_ctx* ctx);
int ut_comm_info(ut_ctx* ctx, int32_t* rank, int32_t* nranks);
/* the merged top-k of every rank's local top-k (all-gather + ut_topk_merge):
 * in: idx [k] (global, -1 = empty), score [k], digest [k][8], and optionally
 * the selected rows [ncols][ld_rows] (ncols = 0: none).  out: the merged
 * idx / score / digest [k] and rows [ncols][ld_out], identical on every rank
 * (any output may be NULL).  When a call needs larger record buffers than the
 * ranks last agreed on, every rank allocates and the ranks agree on success
 * (an all-reduce MIN) before the all-gather: an allocation failure on any
 * rank returns UT_ENOMEM on every rank, none is left inside the collective. */
int ut_comm_allgather_topk(ut_ctx* ctx, int32_t k, const int64_t* idx, const double* score, const uint32_t* digest,
                           const double* rows, int64_t ld_rows, int32_t ncols, int64_t* out_idx, double* out_score,
                           uint32_t* out_digest, double* out_rows, int64_t ld_out);
/* the merge alone, on n gathered records (no communicator needed): records
 * with idx < 0 or a NaN score are empty; among records with equal digests only
 * the smallest global index survives (a configuration proposed on two shards
 * is requested once); the k best survivors by (-score, idx) fill the output in
 * that order, empty slots get idx -1, score -inf, a zero digest and zero rows. */
int ut_topk_merge(ut_ctx* ctx, int64_t n, int32_t k, const int64_t* idx, const double* score, const uint32_t* digest,
                  const double* rows, int64_t ld_rows, int32_t ncols, int64_t* out_idx, double* out_score,
                  uint32_t* out_digest, double* out_rows, int64_t ld_out);
/* the per-round history delta from `root`: objective values y [n] and digests
 * [n][8] (device buffers of capacity `cap` on every rank).  The root's n goes
 * first, so every rank learns it (*n_out_host) and takes part in the payload
 * broadcast even when its own n differs; n > cap is UT_EINVAL after the
 * collective (rows beyond cap are dropped).  No rank is left inside a
 * collective when another fails: a root whose own arguments are bad sends a
 * sentinel count and every rank returns UT_EINVAL; the ranks agree on the
 * payload allocation before the payload broadcast (UT_ENOMEM on all). */
int ut_comm_bcast_results(ut_ctx* ctx, int32_t root, int64_t n, double* y, uint32_t* digest, int64_t cap,
                          int64_t* n_out_host);
/* raw broadcast of `bytes` bytes of a device buffer from `root` */
int ut_comm_bcast(ut_ctx* ctx, void* buf, int64_t bytes, int32_t root);
/* in-place all-reduce of n doubles (device buffer) */
enum { UT_RED_SUM = 0, UT_RED_MAX = 1, UT_RED_MIN = 2 };
int ut_comm_allreduce_f64(ut_ctx* ctx, double* buf, int64_t n, int32_t op);
/* every rank's stream reaches this point (an all-reduce, then a stream sync) */
int ut_comm_barrier(ut_ctx* ctx);
/* Fault injection for tests: the next `count` counted device allocations of
 * the context all fail with UT_ENOMEM (0 clears it).  Counted are the growths
 * of the context's scratch buffers and every array of the history table
 * (ut_history_reset and a growing ut_history_add allocate two: the keys, then
 * the slot states) and of ut_dedup's batch table.  A call stops at its first
 * failed allocation, so any count >= 1 fails the first array it needs. */
int ut_debug_fail_alloc(ut_ctx* ctx, int32_t count);
/* The same, after `skip` counted allocations have gone through: skip = 1,
 * count = 1 lets a history call obtain its keys array and fails the slot
 * states.  Replaces any injection set before; count = 0 clears it. */
int ut_debug_fail_alloc_after(ut_ctx* ctx, int32_t skip, int32_t count);

/* per-kernel device time (ms) of the ut_score_round_* calls since timing was
 * enabled with ut_set_timing(ctx, 1), averaged over those rounds.  Events are
 * recorded without host synchronisation; ut_stage_time synchronises once.  names: "propose", "hash",
 * "dedup", "encode", "gp_fit", "kstar", "var", "finalize", "topk" */
int ut_set_timing(ut_ctx* ctx, int32_t on);
int ut_stage_time(ut_ctx* ctx, const char* stage, double* ms);

#ifdef __cplusplus
}
#endif
#endif /* UTHOT_H */
