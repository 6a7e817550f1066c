// gp_prune.hip -- the top-k of a batch without every candidate's full variance.
// ---------------------------------------------------------------------------
// Selection-exact EI-bound pruning (ut_gp_topk_pruned).
//   var = sf2 - sum_r (L^-1 k*)_r^2 and every term is >= 0, so the partial
//   sum over the first R row tiles bounds var from above; EI (and UCB with
//   kappa >= 0) increases with sigma, so the same holds for the score.  The
//   R-tile partials are bitwise the first R partials of the full GEMM (same
//   tiles, same k order) and fp addition of non-negative terms and sf2 - x are
//   monotone, so var_exact <= var_bound holds in floating point too; the score
//   bound gets a 1e-12 relative margin for the acquisition's own rounding.
//
// Weighted (ut_gp_set_prune_weighted, with failed rows and / or constraint
// values loaded; EI only).  The score is S = (E P) p^gamma, E the EI at f_best_c
// (1 when no row is feasible), P = prod_j Phi((tau_j - mu_cj) / sigma), p the
// feasibility vote.  Every factor lies in [0, 1], and per candidate
//   ub_w  = ub_E prod_j Pub_j,
//   Pub_j = 1 where tau_j - mu_cj >= 0, else Phi((tau_j - mu_cj) / sqrt(var_ub))
// bounds S: Phi of a negative ratio rises with sigma and var <= var_ub holds
// bitwise (above); the vote gets no bound (factor 1).  mu_cj is exact for every
// candidate: k_kstar_sums runs once over the round's K* operands (fp64, at both
// passes) and the exact stage reads the same partials at the candidate's own
// index.  erfc is only nearly monotone in floating point, so the 1e-12 / 1e-300
// margin goes on after the product.  A bound keeps its exact flag only when the
// pass's own test pins var and the EI argument AND no failed rows are loaded;
// the stored double is then E P by the exact stage's own device function
// (PruneW::EP).  With failed rows loaded no candidate is flagged exact, so a
// flat GP (every score one double) keeps every candidate and falls back to the
// dense branch, which ends with cons_weight then feas_weight as gp_score_impl.
// ---------------------------------------------------------------------------
#include "gp_post.h"

#include <cstdlib>

namespace ut {

// The score bound of a candidate from the first RTv row tiles of the
// variance contraction.  The mean is exact (every row's k* went into it).
//   var_ub = sf2 - S_R, S_R = the sum of the first RTv partials; the score of
//   var_ub, raised by a 1e-12 relative margin for the rounding of the
//   acquisition function, bounds the exact score from above.
//   Exactness test: the rows past the bound contribute at most
//   T = sum_{r >= R} v_r^2 <= |L^-1|_F^2 |k*|^2 (|v_r| <= |L^-1_r| |k*|), the
//   computed partials at most 1.001 T, and the exact path's running sum starts
//   from the same S_R (its first RTv partials are bitwise these) and only adds
//   non-negative terms, so its var lies in [max(sf2 - S_hi, 0), var_ub] with
//   S_hi = (S_R + 1.001 T)(1 + 2^-40).  When both ends round to the same double
//   the exact var IS var_ub, and so is the exact score: it is stored without
//   the margin and flagged exact, and ties with it can be broken by index
//   (a flat GP -- every k* ~ 0 -- gives every candidate the same score).
// a bound's way out: NaN after a failed fit, -inf for a duplicate
__device__ __forceinline__ void store_bound(const Acq& a, const uint8_t* __restrict__ dup, int64_t i, double ub,
                                            bool exact, double* __restrict__ ub_out, uint8_t* __restrict__ exact_out) {
  if (*a.fit_flag != 0) {
    ub = __builtin_nan("");
    exact = false;
  }
  if (dup && dup[i]) ub = -1.0 / 0.0;
  ub_out[i] = ub;
  if (exact_out) exact_out[i] = exact ? 1 : 0;
}

__global__ void k_prune_bound(int64_t m, int32_t RTm, const double* __restrict__ mu_part, int32_t RTv,
                              const double* __restrict__ var_part, int64_t ldp, Acq a,
                              const uint8_t* __restrict__ dup, double* __restrict__ mu_out,
                              double* __restrict__ ub_out, const double* __restrict__ k2_part,
                              const double* __restrict__ linv_f2, uint8_t* __restrict__ exact_out, PruneW w) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const double mu = part_sum(mu_part, RTm, ldp, i);
  const double vs = part_sum(var_part, RTv, ldp, i);
  const double var = clamped_var(a.sf2, vs);
  double ub = a.score(mu, var);
  bool exact = false;
  if (k2_part && RTv < RTm) {
    const double k2 = part_sum(k2_part, RTm, ldp, i);
    const double tail = 1.001 * (*linv_f2) * k2;
    const double s_hi = (vs + tail) * (1.0 + 0x1p-40);
    const double var_lo = clamped_var(a.sf2, s_hi);
    exact = tail == tail && var_lo == var;   // (NaN tail: not exact)
  } else if (RTv >= RTm) {
    exact = true;   // the bound GEMM covered every row
  }
  if (w.on()) {
    exact = exact && !w.vote;
    ub = exact ? w.EP(ub, i, var) : w.EP_ub(ub, i, var);
  }
  if (!exact) ub = ub + fabs(ub) * 1e-12 + 1e-300;
  mu_out[i] = *a.fit_flag != 0 ? __builtin_nan("") : mu;
  store_bound(a, dup, i, ub, exact, ub_out, exact_out);
}

// The bound of the f32 pass (ut_gp_set_prune_pass 32, k_gp_kstar_f32c): the
// stored bound rows in fp64 as before, every other k*^ = sf2 2^t^ with |k*^ -
// k*| <= rho k*^ / (1 - rho) + 2^-125 sf2 (v_exp_f32 flushes below 2^-126), its
// f32 tile sums within 2^-19 of sum |alpha| k*^.  rho = 2^dt (1 + 2^-21) - 1 per
// candidate, dt = (Kc + 9) 2^-24 (2 |c0| + max_r |x_r|^2 + |u|^2) / ln 2 (log2
// units; Kc the contraction length, c0 the categorical offset; the f32
// contraction's bound, see k_gp_kstar_f32c).  Per candidate:
//   mean  |mu - mu^| <= dmu = (rho / (1 - rho) + 2^-19) S + 2^-125 sf2 sum|alpha|
//         + RT 2^-51 sum_rt |mu^_rt|: S = sum_r |alpha_r| k*^_r over the f32 rows (part3),
//         mu the fp64 k* . alpha the survivors are scored with (k_gp_kstar's
//         fp64 epilogue on their columns: its bound-row tile partials are these
//         bitwise, its other tiles within the first term; the last term the
//         different rounding of the two sums over tiles);
//   bound rows  exact k*: var <= var_ub = sf2 - |v^_R|^2 (as k_prune_bound);
//   lower end (rows past R: |L^-1|_F^2 |k*|^2 as k_prune_bound's tail)
//         var >= var_lo = sf2 - (|v^_R|^2 + 1.001 |L^-1|_F^2 ((1 + rho') |k*^| +
//         sqrt(n) 2^-125 sf2)^2);
// the score bound is the acquisition at (mu^ - dmu, var_ub), raised by
// k_prune_bound's 1e-12 margin -- unless both ends pin the exact score: var_lo
// == var_ub and the mean's two ends give the same I = f_best - mu - xi (EI) or
// the same score (UCB); then the exact score is that double, stored as is and
// flagged exact (a flat GP keeps its index tie-break).  fp64 rounding of the
// sums: a 2^-36 margin.  cst: [0] |L^-1|_F^2, [1 + SQ_BLOCKS] sum |alpha|,
// [2 + SQ_BLOCKS] max_r |x_r|^2.
constexpr int SQ_BLOCKS = 1024;
__global__ void k_prune_bound32(int64_t m, int32_t RTm, const double* __restrict__ mu_part,
                                const double* __restrict__ sa_part, const double* __restrict__ k2_part, int32_t RTv,
                                const double* __restrict__ var_part, int64_t ldp, Acq a, int32_t n,
                                const uint8_t* __restrict__ dup,
                                const double* __restrict__ cst, double* __restrict__ ub_out,
                                uint8_t* __restrict__ exact_out, int32_t Kc, double c0abs,
                                const double* __restrict__ cnorm, PruneW w) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const double sf2 = a.sf2;
  double mu = 0.0, mabs = 0.0, sa = 0.0, k2 = 0.0;
  for (int32_t r = 0; r < RTm; ++r) {
    const int64_t o = (int64_t)r * ldp + i;
    mu += mu_part[o];
    mabs += fabs(mu_part[o]);
    sa += sa_part[o];
    k2 += k2_part[o];
  }
  const double vs = part_sum(var_part, RTv, ldp, i);
  const double F2 = cst[0], A1 = cst[1 + SQ_BLOCKS];
  const double tiny = 0x1p-125 * sf2;
  const double dt = (Kc + 9.0) * 0x1p-24 * (2.0 * c0abs + cst[2 + SQ_BLOCKS] + cnorm[i]) * 1.4426950408889634 *
                        (1.0 + 0x1p-20) + Kc * 0x1p-120;
  const double rho = (exp2(dt) * (1.0 + 0x1p-21) - 1.0) * (1.0 + 0x1p-20) + 0x1p-50;
  const double rp = rho / (1.0 - rho);   // |k*^ - k*| / k*^ (rho < 1/2, or the bound is useless: NaN below)
  const double dmu = ((rp + 0x1p-19) * sa * (1.0 + 0x1p-18) + tiny * A1 + (double)RTm * 0x1p-51 * mabs) *
                     (1.0 + 0x1p-20);
  // (the bound rows' partials: bitwise the exact GEMM's first RTv, k_prune_bound)
  const double var_ub = clamped_var(sf2, vs);
  const double kn = (1.0 + rp) * sqrt(k2 * (1.0 + 0x1p-18)) + sqrt((double)n) * tiny;
  const double tail = 1.001 * F2 * kn * kn;
  const double var_lo = clamped_var(sf2, (vs + tail) * (1.0 + 0x1p-36));
  double ub = a.score(mu - dmu, var_ub);
  bool exact = var_lo == var_ub && dmu == dmu;
  if (exact && !w.no_ei()) {   // (no feasible row: the score has no EI factor to pin)
    if (a.kind == UT_ACQ_UCB)
      exact = ub == a.score(mu + dmu, var_lo);
    else
      exact = (a.stats[0] - (mu - dmu) - a.xi) == (a.stats[0] - (mu + dmu) - a.xi);
  }
  if (w.on()) {   // (the constraint means are fp64 and exact: no error term of this pass)
    exact = exact && !w.vote;
    ub = exact ? w.EP(ub, i, var_ub) : w.EP_ub(ub, i, var_ub);
  }
  if (!exact) ub = ub + fabs(ub) * 1e-12 + 1e-300;
  if (!(rho < 0.5)) {   // no usable bound: the candidate survives
    ub = 1.0 / 0.0;
    exact = false;
  }
  store_bound(a, dup, i, ub, exact, ub_out, exact_out);
}

// max of x[0 .. n) (one workgroup): the f32-contraction bound's max_r |x_r|^2
__global__ __launch_bounds__(256) void k_max_n(const double* __restrict__ x, int32_t n, double* __restrict__ out) {
  __shared__ double red[4];
  double v = 0.0;
  for (int32_t e = threadIdx.x; e < n; e += 256) v = fmax(v, x[e]);
  for (int d = 32; d > 0; d >>= 1) v = fmax(v, __shfl_xor(v, d, 64));
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
  __syncthreads();
  if (threadIdx.x == 0) *out = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
}

// sum of squares of cnt doubles (|L^-1|_F^2), deterministic: pass 1 writes one
// partial per block (grid-stride), pass 2 (one block) adds them in order
template <bool ABS>   // ABS: sum |x| instead
__global__ __launch_bounds__(256) void k_sumsq_part(const double* __restrict__ x, int64_t cnt,
                                                    double* __restrict__ part) {
  __shared__ double red[4];
  double s = 0.0;
  for (int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x; e < cnt; e += (int64_t)gridDim.x * 256)
    s += ABS ? fabs(x[e]) : x[e] * x[e];
  for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) part[blockIdx.x] = (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(256) void k_sumsq_final(const double* __restrict__ part, int32_t n,
                                                     double* __restrict__ out) {
  __shared__ double red[4];
  double s = 0.0;
  for (int32_t e = threadIdx.x; e < n; e += 256) s += part[e];
  for (int d = 32; d > 0; d >>= 1) s += __shfl_xor(s, d, 64);
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) *out = (red[0] + red[1]) + (red[2] + red[3]);
}

// exact scores of the gathered candidates: compact[j], and scattered to full[idx[j]]
// mu_full: the bound pass's exact mean by global index; or (nullptr) the fp64
// mean partials k* . alpha of these columns' K* (gather_kstar_cols: the f32
// bound pass has no exact mean)
// w: the weighted form, S = (E P) p^gamma in the dense order -- the constraint
// means by global index as mu_full, p_vote[j] the vote of gathered column j
__global__ void k_prune_exact(int64_t n, const int64_t* __restrict__ idx, int64_t base, int32_t RT,
                              const double* __restrict__ var_part, int64_t ldp, const double* __restrict__ mu_full,
                              Acq a, double* __restrict__ compact, double* __restrict__ full,
                              const double* __restrict__ mu_part, PruneW w, const double* __restrict__ p_vote) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const int64_t q = idx[j];
  if (q < 0) {
    if (compact) compact[j] = -1.0 / 0.0;
    return;
  }
  const double vs = part_sum(var_part, RT, ldp, j);
  const double mu = mu_full ? mu_full[q - base] : part_sum(mu_part, RT, ldp, j);
  const double var = clamped_var(a.sf2, vs);
  double sc = a.score(mu, var);
  if (w.on()) {
    sc = w.EP(sc, q - base, var);
    if (w.vote) sc = sc * feas_factor(p_vote[j], w.gamma);
  }
  if (*a.fit_flag != 0) sc = __builtin_nan("");
  if (compact) compact[j] = sc;
  if (full) full[q - base] = sc;
}

// survivors: candidates that may be in the top-k (appended with one atomic per
// wave; tau and its index are device scalars).  An exact candidate (its
// stored score is its exact score) survives iff (score, -index) >= (tau,
// -tau_index), the k-th best pair of the threshold set -- a lower bound on the
// k-th best pair overall; any other survives iff its bound >= tau.  A threshold
// set with fewer than k valid entries (m < k, or nearly every candidate a
// duplicate) has no k-th best pair: its slot is an invalid entry (index < 0)
// whose stored score means nothing (0 for the sort's padding, -inf for a
// duplicate), so tau is -inf and nothing is pruned.
__global__ void k_prune_survivors(int64_t m, const double* __restrict__ ub, const double* __restrict__ tau_p,
                                  const int64_t* __restrict__ tau_idx_p, const uint8_t* __restrict__ exact,
                                  int64_t cand_base, int64_t* __restrict__ out, unsigned long long* __restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t tau_g = *tau_idx_p;
  const double tau = tau_g < 0 ? -1.0 / 0.0 : *tau_p;
  bool keep = false;
  if (i < m) {
    const double b = ub[i];
    if (exact && exact[i])
      keep = b > tau || (b == tau && (tau_g < 0 || cand_base + i <= tau_g));
    else
      keep = b >= tau;
  }
  wave_append(keep, i, out, count);
}

__global__ void k_fill(double* __restrict__ p, int64_t n, double v) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < n) p[i] = v;
}

int gp_topk_pruned_impl(ut_ctx* c, const double* feat, int64_t ld, int64_t m, const ut_acq* acq, const uint8_t* dup,
                        int64_t cand_base, int32_t k, int32_t bound_rows, int64_t* out_idx, double* out_score,
                        ut_prune_stats* stats, hipEvent_t dup_ready) {
  c->pr_m = 0;   // (set again once this call's bounds are enqueued)
  UT_CHECK(c, c->gp_ready, UT_EINVAL, "gp_topk_pruned: call ut_gp_fit first");
  UT_CHECK(c, c->gp_fit_prec == 64, UT_EINVAL, "gp_topk_pruned: needs an fp64 fit (ut_gp_set_precision 64)");
  UT_CHECK(c, acq->kind == UT_ACQ_EI || (acq->kind == UT_ACQ_UCB && acq->kappa >= 0.0), UT_EINVAL,
           "gp_topk_pruned: the score must increase with sigma (EI, or UCB with kappa >= 0)");
  UT_CHECK(c, k >= 1 && k <= 1024, UT_EINVAL, "gp_topk_pruned: k must be in [1, 1024]");
  // the weighted form (ut_gp_set_prune_weighted; the entry points refuse loaded rows / values without it)
  const bool wv = c->prune_weighted && c->fs_n > 0, wc = c->prune_weighted && c->cs_nc > 0;
  if (int rc0 = weights_refuse_ucb(c, acq, wv, wc)) return rc0;
  if (wc)
    if (int rc0 = cons_stale(c, "gp_topk_pruned")) return rc0;
  if (int rc0 = gp_fit_flush(c)) return rc0;
  // the candidates' K* operands need only the fit's scaled inputs (1/ell):
  // they are prepared while the factorisation still runs, and K* then waits
  // for the whole fit (C3 pruned: the 2.8-ms categorical prep came off the
  // critical path, scripts/ab/r04ad_prep_early.sh)
  if (c->fit_pending) UT_HIP(c, hipStreamWaitEvent(c->stream, c->ev_fit_x, 0));
  // feat == nullptr: the K* operands are already in c->ucand / c->cnorm (/ c->bcat),
  // from gp_encode_scaled (a scoring round's fused encode, the only maker of the
  // categorical K*'s operands); a feature matrix takes the dense contraction
  const bool cat = !feat && c->ucand_cat;
  const ScoreShape s = score_shape(c, m, cat);
  const int32_t n = s.n, npad = s.npad, dpad = s.dpad, RT = s.RT;
  const int64_t ldk = s.ldk;
  int32_t R = gp_npad(bound_rows) / NPAD;
  R = R < 1 ? 1 : (R > RT ? RT : R);
  Acq pa = make_acq(c, acq);
  int rc;
  if (wv && (rc = ensure(c, c->pr_p, (size_t)ldk))) return rc;
  c->kst_desc.invalidate();   // (c->kst becomes this call's bound rows: nothing ut_gp_kstar_read reads)
  if ((rc = ensure(c, c->kst, (size_t)npad * ldk))) return rc;
  if ((rc = ensure(c, c->mu_part, (size_t)RT * ldk))) return rc;
  if ((rc = ensure(c, c->var_part, (size_t)RT * ldk))) return rc;
  if ((rc = ensure(c, c->pr_mpart, (size_t)RT * ldk))) return rc;
  if (cat && (rc = ensure(c, c->bcat, (size_t)c->space.cat_k * ldk))) return rc;
  if ((rc = ensure(c, c->pr_mu, (size_t)ldk))) return rc;
  if ((rc = ensure(c, c->pr_ub, (size_t)ldk))) return rc;
  if ((rc = ensure(c, c->pr_score, (size_t)ldk + 2048))) return rc;   // + the threshold set's two [1024] arrays
  if ((rc = ensure(c, c->pr_idx, (size_t)ldk + 2048))) return rc;
  if ((rc = ensure(c, c->pr_count, 1))) return rc;
  if ((rc = ensure(c, c->pr_k2, (size_t)RT * ldk))) return rc;
  // [0] |L^-1|_F^2, [1..] block partials, then the f32 passes' sum |alpha|, max |x|^2
  if ((rc = ensure(c, c->pr_f2, 3 + SQ_BLOCKS))) return rc;
  const bool f32 = c->prune_pass == 32;   // the bound pass in f32 (k_gp_kstar_f32c)
  if (f32 && (rc = ensure(c, c->pr_sa, (size_t)RT * ldk))) return rc;
  if (f32 && (rc = ensure(c, c->pr_gmu, (size_t)RT * (ldk + 1024)))) return rc;   // survivors / threshold set
  if ((rc = ensure(c, c->pr_exact, (size_t)ldk))) return rc;
  // 1. K* with the mean in its epilogue, 2. the first R row tiles of L^-1 K*^T
  if (feat) {
    if ((rc = prep_cand_features(c, s, feat, ld, m))) return rc;
    mark(c, "prep");
  }
  if (c->fit_pending) UT_HIP(c, hipStreamWaitEvent(c->stream, c->ev_fit, 0));   // K* takes mu = k* . alpha
  mark(c, "fit_wait");   // (the wait is not K* time)
  // every K* of this call over all m candidates: c->ucand / c->cnorm into
  // c->kst, the mean k* . alpha in its epilogue
  KstarArgs ka;
  ka.train = kstar_train(c, cat, c->bcat.p);
  ka.ucand = c->ucand.p, ka.dpad = dpad;
  ka.m = m, ka.kst = c->kst.p, ka.ldk = ldk, ka.part = c->mu_part.p;
  // K* stores only the bound rows; the mean sums every row.  The few
  // candidates that need every row (threshold set, survivors) get their K*
  // columns recomputed from their features (gather_kstar_cols below): cheaper than
  // writing and re-reading the whole n x m matrix
  KstarArgs kb = ka;
  kb.store_rows = R * NPAD, kb.part2 = c->pr_k2.p;
  if (f32) {
    // the bound rows through the fp64 kernel (tiles < R), every other tile
    // through k_gp_kstar_f32c on f32 copies of the operands (Xs^T once per fit)
    const double* xnn = ka.train.xnorm ? ka.train.xnorm : c->gp_xnorm.p;
    // the f32 copy depends on the operand as well as the fit: the numeric
    // block (categorical mode, cat_dpad rows, gp_xnorm_num) or every feature
    // (kstar_dpad rows, gp_xnorm) -- within one categorical fit the feature
    // entry (ut_gp_topk_pruned: cat = false) and the fused DE round (cat =
    // true) take different ones, so the cache is keyed on (fit, cat, dpad)
    if (c->pr_xf_gen != c->fit_gen || c->pr_xf_cat != cat || c->pr_xf_dpad != dpad) {
      if ((rc = ensure(c, c->pr_xsT_f, (size_t)dpad * npad))) return rc;
      if ((rc = launch_to_f32(c, ka.train.XsT, c->pr_xsT_f.p, (int64_t)dpad * npad))) return rc;
      hipLaunchKernelGGL(k_max_n, dim3(1), dim3(256), 0, c->stream, xnn, n, c->pr_f2.p + 2 + SQ_BLOCKS);
      UT_LAUNCH_CHECK(c);
      c->pr_xf_gen = c->fit_gen;
      c->pr_xf_cat = cat;
      c->pr_xf_dpad = dpad;
    }
    if ((rc = ensure(c, c->pr_ucand_f, s.urows() * ldk))) return rc;
    if ((rc = launch_to_f32(c, c->ucand.p, c->pr_ucand_f.p, (int64_t)dpad * ldk))) return rc;
    KstarArgs kf = kb;   // the tiles from R on: their mean, |k*|^2 and sum |alpha| k* partials
    kf.rt0 = R, kf.part3 = c->pr_sa.p;
    kb.row_tiles = R;
    if ((rc = launch_gemm_kstar(c, 64, npad, kb))) return rc;
    UT_HIP(c, hipMemsetAsync(c->pr_sa.p, 0, sizeof(double) * R * ldk, c->stream));
    if (R < RT && (rc = launch_gemm_kstar_f32c(c, c->pr_xsT_f.p, c->pr_ucand_f.p, npad, kf))) return rc;
  } else if ((rc = launch_gemm_kstar(c, 64, npad, kb))) {
    return rc;
  }
  // |L^-1|_F^2 for the variance tail bound, once per fit (the block partials
  // in pr_f2[1..] are scratch, reused pass after pass in stream order)
  auto sumsq = [&](bool abs_, const double* x, int64_t cnt, double* out) -> int {
    hipLaunchKernelGGL(abs_ ? k_sumsq_part<true> : k_sumsq_part<false>, dim3(SQ_BLOCKS), dim3(256), 0, c->stream, x,
                       cnt, c->pr_f2.p + 1);
    hipLaunchKernelGGL(k_sumsq_final, dim3(1), dim3(256), 0, c->stream, c->pr_f2.p + 1, SQ_BLOCKS, out);
    UT_LAUNCH_CHECK(c);
    return 0;
  };
  if (c->pr_f2_gen != c->fit_gen) {
    if ((rc = sumsq(false, c->gp_Linv.p, (int64_t)npad * npad, c->pr_f2.p))) return rc;
    c->pr_f2_gen = c->fit_gen;
  }
  if (f32 && c->pr_ab_gen != c->fit_gen) {   // the f32 bound's per-fit constants
    double* cst = c->pr_f2.p + 1 + SQ_BLOCKS;
    if ((rc = sumsq(true, c->gp_alpha.p, n, cst))) return rc;
    c->pr_ab_gen = c->fit_gen;
  }
  mark(c, "kstar");
  if (wc) {   // mu_cj of every candidate, once, over the same operands (fp64 at both passes)
    if ((rc = cons_means(c, s, m))) return rc;
    mark(c, "cons");
    pa = make_acq_cons(c, acq);   // (f_best_c lives in cs_stats, which cons_means may just have allocated)
  }
  // UT_PRUNE_WEIGHT_BOUND=0 (scripts/prune_weight_bench.py): Pub_j = 1, the EI bound alone -- still a bound
  const char* pub_env = getenv("UT_PRUNE_WEIGHT_BOUND");
  const PruneW pw{wc ? c->cs_nc : 0, RT, c->cs_part.p, ldk, c->cs_stats.p, c->gp_sf2, wv ? 1 : 0, c->fs_par.power,
                  pub_env && atoi(pub_env) == 0 ? 0 : 1};
  // the vote of gathered columns (threshold set, survivors), from their gathered operands
  auto vote = [&](int64_t cnt, int64_t ldc) -> int {
    return wv ? feas_prob_cols(c, s, CandOps{c->pr_ucand.p, c->pr_cnorm.p, c->pr_bcat.p, ldc}, cnt, c->pr_p.p) : 0;
  };
  if ((rc = launch_gemm_var64(c, npad, c->kst.p, ldk, R * NPAD, m, c->var_part.p))) return rc;
  mark(c, "bound");
  if (dup_ready) UT_HIP(c, hipStreamWaitEvent(c->stream, dup_ready, 0));   // the dup mask (side stream)
  if (f32)
    hipLaunchKernelGGL(k_prune_bound32, dim3(grid1(m, 256)), dim3(256), 0, c->stream, m, RT, c->mu_part.p,
                       c->pr_sa.p, c->pr_k2.p, R, c->var_part.p, ldk, pa, n, dup, c->pr_f2.p, c->pr_ub.p,
                       c->pr_exact.p, dpad + (cat ? 1 : 0), cat ? fabs(c->cat_c0) : 0.0, c->cnorm.p, pw);
  else
    hipLaunchKernelGGL(k_prune_bound, dim3(grid1(m, 256)), dim3(256), 0, c->stream, m, RT, c->mu_part.p, R,
                       c->var_part.p, ldk, pa, dup, c->pr_mu.p, c->pr_ub.p, c->pr_k2.p, c->pr_f2.p, c->pr_exact.p, pw);
  UT_LAUNCH_CHECK(c);
  c->pr_m = m;   // pr_ub / pr_exact hold this call's bounds (ut_gp_prune_bounds)
  // 3. threshold: exact scores of the best 1024 bounds, tau = their k-th best
  const int32_t kp = (int32_t)(m < 1024 ? m : 1024);
  int64_t* tset = c->pr_idx.p + ldk;                   // [1024] threshold set (global indices)
  double* tsc = c->pr_score.p + ldk;                   // [1024] their bounds
  double* tex = c->pr_score.p + ldk + 1024;            // [1024] their exact scores
  if ((rc = topk_impl(c, c->pr_ub.p, dup, m, cand_base, kp < k ? k : kp, tset, tsc))) return rc;
  // (the f32 pass has no exact mean: the recomputed columns' fp64 k* . alpha)
  double* gmu = f32 ? c->pr_gmu.p : nullptr;
  const int64_t ldt = gp_ldk(kp);
  if ((rc = gather_kstar_cols(c, s, tset, cand_base, kp, ldt, gmu))) return rc;
  if ((rc = launch_gemm_var64(c, npad, c->pr_kst.p, ldt, npad, kp, c->pr_vpart.p))) return rc;
  if ((rc = vote(kp, ldt))) return rc;
  const double* mu_full = f32 ? nullptr : c->pr_mu.p;
  hipLaunchKernelGGL(k_prune_exact, dim3(grid1(kp, 256)), dim3(256), 0, c->stream, (int64_t)kp, tset, cand_base, RT,
                     c->pr_vpart.p, ldt, mu_full, pa, tex, nullptr, gmu, pw, c->pr_p.p);
  UT_LAUNCH_CHECK(c);
  int64_t* tk_i = out_idx;   // the caller's [k] outputs hold tau's top-k for now
  double* tk_s = out_score;
  // tau: the k-th best (exact score, global index) pair of the threshold set
  if ((rc = topk_pairs_impl(c, tex, tset, kp, k, tk_i, tk_s))) return rc;
  // 4. survivors: bound >= tau
  UT_HIP(c, hipMemsetAsync(c->pr_count.p, 0, sizeof(int64_t), c->stream));
  hipLaunchKernelGGL(k_prune_survivors, dim3(grid1(m, 256)), dim3(256), 0, c->stream, m, c->pr_ub.p, tk_s + (k - 1),
                     tk_i + (k - 1), c->pr_exact.p, cand_base, c->pr_idx.p,
                     reinterpret_cast<unsigned long long*>(c->pr_count.p));
  UT_LAUNCH_CHECK(c);
  int64_t ns = 0, tau_g = -1;
  double tau = 0.0;
  UT_HIP(c, hipMemcpyAsync(&ns, c->pr_count.p, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  UT_HIP(c, hipMemcpyAsync(&tau, tk_s + (k - 1), sizeof(double), hipMemcpyDeviceToHost, c->stream));
  UT_HIP(c, hipMemcpyAsync(&tau_g, tk_i + (k - 1), sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  UT_HIP(c, hipStreamSynchronize(c->stream));
  if (tau_g < 0) tau = -1.0 / 0.0;   // no k-th best pair (k_prune_survivors)
  mark(c, "prune");
  const bool dense = ns * 2 > m;
  if (dense) {
    // most candidates survive: the whole K* (this time every row) and the dense variance
    if ((rc = launch_gemm_kstar(c, 64, npad, ka))) return rc;
    if ((rc = launch_gemm_var64(c, npad, c->kst.p, ldk, npad, m, c->var_part.p))) return rc;
    // (weighted: the plain EI first, then the dense path's own tails in its order)
    if (wc && (rc = ensure(c, c->cs_mu, (size_t)ldk))) return rc;
    if (wc && (rc = ensure(c, c->cs_var, (size_t)ldk))) return rc;
    if ((rc = launch_gp_finalize(c, m, RT, RT, c->mu_part.p, c->var_part.p, ldk, make_acq(c, acq), dup,
                                 wc ? c->cs_mu.p : nullptr, wc ? c->cs_var.p : nullptr, c->pr_score.p)))
      return rc;
    if (wc || wv) mark(c, "var");   // (the tails mark their own stages: cons, feas)
    if (wc && (rc = cons_weight(c, s, m, acq->xi, c->cs_mu.p, c->cs_var.p, c->pr_score.p))) return rc;
    if (wv && (rc = feas_weight(c, s, m, c->pr_score.p))) return rc;
  } else {
    // 5. the full variance for the survivors only, their exact scores into a -inf array
    hipLaunchKernelGGL(k_fill, dim3(grid1(m, 256)), dim3(256), 0, c->stream, c->pr_score.p, m, -1.0 / 0.0);
    UT_LAUNCH_CHECK(c);
    if (ns > 0) {
      const int64_t lds = gp_ldk(ns);
      if ((rc = gather_kstar_cols(c, s, c->pr_idx.p, 0, ns, lds, gmu))) return rc;
      if ((rc = launch_gemm_var64(c, npad, c->pr_kst.p, lds, npad, ns, c->pr_vpart.p))) return rc;
      if ((rc = vote(ns, lds))) return rc;
      hipLaunchKernelGGL(k_prune_exact, dim3(grid1(ns, 256)), dim3(256), 0, c->stream, ns, c->pr_idx.p, (int64_t)0,
                         RT, c->pr_vpart.p, lds, mu_full, pa, nullptr, c->pr_score.p, gmu, pw, c->pr_p.p);
      UT_LAUNCH_CHECK(c);
    }
  }
  mark(c, "var");
  if ((rc = topk_impl(c, c->pr_score.p, dup, m, cand_base, k, out_idx, out_score))) return rc;
  mark(c, "topk");
  if (stats) {
    stats->survivors = dense ? m : ns;
    stats->bound_rows = R * NPAD;
    stats->dense = dense ? 1 : 0;
    stats->threshold = tau;
  }
  return 0;
}

}  // namespace ut
