// gp_score.hip -- the dense GP posterior of a batch (the spec: gp_fit.hip).
// Score (per candidate, the MFMA-bound stage): both dense contractions are
//   C[n x m] = A[n x K] * B[K x m]
// with A small and row-major (L2/MALL resident) and B the candidate-major
// stream (columns = candidates, coalesced along m):
//   GEMM1: A = Xs [n x d],    B = U^T (features, [d][m]) -> K*^T  [n][m] + mu partials
//   GEMM2: A = L^-1 [n x n],  B = K*^T [n][m]  (lower-triangular A: K loop stops
//          at the tile's diagonal)  -> |L^-1 k*|^2 partials
// Both run in gp_gemm.hip (fp64 MFMA by default, fp32 MFMA when
// ut_gp_set_precision(ctx, 32); with 16 the variance GEMM runs as three fp16
// MFMA products of hi/lo split operands, fp32-class accuracy).
#include "gp_post.h"

namespace ut {

// mu, var and the score of column j (candidate i: its dup flag and outputs)
// from its row-tile partials, RT1 of the mean and RT2 of |v|^2: NaN after a
// failed fit, score -inf for a duplicate.
//
// Ebound: precision 8 (gp_i8.hip), |v|^2 and the mean mu = v . beta (beta = L^-1 y)
// from the int8 contraction's partials; a candidate is finished here only if
//   | |v|^2 - s | <= E (2 sqrt(s) + E) + s (2n + 64) 2^-53     (s = the computed sum)
// is at most tol * (sf2 - s) -- its variance is then within tol relative of the
// exact one -- and the mean's bound Emu = sum_r e_r |beta_r| (+ the fp64
// rounding of the sums, (2n + 64) 2^-53 |mu| |beta|-weighted, below Emu's own
// 2^-40 slack at these sizes) is at most tol * sigma: the mean within tol of
// the posterior's own scale.  Every other candidate (near a training point
// sf2 - |v|^2 cancels) returns true, for the fp64 recompute; its outputs are
// written anyway and overwritten there.  Neither a failed fit (nothing to
// recompute) nor a duplicate does.
__device__ __forceinline__ bool finalize_col(int64_t j, int64_t i, int32_t RT1, int32_t RT2,
                                             const double* __restrict__ mu_part, const double* __restrict__ var_part,
                                             int64_t ldp, const Acq& a, const uint8_t* __restrict__ dup,
                                             double* __restrict__ mu_out, double* __restrict__ var_out,
                                             double* __restrict__ score_out, const double* __restrict__ Ebound = nullptr,
                                             double tol = 0.0, int32_t n = 0) {
  double mu = part_sum(mu_part, RT1, ldp, j);
  const double vs = part_sum(var_part, RT2, ldp, j);
  double var = clamped_var(a.sf2, vs);
  bool flag = false;
  if (Ebound) {
    const double E = Ebound[0], Emu = Ebound[1];
    const double bound = E * (2.0 * sqrt(vs) + E) + vs * (double)(2 * n + 64) * 0x1p-53;
    flag = !(bound <= tol * var) || !(Emu <= tol * sqrt(var));   // (NaN: flagged)
  }
  double sc = a.score(mu, var);
  if (*a.fit_flag != 0) {  // failed (asynchronous) fit: nothing is selectable
    mu = var = sc = __builtin_nan("");
    flag = false;
  }
  if (dup && dup[i]) {
    // a duplicate of the history is a training point, where sf2 - |v|^2
    // cancels and the bound always fails: its score is -inf whatever the
    // variance, so it is not recomputed (its var output stays this tier's)
    sc = -1.0 / 0.0;
    flag = false;
  }
  if (mu_out) mu_out[i] = mu;
  if (var_out) var_out[i] = var;
  if (score_out) score_out[i] = sc;
  return flag;
}

// out_idx: column j is candidate out_idx[j] (precision 8's flagged candidates:
// their recomputed K* columns through the fp64 contraction); nullptr: candidate j
__global__ void k_gp_finalize(int64_t m, int32_t RT1, int32_t RT2, const double* __restrict__ mu_part,
                              const double* __restrict__ var_part, int64_t ldp, Acq a,
                              const uint8_t* __restrict__ dup, double* __restrict__ mu_out,
                              double* __restrict__ var_out, double* __restrict__ score_out,
                              const int64_t* __restrict__ out_idx) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= m) return;
  finalize_col(j, out_idx ? out_idx[j] : j, RT1, RT2, mu_part, var_part, ldp, a, dup, mu_out, var_out, score_out);
}

int launch_gp_finalize(ut_ctx* c, int64_t m, int32_t RT1, int32_t RT2, const double* mu_part, const double* var_part,
                       int64_t ldp, const Acq& a, const uint8_t* dup, double* mu, double* var, double* score,
                       const int64_t* out_idx) {
  hipLaunchKernelGGL(k_gp_finalize, dim3(grid1(m, 256)), dim3(256), 0, c->stream, m, RT1, RT2, mu_part, var_part, ldp,
                     a, dup, mu, var, score, out_idx);
  UT_LAUNCH_CHECK(c);
  return 0;
}

// precision 8: the candidates the acceptance test does not clear are appended
// to idx_out, one atomic per wave
__global__ void k_gp_finalize_i8(int64_t m, int32_t RT1, int32_t RT2, const double* __restrict__ mu_part,
                                 const double* __restrict__ var_part, int64_t ldp, Acq a,
                                 const uint8_t* __restrict__ dup, double* __restrict__ mu_out,
                                 double* __restrict__ var_out, double* __restrict__ score_out,
                                 const double* __restrict__ Ebound, double tol, int32_t n, int64_t* __restrict__ idx_out,
                                 unsigned long long* __restrict__ count) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const bool flag = i < m && finalize_col(i, i, RT1, RT2, mu_part, var_part, ldp, a, dup, mu_out, var_out, score_out,
                                          Ebound, tol, n);
  wave_append(flag, i, idx_out, count);
}

// the categorical K* codes of gathered candidates: 16-byte pieces of their
// 128-byte rows, code block blockIdx.y (zeros past n and for empty slots)
__global__ void k_gather_code_rows(const int8_t* __restrict__ bcat, int64_t ldk, const int64_t* __restrict__ idx,
                                   int64_t base, int64_t n, int64_t ldo, int8_t* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t kb = blockIdx.y;
  const int64_t j = e >> 3;
  const int piece = (int)(e & 7);
  if (j >= ldo) return;
  uint4 v = make_uint4(0u, 0u, 0u, 0u);
  if (j < n) {
    const int64_t q = idx[j];
    if (q >= 0) v = reinterpret_cast<const uint4*>(bcat + (kb * ldk + (q - base)) * 128)[piece];
  }
  reinterpret_cast<uint4*>(out + (kb * ldo + j) * 128)[piece] = v;
}

__global__ void k_gather_cols(const double* __restrict__ kst, int64_t ldk, const int64_t* __restrict__ idx,
                                  int64_t base, int64_t n, int64_t ldo, double* __restrict__ out) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  const int64_t r = blockIdx.y;
  if (j >= ldo) return;
  double v = 0.0;
  if (j < n) {
    const int64_t q = idx[j];
    if (q >= 0) v = kst[r * ldk + (q - base)];
  }
  out[r * ldo + j] = v;
}

// full fp64 K* columns of the candidates idx[0..nc) (global indices - base;
// idx < 0: an empty slot) into c->pr_kst [npad][ldc]: their scaled features
// and norms (and categorical codes) gathered from the K* operands of the
// round (c->ucand / c->cnorm / c->bcat, of shape s), then the K*
// GEMM on those columns only (pruned scoring's threshold set and survivors,
// precision 8's flagged candidates); mu_part: also their fp64 mean partials
// k* . alpha per row tile [RT][ldc] (pruned scoring's f32 bound pass)
int gather_kstar_cols(ut_ctx* c, const ScoreShape& s, const int64_t* idx, int64_t base, int64_t nc, int64_t ldc,
                      double* mu_part) {
  int r2;
  if ((r2 = ensure(c, c->pr_kst, (size_t)s.npad * ldc))) return r2;
  if ((r2 = ensure(c, c->pr_vpart, (size_t)s.RT * ldc))) return r2;
  if ((r2 = ensure(c, c->pr_ucand, s.urows() * ldc))) return r2;
  if ((r2 = ensure(c, c->pr_cnorm, (size_t)ldc))) return r2;
  if (s.dpad > 0)
    hipLaunchKernelGGL(k_gather_cols, dim3(grid1(ldc, 256), (unsigned)s.dpad), dim3(256), 0, c->stream, c->ucand.p,
                       s.ldk, idx, base, nc, ldc, c->pr_ucand.p);
  hipLaunchKernelGGL(k_gather_cols, dim3(grid1(ldc, 256), 1u), dim3(256), 0, c->stream, c->cnorm.p, s.ldk, idx, base,
                     nc, ldc, c->pr_cnorm.p);
  if (s.cat) {   // the gathered candidates' 128-byte code rows, per code block
    if ((r2 = ensure(c, c->pr_bcat, (size_t)c->space.cat_k * ldc))) return r2;
    hipLaunchKernelGGL(k_gather_code_rows, dim3(grid1(ldc * 8, 256), (unsigned)(c->space.cat_k / 128)), dim3(256), 0,
                       c->stream, c->bcat.p, s.ldk, idx, base, nc, ldc, c->pr_bcat.p);
  }
  UT_LAUNCH_CHECK(c);
  KstarArgs ka;
  ka.train = kstar_train(c, s.cat, c->pr_bcat.p);
  ka.ucand = c->pr_ucand.p, ka.dpad = s.dpad, ka.cn = c->pr_cnorm.p;
  ka.m = nc, ka.kst = c->pr_kst.p, ka.ldk = ldc, ka.part = mu_part;
  return launch_gemm_kstar(c, 64, s.npad, ka);
}

int gp_encode_scaled(ut_ctx* c, const double* values, int64_t ld, int64_t m) {
  UT_CHECK(c, c->gp_ready, UT_EINVAL, "gp_score: call ut_gp_fit first");
  if (m <= 0) return 0;
  int rc;
  if ((rc = gp_fit_flush(c))) return rc;
  // 1/ell comes with the fit's scaled training inputs
  if (c->fit_pending) UT_HIP(c, hipStreamWaitEvent(c->stream, c->ev_fit_x, 0));
  const ScoreShape s = score_shape(c, m, c->cat_on);
  if ((rc = ensure(c, c->cnorm, (size_t)s.ldk))) return rc;
  if ((rc = ensure(c, c->ucand, s.urows() * s.ldk))) return rc;
  if (s.cat) {   // numeric U', norms and the one-hot codes (categorical K*)
    if ((rc = ensure(c, c->bcat, (size_t)c->space.cat_k * s.ldk))) return rc;
    c->ucand_cat = true;
    return launch_encode_scaled_cat(c, values, ld, m, c->ucand.p, s.dpad, s.ldk, c->cnorm.p, c->bcat.p);
  }
  c->ucand_cat = false;
  return launch_encode_scaled(c, values, ld, m, c->ucand.p, s.dpad, s.ldk, c->cnorm.p);
}

// Precision 8's dense tail, from K* on: plan, K*, variance, the bound test, the
// call's one host sync (the flagged count and the K* counts that make the next
// call's hints), the fp64 recompute of the candidates the bound did not clear.
// ka: gp_score_dense's K* of all m candidates into c->kst (its fp64-MFMA
// kernels here and in the whole-round fallback).
static int gp_score_dense_i8(ut_ctx* c, const ScoreShape& s, int64_t m, const KstarArgs& ka, const Acq& pa,
                             const uint8_t* dup, double* mu, double* var, double* score, hipEvent_t dup_ready) {
  const int32_t npad = s.npad, RT = s.RT;
  const int64_t ldk = s.ldk;
  int rc;
  UT_CHECK(c, npad <= I8_MAX_K, UT_EINVAL, "gp_score: precision 8 takes at most 16384 training points");
  if ((rc = ensure(c, c->pr_idx, (size_t)ldk))) return rc;
  if ((rc = ensure(c, c->pr_count, 1))) return rc;
  // the distance contraction on the int8 MFMA (gp_kq.hip): beside the round's
  // hash its MFMAs issue under the hash's integer VALU work (C2 ~1 % per
  // round).  Categorical fits keep the fp64-MFMA K* (C3 HPL-64: K* 43 against
  // 28.5 ms, the round 288 against 270; C4 no better; scripts/r06_lines.sh),
  // which leaves no mask: the default plan
  const bool kq = c->kstar_q && !c->cat_on && c->gp_x8.p;
  const I8Plan plan = kq ? i8_plan(npad, kstar_q_k32(s.dpad), i8_env_read(), c->i8_hints) : I8Plan{};
  if (kq) rc = launch_gemm_kstar_q(c, plan, c->ucand.p, s.dpad, m, c->kst.p, ldk, c->u8, c->scol);
  else rc = launch_gemm_kstar(c, 8, npad, ka);
  if (rc) return rc;
  mark(c, "kstar");
  if (c->fit_pending) UT_HIP(c, hipStreamWaitEvent(c->stream, c->ev_fit, 0));
  // the variance GEMM starts when K* ends and the side stream's hash tail runs
  // beside it (only the finalize needs the dup mask): C2 16.60 -> 16.40 ms at
  // ell 0.2, 19.62 -> 19.36 at ell 2, C3 / C4 unchanged (their hash ends before
  // K*; scripts/ab/r06_varjoin*.sh, r06_sched.sh)
  mark(c, "var_wait");  // the wait for the fit is not variance time
  if ((rc = launch_gemm_var_i8(c, npad, reinterpret_cast<const int8_t*>(c->kst.p), ldk, m, c->var_part.p,
                               c->mu_part.p, plan.var)))
    return rc;
  mark(c, "var");
  if (dup_ready) UT_HIP(c, hipStreamWaitEvent(c->stream, dup_ready, 0));
  UT_HIP(c, hipMemsetAsync(c->pr_count.p, 0, sizeof(int64_t), c->stream));
  hipLaunchKernelGGL(k_gp_finalize_i8, dim3(grid1(m, 256)), dim3(256), 0, c->stream, m, 2 * RT, 2 * RT, c->mu_part.p,
                     c->var_part.p, ldk, pa, dup, mu, var, score, c->gp_i8rs.p + 2 * npad, c->i8_tol, s.n,
                     c->pr_idx.p, reinterpret_cast<unsigned long long*>(c->pr_count.p));
  UT_LAUNCH_CHECK(c);
  mark(c, "finalize");
  int64_t nf = 0;
  int32_t nsparse = 0, ksc[2] = {0, 0};   // ks_cnt[16], [17]: certified units, an unscreened mask's all-zero bytes
  UT_HIP(c, hipMemcpyAsync(&nf, c->pr_count.p, sizeof(int64_t), hipMemcpyDeviceToHost, c->stream));
  if (plan.mask)
    UT_HIP(c, hipMemcpyAsync(&nsparse, c->kmask_cnt.p, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  if (plan.screen || plan.count)
    UT_HIP(c, hipMemcpyAsync(ksc, c->ks_cnt.p + 16, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
  UT_HIP(c, hipStreamSynchronize(c->stream));
  I8Counts cnt;
  cnt.nsparse = nsparse, cnt.cert = plan.screen ? ksc[0] : 0, cnt.zero_bytes = plan.count ? ksc[1] : 0;
  cnt.blocks = (int64_t)(npad / 32) * (ldk / 32);
  c->i8_hints = i8_hints_next(c->i8_hints, plan, cnt);
  // most candidates need fp64: the whole K* (fp64, over the planes) and the
  // fp64 contraction, with the mean from its epilogue
  const bool whole = nf * 2 > m;
  c->i8_stats = I8Stats{plan.screen ? 1 : 0, cnt.cert, plan.mask ? cnt.blocks / 8 : 0, whole ? -1 : nf};
  if (nf > 0 && (rc = gp_ensure_linvt(c))) return rc;   // (the fp64 contraction reads (L^-1)^T)
  if (whole) {
    if ((rc = ensure(c, c->pr_mpart, (size_t)RT * ldk))) return rc;
    if ((rc = launch_gemm_kstar(c, 64, npad, ka))) return rc;
    if ((rc = launch_gemm_var64(c, npad, c->kst.p, ldk, npad, m, c->var_part.p))) return rc;
    if ((rc = launch_gp_finalize(c, m, RT, RT, c->pr_mpart.p, c->var_part.p, ldk, pa, dup, mu, var, score))) return rc;
  } else if (nf > 0) {
    const int64_t ldf = gp_ldk(nf);
    if ((rc = ensure(c, c->pr_mpart, (size_t)RT * ldf))) return rc;
    if ((rc = gather_kstar_cols(c, s, c->pr_idx.p, 0, nf, ldf))) return rc;
    if ((rc = launch_gemm_var64(c, npad, c->pr_kst.p, ldf, npad, nf, c->pr_vpart.p))) return rc;
    if ((rc = launch_gp_finalize(c, nf, RT, RT, c->pr_mpart.p, c->pr_vpart.p, ldf, pa, dup, mu, var, score,
                                 c->pr_idx.p)))
      return rc;
  }
  mark(c, "recompute");
  // the digit planes and their mask, or the fp64 rows the whole-round fallback wrote over them
  if (whole) c->kst_desc.set(64, npad, ldk, false);
  else c->kst_desc.set(8, npad, ldk, plan.mask);
  return 0;
}

// the dense posterior and acquisition of every tier (gp_score_impl below adds the feasibility weight)
static int gp_score_dense(ut_ctx* c, const double* feat, int64_t ld, int64_t m, const ut_acq* acq, const uint8_t* dup,
                          double* mu, double* var, double* score, hipEvent_t dup_ready) {
  UT_CHECK(c, c->gp_ready, UT_EINVAL, "gp_score: call ut_gp_fit first");
  UT_CHECK(c, acq != nullptr, UT_EINVAL, "gp_score: acq is NULL");
  if (m <= 0) return 0;
  c->kst_desc.invalidate();   // (set again where this call returns with K* in c->kst)
  if (int rc0 = gp_fit_flush(c)) return rc0;
  const int prec = c->gp_fit_prec;
  const bool fp32 = prec != 64;  // fp32, h3 (f16x3) and i8: K* stores a reduced-precision K*
  const bool i8 = prec == 8;
  // the mean in K*'s fp64 epilogue (k* . alpha, before k* is rounded): fp32 and h3
  const bool kmu = fp32 && !i8;
  // fp64 and i8: K* needs only the scaled training inputs (ev_fit_x) and the
  // mean comes from the variance epilogue, mu = (L^-1 k*) . (L^-1 y), so K*
  // overlaps the rest of an asynchronous fit and only the variance GEMM waits
  // for L^-1 (i8: |mu - mu^| <= Emu, gp_i8.hip).  fp32 / h3 keep the mean in
  // K*'s fp64 epilogue and wait for the whole fit.
  if (c->fit_pending) UT_HIP(c, hipStreamWaitEvent(c->stream, kmu ? c->ev_fit : c->ev_fit_x, 0));
  mark(c, "fit_wait");   // (the wait is not K* time)
  // the categorical K* when the candidates came through ut's encoder
  // (gp_encode_scaled in categorical mode); a caller's feature matrix takes the
  // dense contraction over every feature
  const ScoreShape s = score_shape(c, m, !feat && c->cat_on && c->ucand_cat);
  const int32_t npad = s.npad, RT = s.RT;
  const int64_t ldk = s.ldk;
  const Acq pa = make_acq(c, acq);
  int rc;
  if ((rc = ensure(c, c->kst, (size_t)npad * ldk))) return rc;
  // (i8: the variance and mean partials come per 64-row tile)
  if ((rc = ensure(c, c->mu_part, (size_t)(i8 ? 2 * RT : RT) * ldk))) return rc;
  if ((rc = ensure(c, c->var_part, (size_t)(i8 ? 2 * RT : RT) * ldk))) return rc;
  if (feat) {
    if ((rc = prep_cand_features(c, s, feat, ld, m))) return rc;
    mark(c, "cnorm");
  }
  // every K* of this call: all m candidates from c->ucand / c->cnorm into c->kst
  KstarArgs ka;
  ka.train = kstar_train(c, s.cat, c->bcat.p);
  ka.ucand = c->ucand.p, ka.dpad = s.dpad;
  ka.m = m, ka.kst = c->kst.p, ka.ldk = ldk;
  ka.part = kmu ? c->mu_part.p : nullptr;   // (i8's fp64 recompute: the mean from the variance epilogue)
  if (i8) return gp_score_dense_i8(c, s, m, ka, pa, dup, mu, var, score, dup_ready);
  if ((rc = launch_gemm_kstar(c, prec, npad, ka))) return rc;
  mark(c, "kstar");
  if (c->fit_pending && !kmu) UT_HIP(c, hipStreamWaitEvent(c->stream, c->ev_fit, 0));
  // the variance GEMM runs alone, the side stream's hash + dedup share the CUs
  // with K* only (C2: 27.95 -> 28.2 ms per round when they spilled into it, the
  // GEMM at 0.74 instead of 0.80 of peak; round 1); precision 8 joins them later
  if (dup_ready) UT_HIP(c, hipStreamWaitEvent(c->stream, dup_ready, 0));
  mark(c, "var_wait");  // the wait for the fit (and the dup mask) is not variance time
  if ((rc = launch_gemm_var(c, prec, fp32 ? (const void*)c->gp_LinvT_f.p : (const void*)c->gp_LinvT.p, npad, c->kst.p,
                            ldk, npad, m, c->var_part.p, fp32 ? nullptr : c->gp_beta.p,
                            fp32 ? nullptr : c->mu_part.p)))
    return rc;
  mark(c, "var");
  // h3's variance partials come per 256-row tile
  const int32_t RTv = prec == 16 ? (npad + 255) / 256 : RT;
  if ((rc = launch_gp_finalize(c, m, RT, RTv, c->mu_part.p, c->var_part.p, ldk, pa, dup, mu, var, score))) return rc;
  mark(c, "finalize");
  c->kst_desc.set(prec == 64 ? 64 : -1, npad, ldk, false);
  return 0;
}

// the weights are defined for EI only (dense scoring, and pruned scoring under ut_gp_set_prune_weighted)
int weights_refuse_ucb(ut_ctx* c, const ut_acq* acq, bool feas, bool cons) {
  UT_CHECK(c, !(feas && acq && acq->kind == UT_ACQ_UCB), UT_EUNSUPPORTED,
           "gp_score: failed rows are loaded (ut_gp_feas_set) and the feasibility weight is defined for EI only: "
           "a UCB score can be negative");
  UT_CHECK(c, !(cons && acq && acq->kind == UT_ACQ_UCB), UT_EUNSUPPORTED,
           "gp_score: constraint values are loaded (ut_gp_cons_set) and the constraint weight is defined for EI "
           "only: a UCB score can be negative");
  return 0;
}

// The single choke point of dense scoring (ut_gp_score, ut_gp_score_values,
// the DE and GA rounds, every precision tier and both of precision 8's
// recompute paths).  While failed rows are loaded (ut_gp_feas_set) the scores
// the dense body wrote are weighted by the feasibility vote (gp_feas.hip) over
// the K* operands it left in c->ucand / c->cnorm / c->bcat, categorical
// exactly when its K* was.  While constraint values are loaded
// (ut_gp_cons_set) the constrained-EI tail (gp_cons.hip) rewrites the scores
// first, from the posterior the dense body wrote (into context scratch where
// the caller asked for no mu or var): dense, constraint tail, vote.  While a
// second objective is loaded (ut_gp_mo_set; refused beside rows or values) the
// EHVI tail (gp_mo.hip) rewrites the scores in the constraint tail's place.
// With nothing loaded: no launch, no wait.
int gp_score_impl(ut_ctx* c, const double* feat, int64_t ld, int64_t m, const ut_acq* acq, const uint8_t* dup,
                  double* mu, double* var, double* score, hipEvent_t dup_ready) {
  const bool weigh = c->fs_n > 0 && score != nullptr;
  const bool cons = c->cs_nc > 0 && score != nullptr;
  // a second objective (ut_gp_mo_set; never beside rows or values): the EHVI tail (gp_mo.hip) in the same place
  const bool mo = c->mo_n > 0 && score != nullptr;
  int rc;
  if ((rc = weights_refuse_ucb(c, acq, weigh, cons))) return rc;
  if (mo && (rc = mo_check(c, "gp_score", acq))) return rc;
  if ((cons || mo) && m > 0) {
    if ((rc = cons_stale(c, "gp_score"))) return rc;
    const int64_t ldk = gp_ldk(m);
    if (!mu && (rc = ensure(c, c->cs_mu, (size_t)ldk))) return rc;
    if (!var && (rc = ensure(c, c->cs_var, (size_t)ldk))) return rc;
    if (!mu) mu = c->cs_mu.p;
    if (!var) var = c->cs_var.p;
  }
  rc = gp_score_dense(c, feat, ld, m, acq, dup, mu, var, score, dup_ready);
  if (rc || !(weigh || cons || mo) || m <= 0) return rc;
  const ScoreShape s = score_shape(c, m, !feat && c->cat_on && c->ucand_cat);
  if (mo) return mo_weight(c, s, m, mu, var, score);
  if (cons && (rc = cons_weight(c, s, m, acq->xi, mu, var, score))) return rc;
  return weigh ? feas_weight(c, s, m, score) : 0;
}

}  // namespace ut
