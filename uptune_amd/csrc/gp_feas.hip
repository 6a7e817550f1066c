// gp_feas.hip -- failure-aware scoring: EI weighted by a kernel vote over the
// results that succeeded and the configurations that failed (uthot.h
// "failure-aware scoring"):
//   k(a, u) = exp(-1/2 |(a - u) / ell|^2 / s^2)
//   S_ok(u) = sum_{r < n} k(x_r, u),  S_fail(u) = sum_{q < nf} k(f_q, u)
//   p(u)    = (S_ok + lambda p0) / (S_ok + S_fail + lambda),   score <- score p^gamma
// Both sums are one launch of the column-sum K* kernel (gp_kstar_sums.hip: no
// weights, the exponent scaled by 1 / s^2, the failed rows as its second row
// set), over operands the scoring call already has: the fit's scaled training
// operand (Xs^T, or its numeric block and the one-hot codes), the candidates'
// U', norms and codes in c->ucand / c->cnorm / c->bcat.  The failed rows get
// the same operands, built by the fit's own kernels once per fit
// (feas_operands).  part [RT_ok + RT_fail][ldk]: the training tiles' sums, then
// the failed ones'.
#include "gp_post.h"
#include "ut_internal.h"

#include <cmath>

namespace ut {

// One lane per candidate: the OK partials tile 0 upward, then the failed
// ones; p; the outputs asked for; a finite score times p^gamma.
__global__ void k_feas_apply(int64_t m, int32_t RT_ok, int32_t RT_fail, const double* __restrict__ part, int64_t ldp,
                             double lam_p0, double lam, double gamma, double* __restrict__ p_out,
                             double* __restrict__ s_ok_out, double* __restrict__ s_fail_out,
                             double* __restrict__ score) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const double s_ok = part_sum(part, RT_ok, ldp, i);
  const double s_fail = part_sum(part + (int64_t)RT_ok * ldp, RT_fail, ldp, i);
  const double p = (s_ok + lam_p0) / ((s_ok + s_fail) + lam);
  if (p_out) p_out[i] = p;
  if (s_ok_out) s_ok_out[i] = s_ok;
  if (s_fail_out) s_fail_out[i] = s_fail;
  if (score) {
    const double sc = score[i];
    // -inf (a duplicate) and NaN (a failed fit) pass through
    if (__builtin_isfinite(sc)) score[i] = sc * feas_factor(p, gamma);
  }
}

// The failed rows' K* operands under the current fit's lengthscales, by the
// kernels the fit builds its own with (so KSTAR_T_SCALE and the categorical
// conventions are theirs): rebuilt when the fit changed (fit_gen) or the rows
// did (ut_gp_feas_set zeroes fs_gen).  On c->stream, after the fit's 1/ell.
static int feas_operands(ut_ctx* c) {
  if (c->fs_n == 0 || c->fs_gen == c->fit_gen) return 0;
  const int32_t nf = c->fs_n, d = c->gp_d, nfpad = gp_npad(nf), dpad = kstar_dpad(d);
  int rc;
  if ((rc = ensure(c, c->fs_Xs, (size_t)nfpad * d))) return rc;
  if ((rc = ensure(c, c->fs_norm, (size_t)nfpad))) return rc;
  if ((rc = ensure(c, c->fs_XsT, (size_t)dpad * nfpad))) return rc;
  const bool cat = c->cat_on && c->fs_bad_row < 0;
  const int32_t dpn = cat_dpad(c);
  if (cat) {
    if ((rc = ensure(c, c->fs_XsT_num, (size_t)(dpn > 0 ? dpn : 1) * nfpad))) return rc;
    if ((rc = ensure(c, c->fs_norm_num, (size_t)nfpad))) return rc;
    if ((rc = ensure(c, c->fs_acat, (size_t)c->space.cat_k * nfpad))) return rc;
  }
  if ((rc = launch_gp_prep_train(c, c->fs_X.p, nf, nfpad, d, c->gp_inv_ell.p, c->fs_Xs.p, c->fs_norm.p))) return rc;
  if ((rc = launch_xs_t(c, c->fs_Xs.p, nfpad, d, dpad, c->fs_XsT.p))) return rc;
  if (cat && (rc = launch_gp_cat_train(c, c->fs_Xs.p, c->fs_X.p, nf, nfpad, d, dpn, c->fs_XsT_num.p,
                                       c->fs_norm_num.p, c->fs_acat.p)))
    return rc;
  c->fs_gen = c->fit_gen;
  return 0;
}

// The vote over the m candidates whose K* operands (shape s) are in c->ucand /
// c->cnorm / c->bcat -- or, given ops, in its arrays (pruned scoring's gathered
// columns; only the candidate padding differs from s) -- then k_feas_apply with
// the given outputs.
static int feas_vote(ut_ctx* c, const ScoreShape& s, int64_t m, double* p_out, double* s_ok_out, double* s_fail_out,
                     double* score, const CandOps* ops = nullptr) {
  const CandOps own{c->ucand.p, c->cnorm.p, c->bcat.p, s.ldk};
  const CandOps& u = ops ? *ops : own;
  const int32_t nf = c->fs_n;
  UT_CHECK(c, nf == 0 || c->fs_d == s.d, UT_EINVAL,
           "gp_feas: the failed rows have " + std::to_string(c->fs_d) + " features, the fit " + std::to_string(s.d));
  UT_CHECK(c, !(s.cat && nf > 0 && c->fs_bad_row >= 0), UT_EINVAL,
           "gp_feas: the fit scores with the categorical K* and failed row " + std::to_string(c->fs_bad_row) +
               " is not one-hot in an ENUM block / 0-1 in a BOOL column");
  const int64_t ldk = u.ld;
  int rc;
  if ((rc = feas_operands(c))) return rc;
  const int32_t nfpad = nf > 0 ? gp_npad(nf) : 0;
  const int32_t RT_ok = s.RT, RT_fail = nfpad / NPAD;
  if ((rc = ensure(c, c->fs_part, (size_t)(RT_ok + RT_fail) * ldk))) return rc;
  const KstarRowSet fail = s.cat ? KstarRowSet{c->fs_XsT_num.p, c->fs_norm_num.p, c->fs_acat.p, nullptr, nf, nfpad}
                                 : KstarRowSet{c->fs_XsT.p, c->fs_norm.p, nullptr, nullptr, nf, nfpad};
  const ut_feas_params& fp = c->fs_par;
  if ((rc = launch_kstar_sums(c, "gp_feas", s, u, m, nullptr, 0, fail, 1.0 / (fp.ell_scale * fp.ell_scale),
                              c->fs_part.p)))
    return rc;
  // the prior success rate: as given, or the share of successes among the rows in use
  const double p0 = fp.prior > 0.0 ? fp.prior : (double)s.n / (double)(s.n + nf);
  hipLaunchKernelGGL(k_feas_apply, dim3(grid1(m, 256)), dim3(256), 0, c->stream, m, RT_ok, RT_fail, c->fs_part.p, ldk,
                     fp.strength * p0, fp.strength, fp.power, p_out, s_ok_out, s_fail_out, score);
  UT_LAUNCH_CHECK(c);
  mark(c, "feas");
  return 0;
}

int feas_weight(ut_ctx* c, const ScoreShape& s, int64_t m, double* score) {
  return feas_vote(c, s, m, nullptr, nullptr, nullptr, score);
}

int feas_prob_cols(ut_ctx* c, const ScoreShape& s, const CandOps& ops, int64_t m, double* p_out) {
  return feas_vote(c, s, m, p_out, nullptr, nullptr, nullptr, &ops);
}

int gp_feas_prob_impl(ut_ctx* c, const double* values, const double* features, int64_t ld, int64_t m, double* p_out,
                      double* s_ok_out, double* s_fail_out) {
  UT_CHECK(c, m >= 0 && ld >= m && (values != nullptr) != (features != nullptr) && (p_out || m == 0), UT_EINVAL,
           "gp_feas_prob: bad arguments (exactly one of values and features, p_out required)");
  UT_CHECK(c, c->gp_ready, UT_EINVAL, "gp_feas_prob: call ut_gp_fit first");
  if (m == 0) return 0;
  int rc;
  if (values) {
    UT_CHECK(c, c->has_space, UT_ENOSPACE, "space not defined");
    UT_CHECK(c, c->gp_d == c->space.n_feat, UT_EINVAL, "gp_feas_prob: GP feature width != space feature width");
    // (flushes a staged fit and waits on the device for its scaled inputs)
    if ((rc = gp_encode_scaled(c, values, ld, m))) return rc;
    mark(c, "encode");
    return feas_vote(c, score_shape(c, m, c->cat_on && c->ucand_cat), m, p_out, s_ok_out, s_fail_out, nullptr);
  }
  if ((rc = gp_fit_flush(c))) return rc;
  if (c->fit_pending) UT_HIP(c, hipStreamWaitEvent(c->stream, c->ev_fit_x, 0));
  const ScoreShape s = score_shape(c, m, false);
  if ((rc = prep_cand_features(c, s, features, ld, m))) return rc;
  mark(c, "cnorm");
  return feas_vote(c, s, m, p_out, s_ok_out, s_fail_out, nullptr);
}

int gp_feas_set_impl(ut_ctx* c, const double* X, int32_t nf, int32_t d, const ut_feas_params* p) {
  UT_CHECK(c, nf >= 0, UT_EINVAL, "gp_feas_set: nf < 0");
  const ut_feas_params par = p ? *p : ut_feas_params{0.0, 1.0, 1.0, 1.0};
  if (nf > 0) {
    UT_CHECK(c, X != nullptr, UT_EINVAL, "gp_feas_set: Xfail_host is NULL");
    UT_CHECK(c, c->has_space, UT_ENOSPACE, "space not defined");
    UT_CHECK(c, d == c->space.n_feat, UT_EINVAL,
             "gp_feas_set: d = " + std::to_string(d) + ", the space has " + std::to_string(c->space.n_feat) +
                 " features");
    UT_CHECK(c, std::isfinite(par.strength) && par.strength > 0.0, UT_EINVAL,
             "gp_feas_set: strength must be finite and > 0");
    const double inv_s2 = 1.0 / (par.ell_scale * par.ell_scale);
    UT_CHECK(c, std::isfinite(par.ell_scale) && par.ell_scale > 0.0 && std::isnormal(inv_s2), UT_EINVAL,
             "gp_feas_set: ell_scale must be finite and > 0 (and 1 / ell_scale^2 a normal number)");
    UT_CHECK(c, std::isfinite(par.power) && par.power >= 0.0, UT_EINVAL, "gp_feas_set: power must be finite and >= 0");
    UT_CHECK(c, par.prior <= 1.0, UT_EINVAL, "gp_feas_set: prior must be <= 1 (<= 0: from the fit)");   // (NaN fails)
    for (size_t e = 0; e < (size_t)nf * d; ++e)
      UT_CHECK(c, std::isfinite(X[e]), UT_EINVAL,
               "gp_feas_set: row " + std::to_string(e / d) + " has a non-finite entry");
  }
  if (nf == 0) {
    // nothing is weighted from here on; the rows go once no kernel can be reading them
    UT_HIP(c, ut::sync_all(c));
    c->fs_X.reset();
    c->fs_n = 0, c->fs_d = 0, c->fs_bad_row = -1, c->fs_gen = 0;
    c->fs_par = ut_feas_params{0.0, 1.0, 1.0, 1.0};
    return 0;
  }
  // the first row the categorical K* could not read as option codes
  int32_t bad = -1;
  for (int32_t r = 0; r < nf && bad < 0; ++r)
    if (!cat_rows_ok(c->space, X, d, r, r + 1)) bad = r;
  // staged into a new array; what was loaded stays until it is complete
  DevBuf<double> q;
  int rc;
  if ((rc = dalloc(c, q, (size_t)nf * d))) return rc;
  UT_HIP(c, hipMemcpy(q.p, X, sizeof(double) * (size_t)nf * d, hipMemcpyHostToDevice));
  UT_HIP(c, ut::sync_all(c));   // an operand build enqueued earlier may still read the old rows
  c->fs_X.swap(q);
  c->fs_n = nf, c->fs_d = d, c->fs_bad_row = bad, c->fs_gen = 0;
  c->fs_par = par;
  return 0;
}

}  // namespace ut
