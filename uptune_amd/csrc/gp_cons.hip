// gp_cons.hip -- constrained EI (uthot.h "constrained EI"): up to UT_CONS_MAX
// measured constraints c_j(x) <= t_j as further GP targets on the fit's own
// factor.  With the same inputs, kernel and hyperparameters a second target
// shares L and L^-1; it needs only
//   alpha_j = K^-1 chat_j = L^-T (L^-1 chat_j)
// and its posterior mean mu_cj(u) = k*(u) . alpha_j is the K* contraction over
// the training rows with a weighted epilogue (the column-sum K* kernel,
// gp_kstar_sums.hip, with alpha_j as the rows' weights); its variance is the
// objective's.
//   P(u)     = prod_j Phi((tau_j - mu_cj(u)) / sqrt(var(u)))
//   score(u) = EI(mu, var; f_best_c, xi) P(u),  f_best_c = min ys over the feasible rows
// (P(u) alone when no row is feasible).  The operands (chat, beta, alpha, tau,
// f_best_c) are a per-fit cache built by small fp64 kernels after the whole fit;
// the hot kernel is k_kstar_sums.
#include "gp_post.h"
#include "ut_internal.h"

#include <cmath>
#include <cstring>

namespace ut {

// One lane per candidate: mu_cj = sigma_f2 * its partials tile 0 upward, P_j, P
// (j ascending); the outputs asked for; a finite score becomes
// EI(mu, var; f_best_c, xi) P, or P when no row is feasible.
// st: cs_stats -- [4 j + 3] = tau_j, [CS_INFO] = f_best_c, [CS_INFO + 1] = n_feasible
__global__ void k_cons_apply(int64_t m, int32_t RT, int32_t nc, const double* __restrict__ part, int64_t ldp,
                             double sf2, const double* __restrict__ st, const double* __restrict__ mu,
                             const double* __restrict__ var, double xi, double* __restrict__ p_out,
                             double* __restrict__ mu_c_out, int64_t ldo, double* __restrict__ score) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const double v = var[i];
  const double sigma = sqrt(v);
  double P = 1.0;
  for (int32_t j = 0; j < nc; ++j) {
    const double mc = sf2 * part_sum(part + (int64_t)j * ldp, RT, (int64_t)nc * ldp, i);
    const double tau = st[4 * j + 3];
    P *= cons_prob1(mc, tau, v, sigma);
    if (mu_c_out) mu_c_out[(int64_t)j * ldo + i] = mc;
  }
  if (p_out) p_out[i] = P;
  if (score) {
    const double sc = score[i];
    // -inf (a duplicate) and NaN (a failed fit) pass through
    if (__builtin_isfinite(sc))
      score[i] = st[CS_INFO + 1] > 0.0 ? acq_score(UT_ACQ_EI, mu[i], v, st[CS_INFO], xi, 0.0) * P : P;
  }
}

// tau_j = (t_j - m_j) / s_j beside column j's stats; the feasible rows (every
// raw value <= its threshold): their count and the smallest standardised
// objective among them (NaN when there is none).  One workgroup.
__global__ __launch_bounds__(256) void k_cons_scan(const double* __restrict__ C, const double* __restrict__ thr,
                                                   int32_t n, int32_t npad, int32_t nc, const double* __restrict__ ys,
                                                   double* __restrict__ st) {
  __shared__ double rmin[256];
  __shared__ int32_t rcnt[256];
  const int t = threadIdx.x;
  double mn = 1.0 / 0.0;
  int32_t cnt = 0;
  for (int32_t r = t; r < n; r += 256) {
    bool ok = true;
    for (int32_t j = 0; j < nc; ++j) ok = ok && C[(int64_t)j * npad + r] <= thr[j];
    if (ok) {
      ++cnt;
      const double v = ys[r];
      mn = v < mn ? v : mn;
    }
  }
  rmin[t] = mn;
  rcnt[t] = cnt;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) {
      rmin[t] = rmin[t + w] < rmin[t] ? rmin[t + w] : rmin[t];
      rcnt[t] += rcnt[t + w];
    }
    __syncthreads();
  }
  if (t < nc) st[4 * t + 3] = (thr[t] - st[4 * t + 1]) / st[4 * t + 2];
  if (t == 0) {
    st[CS_INFO] = rcnt[0] > 0 ? rmin[0] : __builtin_nan("");
    st[CS_INFO + 1] = (double)rcnt[0];
  }
}

int cons_stale(ut_ctx* c, const char* who) {
  UT_CHECK(c, c->cs_nc == 0 || c->cs_fit == c->fit_gen, UT_EINVAL,
           std::string(who) + ": the constraint values were loaded for fit " + std::to_string(c->cs_fit) +
               " and fit " + std::to_string(c->fit_gen) +
               " is current (stale: call ut_gp_cons_set again after every fit, or clear them)");
  return 0;
}

// The per-fit operands of the loaded values: standardised columns (the fit's
// own k_gp_ystats), beta_j = L^-1 chat_j and alpha_j = L^-T beta_j (the fit's
// own mat-vecs over the explicit inverse), tau_j, the feasible-row scan.
// Rebuilt when the fit changed (fit_gen) or the values did (ut_gp_cons_set
// zeroes cs_gen).  On c->stream, after the whole fit: it reads L^-1 and ys.
static int cons_operands(ut_ctx* c) {
  if (c->cs_nc == 0 || c->cs_gen == c->fit_gen) return 0;
  int rc;
  if ((rc = gp_fit_flush(c))) return rc;
  if (c->fit_pending) UT_HIP(c, hipStreamWaitEvent(c->stream, c->ev_fit, 0));
  const int32_t n = c->cs_n, nc = c->cs_nc, npad = gp_npad(n);
  UT_CHECK(c, n == c->gp_n && npad == c->gp_npad_fit, UT_EINVAL, "gp_cons: the values are not the fit's rows");
  const size_t cols = (size_t)nc * npad;
  if ((rc = ensure(c, c->cs_C, cols + UT_CONS_MAX))) return rc;
  if ((rc = ensure(c, c->cs_chat, cols))) return rc;
  if ((rc = ensure(c, c->cs_beta, cols))) return rc;
  if ((rc = ensure(c, c->cs_alpha, cols))) return rc;
  if ((rc = ensure(c, c->cs_stats, (size_t)CS_INFO + 2))) return rc;
  UT_HIP(c, hipMemcpyAsync(c->cs_C.p, c->cs_host, sizeof(double) * (cols + UT_CONS_MAX), hipMemcpyHostToDevice,
                           c->stream));
  UT_HIP(c, hipEventRecord(c->cs_ev, c->stream));
  for (int32_t j = 0; j < nc; ++j) {
    const int64_t o = (int64_t)j * npad;
    if ((rc = launch_gp_ystats(c, c->cs_C.p + o, n, npad, c->cs_chat.p + o, c->cs_stats.p + 4 * j))) return rc;
    if ((rc = launch_gp_lower_mv(c, c->cs_chat.p + o, c->cs_beta.p + o))) return rc;
    if ((rc = launch_gp_upper_mv(c, c->cs_beta.p + o, c->cs_alpha.p + o))) return rc;
  }
  hipLaunchKernelGGL(k_cons_scan, dim3(1), dim3(256), 0, c->stream, c->cs_C.p, c->cs_C.p + cols, n, npad, nc,
                     c->gp_y.p, c->cs_stats.p);
  UT_LAUNCH_CHECK(c);
  c->cs_gen = c->fit_gen;
  return 0;
}

// The constraint-mean partials (c->cs_part [RT][nc][ld]) of the m candidates
// whose K* operands (shape s) are in c->ucand / c->cnorm / c->bcat -- or, given
// ops, in its arrays -- after the per-fit operands.  A column's sums do not
// depend on its neighbours, so pruned scoring reads a gathered candidate's
// means at its own index.
int cons_means(ut_ctx* c, const ScoreShape& s, int64_t m, const CandOps* ops) {
  const CandOps own{c->ucand.p, c->cnorm.p, c->bcat.p, s.ldk};
  const CandOps& u = ops ? *ops : own;
  const int32_t nc = c->cs_nc;
  int rc;
  if ((rc = cons_stale(c, "gp_cons"))) return rc;
  if ((rc = cons_operands(c))) return rc;
  if (nc == 0) return 0;
  if ((rc = ensure(c, c->cs_part, (size_t)s.RT * nc * u.ld))) return rc;
  return launch_kstar_sums(c, "gp_cons", s, u, m, c->cs_alpha.p, nc, KstarRowSet{}, 1.0, c->cs_part.p);
}

// cons_means, then k_cons_apply on the candidates' posterior mu / var with the
// given outputs.
static int cons_tail(ut_ctx* c, const ScoreShape& s, int64_t m, double xi, const double* mu, const double* var,
                     double* p_out, double* mu_c_out, int64_t ldo, double* score) {
  if (int rc = cons_means(c, s, m)) return rc;
  const int32_t nc = c->cs_nc;
  const int64_t ldk = s.ldk;
  hipLaunchKernelGGL(k_cons_apply, dim3(grid1(m, 256)), dim3(256), 0, c->stream, m, s.RT, nc, c->cs_part.p, ldk,
                     c->gp_sf2, c->cs_stats.p, mu, var, xi, p_out, mu_c_out, ldo, score);
  UT_LAUNCH_CHECK(c);
  mark(c, "cons");
  return 0;
}

int cons_weight(ut_ctx* c, const ScoreShape& s, int64_t m, double xi, const double* mu, const double* var,
                double* score) {
  return cons_tail(c, s, m, xi, mu, var, nullptr, nullptr, 0, score);
}

int gp_cons_prob_impl(ut_ctx* c, const double* values, const double* features, int64_t ld, int64_t m, double* p_out,
                      double* mu_c_out) {
  UT_CHECK(c, m >= 0 && ld >= m && (values != nullptr) != (features != nullptr) && (p_out || m == 0), UT_EINVAL,
           "gp_cons_prob: bad arguments (exactly one of values and features, p_out required)");
  UT_CHECK(c, c->gp_ready, UT_EINVAL, "gp_cons_prob: call ut_gp_fit first");
  if (m == 0) return 0;
  int rc;
  if ((rc = cons_stale(c, "gp_cons_prob"))) return rc;
  if (values) {
    UT_CHECK(c, c->has_space, UT_ENOSPACE, "space not defined");
    UT_CHECK(c, c->gp_d == c->space.n_feat, UT_EINVAL, "gp_cons_prob: GP feature width != space feature width");
    if ((rc = gp_encode_scaled(c, values, ld, m))) return rc;
    mark(c, "encode");
  }
  // the objective's posterior, for var(u): no score, so nothing is weighted in there
  const int64_t ldk = gp_ldk(m);
  if ((rc = ensure(c, c->cs_mu, (size_t)ldk))) return rc;
  if ((rc = ensure(c, c->cs_var, (size_t)ldk))) return rc;
  const ut_acq ei{UT_ACQ_EI, 0, 0.0, 0.0};
  if ((rc = gp_score_impl(c, features, ld, m, &ei, nullptr, c->cs_mu.p, c->cs_var.p, nullptr))) return rc;
  return cons_tail(c, score_shape(c, m, !features && c->cat_on && c->ucand_cat), m, 0.0, c->cs_mu.p, c->cs_var.p, p_out,
                   mu_c_out, ld, nullptr);
}

int gp_cons_info_impl(ut_ctx* c, int32_t* n, int32_t* nc, int32_t* n_feasible, double* f_best_c) {
  if (n) *n = c->cs_n;
  if (nc) *nc = c->cs_nc;
  if (n_feasible) *n_feasible = 0;
  if (f_best_c) *f_best_c = std::nan("");
  if (c->cs_nc == 0 || (!n_feasible && !f_best_c)) return 0;   // (the counts alone: no wait)
  int rc;
  if ((rc = gp_wait_fit(c))) return rc;
  if ((rc = cons_stale(c, "gp_cons_info"))) return rc;
  if ((rc = cons_operands(c))) return rc;
  double st[2];
  UT_HIP(c, hipMemcpyAsync(st, c->cs_stats.p + CS_INFO, sizeof(st), hipMemcpyDeviceToHost, c->stream));
  UT_HIP(c, hipStreamSynchronize(c->stream));
  if (n_feasible) *n_feasible = (int32_t)st[1];
  if (f_best_c) *f_best_c = st[0];
  return 0;
}

int gp_cons_set_impl(ut_ctx* c, const double* C, int32_t n, int32_t nc, const double* thr) {
  UT_CHECK(c, nc >= 0 && nc <= UT_CONS_MAX, UT_EINVAL,
           "gp_cons_set: nc = " + std::to_string(nc) + " is not in [0, " + std::to_string(UT_CONS_MAX) + "]");
  if (nc == 0) {
    // nothing is weighted from here on (the device arrays stay: a kernel may still be reading them)
    c->cs_n = 0, c->cs_nc = 0, c->cs_fit = 0, c->cs_gen = 0;
    return 0;
  }
  UT_CHECK(c, c->gp_ready, UT_EINVAL, "gp_cons_set: call ut_gp_fit first (the values belong to a fit)");
  UT_CHECK(c, C != nullptr && thr != nullptr, UT_EINVAL, "gp_cons_set: C_host or threshold_host is NULL");
  UT_CHECK(c, n == c->gp_n, UT_EINVAL,
           "gp_cons_set: n = " + std::to_string(n) + ", the fit has " + std::to_string(c->gp_n) + " rows");
  for (int32_t j = 0; j < nc; ++j)
    UT_CHECK(c, !std::isnan(thr[j]), UT_EINVAL, "gp_cons_set: threshold " + std::to_string(j) + " is NaN");
  for (size_t e = 0; e < (size_t)n * nc; ++e)
    UT_CHECK(c, std::isfinite(C[e]), UT_EINVAL,
             "gp_cons_set: row " + std::to_string(e / nc) + " has a non-finite value");
  // Staged in pinned memory as the device layout, C^T [nc][npad] then the
  // thresholds: cons_operands copies it on the scoring stream, after the fit,
  // so this call neither touches the device nor waits for a staged or in-flight
  // fit.  Only a copy of the previous values still queued is waited for.
  const int32_t npad = gp_npad(n);
  const size_t need = (size_t)UT_CONS_MAX * npad + UT_CONS_MAX;
  if (!c->cs_ev) UT_HIP(c, hipEventCreateWithFlags(&c->cs_ev, hipEventDisableTiming));
  UT_HIP(c, hipEventSynchronize(c->cs_ev));
  if (c->cs_host_n < need) {
    double* q = nullptr;
    const size_t cap = need + need / 4;
    UT_HIP(c, hipHostMalloc((void**)&q, sizeof(double) * cap, hipHostMallocDefault));
    if (c->cs_host) (void)hipHostFree(c->cs_host);
    c->cs_host = q;
    c->cs_host_n = cap;
  }
  std::memset(c->cs_host, 0, sizeof(double) * ((size_t)nc * npad + UT_CONS_MAX));
  for (int32_t r = 0; r < n; ++r)
    for (int32_t j = 0; j < nc; ++j) c->cs_host[(size_t)j * npad + r] = C[(size_t)r * nc + j];
  for (int32_t j = 0; j < nc; ++j) c->cs_host[(size_t)nc * npad + j] = thr[j];
  c->cs_n = n, c->cs_nc = nc, c->cs_fit = c->fit_gen, c->cs_gen = 0;
  return 0;
}

}  // namespace ut
