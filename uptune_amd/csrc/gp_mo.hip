// gp_mo.hip -- two objectives (uthot.h "two objectives"): the second objective
// as a further GP target on the fit's own factor, exactly as a measured
// constraint is (gp_cons.hip):
//   alpha_2 = K^-1 y2s = L^-T (L^-1 y2s),  mu_2(u) = sigma_f2 k*(u) . alpha_2
// by the column-sum K* kernel (gp_kstar_sums.hip), its variance the
// objective's.  The Pareto front of the fit's rows in standardised units is a
// per-fit operand beside alpha_2 (k_mo_mark, k_mo_place: no atomics, so its
// order is fixed), and the score of a candidate is the exact expected
// hypervolume improvement against it (k_mo_ehvi), linear in the front's size.
#include "gp_post.h"
#include "ut_internal.h"

#include <cmath>
#include <cstring>

namespace ut {

// strips of the front staged in LDS at a time (k_mo_ehvi), rows per tile of the front kernels
constexpr int MO_CH = 256;

// psi(t; mu) = E[(t - Y)+], Y ~ N(mu, v): acq_score's EI with t in place of
// f_best.  (t = -inf, the sentinel a_0, is never evaluated: its psi is the 0
// the strip walk starts from.)
__device__ __forceinline__ double mo_psi(double t, double mu, double v, double sigma) {
  const double I = t - mu;
  if (v == 0.0) return I > 0.0 ? I : 0.0;
  const double z = I / sigma;
  const double Phi = 0.5 * erfc(-z * 0.70710678118654752440);
  const double phi = exp(-0.5 * z * z) * 0.39894228040143267794;
  return I * Phi + sigma * phi;
}

// One lane per candidate: mu_2 = sigma_f2 * its partials tile 0 upward, then
// the strips i = 0 .. P in order, w_i = max(psi(a_{i+1}; mu_1) - psi(a_i; mu_1), 0)
// with each psi(a_i) carried to the next strip, EHVI = sum_i w_i psi(b_i; mu_2).
// The workgroup stages MO_CH strips (a_{i+1}, b_i) in LDS at a time; every lane
// reads the same element, so the reads are broadcasts.  A finite score becomes
// EHVI; -inf (a duplicate) and NaN (a failed fit) pass through.
// fr: mo_fr -- [3] = P, a at MO_A, b at boff
__global__ __launch_bounds__(256) void k_mo_ehvi(int64_t m, int32_t RT, const double* __restrict__ part, int64_t ldp,
                                                 double sf2, const double* __restrict__ fr, int64_t boff,
                                                 const double* __restrict__ mu, const double* __restrict__ var,
                                                 double* __restrict__ ehvi_out, double* __restrict__ mu2_out,
                                                 double* __restrict__ score) {
  __shared__ double sa[MO_CH];
  __shared__ double sb[MO_CH];
  const int t = threadIdx.x;
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + t;
  const bool on = i < m;   // (no early return: every lane stages the front)
  const int32_t P = (int32_t)fr[3];
  const double* __restrict__ A = fr + MO_A;
  const double* __restrict__ B = fr + boff;
  double m1 = 0.0, v = 0.0, sigma = 0.0, m2 = 0.0;
  if (on) {
    m1 = mu[i];
    v = var[i];
    sigma = sqrt(v);
    m2 = sf2 * part_sum(part, RT, ldp, i);
  }
  double prev = 0.0, acc = 0.0;
  for (int32_t c0 = 0; c0 <= P; c0 += MO_CH) {
    const int32_t cnt = P + 1 - c0 < MO_CH ? P + 1 - c0 : MO_CH;
    __syncthreads();
    if (t < cnt) {
      sa[t] = A[c0 + t + 1];
      sb[t] = B[c0 + t];
    }
    __syncthreads();
    if (on) {
      for (int32_t k = 0; k < cnt; ++k) {
        const double next = mo_psi(sa[k], m1, v, sigma);
        const double w = next - prev;
        acc += (w > 0.0 ? w : 0.0) * mo_psi(sb[k], m2, v, sigma);
        prev = next;
      }
    }
  }
  if (!on) return;
  if (mu2_out) mu2_out[i] = m2;
  if (ehvi_out) ehvi_out[i] = acc;
  if (score && __builtin_isfinite(score[i])) score[i] = acc;
}

// Step 1 of the front, a grid over rows: row r stays iff it lies inside the
// reference box and no row s has a_s <= a_r, b_s <= b_r and one of a_s < a_r,
// b_s < b_r, s < r (of identical points the smallest row stays).  The rows are
// compared tile by tile out of LDS.  Block 0 also writes the standardised
// reference point.  gst: the fit's gp_stats, st2: the second objective's, ref: raw
__global__ __launch_bounds__(256) void k_mo_mark(const double* __restrict__ ys, const double* __restrict__ y2s,
                                                 int32_t n, const double* __restrict__ gst,
                                                 const double* __restrict__ st2, const double* __restrict__ ref,
                                                 uint8_t* __restrict__ keep, double* __restrict__ fr) {
  __shared__ double sa[MO_CH];
  __shared__ double sb[MO_CH];
  const int t = threadIdx.x;
  const int32_t r = (int32_t)blockIdx.x * MO_CH + t;
  const double r1 = (ref[0] - gst[1]) / gst[2], r2 = (ref[1] - st2[1]) / st2[2];
  const double a = r < n ? ys[r] : 0.0, b = r < n ? y2s[r] : 0.0;
  bool dom = false;
  for (int32_t s0 = 0; s0 < n; s0 += MO_CH) {
    const int32_t cnt = n - s0 < MO_CH ? n - s0 : MO_CH;
    __syncthreads();
    if (t < cnt) {
      sa[t] = ys[s0 + t];
      sb[t] = y2s[s0 + t];
    }
    __syncthreads();
    for (int32_t k = 0; k < cnt; ++k) {
      const double as = sa[k], bs = sb[k];
      dom = dom || (as <= a && bs <= b && (as < a || bs < b || s0 + k < r));
    }
  }
  if (r < n) keep[r] = (a < r1 && b < r2 && !dom) ? 1 : 0;
  if (blockIdx.x == 0 && t == 0) fr[0] = r1, fr[1] = r2;
}

// Step 2, one workgroup: each member goes to the rank given by the count of
// members with smaller (a, r); then the sentinels a_0 = -inf, a_{P+1} = r_1,
// b_0 = r_2, P, and the front's hypervolume sum_i (a_{i+1} - a_i) (r_2 - b_i)
// (per-thread sums over i = t + 1, t + 257, ..., then a tree: a fixed order).
__global__ __launch_bounds__(256) void k_mo_place(const double* __restrict__ ys, const double* __restrict__ y2s,
                                                  int32_t n, const uint8_t* __restrict__ keep, int64_t boff,
                                                  double* __restrict__ fr, int32_t* __restrict__ rows) {
  __shared__ double sa[MO_CH];
  __shared__ uint8_t sk[MO_CH];
  __shared__ int32_t rcnt[256];
  __shared__ double rsum[256];
  const int t = threadIdx.x;
  double* __restrict__ A = fr + MO_A;
  double* __restrict__ B = fr + boff;
  int32_t mine_n = 0;
  for (int32_t rb = 0; rb < n; rb += MO_CH) {
    const int32_t r = rb + t;
    const bool mine = r < n && keep[r] != 0;
    const double a = mine ? ys[r] : 0.0;
    int32_t rank = 0;
    for (int32_t s0 = 0; s0 < n; s0 += MO_CH) {
      const int32_t cnt = n - s0 < MO_CH ? n - s0 : MO_CH;
      __syncthreads();
      if (t < cnt) {
        sa[t] = ys[s0 + t];
        sk[t] = keep[s0 + t];
      }
      __syncthreads();
      if (mine)
        for (int32_t k = 0; k < cnt; ++k) rank += (sk[k] != 0 && (sa[k] < a || (sa[k] == a && s0 + k < r))) ? 1 : 0;
    }
    if (mine) {
      A[rank + 1] = a;
      B[rank + 1] = y2s[r];
      rows[rank] = r;
      ++mine_n;
    }
  }
  rcnt[t] = mine_n;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) rcnt[t] += rcnt[t + w];
    __syncthreads();
  }
  const int32_t P = rcnt[0];
  const double r1 = fr[0], r2 = fr[1];
  if (t == 0) {
    A[0] = -1.0 / 0.0;
    A[P + 1] = r1;
    B[0] = r2;
    fr[3] = (double)P;
  }
  __threadfence_block();
  __syncthreads();   // (the members and sentinels written above are read below)
  double hv = 0.0;
  for (int32_t i = t + 1; i <= P; i += 256) hv += (A[i + 1] - A[i]) * (r2 - B[i]);
  rsum[t] = hv;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) rsum[t] += rsum[t + w];
    __syncthreads();
  }
  if (t == 0) fr[2] = rsum[0];
}

int mo_refuse(ut_ctx* c, const char* who, const char* why) {
  UT_CHECK(c, c->mo_n == 0, UT_EUNSUPPORTED,
           std::string(who) + ": a second objective is loaded (ut_gp_mo_set) and " + why);
  return 0;
}

static int mo_stale(ut_ctx* c, const char* who) {
  UT_CHECK(c, c->mo_n == 0 || c->mo_fit == c->fit_gen, UT_EINVAL,
           std::string(who) + ": the second objective's values were loaded for fit " + std::to_string(c->mo_fit) +
               " and fit " + std::to_string(c->fit_gen) +
               " is current (stale: call ut_gp_mo_set again after every fit, or clear them)");
  return 0;
}

int mo_check(ut_ctx* c, const char* who, const ut_acq* acq) {
  if (c->mo_n == 0) return 0;
  if (int rc = mo_stale(c, who)) return rc;
  UT_CHECK(c, !(acq && acq->kind == UT_ACQ_UCB), UT_EUNSUPPORTED,
           std::string(who) + ": a second objective is loaded (ut_gp_mo_set) and the expected hypervolume "
                              "improvement stands in for EI only: there is no two-objective UCB");
  return 0;
}

// The per-fit operands of the loaded values: y2s and its stats (the fit's own
// k_gp_ystats), beta_2 = L^-1 y2s and alpha_2 = L^-T beta_2 (the fit's own
// mat-vecs), the front.  Rebuilt when the fit changed (fit_gen) or the values
// did (ut_gp_mo_set zeroes mo_gen).  On c->stream, after the whole fit.
static int mo_operands(ut_ctx* c) {
  if (c->mo_n == 0 || c->mo_gen == c->fit_gen) return 0;
  int rc;
  if ((rc = gp_fit_flush(c))) return rc;
  if (c->fit_pending) UT_HIP(c, hipStreamWaitEvent(c->stream, c->ev_fit, 0));
  const int32_t n = c->mo_n, npad = gp_npad(n);
  UT_CHECK(c, n == c->gp_n && npad == c->gp_npad_fit, UT_EINVAL, "gp_mo: the values are not the fit's rows");
  if ((rc = ensure(c, c->mo_Y, (size_t)npad + 2))) return rc;
  if ((rc = ensure(c, c->mo_y2s, (size_t)npad))) return rc;
  if ((rc = ensure(c, c->mo_beta, (size_t)npad))) return rc;
  if ((rc = ensure(c, c->mo_alpha, (size_t)npad))) return rc;
  if ((rc = ensure(c, c->mo_stats, 4))) return rc;
  if ((rc = ensure(c, c->mo_keep, (size_t)npad))) return rc;
  if ((rc = ensure(c, c->mo_fr, (size_t)MO_A + 2 * ((size_t)npad + 2)))) return rc;
  if ((rc = ensure(c, c->mo_rows, (size_t)npad))) return rc;
  UT_HIP(c, hipMemcpyAsync(c->mo_Y.p, c->mo_host, sizeof(double) * ((size_t)npad + 2), hipMemcpyHostToDevice,
                           c->stream));
  UT_HIP(c, hipEventRecord(c->mo_ev, c->stream));
  if ((rc = launch_gp_ystats(c, c->mo_Y.p, n, npad, c->mo_y2s.p, c->mo_stats.p))) return rc;
  if ((rc = launch_gp_lower_mv(c, c->mo_y2s.p, c->mo_beta.p))) return rc;
  if ((rc = launch_gp_upper_mv(c, c->mo_beta.p, c->mo_alpha.p))) return rc;
  mark(c, "mo_ops");
  hipLaunchKernelGGL(k_mo_mark, dim3(grid1(n, MO_CH)), dim3(MO_CH), 0, c->stream, c->gp_y.p, c->mo_y2s.p, n,
                     c->gp_stats.p, c->mo_stats.p, c->mo_Y.p + npad, c->mo_keep.p, c->mo_fr.p);
  UT_LAUNCH_CHECK(c);
  hipLaunchKernelGGL(k_mo_place, dim3(1), dim3(256), 0, c->stream, c->gp_y.p, c->mo_y2s.p, n, c->mo_keep.p,
                     mo_b_off(npad), c->mo_fr.p, c->mo_rows.p);
  UT_LAUNCH_CHECK(c);
  mark(c, "mo_front");   // (k_mo_mark + k_mo_place)
  c->mo_gen = c->fit_gen;
  return 0;
}

// the per-fit operands, the second objective's mean partials (k_kstar_sums with
// alpha_2 as the rows' weights) and k_mo_ehvi on the candidates' posterior
static int mo_tail(ut_ctx* c, const ScoreShape& s, int64_t m, const double* mu, const double* var, double* ehvi_out,
                   double* mu2_out, double* score) {
  int rc;
  if ((rc = mo_stale(c, "gp_mo"))) return rc;
  if ((rc = mo_operands(c))) return rc;
  if ((rc = ensure(c, c->mo_part, (size_t)s.RT * s.ldk))) return rc;
  const CandOps u{c->ucand.p, c->cnorm.p, c->bcat.p, s.ldk};
  if ((rc = launch_kstar_sums(c, "gp_mo", s, u, m, c->mo_alpha.p, 1, KstarRowSet{}, 1.0, c->mo_part.p))) return rc;
  mark(c, "mo_means");
  hipLaunchKernelGGL(k_mo_ehvi, dim3(grid1(m, 256)), dim3(256), 0, c->stream, m, s.RT, c->mo_part.p, s.ldk, c->gp_sf2,
                     c->mo_fr.p, mo_b_off(s.npad), mu, var, ehvi_out, mu2_out, score);
  UT_LAUNCH_CHECK(c);
  mark(c, "mo_ehvi");
  return 0;
}

int mo_weight(ut_ctx* c, const ScoreShape& s, int64_t m, const double* mu, const double* var, double* score) {
  return mo_tail(c, s, m, mu, var, nullptr, nullptr, score);
}

int gp_mo_score_impl(ut_ctx* c, const double* values, const double* features, int64_t ld, int64_t m, double* ehvi_out,
                     double* mu2_out) {
  UT_CHECK(c, m >= 0 && ld >= m && (values != nullptr) != (features != nullptr) && (ehvi_out || m == 0), UT_EINVAL,
           "gp_mo_score: bad arguments (exactly one of values and features, ehvi_out required)");
  UT_CHECK(c, c->gp_ready, UT_EINVAL, "gp_mo_score: call ut_gp_fit first");
  UT_CHECK(c, c->mo_n > 0, UT_EINVAL, "gp_mo_score: no second objective is loaded (ut_gp_mo_set)");
  if (m == 0) return 0;
  int rc;
  if ((rc = mo_stale(c, "gp_mo_score"))) return rc;
  if (values) {
    UT_CHECK(c, c->has_space, UT_ENOSPACE, "space not defined");
    UT_CHECK(c, c->gp_d == c->space.n_feat, UT_EINVAL, "gp_mo_score: GP feature width != space feature width");
    if ((rc = gp_encode_scaled(c, values, ld, m))) return rc;
    mark(c, "encode");
  }
  // the objective's posterior: no score, so no tail runs in there
  const int64_t ldk = gp_ldk(m);
  if ((rc = ensure(c, c->cs_mu, (size_t)ldk))) return rc;
  if ((rc = ensure(c, c->cs_var, (size_t)ldk))) return rc;
  const ut_acq ei{UT_ACQ_EI, 0, 0.0, 0.0};
  if ((rc = gp_score_impl(c, features, ld, m, &ei, nullptr, c->cs_mu.p, c->cs_var.p, nullptr))) return rc;
  return mo_tail(c, score_shape(c, m, !features && c->cat_on && c->ucand_cat), m, c->cs_mu.p, c->cs_var.p, ehvi_out,
                 mu2_out, nullptr);
}

// the fit waited for, the operands built and the stream drained: mo_fr's header on the host
static int mo_header(ut_ctx* c, const char* who, double (&h)[MO_A]) {
  int rc;
  if ((rc = gp_wait_fit(c))) return rc;
  if ((rc = mo_stale(c, who))) return rc;
  if ((rc = mo_operands(c))) return rc;
  UT_HIP(c, hipMemcpyAsync(h, c->mo_fr.p, sizeof(h), hipMemcpyDeviceToHost, c->stream));
  UT_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

int gp_mo_info_impl(ut_ctx* c, int32_t* n, int32_t* P, double* ref_std, double* hv) {
  if (n) *n = c->mo_n;
  if (P) *P = 0;
  if (ref_std) ref_std[0] = ref_std[1] = std::nan("");
  if (hv) *hv = std::nan("");
  if (c->mo_n == 0 || (!P && !ref_std && !hv)) return 0;   // (the count alone: no wait)
  double h[MO_A];
  if (int rc = mo_header(c, "gp_mo_info", h)) return rc;
  if (P) *P = (int32_t)h[3];
  if (ref_std) ref_std[0] = h[0], ref_std[1] = h[1];
  if (hv) *hv = h[2];
  return 0;
}

int gp_mo_front_impl(ut_ctx* c, int32_t* rows_host, double* a_host, double* b_host, int32_t cap, int32_t* P) {
  UT_CHECK(c, cap >= 0 && P != nullptr, UT_EINVAL, "gp_mo_front: cap < 0 or P is NULL");
  UT_CHECK(c, c->mo_n > 0, UT_EINVAL, "gp_mo_front: no second objective is loaded (ut_gp_mo_set)");
  double h[MO_A];
  if (int rc = mo_header(c, "gp_mo_front", h)) return rc;
  *P = (int32_t)h[3];
  const size_t k = (size_t)std::min(*P, cap);
  if (k == 0) return 0;
  const int32_t npad = gp_npad(c->mo_n);
  if (rows_host) UT_HIP(c, hipMemcpy(rows_host, c->mo_rows.p, sizeof(int32_t) * k, hipMemcpyDeviceToHost));
  if (a_host) UT_HIP(c, hipMemcpy(a_host, c->mo_fr.p + MO_A + 1, sizeof(double) * k, hipMemcpyDeviceToHost));
  if (b_host) UT_HIP(c, hipMemcpy(b_host, c->mo_fr.p + mo_b_off(npad) + 1, sizeof(double) * k, hipMemcpyDeviceToHost));
  return 0;
}

int gp_mo_read_impl(ut_ctx* c, int32_t what, double* out_host) {
  UT_CHECK(c, what >= 0 && what <= 2 && out_host != nullptr, UT_EINVAL, "gp_mo_read: unknown operand or NULL output");
  UT_CHECK(c, c->mo_n > 0, UT_EINVAL, "gp_mo_read: no second objective is loaded (ut_gp_mo_set)");
  double h[MO_A];
  if (int rc = mo_header(c, "gp_mo_read", h)) return rc;
  const double* src = what == 0 ? c->mo_y2s.p : what == 1 ? c->mo_alpha.p : c->mo_stats.p + 1;
  const size_t cnt = what == 2 ? 2 : (size_t)c->mo_n;
  UT_HIP(c, hipMemcpy(out_host, src, sizeof(double) * cnt, hipMemcpyDeviceToHost));
  return 0;
}

int gp_mo_set_impl(ut_ctx* c, const double* Y2, int32_t n, const double* ref) {
  if (n == 0) {
    // every score is the plain acquisition from here on (the device arrays stay: a kernel may still be reading them)
    c->mo_n = 0, c->mo_fit = 0, c->mo_gen = 0;
    return 0;
  }
  UT_CHECK(c, c->gp_ready, UT_EINVAL, "gp_mo_set: call ut_gp_fit first (the values belong to a fit)");
  UT_CHECK(c, Y2 != nullptr && ref != nullptr, UT_EINVAL, "gp_mo_set: Y2_host or ref_host is NULL");
  UT_CHECK(c, n == c->gp_n, UT_EINVAL,
           "gp_mo_set: n = " + std::to_string(n) + ", the fit has " + std::to_string(c->gp_n) + " rows");
  for (int32_t r = 0; r < n; ++r)
    UT_CHECK(c, std::isfinite(Y2[r]), UT_EINVAL, "gp_mo_set: row " + std::to_string(r) + " has a non-finite value");
  UT_CHECK(c, std::isfinite(ref[0]) && std::isfinite(ref[1]), UT_EINVAL,
           "gp_mo_set: a reference coordinate is not finite");
  UT_CHECK(c, c->cs_nc == 0, UT_EUNSUPPORTED,
           "gp_mo_set: constraint values are loaded (ut_gp_cons_set): constrained EHVI is not built");
  UT_CHECK(c, c->fs_n == 0, UT_EUNSUPPORTED,
           "gp_mo_set: failed rows are loaded (ut_gp_feas_set): EHVI under the feasibility vote is not built");
  // staged in pinned memory as the device layout (ut_gp_cons_set's way): mo_operands copies it on the scoring
  // stream, after the fit, so this call neither touches the device nor waits for a staged or in-flight fit
  const int32_t npad = gp_npad(n);
  const size_t need = (size_t)npad + 2;
  if (!c->mo_ev) UT_HIP(c, hipEventCreateWithFlags(&c->mo_ev, hipEventDisableTiming));
  UT_HIP(c, hipEventSynchronize(c->mo_ev));
  if (c->mo_host_n < need) {
    double* q = nullptr;
    const size_t cap = need + need / 4;
    UT_HIP(c, hipHostMalloc((void**)&q, sizeof(double) * cap, hipHostMallocDefault));
    if (c->mo_host) (void)hipHostFree(c->mo_host);
    c->mo_host = q;
    c->mo_host_n = cap;
  }
  std::memset(c->mo_host, 0, sizeof(double) * need);
  std::memcpy(c->mo_host, Y2, sizeof(double) * (size_t)n);
  c->mo_host[npad] = ref[0], c->mo_host[npad + 1] = ref[1];
  c->mo_n = n, c->mo_fit = c->fit_gen, c->mo_gen = 0;
  return 0;
}

}  // namespace ut
