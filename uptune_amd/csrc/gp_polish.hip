// gp_polish.hip -- the acquisition's gradient in the unit features
// (ut_gp_acq_grad) and the projected-ascent polish of a shortlist
// (ut_gp_polish); include/uthot.h states both rules in full.  With U the p
// candidates' features, us = u / ell, and what the fit left on the device:
//
//   K* [n][p],  V = L^-1 K*,  W = L^-T V,
//   mu = V^T beta,  var = max(sf2 - colsum(V o V), 0)
//   dmu/du_j  = -(1/ell_j) (us_j sum_i alpha_i k_i - sum_i alpha_i k_i xs_ij)
//   dvar/du_j = +(2/ell_j) (us_j sum_i w_i k_i     - sum_i w_i k_i xs_ij)
//   ds/du_j   = cm dmu/du_j + cs dvar/du_j
//     EI:  cm = -Phi(z), cs = phi(z) / (2 sigma);  sigma not > 0: cm = -[I > 0], cs = 0
//     UCB: cm = -1, cs = kappa / (2 sigma);        sigma not > 0: cs = 0
//
//   K*, V       gp_batch.hip's: launch_encode_scaled, launch_gemm_kstar(c, 64, ..), k_bs_v
//   k_pl_tail   mu and |v|^2 per candidate, the rows in 16 groups summed in
//               order and the groups added in order; the score through
//               Acq::score, cm, cs
//   k_pl_w      W tile = (L^-1)^T [64 rows][k] V [k][64 columns]: gp_Linv read
//               with the k index as the row (a two-matrix tile64_tn: both staged
//               lines are 64 contiguous doubles, no transpose of the factor is
//               needed); (L^-1)^T is upper triangular, so row tile rt STARTS its
//               k loop at its diagonal tile and ends at ceil16(n) (V is zero below)
//   k_pl_grad   one workgroup per 64 features x 64 candidates: the scaled
//               training rows staged once per k step for both products (from
//               gp_Xs, the rows as the fit scaled them: gp_XsT holds them
//               times 256 / ln 2 for the K* contraction, one rounding more),
//               the B operands K* o alpha and K* o W formed while staging,
//               their column sums taken from the staged lines in k order; the
//               epilogue applies the us_j terms, 1/ell_j and cm, cs and writes
//               ds/du
//   k_pl_*      the polish's elementwise steps, one candidate per thread, the
//               features in ascending order
// alpha = L^-T beta is the fit's (gp_ensure_linvt writes it where a
// precision-8 refit left it out).  Always fp64 and over every feature.  Every
// sum runs in a fixed order and nothing is accumulated by atomics, so two calls
// on one fit return the same bits.  Scratch: the context's bs_* arrays.
#include "gp_post.h"
#include "gp_tiles.h"
#include "ut_param.h"

namespace ut {

constexpr int32_t PL_MAX_P = 4096;

struct PolishShape {
  int32_t n, npad, d, dpad, p, CT, kend;
  int64_t ldp;
};

// per-candidate vectors in bs_pvec, [ldp] each
enum : int { PV_MU = 0, PV_VAR, PV_SCORE, PV_CM, PV_CS, PV_S, PV_S0, PV_ETA, PV_COUNT };

// 16 candidates per workgroup, the rows in 16 contiguous groups (thread t:
// candidate t & 15, group t >> 4); the groups' partial sums are added in group
// order by the candidate's first thread
constexpr int TAIL_C = 16, TAIL_G = 16;
__global__ __launch_bounds__(256) void k_pl_tail(const double* __restrict__ V, int64_t ldp,
                                                 const double* __restrict__ beta, int32_t n, int32_t p, Acq a,
                                                 double* __restrict__ mu, double* __restrict__ var,
                                                 double* __restrict__ score, double* __restrict__ cm,
                                                 double* __restrict__ cs) {
  __shared__ double pm[TAIL_G][TAIL_C], pq[TAIL_G][TAIL_C];
  const int cl = threadIdx.x & (TAIL_C - 1), grp = threadIdx.x / TAIL_C;
  const int32_t i = blockIdx.x * TAIL_C + cl;
  const int32_t chunk = (n + TAIL_G - 1) / TAIL_G;
  const int32_t r0 = grp * chunk, r1 = r0 + chunk < n ? r0 + chunk : n;
  double m = 0.0, vs = 0.0;
  if (i < p)
    for (int32_t r = r0; r < r1; ++r) {
      const double v = V[(int64_t)r * ldp + i];
      m = __builtin_fma(v, beta[r], m);
      vs = __builtin_fma(v, v, vs);
    }
  pm[grp][cl] = m;
  pq[grp][cl] = vs;
  __syncthreads();
  if (grp != 0 || i >= p) return;
  for (int g = 1; g < TAIL_G; ++g) m += pm[g][cl], vs += pq[g][cl];
  const double vr = clamped_var(a.sf2, vs);
  const double sigma = sqrt(vr);
  double sc = a.score(m, vr);
  if (*a.fit_flag != 0) sc = __builtin_nan("");   // failed fit: nothing is selectable
  double c_mu, c_var = 0.0;
  if (a.kind == UT_ACQ_UCB) {
    c_mu = -1.0;
    if (sigma > 0.0) c_var = a.kappa / (2.0 * sigma);
  } else {
    const double I = a.stats[0] - m - a.xi;
    if (!(sigma > 0.0)) {
      c_mu = I > 0.0 ? -1.0 : 0.0;
    } else {
      const double z = I / sigma;
      c_mu = -0.5 * erfc(-z * 0.70710678118654752440);
      c_var = exp(-0.5 * z * z) * 0.39894228040143267794 / (2.0 * sigma);
    }
  }
  mu[i] = m;
  var[i] = vr;
  score[i] = sc;
  cm[i] = c_mu;
  cs[i] = c_var;
}

// W[row0 .. + 64)[col0 .. + 64) of L^-T V.  Linv [npad][npad] row-major, V / W
// [npad][ldp]; grid (column tiles, npad / 64); kend = ceil16(n)
__global__ __launch_bounds__(256) void k_pl_w(const double* __restrict__ Linv, int32_t npad,
                                              const double* __restrict__ V, int64_t ldp, int32_t kend,
                                              double* __restrict__ W) {
  __shared__ double As[16 * 80];
  __shared__ double Bs[16 * 80];
  const int t = threadIdx.x;
  const int64_t col0 = (int64_t)blockIdx.x * 64, row0 = (int64_t)blockIdx.y * 64;
  fd4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = (fd4){0.0, 0.0, 0.0, 0.0};
  for (int32_t k0 = (int32_t)row0; k0 < kend; k0 += 16) {   // (row0 >= kend: the tile is zero)
    for (int e = t; e < 64 * 16; e += 256) {
      const int kk = e >> 6, r = e & 63;
      As[kk * 80 + r] = Linv[(int64_t)(k0 + kk) * npad + row0 + r];
      Bs[kk * 80 + r] = V[(int64_t)(k0 + kk) * ldp + col0 + r];
    }
    __syncthreads();
    tile64_step(As, Bs, acc);
    __syncthreads();
  }
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) W[(row0 + tile_row(a, r)) * ldp + col0 + tile_col(b)] = acc[a][b][r];
}

// ds/du of features [f0, f0 + 64) x candidates [col0, col0 + 64).  Xs [npad][d]
// (a staged line is one training row's features), kst / W / U [.][ldp]; grid
// (column tiles, ceil(d / 64))
__global__ __launch_bounds__(256) void k_pl_grad(const double* __restrict__ Xs, const double* __restrict__ kst,
                                                 const double* __restrict__ W,
                                                 const double* __restrict__ alpha, const double* __restrict__ U,
                                                 const double* __restrict__ inv_ell,
                                                 const double* __restrict__ cm, const double* __restrict__ cs,
                                                 int64_t ldp, int32_t n, int32_t kend, int32_t d, int32_t p,
                                                 double* __restrict__ out, int64_t ldg) {
  __shared__ double As[16 * 80];
  __shared__ double Bm[16 * 80];
  __shared__ double Bw[16 * 80];
  __shared__ double colsum[2 * 64];
  const int t = threadIdx.x;
  const int64_t col0 = (int64_t)blockIdx.x * 64;
  const int32_t f0 = blockIdx.y * 64;
  fd4 am[2][2], aw[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) am[a][b] = aw[a][b] = (fd4){0.0, 0.0, 0.0, 0.0};
  double cs_run = 0.0;   // threads 0 .. 63: sum alpha k of column t; 64 .. 127: sum w k of column t - 64
  for (int32_t k0 = 0; k0 < kend; k0 += 16) {
    for (int e = t; e < 64 * 16; e += 256) {
      const int k2 = e >> 6, cc = e & 63;
      const bool in = k0 + k2 < n;
      As[k2 * 80 + cc] = in && f0 + cc < d ? Xs[(int64_t)(k0 + k2) * d + f0 + cc] : 0.0;
      const int64_t at = (int64_t)(k0 + k2) * ldp + col0 + cc;
      const double kv = kst[at];
      Bm[k2 * 80 + cc] = in ? kv * alpha[k0 + k2] : 0.0;
      Bw[k2 * 80 + cc] = in ? kv * W[at] : 0.0;
    }
    __syncthreads();
    if (t < 128) {
      const double* B = t < 64 ? Bm : Bw;
#pragma unroll
      for (int kk = 0; kk < 16; ++kk) cs_run += B[kk * 80 + (t & 63)];
    }
    tile64_step(As, Bm, am);
    tile64_step(As, Bw, aw);
    __syncthreads();
  }
  if (t < 128) colsum[t] = cs_run;
  __syncthreads();
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    const int cl = tile_col(b);
    const int64_t i = col0 + cl;
    if (i >= p) continue;
    const double sa = colsum[cl], sw = colsum[64 + cl];
    const double c_mu = cm[i], c_var = cs[i];
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int32_t j = f0 + tile_row(a, r);
        if (j >= d) continue;
        const double usj = U[(int64_t)j * ldp + i], ie = inv_ell[j];
        const double dmu = -ie * (usj * sa - am[a][b][r]);
        const double dvar = 2.0 * ie * (usj * sw - aw[a][b][r]);
        // (a zero coefficient drops its term whatever the term is)
        double g = c_mu != 0.0 ? c_mu * dmu : 0.0;
        if (c_var != 0.0) g += c_var * dvar;
        out[(int64_t)j * ldg + i] = g;
      }
  }
}

// free[j] = 1 on the unit-value column of a FLOAT / INT / LOGINT / POW2 parameter with u_lo < u_hi
__global__ __launch_bounds__(256) void k_pl_free(const DevParam* __restrict__ params, int32_t P, int32_t d,
                                                 uint8_t* __restrict__ free_) {
  const int32_t q = blockIdx.x * 256 + threadIdx.x;
  if (q >= P) return;
  const DevParam pr = params[q];
  if (is_primitive(pr.kind) && pr.u_lo < pr.u_hi && pr.feat_col >= 0 && pr.feat_col < d) free_[pr.feat_col] = 1;
}

__global__ __launch_bounds__(256) void k_pl_init(int32_t p, const double* __restrict__ score, double step0,
                                                 double* __restrict__ s, double* __restrict__ s0,
                                                 double* __restrict__ eta, uint8_t* __restrict__ accepted) {
  const int32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= p) return;
  s[i] = s0[i] = score[i];
  eta[i] = step0;
  accepted[i] = 0;
}

// mask and project the gradient, N, and the trial's K* operands.  One
// candidate per thread over all ldp columns (the padding columns get zeros).
__global__ __launch_bounds__(256) void k_pl_trial(int32_t d, int32_t dpad, int32_t p, int64_t ldp,
                                                  const uint8_t* __restrict__ free_,
                                                  const double* __restrict__ inv_ell,
                                                  const double* __restrict__ ucur, double* __restrict__ utrial,
                                                  double* __restrict__ G, const double* __restrict__ eta,
                                                  const uint8_t* __restrict__ dup, uint8_t* __restrict__ act,
                                                  double* __restrict__ us, double* __restrict__ cn) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= ldp) return;
  if (i >= p) {
    for (int32_t j = 0; j < dpad; ++j) us[(int64_t)j * ldp + i] = 0.0;
    cn[i] = 0.0;
    return;
  }
  double n2 = 0.0;
  for (int32_t j = 0; j < d; ++j) {
    const int64_t at = (int64_t)j * ldp + i;
    double g = G[at];
    const double u = ucur[at];
    if (!free_[j] || (u <= 0.0 && g < 0.0) || (u >= 1.0 && g > 0.0)) g = 0.0;
    G[at] = g;
    const double lg = g / inv_ell[j];
    n2 += lg * lg;
  }
  const double N = sqrt(n2);
  const bool on = !(dup && dup[i]) && N > 0.0 && N < 1.0 / 0.0;
  act[i] = on ? 1 : 0;
  const double e = eta[i];
  double s = 0.0;
  for (int32_t j = 0; j < d; ++j) {
    const int64_t at = (int64_t)j * ldp + i;
    double u = ucur[at];
    if (on && free_[j]) {
      const double l = 1.0 / inv_ell[j];
      u = u + e * l * l * G[at] / N;
      u = u < 0.0 ? 0.0 : (u > 1.0 ? 1.0 : u);
    }
    utrial[at] = u;
    const double v = u * inv_ell[j];
    us[at] = v;
    s += v * v;
  }
  for (int32_t j = d; j < dpad; ++j) us[(int64_t)j * ldp + i] = 0.0;
  cn[i] = s;
}

// accept or reject the trial, then the current point's K* operands (the next step's gradient is taken there)
__global__ __launch_bounds__(256) void k_pl_accept(int32_t d, int32_t dpad, int32_t p, int64_t ldp,
                                                   const uint8_t* __restrict__ act,
                                                   const double* __restrict__ strial, double grow, double shrink,
                                                   double step_max, const double* __restrict__ inv_ell,
                                                   double* __restrict__ ucur, const double* __restrict__ utrial,
                                                   double* __restrict__ s, double* __restrict__ eta,
                                                   uint8_t* __restrict__ accepted, double* __restrict__ us,
                                                   double* __restrict__ cn) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= p) return;   // (the padding columns hold k_pl_trial's zeros)
  bool take = false;
  if (act[i]) {
    const double sp = strial[i];
    take = sp > s[i];
    if (take) {
      s[i] = sp;
      const double e = grow * eta[i];
      eta[i] = e < step_max ? e : step_max;
      accepted[i] = 1;
    } else {
      eta[i] = shrink * eta[i];
    }
  }
  double q = 0.0;
  for (int32_t j = 0; j < d; ++j) {
    const int64_t at = (int64_t)j * ldp + i;
    const double u = take ? utrial[at] : ucur[at];
    if (take) ucur[at] = u;
    const double v = u * inv_ell[j];
    us[at] = v;
    q += v * v;
  }
  cn[i] = q;
}

// v' = set_unit_value(u) on the free parameters of a candidate that accepted a step; every other value as it came
__global__ __launch_bounds__(256) void k_pl_decode(const DevParam* __restrict__ params, int32_t P,
                                                   const double* __restrict__ values, int64_t ld, int32_t p,
                                                   const double* __restrict__ ucur, int64_t ldp,
                                                   const uint8_t* __restrict__ accepted,
                                                   double* __restrict__ vout) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= p) return;
  const bool acc = accepted[i] != 0;
  for (int32_t q = 0; q < P; ++q) {
    const DevParam& pr = params[q];
    const int32_t w = pr.psize > 1 ? pr.psize : 1;
    for (int32_t s = 0; s < w; ++s) {
      double v = values[(int64_t)(pr.col + s) * ld + i];
      if (acc && s == 0 && is_primitive(pr.kind)) v = from_unit(pr, ucur[(int64_t)pr.feat_col * ldp + i], v);
      vout[(int64_t)(pr.col + s) * ldp + i] = v;
    }
  }
}

__global__ __launch_bounds__(256) void k_pl_final(int32_t ncols, int32_t p, const double* __restrict__ values,
                                                  int64_t ld, const double* __restrict__ vnew, int64_t ldp,
                                                  const double* __restrict__ sv, const double* __restrict__ s0,
                                                  const uint8_t* __restrict__ dup,
                                                  const uint8_t* __restrict__ accepted,
                                                  double* __restrict__ out_values, int64_t ldo,
                                                  double* __restrict__ out_score, double* __restrict__ out_score0,
                                                  uint8_t* __restrict__ out_moved) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= p) return;
  const bool isdup = dup && dup[i];
  const bool mv = !isdup && accepted[i] && sv[i] > s0[i];
  for (int32_t cidx = 0; cidx < ncols; ++cidx)
    out_values[(int64_t)cidx * ldo + i] = mv ? vnew[(int64_t)cidx * ldp + i] : values[(int64_t)cidx * ld + i];
  out_score[i] = isdup ? -1.0 / 0.0 : (mv ? sv[i] : s0[i]);
  if (out_score0) out_score0[i] = isdup ? -1.0 / 0.0 : s0[i];
  if (out_moved) out_moved[i] = mv ? 1 : 0;
}

// the checks both calls share, the fit on the device, the shape and the scratch of one evaluation
static int pl_prepare(ut_ctx* c, const char* who, const double* values, int64_t ld, int32_t p, const ut_acq* acq,
                      PolishShape& s) {
  const std::string w(who);
  UT_CHECK(c, values && acq, UT_EINVAL, w + ": NULL values or acq");
  UT_CHECK(c, p >= 1 && p <= PL_MAX_P && ld >= p, UT_EINVAL, w + ": needs 1 <= p <= 4096 and ld >= p");
  UT_CHECK(c, c->cs_nc == 0, UT_EINVAL,
           w + ": constraint values are loaded (ut_gp_cons_set) and the gradient of the weighted score is not built");
  UT_CHECK(c, c->fs_n == 0, UT_EINVAL,
           w + ": failed rows are loaded (ut_gp_feas_set) and the gradient of the weighted score is not built");
  UT_CHECK(c, c->gp_ready, UT_EINVAL, "gp_score: call ut_gp_fit first");
  int rc;
  if ((rc = gp_fit_flush(c))) return rc;
  UT_CHECK(c, c->has_space && c->space.n_feat == c->gp_d, UT_EINVAL,
           w + ": the fit's feature count is not the space's");
  // the whole fit (L^-1, beta), on the device
  if (c->fit_pending) UT_HIP(c, hipStreamWaitEvent(c->stream, c->ev_fit, 0));
  s.n = c->gp_n, s.npad = c->gp_npad_fit;
  UT_CHECK(c, s.npad == gp_npad(s.n) && s.npad % 64 == 0, UT_EINVAL, w + ": no fitted GP");
  s.d = c->gp_d, s.dpad = kstar_dpad(c->gp_d);
  s.p = p, s.ldp = gp_ldk(p), s.CT = (p + 63) / 64;
  s.kend = (s.n + 15) / 16 * 16;   // (<= npad) V is zero in the padding rows
  if ((rc = ensure(c, c->bs_u, (size_t)s.dpad * s.ldp))) return rc;
  if ((rc = ensure(c, c->bs_cn, (size_t)s.ldp))) return rc;
  if ((rc = ensure(c, c->bs_kst, (size_t)s.npad * s.ldp))) return rc;
  if ((rc = ensure(c, c->bs_v, (size_t)s.npad * s.ldp))) return rc;
  if ((rc = ensure(c, c->bs_w, (size_t)s.npad * s.ldp))) return rc;
  if ((rc = ensure(c, c->bs_pvec, (size_t)PV_COUNT * s.ldp))) return rc;
  return gp_ensure_linvt(c);   // alpha (a precision-8 refit leaves it out)
}

// mu, var, score, cm, cs of the candidates whose operands are in bs_u / bs_cn;
// grad: ds/du as well, [d][ldg]
static int pl_eval(ut_ctx* c, const PolishShape& s, const Acq& a, double* grad, int64_t ldg) {
  int rc;
  KstarArgs ka;
  ka.train = KstarTrain{c->gp_XsT.p};
  ka.ucand = c->bs_u.p, ka.dpad = s.dpad, ka.cn = c->bs_cn.p;
  ka.m = s.p, ka.kst = c->bs_kst.p, ka.ldk = s.ldp;
  if ((rc = launch_gemm_kstar(c, 64, s.npad, ka))) return rc;
  mark(c, "pl_kstar");
  if ((rc = launch_bs_v(c, s.CT, s.npad, c->bs_kst.p, s.ldp, c->bs_v.p))) return rc;
  mark(c, "pl_v");
  double* pv = c->bs_pvec.p;
  hipLaunchKernelGGL(k_pl_tail, dim3((s.p + TAIL_C - 1) / TAIL_C), dim3(256), 0, c->stream, c->bs_v.p, s.ldp, c->gp_beta.p, s.n,
                     s.p, a, pv + PV_MU * s.ldp, pv + PV_VAR * s.ldp, pv + PV_SCORE * s.ldp, pv + PV_CM * s.ldp,
                     pv + PV_CS * s.ldp);
  UT_LAUNCH_CHECK(c);
  mark(c, "pl_tail");
  if (!grad) return 0;
  hipLaunchKernelGGL(k_pl_w, dim3(s.CT, s.npad / 64), dim3(256), 0, c->stream, c->gp_Linv.p, s.npad, c->bs_v.p, s.ldp,
                     s.kend, c->bs_w.p);
  UT_LAUNCH_CHECK(c);
  mark(c, "pl_w");
  hipLaunchKernelGGL(k_pl_grad, dim3(s.CT, (s.d + 63) / 64), dim3(256), 0, c->stream, c->gp_Xs.p, c->bs_kst.p, c->bs_w.p, c->gp_alpha.p, c->bs_u.p, c->gp_inv_ell.p, pv + PV_CM * s.ldp,
                     pv + PV_CS * s.ldp, s.ldp, s.n, s.kend, s.d, s.p, grad, ldg);
  UT_LAUNCH_CHECK(c);
  mark(c, "pl_grad");
  return 0;
}

int gp_acq_grad_impl(ut_ctx* c, const double* values, int64_t ld, int32_t p, const ut_acq* acq, double* out_score,
                     double* out_mu, double* out_var, double* out_grad, int64_t ld_g) {
  UT_CHECK(c, out_mu && out_grad, UT_EINVAL, "gp_acq_grad: NULL out_mu or out_grad");
  UT_CHECK(c, ld_g >= p, UT_EINVAL, "gp_acq_grad: needs ld_g >= p");
  PolishShape s;
  int rc;
  if ((rc = pl_prepare(c, "gp_acq_grad", values, ld, p, acq, s))) return rc;
  if ((rc = launch_encode_scaled(c, values, ld, p, c->bs_u.p, s.dpad, s.ldp, c->bs_cn.p))) return rc;
  if ((rc = pl_eval(c, s, make_acq(c, acq), out_grad, ld_g))) return rc;
  const double* pv = c->bs_pvec.p;
  const size_t bytes = sizeof(double) * (size_t)p;
  UT_HIP(c, hipMemcpyAsync(out_mu, pv + PV_MU * s.ldp, bytes, hipMemcpyDeviceToDevice, c->stream));
  if (out_var) UT_HIP(c, hipMemcpyAsync(out_var, pv + PV_VAR * s.ldp, bytes, hipMemcpyDeviceToDevice, c->stream));
  if (out_score)
    UT_HIP(c, hipMemcpyAsync(out_score, pv + PV_SCORE * s.ldp, bytes, hipMemcpyDeviceToDevice, c->stream));
  return 0;
}

int gp_polish_impl(ut_ctx* c, const double* values, int64_t ld, int32_t p, const ut_acq* acq, const uint8_t* dup,
                   const ut_polish_params* prm, double* out_values, int64_t ld_o, double* out_score,
                   double* out_score0, uint8_t* out_moved) {
  UT_CHECK(c, prm && out_values && out_score, UT_EINVAL, "gp_polish: NULL prm, out_values or out_score");
  UT_CHECK(c, ld_o >= p, UT_EINVAL, "gp_polish: needs ld_o >= p");
  UT_CHECK(c, prm->steps >= 0, UT_EINVAL, "gp_polish: steps is negative");
  const double step0 = prm->step0 == 0.0 ? 0.25 : prm->step0, step_max = prm->step_max == 0.0 ? 1.0 : prm->step_max;
  const double grow = prm->grow == 0.0 ? 2.0 : prm->grow, shrink = prm->shrink == 0.0 ? 0.5 : prm->shrink;
  for (double v : {step0, step_max, grow, shrink})
    UT_CHECK(c, v > 0.0 && v < 1.0 / 0.0, UT_EINVAL, "gp_polish: step0, step_max, grow and shrink must be positive");
  PolishShape s;
  int rc;
  if ((rc = pl_prepare(c, "gp_polish", values, ld, p, acq, s))) return rc;
  const int32_t T = prm->steps, d = s.d, ncols = c->space.ncols;
  const int64_t ldp = s.ldp;
  if ((rc = ensure(c, c->bs_pu, (size_t)3 * d * ldp))) return rc;
  if ((rc = ensure(c, c->bs_pval, (size_t)ncols * ldp))) return rc;
  const size_t frow = ((size_t)d + 255) / 256 * 256;
  if ((rc = ensure(c, c->bs_pflag, frow + 2 * (size_t)ldp))) return rc;
  double* ucur = c->bs_pu.p;
  double* utrial = ucur + (size_t)d * ldp;
  double* G = utrial + (size_t)d * ldp;
  double* pv = c->bs_pvec.p;
  uint8_t* free_ = c->bs_pflag.p;
  uint8_t* act = free_ + frow;
  uint8_t* accepted = act + ldp;
  const Acq a = make_acq(c, acq);
  const dim3 gp((unsigned)((p + 255) / 256)), gl((unsigned)(ldp / 256)), b(256);
  // s0 at the encoder's operands; the first step's gradient is taken there too
  if ((rc = launch_encode(c, values, ld, p, ucur, ldp))) return rc;
  if ((rc = launch_encode_scaled(c, values, ld, p, c->bs_u.p, s.dpad, ldp, c->bs_cn.p))) return rc;
  if ((rc = pl_eval(c, s, a, T > 0 ? G : nullptr, ldp))) return rc;
  hipLaunchKernelGGL(k_pl_init, gp, b, 0, c->stream, p, pv + PV_SCORE * ldp, step0, pv + PV_S * ldp, pv + PV_S0 * ldp,
                     pv + PV_ETA * ldp, accepted);
  UT_LAUNCH_CHECK(c);
  if (T > 0) {
    UT_HIP(c, hipMemsetAsync(free_, 0, frow, c->stream));
    hipLaunchKernelGGL(k_pl_free, dim3((c->space.P + 255) / 256), b, 0, c->stream, c->space.d_params.p, c->space.P, d,
                       free_);
    UT_LAUNCH_CHECK(c);
  }
  for (int32_t t = 0; t < T; ++t) {
    if (t > 0 && (rc = pl_eval(c, s, a, G, ldp))) return rc;   // (bs_u / bs_cn: k_pl_accept's)
    hipLaunchKernelGGL(k_pl_trial, gl, b, 0, c->stream, d, s.dpad, p, ldp, free_, c->gp_inv_ell.p, ucur, utrial, G,
                       pv + PV_ETA * ldp, dup, act, c->bs_u.p, c->bs_cn.p);
    UT_LAUNCH_CHECK(c);
    if ((rc = pl_eval(c, s, a, nullptr, 0))) return rc;
    hipLaunchKernelGGL(k_pl_accept, gp, b, 0, c->stream, d, s.dpad, p, ldp, act, pv + PV_SCORE * ldp, grow, shrink,
                       step_max, c->gp_inv_ell.p, ucur, utrial, pv + PV_S * ldp, pv + PV_ETA * ldp, accepted,
                       c->bs_u.p, c->bs_cn.p);
    UT_LAUNCH_CHECK(c);
    mark(c, "pl_step");
  }
  // decode, encode again, score: s_v
  hipLaunchKernelGGL(k_pl_decode, gp, b, 0, c->stream, c->space.d_params.p, c->space.P, values, ld, p, ucur, ldp,
                     accepted, c->bs_pval.p);
  UT_LAUNCH_CHECK(c);
  if ((rc = launch_encode_scaled(c, c->bs_pval.p, ldp, p, c->bs_u.p, s.dpad, ldp, c->bs_cn.p))) return rc;
  if ((rc = pl_eval(c, s, a, nullptr, 0))) return rc;
  hipLaunchKernelGGL(k_pl_final, gp, b, 0, c->stream, ncols, p, values, ld, c->bs_pval.p, ldp, pv + PV_SCORE * ldp,
                     pv + PV_S0 * ldp, dup, accepted, out_values, ld_o, out_score, out_score0, out_moved);
  UT_LAUNCH_CHECK(c);
  mark(c, "pl_final");
  return 0;
}

}  // namespace ut
