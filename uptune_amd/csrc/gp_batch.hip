// gp_batch.hip -- batch-aware selection (ut_gp_select_batch): k picks from a
// shortlist of p candidates, each conditioned on the picks before it.  The
// rule (include/uthot.h states it in full), with U the shortlist's features:
//
//   mu = K* alpha = V^T beta,   V = L^-1 K*^T  [n][p],   beta = L^-1 ys
//   Sigma = Kss - V^T V,        Kss_ij = sf2 exp(-1/2 |us_i - us_j|^2)
//   var_i = max(Sigma_ii, 0)
//   for t = 0 .. k-1:
//     s_i = acq(mu_i, var_i)        (-inf: dup or already picked)
//     j   = argmax s                (ties: smallest position; -inf / NaN: this
//                                    and every later slot is empty)
//     c_i = Sigma_ij - sum_{s<t} G_is G_js,   q = c_j + sn2 + jitter
//     G_it = c_i / sqrt(q),   var_i <- max(var_i - G_it^2, 0)
//
// mu and f_best never change (GP-BUCB's variance-only update, for EI too).
// Everything is read from what the fit left on the device (gp_XsT, gp_xnorm,
// gp_Linv, gp_beta, gp_stats, gp_flag); nothing of the fit, of a scoring
// result or of the round buffers is written: the scratch is the context's
// bs_* arrays.  Always fp64 and over every feature (the dense K*), whatever
// ut_gp_set_precision says and whichever K* the fit scores with.
//
//   k_bs_v      V tile = L^-1 [64 rows][k] K*^T [k][64 columns] on the fp64
//               MFMA; L^-1 is lower triangular, so row tile rt stops its k
//               loop at its diagonal tile, (rt + 1) * 64
//   k_bs_mu     mu_i = sum_{r<n} V[r][i] beta_r, rows in order
//   k_bs_sigma  one workgroup per lower 64 x 64 tile (I, J): V^T V over the
//               training rows and us_i . us_j over the features, both by
//               gp_tiles.h's tile product; the RBF term in the epilogue; the
//               tile and its mirror are stored (the loop reads whole rows)
//   k_bs_pick   launch t of k + 1, ceil(p / 256) workgroups, one shortlist
//               row per thread: every workgroup reduces launch t-1's
//               per-workgroup (score, position) partials to the pivot in
//               workgroup order, writes slot t-1, stages the pivot's G row in
//               LDS, forms c_i, updates var_i, rescores and writes its own
//               partial.  The launches are chained on the stream: no
//               cooperative launch, no grid barrier, no spin.
// Every sum runs in a fixed order, so two calls on one fit return the same bits.
#include "gp_post.h"
#include "gp_tiles.h"

namespace ut {

constexpr int32_t BS_MAX_P = 4096;
constexpr int BS_WG = 256;
constexpr int BS_MAX_WG = BS_MAX_P / BS_WG;   // partial slots per launch parity
constexpr int32_t BS_NOPOS = 0x7fffffff;      // the position of a thread past p

// V[row0 .. + 64)[col0 .. + 64) of L^-1 K*^T.  Linv [npad][npad] row-major,
// kst / V [npad][ldp]; grid (column tiles, npad / 64)
__global__ __launch_bounds__(256) void k_bs_v(const double* __restrict__ Linv, int32_t npad,
                                              const double* __restrict__ kst, int64_t ldp, double* __restrict__ V) {
  __shared__ double As[16 * 80];
  __shared__ double Bs[16 * 80];
  const int t = threadIdx.x;
  const int64_t col0 = (int64_t)blockIdx.x * 64, row0 = (int64_t)blockIdx.y * 64;
  fd4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = (fd4){0.0, 0.0, 0.0, 0.0};
  const int32_t kend = (int32_t)row0 + 64;   // (<= npad) the diagonal tile is the last
  for (int32_t k0 = 0; k0 < kend; k0 += 16) {
    for (int e = t; e < 64 * 16; e += 256) {
      const int r = e >> 4, kk = e & 15;
      As[kk * 80 + r] = Linv[(row0 + r) * npad + k0 + kk];
      const int k2 = e >> 6, cc = e & 63;
      Bs[k2 * 80 + cc] = kst[(int64_t)(k0 + k2) * ldp + col0 + cc];
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
      for (int r = 0; r < 4; ++r) V[(row0 + tile_row(a, r)) * ldp + col0 + tile_col(b)] = acc[a][b][r];
}

int launch_bs_v(ut_ctx* c, int32_t CT, int32_t npad, const double* kst, int64_t ldp, double* V) {
  hipLaunchKernelGGL(k_bs_v, dim3(CT, npad / 64), dim3(256), 0, c->stream, c->gp_Linv.p, npad, kst, ldp, V);
  UT_LAUNCH_CHECK(c);
  return 0;
}

__global__ __launch_bounds__(256) void k_bs_mu(const double* __restrict__ V, int64_t ldp, const double* __restrict__ beta,
                                               int32_t n, int32_t p, double* __restrict__ mu) {
  const int32_t i = blockIdx.x * 256 + threadIdx.x;
  if (i >= p) return;
  double s = 0.0;
  for (int32_t r = 0; r < n; ++r) s = __builtin_fma(V[(int64_t)r * ldp + i], beta[r], s);
  mu[i] = s;
}

// Sigma [CT * 64][ldp] from V [npad][ldp] (rows < kend) and the scaled
// features U [dp16][ldp] (dp16 a multiple of 16, the rows past the features
// zero) with their norms cn
__global__ __launch_bounds__(256) void k_bs_sigma(const double* __restrict__ V, const double* __restrict__ U,
                                                  const double* __restrict__ cn, int64_t ldp, int32_t kend,
                                                  int32_t dp16, double sf2, double* __restrict__ Sig) {
  __shared__ double As[16 * 80];
  __shared__ double Bs[16 * 80];
  int32_t ti, tj;
  lower_tile(blockIdx.x, ti, tj);
  const int64_t ib = (int64_t)ti * 64, jb = (int64_t)tj * 64;
  fd4 vv[2][2], dot[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) vv[a][b] = dot[a][b] = (fd4){0.0, 0.0, 0.0, 0.0};
  tile64_tn(V, ldp, ib, jb, 0, kend, As, Bs, vv);
  tile64_tn(U, ldp, ib, jb, 0, dp16, As, Bs, dot);
  double ci[2][4], cj[2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) ci[a][r] = cn[ib + tile_row(a, r)];
#pragma unroll
  for (int b = 0; b < 2; ++b) cj[b] = cn[jb + tile_col(b)];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t i = ib + tile_row(a, r), j = jb + tile_col(b);
        const double d2 = ci[a][r] + cj[b] - 2.0 * dot[a][b][r];
        // (a candidate is at distance 0 from itself whatever the rounding of its norm)
        const double kss = i == j ? sf2 : sf2 * exp(-0.5 * (d2 > 0.0 ? d2 : 0.0));
        const double s = kss - vv[a][b][r];
        Sig[i * ldp + j] = s;
        if (ti != tj) Sig[j * ldp + i] = s;
      }
}

// (sa, pa) is selected before (sb, pb): a NaN first (the maximum of a set
// with a NaN is NaN), then the larger score, then the smaller position
__device__ __forceinline__ bool bs_before(double sa, int32_t pa, double sb, int32_t pb) {
  const bool na = sa != sa, nb = sb != sb;
  if (na || nb) return na && (!nb || pa < pb);
  return sa > sb || (sa == sb && pa < pb);
}

__global__ __launch_bounds__(BS_WG) void k_bs_pick(int32_t t, int32_t p, int32_t k, int64_t ldp,
                                                   const double* __restrict__ Sig, const double* __restrict__ mu,
                                                   double* __restrict__ var, double* __restrict__ G,
                                                   uint8_t* __restrict__ picked, const uint8_t* __restrict__ dup,
                                                   Acq a, double diag, double* __restrict__ pscore,
                                                   int32_t* __restrict__ ppos, int64_t* __restrict__ out_pos,
                                                   double* __restrict__ out_score, double* __restrict__ out_var) {
  __shared__ double gj[BS_MAX_P];   // the pivot's G row (t - 1 <= k - 1 < 4096 entries)
  __shared__ double rs[BS_WG / 64];
  __shared__ int32_t rp[BS_WG / 64];
  const int tid = threadIdx.x;
  const int32_t i = blockIdx.x * BS_WG + tid;
  const bool in = i < p;
  const int32_t nwg = gridDim.x;
  double v = 0.0;
  bool taken = false;
  if (t == 0) {
    if (in) {
      const double s0 = Sig[(int64_t)i * ldp + i];
      v = s0 > 0.0 ? s0 : 0.0;
      var[i] = v;
      picked[i] = 0;
    }
  } else {
    // launch t-1's partials, in workgroup order (every workgroup the same)
    const double* ps = pscore + ((t - 1) & 1) * BS_MAX_WG;
    const int32_t* pp = ppos + ((t - 1) & 1) * BS_MAX_WG;
    double bsc = ps[0];
    int32_t bp = pp[0];
    for (int32_t w = 1; w < nwg; ++w)
      if (bs_before(ps[w], pp[w], bsc, bp)) bsc = ps[w], bp = pp[w];
    const bool empty = bsc != bsc || bsc == -1.0 / 0.0 || bp < 0 || bp >= p;
    if (in) {
      v = var[i];
      taken = picked[i] != 0;
    }
    if (empty) {
      if (blockIdx.x == 0 && tid == 0) {
        out_pos[t - 1] = -1;
        if (out_score) out_score[t - 1] = -1.0 / 0.0;
        if (out_var) out_var[t - 1] = __builtin_nan("");
      }
    } else if (i == bp) {   // the pivot's own thread holds its variance at pick time
      out_pos[t - 1] = bp;
      if (out_score) out_score[t - 1] = bsc;
      if (out_var) out_var[t - 1] = v;
    }
    if (t == k) return;
    if (!empty) {   // (uniform over the grid)
      const int32_t nprev = t - 1;
      for (int32_t s = tid; s < nprev; s += BS_WG) gj[s] = G[(int64_t)s * ldp + bp];
      __syncthreads();
      if (in) {
        double ci = Sig[(int64_t)bp * ldp + i];   // Sigma is symmetric: the pivot's row, coalesced
        double cj = Sig[(int64_t)bp * ldp + bp];
#pragma unroll 8
        for (int32_t s = 0; s < nprev; ++s) {   // (loading 32 rows ahead by hand was slower: 11.0 against 8.8 us per launch)
          const double g = gj[s];
          ci = __builtin_fma(-G[(int64_t)s * ldp + i], g, ci);
          cj = __builtin_fma(-g, g, cj);
        }
        const double gi = ci / sqrt(cj + diag);
        G[(int64_t)nprev * ldp + i] = gi;
        const double nv = v - gi * gi;
        v = nv > 0.0 ? nv : 0.0;
        var[i] = v;
        if (i == bp) {
          taken = true;
          picked[i] = 1;
        }
      }
    }
  }
  double sc = -1.0 / 0.0;
  int32_t pos = BS_NOPOS;
  if (in) {
    pos = i;
    sc = a.score(mu[i], v);
    if (*a.fit_flag != 0) sc = __builtin_nan("");   // failed fit: nothing is selectable
    if (taken || (dup && dup[i])) sc = -1.0 / 0.0;
  }
  // the workgroup's first: lanes by xor-shuffles, then the four waves in order
  for (int off = 32; off > 0; off >>= 1) {
    const double so = __shfl_xor(sc, off);
    const int32_t po = __shfl_xor(pos, off);
    if (bs_before(so, po, sc, pos)) sc = so, pos = po;
  }
  if ((tid & 63) == 0) rs[tid >> 6] = sc, rp[tid >> 6] = pos;
  __syncthreads();
  if (tid == 0) {
    for (int w = 1; w < BS_WG / 64; ++w)
      if (bs_before(rs[w], rp[w], sc, pos)) sc = rs[w], pos = rp[w];
    pscore[(t & 1) * BS_MAX_WG + blockIdx.x] = sc;
    ppos[(t & 1) * BS_MAX_WG + blockIdx.x] = pos;
  }
}

int gp_select_batch_impl(ut_ctx* c, const double* values, int64_t ld, int32_t p, const ut_acq* acq,
                         const uint8_t* dup, int32_t k, int64_t* out_pos, double* out_score, double* out_var) {
  UT_CHECK(c, values && acq && out_pos, UT_EINVAL, "gp_select_batch: NULL values, acq or out_pos");
  UT_CHECK(c, p >= 1 && p <= BS_MAX_P && k >= 1 && k <= p && ld >= p, UT_EINVAL,
           "gp_select_batch: needs 1 <= k <= p <= 4096 and ld >= p");
  UT_CHECK(c, c->gp_ready, UT_EINVAL, "gp_score: call ut_gp_fit first");
  int rc;
  if ((rc = gp_fit_flush(c))) return rc;
  UT_CHECK(c, c->has_space && c->space.n_feat == c->gp_d, UT_EINVAL,
           "gp_select_batch: the fit's feature count is not the space's");
  // the whole fit (L^-1, beta), on the device
  if (c->fit_pending) UT_HIP(c, hipStreamWaitEvent(c->stream, c->ev_fit, 0));
  const int32_t n = c->gp_n, npad = c->gp_npad_fit;
  UT_CHECK(c, npad == gp_npad(n) && npad % 64 == 0, UT_EINVAL, "gp_select_batch: no fitted GP");
  const int32_t dpad = kstar_dpad(c->gp_d), dp16 = (dpad + 15) / 16 * 16;
  const int64_t ldp = gp_ldk(p);
  const int32_t CT = (p + 63) / 64, nwg = (p + BS_WG - 1) / BS_WG;
  const int32_t kend = (n + 15) / 16 * 16;   // (<= npad) V is zero in the padding rows
  // bs_vec: mu [ldp] | var [ldp] | the partial scores [2][16]
  if ((rc = ensure(c, c->bs_u, (size_t)dp16 * ldp))) return rc;
  if ((rc = ensure(c, c->bs_cn, (size_t)ldp))) return rc;
  if ((rc = ensure(c, c->bs_kst, (size_t)npad * ldp))) return rc;
  if ((rc = ensure(c, c->bs_v, (size_t)npad * ldp))) return rc;
  if ((rc = ensure(c, c->bs_sig, (size_t)CT * 64 * ldp))) return rc;
  if ((rc = ensure(c, c->bs_g, (size_t)k * ldp))) return rc;
  if ((rc = ensure(c, c->bs_vec, (size_t)2 * ldp + 2 * BS_MAX_WG))) return rc;
  if ((rc = ensure(c, c->bs_pos, (size_t)2 * BS_MAX_WG))) return rc;
  if ((rc = ensure(c, c->bs_picked, (size_t)ldp))) return rc;
  double* mu = c->bs_vec.p;
  double* var = mu + ldp;
  double* pscore = var + ldp;
  // K*^T over every feature: the dense operands, whichever K* the fit scores with
  if (dp16 > dpad)
    UT_HIP(c, hipMemsetAsync(c->bs_u.p + (size_t)dpad * ldp, 0, sizeof(double) * (size_t)(dp16 - dpad) * ldp, c->stream));
  if ((rc = launch_encode_scaled(c, values, ld, p, c->bs_u.p, dpad, ldp, c->bs_cn.p))) return rc;
  KstarArgs ka;
  ka.train = KstarTrain{c->gp_XsT.p};
  ka.ucand = c->bs_u.p, ka.dpad = dpad, ka.cn = c->bs_cn.p;
  ka.m = p, ka.kst = c->bs_kst.p, ka.ldk = ldp;
  if ((rc = launch_gemm_kstar(c, 64, npad, ka))) return rc;
  mark(c, "bs_kstar");
  hipLaunchKernelGGL(k_bs_v, dim3(CT, npad / 64), dim3(256), 0, c->stream, c->gp_Linv.p, npad, c->bs_kst.p, ldp,
                     c->bs_v.p);
  hipLaunchKernelGGL(k_bs_mu, dim3(nwg), dim3(256), 0, c->stream, c->bs_v.p, ldp, c->gp_beta.p, n, p, mu);
  UT_LAUNCH_CHECK(c);
  mark(c, "bs_v");
  hipLaunchKernelGGL(k_bs_sigma, dim3(CT * (CT + 1) / 2), dim3(256), 0, c->stream, c->bs_v.p, c->bs_u.p, c->bs_cn.p,
                     ldp, kend, dp16, c->gp_sf2, c->bs_sig.p);
  UT_LAUNCH_CHECK(c);
  mark(c, "bs_sigma");
  const Acq pa = make_acq(c, acq);
  for (int32_t t = 0; t <= k; ++t)
    hipLaunchKernelGGL(k_bs_pick, dim3(nwg), dim3(BS_WG), 0, c->stream, t, p, k, ldp, c->bs_sig.p, mu, var, c->bs_g.p,
                       c->bs_picked.p, dup, pa, c->gp_diag_fit, pscore, c->bs_pos.p, out_pos, out_score, out_var);
  UT_LAUNCH_CHECK(c);
  mark(c, "bs_loop");
  return 0;
}

}  // namespace ut
