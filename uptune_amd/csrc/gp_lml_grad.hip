// gp_lml_grad.hip -- gradient of the log marginal likelihood of the fit in
// place (ut_gp_lml_grad), with K, ys and the standardisation of oracle/gp.py
// and gp_lml.hip:
//
//   W  = alpha alpha^T - K^-1,   K^-1 = L^-T L^-1,   alpha = L^-T beta
//   Kf_ij = sf2 exp(-1/2 |xs_i - xs_j|^2),   M = W o Kf
//   dLML / dlog ell_k = 1/2 sum_ij M_ij (xs_ik - xs_jk)^2
//   dLML / dlog sf2   = 1/2 sum_ij M_ij
//   dLML / dlog sn2   = 1/2 sn2 tr W              (the jitter is a constant)
//
// over the n real rows.  Everything is read from what the fit left on the
// device (gp_Linv, gp_beta, gp_Xs, gp_xnorm); nothing of the fit or of the
// scoring state is written, alpha included (a precision-8 refit has not formed
// it yet: k_grad_alpha makes a copy in the scratch).  Always fp64.
//
// k_grad_tile, one workgroup per lower 64 x 64 tile (I, J), J <= I:
//   (K^-1)_ij = sum_{r >= max(i, j)} Linv[r][i] Linv[r][j] on the fp64 MFMA, the
//   k range starting at row 64 I (L^-1 is zero above its diagonal) and ending
//   at n; xs_i . xs_j by gp_tiles.h's tile product and the distance of
//   k_lml_d2 from it; M in registers (rows / columns >= n are 0); then one more
//   pass over the features, 16 at a time through LDS, for the tile's share
//   of every component in the direct form sum M (xs_ik - xs_jk)^2, which has
//   no cancellation.  M is symmetric, so an off-diagonal tile counts twice.
// Components are summed in a fixed order (lanes by xor-shuffles, waves and
// then tiles in index order: k_grad_sum), so two calls give the same bits.
#include <cmath>

#include "gp_tiles.h"
#include "ut_internal.h"

namespace ut {

// alpha_i = sum_{r >= i, r < n} Linv[r][i] beta_r for 64 columns per workgroup
// (4 row groups meet in LDS)
__global__ __launch_bounds__(256) void k_grad_alpha(const double* __restrict__ Linv, const double* __restrict__ beta,
                                                    int32_t n, int32_t npad, double* __restrict__ alpha) {
  __shared__ double red[4][64];
  const int t = threadIdx.x, cidx = t & 63, g = t >> 6;
  const int32_t i = blockIdx.x * 64 + cidx;
  double s = 0.0;
  for (int32_t r = blockIdx.x * 64 + g; r < n; r += 4) s = __builtin_fma(Linv[(int64_t)r * npad + i], beta[r], s);
  red[g][cidx] = s;
  __syncthreads();
  if (t < 64) alpha[i] = i < n ? (red[0][t] + red[1][t]) + (red[2][t] + red[3][t]) : 0.0;
}

// the workgroup's sum of s in lane / wave order; red [4]; every thread gets it
__device__ __forceinline__ double wg_sum(double s, double* red) {
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  __syncthreads();   // red's previous readers are done
  if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = s;
  __syncthreads();
  return (red[0] + red[1]) + (red[2] + red[3]);
}

// part [tiles][d + 2]: the tile's share of dlog_ell [d], of 1/2 sum M and of 1/2 tr W
__global__ __launch_bounds__(256) void k_grad_tile(const double* __restrict__ Linv, const double* __restrict__ alpha,
                                                   const double* __restrict__ Xs, const double* __restrict__ xnorm,
                                                   int32_t n, int32_t npad, int32_t d, double sf2,
                                                   double* __restrict__ part) {
  __shared__ double As[16 * 80];
  __shared__ double Bs[16 * 80];
  __shared__ double red[4][16];
  int32_t ti, tj;
  lower_tile(blockIdx.x, ti, tj);
  const int64_t ib = (int64_t)ti * 64, jb = (int64_t)tj * 64;
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  double* out = part + (int64_t)blockIdx.x * (d + 2);
  fd4 kin[2][2], dot[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) kin[a][b] = dot[a][b] = (fd4){0.0, 0.0, 0.0, 0.0};
  const int32_t kend = (n + 15) / 16 * 16;   // (<= npad) rows >= n of L^-1 are zero in the columns < n
  tile64_tn(Linv, npad, ib, jb, (int32_t)ib, kend, As, Bs, kin);
  tile64_nt(Xs + ib * d, d, Xs + jb * d, d, d, As, Bs, dot);
  // M = (alpha_i alpha_j - K^-1_ij) Kf_ij in place of K^-1; the diagonal's W_ii on the way
  const double wt = ti == tj ? 0.5 : 1.0;   // 1/2 (once) or 1/2 (twice: the mirrored tile)
  double al[2][4], xi[2][4], aj[2], xj[2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      al[a][r] = alpha[ib + tile_row(a, r)];
      xi[a][r] = xnorm[ib + tile_row(a, r)];
    }
#pragma unroll
  for (int b = 0; b < 2; ++b) {
    aj[b] = alpha[jb + tile_col(b)];
    xj[b] = xnorm[jb + tile_col(b)];
  }
  double sm = 0.0, sw = 0.0;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t i = ib + tile_row(a, r), j = jb + tile_col(b);
        const double d2 = xi[a][r] + xj[b] - 2.0 * dot[a][b][r];
        const double wij = al[a][r] * aj[b] - kin[a][b][r];
        const bool in = i < n && j < n;
        const double m = in ? wij * (sf2 * exp(-0.5 * (d2 > 0.0 ? d2 : 0.0))) : 0.0;
        kin[a][b][r] = m;
        sm += m;
        if (in && i == j) sw += wij;
      }
  sm = wg_sum(sm, &red[0][0]);
  sw = wg_sum(sw, &red[0][0]);
  if (t == 0) {
    out[d] = wt * sm;
    out[d + 1] = ti == tj ? 0.5 * sw : 0.0;
  }
  // the features, 16 at a time: As / Bs [kk][row] hold xs of the tile's rows / columns
  for (int32_t k0 = 0; k0 < d; k0 += 16) {
    __syncthreads();   // the previous chunk's readers of As / Bs / red are done
    for (int e = t; e < 64 * 16; e += 256) {
      const int r = e >> 4, kk = e & 15;
      const bool in = (k0 + kk) < d;
      As[kk * 80 + r] = in ? Xs[(ib + r) * d + k0 + kk] : 0.0;
      Bs[kk * 80 + r] = in ? Xs[(jb + r) * d + k0 + kk] : 0.0;
    }
    __syncthreads();
#pragma unroll 4
    for (int kk = 0; kk < 16; ++kk) {
      double xa[2][4], xb[2];
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int r = 0; r < 4; ++r) xa[a][r] = As[kk * 80 + tile_row(a, r)];
#pragma unroll
      for (int b = 0; b < 2; ++b) xb[b] = Bs[kk * 80 + tile_col(b)];
      double s = 0.0;
#pragma unroll
      for (int a = 0; a < 2; ++a)
#pragma unroll
        for (int b = 0; b < 2; ++b)
#pragma unroll
          for (int r = 0; r < 4; ++r) {
            const double df = xa[a][r] - xb[b];
            s = __builtin_fma(kin[a][b][r] * df, df, s);
          }
      for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
      if (lane == 0) red[w][kk] = s;
    }
    __syncthreads();
    if (t < 16 && k0 + t < d) out[k0 + t] = wt * ((red[0][t] + red[1][t]) + (red[2][t] + red[3][t]));
  }
}

// out[k] = sum over the tiles of part[tile][k], in tile order; one workgroup per component
__global__ __launch_bounds__(256) void k_grad_sum(const double* __restrict__ part, int32_t tiles, int32_t dp,
                                                  double* __restrict__ out) {
  __shared__ double red[256];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int32_t z = t; z < tiles; z += 256) s += part[(int64_t)z * dp + blockIdx.x];
  red[t] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  if (t == 0) out[blockIdx.x] = red[0];
}

int gp_lml_grad_impl(ut_ctx* c, int32_t d, double* dlog_ell_host, double* dlog_sf2_host, double* dlog_sn2_host) {
  UT_CHECK(c, dlog_ell_host != nullptr, UT_EINVAL, "gp_lml_grad: NULL output");
  UT_CHECK(c, c->gp_ready || c->fit_pending, UT_EINVAL, "gp_lml_grad: call ut_gp_fit first");
  int rc;
  if ((rc = gp_wait_fit(c))) return rc;   // a staged fit is flushed, a failed one reported
  UT_CHECK(c, c->gp_ready && c->gp_Linv.p && c->gp_beta.p, UT_EINVAL, "gp_lml_grad: no fitted GP");
  UT_CHECK(c, d == c->gp_d, UT_EINVAL, "gp_lml_grad: d is not the fit's");
  const int32_t n = c->gp_n, npad = c->gp_npad_fit, nb = npad / NB, dp = d + 2;
  const int32_t tiles = nb * (nb + 1) / 2;
  // lml_grad: alpha [npad] | the components [d + 2] | the tiles' shares [tiles][d + 2]
  const size_t oout = (size_t)npad, opart = oout + dp;
  if ((rc = ensure(c, c->lml_grad, opart + (size_t)tiles * dp))) return rc;
  double* g = c->lml_grad.p;
  // the fit stream is idle (gp_wait_fit); scoring on the caller's stream only reads the factor
  hipLaunchKernelGGL(k_grad_alpha, dim3(nb), dim3(256), 0, c->stream, c->gp_Linv.p, c->gp_beta.p, n, npad, g);
  hipLaunchKernelGGL(k_grad_tile, dim3(tiles), dim3(256), 0, c->stream, c->gp_Linv.p, g, c->gp_Xs.p, c->gp_xnorm.p, n,
                     npad, d, c->gp_sf2, g + opart);
  hipLaunchKernelGGL(k_grad_sum, dim3(dp), dim3(256), 0, c->stream, g + opart, tiles, dp, g + oout);
  UT_LAUNCH_CHECK(c);
  std::vector<double> out((size_t)dp);
  UT_HIP(c, hipMemcpyAsync(out.data(), g + oout, sizeof(double) * dp, hipMemcpyDeviceToHost, c->stream));
  UT_HIP(c, hipStreamSynchronize(c->stream));
  std::copy(out.begin(), out.begin() + d, dlog_ell_host);
  if (dlog_sf2_host) *dlog_sf2_host = out[d];
  if (dlog_sn2_host) *dlog_sn2_host = c->gp_sn2_fit * out[d + 1];
  return 0;
}

}  // namespace ut
