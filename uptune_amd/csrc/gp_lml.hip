// gp_lml.hip -- log marginal likelihood of the GP surrogate (standardised y):
//
//   lml = -1/2 |beta|^2 - sum_{i<n} log L_ii - (n/2) log 2 pi,
//   beta = L^-1 ys,  L = chol(K + (sn2 + jitter) I)
//
// with K, ys and the standardisation of oracle/gp.py.  The reference has no
// GP, so no marginal likelihood either; this is what chooses
// the lengthscale the reference never had to choose.
//
// ut_gp_lml: the fit in place already holds L's diagonal (gp_K) and beta
// (gp_beta), so its LML is one reduction (k_lml_fit).
//
// ut_gp_lml_grid: g hyperparameter points (a common scale on the ARD
// lengthscales and a noise each) over one training set are g independent
// factorisations of one size -- the launches a single fit's serial chain cannot
// fill the chip with.  A chunk of B points goes through ONE chain of launches,
// every kernel with the point as a grid dimension:
//   |xs_i - xs_j|^2 once (k_lml_d2), K_z from it per point (k_lml_kmat), then
//   per 64-column panel the fit's three steps (diagonal block, row blocks,
//   trailing update; gp_tiles.h), and one reduction.
// The launch count depends on npad alone.  No L^-1 is formed: the right-hand
// side rides through the panel loop.  After panel kb's diagonal step
// beta_kb = inv(L_kk) r_kb, and the workgroup that has just produced L_i,kb
// takes L_i,kb beta_kb off r_i.  Each point has its own not-positive-definite
// flag and its own buffers, so a failed point is a NaN in its own slot only.
#include <cmath>

#include "gp_tiles.h"
#include "ut_internal.h"

namespace ut {

constexpr size_t LML_BUDGET = (size_t)1 << 30;      // bytes of K_z matrices one chunk may hold

// sum over rows < n of log L_ii and of beta_i^2 -> the LML; one workgroup
__device__ __forceinline__ double lml_reduce(const double* __restrict__ L, const double* __restrict__ beta, int32_t n,
                                             int32_t npad, double* red) {
  const int t = threadIdx.x;
  double sl = 0.0, sb = 0.0;
  for (int32_t i = t; i < n; i += 256) {
    sl += log(L[(int64_t)i * npad + i]);
    const double b = beta[i];
    sb += b * b;
  }
  red[t] = sl;
  red[256 + t] = sb;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) {
      red[t] += red[t + w];
      red[256 + t] += red[256 + t + w];
    }
    __syncthreads();
  }
  return -0.5 * red[256] - red[0] - 0.5 * (double)n * 1.8378770664093454836;   // log 2 pi
}

// the current fit: out points to pinned host memory
__global__ __launch_bounds__(256) void k_lml_fit(const double* __restrict__ L, const double* __restrict__ beta,
                                                 const int32_t* __restrict__ flag, int32_t n, int32_t npad,
                                                 double* __restrict__ out) {
  __shared__ double red[512];
  const double v = lml_reduce(L, beta, n, npad, red);
  if (threadIdx.x == 0) out[0] = *flag != 0 ? __builtin_nan("") : v;
}

// D2[i][j] = max(|xs_i|^2 + |xs_j|^2 - 2 xs_i . xs_j, 0) (k_gp_kmat's distance), lower tiles
__global__ __launch_bounds__(256) void k_lml_d2(const double* __restrict__ Xs, const double* __restrict__ xnorm,
                                                int32_t npad, int32_t d, double* __restrict__ D2) {
  __shared__ double As[16 * 80];
  __shared__ double Bs[16 * 80];
  int32_t ti, tj;
  lower_tile(blockIdx.x, ti, tj);
  const int64_t ib = (int64_t)ti * 64, jb = (int64_t)tj * 64;
  fd4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = (fd4){0.0, 0.0, 0.0, 0.0};
  tile64_nt(Xs + ib * d, d, Xs + jb * d, d, d, As, Bs, acc);
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t i = ib + tile_row(a, r), j = jb + tile_col(b);
        const double d2 = xnorm[i] + xnorm[j] - 2.0 * acc[a][b][r];
        D2[i * npad + j] = d2 > 0.0 ? d2 : 0.0;
      }
}

// K_z = sf2 exp(-D2 hs_z) + dg_z I for the chunk's points z0 + blockIdx.y
// (hs = 0.5 / scale^2); rows / columns >= n form an identity block; lower tiles
__global__ __launch_bounds__(256) void k_lml_kmat(const double* __restrict__ D2, int32_t n, int32_t npad, double sf2,
                                                  const double* __restrict__ hs, const double* __restrict__ dg,
                                                  int32_t z0, double* __restrict__ K) {
  int32_t ti, tj;
  lower_tile(blockIdx.x, ti, tj);
  const int64_t ib = (int64_t)ti * 64, jb = (int64_t)tj * 64;
  const double h = hs[z0 + blockIdx.y], diag = dg[z0 + blockIdx.y];
  double* Kz = K + (int64_t)blockIdx.y * npad * npad;
  for (int e = threadIdx.x; e < 64 * 64; e += 256) {
    const int64_t i = ib + (e >> 6), j = jb + (e & 63);
    double v;
    if (i >= n || j >= n) {
      v = (i == j) ? 1.0 : 0.0;
    } else {
      v = sf2 * exp(-(D2[i * npad + j] * h));
      if (i == j) v += diag;
    }
    Kz[i * npad + j] = v;
  }
}

// every point's right-hand side starts as ys
__global__ void k_lml_rhs(const double* __restrict__ ys, int32_t npad, double* __restrict__ rhs) {
  const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < npad) rhs[(int64_t)blockIdx.y * npad + i] = ys[i];
}

// Panel kb, step 1, one workgroup per point: L_kk = chol(A_kk) into K_z,
// inv(L_kk) into the point's stripe Li_z [64][npad] (columns 0 .. 63), then
// beta_kb = inv(L_kk) r_kb in place (one wave per 16 rows, a lane per column)
__global__ __launch_bounds__(256) void k_lml_diag(double* __restrict__ K, double* __restrict__ Li,
                                                  double* __restrict__ rhs, int32_t npad, int32_t kb,
                                                  int32_t* __restrict__ flag) {
  __shared__ double col[2][NB];
  __shared__ double invd[NB];
  __shared__ double rv[NB];
  const int t = threadIdx.x, r = t & 63;
  const int g = __builtin_amdgcn_readfirstlane(t >> 6);
  const int64_t base = (int64_t)kb * NB;
  double* Kb = K + (int64_t)blockIdx.x * npad * npad + base * npad + base;   // the block's origin
  double* Lz = Li + (int64_t)blockIdx.x * NB * npad;
  double* rz = rhs + (int64_t)blockIdx.x * npad + base;
  double a[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) a[j] = Kb[(int64_t)r * npad + 16 * g + j];
  chol_diag_core<true>(a, Kb, Lz, npad, 0, flag + blockIdx.x, col, nullptr, invd);
  if (t < NB) rv[t] = rz[t];
  __syncthreads();   // inv(L_kk) written by this workgroup, r_kb staged
  for (int q = 0; q < 16; ++q) {
    const int row = 16 * g + q;
    double s = Lz[(int64_t)row * npad + r] * rv[r];   // (zeros above the diagonal)
    for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
    if (r == 0) rz[row] = s;
  }
}

// Panel kb, step 2: row block i > kb of point blockIdx.y: L_i,kb = A_i,kb inv(L_kk)^T,
// then r_i -= L_i,kb beta_kb from the accumulators (16 lanes share a row, the
// two column waves meet in LDS)
__global__ __launch_bounds__(256) void k_lml_rows(double* __restrict__ K, const double* __restrict__ Li,
                                                  double* __restrict__ rhs, int32_t npad, int32_t kb) {
  __shared__ double As[16 * 80];
  __shared__ double Bs[16 * 80];
  __shared__ double red[2][NB];
  const int64_t base = (int64_t)kb * NB, rb = (int64_t)(kb + 1 + blockIdx.x) * NB;
  double* Kz = K + (int64_t)blockIdx.y * npad * npad;
  const double* Lz = Li + (int64_t)blockIdx.y * NB * npad;
  double* rz = rhs + (int64_t)blockIdx.y * npad;
  fd4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (fd4){0.0, 0.0, 0.0, 0.0};
  tile64_nt(Kz + rb * npad + base, npad, Lz, npad, NB, As, Bs, acc);
  double bet[2];
#pragma unroll
  for (int j = 0; j < 2; ++j) bet[j] = rz[base + tile_col(j)];
  const int lane = threadIdx.x & 63, wc = (threadIdx.x >> 6) & 1;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int r = 0; r < 4; ++r) {
      double p = 0.0;
#pragma unroll
      for (int j = 0; j < 2; ++j) {
        Kz[(rb + tile_row(i, r)) * npad + base + tile_col(j)] = acc[i][j][r];
        p = __builtin_fma(acc[i][j][r], bet[j], p);
      }
      for (int off = 8; off > 0; off >>= 1) p += __shfl_xor(p, off);
      if ((lane & 15) == 0) red[wc][tile_row(i, r)] = p;
    }
  __syncthreads();
  if (threadIdx.x < NB) rz[rb + threadIdx.x] -= red[0][threadIdx.x] + red[1][threadIdx.x];
}

// Trailing update A_ij -= L_i,kb L_j,kb^T for kb < j <= i < nb, point blockIdx.y
__global__ __launch_bounds__(256) void k_lml_update(double* __restrict__ K, int32_t npad, int32_t kb) {
  __shared__ double As[16 * 80];
  __shared__ double Bs[16 * 80];
  int32_t i, j;
  lower_tile(blockIdx.x, i, j);
  double* Kz = K + (int64_t)blockIdx.y * npad * npad;
  const int64_t ib = (int64_t)(kb + 1 + i) * NB, jb = (int64_t)(kb + 1 + j) * NB, cb = (int64_t)kb * NB;
  fd4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = (fd4){0.0, 0.0, 0.0, 0.0};
  tile64_nt(Kz + ib * npad + cb, npad, Kz + jb * npad + cb, npad, NB, As, Bs, acc);
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) Kz[(ib + tile_row(a, r)) * npad + jb + tile_col(b)] -= acc[a][b][r];
}

// the chunk's LML values, NaN where the point's flag is set; one workgroup per point
__global__ __launch_bounds__(256) void k_lml_points(const double* __restrict__ K, const double* __restrict__ rhs,
                                                    const int32_t* __restrict__ flag, int32_t n, int32_t npad,
                                                    double* __restrict__ out) {
  __shared__ double red[512];
  const double v = lml_reduce(K + (int64_t)blockIdx.x * npad * npad, rhs + (int64_t)blockIdx.x * npad, n, npad, red);
  if (threadIdx.x == 0) out[blockIdx.x] = flag[blockIdx.x] != 0 ? __builtin_nan("") : v;
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
int gp_lml_impl(ut_ctx* c, double* lml_host) {
  UT_CHECK(c, lml_host != nullptr, UT_EINVAL, "gp_lml: NULL output");
  UT_CHECK(c, c->gp_ready || c->fit_pending, UT_EINVAL, "gp_lml: call ut_gp_fit first");
  int rc;
  if ((rc = gp_wait_fit(c))) return rc;   // a staged fit is flushed, a failed one reported
  UT_CHECK(c, c->gp_ready && c->gp_K.p && c->gp_beta.p, UT_EINVAL, "gp_lml: no fitted GP");
  if (!c->lml_host) UT_HIP(c, hipHostMalloc((void**)&c->lml_host, sizeof(double), hipHostMallocDefault));
  // the fit stream is idle (gp_wait_fit); scoring on the caller's stream only reads the factor
  hipLaunchKernelGGL(k_lml_fit, dim3(1), dim3(256), 0, c->stream, c->gp_K.p, c->gp_beta.p, c->gp_flag.p, c->gp_n,
                     c->gp_npad_fit, c->lml_host);
  UT_LAUNCH_CHECK(c);
  UT_HIP(c, hipStreamSynchronize(c->stream));
  *lml_host = *c->lml_host;
  return 0;
}

int gp_lml_grid_impl(ut_ctx* c, const double* X, const double* y, int32_t n, int32_t d, const ut_gp_hyper* h,
                     int32_t g, const double* scale, const double* noise, double* lml_host, int32_t* best_host) {
  UT_CHECK(c, n >= 1 && d >= 1 && g >= 1, UT_EINVAL, "gp_lml_grid: n, d and g must be at least 1");
  UT_CHECK(c, X && y && h && h->lengthscale_host && scale && lml_host && best_host, UT_EINVAL,
           "gp_lml_grid: NULL argument");
  for (int32_t z = 0; z < g; ++z)
    UT_CHECK(c, std::isfinite(scale[z]) && scale[z] > 0.0, UT_EINVAL, "gp_lml_grid: scales must be finite and > 0");
  const int64_t npad = gp_npad(n);   // the fit's padding
  const int32_t nb = (int32_t)(npad / NB);
  const size_t mat = (size_t)npad * npad;
  int64_t B = c->lml_batch > 0 ? c->lml_batch : (int64_t)(LML_BUDGET / (mat * sizeof(double)));
  B = std::max<int64_t>(1, std::min<int64_t>(B, g));
  // lml_in: X | y | 1/ell | scaled rows | norms | ys | stats | hs | dg | lml
  const size_t oy = (size_t)n * d, oinv = oy + n, oXs = oinv + d, oxn = oXs + (size_t)npad * d, oys = oxn + npad;
  const size_t ost = oys + npad, ohs = ost + 4, odg = ohs + g, olml = odg + g;
  int rc;
  if ((rc = ensure(c, c->lml_in, olml + g))) return rc;
  if ((rc = ensure(c, c->lml_d2, mat))) return rc;
  if ((rc = ensure(c, c->lml_k, (size_t)B * mat))) return rc;
  if ((rc = ensure(c, c->lml_li, (size_t)B * NB * npad))) return rc;
  if ((rc = ensure(c, c->lml_rhs, (size_t)B * npad))) return rc;
  if ((rc = ensure(c, c->lml_flag, (size_t)g))) return rc;
  double* in = c->lml_in.p;
  // the small host arrays: 1/ell, then per point 0.5 / scale^2 and the diagonal
  std::vector<double> hp((size_t)d + 2 * g);
  for (int32_t k = 0; k < d; ++k) hp[k] = 1.0 / h->lengthscale_host[k];
  for (int32_t z = 0; z < g; ++z) {
    hp[(size_t)d + z] = 0.5 / (scale[z] * scale[z]);
    hp[(size_t)d + g + z] = (noise ? noise[z] : h->sigma_n2) + h->jitter;
  }
  const int32_t ntile = nb * (nb + 1) / 2;
  auto enqueue = [&]() -> int {
  UT_HIP(c, hipMemcpyAsync(in, X, sizeof(double) * oy, hipMemcpyHostToDevice, c->stream));
  UT_HIP(c, hipMemcpyAsync(in + oy, y, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
  UT_HIP(c, hipMemcpyAsync(in + oinv, hp.data(), sizeof(double) * d, hipMemcpyHostToDevice, c->stream));
  UT_HIP(c, hipMemcpyAsync(in + ohs, hp.data() + d, sizeof(double) * 2 * g, hipMemcpyHostToDevice, c->stream));
  UT_HIP(c, hipMemsetAsync(c->lml_flag.p, 0, sizeof(int32_t) * g, c->stream));
  if ((rc = launch_gp_prep_train(c, in, n, (int32_t)npad, d, in + oinv, in + oXs, in + oxn))) return rc;
  if ((rc = launch_gp_ystats(c, in + oy, n, (int32_t)npad, in + oys, in + ost))) return rc;
  hipLaunchKernelGGL(k_lml_d2, dim3(ntile), dim3(256), 0, c->stream, in + oXs, in + oxn, (int32_t)npad, d,
                     c->lml_d2.p);
  UT_LAUNCH_CHECK(c);
  for (int32_t z0 = 0; z0 < g; z0 += (int32_t)B) {
    const int32_t bz = std::min<int32_t>((int32_t)B, g - z0);
    hipLaunchKernelGGL(k_lml_kmat, dim3(ntile, bz), dim3(256), 0, c->stream, c->lml_d2.p, n, (int32_t)npad,
                       h->sigma_f2, in + ohs, in + odg, z0, c->lml_k.p);
    hipLaunchKernelGGL(k_lml_rhs, dim3(grid1(npad, 256), bz), dim3(256), 0, c->stream, in + oys, (int32_t)npad,
                       c->lml_rhs.p);
    for (int32_t kb = 0; kb < nb; ++kb) {
      hipLaunchKernelGGL(k_lml_diag, dim3(bz), dim3(256), 0, c->stream, c->lml_k.p, c->lml_li.p, c->lml_rhs.p,
                         (int32_t)npad, kb, c->lml_flag.p + z0);
      const int32_t T = nb - kb - 1;
      if (T > 0) {
        hipLaunchKernelGGL(k_lml_rows, dim3(T, bz), dim3(256), 0, c->stream, c->lml_k.p, c->lml_li.p, c->lml_rhs.p,
                           (int32_t)npad, kb);
        hipLaunchKernelGGL(k_lml_update, dim3(T * (T + 1) / 2, bz), dim3(256), 0, c->stream, c->lml_k.p,
                           (int32_t)npad, kb);
      }
    }
    hipLaunchKernelGGL(k_lml_points, dim3(bz), dim3(256), 0, c->stream, c->lml_k.p, c->lml_rhs.p,
                       c->lml_flag.p + z0, n, (int32_t)npad, in + olml + z0);
    UT_LAUNCH_CHECK(c);
  }
  UT_HIP(c, hipMemcpyAsync(lml_host, in + olml, sizeof(double) * g, hipMemcpyDeviceToHost, c->stream));
  return 0;
  };
  // the caller's arrays and hp are read by copies in flight: wait whatever happened
  rc = enqueue();
  const hipError_t es = hipStreamSynchronize(c->stream);
  if (rc) return rc;
  UT_HIP(c, es);
  int32_t best = -1;
  for (int32_t z = 0; z < g; ++z) {
    if (!std::isfinite(lml_host[z])) {
      lml_host[z] = std::nan("");
      continue;
    }
    if (best < 0 || lml_host[z] > lml_host[best]) best = z;
  }
  *best_host = best;
  return 0;
}

}  // namespace ut
