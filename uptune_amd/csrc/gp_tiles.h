// gp_tiles.h -- device building blocks of the blocked Cholesky shared by the
// GP fit (gp_fit.hip), the batched log-marginal-likelihood grid (gp_lml.hip)
// and its gradient (gp_lml_grad.hip): the 64 x 64 fp64-MFMA tile product, its
// accumulator -> tile coordinates, the lower-triangle tile numbering and the
// diagonal-block factor + inverse.
#pragma once
#include "ut_internal.h"

namespace ut {

constexpr int NB = 64;     // Cholesky / inverse block

// 64 x 64 tile  acc = A[64 x K] * B[64 x K]^T  (both row-major in global,
// leading dims lda / ldb) on v_mfma_f64_16x16x4; each wave 32 x 32.
typedef double fd4 __attribute__((ext_vector_type(4)));
// one staged 16-k step: As / Bs [16][80] hold the operands k-major (element (k, row) at k * 80 + row)
__device__ __forceinline__ void tile64_step(const double* As, const double* Bs, fd4 (&acc)[2][2]) {
  const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int wr = w >> 1, wc = w & 1;
#pragma unroll
  for (int ks = 0; ks < 4; ++ks) {
    const int kr = ks * 4 + (lane >> 4);
    double af[2], bf[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) af[i] = As[kr * 80 + wr * 32 + i * 16 + (lane & 15)];
#pragma unroll
    for (int j = 0; j < 2; ++j) bf[j] = Bs[kr * 80 + wc * 32 + j * 16 + (lane & 15)];
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
      for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i], bf[j], acc[i][j], 0, 0, 0);
  }
}

__device__ void tile64_nt(const double* __restrict__ A, int64_t lda, const double* __restrict__ B, int64_t ldb,
                          int32_t K, double* As, double* Bs, fd4 (&acc)[2][2]) {
  const int t = threadIdx.x;
  for (int32_t k0 = 0; k0 < K; k0 += 16) {
    for (int e = t; e < 64 * 16; e += 256) {
      const int r = e >> 4, kk = e & 15;
      const bool in = (k0 + kk) < K;
      As[kk * 80 + r] = in ? A[(int64_t)r * lda + k0 + kk] : 0.0;
      Bs[kk * 80 + r] = in ? B[(int64_t)r * ldb + k0 + kk] : 0.0;
    }
    __syncthreads();
    tile64_step(As, Bs, acc);
    __syncthreads();
  }
}

// 64 x 64 tile  acc += A[k0 .. k1)[ia .. ia + 64)^T A[k0 .. k1)[ja .. ja + 64)
// of one row-major matrix A (leading dim ld; k0, k1 multiples of 16): the
// operands' k index is the row, so a staged line is 64 contiguous doubles
__device__ __forceinline__ void tile64_tn(const double* __restrict__ A, int64_t ld, int64_t ia, int64_t ja, int32_t k0,
                                          int32_t k1, double* As, double* Bs, fd4 (&acc)[2][2]) {
  const int t = threadIdx.x;
  for (int32_t kb = k0; kb < k1; kb += 16) {
    for (int e = t; e < 64 * 16; e += 256) {
      const int kk = e >> 6, r = e & 63;
      const double* row = A + (int64_t)(kb + kk) * ld;
      As[kk * 80 + r] = row[ia + r];
      Bs[kk * 80 + r] = row[ja + r];
    }
    __syncthreads();
    tile64_step(As, Bs, acc);
    __syncthreads();
  }
}

// acc element (i, j, r) -> tile row / column
__device__ __forceinline__ int tile_row(int i, int r) { return ((threadIdx.x >> 6) >> 1) * 32 + i * 16 + ((threadIdx.x & 63) >> 4) + 4 * r; }
__device__ __forceinline__ int tile_col(int j) { return ((threadIdx.x >> 6) & 1) * 32 + j * 16 + (threadIdx.x & 15); }

// lower-triangle tile number -> (i, j), j <= i
__device__ __forceinline__ void lower_tile(int32_t tid, int32_t& i, int32_t& j) {
  i = 0;
  while ((i + 1) * (i + 2) / 2 <= tid) ++i;
  j = tid - i * (i + 1) / 2;
}

__device__ __forceinline__ double readlane_f64(double v, int lane) {
  const uint64_t u = __builtin_bit_cast(uint64_t, v);
  const uint32_t lo = __builtin_amdgcn_readlane((uint32_t)u, lane);
  const uint32_t hi = __builtin_amdgcn_readlane((uint32_t)(u >> 32), lane);
  return __builtin_bit_cast(double, ((uint64_t)hi << 32) | lo);
}

// the diagonal block kb from a[] (thread t: row t & 63, columns 16 (t >> 6) ..
// + 15 of the updated block); col [2][NB], Ls [NB][NB + 1], invd [NB] in LDS.
// MERGED (ut_ctx::chol_merged): the substitution for inv(L_kk) runs inside the
// column loop instead of after it: at step c, row c of the solution is final
// (its accumulator took every earlier column's update), so each wave reads it
// from lane c and applies column c of L to the rows below, behind the same
// barrier as the factor's rank-1 update.  The same operations in the same
// order as the separate sweep (x_c = acc_c * (1 / piv_c), acc_r -= l_r x_c by
// fma, the rows' final scaling by 1 / piv_r), so the same bits, with 64 steps
// of latency fewer.
template <bool MERGED>
__device__ __forceinline__ void chol_diag_core(double (&a)[16], double* __restrict__ K, double* __restrict__ Li,
                                               int32_t npad, int32_t kb, int32_t* flag, double (*col)[NB],
                                               double* Ls, double* invd) {
  const int t = threadIdx.x, r = t & 63;
  const int g = __builtin_amdgcn_readfirstlane(t >> 6);
  const int64_t base = (int64_t)kb * NB;
  double* rowp = K + (base + r) * npad + base + 16 * g;
  if constexpr (MERGED) {
    double b[16];
#pragma unroll
    for (int j = 0; j < 16; ++j) b[j] = (16 * g + j == r) ? 1.0 : 0.0;
    for (int cb = 0; cb < NB / 16; ++cb) {
#pragma unroll
      for (int cc = 0; cc < 16; ++cc) {
        const int c = 16 * cb + cc;
        double* cl = col[c & 1];
        if (g == cb) {  // wave-uniform: the owner of column c
          const double dv = readlane_f64(a[cc], c);
          if (r == 0 && !(dv > 0.0)) atomicOr(flag, 1);
          const double piv = sqrt(dv > 0.0 ? dv : 1e-300);
          const double ip = 1.0 / piv;
          const double l = a[cc] * ip;
          cl[r] = r > c ? l : 0.0;
          if (r == 0) invd[c] = ip;
          a[cc] = r > c ? l : (r == c ? piv : a[cc]);
        }
        __syncthreads();  // column c published; the buffer written at step c+1 was last read at step c-1
        const double lr = cl[r];
        const double is = invd[c];
#pragma unroll
        for (int j = 0; j < 16; ++j) a[j] = __builtin_fma(-lr, cl[16 * g + j], a[j]);
#pragma unroll
        for (int j = 0; j < 16; ++j) b[j] = __builtin_fma(-lr, readlane_f64(b[j], c) * is, b[j]);
      }
    }
#pragma unroll
    for (int j = 0; j < 16; ++j) {
      const int sc = 16 * g + j;
      rowp[j] = sc <= r ? a[j] : 0.0;
    }
    const double ir = invd[r];   // written at step r, behind that step's barrier
    double* lip = Li + (base + r) * npad + base + 16 * g;
#pragma unroll
    for (int j = 0; j < 16; ++j) lip[j] = b[j] * ir;
    return;
  }
  for (int cb = 0; cb < NB / 16; ++cb) {
#pragma unroll
    for (int cc = 0; cc < 16; ++cc) {
      const int c = 16 * cb + cc;
      double* cl = col[c & 1];
      if (g == cb) {  // wave-uniform: the owner of column c
        const double dv = readlane_f64(a[cc], c);
        if (r == 0 && !(dv > 0.0)) atomicOr(flag, 1);
        const double piv = sqrt(dv > 0.0 ? dv : 1e-300);
        const double l = a[cc] * (1.0 / piv);
        cl[r] = r > c ? l : 0.0;
        a[cc] = r > c ? l : (r == c ? piv : a[cc]);
      }
      __syncthreads();  // column c published; the buffer written at step c+1 was last read at step c-1
      const double lr = cl[r];
#pragma unroll
      for (int j = 0; j < 16; ++j) a[j] = __builtin_fma(-lr, cl[16 * g + j], a[j]);
    }
  }
  // L to K (zeros above the diagonal) and to LDS for the substitution
#pragma unroll
  for (int j = 0; j < 16; ++j) {
    const int sc = 16 * g + j;
    const double v = sc <= r ? a[j] : 0.0;
    rowp[j] = v;
    Ls[r * (NB + 1) + sc] = v;
  }
  __syncthreads();
  if (t < NB) invd[t] = 1.0 / Ls[t * (NB + 1) + t];
  __syncthreads();
  // forward substitution L X = I, columns 16 g .. 16 g + 15 of X in b[]
  double b[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) b[j] = (16 * g + j == r) ? 1.0 : 0.0;
  for (int s2 = 0; s2 < NB; ++s2) {
    const double lrs = r > s2 ? Ls[r * (NB + 1) + s2] : 0.0;
    const double is = invd[s2];
#pragma unroll
    for (int j = 0; j < 16; ++j) b[j] = __builtin_fma(-lrs, readlane_f64(b[j], s2) * is, b[j]);
  }
  const double ir = invd[r];
  double* lip = Li + (base + r) * npad + base + 16 * g;
#pragma unroll
  for (int j = 0; j < 16; ++j) lip[j] = b[j] * ir;
}

}  // namespace ut
