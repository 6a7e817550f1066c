// gp_fit.hip -- Gaussian-process surrogate: the spec, and the fit.  (The
// batched posterior + acquisition: gp_score.hip; the pruned top-k: gp_prune.hip.)
//
// No reference arithmetic exists for this stage; the spec is
// SURVEY.md §8(a) row a7 / "GP spec for a7":
//   features u (unit encoding), us = u / ell (ARD), y standardised,
//   K = sf2 * exp(-0.5 |xs_i - xs_j|^2) + (sn2 + jitter) I,  L = chol(K),
//   alpha = K^-1 ys,  k* = sf2 * exp(-0.5 |us - xs_j|^2)  (via |a|^2+|b|^2-2ab),
//   mu = k*.alpha,  var = max(sf2 - |L^-1 k*|^2, 0),
//   EI = I Phi(I/sigma) + sigma phi(I/sigma), I = f_best - mu - xi  (max(I,0) if sigma == 0)
//   UCB score = kappa * sigma - mu
// The fp64 oracle is oracle/gp.py.
//
// Fit (per round, O(n^3), small): blocked right-looking Cholesky (NB = 64,
// panel factor + solve in LDS, trailing update tiles), blocked triangular
// inverse by block rows, two mat-vecs for alpha.
#include <cstring>
#include <thread>

#include "gp_tiles.h"
#include "ut_internal.h"

namespace ut {

// ---------------------------------------------------------------------------
// fit
// ---------------------------------------------------------------------------
// The fit's kernels are a chain of small, latency-bound launches on the fit
// stream, beside the round's hash / proposal / encode on the other streams.
// With g_fit_prio set (UT_FIT_SETPRIO) every fit wave raises its issue
// priority (s_setprio 3): where it shares a SIMD with the hash's waves, its
// instructions go first.
__device__ int32_t g_fit_prio = 0;
__device__ __forceinline__ void fit_prio() {
  if (g_fit_prio) __builtin_amdgcn_s_setprio(3);
}

int set_fit_prio(int32_t on) {
  if (hipMemcpyToSymbol(HIP_SYMBOL(g_fit_prio), &on, sizeof(on)) != hipSuccess) return UT_EHIP;
  return set_fit_prio_gemm(on);
}

__global__ void k_gp_prep_train(const double* __restrict__ X, int32_t n, int32_t npad, int32_t d,
                                const double* __restrict__ inv_ell, double* __restrict__ Xs,
                                double* __restrict__ xnorm) {
  fit_prio();
  const int32_t j = blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= npad) return;
  double s = 0.0;
  for (int32_t k = 0; k < d; ++k) {
    const double v = (j < n) ? X[(int64_t)j * d + k] * inv_ell[k] : 0.0;
    Xs[(int64_t)j * d + k] = v;
    s += v * v;
  }
  xnorm[j] = s;
}

// categorical K* operands of the training rows (gp_kstar_tile.h "Categorical K*"):
// XsT_num [dpad_num][npad] = the numeric features of Xs, transposed, and their
// norms in feature order; one thread per row
__global__ void k_gp_num_train(const double* __restrict__ Xs, int32_t npad, int32_t d,
                               const int32_t* __restrict__ num_feat, int32_t n_num, int32_t dpad_num,
                               double* __restrict__ XsT_num, double* __restrict__ xnorm_num) {
  fit_prio();
  const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= npad) return;
  double s = 0.0;
  for (int32_t k = 0; k < dpad_num; ++k) {
    const double v = k < n_num ? Xs[(int64_t)r * d + num_feat[k]] : 0.0;
    XsT_num[(int64_t)k * npad + r] = v * KSTAR_T_SCALE;   // the K* operand, in 2^(1/256) units (gp_gemm.hip)
    s += v * v;
  }
  xnorm_num[r] = s;
}

// the training rows' weighted one-hot codes [cat_k / 128][npad][128] (zeroed
// before): ENUM option o -> 2 at code column ccol + o, BOOL b -> 1 at ccol + b;
// X (unscaled features, rows < n) was checked one-hot on the host
__global__ void k_gp_cat_train(const DevParam* __restrict__ params, int32_t P, const int32_t* __restrict__ cat_ccol,
                               const double* __restrict__ X, int32_t n, int32_t d, int32_t npad,
                               int8_t* __restrict__ acat) {
  fit_prio();
  const int32_t r = blockIdx.x * blockDim.x + threadIdx.x;
  if (r >= n) return;
  for (int32_t p = 0; p < P; ++p) {
    const int32_t cc = cat_ccol[p];
    if (cc < 0) continue;
    const DevParam pr = params[p];
    const double* x = X + (int64_t)r * d + pr.feat_col;
    int32_t o = 0;
    if (pr.kind == UT_BOOL) {
      o = x[0] != 0.0 ? 1 : 0;
    } else {
      for (int32_t k = 0; k < (int32_t)pr.n_opt; ++k)
        if (x[k] == 1.0) { o = k; break; }
    }
    const int32_t q = cc + o;
    acat[((int64_t)(q >> 7) * npad + r) * 128 + (q & 127)] = (int8_t)(pr.kind == UT_BOOL ? 1 : 2);
  }
}

// mean / std (ddof=0) / standardise / f_best = min(ys); one workgroup
__global__ __launch_bounds__(256) void k_gp_ystats(const double* __restrict__ y, int32_t n, int32_t npad,
                                                   double* __restrict__ ys, double* __restrict__ stats) {
  fit_prio();
  __shared__ double red[256];
  const int t = threadIdx.x;
  double s = 0.0;
  for (int32_t i = t; i < n; i += 256) s += y[i];
  red[t] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  const double mean = red[0] / (double)n;
  __syncthreads();
  s = 0.0;
  for (int32_t i = t; i < n; i += 256) {
    const double dlt = y[i] - mean;
    s += dlt * dlt;
  }
  red[t] = s;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) red[t] += red[t + w];
    __syncthreads();
  }
  double sd = sqrt(red[0] / (double)n);
  if (!(sd > 0.0)) sd = 1.0;
  __syncthreads();
  double mn = 1.0 / 0.0;
  for (int32_t i = t; i < npad; i += 256) {
    const double v = (i < n) ? (y[i] - mean) / sd : 0.0;
    ys[i] = v;
    if (i < n) mn = v < mn ? v : mn;
  }
  red[t] = mn;
  __syncthreads();
  for (int w = 128; w > 0; w >>= 1) {
    if (t < w) red[t] = red[t + w] < red[t] ? red[t + w] : red[t];
    __syncthreads();
  }
  if (t == 0) {
    stats[0] = red[0];
    stats[1] = mean;
    stats[2] = sd;
  }
}

// the two staging kernels above on buffers other than the fit's (gp_lml.hip)
int launch_gp_prep_train(ut_ctx* c, const double* X, int32_t n, int32_t npad, int32_t d, const double* inv_ell,
                         double* Xs, double* xnorm) {
  hipLaunchKernelGGL(k_gp_prep_train, dim3(grid1(npad, 256)), dim3(256), 0, c->stream, X, n, npad, d, inv_ell, Xs,
                     xnorm);
  UT_LAUNCH_CHECK(c);
  return 0;
}

int launch_gp_ystats(ut_ctx* c, const double* y, int32_t n, int32_t npad, double* ys, double* stats) {
  hipLaunchKernelGGL(k_gp_ystats, dim3(1), dim3(256), 0, c->stream, y, n, npad, ys, stats);
  UT_LAUNCH_CHECK(c);
  return 0;
}

// the categorical K*'s training-side operands (numeric block, its norms, the
// weighted one-hot codes) of npad scaled rows Xs whose first n raw rows are X:
// the fit's own rows, and the failed rows of the feasibility vote (gp_feas.hip)
int launch_gp_cat_train(ut_ctx* c, const double* Xs, const double* X, int32_t n, int32_t npad, int32_t d, int32_t dpn,
                        double* XsT_num, double* xnorm_num, int8_t* acat) {
  const Space& sp = c->space;
  hipLaunchKernelGGL(k_gp_num_train, dim3(grid1(npad, 256)), dim3(256), 0, c->stream, Xs, npad, d, sp.d_num_feat.p,
                     sp.n_num, dpn, XsT_num, xnorm_num);
  UT_HIP(c, hipMemsetAsync(acat, 0, (size_t)sp.cat_k * npad, c->stream));
  hipLaunchKernelGGL(k_gp_cat_train, dim3(grid1(n, 256)), dim3(256), 0, c->stream, sp.d_params.p, sp.P, sp.d_cat_ccol.p,
                     X, n, d, npad, acat);
  UT_LAUNCH_CHECK(c);
  return 0;
}

// (tile64_nt, tile_row / tile_col, readlane_f64 and chol_diag_core: gp_tiles.h)
//
// Panel kb, step 1 (one workgroup): L_kk = chol(A_kk) written to K, and
// inv(L_kk) written as the diagonal block of L^-1.
//
// This is the serial spine of the fit (NB column steps, then NB substitution
// steps, per diagonal block), so every step is kept short.  Thread t owns row
// r = t & 63 and columns 16 g .. 16 g + 15 of the block (g = wave) in
// registers.  Cholesky step c: the wave that owns column c takes the pivot by
// readlane, scales its column and publishes l = L[:, c] (0 above the
// diagonal) in a double-buffered LDS column; after ONE barrier every wave
// applies the rank-1 update a[j] -= l_r l_s to its 16 columns.  Entries above
// the diagonal are updated as well but never read.  The inverse solves
// L X = I for all 64 columns at once, each wave its 16 columns with no
// barrier: step s broadcasts row s of the partial solution by readlane.
// (The previous LDS version took 122 us per block at n = 1024, 70% of the fit.)
template <bool MERGED>
__global__ __launch_bounds__(256) void k_chol_diag(double* __restrict__ K, double* __restrict__ Li, int32_t npad,
                                                   int32_t kb, int32_t* flag) {
  fit_prio();
  __shared__ double col[2][NB];
  __shared__ double Ls[NB * (NB + 1)];
  __shared__ double invd[NB];
  const int t = threadIdx.x, r = t & 63;
  const int g = __builtin_amdgcn_readfirstlane(t >> 6);
  const int64_t base = (int64_t)kb * NB;
  const double* rowp = K + (base + r) * npad + base + 16 * g;
  double a[16];
#pragma unroll
  for (int j = 0; j < 16; ++j) a[j] = rowp[j];
  chol_diag_core<MERGED>(a, K, Li, npad, kb, flag, col, Ls, invd);
}

// Panel kb, step 2: row block i > kb:  L_ik = A_ik * inv(L_kk)^T  (NT product)
__global__ __launch_bounds__(256) void k_chol_rows(double* __restrict__ K, const double* __restrict__ Li,
                                                   int32_t npad, int32_t kb) {
  fit_prio();
  __shared__ double As[16 * 80];
  __shared__ double Bs[16 * 80];
  const int64_t base = (int64_t)kb * NB, rb = (int64_t)(kb + 1 + blockIdx.x) * NB;
  fd4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (fd4){0.0, 0.0, 0.0, 0.0};
  tile64_nt(K + rb * npad + base, npad, Li + base * npad + base, npad, NB, As, Bs, acc);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) K[(rb + tile_row(i, r)) * npad + base + tile_col(j)] = acc[i][j][r];
}

// Trailing update A_ij -= L_i,kb L_j,kb^T for kb < j <= i < nb.
__global__ __launch_bounds__(256) void k_chol_update(double* __restrict__ K, int32_t npad, int32_t kb) {
  fit_prio();
  __shared__ double As[16 * 80];
  __shared__ double Bs[16 * 80];
  int32_t tid = blockIdx.x;
  int32_t i = 0;
  while ((i + 1) * (i + 2) / 2 <= tid) ++i;
  const int32_t j = tid - i * (i + 1) / 2;
  const int64_t ib = (int64_t)(kb + 1 + i) * NB, jb = (int64_t)(kb + 1 + j) * NB, cb = (int64_t)kb * NB;
  fd4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = (fd4){0.0, 0.0, 0.0, 0.0};
  tile64_nt(K + ib * npad + cb, npad, K + jb * npad + cb, npad, NB, As, Bs, acc);
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) K[(ib + tile_row(a, r)) * npad + jb + tile_col(b)] -= acc[a][b][r];
}

// k_chol_update with the next panel's diagonal block factored in the same
// launch: the workgroup that updates block (kb + 1, kb + 1) keeps it in LDS
// and runs k_chol_diag's steps on it while the others update the rest, so the
// fit's serial chain loses one launch per level (ut_ctx::chol_fuse)
template <bool MERGED>
__global__ __launch_bounds__(256) void k_chol_update_diag(double* __restrict__ K, double* __restrict__ Li,
                                                          int32_t npad, int32_t kb, int32_t* flag) {
  fit_prio();
  // As / Bs of the tile product, then (workgroup 0) Ls, col, invd of the diagonal block
  __shared__ double sm[NB * (NB + 1) + 2 * NB + NB];
  double* As = sm;
  double* Bs = sm + 16 * 80;
  const int32_t tid = blockIdx.x;
  int32_t i = 0;
  while ((i + 1) * (i + 2) / 2 <= tid) ++i;
  const int32_t j = tid - i * (i + 1) / 2;
  const int64_t ib = (int64_t)(kb + 1 + i) * NB, jb = (int64_t)(kb + 1 + j) * NB, cb = (int64_t)kb * NB;
  fd4 acc[2][2];
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b) acc[a][b] = (fd4){0.0, 0.0, 0.0, 0.0};
  tile64_nt(K + ib * npad + cb, npad, K + jb * npad + cb, npad, NB, As, Bs, acc);
  if (tid != 0) {
#pragma unroll
    for (int a = 0; a < 2; ++a)
#pragma unroll
      for (int b = 0; b < 2; ++b)
#pragma unroll
        for (int r = 0; r < 4; ++r) K[(ib + tile_row(a, r)) * npad + jb + tile_col(b)] -= acc[a][b][r];
    return;
  }
  // block (kb + 1, kb + 1): the updated values (the same arithmetic as the
  // store above) into LDS, then the diagonal steps on them
  double* Ls = sm;
  double(*col)[NB] = reinterpret_cast<double(*)[NB]>(sm + NB * (NB + 1));
  double* invd = sm + NB * (NB + 1) + 2 * NB;
#pragma unroll
  for (int a = 0; a < 2; ++a)
#pragma unroll
    for (int b = 0; b < 2; ++b)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int tr = tile_row(a, r), tc = tile_col(b);
        Ls[tr * (NB + 1) + tc] = K[(ib + tr) * npad + jb + tc] - acc[a][b][r];
      }
  __syncthreads();
  const int t = threadIdx.x, rr = t & 63, g = t >> 6;
  double av[16];
#pragma unroll
  for (int q = 0; q < 16; ++q) av[q] = Ls[rr * (NB + 1) + 16 * g + q];
  __syncthreads();   // Ls is rewritten by the substitution's setup
  chol_diag_core<MERGED>(av, K, Li, npad, kb + 1, flag, col, Ls, invd);
}

// K = sf2 exp(-0.5 |xs_i - xs_j|^2) + diag I, 64 x 64 tiles on fp64 MFMA;
// padded rows/columns (>= n) form an identity block; block rows from rb0 on
__global__ __launch_bounds__(256) void k_gp_kmat(const double* __restrict__ Xs, const double* __restrict__ xnorm,
                                                 int32_t n, int32_t npad, int32_t d, double sf2, double diag,
                                                 double* __restrict__ K, int32_t rb0) {
  fit_prio();
  __shared__ double As[16 * 80];
  __shared__ double Bs[16 * 80];
  const int64_t ib = (int64_t)(blockIdx.y + rb0) * 64, jb = (int64_t)blockIdx.x * 64;
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
        double v;
        if (i >= n || j >= n) {
          v = (i == j) ? 1.0 : 0.0;
        } else {
          double d2 = xnorm[i] + xnorm[j] - 2.0 * acc[a][b][r];
          d2 = d2 > 0.0 ? d2 : 0.0;
          v = sf2 * exp(-0.5 * d2);
          if (i == j) v += diag;
        }
        K[i * npad + j] = v;
      }
}

// Batched fp64 GEMM for the recursive triangular inverse.  Pair z at level
// size s (offset o = z * 2s):
//   phase 0:  T_z = B * Ai     B = L[o+s:o+2s, o:o+s],  Ai = Li[o:o+s, o:o+s]  (lower)
//   phase 1:  Li[o+s:o+2s, o:o+s] = -Ci * T_z            Ci = Li[o+s:o+2s, o+s:o+2s]  (lower)
// 64 x 64 output tile per 256-thread workgroup, v_mfma_f64_16x16x4 (each
// wave 32 x 32 = 2 x 2 MFMA tiles), K step 16; the triangular operand limits
// the K range of each tile.
__global__ __launch_bounds__(256) void k_trinv_level(const double* __restrict__ L, double* __restrict__ Li,
                                                     double* __restrict__ T, int32_t npad, int32_t s, int32_t phase) {
  fit_prio();
  __shared__ double As[16 * 80];
  __shared__ double Bs[16 * 80];
  const int32_t z = blockIdx.z;
  const int64_t o = (int64_t)z * 2 * s;
  const int32_t s2 = (int32_t)min((int64_t)s, (int64_t)npad - o - s);  // ragged last pair (multiple of 64)
  const int32_t tr = blockIdx.y * 64, tc = blockIdx.x * 64;  // output tile inside the s2 x s block
  if (s2 <= 0 || tr >= s2) return;
  const double* A;
  const double* B;
  int64_t lda, ldb;
  int32_t k_lo, k_hi;
  double* C;
  int64_t ldc;
  double sign;
  if (phase == 0) {
    A = L + (o + s) * npad + o; lda = npad;                       // B (dense)
    B = Li + o * npad + o; ldb = npad;                            // Ai (lower): rows k >= tc contribute
    k_lo = tc; k_hi = s;
    C = T + (int64_t)z * s * s; ldc = s; sign = 1.0;
  } else {
    A = Li + (o + s) * npad + (o + s); lda = npad;                // Ci (lower): k <= tr + 63
    B = T + (int64_t)z * s * s; ldb = s;
    k_lo = 0; k_hi = min(tr + 64, s2);
    C = Li + (o + s) * npad + o; ldc = npad; sign = -1.0;
  }
  typedef double d4 __attribute__((ext_vector_type(4)));
  const int t = threadIdx.x, lane = t & 63, w = t >> 6;
  const int wr = w >> 1, wc = w & 1;
  d4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (d4){0.0, 0.0, 0.0, 0.0};
  for (int32_t k0 = k_lo; k0 < k_hi; k0 += 16) {
    // A tile 64 x 16 -> As[k][row]; B tile 16 x 64 -> Bs[k][col]
    for (int e = t; e < 64 * 16; e += 256) {
      const int r = e >> 4, kk = e & 15;
      As[kk * 80 + r] = A[(int64_t)(tr + r) * lda + k0 + kk];
      const int kb = e >> 6, c = e & 63;
      Bs[kb * 80 + c] = B[(int64_t)(k0 + kb) * ldb + tc + c];
    }
    __syncthreads();
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
    __syncthreads();
  }
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = tr + wr * 32 + i * 16 + (lane >> 4) + 4 * r;
        const int col = tc + wc * 32 + j * 16 + (lane & 15);
        C[(int64_t)row * ldc + col] = sign * acc[i][j][r];
      }
}

// The same two products for levels s >= TRB_MIN, where k_trinv_level's 64 x 64
// tiles and plain loads dominate the fit (at n = 4096 the top level is 75 % of
// the inverse's 23 GFLOP).  128 x 128 output tile per 256-thread workgroup
// (2 x 2 waves of 64 x 64, 4 x 4 v_mfma_f64_16x16x4 sub-tiles each), 16-k
// stages through a 2-deep global_load_lds ring (k_gp_var_pp's pipeline), two
// workgroups per CU.
//   right operand, [k][col] row-major (Ai, T): one 1-KiB wave-instruction per k row;
//   left operand, [row][k] row-major (the L block, Ci): one wave-instruction
//   moves 8 rows x 16 k; lane l fetches 16-B chunk (l & 7) ^ ((row >> 1) & 7)
//   of its row, so an MFMA fragment read (16 rows at one k) hits 16 distinct
//   bank pairs.
// k runs upward in MFMA groups of 4 from a multiple of 64, as in k_trinv_level;
// the extra products a 128-wide tile takes on are exact zeros of the
// triangular operand, so the two kernels give the same bits.
constexpr int TRB_MIN = 256, TRB_BM = 128, TRB_BK = 16, TRB_SL = TRB_BM * TRB_BK;

__global__ __launch_bounds__(256, 2) void k_trinv_big(const double* __restrict__ L, double* __restrict__ Li,
                                                      double* __restrict__ T, int32_t npad, int32_t s, int32_t phase) {
  fit_prio();
  // one __shared__ object (see k_gp_var): [stage][left | right]
  __shared__ __attribute__((aligned(16))) double lds[2 * 2 * TRB_SL];
  const int32_t z = blockIdx.z;
  const int64_t o = (int64_t)z * 2 * s;
  const int32_t s2 = (int32_t)min((int64_t)s, (int64_t)npad - o - s);  // multiple of 128 (npad % NPAD == 0)
  const int32_t tr = blockIdx.y * TRB_BM, tc = blockIdx.x * TRB_BM;
  if (s2 <= 0 || tr >= s2) return;
  const double* A;
  const double* B;
  int64_t lda, ldb, ldc;
  int32_t k_lo, k_hi;
  double* C;
  double sign;
  if (phase == 0) {
    A = L + (o + s) * npad + o; lda = npad;
    B = Li + o * npad + o; ldb = npad;
    k_lo = tc; k_hi = s;
    C = T + (int64_t)z * s * s; ldc = s; sign = 1.0;
  } else {
    A = Li + (o + s) * npad + (o + s); lda = npad;
    B = T + (int64_t)z * s * s; ldb = s;
    k_lo = 0; k_hi = min(tr + TRB_BM, s2);
    C = Li + (o + s) * npad + o; ldc = npad; sign = -1.0;
  }
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = w >> 1, wn = w & 1;
  auto issue = [&](int32_t k0, double* st) {
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = 4 * w + u;
      const int row = 8 * q + (lane >> 3);
      const int ch = (lane & 7) ^ ((row >> 1) & 7);
      __builtin_amdgcn_global_load_lds(A + (int64_t)(tr + row) * lda + k0 + 2 * ch,
                                       (__attribute__((address_space(3))) void*)(st + q * 128), 16, 0, 0);
    }
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const int q = 4 * w + u;
      __builtin_amdgcn_global_load_lds(B + (int64_t)(k0 + q) * ldb + tc + lane * 2,
                                       (__attribute__((address_space(3))) void*)(st + TRB_SL + q * 128), 16, 0, 0);
    }
  };
  typedef double d4 __attribute__((ext_vector_type(4)));
  d4 acc[4][4];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j) acc[i][j] = (d4){0.0, 0.0, 0.0, 0.0};
  const int32_t nk = (k_hi - k_lo) / TRB_BK;
  issue(k_lo, lds);
  for (int32_t kt = 0; kt < nk; ++kt) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // stage kt landed everywhere; stage kt-1 fully read
    asm volatile("" ::: "memory");
    if (kt + 1 < nk) issue(k_lo + (kt + 1) * TRB_BK, lds + ((kt + 1) & 1) * 2 * TRB_SL);
    const double* as = lds + (kt & 1) * 2 * TRB_SL;
    const double* bs = as + TRB_SL;
#pragma unroll
    for (int ks = 0; ks < TRB_BK / 4; ++ks) {
      const int kr = ks * 4 + (lane >> 4);
      double af[4], bf[4];
#pragma unroll
      for (int j = 0; j < 4; ++j) bf[j] = bs[kr * TRB_BM + wn * 64 + j * 16 + (lane & 15)];
#pragma unroll
      for (int i = 0; i < 4; ++i) {
        const int row = wm * 64 + i * 16 + (lane & 15);
        af[i] = as[row * TRB_BK + 2 * ((kr >> 1) ^ ((row >> 1) & 7)) + (kr & 1)];
      }
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) acc[i][j] = __builtin_amdgcn_mfma_f64_16x16x4f64(af[i], bf[j], acc[i][j], 0, 0, 0);
    }
  }
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int j = 0; j < 4; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int row = tr + wm * 64 + i * 16 + (lane >> 4) + 4 * r;
        const int col = tc + wn * 64 + j * 16 + (lane & 15);
        C[(int64_t)row * ldc + col] = sign * acc[i][j][r];
      }
}

// out = Linv * v  (one wave per row)
__global__ __launch_bounds__(256) void k_lower_mv(const double* __restrict__ Li, int32_t npad,
                                                  const double* __restrict__ v, double* __restrict__ out) {
  fit_prio();
  const int32_t r = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= npad) return;
  double s = 0.0;
  for (int32_t c = lane; c <= r; c += 64) s += Li[(int64_t)r * npad + c] * v[c];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if (lane == 0) out[r] = s;
}

// out = Linv^T * v, read through LinvT (row c of LinvT = column c of L^-1,
// nonzero from c on): one wave per row, coalesced (the column-strided read of
// L^-1 ran on npad / 64 workgroups at ~250 GB/s)
__global__ __launch_bounds__(256) void k_upper_mv(const double* __restrict__ LiT, int32_t npad,
                                                  const double* __restrict__ v, double* __restrict__ out) {
  fit_prio();
  const int32_t r = blockIdx.x * 4 + (threadIdx.x >> 6);
  const int lane = threadIdx.x & 63;
  if (r >= npad) return;
  double s = 0.0;
  for (int32_t c = r + lane; c < npad; c += 64) s += LiT[(int64_t)r * npad + c] * v[c];
  for (int off = 32; off > 0; off >>= 1) s += __shfl_xor(s, off);
  if (lane == 0) out[r] = s;
}

// ---------------------------------------------------------------------------
// incremental fit: append block row b (64 rows) to an existing factor
// ---------------------------------------------------------------------------
// With the old factor L (rows < 64 b) and its inverse L^-1, the new rows'
// kernel block [K21 K22] extends it as
//   [[L, 0], [B, D]],  B = K21 L^-T,  D = chol(K22 - B B^T)
// and the inverse as
//   [[L^-1, 0], [-D^-1 B L^-1, D^-1]].
// A few small launches per block (O(n^2) work against the O(n^3) refit); the
// scratch T holds B [64][npad] at offset 0 and E = B L^-1, transposed
// ([npad][64]), at offset 64 npad.  Padded rows (>= n) are identity rows of
// K, so they stay identity rows of L^-1.

// The three products of block b, split over K in APP_KC chunks (one
// workgroup per tile x chunk, so a few hundred workgroups instead of b long
// serial K loops) and summed in chunk order by k_app_red (deterministic):
//   MODE 0  B[j][c]     = sum_c' K21[j][c'] L^-1[c][c']   tile cb < b, c' < 64 cb + 64
//   MODE 1  (B B^T)[j][j'] = sum_c' B[j][c'] B[j'][c']     one tile,   c' < 64 b
//   MODE 2  E^T[c][j]   = sum_c' B[j][c'] L^-1[c'][c]     tile cb < b, 64 cb <= c' < 64 b
//           (L^-1 read through LinvT, whose rows are its columns)
constexpr int APP_KC = 256;

struct AppGemm {
  const double* A;
  const double* B;
  int32_t klo, khi;
};

template <int MODE>
__device__ __forceinline__ AppGemm app_gemm(const double* Li, const double* LinvT, const double* K,
                                            const double* T, int32_t npad, int32_t b, int64_t t) {
  if (MODE == 0) return {Li + t * 64 * npad, K + (int64_t)b * 64 * npad, 0, (int32_t)(t * 64 + 64)};
  if (MODE == 1) return {T, T, 0, b * 64};
  return {T, LinvT + t * 64 * npad, (int32_t)(t * 64), b * 64};
}

template <int MODE>
__global__ __launch_bounds__(256) void k_app_part(const double* __restrict__ Li, const double* __restrict__ LinvT,
                                                  const double* __restrict__ K, const double* __restrict__ T,
                                                  int32_t npad, int32_t b, int32_t maxq, double* __restrict__ W) {
  fit_prio();
  __shared__ double As[16 * 80];
  __shared__ double Bs[16 * 80];
  const int64_t q = blockIdx.x, t = blockIdx.y;
  const AppGemm g = app_gemm<MODE>(Li, LinvT, K, T, npad, b, t);
  const int32_t k0 = g.klo + (int32_t)q * APP_KC;
  if (k0 >= g.khi) return;
  fd4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (fd4){0.0, 0.0, 0.0, 0.0};
  tile64_nt(g.A + k0, npad, g.B + k0, npad, min(APP_KC, g.khi - k0), As, Bs, acc);
  double* w = W + (t * maxq + q) * 4096;
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) w[tile_row(i, r) * 64 + tile_col(j)] = acc[i][j][r];
}

// MODE 0 -> B into T [64][npad];  MODE 1 -> K22 -= B B^T (in place; k_chol_diag
// factors it next);  MODE 2 -> E^T into Et [npad][64]
template <int MODE>
__global__ __launch_bounds__(256) void k_app_red(const double* __restrict__ Li, const double* __restrict__ LinvT,
                                                 double* __restrict__ K, double* __restrict__ T, int32_t npad,
                                                 int32_t b, int32_t maxq, const double* __restrict__ W,
                                                 double* __restrict__ Et) {
  fit_prio();
  const int64_t t = blockIdx.x, base = (int64_t)b * 64;
  const AppGemm g = app_gemm<MODE>(Li, LinvT, K, T, npad, b, t);
  const int32_t nq = (g.khi - g.klo + APP_KC - 1) / APP_KC;
  const double* w = W + t * maxq * 4096;
  for (int e = threadIdx.x; e < 4096; e += 256) {
    double s = 0.0;
    for (int32_t q = 0; q < nq; ++q) s += w[(int64_t)q * 4096 + e];
    const int i = e >> 6, j = e & 63;
    if (MODE == 0) T[(int64_t)j * npad + t * 64 + i] = s;
    else if (MODE == 1) K[(base + i) * npad + base + j] -= s;
    else Et[(t * 64 + j) * 64 + i] = s;
  }
}

// new L^-1 rows: C = -D^-1 E for column blocks cb < b (written to L^-1 and
// LinvT); workgroup cb == b copies D^-1 (k_chol_diag's output) into LinvT
__global__ __launch_bounds__(256) void k_app_c(double* __restrict__ Li, double* __restrict__ LinvT,
                                               const double* __restrict__ Et, int32_t npad, int32_t b) {
  fit_prio();
  __shared__ double As[16 * 80];
  __shared__ double Bs[16 * 80];
  const int64_t cb = blockIdx.x, base = (int64_t)b * 64;
  if (cb == b) {
    for (int e = threadIdx.x; e < 64 * 64; e += 256) {
      const int j = e >> 6, cc = e & 63;
      LinvT[(base + cc) * npad + base + j] = Li[(base + j) * npad + base + cc];
    }
    return;
  }
  fd4 acc[2][2];
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j) acc[i][j] = (fd4){0.0, 0.0, 0.0, 0.0};
  tile64_nt(Li + base * npad + base, npad, Et + cb * 64 * 64, 64, 64, As, Bs, acc);
#pragma unroll
  for (int i = 0; i < 2; ++i)
#pragma unroll
    for (int j = 0; j < 2; ++j)
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int64_t row = base + tile_row(i, r), col = cb * 64 + tile_col(j);
        const double v = -acc[i][j][r];
        Li[row * npad + col] = v;
        LinvT[col * npad + row] = v;
      }
}

// ---------------------------------------------------------------------------
// host side
// ---------------------------------------------------------------------------
static void launch_chol_diag(ut_ctx* c, int32_t npad, int32_t kb) {
  hipLaunchKernelGGL(c->chol_merged ? k_chol_diag<true> : k_chol_diag<false>, dim3(1), dim3(256), 0, c->stream,
                     c->gp_K.p, c->gp_Linv.p, npad, kb, c->gp_flag.p);
}

static int gp_alloc(ut_ctx* c, int32_t npad_need, int32_t d) {
  if (c->gp_cap_n >= npad_need && c->gp_d == d) return 0;
  // room for a growing training set (the tuning loop adds a few rows per fit):
  // a new padded size then reuses the buffers instead of freeing and
  // allocating ~5 n^2 doubles behind a device-wide sync (2.5-10 ms per 128
  // rows in the C5 loop).  Every kernel indexes with the fit's own npad.
  const size_t npad = (size_t)gp_npad(npad_need + npad_need / 4);
  UT_HIP(c, ut::sync_all(c));   // earlier rounds may still read the buffers replaced here
  // no capacity until every buffer exists: after a failure part-way the next
  // call allocates them all again
  c->gp_cap_n = 0;
  UT_HIP(c, c->gp_Xs.alloc(npad * d));
  UT_HIP(c, c->gp_xnorm.alloc(npad));
  UT_HIP(c, c->gp_K.alloc(npad * npad));
  UT_HIP(c, c->gp_Linv.alloc(npad * npad));
  UT_HIP(c, c->gp_y.alloc(npad));
  UT_HIP(c, c->gp_tmp.alloc(npad * (d + 1)));
  UT_HIP(c, c->gp_alpha.alloc(npad));
  UT_HIP(c, c->gp_beta.alloc(npad));
  UT_HIP(c, c->gp_inv_ell.alloc(d));
  UT_HIP(c, c->gp_stats.alloc(4));
  UT_HIP(c, c->gp_flag.alloc(1));
  UT_HIP(c, c->gp_T.alloc(npad * npad));
  UT_HIP(c, c->gp_Xs_f.alloc(npad * d));
  UT_HIP(c, c->gp_LinvT.alloc(npad * npad));
  // fp32: (L^-1)^T; h3: the blocked fp16 hi / lo planes, rows padded to 256
  UT_HIP(c, c->gp_LinvT_f.alloc((((npad + 255) / 256) * 256) * npad));
  UT_HIP(c, c->gp_ctr.alloc(32));
  UT_HIP(c, c->gp_XsT.alloc(npad * kstar_dpad(d)));
  c->gp_cap_n = (int64_t)npad;
  c->gp_d = d;
  return 0;
}

// rows [r0, r1) of X [n][d] have exact one-hot ENUM blocks and 0 / 1 BOOL
// features: the categorical K* reads the training rows as option codes
bool cat_rows_ok(const Space& s, const double* X, int32_t d, int32_t r0, int32_t r1) {
  for (int32_t r = r0; r < r1; ++r) {
    const double* row = X + (size_t)r * d;
    for (int32_t p : s.host_cat) {
      const DevParam& q = s.host_params[p];
      const double* x = row + q.feat_col;
      if (q.kind == UT_BOOL) {
        if (!(x[0] == 0.0 || x[0] == 1.0)) return false;
        continue;
      }
      int32_t ones = 0;
      for (int32_t k = 0; k < (int32_t)q.n_opt; ++k) {
        if (x[k] == 1.0) ++ones;
        else if (x[k] != 0.0) return false;
      }
      if (ones != 1) return false;
    }
  }
  return true;
}

// The fit's device work on c->stream (the fit stream), in two parts split at
// ev_fit_x: part 0 the staging copies from the pinned host buffer and the
// scaled inputs; part 1 the factor and L^-1 (a refit, or block rows appended
// to the previous factor), beta / alpha, and the scoring precision's
// operands.  Enqueues only: every buffer is allocated by the caller.
static int fit_device(ut_ctx* c, int part, int32_t n, int32_t n0, int32_t d, int32_t npad, int32_t dpn, bool app,
                      int32_t xr0, double diag, double sf2) {
  int rc;
  double* hX = c->fit_host;
  double* hy = hX + (size_t)n * d;
  double* hinv = hy + n;
  double* dX = c->gp_tmp.p;           // [n][d] staging (gp_tmp holds npad*(d+1))
  double* dy = c->gp_tmp.p + (int64_t)npad * d;
  if (part == 0) {
    UT_HIP(c, hipMemcpyAsync(c->gp_inv_ell.p, hinv, sizeof(double) * d, hipMemcpyHostToDevice, c->stream));
    UT_HIP(c, hipMemcpyAsync(dX + (size_t)xr0 * d, hX + (size_t)xr0 * d, sizeof(double) * (size_t)(n - xr0) * d,
                             hipMemcpyHostToDevice, c->stream));
    UT_HIP(c, hipMemcpyAsync(dy, hy, sizeof(double) * n, hipMemcpyHostToDevice, c->stream));
    if (!app) UT_HIP(c, hipMemsetAsync(c->gp_flag.p, 0, sizeof(int32_t), c->stream));
    hipLaunchKernelGGL(k_gp_prep_train, dim3(grid1(npad, 256)), dim3(256), 0, c->stream, dX, n, npad, d,
                       c->gp_inv_ell.p, c->gp_Xs.p, c->gp_xnorm.p);
    // the candidate side of K* needs only the scaled inputs: fp64 scoring starts
    // its K* here while the factorisation below is still running
    if ((rc = launch_xs_t(c, c->gp_Xs.p, npad, d, kstar_dpad(d), c->gp_XsT.p))) return rc;
    if (c->cat_on && (rc = launch_gp_cat_train(c, c->gp_Xs.p, dX, n, npad, d, dpn, c->gp_XsT_num.p, c->gp_xnorm_num.p,
                                               c->gp_acat.p)))
      return rc;
    // precision 8: K*'s training operand as int8 digit planes (gp_kq.hip;
    // numeric fits only, gp_score_impl)
    if (c->gp_prec == 8 && c->kstar_q && !c->cat_on &&
        (rc = launch_split_x8(c, c->gp_XsT.p, kstar_dpad(d), npad)))
      return rc;
    return 0;
  }
  if (app) {
    // (the previous precision-8 refit left (L^-1)^T to its readers)
    if ((rc = gp_ensure_linvt(c))) return rc;
    // block rows b0 .. b1 hold the new rows (b0 may also hold old ones: it is
    // recomputed whole)
    const int32_t b0 = n0 / NB, b1 = (n - 1) / NB;
    hipLaunchKernelGGL(k_gp_kmat, dim3(b1 + 1, b1 - b0 + 1), dim3(256), 0, c->stream, c->gp_Xs.p, c->gp_xnorm.p, n,
                       npad, d, sf2, diag, c->gp_K.p, b0);
    hipLaunchKernelGGL(k_gp_ystats, dim3(1), dim3(256), 0, c->stream, dy, n, npad, c->gp_y.p, c->gp_stats.p);
    double* Et = c->gp_T.p + (int64_t)NB * npad;
    for (int32_t b = b0; b <= b1; ++b) {
      const int32_t maxq = (b * NB + APP_KC - 1) / APP_KC;
      if (b > 0) {
        double* W = c->app_ws.p;
        hipLaunchKernelGGL(k_app_part<0>, dim3(maxq, b), dim3(256), 0, c->stream, c->gp_Linv.p, c->gp_LinvT.p,
                           c->gp_K.p, c->gp_T.p, npad, b, maxq, W);
        hipLaunchKernelGGL(k_app_red<0>, dim3(b), dim3(256), 0, c->stream, c->gp_Linv.p, c->gp_LinvT.p, c->gp_K.p,
                           c->gp_T.p, npad, b, maxq, W, Et);
        hipLaunchKernelGGL(k_app_part<1>, dim3(maxq, 1), dim3(256), 0, c->stream, c->gp_Linv.p, c->gp_LinvT.p,
                           c->gp_K.p, c->gp_T.p, npad, b, maxq, W);
        hipLaunchKernelGGL(k_app_red<1>, dim3(1), dim3(256), 0, c->stream, c->gp_Linv.p, c->gp_LinvT.p, c->gp_K.p,
                           c->gp_T.p, npad, b, maxq, W, Et);
      }
      launch_chol_diag(c, npad, b);
      if (b > 0) {
        double* W = c->app_ws.p;
        hipLaunchKernelGGL(k_app_part<2>, dim3(maxq, b), dim3(256), 0, c->stream, c->gp_Linv.p, c->gp_LinvT.p,
                           c->gp_K.p, c->gp_T.p, npad, b, maxq, W);
        hipLaunchKernelGGL(k_app_red<2>, dim3(b), dim3(256), 0, c->stream, c->gp_Linv.p, c->gp_LinvT.p, c->gp_K.p,
                           c->gp_T.p, npad, b, maxq, W, Et);
      }
      hipLaunchKernelGGL(k_app_c, dim3(b + 1), dim3(256), 0, c->stream, c->gp_Linv.p, c->gp_LinvT.p, Et, npad, b);
    }
    UT_LAUNCH_CHECK(c);
  } else {
    hipLaunchKernelGGL(k_gp_kmat, dim3(npad / 64, npad / 64), dim3(256), 0, c->stream, c->gp_Xs.p,
                       c->gp_xnorm.p, n, npad, d, sf2, diag, c->gp_K.p, 0);
    hipLaunchKernelGGL(k_gp_ystats, dim3(1), dim3(256), 0, c->stream, dy, n, npad, c->gp_y.p, c->gp_stats.p);
    UT_LAUNCH_CHECK(c);
    const int32_t nb = npad / NB;
    UT_HIP(c, hipMemsetAsync(c->gp_Linv.p, 0, sizeof(double) * npad * npad, c->stream));
    const bool fuse = c->chol_fuse > 0 || (c->chol_fuse < 0 && npad >= 2048);
    for (int32_t kb = 0; kb < nb; ++kb) {
      // (fused: diagonal blocks after the first come from the previous update)
      if (!fuse || kb == 0)
        launch_chol_diag(c, npad, kb);
      const int32_t T = nb - kb - 1;
      if (T > 0) {
        hipLaunchKernelGGL(k_chol_rows, dim3(T), dim3(256), 0, c->stream, c->gp_K.p, c->gp_Linv.p, npad, kb);
        if (fuse)
          hipLaunchKernelGGL(c->chol_merged ? k_chol_update_diag<true> : k_chol_update_diag<false>,
                             dim3(T * (T + 1) / 2), dim3(256), 0, c->stream, c->gp_K.p, c->gp_Linv.p, npad, kb, c->gp_flag.p);
        else
          hipLaunchKernelGGL(k_chol_update, dim3(T * (T + 1) / 2), dim3(256), 0, c->stream, c->gp_K.p, npad, kb);
      }
    }
    UT_LAUNCH_CHECK(c);
    // off-diagonal blocks of L^-1 by recursive doubling (diagonal blocks came from k_chol_diag)
    for (int32_t lv = NB; lv < npad; lv *= 2) {
      const int32_t pairs = (int32_t)((npad - lv + 2 * lv - 1) / (2 * lv));
      if (c->trinv_big && lv >= TRB_MIN) {
        // k_trinv_big's tiles: every pair's sizes are multiples of 128
        UT_CHECK(c, npad % TRB_BM == 0 && lv % TRB_BM == 0, UT_EINVAL, "gp_fit: npad not a multiple of 128");
        const dim3 gb(lv / TRB_BM, lv / TRB_BM, pairs);
        hipLaunchKernelGGL(k_trinv_big, gb, dim3(256), 0, c->stream, c->gp_K.p, c->gp_Linv.p, c->gp_T.p, npad, lv, 0);
        hipLaunchKernelGGL(k_trinv_big, gb, dim3(256), 0, c->stream, c->gp_K.p, c->gp_Linv.p, c->gp_T.p, npad, lv, 1);
        continue;
      }
      const dim3 grid(lv / 64, lv / 64, pairs);
      hipLaunchKernelGGL(k_trinv_level, grid, dim3(256), 0, c->stream, c->gp_K.p, c->gp_Linv.p, c->gp_T.p, npad, lv, 0);
      hipLaunchKernelGGL(k_trinv_level, grid, dim3(256), 0, c->stream, c->gp_K.p, c->gp_Linv.p, c->gp_T.p, npad, lv, 1);
    }
    UT_LAUNCH_CHECK(c);
  }
  hipLaunchKernelGGL(k_lower_mv, dim3(grid1(npad, 4)), dim3(256), 0, c->stream, c->gp_Linv.p, npad, c->gp_y.p,
                     c->gp_beta.p);
  UT_LAUNCH_CHECK(c);
  if (c->gp_prec == 32 && (rc = launch_to_f32(c, c->gp_Xs.p, c->gp_Xs_f.p, (int64_t)npad * d))) return rc;
  // precision 8 scores from the digit planes of L^-1 and beta alone: a refit
  // leaves (L^-1)^T and alpha = L^-T beta to the paths that read them (the fp64
  // recompute, the next append: gp_ensure_linvt), off the chain the variance
  // GEMM waits for
  if (c->gp_prec == 8 && !app) {
    if ((rc = launch_split_i8(c, n, npad))) return rc;
    c->gp_linvt_stale = true;
    return 0;
  }
  // (an append wrote its rows of LinvT itself)
  if ((!app || c->gp_prec == 32) &&
      (rc = launch_transpose(c, c->gp_Linv.p, npad, c->gp_LinvT.p, c->gp_prec == 32 ? c->gp_LinvT_f.p : nullptr)))
    return rc;
  hipLaunchKernelGGL(k_upper_mv, dim3(grid1(npad, 4)), dim3(256), 0, c->stream, c->gp_LinvT.p, npad, c->gp_beta.p,
                     c->gp_alpha.p);
  UT_LAUNCH_CHECK(c);
  c->gp_linvt_stale = false;
  if (c->gp_prec == 16 && (rc = launch_split_h3(c, c->gp_Linv.p, npad, reinterpret_cast<_Float16*>(c->gp_LinvT_f.p))))
    return rc;
  if (c->gp_prec == 8 && (rc = launch_split_i8(c, n, npad))) return rc;
  return 0;
}

// (L^-1)^T and alpha of a precision-8 refit, on c->stream, once (fit_device)
int gp_ensure_linvt(ut_ctx* c) {
  if (!c->gp_linvt_stale) return 0;
  const int32_t npad = c->gp_npad_fit;
  int rc;
  if ((rc = launch_transpose(c, c->gp_Linv.p, npad, c->gp_LinvT.p, nullptr))) return rc;
  hipLaunchKernelGGL(k_upper_mv, dim3(grid1(npad, 4)), dim3(256), 0, c->stream, c->gp_LinvT.p, npad, c->gp_beta.p,
                     c->gp_alpha.p);
  UT_LAUNCH_CHECK(c);
  c->gp_linvt_stale = false;
  return 0;
}

// the fit's two mat-vecs on another right-hand side (gp_cons.hip: a further
// target on the same factor), on c->stream after the whole fit:
// out = L^-1 v, and out = L^-T v through (L^-1)^T
int launch_gp_lower_mv(ut_ctx* c, const double* v, double* out) {
  const int32_t npad = c->gp_npad_fit;
  hipLaunchKernelGGL(k_lower_mv, dim3(grid1(npad, 4)), dim3(256), 0, c->stream, c->gp_Linv.p, npad, v, out);
  UT_LAUNCH_CHECK(c);
  return 0;
}
int launch_gp_upper_mv(ut_ctx* c, const double* v, double* out) {
  if (int rc = gp_ensure_linvt(c)) return rc;
  const int32_t npad = c->gp_npad_fit;
  hipLaunchKernelGGL(k_upper_mv, dim3(grid1(npad, 4)), dim3(256), 0, c->stream, c->gp_LinvT.p, npad, v, out);
  UT_LAUNCH_CHECK(c);
  return 0;
}

// (for tests: ut_gp_fit_read) the factor without what gp_K keeps above its
// diagonal, and the f32 operand widened
__global__ __launch_bounds__(256) void k_fit_read_lower(const double* __restrict__ src, int32_t npad,
                                                        double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)npad * npad) return;
  out[e] = e % npad <= e / npad ? src[e] : 0.0;
}

__global__ __launch_bounds__(256) void k_fit_read_f32(const float* __restrict__ src, int64_t n,
                                                      double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e < n) out[e] = (double)src[e];
}

int launch_fit_read_lower(ut_ctx* c, const double* src, int32_t npad, double* out) {
  hipLaunchKernelGGL(k_fit_read_lower, dim3(grid1((int64_t)npad * npad, 256)), dim3(256), 0, c->stream, src, npad, out);
  UT_LAUNCH_CHECK(c);
  return 0;
}

int launch_fit_read_f32(ut_ctx* c, const float* src, int64_t n, double* out) {
  hipLaunchKernelGGL(k_fit_read_f32, dim3(grid1(n, 256)), dim3(256), 0, c->stream, src, n, out);
  UT_LAUNCH_CHECK(c);
  return 0;
}

// Host work over the training rows in 8 threads when it is large (C4: 3,680
// rows x 707 features, 20.8 MB to stage and every one-hot block to check:
// ~2-3 ms on one thread, most of it with the device idle between rounds)
template <class F>
static bool par_rows(int32_t r0, int32_t r1, int32_t d, F&& f) {
  const size_t work = (size_t)(r1 > r0 ? r1 - r0 : 0) * (size_t)d;
  const unsigned hw = std::thread::hardware_concurrency();
  const int32_t nt = work < ((size_t)1 << 19) ? 1 : (int32_t)std::min<unsigned>(8, hw > 1 ? hw : 1);
  if (nt <= 1) return f(r0, r1);
  const int32_t step = (r1 - r0 + nt - 1) / nt;
  std::vector<std::thread> th;
  std::vector<char> ok(nt, 1);
  for (int32_t t = 0; t < nt; ++t) {
    const int32_t a = r0 + t * step, b = std::min(r1, a + step);
    if (a >= b) break;
    th.emplace_back([&, t, a, b] { ok[t] = f(a, b) ? 1 : 0; });
  }
  for (auto& x : th) x.join();
  for (char v : ok)
    if (!v) return false;
  return true;
}

// Stage a fit (X, y, 1/ell in pinned memory, every buffer allocated, the
// append / categorical decisions taken) whose device work gp_fit_flush
// enqueues on the fit stream, ordered after everything already enqueued on the
// caller's stream (earlier rounds read the GP state being replaced).  Scoring
// waits on ev_fit; failure (not positive definite) is reported by gp_wait_fit
// and, on the device, by NaN scores from k_gp_finalize.
int gp_fit_enqueue(ut_ctx* c, const double* X, const double* y, int32_t n, int32_t d, const ut_gp_hyper* h) {
  UT_CHECK(c, n >= 1 && d >= 1 && X && y && h && h->lengthscale_host, UT_EINVAL, "gp_fit: bad arguments");
  const int32_t npad = gp_npad(n);
  UT_CHECK(c, c->gp_prec != 8 || npad <= I8_MAX_K, UT_EINVAL,
           "gp_fit: precision 8 takes at most 16384 training points (exact int32 digit sums)");
  c->kst_desc.invalidate();   // (ut_gp_kstar_read: c->kst is an earlier fit's from here on)
  // a fit staged and never used is enqueued first (its staging is about to be
  // reused; an append compares against it), then the previous fit's copies out
  // of the pinned staging (and its factor) are complete once ev_fit is
  int rc = gp_fit_flush(c);
  if (rc) return rc;
  if (c->fit_pending) UT_HIP(c, hipEventSynchronize(c->ev_fit));
  // Incremental fit: new rows appended to the previous fit's training set
  // (its rows a bitwise prefix of X, same hyperparameters, same padded size,
  // a positive-definite previous factor) extend L^-1 by block rows instead of
  // refactoring (k_app_*).  y is restandardised in full either way.
  const int32_t n0 = c->gp_n;
  bool app = false;
  if (c->fit_append && c->gp_ready && c->gp_Xs.p && n > n0 && npad == c->gp_npad_fit && d == c->gp_d &&
      c->gp_prec == c->gp_fit_prec && c->gp_sf2 == h->sigma_f2 && c->gp_diag_fit == h->sigma_n2 + h->jitter) {
    const double* oinv = c->fit_host + (size_t)n0 * d + n0;
    app = std::memcmp(c->fit_host, X, sizeof(double) * n0 * d) == 0;
    for (int32_t k = 0; app && k < d; ++k) {
      const double v = 1.0 / h->lengthscale_host[k];
      app = std::memcmp(&v, oinv + k, sizeof(double)) == 0;
    }
    if (app) {
      if (!c->flag_host) UT_HIP(c, hipHostMalloc((void**)&c->flag_host, sizeof(int32_t), hipHostMallocDefault));
      UT_HIP(c, hipMemcpyAsync(c->flag_host, c->gp_flag.p, sizeof(int32_t), hipMemcpyDeviceToHost, c->fit_stream));
      UT_HIP(c, hipStreamSynchronize(c->fit_stream));
      app = *c->flag_host == 0;
    }
  }
  if ((rc = gp_alloc(c, npad, d))) return rc;
  ++c->fit_gen;   // what pruned scoring cached of the previous fit (|L^-1|_F^2, ...) is stale
  const size_t need = (size_t)n * d + n + d;
  bool fresh = false;   // a new staging buffer holds no previous rows
  if (c->fit_host_n < need) {
    if (c->fit_host) hipHostFree(c->fit_host);
    c->fit_host = nullptr;
    c->fit_host_n = 0;
    // room for growth: the tuning loop appends a few rows per fit
    const size_t cap = need + need / 4 + 4096;
    UT_HIP(c, hipHostMalloc((void**)&c->fit_host, sizeof(double) * cap, hipHostMallocDefault));
    c->fit_host_n = cap;
    fresh = true;
  }
  double* hX = c->fit_host;
  double* hy = hX + (size_t)n * d;
  double* hinv = hy + n;
  // an append stages and copies only the new rows: the staging prefix was just
  // compared equal to X's (unless the staging buffer was just reallocated), and
  // the device staging (gp_tmp, same npad) still holds the previous fit's rows
  const int32_t xr0 = app && !fresh ? n0 : 0;
  par_rows(xr0, n, d, [&](int32_t a, int32_t b) {
    std::memcpy(hX + (size_t)a * d, X + (size_t)a * d, sizeof(double) * (size_t)(b - a) * d);
    return true;
  });
  std::memcpy(hy, y, sizeof(double) * n);
  for (int32_t k = 0; k < d; ++k) hinv[k] = 1.0 / h->lengthscale_host[k];
  // categorical K*: every ENUM / BOOL feature under one lengthscale and every
  // training row one-hot there (an append checks only its new rows)
  const Space& sp = c->space;
  // (and the candidates' code rows fit one workgroup's LDS: a space with
  // thousands of ENUM options scores with the dense contraction)
  bool cat = c->cat_enable && c->has_space && sp.n_cat > 0 && d == sp.n_feat && code_rows_lds(sp.cat_k) <= c->max_lds;
  double cinv = 0.0;
  if (cat) {
    cinv = hinv[sp.host_params[sp.host_cat[0]].feat_col];
    for (int32_t p : sp.host_cat) {
      const DevParam& q = sp.host_params[p];
      for (int32_t f = 0; f < q.n_feat && cat; ++f) cat = std::memcmp(&hinv[q.feat_col + f], &cinv, sizeof(double)) == 0;
      if (!cat) break;
    }
  }
  if (cat) {
    const bool prefix_ok = app && c->cat_x_ok;
    cat = par_rows(prefix_ok ? n0 : 0, n, d, [&](int32_t a, int32_t b) { return cat_rows_ok(sp, X, d, a, b); });
  }
  c->cat_x_ok = cat;
  c->cat_on = cat;
  if (cat) {
    int32_t pw = 0;
    for (int32_t p : sp.host_cat) pw += sp.host_params[p].kind == UT_BOOL ? 1 : 2;
    const double base = cinv * cinv;
    c->cat_c1 = 0.5 * base;
    c->cat_c0 = -0.5 * base * (double)pw;
  }
  const double diag = h->sigma_n2 + h->jitter;
  // every buffer the device work touches exists before it is enqueued
  const int32_t dpn = cat_dpad(c);
  if (c->cat_on) {
    if ((rc = ensure(c, c->gp_XsT_num, (size_t)(dpn > 0 ? dpn : 1) * npad))) return rc;
    if ((rc = ensure(c, c->gp_xnorm_num, (size_t)npad))) return rc;
    if ((rc = ensure(c, c->gp_acat, (size_t)sp.cat_k * npad))) return rc;
  }
  if (app) {
    size_t ws = 0;
    for (int32_t b = std::max(n0 / NB, 1); b <= (n - 1) / NB; ++b)
      ws = std::max(ws, (size_t)b * ((b * NB + APP_KC - 1) / APP_KC) * 4096);
    if (ws && (rc = ensure(c, c->app_ws, ws))) return rc;
  }
  if (c->gp_prec == 8) {
    if ((rc = alloc_split_i8(c, npad))) return rc;
    c->gp_i8_eb = i8_kstar_exp(h->sigma_f2);
    if (c->kstar_q && !c->cat_on && (rc = alloc_split_x8(c, npad, kstar_dpad(d)))) return rc;
  }
  c->gp_n = n;
  c->gp_sf2 = h->sigma_f2;
  c->gp_fit_prec = c->gp_prec;
  c->gp_npad_fit = npad;
  c->gp_diag_fit = diag;
  c->gp_sn2_fit = h->sigma_n2;
  c->gp_fit_kind = app ? 1 : 0;
  c->gp_l_rows = app ? std::min(c->gp_l_rows, n0 / NB * NB) : npad;
  c->gp_ready = true;
  ut_ctx::FitJob& j = c->fit_job;
  j.n = n, j.n0 = n0, j.d = d, j.npad = npad, j.dpn = dpn, j.xr0 = xr0;
  j.app = app, j.diag = diag, j.sf2 = h->sigma_f2;
  j.on = true;
  c->fit_prefit_set = false;
  return c->fit_defer ? 0 : gp_fit_flush(c);
}

// The staged fit's place on the caller's stream: recorded before a proposal
// is enqueued, so the fit flushed after it still runs beside it.
int gp_fit_prefit(ut_ctx* c) {
  if (!c->fit_job.on || c->fit_prefit_set) return 0;
  UT_HIP(c, hipEventRecord(c->ev_prefit, c->stream));
  c->fit_prefit_set = true;
  return 0;
}

// Enqueue the staged fit's device work on the fit stream, ordered after what
// the caller's stream held at gp_fit_prefit (or now).  Scoring waits on
// ev_fit_x (scaled inputs) / ev_fit (the factor).
int gp_fit_flush(ut_ctx* c) {
  if (!c->fit_job.on) return 0;
  const ut_ctx::FitJob j = c->fit_job;
  c->fit_job.on = false;
  // (a launch that fails below leaves no usable factor)
  c->gp_ready = false;
  if (!c->fit_prefit_set) UT_HIP(c, hipEventRecord(c->ev_prefit, c->stream));
  c->fit_prefit_set = false;
  UT_HIP(c, hipStreamWaitEvent(c->fit_stream, c->ev_prefit, 0));
  int rc;
  {
    StreamScope on_fit(c, c->fit_stream);
    if ((rc = fit_device(c, 0, j.n, j.n0, j.d, j.npad, j.dpn, j.app, j.xr0, j.diag, j.sf2))) return rc;
    UT_HIP(c, hipEventRecord(c->ev_fit_x, c->stream));   // the scaled inputs: fp64 K* may start
    if ((rc = fit_device(c, 1, j.n, j.n0, j.d, j.npad, j.dpn, j.app, j.xr0, j.diag, j.sf2))) return rc;
    UT_HIP(c, hipEventRecord(c->ev_fit, c->stream));
  }
  c->fit_pending = true;
  c->gp_ready = true;
  return 0;
}

// Wait for the enqueued fit and check it (positive definite).
int gp_wait_fit(ut_ctx* c) {
  int rc;
  if ((rc = gp_fit_flush(c))) return rc;
  if (!c->fit_pending) return 0;
  // the flag is read on the fit stream itself, after the fit (a pinned
  // asynchronous copy and that stream's sync: ~10 us once the fit is done,
  // where a blocking hipMemcpy took ~1 ms per call in the C5 loop)
  if (!c->flag_host) UT_HIP(c, hipHostMalloc((void**)&c->flag_host, sizeof(int32_t), hipHostMallocDefault));
  UT_HIP(c, hipMemcpyAsync(c->flag_host, c->gp_flag.p, sizeof(int32_t), hipMemcpyDeviceToHost, c->fit_stream));
  UT_HIP(c, hipStreamSynchronize(c->fit_stream));
  const int32_t flag = *c->flag_host;
  if (flag != 0) {
    c->gp_ready = false;
    return set_err(c, UT_ENOTPD, "gp_fit: kernel matrix is not positive definite (raise jitter)");
  }
  return 0;
}

}  // namespace ut
