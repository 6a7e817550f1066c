// tree_fit.h -- what the two device tree fits (forest_fit.hip, gbt_fit.hip)
// share: the 256-bin codes in both layouts, the target normalisation, the
// fractional Philox draw, the histogram block that turns a node's rows into its
// best split, the prefix over a workgroup, and the host half of the two entry
// points.  What differs, the launch structure, is the reason there are two files
// and is described there.  (The rows' move to the children stays in each fit: as
// a template over the per-child sums it put the accumulators into scratch.)
#pragma once
#include "ut_internal.h"

namespace ut {

constexpr int32_t TREE_F = 16;     // features per histogram block
constexpr int32_t TREE_NT = 256;   // threads of every kernel of the fits: 4 waves

__device__ __forceinline__ uint8_t rf_code(double x) {
  const float v = floorf((float)x * 256.0f);
  return !(v > 0.0f) ? 0 : (v > 255.0f ? 255 : (uint8_t)(int32_t)v);   // NaN -> 0
}

// (s, j, b) order of the split choice: larger s, then smaller j, then smaller b
__device__ __forceinline__ bool rf_better(double s, int32_t j, int32_t b, double s2, int32_t j2, int32_t b2) {
  return s > s2 || (s == s2 && (j < j2 || (j == j2 && b < b2)));
}

// word (k & 3) of a draw: draws 4b .. 4b + 3 are the words of one Philox block
__device__ __forceinline__ uint32_t rf_word(const u32x4& r, uint32_t k) {
  k &= 3u;
  return k == 0 ? r.x : (k == 1 ? r.y : (k == 2 ? r.z : r.w));
}

// draw k of its block falls below frac, frac in (0, 1].  word < frac * 2^32 and
// word * 2^-32 < frac are the same predicate: both scalings are exact in fp64
__device__ __forceinline__ bool tree_draw_below(const u32x4& block, uint32_t k, double frac) {
  return (double)rf_word(block, k) < frac * 4294967296.0;
}

// a target in the fits' units, clamped to +-32
__device__ __forceinline__ double tree_norm(double y, double shift, double scale) {
  const double z = (y - shift) / scale;
  return z < -32.0 ? -32.0 : (z > 32.0 ? 32.0 : z);
}

// element idx of the row-major codes [n][d_pad] (padding columns 0) and its
// twin in the feature-major codes [d][n_pad]
__device__ __forceinline__ void tree_codes(int64_t idx, int32_t n, int32_t d, int32_t d_pad, int32_t n_pad,
                                           const double* __restrict__ X, uint8_t* __restrict__ rm,
                                           uint8_t* __restrict__ fm) {
  if (idx >= (int64_t)n * d_pad) return;
  const int32_t row = (int32_t)(idx / d_pad), j = (int32_t)(idx % d_pad);
  const uint8_t code = j < d ? rf_code(X[(int64_t)row * d + j]) : (uint8_t)0;
  rm[idx] = code;
  if (j < d) fm[(int64_t)j * n_pad + row] = code;
}

// exclusive prefix of a per-thread count over the workgroup's TREE_NT threads,
// and their total; wsum is free again after the caller's next barrier
// (k_gbt_round's layout scan; k_rf_split keeps its ballot, which reads as well)
__device__ __forceinline__ int32_t tree_prefix(int32_t cnt, int32_t* wsum, int32_t* total) {
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int32_t incl = cnt;
#pragma unroll
  for (int32_t o = 1; o < 64; o <<= 1) {
    const int32_t a = __shfl_up(incl, o);
    if (lane >= o) incl += a;
  }
  if (lane == 63) wsum[wave] = incl;
  __syncthreads();
  int32_t excl = incl - cnt;
  for (int32_t w = 0; w < wave; ++w) excl += wsum[w];
  *total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
  return excl;
}

// the best of the four waves' candidates
__device__ __forceinline__ RfCand tree_wave_best(const RfCand* wbest) {
  RfCand r = wbest[0];
  for (int32_t k = 1; k < 4; ++k)
    if (rf_better(wbest[k].s, wbest[k].j, wbest[k].b, r.s, r.j, r.b)) r = wbest[k];
  return r;
}

// ---- the histogram block -------------------------------------------------------
// The (W: u32, Q: i64) histograms of TREE_F features x 256 bins x 12 B = 48 KiB
// of LDS: three workgroups, twelve waves per CU of 160 KiB.  Aligned to 16 so
// that a lane's four bins are one ds_read_b128 of W and two of Q: at the
// struct's natural 8 they are ds_read2_b64 and the forest fit is 5 % slower.
struct alignas(16) TreeHistLds {
  uint32_t W[TREE_F * 256];
  unsigned long long Q[TREE_F * 256];   // an int64 added in two's complement
  RfCand wbest[4];
};
// what a row adds to its bin of every feature; w = 0: the row is skipped
struct TreeAdd {
  uint32_t w;
  int64_t v;
};

// The best split of the node whose rows are list[0 .. count) among the feature
// blocks first, first + stride, .. < nfb; the result is thread 0's alone (s < 0:
// none).  A wave takes 4 rows x 16 features per step: a lane reads one code
// byte of its row (16 contiguous bytes per row, row-major codes) and issues two
// return-less LDS atomics with what add(row) returns.  Then wave w scans
// features w, w + 4, ..: 4 bins per lane, a shuffle scan across the lanes, the
// gain SL^2 / (WL + lambda) + SR^2 / (WR + lambda) against the node's totals
// (W, Q) at the occupied bins only (an empty bin repeats its left neighbour's
// gain and loses the tie) with at least min_side on both sides, a butterfly
// reduction of (s, b).  eligible(j) must be uniform over the wave.  kSkip and
// kLambda are the forest's two savings, taken at compile time because its fit
// measured 3 to 5 % slower with them passed at run time: no row of its lists
// has w = 0, and its lambda is 0, where (double)WL + 0.0 is (double)WL bit for
// bit (profiles/tree_fit_refactor.json).
template <bool kSkip, bool kLambda, class Add, class Eligible>
__device__ __forceinline__ RfCand tree_hist_best(TreeHistLds& lds, const int32_t* __restrict__ list, int32_t count,
                                                 const uint8_t* __restrict__ rm, int32_t d, int32_t d_pad,
                                                 int32_t nfb, int32_t first, int32_t stride, uint32_t W, int64_t Q,
                                                 uint32_t min_side, double lambda, Add add, Eligible eligible) {
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  double bs = -1.0;
  int32_t bj = d, bb = 256;
  for (int32_t fb = first; fb < nfb; fb += stride) {
    for (int32_t i = threadIdx.x; i < TREE_F * 256; i += TREE_NT) lds.W[i] = 0, lds.Q[i] = 0;
    __syncthreads();
    {
      const int32_t f = lane & (TREE_F - 1), j = fb * TREE_F + f;
      if (j < d) {
        for (int32_t i = wave * 4 + (lane >> 4); i < count; i += 16) {
          const int32_t row = list[i];
          const uint32_t code = rm[(int64_t)row * d_pad + j];
          const TreeAdd a = add(row);
          if (kSkip && a.w == 0) continue;
          atomicAdd(&lds.W[f * 256 + code], a.w);
          atomicAdd(&lds.Q[f * 256 + code], (unsigned long long)a.v);
        }
      }
    }
    __syncthreads();
    for (int32_t f = wave; f < TREE_F; f += 4) {
      const int32_t j = fb * TREE_F + f;
      if (j >= d || !eligible(j)) continue;
      uint32_t hw[4], pw[4];
      int64_t pq[4];
#pragma unroll
      for (int32_t k = 0; k < 4; ++k) {
        hw[k] = lds.W[f * 256 + 4 * lane + k];
        const int64_t hq = (int64_t)lds.Q[f * 256 + 4 * lane + k];
        pw[k] = k ? pw[k - 1] + hw[k] : hw[k];
        pq[k] = k ? pq[k - 1] + hq : hq;
      }
      uint32_t sw = pw[3];
      long long sq = pq[3];
#pragma unroll
      for (int32_t o = 1; o < 64; o <<= 1) {
        const uint32_t a = __shfl_up(sw, o);
        const long long b = __shfl_up(sq, o);
        if (lane >= o) sw += a, sq += b;
      }
      const uint32_t ew = sw - pw[3];
      const int64_t eq = sq - pq[3];
      double s = -1.0;
      int32_t b = 256;
#pragma unroll
      for (int32_t k = 0; k < 4; ++k) {
        const uint32_t WL = ew + pw[k], WR = W - WL;
        if (hw[k] == 0 || 4 * lane + k > 254 || WL < min_side || WR < min_side) continue;
        const double SL = (double)(eq + pq[k]), SR = (double)(Q - (eq + pq[k]));
        const double a = SL * SL, c = SR * SR;
        const double v = kLambda ? a / ((double)WL + lambda) + c / ((double)WR + lambda)
                                 : a / (double)WL + c / (double)WR;
        if (v > s) s = v, b = 4 * lane + k;
      }
#pragma unroll
      for (int32_t o = 32; o >= 1; o >>= 1) {
        const double s2 = __shfl_xor(s, o);
        const int32_t b2 = __shfl_xor(b, o);
        if (s2 > s || (s2 == s && b2 < b)) s = s2, b = b2;
      }
      if (s >= 0.0 && rf_better(s, j, b, bs, bj, bb)) bs = s, bj = j, bb = b;
    }
    __syncthreads();   // the next block's clear
  }
  if (lane == 0) lds.wbest[wave] = RfCand{bs, bj, bb};
  __syncthreads();
  RfCand r{bs, bj, bb};
  if (threadIdx.x == 0) r = tree_wave_best(lds.wbest);
  return r;
}

// ---- the host half of ut_forest_fit and ut_gbt_fit ---------------------------------
// The arguments both take, in the order both check them: own() holds the fit's
// own checks of *fp and returns 0 or the error it set.
template <class Params, class Own>
int tree_fit_check(ut_ctx* c, const std::string& who, const double* X_host, const double* y_host, int32_t n, int32_t d,
                   const Params* fp, Own own) {
  UT_CHECK(c, X_host && y_host && fp, UT_EINVAL, who + ": X, y or the parameters are NULL");
  UT_CHECK(c, n >= 1 && n <= 16384 && d >= 1 && d <= 4096, UT_EINVAL,
           who + ": n must be in [1, 16384] and d in [1, 4096]");
  if (int e = own()) return e;
  UT_CHECK(c, __builtin_isfinite(fp->y_shift) && __builtin_isfinite(fp->y_scale) && fp->y_scale > 0.0, UT_EINVAL,
           who + ": y_shift must be finite and y_scale finite and positive");
  UT_CHECK(c, fp->round_ < (1u << 24), UT_EINVAL, who + ": round_ must be below 2^24");
  for (int32_t i = 0; i < n; ++i)
    UT_CHECK(c, __builtin_isfinite(y_host[i]), UT_EINVAL, who + ": y[" + std::to_string(i) + "] is not finite");
  return 0;
}

// The codes' padded shapes (d_pad columns in nfb blocks, n_pad rows), the
// scratch both fits fill first, and X and y on their way into it.  It writes to
// scratch alone: the fit's own allocations may follow it and still come before
// anything of the loaded ensemble is touched.
inline int tree_fit_stage(ut_ctx* c, const double* X_host, const double* y_host, int32_t n, int32_t d, int32_t* d_pad,
                          int32_t* n_pad, int32_t* nfb) {
  *nfb = (d + TREE_F - 1) / TREE_F;
  *d_pad = *nfb * TREE_F;
  *n_pad = (n + 63) / 64 * 64;
  UT_HIP(c, hipSetDevice(c->device));
  if (int e = ensure(c, c->rf_X, (size_t)n * d)) return e;
  if (int e = ensure(c, c->rf_y, (size_t)n)) return e;
  if (int e = ensure(c, c->rf_rm, (size_t)n * *d_pad)) return e;
  if (int e = ensure(c, c->rf_fm, (size_t)d * *n_pad)) return e;
  if (!c->rf_host) UT_HIP(c, hipHostMalloc((void**)&c->rf_host, 2 * sizeof(int32_t), hipHostMallocDefault));
  UT_HIP(c, hipMemcpyAsync(c->rf_X.p, X_host, sizeof(double) * (size_t)n * d, hipMemcpyHostToDevice, c->stream));
  UT_HIP(c, hipMemcpyAsync(c->rf_y.p, y_host, sizeof(double) * (size_t)n, hipMemcpyHostToDevice, c->stream));
  return 0;
}

}  // namespace ut
