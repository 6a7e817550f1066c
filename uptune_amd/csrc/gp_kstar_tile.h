// gp_kstar_tile.h -- the K* distance contraction, once: the tile's sizes and
// vector types, the glds stage loaders, one item's contraction (int8 code
// stages, then the fp64 or f32 ones, through the 2-stage ring), the ticket draw
// of its persistent kernels, the column reduction of an item's sums, and the
// host side's operand struct and padding check.  Its kernels are k_gp_kstar /
// k_gp_kstar_f32c (gp_gemm.hip: K* stored, or the f32 bound pass) and
// k_kstar_sums (gp_kstar_sums.hip: column sums alone, for the failure vote and
// the constraint means); each keeps its LDS layout and its epilogue.
//   256-thread workgroups (2 x 2 waves of 64 x 64) on 128 x 128 tiles, K in
//   steps of 16, a 2-stage glds ring (64 KiB) so two workgroups share a CU
#pragma once
#include "ut_internal.h"

namespace ut {

constexpr int K_NT = 256, K_BM = 128, K_BN = 128, K_BK = 16;

constexpr int K_SA = K_BK * K_BM, K_SB = K_BK * K_BN, K_STAGE = K_SA + K_SB;

typedef double kd4 __attribute__((ext_vector_type(4)));
typedef float kf4 __attribute__((ext_vector_type(4)));
typedef int32_t ki4 __attribute__((ext_vector_type(4)));

// one 16-k stage of the contraction's own operands, fp64 or f32 (overloads).
//   fp64: 16 KiB of A and 16 KiB of B = 32 wave-instructions, 8 per wave: wave
//         w loads k rows 4w .. 4w+3, one 1-KiB row per glds;
//   f32:  8 KiB each (the ring's stage is half used): the same k rows, two
//         512-B rows per glds (lanes 0-31 row q, 32-63 row q + 1).
// No k row at or past dpad (a multiple of 4: the last stage of a dpad that is
// not a multiple of 16 is partial).
__device__ __forceinline__ void kstar_issue(const double* __restrict__ AT, int64_t lda, const double* __restrict__ B,
                                            int64_t ldb, int32_t row0, int64_t col0, int32_t k0, double* st, int w,
                                            int lane, int32_t dpad) {
  if (k0 + 4 * w >= dpad) return;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int q = 4 * w + u;  // 0..15: A tile row k = q (128 doubles = 1 KiB)
    const double* src = AT + (int64_t)(k0 + q) * lda + row0 + lane * 2;
    __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)(st + q * 128), 16, 0, 0);
  }
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int q = 4 * w + u;
    const double* src = B + (int64_t)(k0 + q) * ldb + col0 + lane * 2;
    __builtin_amdgcn_global_load_lds(src, (__attribute__((address_space(3))) void*)(st + K_SA + q * 128), 16, 0, 0);
  }
}

__device__ __forceinline__ void kstar_issue(const float* __restrict__ AT, int64_t lda, const float* __restrict__ B,
                                            int64_t ldb, int32_t row0, int64_t col0, int32_t k0, float* st, int w,
                                            int lane, int32_t dpad) {
  if (k0 + 4 * w >= dpad) return;
  const int rr = lane >> 5, cc = (lane & 31) * 4;
#pragma unroll
  for (int u = 0; u < 2; ++u) {
    const int q = 4 * w + 2 * u;
    __builtin_amdgcn_global_load_lds(AT + (int64_t)(k0 + q + rr) * lda + row0 + cc,
                                     (__attribute__((address_space(3))) void*)(st + q * 128), 16, 0, 0);
    __builtin_amdgcn_global_load_lds(B + (int64_t)(k0 + q + rr) * ldb + col0 + cc,
                                     (__attribute__((address_space(3))) void*)(st + K_SA + q * 128), 16, 0, 0);
  }
}

// Categorical K* (CAT): ENUM and BOOL params are one-hot blocks of the GP
// features (SURVEY.md §8 GP spec: Enum one-hot, Bool {0, 1}), and with one
// lengthscale ell over those blocks a block contributes to |x - u|^2 exactly
//   2 / ell^2 (ENUM) or 1 / ell^2 (BOOL)  when the two configurations' options
//   differ, and 0 when they match.
// So -|x - u|^2 / 2 over the categorical features is c0 + c1 * M with
//   M = sum_j w_j [opt_x(j) == opt_u(j)],  w_j = 2 (ENUM), 1 (BOOL),
//   c1 = 1 / (2 ell^2),  c0 = -c1 * sum_j w_j,
// and M is the integer dot product of the training rows' weighted one-hot
// codes with the candidates' 0/1 codes (ENUM: n_opt columns, BOOL: 2).  That
// product runs on v_mfma_i32_16x16x64_i8 (exact int32, 4x the fp64 MFMA's
// rate per instruction at 16x the K), ahead of the fp64 contraction over the
// remaining ("numeric") features, and c0 + c1 M starts the fp64 accumulator.
// At C3 (HPL-64: 79 of 119 features one-hot / 0-1) the fp64 contraction's K
// drops 120 -> 40, at C4 (gcc: 552 of 707) 708 -> 156.
//   int8 stage: 128 code columns x 128 rows (A) / candidates (B) = 16 KiB per
//   operand, the fp64 stage's footprint; global layout [k / 128][row][128 B],
//   LDS row r's 16-B chunk c at position c ^ (r & 7) (swizzled through the
//   glds source address: the fragment reads are at most 2-way conflicted).
__device__ __forceinline__ void kcat_issue(const int8_t* __restrict__ Ab, const int8_t* __restrict__ Bb,
                                           double* st, int w, int lane) {
  uint8_t* sb = reinterpret_cast<uint8_t*>(st);
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int q = 4 * w + u;                      // rows 8q .. 8q + 7 of the tile (1 KiB)
    const int r = 8 * q + (lane >> 3);
    const int cch = (lane & 7) ^ (r & 7);         // the global chunk that lands at position lane & 7
    __builtin_amdgcn_global_load_lds(Ab + r * 128 + cch * 16, (__attribute__((address_space(3))) void*)(sb + q * 1024),
                                     16, 0, 0);
    __builtin_amdgcn_global_load_lds(Bb + r * 128 + cch * 16,
                                     (__attribute__((address_space(3))) void*)(sb + K_SA * 8 + q * 1024), 16, 0, 0);
  }
}

// Which tile row of A a lane feeds to MFMA row rho = lane & 15: `sig` for the
// int8 stages, `arow` for the fp64 / f32 ones.  The three MFMAs' C/D rows are
//   f64 16x16x4:               (l >> 4) + 4 q
//   i8 16x16x64, f32 16x16x4:  4 (l >> 4) + q
// and the int8 stages' accumulator has to sit where the stages after it go on:
//   kstar_rows_f64:  fp64 rows as they come; the i8 MFMA's row rho loads tile
//                    row sigma(rho) = (rho >> 2) + 4 (rho & 3), so iacc[i][jj][q]
//                    sits where acc[i][jj][q] does (scripts/exp/i8_mfma_probe.hip
//                    checks both maps);
//   kstar_rows_perm: (h3 and precision 8) the f64 MFMA's row rho loads tile row
//                    pi(rho) = 4 (rho & 3) + (rho >> 2), so a lane's four
//                    accumulator rows (l >> 4) + 4 r hold the training rows
//                    4 (l >> 4) + r; the i8 MFMA has that map by itself;
//   kstar_rows_f32:  the f32 MFMA's rows are the i8 one's.
struct KstarRows {
  int sig, arow;
};
__device__ __forceinline__ KstarRows kstar_rows_f64(int lane) {
  return {((lane & 15) >> 2) + 4 * (lane & 3), lane & 15};
}
__device__ __forceinline__ KstarRows kstar_rows_perm(int lane) {
  return {lane & 15, 4 * (lane & 3) + ((lane & 15) >> 2)};
}
__device__ __forceinline__ KstarRows kstar_rows_f32(int lane) { return {lane & 15, lane & 15}; }

// what an item's contraction reads: A = the scaled rows transposed [dpad][lda]
// (rows >= d zero), B = U' [dpad][ldb], both times KSTAR_T_SCALE; CAT: the
// codes acat [nkc][npad_a][128], bcat [nkc][ldb][128] and c0, c1 in t units
template <typename T>
struct KstarOperands {
  const T *AT, *B;
  int64_t lda, ldb;
  int32_t dpad;
  const int8_t *acat, *bcat;
  int32_t npad_a, nkc;
  T c0, c1;
};
// ... of a launch over npad training rows (AT [dpad][npad]) and ldk candidates (B [dpad][ldk])
template <typename T>
inline KstarOperands<T> kstar_operands(const T* AT, const T* B, const KstarCat& cat, int32_t npad, int64_t ldk,
                                       int32_t dpad) {
  return {AT,       B,        npad, ldk,     dpad,
          cat.acat, cat.bcat, npad, cat.nkc, (T)(cat.c0 * KSTAR_T_SCALE),
          (T)(cat.c1 * KSTAR_T_SCALE)};
}
// ... and the padding it relies on: whole row and column tiles, whole k4 steps, something to contract
inline int kstar_check(ut_ctx* c, const char* who, int32_t npad, int32_t dpad, int64_t ldk, int64_t m,
                       const KstarCat& cat) {
  const bool has_cat = cat.nkc > 0;
  UT_CHECK(c, npad % K_BM == 0 && dpad % 4 == 0 && (dpad >= 4 || has_cat) && ldk % K_BN == 0 && ldk >= m, UT_EINVAL,
           std::string(who) + ": bad padding");
  UT_CHECK(c, !has_cat || (cat.acat && cat.bcat), UT_EINVAL, std::string(who) + ": categorical operands missing");
  return 0;
}

// The ticket draw of a persistent K* kernel: the items of XCD group xcd are
// ticket[xcd]'s values j = 0, 1, ..., item j being row tile j % RTe of column
// tile ct = (j / RTe) * 8 + xcd, until ct >= CT.  The next item's ticket is
// taken at the start of the current one, so its atomic round trip overlaps the
// item's first K stage instead of sitting between two items (one ticket past
// the end per workgroup is drawn and unused).  The barrier that publishes the
// item through s_item (LDS) also publishes the exp table built before the loop.
// kstar_draw takes a ticket (thread 0 holds it); kstar_item publishes it as the
// current item j and returns its column tile; the loop is
//   kstar_draw(nxt, ...);
//   for (;;) { ct = kstar_item(nxt, ..., j); if (ct >= CT) break; kstar_draw(nxt, ...); ... }
// UNIFORM: j through readfirstlane, where per-item pointers chosen by it are to
// stay scalar.
__device__ __forceinline__ void kstar_draw(int32_t& nxt, int32_t* __restrict__ ticket, int32_t xcd) {
  if (threadIdx.x == 0) nxt = atomicAdd(&ticket[xcd], 1);
}
template <bool UNIFORM = false>
__device__ __forceinline__ int32_t kstar_item(int32_t nxt, int32_t& s_item, int32_t xcd, int32_t RTe, int32_t& j) {
  if (threadIdx.x == 0) s_item = nxt;
  __syncthreads();
  j = UNIFORM ? __builtin_amdgcn_readfirstlane(s_item) : s_item;
  return (j / RTe) * 8 + xcd;
}

// the 64 x 64 outputs of a wave, [i][jj][r]: row group i, column group jj, C/D row r
template <typename T>
struct KstarAcc {
  typedef T v4 __attribute__((ext_vector_type(4)));
  v4 a[4][4];
};

__device__ __forceinline__ kd4 kstar_mfma(double a, double b, kd4 c) {
  return __builtin_amdgcn_mfma_f64_16x16x4f64(a, b, c, 0, 0, 0);
}
__device__ __forceinline__ kf4 kstar_mfma(float a, float b, kf4 c) {
  return __builtin_amdgcn_mfma_f32_16x16x4f32(a, b, c, 0, 0, 0);
}

// The lane index afresh for an item.  The per-lane glds addresses derived from a
// loop-invariant lane index are hoisted to kernel entry; where the epilogue leaves
// no registers for them beside the 128 accumulator registers (k_kstar_sums)
// they are spilled around the item loop, and recomputing them per item from
// this opaque copy is the cheaper end.
__device__ __forceinline__ int kstar_item_lane(int lane) {
  asm volatile("" : "+v"(lane));
  return lane;
}

// One item's contraction: C = A^T B over rows row0 .. + 127 and columns col0 ..
// + 127, the CAT int8 stages first (their c0 + c1 M starts the accumulator),
// then the dpad / 16 stages of T, the last one partial.  `ring` is the 2-stage
// ring (2 * K_STAGE doubles); stage s + 1 is issued behind the barrier that
// publishes stage s.  first() issues the caller's epilogue operands by glds
// beside stage 0: they have landed when this returns, and a __syncthreads()
// then frees the ring.
// `lane` is the caller's choice, and the compiler's resource report decides it
// (-Rpass-analysis=kernel-resource-usage): pass threadIdx.x & 63 as it is where
// the kernel then has no scratch (k_gp_kstar, k_gp_kstar_f32c: the hoisted glds
// addresses fit and cost nothing per item), and kstar_item_lane of it, taken
// once per item and used by the epilogue too, where it otherwise spills
// (k_kstar_sums).  The accumulators are a local array copied into the
// value returned: taken by reference, or built in the returned struct, the
// kernels without code stages spill 108-116 B/lane.
template <typename T, bool CAT, typename First>
__device__ __forceinline__ KstarAcc<T> kstar_contract(const KstarOperands<T>& o, const KstarRows rows, int32_t row0,
                                                      int64_t col0, double* ring, int w, int lane, First&& first) {
  typedef typename KstarAcc<T>::v4 v4;
  const int wm = w >> 1, wn = w & 1;
  // dpad % 4 == 0: whole 16-k stages, then one stage of k_rem k4 steps
  const int32_t nk_full = o.dpad / K_BK, k_rem = (o.dpad % K_BK) / 4;
  const int32_t ncs = CAT ? o.nkc : 0;          // int8 stages first, then T's
  const int32_t ntot = ncs + nk_full + (k_rem ? 1 : 0);
  auto issue_stage = [&](int32_t s2, double* st) {
    if (CAT && s2 < ncs)
      kcat_issue(o.acat + ((int64_t)s2 * o.npad_a + row0) * 128, o.bcat + ((int64_t)s2 * o.ldb + col0) * 128, st, w,
                 lane);
    else
      kstar_issue(o.AT, o.lda, o.B, o.ldb, row0, col0, (s2 - ncs) * K_BK, reinterpret_cast<T*>(st), w, lane, o.dpad);
  };
  if (ntot > 0) issue_stage(0, ring);
  first();
  v4 acc[4][4];
  if constexpr (CAT) {
    // the int8 stages: M into int32 accumulators (dead once acc is started)
    ki4 iacc[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) iacc[i][jj] = (ki4){0, 0, 0, 0};
    for (int32_t s2 = 0; s2 < ncs; ++s2) {
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();  // stage s2 landed everywhere; stage s2-1 fully read
      asm volatile("" ::: "memory");
      if (s2 + 1 < ntot) issue_stage(s2 + 1, ring + ((s2 + 1) & 1) * K_STAGE);
      const int8_t* as8 = reinterpret_cast<const int8_t*>(ring + (s2 & 1) * K_STAGE);
      const int8_t* bs8 = as8 + K_SA * 8;
#pragma unroll
      for (int kk = 0; kk < 2; ++kk) {
        const int c16 = (lane >> 4) + 4 * kk;
        ki4 af[4], bf[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) {
          const int row = wm * 64 + i * 16 + rows.sig;
          af[i] = *reinterpret_cast<const ki4*>(as8 + row * 128 + ((c16 ^ (row & 7)) << 4));
        }
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const int col = wn * 64 + jj * 16 + (lane & 15);
          bf[jj] = *reinterpret_cast<const ki4*>(bs8 + col * 128 + ((c16 ^ (col & 7)) << 4));
        }
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int jj = 0; jj < 4; ++jj)
            iacc[i][jj] = __builtin_amdgcn_mfma_i32_16x16x64_i8(af[i], bf[jj], iacc[i][jj], 0, 0, 0);
      }
    }
    // c0 + c1 M (in t units: see the launches) starts T's accumulators
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          if constexpr (sizeof(T) == 8) acc[i][jj][r] = __builtin_fma((double)iacc[i][jj][r], o.c1, o.c0);
          else acc[i][jj][r] = __builtin_fmaf((float)iacc[i][jj][r], o.c1, o.c0);
        }
  } else {
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) acc[i][jj] = (v4){0, 0, 0, 0};
  }
  for (int32_t s2 = ncs; s2 < ntot; ++s2) {
    asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
    __builtin_amdgcn_s_barrier();  // stage s2 landed everywhere; stage s2-1 fully read
    asm volatile("" ::: "memory");
    if (s2 + 1 < ntot) issue_stage(s2 + 1, ring + ((s2 + 1) & 1) * K_STAGE);
    const T* as = reinterpret_cast<const T*>(ring + (s2 & 1) * K_STAGE);
    const T* bs = as + K_SA;
    // the last stage of a dpad that is not a multiple of 16 has k_rem k4 steps
    const int nks = s2 - ncs < nk_full ? K_BK / 4 : k_rem;
    // (kept a loop: unrolled around its early exit the MFMAs of a stage run 5 % slower
    // in the kernels whose epilogue needs the most registers)
#pragma nounroll
    for (int ks = 0; ks < K_BK / 4; ++ks) {
      if (ks >= nks) break;
      const int kr = ks * 4 + (lane >> 4);
      T af[4], bf[4];
#pragma unroll
      for (int i = 0; i < 4; ++i) af[i] = as[kr * K_BM + wm * 64 + i * 16 + rows.arow];
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) bf[jj] = bs[kr * K_BN + wn * 64 + jj * 16 + (lane & 15)];
#pragma unroll
      for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) acc[i][jj] = kstar_mfma(af[i], bf[jj], acc[i][jj]);
    }
  }
  if (ntot == 0) asm volatile("s_waitcnt vmcnt(0)" ::: "memory");   // the epilogue operands
  KstarAcc<T> out;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) out.a[i][jj] = acc[i][jj];
  return out;
}

// Every sum of an item's epilogue is complete here.  Without this the optimizer
// sinks column group jj's whole chain of exps below the lane test of group
// jj - 1's reduction, every row's LDS operands stay live across all four, and
// k_kstar_sums / k_gp_kstar<_Float16> spill.  The other k_gp_kstar
// and k_gp_kstar_f32c do not spill without it and lose 1 % of the pruned round
// with it: they do not call it.
template <int NA>
__device__ __forceinline__ void kstar_sums_done(double (&s)[NA][4]) {
#pragma unroll
  for (int q = 0; q < NA; ++q)
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) asm volatile("" : "+v"(s[q][jj]));
}

// The column reduction of an item's sums.  s[q][jj] is a lane's partial of sum
// q over its four rows in column group jj (column wn * 64 + jj * 16 +
// (lane & 15)).  The first NS rows of s are reduced; s may hold more
// (k_gp_kstar passes its s[2][4] with NS = 1 when only the mean is wanted).
// Lane rows by __shfl_xor 16 / 32, the two wave rows through red [NS][2][K_BN]
// (the freed ring), and thread t < K_BN gets column t's totals as out(q, total).
template <int NS, int NA, typename Out>
__device__ __forceinline__ void kstar_colsums(double (&s)[NA][4], double* red, int lane, int w, Out&& out) {
  static_assert(NS <= NA, "more sums asked for than held");
  const int t = threadIdx.x, wm = w >> 1, wn = w & 1;
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) {
    const int cl = wn * 64 + jj * 16 + (lane & 15);
    double a[NS];
#pragma unroll
    for (int q = 0; q < NS; ++q) {
      a[q] = s[q][jj];
      a[q] += __shfl_xor(a[q], 16);
      a[q] += __shfl_xor(a[q], 32);
    }
    if ((lane >> 4) == 0) {
#pragma unroll
      for (int q = 0; q < NS; ++q) red[(q * 2 + wm) * K_BN + cl] = a[q];
    }
  }
  __syncthreads();
  if (t < K_BN) {
#pragma unroll
    for (int q = 0; q < NS; ++q) out(q, red[(q * 2) * K_BN + t] + red[(q * 2 + 1) * K_BN + t]);
  }
}

}  // namespace ut
