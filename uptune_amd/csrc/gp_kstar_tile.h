// gp_kstar_tile.h -- the K* contraction's tile: sizes, vector types and the
// glds stage loaders, shared by k_gp_kstar / k_gp_kstar_f32c (gp_gemm.hip) and
// the feasibility vote's k_feas_sums (gp_feas.hip).
//   256-thread workgroups (2 x 2 waves of 64 x 64) on 128 x 128 tiles, K in
//   steps of 16, a 2-stage glds ring (64 KiB) so two workgroups share a CU
#pragma once
#include "ut_internal.h"

namespace ut {

constexpr int K_NT = 256, K_BM = 128, K_BN = 128, K_BK = 16;
constexpr int KSTAR_SPARE_PER_XCD = 2;   // CUs left to an in-flight GP fit (launch_gemm_kstar)

constexpr int K_SA = K_BK * K_BM, K_SB = K_BK * K_BN, K_STAGE = K_SA + K_SB;

__device__ __forceinline__ void kstar_issue(const double* __restrict__ AT, int64_t lda, const double* __restrict__ B,
                                            int64_t ldb, int32_t row0, int64_t col0, int32_t k0, double* st, int w,
                                            int lane, int32_t dpad) {
  // 16 KiB of A and 16 KiB of B per stage = 32 wave-instructions, 8 per wave;
  // wave w loads k rows 4w .. 4w+3, none past dpad (a multiple of 4: the last
  // stage of a dpad that is not a multiple of 16 is partial)
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

typedef double kd4 __attribute__((ext_vector_type(4)));
typedef int32_t ki4 __attribute__((ext_vector_type(4)));

// one int8 stage of the categorical K* (gp_gemm.hip "Categorical K*"): 128
// code columns x 128 rows (A) / candidates (B), LDS row r's 16-B chunk c at
// position c ^ (r & 7), swizzled through the glds source address
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

}  // namespace ut
