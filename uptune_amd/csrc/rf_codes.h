// rf_codes.h -- what the device tree fits (forest_fit.hip, gbt_fit.hip) share:
// the 256-bin feature code and the order in which split candidates are compared.
#pragma once
#include "ut_internal.h"

namespace ut {

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

}  // namespace ut
