// gp_i8_plan.h -- the host decisions of precision-8 dense scoring (gp_score.hip
// gp_score_dense_i8): which K* kernels and which variance kernel one call runs,
// and what the call's counts make of the hints for the next one.  Pure host
// code with nothing from HIP in it: hostcheck.cpp compiles it with g++ and
// tests/test_i8_plan_cpu.py holds both functions to a Python restatement.
#pragma once
#include <stdint.h>
#include <stdlib.h>

namespace ut {

// the masked variance kernel keeps a tile's live stages in one 64-bit set
// (past 2048 rows a tile has more than 64 stages)
constexpr int32_t I8_MASK_MAX_K = 2048;
// k_q_screen holds a strip's two top planes in LDS: 8 KiB per 32 k (48 KiB with 2048 rows' norms)
constexpr int32_t QS_MAX_K32 = 4;

// The three overrides, read from the environment once per dense call (tests
// change them between calls on one context).
enum class I8Tri : int8_t { Unset = -1, Off = 0, On = 1 };
struct I8Env {
  // UT_VAR_SKIP: any non-zero value forces the masked variance kernel; 0
  // forbids it and, with it, the screen (a screened K* needs a masked kernel)
  I8Tri var_skip = I8Tri::Unset;
  // UT_KSTAR_SCREEN: only 1 forces the screen on; every other value forces it
  // off, and a forced-off screen counts no zero blocks either
  I8Tri screen = I8Tri::Unset;
  // UT_KSTAR_STRIPS: only 1 forces a screened call's variance kernel onto the
  // strip list; every other value keeps it off the list
  I8Tri strips = I8Tri::Unset;
};
inline I8Tri i8_env_tri(const char* name, bool on_is_one) {
  const char* v = getenv(name);
  if (!v) return I8Tri::Unset;
  const int x = atoi(v);
  return (on_is_one ? x == 1 : x != 0) ? I8Tri::On : I8Tri::Off;
}
inline I8Env i8_env_read() {
  return I8Env{i8_env_tri("UT_VAR_SKIP", false), i8_env_tri("UT_KSTAR_SCREEN", true),
               i8_env_tri("UT_KSTAR_STRIPS", true)};
}

// What persists from one precision-8 dense call to the next: what the last
// call's K* looked like, read back in that call's one sync (i8_hints_next).
// Every kernel choice gives the same bits, so a stale hint costs time only.
struct I8Hints {
  // a zero plane in at least 1 block of 16: the masked variance kernel pays
  // (its guarded MFMA groups cost a dense K* about 3 %, C2 at ell = 2: 10.5 -> 10.9 ms)
  bool var_skip = true;
  bool screen = false;   // at least half of the blocks all-zero: screen the next K*
  // at least 7 blocks in 8 all-zero: the strip list.  Its instance of
  // k_gp_var_i8 is about 18 % slower per live strip than the plain masked one
  // (C2 at ell = 0.5, screen forced: 7.78 against 6.63 ms): it pays where
  // nearly all strips are dead.
  bool list = false;
  int32_t backoff = 0;   // unscreened calls left before `screen` may turn on again
};

enum class I8Var : int8_t {
  Unmasked,    // k_gp_var_i8<false>
  Masked,      // k_gp_var_i8<true>: every strip, all-zero blocks skipped
  MaskedList   // k_gp_var_i8<true, true>: only the strips of the screen's list
};

// What one call will do.
struct I8Plan {
  bool mask = false;     // K* is k_gp_kstar_q's and leaves its occupancy mask
  bool screen = false;   // k_q_screen, then the list instance of k_gp_kstar_q
  bool count = false;    // k_q_mask_zeros: the unscreened mask's all-zero bytes, for the screen hint
  I8Var var = I8Var::Unmasked;
};
// (the default I8Plan is the plan of a K* that does not go through
// launch_gemm_kstar_q -- categorical fits, UT_KSTAR_Q=0, fits with no training
// planes: no mask, so no screen, no count, the unmasked kernel, and
// i8_hints_next leaves the hints alone)

// The plan of a k_gp_kstar_q call.  The screen runs where the masked variance
// kernel can follow it (a screened K* leaves the planes of its certified units
// unwritten behind cleared mask dwords: npad <= I8_MASK_MAX_K, UT_VAR_SKIP not
// 0) and its strip's planes fit in LDS (K32 <= QS_MAX_K32).  The masked
// kernels exist up to I8_MASK_MAX_K rows only: this is the one place that
// decides by it (launch_gemm_var_i8 refuses a masked kernel past it).
inline I8Plan i8_plan(int32_t npad, int32_t K32, const I8Env& env, const I8Hints& h) {
  I8Plan p;
  p.mask = true;
  const bool can_mask = npad <= I8_MASK_MAX_K;
  const bool can_screen = can_mask && K32 <= QS_MAX_K32 && env.var_skip != I8Tri::Off;
  p.screen = can_screen && (env.screen != I8Tri::Unset ? env.screen == I8Tri::On : h.screen);
  p.count = can_screen && !p.screen && env.screen == I8Tri::Unset;
  const bool list = p.screen && (env.strips != I8Tri::Unset ? env.strips == I8Tri::On : h.list);
  const bool skip = p.screen || (env.var_skip != I8Tri::Unset ? env.var_skip == I8Tri::On : h.var_skip);
  p.var = list ? I8Var::MaskedList : (skip && can_mask ? I8Var::Masked : I8Var::Unmasked);
  return p;
}

// What a call's one sync reads back.
struct I8Counts {
  int64_t nsparse = 0;      // blocks whose mask byte is not 0x3f (kmask_cnt; a certified unit was never visited)
  int64_t cert = 0;         // units the screen certified, 8 blocks each (ks_cnt[16]; 0 unless plan.screen)
  int64_t zero_bytes = 0;   // all-zero bytes of an unscreened mask (ks_cnt[17]; 0 unless plan.count)
  int64_t blocks = 0;       // (npad / 32) * (ldk / 32)
};

inline I8Hints i8_hints_next(I8Hints h, const I8Plan& p, const I8Counts& n) {
  if (!p.mask) return h;
  const int64_t cert_blocks = p.screen ? 8 * n.cert : 0;
  h.var_skip = (n.nsparse + cert_blocks) * 16 >= n.blocks;
  // (a forced-off screen counted nothing: zero_blocks == 0)
  const int64_t zero_blocks = p.screen ? cert_blocks : (p.count ? n.zero_bytes : 0);
  h.screen = 2 * zero_blocks >= n.blocks;
  // (zero blocks the certificate cannot clear -- k* below 2^-49 of the scale by
  // less than its remainder bound -- would turn the screen on after every
  // unscreened call and off after every screened one: a screen that cleared
  // less than half holds the hint off for the next 8 unscreened calls, forced-off ones included)
  if (p.screen && !h.screen) h.backoff = 8;
  else if (!p.screen && h.backoff > 0) --h.backoff, h.screen = false;
  h.list = 8 * zero_blocks >= 7 * n.blocks;
  return h;
}

// (ut_gp_kstar_screen_stats, ut_gp_i8_stats) the last precision-8 dense call
struct I8Stats {
  int32_t screened = 0;             // its K* was screened
  int64_t cert = 0, units = 0;      // certified units; units (0 without a mask)
  int64_t recomputed = 0;           // candidates recomputed in fp64 (-1: all, the whole-round fallback)
};

}  // namespace ut
