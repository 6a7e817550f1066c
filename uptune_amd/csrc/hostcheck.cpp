// Host (g++) build of ut_core.h, used ONLY by tests/test_core_host.py to
// check the shared arithmetic against CPython (repr, hashlib) without a GPU,
// and of gp_i8_plan.h (tests/test_i8_plan_cpu.py: precision 8's call plan and
// hint policy).  Nothing in the product path loads this library.
#include <stddef.h>
#include <string.h>
#include "gp_i8_plan.h"
#include "ut_core.h"
#include "../../include/uthot.h"

namespace {
struct BufEmit {
  char* p;
  void put(int pos, uint8_t c) { p[pos] = (char)c; }
};
// an I8Plan as bits: mask 1, screen 2, count 4, the variance kernel (0 unmasked, 1 masked, 2 the list) << 4
int plan_bits(const ut::I8Plan& p) { return (p.mask ? 1 : 0) | (p.screen ? 2 : 0) | (p.count ? 4 : 0) | ((int)p.var << 4); }
ut::I8Plan plan_of(int bits) {
  ut::I8Plan p;
  p.mask = bits & 1, p.screen = bits & 2, p.count = bits & 4, p.var = (ut::I8Var)(bits >> 4);
  return p;
}
}  // namespace

extern "C" {
// C-ABI struct sizes as the C compiler lays them out (checked against the
// ctypes mirrors in uptune_amd/_lib.py)
long long uthc_sizeof(int which) {
  switch (which) {
    case 0: return (long long)sizeof(ut_param_desc);
    case 1: return (long long)sizeof(ut_gp_hyper);
    case 2: return (long long)sizeof(ut_round_out);
    case 3: return (long long)sizeof(ut_de_params);
    case 4: return (long long)sizeof(ut_acq);
    case 5: return (long long)sizeof(ut_pso_params);
    case 6: return (long long)sizeof(ut_ga_params);
    case 7: return (long long)sizeof(ut_tree_node);
    case 8: return (long long)sizeof(ut_prune_stats);
    case 9: return (long long)sizeof(ut_gp_fit_info);
    case 10: return (long long)sizeof(ut_tr_params);
    default: return -1;
  }
}
int uthc_repr_double(double x, char* out) {
  BufEmit e{out};
  return ut::repr_double(x, e);
}
int uthc_repr_int64(long long v, char* out) {
  BufEmit e{out};
  return ut::repr_int64((int64_t)v, e);
}
void uthc_sha256(const unsigned char* msg, size_t len, unsigned char* out32) {
  uint32_t H[8];
  ut::sha256_init(H);
  size_t total = len + 9;
  size_t nblk = (total + 63) / 64;
  for (size_t b = 0; b < nblk; ++b) {
    uint32_t W[16];
    for (int w = 0; w < 16; ++w) {
      uint32_t v = 0;
      for (int t = 0; t < 4; ++t) {
        size_t pos = b * 64 + w * 4 + t;
        uint32_t byte;
        if (pos < len) byte = msg[pos];
        else if (pos == len) byte = 0x80;
        else if (pos >= nblk * 64 - 8) byte = (uint32_t)(((unsigned long long)len * 8) >> (8 * (nblk * 64 - 1 - pos))) & 0xFF;
        else byte = 0;
        v = (v << 8) | byte;
      }
      W[w] = v;
    }
    ut::sha256_compress(H, W);
  }
  for (int i = 0; i < 8; ++i)
    for (int t = 0; t < 4; ++t) out32[i * 4 + t] = (unsigned char)(H[i] >> (24 - 8 * t));
}
void uthc_philox(unsigned long long seed, unsigned long long cand, unsigned stream, unsigned round_, unsigned op,
                 unsigned* out4) {
  ut::u32x4 r = ut::draw(seed, cand, stream, round_, op);
  out4[0] = r.x; out4[1] = r.y; out4[2] = r.z; out4[3] = r.w;
}
void uthc_py_log2(const double* x, double* out, long long n) {
  for (long long i = 0; i < n; ++i) out[i] = ut::py_log2(x[i]);
}
void uthc_libm_log(const double* x, double* out, long long n) {
  for (long long i = 0; i < n; ++i) out[i] = ut::libm_log(x[i]);
}
void uthc_exp2(const double* x, double* out, long long n) {
  for (long long i = 0; i < n; ++i) out[i] = ut::exp2_cr(x[i]);
}
void uthc_logint_unscale(const double* s, double mn, double* out, long long n) {
  for (long long i = 0; i < n; ++i) out[i] = rint((ut::exp2_cr(s[i]) - 1.0) + mn);
}
void uthc_cos2pi(const double* t, double* out, long long n) {
  for (long long i = 0; i < n; ++i) out[i] = ut::cos2pi(t[i]);
}
void uthc_philox_raw(const unsigned* ctr4, const unsigned* key2, unsigned* out4) {
  ut::u32x4 c{ctr4[0], ctr4[1], ctr4[2], ctr4[3]};
  ut::u32x4 r = ut::philox4x32_10(c, key2[0], key2[1]);
  out4[0] = r.x; out4[1] = r.y; out4[2] = r.z; out4[3] = r.w;
}
// gp_i8_plan.h.  env3: UT_VAR_SKIP, UT_KSTAR_SCREEN, UT_KSTAR_STRIPS as -1 (unset) / 0 / 1;
// hints4: var_skip, screen, list, backoff; counts4: nsparse, cert, zero_bytes, blocks
void uthc_i8_env_read(int* env3) {
  const ut::I8Env e = ut::i8_env_read();
  env3[0] = (int)e.var_skip, env3[1] = (int)e.screen, env3[2] = (int)e.strips;
}
int uthc_i8_plan(int npad, int K32, const int* env3, const int* hints4) {
  const ut::I8Env e{(ut::I8Tri)env3[0], (ut::I8Tri)env3[1], (ut::I8Tri)env3[2]};
  const ut::I8Hints h{hints4[0] != 0, hints4[1] != 0, hints4[2] != 0, hints4[3]};
  return plan_bits(ut::i8_plan(npad, K32, e, h));
}
int uthc_i8_plan_no_mask() { return plan_bits(ut::I8Plan{}); }
void uthc_i8_hints_initial(int* hints4) {
  const ut::I8Hints h;
  hints4[0] = h.var_skip, hints4[1] = h.screen, hints4[2] = h.list, hints4[3] = h.backoff;
}
void uthc_i8_hints_next(const int* hints4, int plan, const long long* counts4, int* out4) {
  ut::I8Counts n;
  n.nsparse = counts4[0], n.cert = counts4[1], n.zero_bytes = counts4[2], n.blocks = counts4[3];
  const ut::I8Hints h = ut::i8_hints_next(ut::I8Hints{hints4[0] != 0, hints4[1] != 0, hints4[2] != 0, hints4[3]},
                                          plan_of(plan), n);
  out4[0] = h.var_skip, out4[1] = h.screen, out4[2] = h.list, out4[3] = h.backoff;
}
}
