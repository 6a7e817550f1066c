// gp_post.h -- the posterior tail shared by the kernels of gp_score.hip and
// gp_prune.hip: partial sums, clamped variance, acquisition, wave append.
#pragma once
#include "ut_internal.h"

namespace ut {

__device__ __forceinline__ double acq_score(int kind, double mu, double var, double f_best, double xi,
                                            double kappa) {
  const double sigma = sqrt(var);
  if (kind == UT_ACQ_UCB) return kappa * sigma - mu;
  const double I = f_best - mu - xi;
  if (!(sigma > 0.0)) return I > 0.0 ? I : 0.0;
  const double z = I / sigma;
  const double Phi = 0.5 * erfc(-z * 0.70710678118654752440);
  const double phi = exp(-0.5 * z * z) * 0.39894228040143267794;
  return I * Phi + sigma * phi;
}

// what every tail kernel needs of the fit and the acquisition, by value
struct Acq {
  double sf2;
  const double* stats;       // the fit's [f_best, mean, std]
  const int32_t* fit_flag;   // != 0: the (asynchronous) fit failed, nothing is selectable
  int32_t kind;
  double xi, kappa;
  __device__ __forceinline__ double score(double mu, double var) const {
    return acq_score(kind, mu, var, stats[0], xi, kappa);
  }
};
inline Acq make_acq(const ut_ctx* c, const ut_acq* a) {
  return Acq{c->gp_sf2, c->gp_stats.p, c->gp_flag.p, a->kind, a->xi, a->kappa};
}

// column i's sum of the first RT row-tile partials, tile 0 upward, one call per
// quantity: the pruning proof (gp_prune.hip) needs the first R partial sums
// bitwise those of the full sum
__device__ __forceinline__ double part_sum(const double* __restrict__ part, int32_t RT, int64_t ld, int64_t i) {
  double s = 0.0;
  for (int32_t r = 0; r < RT; ++r) s += part[(int64_t)r * ld + i];
  return s;
}

// var = max(sf2 - |L^-1 k*|^2, 0)
__device__ __forceinline__ double clamped_var(double sf2, double vs) {
  const double var = sf2 - vs;
  return var > 0.0 ? var : 0.0;
}

// out[old count ..] gets the values of the wave's lanes with keep set, in lane
// order, with one atomic per wave; every lane of the wave must call it
__device__ __forceinline__ void wave_append(bool keep, int64_t value, int64_t* __restrict__ out,
                                            unsigned long long* __restrict__ count) {
  const int lane = threadIdx.x & 63;
  const unsigned long long ball = __ballot(keep);
  const uint32_t n = __builtin_popcountll(ball);
  unsigned long long base = 0;
  if (lane == 0 && n) base = atomicAdd(count, (unsigned long long)n);
  base = __shfl(base, 0, 64);
  if (keep) out[base + __builtin_popcountll(ball & ((1ull << lane) - 1ull))] = value;
}

// gp_score.hip: mu, var and score (each may be nullptr) of m columns from the
// first RT1 mean and RT2 variance partials; out_idx: the candidate of each column
int launch_gp_finalize(ut_ctx* c, int64_t m, int32_t RT1, int32_t RT2, const double* mu_part, const double* var_part,
                       int64_t ldp, const Acq& a, const uint8_t* dup, double* mu, double* var, double* score,
                       const int64_t* out_idx = nullptr);

}  // namespace ut
