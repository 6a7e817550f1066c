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

// ... with f_best read from the loaded constraint values' scan (gp_cons.hip:
// f_best_c, the best feasible standardised y; NaN when no row is feasible --
// the score is then P alone and this EI is never evaluated)
inline Acq make_acq_cons(const ut_ctx* c, const ut_acq* a) {
  return Acq{c->gp_sf2, c->cs_stats.p + CS_INFO, c->gp_flag.p, a->kind, a->xi, a->kappa};
}

// P_j of one constraint (uthot.h "constrained EI"): Phi((tau - mu_c) / sigma),
// sigma = sqrt(v); v == 0: mu_c <= tau ? 1 : 0.  The one place it is computed:
// k_cons_apply, the pruning bound and pruned scoring's exact stage.
__device__ __forceinline__ double cons_prob1(double mc, double tau, double v, double sigma) {
  if (v == 0.0) return mc <= tau ? 1.0 : 0.0;
  const double z = (tau - mc) / sigma;
  return 0.5 * erfc(-z * 0.70710678118654752440);
}
// the feasibility vote's factor p^gamma (k_feas_apply, pruned scoring's exact stage)
__device__ __forceinline__ double feas_factor(double p, double gamma) { return gamma == 1.0 ? p : pow(p, gamma); }

// column i's sum of the first RT row-tile partials, tile 0 upward, one call per
// quantity: the pruning proof (gp_prune.hip) needs the first R partial sums
// bitwise those of the full sum
__device__ __forceinline__ double part_sum(const double* __restrict__ part, int32_t RT, int64_t ld, int64_t i) {
  double s = 0.0;
  for (int32_t r = 0; r < RT; ++r) s += part[(int64_t)r * ld + i];
  return s;
}

// What pruned scoring needs of the loaded weights, by value (nc == 0 and no
// vote: nothing is loaded, every kernel takes its unweighted path).
//   part: cs_part [RT][nc][ldp], the constraint-mean partials of EVERY candidate
//   of the call by its own index (cons_means); st: cs_stats.
struct PruneW {
  int32_t nc, RT;
  const double* part;
  int64_t ldp;
  const double* st;
  double sf2;
  int32_t vote;   // failed rows are loaded: the exact score carries p^gamma, no bound is exact
  double gamma;
  int32_t pub;    // 0: the constraint weight gets no bound either (UT_PRUNE_WEIGHT_BOUND=0, measurements only)
  __device__ __forceinline__ bool on() const { return nc > 0 || vote != 0; }
  // values are loaded and no row is feasible: the score is P alone (k_cons_apply)
  __device__ __forceinline__ bool no_ei() const { return nc > 0 && !(st[CS_INFO + 1] > 0.0); }
  // P = prod_j P_j (j ascending) of candidate i at variance v.  UB: every
  // factor's upper bound over variances <= v instead -- 1 where tau_j - mu_cj
  // >= 0, else P_j at v itself (Phi of a negative ratio rises with sigma; v == 0
  // gives 0, as cons_prob1 does for mu_cj > tau_j)
  template <bool UB>
  __device__ __forceinline__ double P(int64_t i, double v) const {
    const double sigma = sqrt(v);
    double p = 1.0;
    for (int32_t j = 0; j < nc; ++j) {
      const double mc = sf2 * part_sum(part + (int64_t)j * ldp, RT, (int64_t)nc * ldp, i);
      const double tau = st[4 * j + 3];
      p *= UB && mc <= tau ? 1.0 : cons_prob1(mc, tau, v, sigma);
    }
    return p;
  }
  // E P of candidate i in the dense order (k_cons_apply): E its EI at f_best_c
  // (a: make_acq_cons), dropped when no row is feasible
  __device__ __forceinline__ double EP(double E, int64_t i, double v) const {
    const double p = P<false>(i, v);
    return no_ei() ? p : E * p;
  }
  // ... and its bound from a bound ub_E on E and v >= the candidate's variance
  __device__ __forceinline__ double EP_ub(double ub_E, int64_t i, double v) const {
    return (no_ei() ? 1.0 : ub_E) * (pub ? P<true>(i, v) : 1.0);
  }
};

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
