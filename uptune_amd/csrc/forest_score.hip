// forest_score.hip -- mean, variance and acquisition of an averaged tree
// ensemble per candidate in one launch (ut_forest_score): the random-forest
// surrogate of SMAC (Hutter, Hoos, Leyton-Brown 2011), over the reference's own
// model family (plugins/xgbregressor.py:50-63, src/multi_stage.py:8-22).
//
// Tree t = 0..T-1 ends in a leaf with value m_t and variance s_t (the leaf
// records' threshold field, ut_forest_leaf_var).  Every sum is in tree order:
//   mu  = (base + sum scale * m_t) / div             k_forest's pred, bit for bit
//   a_t = m_t - m_0        D1 = sum a_t, D2 = sum a_t^2, SV = sum s_t
//   var = max((D2 + SV) / T - (D1 / T)^2, 0)         law of total variance
// The shift by the candidate's own first leaf keeps D2 / T and (D1 / T)^2 of the
// order of the variance: unshifted, targets offset by 1e3 cancel 1e6-sized
// squares against each other.
//
// Two kernels with the same per-candidate operations in the same order, so
// their outputs agree bit for bit:
//   k_forest_stats         one lane per candidate, as k_forest, four sums
//   k_forest_stats_staged  4 waves per 64 candidates; features once to LDS as
//                          f32, wave w walks trees w, w+4, .. and records the
//                          leaf index; wave 0 accumulates a chunk of trees
//                          while the others walk the next one
// Bound: the chain of dependent node loads (L2), as k_forest; the staged form
// replaces each step's feature load by an LDS read and keeps four chains per
// candidate in flight.  Which one ut_forest_score launches: DESIGN.md.
#include "gp_post.h"
#include "ut_internal.h"

namespace ut {

// the running sums of one candidate, and what they end in
struct ForestSums {
  double acc, m0, D1, D2, SV;
  __device__ __forceinline__ void start(double base) {
    acc = base;
    m0 = D1 = D2 = SV = 0.0;
  }
  __device__ __forceinline__ void add(int32_t t, double scale, double value, double leaf_var) {
    if (t == 0) m0 = value;
    acc += scale * value;
    const double a = value - m0;
    D1 += a;
    D2 += a * a;
    SV += leaf_var;
  }
  __device__ __forceinline__ void finish(int64_t i, int32_t n_trees, double div, const uint8_t* __restrict__ dup,
                                         int32_t kind, double xi, double kappa, double f_best,
                                         double* __restrict__ mu, double* __restrict__ var,
                                         double* __restrict__ score) const {
    const double T = (double)n_trees;
    const double p = acc / div;
    const double e = D1 / T;
    const double v0 = (D2 + SV) / T - e * e;
    const double v = v0 > 0.0 ? v0 : 0.0;
    if (mu) mu[i] = p;
    if (var) var[i] = v;
    if (score) score[i] = (dup && dup[i]) ? -1.0 / 0.0 : acq_score(kind, p, v, f_best, xi, kappa);
  }
};

__global__ __launch_bounds__(256) void k_forest_stats(const ut_tree_node* __restrict__ nodes,
                                                      const int32_t* __restrict__ roots, int32_t n_trees,
                                                      int32_t rule, double base, double scale, double div,
                                                      int32_t n_feat, const double* __restrict__ feat, int64_t ld,
                                                      int64_t m, const uint8_t* __restrict__ dup, int32_t kind,
                                                      double xi, double kappa, double f_best,
                                                      double* __restrict__ mu, double* __restrict__ var,
                                                      double* __restrict__ score) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  ForestSums s;
  s.start(base);
  for (int32_t t = 0; t < n_trees; ++t) {
    int32_t nd = roots[t];
    ut_tree_node q = nodes[nd];
    for (int32_t depth = 0; depth < 4096 && q.feature >= 0; ++depth) {  // bounded, as k_forest
      const int32_t f = q.feature < n_feat ? q.feature : n_feat - 1;
      const double x = feat[(int64_t)f * ld + i];
      bool left;
      if (x != x) {
        left = q.default_left != 0;
      } else if (rule == UT_SPLIT_LE) {
        left = (double)(float)x <= q.threshold;
      } else {
        left = (float)x < (float)q.threshold;
      }
      nd = left ? q.left : q.right;
      q = nodes[nd];
    }
    // a walk cut off at the depth bound ends on a split: its fields are read as a leaf's, as k_forest does
    s.add(t, scale, q.value, q.threshold);
  }
  s.finish(i, n_trees, div, dup, kind, xi, kappa, f_best, mu, var, score);
}

// trees per chunk of the staged kernel: the leaf table is [2][FS_CHUNK][64] int32
constexpr int32_t FS_CHUNK = 32;
// most feature columns the staged kernel stages (64 candidates x 4 B each): 32 KiB,
// with the 16 KiB leaf table three workgroups per CU
constexpr int32_t FS_MAX_FEAT = 128;
// which kernel ut_forest_score launches where both apply: at m = 2^20, d = 64, 64
// trees the staged one takes 0.52 of the one-lane kernel's time (profiles/forest_ei.json)
constexpr bool FS_STAGED_DEFAULT = true;

__global__ __launch_bounds__(256) void k_forest_stats_staged(
    const ut_tree_node* __restrict__ nodes, const int32_t* __restrict__ roots, int32_t n_trees, int32_t rule,
    double base, double scale, double div, int32_t n_feat, const double* __restrict__ feat, int64_t ld, int64_t m,
    const uint8_t* __restrict__ dup, int32_t kind, double xi, double kappa, double f_best, double* __restrict__ mu,
    double* __restrict__ var, double* __restrict__ score) {
  extern __shared__ float fs_lds[];
  float* sx = fs_lds;                                           // [n_feat][64]
  int32_t* leaf = (int32_t*)(fs_lds + (size_t)n_feat * 64);     // [2][FS_CHUNK][64]
  const int32_t lane = threadIdx.x & 63, w = threadIdx.x >> 6;
  const int64_t i = (int64_t)blockIdx.x * 64 + lane;
  const bool live = i < m;
  // (float)x is all either split rule reads of x; a NaN stays a NaN
  for (int32_t f = w; f < n_feat; f += 4) sx[f * 64 + lane] = live ? (float)feat[(int64_t)f * ld + i] : 0.0f;
  __syncthreads();
  ForestSums s;
  s.start(base);
  for (int32_t c0 = 0, buf = 0; c0 < n_trees; c0 += FS_CHUNK, buf ^= 1) {
    const int32_t nc = n_trees - c0 < FS_CHUNK ? n_trees - c0 : FS_CHUNK;
    int32_t* tab = leaf + buf * (FS_CHUNK * 64);
    if (live) {
      for (int32_t j = w; j < nc; j += 4) {
        int32_t nd = roots[c0 + j];
        for (int32_t depth = 0; depth < 4096; ++depth) {
          const ut_tree_node q = nodes[nd];
          if (q.feature < 0) break;
          const int32_t f = q.feature < n_feat ? q.feature : n_feat - 1;
          const float x = sx[f * 64 + lane];
          bool left;
          if (x != x) {
            left = q.default_left != 0;
          } else if (rule == UT_SPLIT_LE) {
            left = (double)x <= q.threshold;
          } else {
            left = x < (float)q.threshold;
          }
          nd = left ? q.left : q.right;
        }
        tab[j * 64 + lane] = nd;
      }
    }
    // one barrier per chunk: the table of chunk c is written again in chunk
    // c + 2, which every wave enters only after wave 0 has passed chunk c + 1's
    // barrier, that is after it has read chunk c
    __syncthreads();
    if (w == 0 && live) {
      for (int32_t j = 0; j < nc; ++j) {
        const ut_tree_node* q = nodes + tab[j * 64 + lane];
        s.add(c0 + j, scale, q->value, q->threshold);
      }
    }
  }
  if (w == 0 && live) s.finish(i, n_trees, div, dup, kind, xi, kappa, f_best, mu, var, score);
}

}  // namespace ut

extern "C" int ut_forest_score(ut_ctx* c, const double* features, int64_t ld, int64_t m, int32_t n_features,
                               const uint8_t* dup, const ut_acq* acq, double f_best, double* mu, double* var,
                               double* score) {
  if (!c) return UT_EINVAL;
  UT_CHECK(c, c->forest_trees > 0, UT_EINVAL, "forest_score: call ut_forest_set first");
  UT_CHECK(c, features && n_features >= 1 && ld >= m && m >= 0, UT_EINVAL, "forest_score: bad arguments");
  UT_CHECK(c, n_features > c->forest_max_feat, UT_EINVAL,
           "forest_score: the ensemble splits on feature " + std::to_string(c->forest_max_feat) +
               " but n_features is " + std::to_string(n_features));
  UT_CHECK(c, acq != nullptr && (acq->kind == UT_ACQ_EI || acq->kind == UT_ACQ_UCB), UT_EINVAL,
           "forest_score: acq is NULL or of an unknown kind");
  UT_CHECK(c, c->forest_base == 0.0 && c->forest_scale == 1.0 && c->forest_div == (double)c->forest_trees,
           UT_EUNSUPPORTED,
           "forest_score: the variance over trees needs an averaged ensemble (base 0, scale 1, div = trees); "
           "a boosted ensemble's stages are not samples of one function");
  if (m == 0) return 0;
  // UT_FOREST_STATS (read per call, measurements only): "lane" / "staged" force a
  // kernel; the staged one still needs its features to fit the LDS budget
  const char* env = getenv("UT_FOREST_STATS");
  const bool fits = n_features <= ut::FS_MAX_FEAT;
  bool staged = fits && ut::FS_STAGED_DEFAULT;
  if (env && std::string(env) == "lane") staged = false;
  if (env && std::string(env) == "staged") staged = fits;
  if (staged) {
    const size_t lds = (size_t)n_features * 64 * sizeof(float) + 2 * ut::FS_CHUNK * 64 * sizeof(int32_t);
    hipLaunchKernelGGL(ut::k_forest_stats_staged, dim3(ut::grid1(m, 64)), dim3(256), lds, c->stream,
                       c->forest_nodes.p, c->forest_roots.p, c->forest_trees, c->forest_rule, c->forest_base,
                       c->forest_scale, c->forest_div, n_features, features, ld, m, dup, acq->kind, acq->xi,
                       acq->kappa, f_best, mu, var, score);
  } else {
    hipLaunchKernelGGL(ut::k_forest_stats, dim3(ut::grid1(m, 256)), dim3(256), 0, c->stream, c->forest_nodes.p,
                       c->forest_roots.p, c->forest_trees, c->forest_rule, c->forest_base, c->forest_scale,
                       c->forest_div, n_features, features, ld, m, dup, acq->kind, acq->xi, acq->kappa, f_best,
                       mu, var, score);
  }
  UT_LAUNCH_CHECK(c);
  return 0;
}
