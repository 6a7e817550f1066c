// forest_fit.hip -- ut_forest_fit: the random-forest surrogate (forest_score.hip)
// grown on the device, in place of the host refit by RandomForestRegressor.fit
// that the reference's model family gets (plugins/xgbregressor.py:50-63,
// src/multi_stage.py:8-22 train on the host too).
//
// A histogram forest whose every sum is an integer (uthot.h states the
// definition): features are binned to 256 codes, targets to 16.16 fixed point,
// so per node and bin W = sum w, Q1 = sum w q, Q2 = sum w q^2 are exact whatever
// the order of the atomics and however the work is split, and the trees depend
// on nothing but the data, the parameters and the Philox draws.
//
// Trees grow level by level, all trees at once; a level's nodes are a
// contiguous index range per tree (breadth first), one launch each of
//   k_rf_hist       (tree, node of the level, feature block): the histogram
//                   block of tree_fit.h over the node's rows, each adding
//                   (w, w q).  One candidate per (node, block) leaves the CU.
//   k_rf_split      one workgroup per tree: reduces the level's candidates,
//                   numbers the children by a scan of the split flags in node
//                   order, writes the records of the nodes that split or end.
//   k_rf_partition  (tree, node that split): moves the node's slice of the row
//                   list to the other copy, left rows from the front, right
//                   rows from the back (order inside a child is free), sums
//                   the children's W, Q1, Q2, min q, max q with LDS atomics
//                   and closes children that are leaves already.
// The host reads one word per level (the widest next level: the next grid, 0 =
// done).  k_rf_offsets / k_rf_compact then lay the trees out contiguously.
#include "ut_internal.h"
#include "tree_fit.h"   // what gbt_fit.hip shares: the codes, the histogram block, the host half

namespace ut {

constexpr int32_t RF_MAX_FB = 64;    // workgroups per node; more feature blocks are strided over them
constexpr int32_t RF_NT = TREE_NT;

struct RfParams {
  int32_t n, d, d_pad, n_pad, T, min_leaf;
  int32_t max_level;   // nodes at this depth are leaves: max_depth, or the bound that n / min_leaf sets
  int32_t bootstrap;
  int32_t cap;         // node records per tree
  int32_t width_cap;   // nodes per level and tree
  int32_t nfb, nfb_grid;
  double feature_frac, y_shift, y_scale;
  uint64_t seed;
  uint32_t round_;
};

// rf_ctl: [0] total nodes, [1] largest split feature, [RF_CTL_W + L] widest level L of any tree,
// then per tree the level ranges (lb, le) by level parity and the tree's size
constexpr int32_t RF_CTL_W = 2;
__host__ __device__ inline int32_t rf_ctl_tree(int32_t max_level, int32_t t) { return RF_CTL_W + max_level + 2 + 5 * t; }

__device__ __forceinline__ int32_t rf_quant(double y, double shift, double scale) {
  return (int32_t)nearbyint(tree_norm(y, shift, scale) * 65536.0);
}

// a node's mean and variance in the caller's units; a leaf's threshold field is its variance
__device__ __forceinline__ double rf_value(const RfParams& p, uint32_t W, int64_t Q1) {
  const double m = (double)Q1 / (double)W;
  return p.y_shift + p.y_scale * (m / 65536.0);
}
__device__ __forceinline__ void rf_leaf(const RfParams& p, ut_tree_node* rec, uint32_t W, int64_t Q1, uint64_t Q2) {
  const double m = (double)Q1 / (double)W;
  const double v0 = (double)Q2 / (double)W - m * m;
  const double v = v0 > 0.0 ? v0 : 0.0;
  ut_tree_node r;
  r.feature = -1, r.left = -1, r.right = -1, r.default_left = 0;
  r.threshold = (p.y_scale * p.y_scale) * (v / 4294967296.0);
  r.value = rf_value(p, W, Q1);
  *rec = r;
}
__device__ __forceinline__ bool rf_closed(const RfParams& p, uint32_t W, int32_t depth, int32_t qmin, int32_t qmax) {
  return W < 2u * (uint32_t)p.min_leaf || depth >= p.max_level || qmin == qmax;
}

__device__ __forceinline__ bool rf_eligible(const RfParams& p, int32_t t, int32_t node, int32_t j) {
  if (p.feature_frac >= 1.0) return true;
  return tree_draw_below(draw(p.seed, ((uint64_t)(uint32_t)node << 32) | (uint32_t)(j >> 2), 0x10000u | (uint32_t)t,
                              p.round_, OP_RF),
                         (uint32_t)j, p.feature_frac);
}

// ---- prepare ---------------------------------------------------------------
// codes in both layouts (padding columns 0), q, and the weights' start value
__global__ __launch_bounds__(RF_NT) void k_rf_prepare(RfParams p, const double* __restrict__ X,
                                                      const double* __restrict__ y, uint8_t* __restrict__ rm,
                                                      uint8_t* __restrict__ fm, int32_t* __restrict__ q,
                                                      uint32_t* __restrict__ w) {
  const int64_t idx = (int64_t)blockIdx.x * RF_NT + threadIdx.x;
  tree_codes(idx, p.n, p.d, p.d_pad, p.n_pad, X, rm, fm);
  if (idx < p.n) q[idx] = rf_quant(y[idx], p.y_shift, p.y_scale);
  const int64_t stride = (int64_t)gridDim.x * RF_NT, nw = (int64_t)p.T * p.n;
  const uint32_t w0 = p.bootstrap ? 0u : 1u;
  for (int64_t k = idx; k < nw; k += stride) w[k] = w0;
}

// draws 4b .. 4b + 3 of tree t: the words of draw(seed, b, t, round, OP_RF)
__global__ __launch_bounds__(RF_NT) void k_rf_bootstrap(RfParams p, uint32_t* __restrict__ w) {
  const int32_t nb = (p.n + 3) / 4;
  const int64_t idx = (int64_t)blockIdx.x * RF_NT + threadIdx.x;
  if (idx >= (int64_t)p.T * nb) return;
  const int32_t t = (int32_t)(idx / nb), b = (int32_t)(idx % nb);
  const u32x4 r = draw(p.seed, (uint64_t)b, (uint32_t)t, p.round_, OP_RF);
  const uint32_t word[4] = {r.x, r.y, r.z, r.w};
#pragma unroll
  for (int32_t k = 0; k < 4; ++k)
    if (4 * b + k < p.n) atomicAdd(&w[(int64_t)t * p.n + umulhi32(word[k], (uint32_t)p.n)], 1u);
}

// the sums of one side of a partition (or of a root), gathered with LDS atomics
struct RfSide {
  uint32_t cnt, W;
  unsigned long long Q1, Q2;   // Q1 is an int64 added in two's complement
  int32_t qmin, qmax;
};
__device__ __forceinline__ void rf_side_clear(RfSide* s) {
  s->cnt = 0, s->W = 0, s->Q1 = 0, s->Q2 = 0, s->qmin = INT32_MAX, s->qmax = INT32_MIN;
}
struct RfAcc {
  uint32_t W = 0;
  int64_t Q1 = 0;
  uint64_t Q2 = 0;
  int32_t qmin = INT32_MAX, qmax = INT32_MIN;
  __device__ __forceinline__ void add(uint32_t w, int32_t q) {
    W += w;
    Q1 += (int64_t)w * q;
    Q2 += (uint64_t)w * (uint64_t)((int64_t)q * q);
    qmin = q < qmin ? q : qmin;
    qmax = q > qmax ? q : qmax;
  }
  __device__ __forceinline__ void flush(RfSide* s) const {
    if (W == 0) return;
    atomicAdd(&s->W, W);
    atomicAdd(&s->Q1, (unsigned long long)Q1);
    atomicAdd(&s->Q2, (unsigned long long)Q2);
    atomicMin(&s->qmin, qmin);
    atomicMax(&s->qmax, qmax);
  }
};
__device__ __forceinline__ void rf_open_node(const RfParams& p, RfState* st, ut_tree_node* rec, int32_t start,
                                             int32_t depth, const RfSide& s) {
  RfState v;
  v.start = start, v.count = (int32_t)s.cnt, v.W = s.W, v.depth = depth;
  v.Q1 = (int64_t)s.Q1, v.Q2 = s.Q2, v.qmin = s.qmin, v.qmax = s.qmax;
  v.closed = rf_closed(p, s.W, depth, s.qmin, s.qmax) ? 1 : 0;
  v.bin = -1;
  *st = v;
  if (v.closed) rf_leaf(p, rec, v.W, v.Q1, v.Q2);
}

// one workgroup per tree: the rows with w > 0 and the root
__global__ __launch_bounds__(RF_NT) void k_rf_rows(RfParams p, const uint32_t* __restrict__ w,
                                                   const int32_t* __restrict__ q, int32_t* __restrict__ rows,
                                                   RfState* __restrict__ state, ut_tree_node* __restrict__ tnodes,
                                                   int32_t* __restrict__ ctl) {
  __shared__ RfSide side;
  const int32_t t = blockIdx.x;
  if (threadIdx.x == 0) rf_side_clear(&side);
  __syncthreads();
  RfAcc acc;
  for (int32_t row = threadIdx.x; row < p.n; row += RF_NT) {
    const uint32_t wv = w[(int64_t)t * p.n + row];
    if (wv == 0) continue;
    rows[(int64_t)t * p.n + atomicAdd(&side.cnt, 1u)] = row;
    acc.add(wv, q[row]);
  }
  acc.flush(&side);
  __syncthreads();
  if (threadIdx.x == 0) {
    rf_open_node(p, &state[(int64_t)t * p.cap], &tnodes[(int64_t)t * p.cap], 0, 0, side);
    int32_t* tc = ctl + rf_ctl_tree(p.max_level, t);
    tc[0] = 0, tc[1] = 1, tc[2] = 0, tc[3] = 0, tc[4] = 1;
  }
}

// ---- the level's histograms and its best split per feature block -------------
__global__ __launch_bounds__(RF_NT) void k_rf_hist(RfParams p, int32_t level, const int32_t* __restrict__ ctl,
                                                   const RfState* __restrict__ state,
                                                   const int32_t* __restrict__ rows, const uint8_t* __restrict__ rm,
                                                   const int32_t* __restrict__ q, const uint32_t* __restrict__ w,
                                                   RfCand* __restrict__ cand) {
  __shared__ TreeHistLds lds;
  const int32_t t = blockIdx.z, pos = blockIdx.y;
  const int32_t* tc = ctl + rf_ctl_tree(p.max_level, t) + 2 * (level & 1);
  const int32_t node = tc[0] + pos;
  if (node >= tc[1]) return;
  const RfState st = state[(int64_t)t * p.cap + node];
  if (st.closed) return;
  const uint32_t* wt = w + (int64_t)t * p.n;
  // the gain is the boosted fit's at lambda = 0; no row of the list has w = 0
  const RfCand r = tree_hist_best<false, false>(
      lds, rows + (int64_t)t * p.n + st.start, st.count, rm, p.d, p.d_pad, p.nfb, (int32_t)blockIdx.x,
      (int32_t)gridDim.x, st.W, st.Q1, (uint32_t)p.min_leaf, 0.0,
      [&](int32_t row) { return TreeAdd{wt[row], (int64_t)wt[row] * q[row]}; },
      [&](int32_t j) { return rf_eligible(p, t, node, j); });
  if (threadIdx.x == 0) cand[((int64_t)t * p.width_cap + pos) * p.nfb_grid + blockIdx.x] = r;
}

// ---- the level's decisions, one workgroup per tree ---------------------------
__global__ __launch_bounds__(RF_NT) void k_rf_split(RfParams p, int32_t level, int32_t* __restrict__ ctl,
                                                    RfState* __restrict__ state, ut_tree_node* __restrict__ tnodes,
                                                    const RfCand* __restrict__ cand) {
  __shared__ int32_t wsum[4];
  __shared__ int32_t base;
  const int32_t t = blockIdx.x, lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  int32_t* tc = ctl + rf_ctl_tree(p.max_level, t);
  const int32_t lb = tc[2 * (level & 1)], le = tc[2 * (level & 1) + 1], width = le - lb;
  // children that still fit the tree's records and the next level's grid (a
  // tree of k leaves has 2k - 1 nodes and k <= n / min_leaf: never the limit)
  const int32_t room = min((p.cap - le) / 2, p.width_cap / 2);
  if (threadIdx.x == 0) base = 0;
  __syncthreads();
  for (int32_t c0 = 0; c0 < width; c0 += RF_NT) {
    const int32_t pos = c0 + threadIdx.x, node = lb + pos;
    RfState* st = state + (int64_t)t * p.cap + node;
    const bool open = pos < width && !st->closed;
    RfCand best{-1.0, p.d, 256};
    if (open) {
      const RfCand* cs = cand + ((int64_t)t * p.width_cap + pos) * p.nfb_grid;
      for (int32_t k = 0; k < p.nfb_grid; ++k) {
        const RfCand v = cs[k];
        if (v.s >= 0.0 && rf_better(v.s, v.j, v.b, best.s, best.j, best.b)) best = v;
      }
    }
    bool split = open && best.s >= 0.0;
    const uint64_t mask = __ballot(split);
    if (lane == 0) wsum[wave] = __popcll(mask);
    __syncthreads();
    int32_t excl = base + __popcll(mask & ((1ull << lane) - 1ull));
    for (int32_t k = 0; k < wave; ++k) excl += wsum[k];
    const int32_t total = wsum[0] + wsum[1] + wsum[2] + wsum[3];
    split = split && excl < room;
    if (open) {
      ut_tree_node* rec = tnodes + (int64_t)t * p.cap + node;
      if (split) {
        ut_tree_node r;
        r.feature = best.j, r.left = le + 2 * excl, r.right = r.left + 1, r.default_left = 1;
        r.threshold = (double)(best.b + 1) / 256.0;
        r.value = rf_value(p, st->W, st->Q1);
        *rec = r;
        st->bin = best.b;
        atomicMax(&ctl[1], best.j);
      } else {
        rf_leaf(p, rec, st->W, st->Q1, st->Q2);
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) base += total;
    __syncthreads();
  }
  if (threadIdx.x == 0) {
    const int32_t nw = 2 * min(base, room);
    tc[2 * ((level + 1) & 1)] = le, tc[2 * ((level + 1) & 1) + 1] = le + nw;
    tc[4] = le + nw;
    if (nw) atomicMax(&ctl[RF_CTL_W + level + 1], nw);
  }
}

// ---- the rows of a node that split go to its children ------------------------
__global__ __launch_bounds__(RF_NT) void k_rf_partition(RfParams p, int32_t level, const int32_t* __restrict__ ctl,
                                                        RfState* __restrict__ state,
                                                        ut_tree_node* __restrict__ tnodes,
                                                        const int32_t* __restrict__ src, int32_t* __restrict__ dst,
                                                        const uint8_t* __restrict__ fm,
                                                        const int32_t* __restrict__ q,
                                                        const uint32_t* __restrict__ w) {
  __shared__ RfSide side[2];
  const int32_t t = blockIdx.y, pos = blockIdx.x;
  const int32_t* tc = ctl + rf_ctl_tree(p.max_level, t) + 2 * (level & 1);
  const int32_t node = tc[0] + pos;
  if (node >= tc[1]) return;
  const RfState st = state[(int64_t)t * p.cap + node];
  const ut_tree_node rec = tnodes[(int64_t)t * p.cap + node];
  if (st.closed || rec.feature < 0) return;
  if (threadIdx.x < 2) rf_side_clear(&side[threadIdx.x]);
  __syncthreads();
  const int32_t* from = src + (int64_t)t * p.n + st.start;
  int32_t* to = dst + (int64_t)t * p.n + st.start;
  const uint8_t* col = fm + (int64_t)rec.feature * p.n_pad;
  const uint32_t* wt = w + (int64_t)t * p.n;
  RfAcc accL, accR;
  for (int32_t i = threadIdx.x; i < st.count; i += RF_NT) {
    const int32_t row = from[i];
    const bool left = (int32_t)col[row] <= st.bin;
    if (left) {
      to[atomicAdd(&side[0].cnt, 1u)] = row;
      accL.add(wt[row], q[row]);
    } else {
      to[st.count - 1 - (int32_t)atomicAdd(&side[1].cnt, 1u)] = row;
      accR.add(wt[row], q[row]);
    }
  }
  accL.flush(&side[0]);
  accR.flush(&side[1]);
  __syncthreads();
  if (threadIdx.x < 2) {
    const int32_t child = threadIdx.x ? rec.right : rec.left;
    const int32_t start = st.start + (threadIdx.x ? (int32_t)side[0].cnt : 0);
    rf_open_node(p, &state[(int64_t)t * p.cap + child], &tnodes[(int64_t)t * p.cap + child], start, st.depth + 1,
                 side[threadIdx.x]);
  }
}

// ---- the contiguous ensemble ----------------------------------------------------
__global__ __launch_bounds__(RF_NT) void k_rf_offsets(RfParams p, int32_t* __restrict__ ctl,
                                                      int32_t* __restrict__ roots) {
  __shared__ int32_t size[256];
  if ((int32_t)threadIdx.x < p.T) size[threadIdx.x] = ctl[rf_ctl_tree(p.max_level, threadIdx.x) + 4];
  __syncthreads();
  if (threadIdx.x == 0) {
    int32_t off = 0;
    for (int32_t t = 0; t < p.T; ++t) roots[t] = off, off += size[t];
    ctl[0] = off;
  }
}

__global__ __launch_bounds__(RF_NT) void k_rf_compact(RfParams p, const int32_t* __restrict__ ctl,
                                                      const int32_t* __restrict__ roots,
                                                      const ut_tree_node* __restrict__ tnodes,
                                                      ut_tree_node* __restrict__ out) {
  const int32_t t = blockIdx.y, k = blockIdx.x * RF_NT + threadIdx.x;
  if (k >= ctl[rf_ctl_tree(p.max_level, t) + 4]) return;
  ut_tree_node r = tnodes[(int64_t)t * p.cap + k];
  if (r.feature >= 0) r.left += roots[t], r.right += roots[t];
  out[(int64_t)roots[t] + k] = r;
}

__global__ void k_rf_ctl_clear(int32_t* __restrict__ ctl, int32_t count) {
  const int32_t i = blockIdx.x * blockDim.x + threadIdx.x;
  if (i < count) ctl[i] = i == 1 ? -1 : 0;
}

}  // namespace ut

extern "C" int ut_forest_fit(ut_ctx* c, const double* X_host, const double* y_host, int32_t n, int32_t d,
                             const ut_forest_fit_params* fp) {
  using namespace ut;
  if (!c) return UT_EINVAL;
  if (int e = tree_fit_check(c, "forest_fit", X_host, y_host, n, d, fp, [&]() -> int {
        UT_CHECK(c, fp->n_trees >= 1 && fp->n_trees <= 256, UT_EINVAL, "forest_fit: n_trees must be in [1, 256]");
        UT_CHECK(c, fp->min_leaf >= 1, UT_EINVAL, "forest_fit: min_leaf must be at least 1");
        UT_CHECK(c, fp->max_depth >= 0 && fp->max_depth <= n, UT_EINVAL,
                 "forest_fit: max_depth must be 0 or in [1, n]");
        UT_CHECK(c, fp->bootstrap == 0 || fp->bootstrap == 1, UT_EINVAL, "forest_fit: bootstrap must be 0 or 1");
        UT_CHECK(c, fp->feature_frac > 0.0 && fp->feature_frac <= 1.0, UT_EINVAL,
                 "forest_fit: feature_frac must be in (0, 1]");
        return 0;
      }))
    return e;

  RfParams p;
  p.n = n, p.d = d, p.T = fp->n_trees, p.min_leaf = fp->min_leaf, p.bootstrap = fp->bootstrap;
  const int32_t leaves = std::max(1, n / p.min_leaf);
  p.max_level = std::min(fp->max_depth ? fp->max_depth : n, n / p.min_leaf + 1);
  p.cap = 2 * leaves + 1;
  p.width_cap = leaves + 1;
  p.feature_frac = fp->feature_frac, p.y_shift = fp->y_shift, p.y_scale = fp->y_scale;
  p.seed = c->seed, p.round_ = fp->round_;
  const int32_t T = p.T;
  const int32_t n_ctl = rf_ctl_tree(p.max_level, T);

  // every allocation before anything of the loaded ensemble is touched
  if (int e = tree_fit_stage(c, X_host, y_host, n, d, &p.d_pad, &p.n_pad, &p.nfb)) return e;
  p.nfb_grid = std::min(p.nfb, RF_MAX_FB);
  if (int e = ensure(c, c->rf_q, (size_t)n)) return e;
  if (int e = ensure(c, c->rf_w, (size_t)T * n)) return e;
  if (int e = ensure(c, c->rf_rows, (size_t)2 * T * n)) return e;
  if (int e = ensure(c, c->rf_state, (size_t)T * p.cap)) return e;
  if (int e = ensure(c, c->rf_tnodes, (size_t)T * p.cap)) return e;
  if (int e = ensure(c, c->rf_cand, (size_t)T * p.width_cap * p.nfb_grid)) return e;
  if (int e = ensure(c, c->rf_ctl, (size_t)n_ctl)) return e;
  DevBuf<int32_t> roots;
  if (int e = dalloc(c, roots, (size_t)T)) return e;

  hipStream_t s = c->stream;
  hipLaunchKernelGGL(k_rf_ctl_clear, dim3(grid1(n_ctl, 256)), dim3(256), 0, s, c->rf_ctl.p, n_ctl);
  hipLaunchKernelGGL(k_rf_prepare, dim3(grid1((int64_t)n * p.d_pad, RF_NT)), dim3(RF_NT), 0, s, p, c->rf_X.p,
                     c->rf_y.p, c->rf_rm.p, c->rf_fm.p, c->rf_q.p, c->rf_w.p);
  if (p.bootstrap)
    hipLaunchKernelGGL(k_rf_bootstrap, dim3(grid1((int64_t)T * ((n + 3) / 4), RF_NT)), dim3(RF_NT), 0, s, p,
                       c->rf_w.p);
  int32_t* rows[2] = {c->rf_rows.p, c->rf_rows.p + (size_t)T * n};
  hipLaunchKernelGGL(k_rf_rows, dim3(T), dim3(RF_NT), 0, s, p, c->rf_w.p, c->rf_q.p, rows[0], c->rf_state.p,
                     c->rf_tnodes.p, c->rf_ctl.p);
  UT_LAUNCH_CHECK(c);

  // one launch of each kernel per level; the level count is bounded on the
  // host, so no outcome on the device can keep this loop going
  int32_t width = 1;
  for (int32_t level = 0; level < p.max_level && width > 0; ++level) {
    hipLaunchKernelGGL(k_rf_hist, dim3(p.nfb_grid, width, T), dim3(RF_NT), 0, s, p, level, c->rf_ctl.p,
                       c->rf_state.p, rows[level & 1], c->rf_rm.p, c->rf_q.p, c->rf_w.p, c->rf_cand.p);
    hipLaunchKernelGGL(k_rf_split, dim3(T), dim3(RF_NT), 0, s, p, level, c->rf_ctl.p, c->rf_state.p,
                       c->rf_tnodes.p, c->rf_cand.p);
    UT_LAUNCH_CHECK(c);
    UT_HIP(c, hipMemcpyAsync(c->rf_host, c->rf_ctl.p + RF_CTL_W + level + 1, sizeof(int32_t),
                             hipMemcpyDeviceToHost, s));
    UT_HIP(c, hipStreamSynchronize(s));
    const int32_t next = std::min(c->rf_host[0], p.width_cap);
    if (next > 0) {
      hipLaunchKernelGGL(k_rf_partition, dim3(width, T), dim3(RF_NT), 0, s, p, level, c->rf_ctl.p, c->rf_state.p,
                         c->rf_tnodes.p, rows[level & 1], rows[(level + 1) & 1], c->rf_fm.p, c->rf_q.p, c->rf_w.p);
      UT_LAUNCH_CHECK(c);
    }
    width = next;
  }

  hipLaunchKernelGGL(k_rf_offsets, dim3(1), dim3(RF_NT), 0, s, p, c->rf_ctl.p, roots.p);
  UT_LAUNCH_CHECK(c);
  UT_HIP(c, hipMemcpyAsync(c->rf_host, c->rf_ctl.p, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  UT_HIP(c, hipStreamSynchronize(s));
  const int32_t total = c->rf_host[0], max_feat = c->rf_host[1];
  UT_CHECK(c, total >= T && (int64_t)total <= (int64_t)T * p.cap, UT_EHIP, "forest_fit: the trees' sizes are off");
  DevBuf<ut_tree_node> nodes;
  if (int e = dalloc(c, nodes, (size_t)total)) return e;
  hipLaunchKernelGGL(k_rf_compact, dim3(grid1(p.cap, RF_NT), T), dim3(RF_NT), 0, s, p, c->rf_ctl.p, roots.p,
                     c->rf_tnodes.p, nodes.p);
  UT_LAUNCH_CHECK(c);
  return forest_install(c, nodes, total, roots, T, max_feat, 0.0, 1.0, (double)T);
}
