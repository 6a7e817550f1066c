// gbt_fit.hip -- ut_gbt_fit: a gradient-boosted tree ensemble fitted on the
// device, the model family the reference retrains every interval on the host
// (plugins/xgbregressor.py:35-41, :72-78: XGBRegressor, 300 rounds of depth 10).
//
// Squared-error boosting on the forest fit's integer footing (uthot.h states the
// definition): features are 256-bin codes, a round's gradients are 16.16 fixed
// point, so per node and bin H = rows and G = sum g are exact whatever the order
// of the atomics, and the ensemble depends on the data, the parameters and the
// Philox draws alone.  The formulae are those of XGBoost's hist method on
// uniform bins; its bits they are not.
//
// Boosted trees come one after another, so the forest fit's scheme (all trees
// at once, three launches and a host read-back per level) has nothing to fill
// the chip with and would wait on the host 3,000 times a refit.  Here a tree is
// max_depth + 2 launches, nothing is read back until the last round is queued,
// and every level's grid is known on the host:
//   k_gbt_round   (rows / 256): the round's gradients from pred, its sample
//                 draw, the root's row list (every row) and its sums (one pair of
//                 global integer atomics per workgroup).  Workgroup 0 first lays
//                 the previous tree out behind the trees before it: a scan of
//                 the live flags of its heap (at most 2^13 - 1), children
//                 numbered by their rank, and the heap cleared for the round
//                 after this one.  The two rounds' heaps are two copies, so no
//                 workgroup clears what another adds to.
//   k_gbt_level   (slice, heap node of the level): a node is addressed by its
//                 heap index, children of k at 2k + 1 and 2k + 2, so level L's
//                 grid is 2^L nodes whatever the tree looks like, and a
//                 workgroup whose node is not open leaves on its first load.
//                 The host picks slices = clamp(ceil(256 / 2^L), 1, feature
//                 blocks): nodes x slices is about the CU count at every level.
//                 A slice takes feature blocks slice, slice + slices, ..: the
//                 histogram block of tree_fit.h, the one k_rf_hist runs, over
//                 the sampled rows only, each adding (1, g), with lambda in
//                 the gain's denominators.  It writes its best candidate and
//                 takes a ticket on the node (agent-scope acq_rel).  The
//                 workgroup that draws the last
//                 ticket reads the slices' candidates and decides the node:
//                 a leaf adds its step to pred of every row it holds, sampled
//                 or not (which is why no round needs a predict pass); a split
//                 moves all its rows to the other copy of the list, left from
//                 the front, right from the back, sums the children's G and H
//                 over the sampled rows and opens them.  Nobody waits for
//                 anybody: a workgroup that is not last has already left.
// Levels past a tree's last open node run as empty grids.
#include "ut_internal.h"
#include "tree_fit.h"

namespace ut {

constexpr int32_t GBT_NT = TREE_NT;
constexpr int32_t GBT_WG = 256;        // workgroups a level aims at: the CUs of gfx950; also the most slices of a node
constexpr int32_t GBT_HEAP_MAX = 8191; // 2^(12 + 1) - 1

struct GbtParams {
  int32_t n, d, d_pad, n_pad, nfb;
  int32_t n_rounds, max_depth, min_child;
  int32_t heap;        // 2^(max_depth + 1) - 1 nodes
  int32_t out_cap;     // records the output holds
  double eta, lambda, gamma, subsample, colsample, y_shift, y_scale;
  uint64_t seed;
  uint32_t round_;
};

__device__ __forceinline__ bool gbt_sampled(const GbtParams& p, int32_t r, int32_t row) {
  if (p.subsample >= 1.0) return true;
  return tree_draw_below(draw(p.seed, (uint64_t)(uint32_t)(row >> 2), (uint32_t)r, p.round_, OP_GBT), (uint32_t)row,
                         p.subsample);
}

// every node of a level sees the same features
__device__ __forceinline__ bool gbt_eligible(const GbtParams& p, int32_t r, int32_t level, int32_t j) {
  if (p.colsample >= 1.0) return true;
  return tree_draw_below(draw(p.seed, ((uint64_t)(uint32_t)level << 32) | (uint32_t)(j >> 2), 0x10000u | (uint32_t)r,
                              p.round_, OP_GBT),
                         (uint32_t)j, p.colsample);
}

// a node's step in normalised units: eta * (-G / (H + lambda)) / 65536, each operation rounded once
__device__ __forceinline__ double gbt_step(const GbtParams& p, uint32_t H, int64_t G) {
  if (H == 0) return 0.0;
  const double t1 = (double)(-G) / ((double)H + p.lambda);
  const double t2 = p.eta * t1;
  return t2 / 65536.0;
}

// ---- prepare ---------------------------------------------------------------
// codes in both layouts (padding columns 0), z, pred = 0, both heaps absent
__global__ __launch_bounds__(GBT_NT) void k_gbt_prepare(GbtParams p, const double* __restrict__ X,
                                                        const double* __restrict__ y, uint8_t* __restrict__ rm,
                                                        uint8_t* __restrict__ fm, double* __restrict__ z,
                                                        double* __restrict__ pred, GbtNode* __restrict__ state,
                                                        int32_t* __restrict__ ctl) {
  const int64_t idx = (int64_t)blockIdx.x * GBT_NT + threadIdx.x;
  tree_codes(idx, p.n, p.d, p.d_pad, p.n_pad, X, rm, fm);
  if (idx < p.n) z[idx] = tree_norm(y[idx], p.y_shift, p.y_scale), pred[idx] = 0.0;
  const int64_t stride = (int64_t)gridDim.x * GBT_NT;
  for (int64_t k = idx; k < 2 * (int64_t)p.heap; k += stride) state[k] = GbtNode{};
  if (idx == 0) ctl[0] = 0, ctl[1] = -1;
}

// ---- a round's start; the tree before it joins the output --------------------
__global__ __launch_bounds__(GBT_NT) void k_gbt_round(GbtParams p, int32_t r, const double* __restrict__ z,
                                                      const double* __restrict__ pred, int32_t* __restrict__ g,
                                                      uint8_t* __restrict__ samp, int32_t* __restrict__ rows,
                                                      GbtNode* __restrict__ state,
                                                      const ut_tree_node* __restrict__ tn, ut_tree_node* __restrict__ out,
                                                      int32_t* __restrict__ roots, int32_t* __restrict__ ctl) {
  __shared__ uint32_t sH;
  __shared__ unsigned long long sG;
  __shared__ uint16_t rank[GBT_HEAP_MAX + 1];
  __shared__ int32_t wsum[4];
  if (r < p.n_rounds) {
    GbtNode* root = state + (int64_t)(r & 1) * p.heap;
    if (threadIdx.x == 0) sH = 0, sG = 0;
    __syncthreads();
    const int32_t i = blockIdx.x * GBT_NT + threadIdx.x;
    if (i < p.n) {
      double e = pred[i] - z[i];
      e = e < -64.0 ? -64.0 : (e > 64.0 ? 64.0 : e);
      const int32_t gi = (int32_t)nearbyint(e * 65536.0);
      const bool in = gbt_sampled(p, r, i);
      g[i] = gi, samp[i] = in ? 1 : 0, rows[i] = i;
      if (in) {
        atomicAdd(&sH, 1u);
        atomicAdd(&sG, (unsigned long long)(int64_t)gi);
      }
    }
    __syncthreads();
    if (threadIdx.x == 0) {
      if (sH) {
        atomicAdd(&root->H, sH);
        atomicAdd(&root->G, sG);
      }
      if (blockIdx.x == 0) root->start = 0, root->count = p.n, root->open = 1;
    }
  }
  if (blockIdx.x != 0 || r == 0) return;

  // tree r - 1: the live nodes in heap order behind the trees before it
  GbtNode* st = state + (int64_t)((r - 1) & 1) * p.heap;
  const ut_tree_node* rec = tn + (int64_t)((r - 1) & 1) * p.heap;
  const int32_t per = (p.heap + GBT_NT - 1) / GBT_NT;
  const int32_t k0 = min((int32_t)threadIdx.x * per, p.heap), k1 = min(k0 + per, p.heap);
  int32_t cnt = 0;
  for (int32_t k = k0; k < k1; ++k) cnt += st[k].open != 0;
  int32_t total;
  int32_t pos = tree_prefix(cnt, wsum, &total);
  for (int32_t k = k0; k < k1; ++k)
    if (st[k].open != 0) rank[k] = (uint16_t)pos++;
  const int32_t base = ctl[0];
  __syncthreads();
  for (int32_t k = k0; k < k1; ++k) {
    if (st[k].open != 0) {
      ut_tree_node v = rec[k];
      if (v.feature >= 0) v.left = base + rank[2 * k + 1], v.right = base + rank[2 * k + 2];
      if (base + rank[k] < p.out_cap) out[base + rank[k]] = v;
    }
    st[k] = GbtNode{};   // the heap of round r + 1
  }
  if (threadIdx.x == 0) roots[r - 1] = base, ctl[0] = base + total;
}

// ---- a level: histograms, the best split, the decision, the rows' move --------
struct GbtSide {
  uint32_t cnt, H;
  unsigned long long G;
};

__global__ __launch_bounds__(GBT_NT) void k_gbt_level(GbtParams p, int32_t r, int32_t level,
                                                      GbtNode* __restrict__ state, ut_tree_node* __restrict__ tn,
                                                      const int32_t* __restrict__ src, int32_t* __restrict__ dst,
                                                      const uint8_t* __restrict__ rm, const uint8_t* __restrict__ fm,
                                                      const int32_t* __restrict__ g, const uint8_t* __restrict__ samp,
                                                      double* __restrict__ pred, RfCand* __restrict__ cand,
                                                      int32_t* __restrict__ ctl) {
  __shared__ TreeHistLds lds;
  __shared__ int32_t s_last;
  __shared__ GbtSide side[2];
  const int32_t k = (1 << level) - 1 + (int32_t)blockIdx.y;
  GbtNode* nd = state + k;
  const int32_t open = nd->open;
  if (open != 1) return;
  const int32_t start = nd->start, count = nd->count;
  const uint32_t H = nd->H;
  const int64_t G = (int64_t)nd->G;
  const int32_t lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
  const int32_t* list = src + start;
  const uint32_t mc = (uint32_t)p.min_child;
  RfCand best{-1.0, p.d, 256};

  // a node at max_depth, or with too few sampled rows for two children, has no
  // candidates: its first slice decides it at once
  const bool search = level < p.max_depth && H >= 2u * mc;
  if (!search && blockIdx.x != 0) return;
  if (search) {
    const RfCand mine = tree_hist_best<true, true>(
        lds, list, count, rm, p.d, p.d_pad, p.nfb, (int32_t)blockIdx.x, (int32_t)gridDim.x, H, G, mc, p.lambda,
        [&](int32_t row) { return samp[row] ? TreeAdd{1u, (int64_t)g[row]} : TreeAdd{0u, 0}; },
        [&](int32_t j) { return gbt_eligible(p, r, level, j); });
    RfCand* cs = cand + (int64_t)blockIdx.y * gridDim.x;
    if (threadIdx.x == 0) {
      cs[blockIdx.x] = mine;
      // the release makes the candidate visible to whoever reads the count after
      // it, the acquire makes the others' visible here: the L2s are per XCD
      const int32_t t = __hip_atomic_fetch_add(&nd->ticket, 1, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
      s_last = t == (int32_t)gridDim.x - 1;
    }
    __syncthreads();
    if (!s_last) return;
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
    // the last ticket: the slices' candidates (at most GBT_WG = GBT_NT) in (s, j, b) order
    RfCand v{-1.0, p.d, 256};
    if (threadIdx.x < gridDim.x) v = cs[threadIdx.x];
#pragma unroll
    for (int32_t o = 32; o >= 1; o >>= 1) {
      const double s2 = __shfl_xor(v.s, o);
      const int32_t j2 = __shfl_xor(v.j, o), b2 = __shfl_xor(v.b, o);
      if (rf_better(s2, j2, b2, v.s, v.j, v.b)) v.s = s2, v.j = j2, v.b = b2;
    }
    // (wbest is free: its last read came before s_last's barrier)
    if (lane == 0) lds.wbest[wave] = v;
    __syncthreads();
    best = tree_wave_best(lds.wbest);
  }

  // the decision, the same in every thread
  const double step = gbt_step(p, H, G);
  bool split = false;
  if (best.s >= 0.0) {
    const double Gd = (double)G;
    const double parent = (Gd * Gd) / ((double)H + p.lambda);
    split = best.s - parent > p.gamma;
  }
  if (threadIdx.x == 0) {
    ut_tree_node v;
    v.feature = split ? best.j : -1, v.left = -1, v.right = -1, v.default_left = split ? 1 : 0;
    v.threshold = split ? (double)(best.b + 1) / 256.0 : 0.0;
    v.value = p.y_scale * step;
    tn[k] = v;
    nd->open = split ? 3 : 2;
    if (split) atomicMax(&ctl[1], best.j);
  }
  if (!split) {
    for (int32_t i = threadIdx.x; i < count; i += GBT_NT) {
      const int32_t row = list[i];
      pred[row] = pred[row] + step;
    }
    return;
  }

  // every row of the node goes to a child; the children's sums are over the sample
  if (threadIdx.x < 2) side[threadIdx.x] = GbtSide{0u, 0u, 0ull};
  __syncthreads();
  int32_t* to = dst + start;
  const uint8_t* col = fm + (int64_t)best.j * p.n_pad;
  uint32_t hl = 0, hr = 0;
  int64_t gl = 0, gr = 0;
  for (int32_t i = threadIdx.x; i < count; i += GBT_NT) {
    const int32_t row = list[i];
    const bool left = (int32_t)col[row] <= best.b;
    const bool in = samp[row] != 0;
    if (left) {
      to[atomicAdd(&side[0].cnt, 1u)] = row;
      if (in) hl += 1, gl += g[row];
    } else {
      to[count - 1 - (int32_t)atomicAdd(&side[1].cnt, 1u)] = row;
      if (in) hr += 1, gr += g[row];
    }
  }
  if (hl) atomicAdd(&side[0].H, hl), atomicAdd(&side[0].G, (unsigned long long)gl);
  if (hr) atomicAdd(&side[1].H, hr), atomicAdd(&side[1].G, (unsigned long long)gr);
  __syncthreads();
  if (threadIdx.x < 2) {
    GbtNode c{};
    c.start = start + (threadIdx.x ? (int32_t)side[0].cnt : 0);
    c.count = (int32_t)side[threadIdx.x].cnt;
    c.H = side[threadIdx.x].H, c.G = side[threadIdx.x].G, c.open = 1;
    state[2 * k + 1 + (int32_t)threadIdx.x] = c;
  }
}

// slice workgroups per node of level L
inline int32_t gbt_slices(int32_t level, int32_t nfb) {
  const int32_t want = (GBT_WG + (1 << level) - 1) >> level;
  return std::max(1, std::min(want, nfb));
}

}  // namespace ut

extern "C" int ut_gbt_fit(ut_ctx* c, const double* X_host, const double* y_host, int32_t n, int32_t d,
                          const ut_gbt_fit_params* fp) {
  using namespace ut;
  if (!c) return UT_EINVAL;
  if (int e = tree_fit_check(c, "gbt_fit", X_host, y_host, n, d, fp, [&]() -> int {
        UT_CHECK(c, fp->n_rounds >= 1 && fp->n_rounds <= 1024, UT_EINVAL, "gbt_fit: n_rounds must be in [1, 1024]");
        UT_CHECK(c, fp->max_depth >= 1 && fp->max_depth <= 12, UT_EINVAL, "gbt_fit: max_depth must be in [1, 12]");
        UT_CHECK(c, fp->min_child >= 1, UT_EINVAL, "gbt_fit: min_child must be at least 1");
        UT_CHECK(c, fp->eta > 0.0 && fp->eta <= 1.0, UT_EINVAL, "gbt_fit: eta must be in (0, 1]");
        UT_CHECK(c, fp->lambda >= 0.0 && __builtin_isfinite(fp->lambda), UT_EINVAL,
                 "gbt_fit: lambda must be finite and >= 0");
        UT_CHECK(c, fp->gamma >= 0.0 && __builtin_isfinite(fp->gamma), UT_EINVAL,
                 "gbt_fit: gamma must be finite and >= 0");
        UT_CHECK(c, fp->subsample > 0.0 && fp->subsample <= 1.0, UT_EINVAL, "gbt_fit: subsample must be in (0, 1]");
        UT_CHECK(c, fp->colsample_bylevel > 0.0 && fp->colsample_bylevel <= 1.0, UT_EINVAL,
                 "gbt_fit: colsample_bylevel must be in (0, 1]");
        return 0;
      }))
    return e;

  GbtParams p;
  p.n = n, p.d = d, p.n_rounds = fp->n_rounds, p.max_depth = fp->max_depth, p.min_child = fp->min_child;
  p.heap = (2 << p.max_depth) - 1;
  // a tree of k leaves has 2k - 1 nodes; a leaf below the root holds min_child sampled rows
  const int32_t leaves = std::min(1 << p.max_depth, std::max(1, n / p.min_child));
  p.out_cap = p.n_rounds * (2 * leaves - 1);
  p.eta = fp->eta, p.lambda = fp->lambda, p.gamma = fp->gamma, p.subsample = fp->subsample;
  p.colsample = fp->colsample_bylevel, p.y_shift = fp->y_shift, p.y_scale = fp->y_scale;
  p.seed = c->seed, p.round_ = fp->round_;
  const int32_t R = p.n_rounds, D = p.max_depth;

  // every allocation before anything of the loaded ensemble is touched
  if (int e = tree_fit_stage(c, X_host, y_host, n, d, &p.d_pad, &p.n_pad, &p.nfb)) return e;
  if (int e = ensure(c, c->rf_rows, (size_t)2 * n)) return e;
  if (int e = ensure(c, c->rf_cand, (size_t)GBT_WG + ((size_t)1 << D))) return e;   // 2^L x slices(L) <= max(256, 2^L)
  if (int e = ensure(c, c->gbt_z, (size_t)n)) return e;
  if (int e = ensure(c, c->gbt_pred, (size_t)n)) return e;
  if (int e = ensure(c, c->gbt_g, (size_t)n)) return e;
  if (int e = ensure(c, c->gbt_samp, (size_t)n)) return e;
  if (int e = ensure(c, c->gbt_state, (size_t)2 * p.heap)) return e;
  if (int e = ensure(c, c->gbt_tn, (size_t)2 * p.heap)) return e;
  if (int e = ensure(c, c->gbt_ctl, (size_t)2)) return e;
  DevBuf<int32_t> roots;
  if (int e = dalloc(c, roots, (size_t)R)) return e;
  DevBuf<ut_tree_node> grown;
  if (int e = dalloc(c, grown, (size_t)p.out_cap)) return e;

  hipStream_t s = c->stream;
  hipLaunchKernelGGL(k_gbt_prepare, dim3(grid1((int64_t)n * p.d_pad, GBT_NT)), dim3(GBT_NT), 0, s, p, c->rf_X.p,
                     c->rf_y.p, c->rf_rm.p, c->rf_fm.p, c->gbt_z.p, c->gbt_pred.p, c->gbt_state.p, c->gbt_ctl.p);
  UT_LAUNCH_CHECK(c);

  // rounds x (max_depth + 2) launches and one more, nothing read back between
  // them: every grid is known here
  int32_t* rows[2] = {c->rf_rows.p, c->rf_rows.p + n};
  for (int32_t r = 0; r <= R; ++r) {
    hipLaunchKernelGGL(k_gbt_round, dim3(r < R ? grid1(n, GBT_NT) : 1u), dim3(GBT_NT), 0, s, p, r, c->gbt_z.p,
                       c->gbt_pred.p, c->gbt_g.p, c->gbt_samp.p, rows[0], c->gbt_state.p, c->gbt_tn.p, grown.p, roots.p,
                       c->gbt_ctl.p);
    if (r == R) break;
    GbtNode* st = c->gbt_state.p + (size_t)(r & 1) * p.heap;
    ut_tree_node* tn = c->gbt_tn.p + (size_t)(r & 1) * p.heap;
    for (int32_t level = 0; level <= D; ++level) {
      const int32_t slices = level < D ? gbt_slices(level, p.nfb) : 1;
      hipLaunchKernelGGL(k_gbt_level, dim3(slices, 1u << level), dim3(GBT_NT), 0, s, p, r, level, st, tn,
                         rows[level & 1], rows[(level + 1) & 1], c->rf_rm.p, c->rf_fm.p, c->gbt_g.p, c->gbt_samp.p,
                         c->gbt_pred.p, c->rf_cand.p, c->gbt_ctl.p);
    }
    UT_LAUNCH_CHECK(c);
  }
  UT_LAUNCH_CHECK(c);

  UT_HIP(c, hipMemcpyAsync(c->rf_host, c->gbt_ctl.p, 2 * sizeof(int32_t), hipMemcpyDeviceToHost, s));
  UT_HIP(c, hipStreamSynchronize(s));
  const int32_t total = c->rf_host[0], max_feat = c->rf_host[1];
  UT_CHECK(c, total >= R && total <= p.out_cap, UT_EHIP, "gbt_fit: the trees' sizes are off");
  DevBuf<ut_tree_node> nodes;
  if (int e = dalloc(c, nodes, (size_t)total)) return e;
  UT_HIP(c, hipMemcpyAsync(nodes.p, grown.p, sizeof(ut_tree_node) * (size_t)total, hipMemcpyDeviceToDevice, s));
  return forest_install(c, nodes, total, roots, R, max_feat, p.y_shift, 1.0, 1.0);
}
