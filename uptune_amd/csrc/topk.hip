// topk.hip -- deterministic top-k: the k largest scores, ties broken by the
// smallest global candidate index, duplicates and NaN scores never selected.
// (= Python sorted(range(m), key=lambda i: (-s[i], i))[:k] over the valid
// candidates)
//
// Each 256-thread workgroup bitonic-sorts a 2048-entry chunk in LDS
// ((score, index) pairs, index -1 = invalid) and keeps its best k; passes
// repeat on the survivors until one chunk remains.  k <= 1024.
// A re-merge pass (mode 1) reads whole sorted lists of k from the pass before;
// for a power-of-two k it loads every odd list reversed, which makes the chunk
// the state of the network after its level-k stage, and starts at level 2k
// (k = 256: 30 compare-exchange phases instead of 66).
#include "ut_internal.h"

namespace ut {

constexpr int TK_CH = 2048;
constexpr int TK_NT = 256;

__device__ __forceinline__ bool better(double sa, int64_t ia, double sb, int64_t ib) {
  if (ia < 0) return false;
  if (ib < 0) return true;
  if (sa != sb) return sa > sb;
  return ia < ib;
}

// mode 0: input = raw scores (+ dup mask), index = cand_base + position
// mode 1: input = (score, index) pairs, sorted lists of k from a previous pass
// mode 2: input = (score, index) pairs in any order
template <int MODE>
__global__ __launch_bounds__(TK_NT) void k_topk_chunk(const double* __restrict__ in_s,
                                                      const int64_t* __restrict__ in_i,
                                                      const uint8_t* __restrict__ dup, int64_t count,
                                                      int64_t cand_base, int32_t k, double* __restrict__ out_s,
                                                      int64_t* __restrict__ out_i,
                                                      const int32_t* __restrict__ gate) {
  __shared__ double ss[TK_CH];
  __shared__ int64_t si[TK_CH];
  if (gate && *gate == 0) return;   // a lazy round's remainder that is not needed (the whole grid returns)
  const int t = threadIdx.x;
  const int64_t base = (int64_t)blockIdx.x * TK_CH;
  // mode 1, k a power of two: the chunk holds 2048 / k sorted lists (best
  // first; invalid entries last, whole padding lists invalid)
  const bool runs = MODE == 1 && (k & (k - 1)) == 0 && k >= 2;
  for (int e = t; e < TK_CH; e += TK_NT) {
    // odd lists enter reversed: alternating best-first / worst-first runs are
    // exactly the network's state after its size-k level
    const int src = (runs && ((e / k) & 1)) ? (e / k) * k + (k - 1 - e % k) : e;
    const int64_t p = base + src;
    double s = 0.0;
    int64_t ix = -1;
    if (p < count) {
      s = in_s[p];
      if (MODE == 0) {
        ix = (dup && dup[p]) ? -1 : cand_base + p;
      } else {
        ix = in_i[p];
      }
      if (ix < 0) ix = -1;
      if (s != s) ix = -1;  // NaN never selected
    }
    ss[e] = s;
    si[e] = ix;
  }
  for (int size = runs ? 2 * k : 2; size <= TK_CH; size <<= 1) {
    for (int stride = size >> 1; stride > 0; stride >>= 1) {
      __syncthreads();
      for (int q = t; q < TK_CH / 2; q += TK_NT) {
        const int lo = 2 * stride * (q / stride) + (q % stride);
        const int hi = lo + stride;
        const bool up = (lo & size) == 0;  // this run wants best first
        const double a = ss[lo], b = ss[hi];
        const int64_t ia = si[lo], ib = si[hi];
        const bool swap = up ? better(b, ib, a, ia) : better(a, ia, b, ib);
        if (swap) {
          ss[lo] = b; ss[hi] = a;
          si[lo] = ib; si[hi] = ia;
        }
      }
    }
  }
  __syncthreads();
  for (int e = t; e < k; e += TK_NT) {
    out_s[(int64_t)blockIdx.x * k + e] = ss[e];
    out_i[(int64_t)blockIdx.x * k + e] = si[e];
  }
}

// the top-k of explicit (score, index) pairs (index -1 = invalid), ties broken
// by the smallest index: the re-merge passes from the start
int topk_pairs_impl(ut_ctx* c, const double* score, const int64_t* idx, int64_t n, int32_t k, int64_t* out_idx,
                    double* out_score) {
  UT_CHECK(c, k >= 1 && k <= TK_CH / 2, UT_EINVAL, "topk: k must be in [1, 1024]");
  int64_t count = n < 1 ? 1 : n;
  int64_t chunks = (count + TK_CH - 1) / TK_CH;
  int rc;
  if ((rc = ensure(c, c->tk_score[0], (size_t)chunks * k))) return rc;
  if ((rc = ensure(c, c->tk_idx[0], (size_t)chunks * k))) return rc;
  if ((rc = ensure(c, c->tk_score[1], (size_t)chunks * k))) return rc;
  if ((rc = ensure(c, c->tk_idx[1], (size_t)chunks * k))) return rc;
  // first pass: whole network (the input is not made of sorted lists)
  hipLaunchKernelGGL(k_topk_chunk<2>, dim3((unsigned)chunks), dim3(TK_NT), 0, c->stream, score, idx, nullptr, n, 0, k,
                     c->tk_score[0].p, c->tk_idx[0].p, nullptr);
  UT_LAUNCH_CHECK(c);
  int cur = 0;
  count = chunks * k;
  while (chunks > 1) {
    chunks = (count + TK_CH - 1) / TK_CH;
    hipLaunchKernelGGL(k_topk_chunk<1>, dim3((unsigned)chunks), dim3(TK_NT), 0, c->stream, c->tk_score[cur].p,
                       c->tk_idx[cur].p, nullptr, count, 0, k, c->tk_score[cur ^ 1].p, c->tk_idx[cur ^ 1].p,
                       nullptr);
    UT_LAUNCH_CHECK(c);
    cur ^= 1;
    count = chunks * k;
  }
  if (out_idx)
    UT_HIP(c, hipMemcpyAsync(out_idx, c->tk_idx[cur].p, sizeof(int64_t) * k, hipMemcpyDeviceToDevice, c->stream));
  if (out_score)
    UT_HIP(c, hipMemcpyAsync(out_score, c->tk_score[cur].p, sizeof(double) * k, hipMemcpyDeviceToDevice,
                             c->stream));
  return 0;
}

// ---------------------------------------------------------------------------
// Large m: top-k by threshold selection.  The tournament above is a chain of
// dependent sorts (six launches, 115 + 5 x 30 us at m = 2^20, k = 512);
// here radix passes over an order-preserving 64-bit key find the k-th largest
// key, the candidates above it (and, of its tie class, the ones with the
// smallest positions) are collected in any order, and one k_topk_chunk<2> sorts
// them: ordering, ties, NaN and the -1 padding stay defined by that kernel.
//
// A pass histograms one digit of the keys that match the prefix found so far
// (LDS histogram per workgroup, non-empty bins added to the global one); the
// last workgroup to arrive (ticket after __threadfence) scans the bins from
// the top, extends the prefix by the bin where the running count reaches what
// is still wanted, and clears the histogram and the ticket for the next pass.
// No kernel waits for another workgroup.  Once everything at or above the
// prefix fits the sort's chunk, `done` is set and the later passes and the tie
// count return at once.  If the last pass ends with a tie class that does not
// fit, k_sel_ties counts each workgroup's ties and k_sel_collect takes those
// whose rank by position (ties of earlier workgroups + earlier ties of this
// one) is below the number wanted: exactly the (-score, index) order.
// ---------------------------------------------------------------------------
constexpr int SEL_NT = 256;
constexpr int SEL_SEG = 4096;     // scores per workgroup, contiguous (16 per thread)
constexpr int SEL_IT = SEL_SEG / SEL_NT;
constexpr int SEL_BINS = 8192;    // 13-bit digits
constexpr int SEL_PASSES = 5;     // 13 + 13 + 13 + 13 + 12 bits
__host__ __device__ constexpr int sel_shift(int pass) { return pass < 4 ? 51 - 13 * pass : 0; }
__host__ __device__ constexpr int sel_width(int pass) { return pass < 4 ? 13 : 12; }

// the selection's device state, behind the global histogram in ctx.tk_sel; the
// histogram and the ticket are zero between kernels (tk_sel is cleared when it
// is allocated, every picker clears what its pass used)
struct SelState {
  uint64_t thr;      // the prefix found so far, as a key with its low bits zero
  uint32_t ticket;   // workgroups that have added their histogram
  uint32_t nsurv;    // survivors collected
  uint32_t done;     // every key >= thr fits one chunk: collect them all
  uint32_t above;    // keys above the prefix's bin, summed over the passes
  uint32_t need;     // still wanted from the prefix's bin (after the last pass: ties wanted)
  uint32_t pad;
};
constexpr size_t SEL_STATE_WORDS = SEL_BINS + sizeof(SelState) / sizeof(uint32_t);

// position p's key: larger score = larger key, -0.0 = +0.0, +-inf ordinary;
// false for the never-selected (NaN, duplicates)
__device__ __forceinline__ bool sel_key(double s, uint8_t dup, uint64_t& key) {
  uint64_t b = (uint64_t)__double_as_longlong(s);
  if ((b << 1) == 0) b = 0;
  key = (b >> 63) ? ~b : (b | 0x8000000000000000ull);
  return s == s && !dup;
}

// a thread's SEL_IT scores and mask bytes of its workgroup's segment, every
// load issued before the first use (between the LDS atomics of the loops
// below the compiler waits for each load in turn); NaN past the end
struct SelVals {
  double s[SEL_IT];
  uint8_t d[SEL_IT];
};
__device__ __forceinline__ void sel_load(const double* __restrict__ score, const uint8_t* __restrict__ dup, int64_t m,
                                         int64_t base, int t, SelVals& v) {
  // (unconditional loads at clamped positions: a branch per load would wait per load)
#pragma unroll
  for (int j = 0; j < SEL_IT; ++j) {
    const int64_t p = base + j * SEL_NT + t;
    v.s[j] = score[p < m ? p : m - 1];
  }
  if (dup) {
#pragma unroll
    for (int j = 0; j < SEL_IT; ++j) {
      const int64_t p = base + j * SEL_NT + t;
      v.d[j] = dup[p < m ? p : m - 1];
    }
  } else {
#pragma unroll
    for (int j = 0; j < SEL_IT; ++j) v.d[j] = 0;
  }
#pragma unroll
  for (int j = 0; j < SEL_IT; ++j)
    if (base + j * SEL_NT + t >= m) v.s[j] = __longlong_as_double(0x7FF8000000000000ll);
}

template <int PASS>
__global__ __launch_bounds__(SEL_NT) void k_sel_pass(const double* __restrict__ score,
                                                     const uint8_t* __restrict__ dup, int64_t m, int32_t k,
                                                     uint32_t* __restrict__ hist, SelState* __restrict__ st,
                                                     double* __restrict__ surv_s, int64_t* __restrict__ surv_i) {
  constexpr int SH = sel_shift(PASS), NB = 1 << sel_width(PASS), BPT = NB / SEL_NT;
  __shared__ uint32_t lh[NB];
  __shared__ uint32_t part[SEL_NT];
  __shared__ uint32_t s_last;
  const int t = threadIdx.x, lane = t & 63;
  uint64_t prefix = 0;   // the key bits above this pass's digit
  if (PASS > 0) {
    if (st->done) return;
    prefix = st->thr >> sel_shift(PASS > 0 ? PASS - 1 : 0);
  }
  for (int b = t; b < NB; b += SEL_NT) lh[b] = 0u;
  if (PASS == 0 && blockIdx.x == 0) {
    // the sort's input: invalid wherever the collection does not write
    for (int e = t; e < TK_CH; e += SEL_NT) {
      surv_s[e] = 0.0;
      surv_i[e] = -1;
    }
    if (t == 0) st->nsurv = 0u;
  }
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * SEL_SEG;
  SelVals sv;
  sel_load(score, dup, m, base, t, sv);
#pragma unroll
  for (int j = 0; j < SEL_IT; ++j) {
    uint64_t key;
    bool ok = sel_key(sv.s[j], sv.d[j], key);
    if (PASS > 0) ok = ok && (key >> sel_shift(PASS > 0 ? PASS - 1 : 0)) == prefix;
    const uint32_t d = ok ? (uint32_t)(key >> SH) & (uint32_t)(NB - 1) : 0u;
    // a wave whose lanes agree adds its count once (equal scores: a million
    // atomics on one bin would serialise)
    const uint64_t mask = __ballot(ok);
    if (mask) {
      const int leader = __ffsll((unsigned long long)mask) - 1;
      const uint32_t d0 = (uint32_t)__shfl((int)d, leader, 64);
      if (__ballot(ok && d != d0) == 0) {
        if (lane == leader) atomicAdd(&lh[d0], (uint32_t)__popcll(mask));
      } else if (ok) {
        atomicAdd(&lh[d], 1u);
      }
    }
  }
  __syncthreads();
  for (int b = t; b < NB; b += SEL_NT) {
    const uint32_t v = lh[b];
    if (v) atomicAdd(&hist[b], v);
  }
  __threadfence();
  __syncthreads();
  if (t == 0) s_last = atomicAdd(&st->ticket, 1u) == gridDim.x - 1 ? 1u : 0u;
  __syncthreads();
  if (!s_last) return;
  __threadfence();
  // the picker: thread t owns the bins NB-1 - BPT t downwards
  // (all of a thread's loads in flight at once: one after the other they were
  // 30 us of L2 round trips per pass)
  uint32_t hv[BPT];
#pragma unroll
  for (int q = 0; q < BPT; ++q)
    hv[q] = __hip_atomic_load(&hist[NB - 1 - (t * BPT + q)], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  uint32_t sum = 0;
#pragma unroll
  for (int q = 0; q < BPT; ++q) {
    const int b = NB - 1 - (t * BPT + q);
    hist[b] = 0u;
    lh[b] = hv[q];
    sum += hv[q];
  }
  // (read before the scan's barriers: the one thread that picks the bin
  // rewrites them after the last barrier)
  const uint32_t need = PASS == 0 ? (uint32_t)k : st->need;
  const uint32_t above = PASS == 0 ? 0u : st->above;
  part[t] = sum;
  __syncthreads();
  for (int d = 1; d < SEL_NT; d <<= 1) {
    const uint32_t v = t >= d ? part[t - d] : 0u;
    __syncthreads();
    part[t] += v;
    __syncthreads();
  }
  const uint32_t incl = part[t], excl = incl - sum, total = part[SEL_NT - 1];
  const bool reached = excl < need && need <= incl;
  // fewer valid keys than wanted (only possible in pass 0, k <= TK_CH / 2): the
  // lowest bin, so that everything is collected
  const bool none = total < need && t == 0;
  if (!reached && !none) return;
  int bin = 0;
  uint32_t before = total - lh[0];
  if (reached) {
    uint32_t c = excl;
    for (int q = 0; q < BPT; ++q) {
      const int b = NB - 1 - (t * BPT + q);
      if (c + lh[b] >= need) {
        bin = b;
        before = c;
        break;
      }
      c += lh[b];
    }
  }
  st->thr = ((prefix << sel_width(PASS)) | (uint64_t)bin) << SH;
  st->above = above + before;
  st->need = need > before ? need - before : 0u;
  st->done = (uint64_t)above + before + lh[bin] <= (uint64_t)TK_CH ? 1u : 0u;
  st->ticket = 0u;
}

// the tie class did not fit: each workgroup's count of keys equal to thr
__global__ __launch_bounds__(SEL_NT) void k_sel_ties(const double* __restrict__ score, const uint8_t* __restrict__ dup,
                                                     int64_t m, const SelState* __restrict__ st,
                                                     uint32_t* __restrict__ wcnt) {
  __shared__ uint32_t s_cnt;
  if (st->done) return;
  const int t = threadIdx.x;
  const uint64_t thr = st->thr;
  if (t == 0) s_cnt = 0u;
  __syncthreads();
  const int64_t base = (int64_t)blockIdx.x * SEL_SEG;
  uint32_t cnt = 0;   // wave-uniform
  SelVals sv;
  sel_load(score, dup, m, base, t, sv);
#pragma unroll
  for (int j = 0; j < SEL_IT; ++j) {
    uint64_t key;
    const bool tie = sel_key(sv.s[j], sv.d[j], key) && key == thr;
    cnt += (uint32_t)__popcll(__ballot(tie));
  }
  if ((t & 63) == 0 && cnt) atomicAdd(&s_cnt, cnt);
  __syncthreads();
  if (t == 0) wcnt[blockIdx.x] = s_cnt;
}

// survivors: every key above thr, and of the keys equal to it all (done) or
// the first `need` by position; appended in any order, one atomic per wave
__global__ __launch_bounds__(SEL_NT) void k_sel_collect(const double* __restrict__ score,
                                                        const uint8_t* __restrict__ dup, int64_t m,
                                                        int64_t cand_base, SelState* __restrict__ st,
                                                        const uint32_t* __restrict__ wcnt,
                                                        double* __restrict__ surv_s, int64_t* __restrict__ surv_i) {
  __shared__ uint32_t wc[SEL_IT * (SEL_NT / 64) + 1];
  __shared__ unsigned long long s_rank;
  const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
  const bool all_ties = st->done != 0u;
  const uint64_t thr = st->thr;
  const uint64_t need = st->need;
  const int64_t base = (int64_t)blockIdx.x * SEL_SEG;
  SelVals sv;
  sel_load(score, dup, m, base, t, sv);
  if (!all_ties) {
    if (t == 0) s_rank = 0ull;
    __syncthreads();
    // ties in the workgroups before this one
    unsigned long long r = 0;
    for (int64_t w = t; w < (int64_t)blockIdx.x; w += SEL_NT) r += wcnt[w];
    if (r) atomicAdd(&s_rank, r);
    // ties of this one, per (iteration, wave) in position order
#pragma unroll
    for (int j = 0; j < SEL_IT; ++j) {
      uint64_t key;
      const bool tie = sel_key(sv.s[j], sv.d[j], key) && key == thr;
      const uint64_t mask = __ballot(tie);
      if (lane == 0) wc[j * (SEL_NT / 64) + wave] = (uint32_t)__popcll(mask);
    }
    __syncthreads();
    if (t == 0) {
      uint32_t c = 0;
      for (int q = 0; q < SEL_IT * (SEL_NT / 64); ++q) {
        const uint32_t v = wc[q];
        wc[q] = c;
        c += v;
      }
    }
    __syncthreads();
  }
  const uint64_t rank0 = all_ties ? 0ull : (uint64_t)s_rank;
#pragma unroll
  for (int j = 0; j < SEL_IT; ++j) {
    const int64_t p = base + j * SEL_NT + t;
    const double s = sv.s[j];
    uint64_t key;
    const bool ok = sel_key(s, sv.d[j], key);
    const bool tie = ok && key == thr;
    bool take = ok && key > thr;
    if (all_ties) {
      take = take || tie;
    } else {
      const uint64_t tmask = __ballot(tie);
      const uint64_t rank = rank0 + wc[j * (SEL_NT / 64) + wave] + (uint64_t)__popcll(tmask & ((1ull << lane) - 1ull));
      take = take || (tie && rank < need);
    }
    const uint64_t mask = __ballot(take);
    if (mask) {
      const int leader = __ffsll((unsigned long long)mask) - 1;
      uint32_t pos = 0;
      if (lane == leader) pos = atomicAdd(&st->nsurv, (uint32_t)__popcll(mask));
      pos = (uint32_t)__shfl((int)pos, leader, 64) + (uint32_t)__popcll(mask & ((1ull << lane) - 1ull));
      if (take && pos < (uint32_t)TK_CH) {   // (by construction at most TK_CH are taken)
        surv_s[pos] = s;
        surv_i[pos] = cand_base + p;
      }
    }
  }
}

// launches of the tournament for this shape
static int tournament_launches(int64_t m, int32_t k) {
  int64_t chunks = (m + TK_CH - 1) / TK_CH;
  int n = 1;
  while (chunks > 1) {
    chunks = (chunks * k + TK_CH - 1) / TK_CH;
    ++n;
  }
  return n;
}

// The selection takes over where the tournament needs more than
// SEL_MIN_TOURNAMENT launches (measured hand-over: profiles/tail_select.json).
// UT_TOPK_SELECT=0 keeps the tournament everywhere, =1 selects at every size.
constexpr int SEL_MIN_TOURNAMENT = 2;

static int topk_select(ut_ctx* c, const double* score, const uint8_t* dup, int64_t m, int64_t cand_base, int32_t k,
                       int64_t* out_idx, double* out_score) {
  const int64_t segs = (m + SEL_SEG - 1) / SEL_SEG;
  int rc;
  if (!c->tk_sel.p) {
    if ((rc = ensure(c, c->tk_sel, SEL_STATE_WORDS))) return rc;
    UT_HIP(c, hipMemsetAsync(c->tk_sel.p, 0, sizeof(uint32_t) * SEL_STATE_WORDS, c->stream));
  }
  if ((rc = ensure(c, c->tk_wcnt, (size_t)segs))) return rc;
  if ((rc = ensure(c, c->tk_score[0], (size_t)TK_CH))) return rc;
  if ((rc = ensure(c, c->tk_idx[0], (size_t)TK_CH))) return rc;
  if ((rc = ensure(c, c->tk_score[1], (size_t)k))) return rc;
  if ((rc = ensure(c, c->tk_idx[1], (size_t)k))) return rc;
  uint32_t* hist = c->tk_sel.p;
  SelState* st = reinterpret_cast<SelState*>(c->tk_sel.p + SEL_BINS);
  double* ss = c->tk_score[0].p;
  int64_t* si = c->tk_idx[0].p;
  const dim3 grid((unsigned)segs), block(SEL_NT);
#define UT_SEL_PASS(P)                                                                                        \
  hipLaunchKernelGGL(k_sel_pass<P>, grid, block, 0, c->stream, score, dup, m, k, hist, st, ss, si);          \
  UT_LAUNCH_CHECK(c);
  UT_SEL_PASS(0) UT_SEL_PASS(1) UT_SEL_PASS(2) UT_SEL_PASS(3) UT_SEL_PASS(4)
#undef UT_SEL_PASS
  static_assert(SEL_PASSES == 5, "one launch per digit");
  hipLaunchKernelGGL(k_sel_ties, grid, block, 0, c->stream, score, dup, m, st, c->tk_wcnt.p);
  UT_LAUNCH_CHECK(c);
  hipLaunchKernelGGL(k_sel_collect, grid, block, 0, c->stream, score, dup, m, cand_base, st, c->tk_wcnt.p, ss, si);
  UT_LAUNCH_CHECK(c);
  // the one sort; it writes the caller's arrays itself when both are wanted
  const bool direct = out_idx && out_score;
  hipLaunchKernelGGL(k_topk_chunk<2>, dim3(1), dim3(TK_NT), 0, c->stream, ss, si, nullptr, (int64_t)TK_CH, 0, k,
                     direct ? out_score : c->tk_score[1].p, direct ? out_idx : c->tk_idx[1].p, nullptr);
  UT_LAUNCH_CHECK(c);
  if (direct) return 0;
  if (out_idx)
    UT_HIP(c, hipMemcpyAsync(out_idx, c->tk_idx[1].p, sizeof(int64_t) * k, hipMemcpyDeviceToDevice, c->stream));
  if (out_score)
    UT_HIP(c, hipMemcpyAsync(out_score, c->tk_score[1].p, sizeof(double) * k, hipMemcpyDeviceToDevice, c->stream));
  return 0;
}

int topk_impl(ut_ctx* c, const double* score, const uint8_t* dup, int64_t m, int64_t cand_base, int32_t k,
              int64_t* out_idx, double* out_score) {
  UT_CHECK(c, k >= 1 && k <= TK_CH / 2, UT_EINVAL, "topk: k must be in [1, 1024]");
  UT_CHECK(c, m >= 0, UT_EINVAL, "topk: m < 0");
  // (gated calls keep the tournament: its passes are no-ops under a closed
  // gate, and no more launches than before; counts are 32-bit in the selection)
  if (!c->round_gate && m < ((int64_t)1 << 31)) {
    const int mode = c->topk_select;   // UT_TOPK_SELECT
    if (mode > 0 || (mode < 0 && tournament_launches(m, k) > SEL_MIN_TOURNAMENT))
      if (m > 0) return topk_select(c, score, dup, m, cand_base, k, out_idx, out_score);
  }
  int64_t chunks = (m + TK_CH - 1) / TK_CH;
  if (chunks < 1) chunks = 1;
  int rc;
  if ((rc = ensure(c, c->tk_score[0], (size_t)chunks * k))) return rc;
  if ((rc = ensure(c, c->tk_idx[0], (size_t)chunks * k))) return rc;
  if ((rc = ensure(c, c->tk_score[1], (size_t)chunks * k))) return rc;
  if ((rc = ensure(c, c->tk_idx[1], (size_t)chunks * k))) return rc;
  // gated (a lazy round's remainder, c->round_gate): every pass returns at
  // once when the gate is 0, and the last pass writes the caller's arrays
  // itself -- a copy after it would overwrite them whatever the gate says
  const int32_t* gate = c->round_gate;
  UT_CHECK(c, !gate || (out_idx && out_score), UT_EINVAL, "topk: a gated call writes both outputs");
  hipLaunchKernelGGL(k_topk_chunk<0>, dim3((unsigned)chunks), dim3(TK_NT), 0, c->stream, score, nullptr, dup, m,
                     cand_base, k, gate && chunks == 1 ? out_score : c->tk_score[0].p,
                     gate && chunks == 1 ? out_idx : c->tk_idx[0].p, gate);
  UT_LAUNCH_CHECK(c);
  int cur = 0;
  int64_t count = chunks * k;
  while (chunks > 1) {
    chunks = (count + TK_CH - 1) / TK_CH;
    hipLaunchKernelGGL(k_topk_chunk<1>, dim3((unsigned)chunks), dim3(TK_NT), 0, c->stream, c->tk_score[cur].p,
                       c->tk_idx[cur].p, nullptr, count, 0, k, gate && chunks == 1 ? out_score : c->tk_score[cur ^ 1].p,
                       gate && chunks == 1 ? out_idx : c->tk_idx[cur ^ 1].p, gate);
    UT_LAUNCH_CHECK(c);
    cur ^= 1;
    count = chunks * k;
  }
  if (gate) return 0;
  if (out_idx)
    UT_HIP(c, hipMemcpyAsync(out_idx, c->tk_idx[cur].p, sizeof(int64_t) * k, hipMemcpyDeviceToDevice, c->stream));
  if (out_score)
    UT_HIP(c, hipMemcpyAsync(out_score, c->tk_score[cur].p, sizeof(double) * k, hipMemcpyDeviceToDevice,
                             c->stream));
  return 0;
}

}  // namespace ut
