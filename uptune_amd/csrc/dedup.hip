// dedup.hip -- history membership + in-batch first-occurrence dedup.
//
// Reference semantics (one SQL round trip per candidate today):
//   SearchDriver.get_configuration / has_results   driver.py:157-158,253-258
//   Configuration.get (by program, hash)           resultsdb/models.py:126-135
//   ParallelTuning.unique -> GlobalResult.get      api.py:254-280, globalmodels.py:38-45
// A candidate is a duplicate when its hash_config digest is already in the
// results history, or when an earlier candidate (smaller global index) of
// the same batch has the same digest.
//
// History: open-addressing table of 32-byte keys (linear probing, home slot
// = first digest word, which is uniformly distributed).  Batch: table of
// candidate indices; equal digests converge on one slot whose value ends as
// the minimum index (atomicMin), so the surviving index does not depend on
// scheduling.  Bound: latency/HBM (one 32-byte read per probe).
#include "ut_internal.h"

namespace ut {

__device__ __forceinline__ bool key_eq(const uint32_t* a, const uint32_t* b) {
  const uint4* x = reinterpret_cast<const uint4*>(a);
  const uint4* y = reinterpret_cast<const uint4*>(b);
  const uint4 x0 = x[0], x1 = x[1], y0 = y[0], y1 = y[1];
  return x0.x == y0.x && x0.y == y0.y && x0.z == y0.z && x0.w == y0.w && x1.x == y1.x && x1.y == y1.y &&
         x1.z == y1.z && x1.w == y1.w;
}

__global__ void k_hist_insert(uint32_t* __restrict__ keys, uint32_t* __restrict__ state, int64_t cap,
                              const uint32_t* __restrict__ dig, int64_t n) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= n) return;
  const uint32_t* d = dig + j * 8;
  uint64_t h = d[0] & (uint64_t)(cap - 1);
  for (int64_t probe = 0; probe < cap; ++probe) {
    if (atomicCAS(&state[h], 0u, 1u) == 0u) {
      for (int w = 0; w < 8; ++w) keys[h * 8 + w] = d[w];
      return;
    }
    h = (h + 1) & (uint64_t)(cap - 1);
  }
}

// gate (both batch kernels): a lazy round's remainder, skipped when *gate == 0
__global__ void k_batch_insert(const uint32_t* __restrict__ dig, int64_t m, int32_t* __restrict__ slots,
                               int64_t cap, const int32_t* __restrict__ gate) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m || (gate && *gate == 0)) return;
  const uint32_t* d = dig + i * 8;
  uint64_t h = d[0] & (uint64_t)(cap - 1);
  for (int64_t probe = 0; probe < cap; ++probe) {
    const int32_t cur = atomicCAS(&slots[h], -1, (int32_t)i);
    if (cur == -1) return;
    if (key_eq(dig + (int64_t)cur * 8, d)) {
      atomicMin(&slots[h], (int32_t)i);
      return;
    }
    h = (h + 1) & (uint64_t)(cap - 1);
  }
}

__global__ void k_dedup_mark(const uint32_t* __restrict__ dig, int64_t m, const int32_t* __restrict__ slots,
                             int64_t cap, const uint32_t* __restrict__ hkeys, const uint32_t* __restrict__ hstate,
                             int64_t hcap, uint8_t* __restrict__ dup, const int32_t* __restrict__ gate) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m || (gate && *gate == 0)) return;
  const uint32_t* d = dig + i * 8;
  bool is_dup = false;
  if (hcap > 0) {
    uint64_t h = d[0] & (uint64_t)(hcap - 1);
    for (int64_t probe = 0; probe < hcap; ++probe) {
      if (hstate[h] == 0u) break;
      if (key_eq(hkeys + h * 8, d)) {
        is_dup = true;
        break;
      }
      h = (h + 1) & (uint64_t)(hcap - 1);
    }
  }
  if (!is_dup) {
    uint64_t h = d[0] & (uint64_t)(cap - 1);
    for (int64_t probe = 0; probe < cap; ++probe) {
      const int32_t cur = slots[h];
      if (cur == -1) break;  // unreachable: our own insert claimed a slot on this path
      if (key_eq(dig + (int64_t)cur * 8, d)) {
        is_dup = (cur != (int32_t)i);
        break;
      }
      h = (h + 1) & (uint64_t)(cap - 1);
    }
  }
  dup[i] = is_dup ? 1 : 0;
}

// re-insert every occupied slot of an old table (capacity growth)
__global__ void k_hist_rehash(const uint32_t* __restrict__ okeys, const uint32_t* __restrict__ ostate, int64_t ocap,
                              uint32_t* __restrict__ keys, uint32_t* __restrict__ state, int64_t cap) {
  const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (j >= ocap || ostate[j] == 0u) return;
  const uint32_t* d = okeys + j * 8;
  uint64_t h = d[0] & (uint64_t)(cap - 1);
  for (int64_t probe = 0; probe < cap; ++probe) {
    if (atomicCAS(&state[h], 0u, 1u) == 0u) {
      for (int w = 0; w < 8; ++w) keys[h * 8 + w] = d[w];
      return;
    }
    h = (h + 1) & (uint64_t)(cap - 1);
  }
}

int launch_hist_rehash(ut_ctx* c, const uint32_t* okeys, const uint32_t* ostate, int64_t ocap, uint32_t* keys,
                       uint32_t* state, int64_t cap) {
  if (ocap <= 0) return 0;
  hipLaunchKernelGGL(k_hist_rehash, dim3(grid1(ocap, 256)), dim3(256), 0, c->stream, okeys, ostate, ocap, keys,
                     state, cap);
  UT_LAUNCH_CHECK(c);
  return 0;
}

int launch_hist_insert(ut_ctx* c, const uint32_t* dig, int64_t n) {
  if (n <= 0) return 0;
  hipLaunchKernelGGL(k_hist_insert, dim3(grid1(n, 256)), dim3(256), 0, c->stream, c->hist_keys.p, c->hist_state.p,
                     c->hist_cap, dig, n);
  UT_LAUNCH_CHECK(c);
  return 0;
}

// dst[i] |= src[i] (a GA round's invalid children join its duplicates)
__global__ void k_mask_or(uint8_t* __restrict__ dst, const uint8_t* __restrict__ src, int64_t m) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i < m && src[i]) dst[i] = 1;
}

int launch_mask_or(ut_ctx* c, uint8_t* dst, const uint8_t* src, int64_t m) {
  if (m <= 0) return 0;
  hipLaunchKernelGGL(k_mask_or, dim3(grid1(m, 256)), dim3(256), 0, c->stream, dst, src, m);
  UT_LAUNCH_CHECK(c);
  return 0;
}

// ---------------------------------------------------------------------------
// Lazy rounds: dedup + compaction of the score-sorted prefix (kp <= 1024
// entries, one workgroup, thread p = prefix entry p).  The batch table lives
// in LDS: a digest's slot is claimed by whichever of its entries comes first
// (cls), and the slot's `best` ends as the smallest candidate index among
// them (atomicMin), so the surviving entry does not depend on scheduling.
// The entries that are neither in the history nor behind a smaller index keep
// their prefix order; the first k of them are the round's selections.
// ---------------------------------------------------------------------------
constexpr int PFX_NT = 1024;
constexpr int PFX_CAP = 2048;   // table slots: twice the entries

__global__ __launch_bounds__(PFX_NT) void k_prefix_dedup(
    const int64_t* __restrict__ idx, const double* __restrict__ score, const uint32_t* __restrict__ dig,
    const double* __restrict__ vals, int32_t NC, int32_t kp, int64_t cand_base, const uint32_t* __restrict__ hkeys,
    const uint32_t* __restrict__ hstate, int64_t hcap, int32_t k, int64_t* __restrict__ out_idx,
    double* __restrict__ out_score, double* __restrict__ out_vals, uint32_t* __restrict__ out_dig,
    int32_t* __restrict__ gate, int64_t* __restrict__ nfall) {
  __shared__ int32_t cls[PFX_CAP];    // slot -> the prefix entry that claimed it, -1 = empty
  __shared__ int32_t best[PFX_CAP];   // slot -> smallest candidate index (local) with its digest
  __shared__ int32_t wkeep[PFX_NT / 64], wvalid[PFX_NT / 64];
  const int p = threadIdx.x;
  for (int e = p; e < PFX_CAP; e += PFX_NT) {
    cls[e] = -1;
    best[e] = 0x7FFFFFFF;
  }
  __syncthreads();
  const int64_t g = p < kp ? idx[p] : -1;
  const bool valid = g >= 0;
  const int32_t li = valid ? (int32_t)(g - cand_base) : 0;
  const uint32_t* d = dig + (int64_t)(p < kp ? p : 0) * 8;
  int32_t slot = -1;
  if (valid) {
    uint32_t h = d[0] & (PFX_CAP - 1);
    for (int probe = 0; probe < PFX_CAP; ++probe) {
      const int32_t cur = atomicCAS(&cls[h], -1, p);
      if (cur == -1 || cur == p || key_eq(dig + (int64_t)cur * 8, d)) {
        slot = (int32_t)h;
        break;
      }
      h = (h + 1) & (PFX_CAP - 1);
    }
    if (slot >= 0) atomicMin(&best[slot], li);
  }
  __syncthreads();
  bool keep = valid && slot >= 0 && best[slot] == li;
  if (keep && hcap > 0) {   // the history probe of k_dedup_mark
    uint64_t h = d[0] & (uint64_t)(hcap - 1);
    for (int64_t probe = 0; probe < hcap; ++probe) {
      if (hstate[h] == 0u) break;
      if (key_eq(hkeys + h * 8, d)) {
        keep = false;
        break;
      }
      h = (h + 1) & (uint64_t)(hcap - 1);
    }
  }
  // rank among the kept entries, in prefix order
  const int lane = p & 63, w = p >> 6;
  const unsigned long long bk = __ballot(keep), bv = __ballot(valid);
  if (lane == 0) {
    wkeep[w] = __builtin_popcountll(bk);
    wvalid[w] = __builtin_popcountll(bv);
  }
  __syncthreads();
  int32_t rank = __builtin_popcountll(bk & ((1ull << lane) - 1ull)), total = 0, nvalid = 0;
  for (int q = 0; q < PFX_NT / 64; ++q) {
    if (q < w) rank += wkeep[q];
    total += wkeep[q];
    nvalid += wvalid[q];
  }
  if (keep && rank < k) {
    out_idx[rank] = g;
    out_score[rank] = score[p];
    for (int32_t col = 0; col < NC; ++col) out_vals[(int64_t)col * k + rank] = vals[(int64_t)col * kp + p];
    for (int q = 0; q < 8; ++q) out_dig[(int64_t)rank * 8 + q] = d[q];
  }
  // fewer than k: empty slots as the row gather writes them; their score is
  // that of the prefix's own empty entry at the slot, -inf (a duplicate's
  // masked score) where the prefix holds a candidate
  for (int32_t j = total + p; j < k; j += PFX_NT) {
    out_idx[j] = -1;
    out_score[j] = (j < kp && idx[j] < 0) ? score[j] : -1.0 / 0.0;
    for (int32_t col = 0; col < NC; ++col) out_vals[(int64_t)col * k + j] = 0.0;
    for (int q = 0; q < 8; ++q) out_dig[(int64_t)j * 8 + q] = 0u;
  }
  if (p == 0) {
    // candidates beyond the prefix exist only if every prefix entry is one
    const int32_t need = (total < k && nvalid == kp) ? 1 : 0;
    *gate = need;
    if (need) *nfall += 1;
  }
}

int launch_prefix_dedup(ut_ctx* c, const int64_t* idx, const double* score, const uint32_t* dig, const double* vals,
                        int32_t kp, int64_t cand_base, int32_t k, int64_t* out_idx, double* out_score,
                        double* out_vals, uint32_t* out_dig, int32_t* gate, int64_t* nfall) {
  UT_CHECK(c, kp >= 1 && kp <= PFX_NT && k >= 1 && k <= kp, UT_EINVAL, "prefix dedup: 1 <= k <= prefix <= 1024");
  hipLaunchKernelGGL(k_prefix_dedup, dim3(1), dim3(PFX_NT), 0, c->stream, idx, score, dig, vals, c->space.ncols, kp,
                     cand_base, c->hist_keys.p, c->hist_state.p, c->hist_cap, k, out_idx, out_score, out_vals, out_dig,
                     gate, nfall);
  UT_LAUNCH_CHECK(c);
  return 0;
}

__global__ void k_mask_score(double* __restrict__ score, const uint8_t* __restrict__ dup, int64_t m,
                             const int32_t* __restrict__ gate) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m || (gate && *gate == 0)) return;
  if (dup[i]) score[i] = -1.0 / 0.0;
}

int launch_mask_score(ut_ctx* c, double* score, const uint8_t* dup, int64_t m) {
  if (m <= 0) return 0;
  hipLaunchKernelGGL(k_mask_score, dim3(grid1(m, 256)), dim3(256), 0, c->stream, score, dup, m, c->round_gate);
  UT_LAUNCH_CHECK(c);
  return 0;
}

int launch_dedup(ut_ctx* c, const uint32_t* dig, int64_t m, uint8_t* dup) {
  if (m <= 0) return 0;
  int64_t cap = 1024;
  while (cap < 2 * m) cap <<= 1;
  UT_CHECK(c, m < (int64_t)0x7FFFFFFF, UT_EINVAL, "dedup batch must be < 2^31 candidates");
  if ((int64_t)c->batch_slots.n < cap) {
    if (c->batch_slots.p) UT_HIP(c, ut::sync_all(c));
    // no table until the new one exists: a failed growth leaves none, so the
    // next call allocates again
    c->batch_slots.reset();
    if (int rc = ut::dalloc(c, c->batch_slots, (size_t)cap)) return rc;
  }
  UT_HIP(c, hipMemsetAsync(c->batch_slots.p, 0xFF, cap * sizeof(int32_t), c->stream));
  hipLaunchKernelGGL(k_batch_insert, dim3(grid1(m, 256)), dim3(256), 0, c->stream, dig, m, c->batch_slots.p, cap,
                     c->round_gate);
  UT_LAUNCH_CHECK(c);
  hipLaunchKernelGGL(k_dedup_mark, dim3(grid1(m, 256)), dim3(256), 0, c->stream, dig, m, c->batch_slots.p, cap,
                     c->hist_keys.p, c->hist_state.p, c->hist_cap, dup, c->round_gate);
  UT_LAUNCH_CHECK(c);
  return 0;
}

}  // namespace ut
