// tpe.hip -- the TPE surrogate (uthot.h states the model): ut_tpe_fit,
// ut_tpe_score, ut_tpe_get, ut_tpe_info.
//
// The fit is two launches behind the host's split of y:
//   k_tpe_fit_num  one workgroup per (numeric feature, set).  The set's s values
//                  of the column and the prior centre go to LDS (8192 doubles,
//                  64 KiB: the cap on a set), padded with +inf to a power of two
//                  and sorted by a bitonic network.  A lane then takes a centre:
//                  its two gaps, the clip, Z from two fp64 erf, and writes mu,
//                  sigma, ln(w / Z) for ut_tpe_get and the packed (mu, A, B) in
//                  both tiers' record formats.
//   k_tpe_fit_cat  one workgroup per categorical column: integer counts of the
//                  rows that read 1, per set, reduced by LDS integer atomics,
//                  then the log-probabilities.
//
// The scoring kernel, k_tpe_score<T>, is bound by VALU issue: one exp2 and five
// full-rate operations per (candidate, numeric feature, component); DESIGN has
// its time against the bare exp2 issue rate.  Its split of the work:
//   * a workgroup of 4 waves owns a tile of 1024 candidates for the whole call;
//     a lane holds R = 4 of them (tile index lane + 256 r, so every load of a
//     feature row is coalesced), so one component read feeds four terms;
//   * the loop runs over items = (numeric feature, chunk of <= 1024 components).
//     A chunk is one LDS stage (16 KiB of f32 records, 24 KiB of fp64 ones),
//     and there are two: while an item's arithmetic runs from one stage, the
//     next item's records sit in registers (4 or 6 x 16 B per lane, loaded
//     before the arithmetic), and go to the other stage after it.  One barrier
//     per item.  A feature with more components than a stage is several items
//     of the same loop;
//   * a component is wave-uniform: every lane reads the same record, a
//     broadcast LDS read (one ds_read_b128 per f32 record), no bank conflict;
//   * per term: d = x - mu in fp64, rounded to the tier; t = d d; e = fma(A, t,
//     B); the sum += exp2(e).  Two running sums per candidate and feature (l's
//     components come first in a feature's table, then g's); at a feature's
//     last item log l - log g joins the fp64 accumulators;
//   * the categorical columns follow, read straight from the feature rows.
// T = double is the same code with the device library's exp2: the reference tier.
#include "ut_internal.h"

#include <algorithm>
#include <numeric>

namespace ut {

constexpr int32_t TPE_NT = 256;
constexpr int32_t TPE_R = 4;                     // candidates per lane
constexpr int32_t TPE_TILE = TPE_NT * TPE_R;     // candidates per workgroup
constexpr int32_t TPE_CH = 1024;                 // components per LDS stage
constexpr int32_t TPE_SET_MAX = 8191;            // rows of one set: its centres and the prior fill the sort's LDS
constexpr int32_t TPE_SORT = TPE_SET_MAX + 1;

struct TpeShape {
  int32_t n, d, nl, ng, dnum, ncat, cpad;
  double pw;
};

// ---- fit: numeric features -------------------------------------------------
__global__ __launch_bounds__(TPE_NT) void k_tpe_fit_num(TpeShape p, const double* __restrict__ X,
                                                        const int32_t* __restrict__ rows,
                                                        const int32_t* __restrict__ numcol, double* __restrict__ mu,
                                                        double* __restrict__ sig, double* __restrict__ lw,
                                                        TpeRec32* __restrict__ t32, TpeRec64* __restrict__ t64) {
  __shared__ double v[TPE_SORT];
  const int32_t k = blockIdx.x, set = blockIdx.y, tid = threadIdx.x;
  const int32_t s = set ? p.ng : p.nl, cnt = s + 1;
  const int32_t* rs = rows + (set ? p.nl : 0);
  const int32_t col = numcol[k];
  int32_t P2 = 2;
  while (P2 < cnt) P2 <<= 1;   // cnt <= TPE_SORT, a power of two
  for (int32_t i = tid; i < P2; i += TPE_NT)
    v[i] = i < s ? X[(int64_t)rs[i] * p.d + col] : (i == s ? 0.5 : (double)INFINITY);
  __syncthreads();
  for (int32_t kk = 2; kk <= P2; kk <<= 1)
    for (int32_t j = kk >> 1; j > 0; j >>= 1) {
      for (int32_t i = tid; i < P2; i += TPE_NT) {
        const int32_t o = i ^ j;
        if (o > i) {
          const double a = v[i], b = v[o];
          if ((a > b) == ((i & kk) == 0)) v[i] = b, v[o] = a;
        }
      }
      __syncthreads();
    }
  // the prior is the first of the centres equal to 0.5: as many centres lie below it
  int32_t lo = 0, hi = cnt;
  while (lo < hi) {
    const int32_t mid = (lo + hi) >> 1;
    if (v[mid] < 0.5) lo = mid + 1;
    else hi = mid;
  }
  const int32_t prior = lo;
  const double floor_ = 1.0 / (double)min(100, s + 2);
  const int64_t out = (int64_t)k * p.cpad + (set ? p.nl + 1 : 0);
  for (int32_t i = tid; i < cnt; i += TPE_NT) {
    const double m = v[i];
    double sg = 1.0;
    if (i != prior) {
      const double gl = i > 0 ? m - v[i - 1] : 0.0, gr = i + 1 < cnt ? v[i + 1] - m : 0.0;
      sg = gl > gr ? gl : gr;
      sg = sg < floor_ ? floor_ : (sg > 1.0 ? 1.0 : sg);
    }
    const double w = (i == prior ? p.pw : 1.0) / ((double)s + p.pw);
    const double r2 = sg * 1.4142135623730951;
    const double Z = 0.5 * (erf((1.0 - m) / r2) - erf(-m / r2));
    const double wz = w / Z;
    const double A = -1.4426950408889634 / ((2.0 * sg) * sg);
    const double B = log2(wz / (sg * 2.5066282746310002));
    mu[out + i] = m, sig[out + i] = sg, lw[out + i] = log(wz);
    t64[out + i] = TpeRec64{m, A, B};
    t32[out + i] = TpeRec32{m, (float)A, (float)B};
  }
  // the padding record of an odd component count is staged with the others and never summed
  if (set == 1 && tid == 0 && p.cpad > p.n + 2) {
    const int64_t o = (int64_t)k * p.cpad + p.n + 2;
    mu[o] = 0.0, sig[o] = 0.0, lw[o] = 0.0;
    t64[o] = TpeRec64{0.0, 0.0, 0.0};
    t32[o] = TpeRec32{0.0, 0.0f, 0.0f};
  }
}

// ---- fit: categorical columns ------------------------------------------------
// log((c + pw / q) / (s + pw)); a probability above 1/2 through log1p of its
// exact complement, so that its rounding does not show in a log near 0
__device__ __forceinline__ double tpe_logp(double c, double s, double pw, double q) {
  const double num = c + pw / q, den = s + pw;
  return 2.0 * num > den ? log1p(-((den - num) / den)) : log(num / den);
}

__global__ __launch_bounds__(TPE_NT) void k_tpe_fit_cat(TpeShape p, const double* __restrict__ X,
                                                        const int32_t* __restrict__ rows,
                                                        TpeCat* __restrict__ cat) {
  __shared__ int32_t ones[2];
  const int32_t tid = threadIdx.x;
  if (tid < 2) ones[tid] = 0;
  __syncthreads();
  const int32_t col = cat[blockIdx.x].col, q = cat[blockIdx.x].q;
  int32_t c[2] = {0, 0};
  for (int32_t i = tid; i < p.n; i += TPE_NT) c[i >= p.nl] += X[(int64_t)rows[i] * p.d + col] != 0.0 ? 1 : 0;
  if (c[0]) atomicAdd(&ones[0], c[0]);
  if (c[1]) atomicAdd(&ones[1], c[1]);
  __syncthreads();
  if (tid == 0) {
    const double cl = (double)ones[0], cg = (double)ones[1], sl = (double)p.nl, sg = (double)p.ng;
    TpeCat r;
    r.col = col, r.q = q;
    if (q == 1) {   // BOOL: the categories are the values 0 and 1
      r.l0 = tpe_logp(sl - cl, sl, p.pw, 2.0), r.l1 = tpe_logp(cl, sl, p.pw, 2.0);
      r.g0 = tpe_logp(sg - cg, sg, p.pw, 2.0), r.g1 = tpe_logp(cg, sg, p.pw, 2.0);
    } else {
      r.l0 = 0.0, r.l1 = tpe_logp(cl, sl, p.pw, (double)q);
      r.g0 = 0.0, r.g1 = tpe_logp(cg, sg, p.pw, (double)q);
    }
    cat[blockIdx.x] = r;
  }
}

// ---- score ---------------------------------------------------------------------
template <class T>
struct TpeTier;
template <>
struct TpeTier<float> {
  using Rec = TpeRec32;
  static __device__ __forceinline__ float term(double x, const Rec& c) {
    const float d = (float)(x - c.mu);
    return __builtin_amdgcn_exp2f(__builtin_fmaf(c.A, d * d, c.B));
  }
};
template <>
struct TpeTier<double> {
  using Rec = TpeRec64;
  static __device__ __forceinline__ double term(double x, const Rec& c) {
    const double d = x - c.mu;
    return exp2(__builtin_fma(c.A, d * d, c.B));
  }
};

template <class T>
__global__ __launch_bounds__(TPE_NT) void k_tpe_score(TpeShape p, const typename TpeTier<T>::Rec* __restrict__ tab,
                                                      const int32_t* __restrict__ numcol,
                                                      const TpeCat* __restrict__ cat,
                                                      const double* __restrict__ feat, int64_t ld, int64_t m,
                                                      const uint8_t* __restrict__ dup, double* __restrict__ score,
                                                      double* __restrict__ logl, double* __restrict__ logg) {
  using Rec = typename TpeTier<T>::Rec;
  constexpr int32_t UNITS = TPE_CH * (int32_t)sizeof(Rec) / 16 / TPE_NT;   // 16-byte units a lane moves per stage
  static_assert(UNITS * 16 * TPE_NT == TPE_CH * (int32_t)sizeof(Rec), "a stage is whole 16-byte units per lane");
  __shared__ __attribute__((aligned(16))) Rec stage[2][TPE_CH];
  const int32_t tid = threadIdx.x;
  const int64_t i0 = (int64_t)blockIdx.x * TPE_TILE + tid;
  const int32_t C = p.n + 2, nl1 = p.nl + 1;
  const int32_t nch = (C + TPE_CH - 1) / TPE_CH, items = p.dnum * nch;
  double sc[TPE_R], ll[TPE_R], lg[TPE_R], x[TPE_R];
  T al[TPE_R], ag[TPE_R];
#pragma unroll
  for (int32_t r = 0; r < TPE_R; ++r) sc[r] = 0.0, ll[r] = 0.0, lg[r] = 0.0, x[r] = 0.5, al[r] = 0, ag[r] = 0;

  uint4 pre[UNITS];
  // item -> registers: the records [c0, c0 + TPE_CH) of its feature, as far as
  // the (even) row goes; the rest of the stage gets zeros
#define TPE_FETCH(item)                                                                              \
  do {                                                                                               \
    const int32_t fk = (item) / nch, fc0 = ((item) % nch) * TPE_CH;                                  \
    const uint4* src = reinterpret_cast<const uint4*>(tab + (int64_t)fk * p.cpad + fc0);            \
    const int32_t units = min(TPE_CH, p.cpad - fc0) * (int32_t)sizeof(Rec) / 16;                    \
    _Pragma("unroll") for (int32_t u = 0; u < UNITS; ++u) {                                          \
      const int32_t idx = tid + u * TPE_NT;                                                          \
      pre[u] = idx < units ? src[idx] : uint4{0u, 0u, 0u, 0u};                                       \
    }                                                                                                \
  } while (0)
#define TPE_PUT(buf)                                                                                 \
  do {                                                                                               \
    uint4* dst = reinterpret_cast<uint4*>(&stage[(buf)][0]);                                         \
    _Pragma("unroll") for (int32_t u = 0; u < UNITS; ++u) dst[tid + u * TPE_NT] = pre[u];           \
  } while (0)

  if (items > 0) {
    TPE_FETCH(0);
    TPE_PUT(0);
  }
  __syncthreads();
  for (int32_t item = 0; item < items; ++item) {
    const int32_t k = item / nch, j = item % nch;
    const int32_t c0 = j * TPE_CH, c1 = min(C, c0 + TPE_CH);
    if (j == 0) {
      const double* row = feat + (int64_t)numcol[k] * ld;
#pragma unroll
      for (int32_t r = 0; r < TPE_R; ++r) {
        const int64_t i = i0 + (int64_t)r * TPE_NT;
        x[r] = i < m ? row[i] : 0.5;
        al[r] = 0, ag[r] = 0;
      }
    }
    if (item + 1 < items) TPE_FETCH(item + 1);
    const Rec* st = stage[item & 1];
    const int32_t le = min(c1, nl1) - c0, gb = max(c0, nl1) - c0, ge = c1 - c0;
#pragma unroll 2
    for (int32_t c = 0; c < le; ++c) {
      const Rec rec = st[c];
#pragma unroll
      for (int32_t r = 0; r < TPE_R; ++r) al[r] += TpeTier<T>::term(x[r], rec);
    }
#pragma unroll 2
    for (int32_t c = gb; c < ge; ++c) {
      const Rec rec = st[c];
#pragma unroll
      for (int32_t r = 0; r < TPE_R; ++r) ag[r] += TpeTier<T>::term(x[r], rec);
    }
    if (item + 1 < items) TPE_PUT((item + 1) & 1);
    __syncthreads();
    if (j == nch - 1) {
#pragma unroll
      for (int32_t r = 0; r < TPE_R; ++r) {
        const double a = log((double)al[r]), b = log((double)ag[r]);
        ll[r] += a, lg[r] += b, sc[r] += a - b;
      }
    }
  }
#undef TPE_FETCH
#undef TPE_PUT

  for (int32_t q = 0; q < p.ncat; ++q) {
    const TpeCat cr = cat[q];
    const double* row = feat + (int64_t)cr.col * ld;
#pragma unroll
    for (int32_t r = 0; r < TPE_R; ++r) {
      const int64_t i = i0 + (int64_t)r * TPE_NT;
      const double xv = i < m ? row[i] : 0.0;
      const double a = xv == 0.0 ? cr.l0 : xv * cr.l1, b = xv == 0.0 ? cr.g0 : xv * cr.g1;
      ll[r] += a, lg[r] += b, sc[r] += a - b;
    }
  }
#pragma unroll
  for (int32_t r = 0; r < TPE_R; ++r) {
    const int64_t i = i0 + (int64_t)r * TPE_NT;
    if (i >= m) continue;
    score[i] = dup && dup[i] ? -(double)INFINITY : sc[r];
    if (logl) logl[i] = ll[r];
    if (logg) logg[i] = lg[r];
  }
}

}  // namespace ut

extern "C" int ut_tpe_fit(ut_ctx* c, const double* X, const double* y, int32_t n, int32_t d, const int32_t* kinds,
                          const ut_tpe_params* tp) {
  using namespace ut;
  if (!c) return UT_EINVAL;
  UT_CHECK(c, X && y && tp, UT_EINVAL, "tpe_fit: X, y or the parameters are NULL");
  UT_CHECK(c, n >= 2 && d >= 1 && d <= 4096, UT_EINVAL, "tpe_fit: n must be at least 2 and d in [1, 4096]");
  UT_CHECK(c, tp->gamma > 0.0 && tp->gamma < 1.0, UT_EINVAL, "tpe_fit: gamma must be in (0, 1)");
  UT_CHECK(c, tp->n_good_max >= 1, UT_EINVAL, "tpe_fit: n_good_max must be at least 1");
  UT_CHECK(c, __builtin_isfinite(tp->prior_weight) && tp->prior_weight > 0.0, UT_EINVAL,
           "tpe_fit: prior_weight must be finite and positive");
  UT_CHECK(c, tp->precision == 32 || tp->precision == 64, UT_EINVAL, "tpe_fit: precision must be 32 or 64");
  for (int32_t i = 0; i < n; ++i)
    UT_CHECK(c, __builtin_isfinite(y[i]), UT_EINVAL, "tpe_fit: y[" + std::to_string(i) + "] is not finite");
  const int32_t nl =
      std::max(1, (int32_t)std::min<double>(std::ceil(tp->gamma * (double)n), std::min(tp->n_good_max, n - 1)));
  const int32_t ng = n - nl;
  UT_CHECK(c, nl <= TPE_SET_MAX && ng <= TPE_SET_MAX, UT_EINVAL,
           "tpe_fit: a set of " + std::to_string(std::max(nl, ng)) + " rows is above the cap of " +
               std::to_string(TPE_SET_MAX) + " (one workgroup sorts a set in LDS)");

  // the columns: numeric index or categorical record of each
  std::vector<int32_t> kv(d, 0), slot(d, -1), numcol;
  std::vector<TpeCat> cats;
  if (kinds) kv.assign(kinds, kinds + d);
  for (int32_t j = 0; j < d;) {
    const int32_t q = kv[j];
    UT_CHECK(c, q >= 0, UT_EINVAL, "tpe_fit: kinds[" + std::to_string(j) + "] continues no block");
    if (q == 0) {
      slot[j] = (int32_t)numcol.size();
      numcol.push_back(j);
      ++j;
      continue;
    }
    const int32_t width = q == 1 ? 1 : q;
    UT_CHECK(c, j + width <= d, UT_EINVAL, "tpe_fit: the block at kinds[" + std::to_string(j) + "] passes d");
    for (int32_t t = 0; t < width; ++t) {
      UT_CHECK(c, t == 0 || kv[j + t] == -1, UT_EINVAL,
               "tpe_fit: kinds[" + std::to_string(j + t) + "] must be -1 inside the block at " + std::to_string(j));
      slot[j + t] = (int32_t)cats.size();
      cats.push_back(TpeCat{j + t, q, 0.0, 0.0, 0.0, 0.0});
    }
    j += width;
  }
  // the training values
  for (int32_t i = 0; i < n; ++i) {
    const double* row = X + (size_t)i * d;
    for (int32_t j = 0; j < d; ++j) {
      const int32_t q = kv[j];
      if (q == 0) {
        UT_CHECK(c, row[j] >= 0.0 && row[j] <= 1.0, UT_EINVAL,
                 "tpe_fit: X[" + std::to_string(i) + "][" + std::to_string(j) + "] is outside [0, 1]");
      } else if (q >= 1) {
        int32_t ones = 0;
        bool ok = true;
        for (int32_t t = 0; t < (q == 1 ? 1 : q); ++t) {
          ok = ok && (row[j + t] == 0.0 || row[j + t] == 1.0);
          ones += row[j + t] == 1.0;
        }
        UT_CHECK(c, ok && (q == 1 || ones == 1), UT_EINVAL,
                 "tpe_fit: row " + std::to_string(i) + " of the block at column " + std::to_string(j) +
                     (q == 1 ? " is not 0 or 1" : " is not one-hot"));
      }
    }
  }
  // the split: the nl smallest y, ties to the earlier row; each set in row order
  std::vector<int32_t> order(n);
  std::iota(order.begin(), order.end(), 0);
  std::stable_sort(order.begin(), order.end(), [&](int32_t a, int32_t b) { return y[a] < y[b]; });
  std::vector<uint8_t> good(n, 0);
  for (int32_t i = 0; i < nl; ++i) good[order[i]] = 1;
  std::vector<int32_t> st;
  st.reserve((size_t)n + numcol.size());
  for (int32_t i = 0; i < n; ++i)
    if (good[i]) st.push_back(i);
  for (int32_t i = 0; i < n; ++i)
    if (!good[i]) st.push_back(i);
  st.insert(st.end(), numcol.begin(), numcol.end());

  TpeShape p;
  p.n = n, p.d = d, p.nl = nl, p.ng = ng, p.dnum = (int32_t)numcol.size(), p.ncat = (int32_t)cats.size();
  p.cpad = (n + 2 + 1) / 2 * 2;
  p.pw = tp->prior_weight;
  const size_t tab = (size_t)p.dnum * p.cpad;

  UT_HIP(c, hipSetDevice(c->device));
  c->tpe_valid = false;   // from here a failure leaves no fit
  if (int e = ensure(c, c->tpe_X, (size_t)n * d)) return e;
  if (int e = ensure(c, c->tpe_rows, (size_t)n)) return e;
  if (int e = ensure(c, c->tpe_numcol, numcol.size())) return e;
  if (int e = ensure(c, c->tpe_mu, tab)) return e;
  if (int e = ensure(c, c->tpe_sig, tab)) return e;
  if (int e = ensure(c, c->tpe_lw, tab)) return e;
  if (int e = ensure(c, c->tpe_t32, tab)) return e;
  if (int e = ensure(c, c->tpe_t64, tab)) return e;
  if (int e = ensure(c, c->tpe_cat, cats.size())) return e;

  // X, st and cats are pageable: such a host-to-device copy has read its source
  // when the call returns (gp_fit.hip and gp_lml.hip rely on the same), so the
  // caller's X and these locals need not outlive this function
  hipStream_t s = c->stream;
  UT_HIP(c, hipMemcpyAsync(c->tpe_X.p, X, sizeof(double) * (size_t)n * d, hipMemcpyHostToDevice, s));
  UT_HIP(c, hipMemcpyAsync(c->tpe_rows.p, st.data(), sizeof(int32_t) * (size_t)n, hipMemcpyHostToDevice, s));
  if (p.dnum)
    UT_HIP(c, hipMemcpyAsync(c->tpe_numcol.p, st.data() + n, sizeof(int32_t) * (size_t)p.dnum,
                             hipMemcpyHostToDevice, s));
  if (p.ncat)
    UT_HIP(c, hipMemcpyAsync(c->tpe_cat.p, cats.data(), sizeof(TpeCat) * (size_t)p.ncat,
                             hipMemcpyHostToDevice, s));
  if (p.dnum)
    hipLaunchKernelGGL(k_tpe_fit_num, dim3(p.dnum, 2), dim3(TPE_NT), 0, s, p, c->tpe_X.p, c->tpe_rows.p,
                       c->tpe_numcol.p, c->tpe_mu.p, c->tpe_sig.p, c->tpe_lw.p, c->tpe_t32.p, c->tpe_t64.p);
  if (p.ncat)
    hipLaunchKernelGGL(k_tpe_fit_cat, dim3(p.ncat), dim3(TPE_NT), 0, s, p, c->tpe_X.p, c->tpe_rows.p, c->tpe_cat.p);
  UT_LAUNCH_CHECK(c);

  c->tpe_d = d, c->tpe_dnum = p.dnum, c->tpe_ncat = p.ncat, c->tpe_nl = nl, c->tpe_ng = ng, c->tpe_cpad = p.cpad;
  c->tpe_par = *tp;
  c->tpe_kinds.swap(kv);
  c->tpe_slot.swap(slot);
  c->tpe_valid = true;
  return 0;
}

extern "C" int ut_tpe_score(ut_ctx* c, const double* features, int64_t ld, int64_t m, int32_t d, const uint8_t* dup,
                            double* score, double* logl, double* logg) {
  using namespace ut;
  if (!c) return UT_EINVAL;
  UT_CHECK(c, c->tpe_valid, UT_EINVAL, "tpe_score: no TPE fit is loaded (ut_tpe_fit)");
  UT_CHECK(c, d == c->tpe_d, UT_EINVAL,
           "tpe_score: " + std::to_string(d) + " features, the fit has " + std::to_string(c->tpe_d));
  UT_CHECK(c, m >= 0 && ld >= m, UT_EINVAL, "tpe_score: m must be >= 0 and ld >= m");
  if (m == 0) return 0;
  UT_CHECK(c, features && score, UT_EINVAL, "tpe_score: features or score is NULL");
  UT_CHECK(c, (m + TPE_TILE - 1) / TPE_TILE <= 0x7fffffff, UT_EINVAL, "tpe_score: m is too large");
  UT_HIP(c, hipSetDevice(c->device));
  TpeShape p;
  p.n = c->tpe_nl + c->tpe_ng, p.d = d, p.nl = c->tpe_nl, p.ng = c->tpe_ng, p.dnum = c->tpe_dnum;
  p.ncat = c->tpe_ncat, p.cpad = c->tpe_cpad, p.pw = c->tpe_par.prior_weight;
  const dim3 grid(grid1(m, TPE_TILE));
  if (c->tpe_par.precision == 64)
    hipLaunchKernelGGL(k_tpe_score<double>, grid, dim3(TPE_NT), 0, c->stream, p, c->tpe_t64.p, c->tpe_numcol.p,
                       c->tpe_cat.p, features, ld, m, dup, score, logl, logg);
  else
    hipLaunchKernelGGL(k_tpe_score<float>, grid, dim3(TPE_NT), 0, c->stream, p, c->tpe_t32.p, c->tpe_numcol.p,
                       c->tpe_cat.p, features, ld, m, dup, score, logl, logg);
  UT_LAUNCH_CHECK(c);
  return 0;
}

extern "C" int ut_tpe_get(ut_ctx* c, int32_t feature, int32_t set, double* mu, double* sigma, double* logw,
                          int32_t cap, int32_t* count) {
  using namespace ut;
  if (!c) return UT_EINVAL;
  UT_CHECK(c, c->tpe_valid, UT_EINVAL, "tpe_get: no TPE fit is loaded (ut_tpe_fit)");
  UT_CHECK(c, count && feature >= 0 && feature < c->tpe_d && (set == 0 || set == 1), UT_EINVAL,
           "tpe_get: feature must be a column of the fit, set 0 or 1, count not NULL");
  const int32_t kind = c->tpe_kinds[feature], sl = c->tpe_slot[feature];
  UT_CHECK(c, kind >= 0, UT_EINVAL, "tpe_get: column " + std::to_string(feature) + " lies inside a one-hot block");
  const int32_t s = set ? c->tpe_ng : c->tpe_nl;
  *count = kind == 0 ? s + 1 : (kind == 1 ? 2 : kind);
  if (!mu && !sigma && !logw) return 0;
  UT_CHECK(c, cap >= *count, UT_EINVAL, "tpe_get: cap is below the count");
  UT_HIP(c, hipSetDevice(c->device));
  if (kind == 0) {
    const size_t off = (size_t)sl * c->tpe_cpad + (set ? c->tpe_nl + 1 : 0), bytes = sizeof(double) * (size_t)*count;
    if (mu) UT_HIP(c, hipMemcpyAsync(mu, c->tpe_mu.p + off, bytes, hipMemcpyDeviceToHost, c->stream));
    if (sigma) UT_HIP(c, hipMemcpyAsync(sigma, c->tpe_sig.p + off, bytes, hipMemcpyDeviceToHost, c->stream));
    if (logw) UT_HIP(c, hipMemcpyAsync(logw, c->tpe_lw.p + off, bytes, hipMemcpyDeviceToHost, c->stream));
    UT_HIP(c, hipStreamSynchronize(c->stream));
    return 0;
  }
  std::vector<TpeCat> rec(kind == 1 ? 1 : kind);
  UT_HIP(c, hipMemcpyAsync(rec.data(), c->tpe_cat.p + sl, sizeof(TpeCat) * rec.size(), hipMemcpyDeviceToHost,
                           c->stream));
  UT_HIP(c, hipStreamSynchronize(c->stream));
  for (int32_t t = 0; t < *count; ++t) {
    const TpeCat& r = rec[kind == 1 ? 0 : t];
    if (mu) mu[t] = (double)t;
    if (sigma) sigma[t] = 0.0;
    if (logw) logw[t] = kind == 1 ? (t ? (set ? r.g1 : r.l1) : (set ? r.g0 : r.l0)) : (set ? r.g1 : r.l1);
  }
  return 0;
}

extern "C" int ut_tpe_info(ut_ctx* c, int32_t* n_l, int32_t* n_g, int32_t* d, ut_tpe_params* params) {
  if (!c) return UT_EINVAL;
  UT_CHECK(c, c->tpe_valid, UT_EINVAL, "tpe_info: no TPE fit is loaded (ut_tpe_fit)");
  if (n_l) *n_l = c->tpe_nl;
  if (n_g) *n_g = c->tpe_ng;
  if (d) *d = c->tpe_d;
  if (params) *params = c->tpe_par;
  return 0;
}
