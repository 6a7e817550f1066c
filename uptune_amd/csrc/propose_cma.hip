// propose_cma.hip -- correlated-Gaussian proposals (ut_propose_cma; the rule is
// stated in include/uthot.h and restated in numpy by tests/_cma_oracle.py).
//
// Candidate i is x = mean + sigma * A z with z ~ N(0, I): a [dn x dn] x [dn x m]
// product whose right operand does not exist anywhere -- every z is a
// counter-based normal draw of (candidate, feature).  The choices:
//
//   * The product runs on v_mfma_f64_16x16x4 with the FEATURES j on the
//     accumulator's rows and 16 CANDIDATES on its columns (the lane-fast axis):
//         D[j][cand] += A[j][k] * z[k][cand]
//     MFMA operand A is the factor (lane l: row j = l & 15, k = l >> 4), read
//     from LDS; operand B is z (lane l: k = l >> 4, candidate l & 15), which the
//     lane DRAWS: the 64 lanes of a wave draw the 64 distinct (k, candidate)
//     elements of a k4 step, so no normal is drawn twice and Z never touches
//     LDS or HBM.  A lane's accumulator rows all belong to its own candidate
//     l & 15, so the epilogue's SoA column store of a 16-candidate group is one
//     contiguous 128-byte piece per lane group.
//   * The factor sits in LDS once per workgroup, transposed and zero-padded:
//     sA[k][j], k padded to 4, the row stride to 32 doubles (dn = 128: 128 KiB
//     of the CU's 160 KiB), with column j stored at j ^ ((k & 1) << 4) so the
//     four k rows of one operand read fall on both halves of the banks.  No
//     padded k draws a normal (its z is 0 and its sA row is 0), and no padded j
//     is written.
//   * Workgroups are persistent: 8 waves, each a 16-candidate group of a
//     128-candidate tile, tiles strided over the grid, so the factor is read
//     from HBM / L2 once per workgroup and not per tile.
//   * Epilogue in the same kernel: x = mean + sigma * acc, the mirror fold to
//     [0, 1], from_unit (ut_param.h) and the stores of value and unit point.  The
//     accumulator registers are walked by ROTATION (a runtime loop over the
//     16-row tiles that shifts the tile array down one place, and over a tile's
//     four rows likewise) so that from_unit -- with LOGINT's double-double 2^x
//     -- is instantiated once, not 32 times, and no register array is indexed
//     dynamically (0 scratch).  The decode's DevParam records, the mean and the
//     centre's values of the dn features are LDS copies beside the factor.
//   * BOOL / ENUM / PERM and the single-point primitives are a second kernel,
//     k_cma_rest, one lane per candidate with a wave-uniform parameter loop as
//     in propose_tr.hip; it clears out_invalid where one of its columns moved.
//
// Bound: the normal draws (Philox, a log, a square root and two divisions each,
// with the polar method's rejections serialised per wave); the MFMAs are
// dn^2 / 64 per 16 candidates.  Compiled with -ffp-contract=off like every
// source here; the bit-exact parts are the draws, the fold and from_unit.
#include "gp_kstar_tile.h"
#include "ut_param.h"
#include "ut_perm.h"

namespace ut {

constexpr int CMA_NT = 512, CMA_WAVES = CMA_NT / 64, CMA_TILE = CMA_WAVES * 16;
constexpr int CMA_MAX_DN = 128;

// rows, row stride and bytes of the LDS image of a dn-feature call
inline int32_t cma_kp(int32_t dn) { return (dn + 3) / 4 * 4; }
inline int32_t cma_njt(int32_t dn) { return (dn + 15) / 16; }
inline int32_t cma_ldl(int32_t njt) { return (njt * 16 + 31) / 32 * 32; }
inline size_t cma_lds(int32_t dn) {
  const int32_t njt = cma_njt(dn);
  return sizeof(double) * ((size_t)cma_kp(dn) * cma_ldl(njt) + 2 * njt * 16) + sizeof(DevParam) * (size_t)dn;
}

// the fold of the line onto [0, 1] by mirroring at 0 and 1: t = x - 2 floor(x / 2),
// u = t > 1 ? 2 - t : t, evaluated on |x| (the fold is even), where every step is
// exact: |x| < 2 leaves t = |x|, |x| >= 2 subtracts a multiple of its own ulp,
// and 2 - t with t in (1, 2) is exact
__device__ __forceinline__ double cma_fold(double x) {
  const double a = fabs(x);
  const double t = a - 2.0 * floor(a * 0.5);
  return t > 1.0 ? 2.0 - t : t;
}

template <int NJT>
__global__ __launch_bounds__(CMA_NT) void k_cma(const DevParam* __restrict__ params, const int32_t* __restrict__ feat,
                                                const double* __restrict__ fac, const double* __restrict__ mean,
                                                const double* __restrict__ centre, int32_t dn, double sigma,
                                                uint64_t seed, uint32_t round_, int64_t cand_base, int64_t m,
                                                double* __restrict__ out, int64_t ldo, uint8_t* __restrict__ invalid,
                                                double* __restrict__ out_unit) {
  extern __shared__ double cma_smem[];
  constexpr int LDL = (NJT * 16 + 31) / 32 * 32;
  const int32_t kp = (dn + 3) / 4 * 4;
  double* sA = cma_smem;                 // [kp][LDL]: sA[k][j ^ ((k & 1) << 4)] = A[j][k]
  double* sMean = sA + kp * LDL;         // [NJT * 16]
  double* sCv = sMean + NJT * 16;        // [NJT * 16] the centre's value of feature j
  DevParam* sPar = reinterpret_cast<DevParam*>(sCv + NJT * 16);   // [dn]
  const int tid = threadIdx.x;
  for (int32_t e = tid; e < kp * LDL; e += CMA_NT) sA[e] = 0.0;
  for (int32_t j = tid; j < NJT * 16; j += CMA_NT) {
    double mj = 0.0, cv = 0.0;
    if (j < dn) {
      const DevParam pr = params[feat[j]];
      sPar[j] = pr;
      mj = mean[j];
      cv = centre[pr.col];
    }
    sMean[j] = mj;
    sCv[j] = cv;
  }
  __syncthreads();
  for (int32_t e = tid; e < dn * dn; e += CMA_NT) {
    const int32_t j = e / dn, k = e - j * dn;
    sA[k * LDL + (j ^ ((k & 1) << 4))] = fac[e];
  }
  __syncthreads();

  const int lane = tid & 63, w = tid >> 6;
  const int cl = lane & 15, kq = lane >> 4;
  const int64_t ntiles = (m + CMA_TILE - 1) / CMA_TILE;
  for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
    const int64_t i0 = t * CMA_TILE + w * 16;
    if (i0 >= m) continue;              // (wave-uniform; the loop holds no barrier)
    const int64_t i = i0 + cl;
    const bool live = i < m;
    const uint64_t g = (uint64_t)(cand_base + i);
    kd4 acc[NJT];
#pragma unroll
    for (int jt = 0; jt < NJT; ++jt) acc[jt] = (kd4){0.0, 0.0, 0.0, 0.0};
    for (int32_t k0 = 0; k0 < kp; k0 += 4) {
      const int32_t k = k0 + kq;
      double z = 0.0;
      if (live && k < dn) z = normal_draw(seed, g, (uint32_t)k | (1u << STREAM_SUB_SHIFT), round_, OP_CMA);
      const double* row = sA + k * LDL;
      const int sw = (k & 1) << 4;
#pragma unroll
      for (int jt = 0; jt < NJT; ++jt) acc[jt] = kstar_mfma(row[(jt * 16 + cl) ^ sw], z, acc[jt]);
    }
    // the lane's rows: feature jt * 16 + kq + 4 q of candidate i, walked by rotation
    bool same = true;
#pragma nounroll
    for (int jt = 0; jt < NJT; ++jt) {
      kd4 cur = acc[0];
#pragma unroll
      for (int s = 0; s + 1 < NJT; ++s) acc[s] = acc[s + 1];
#pragma nounroll
      for (int q = 0; q < 4; ++q) {
        const double s = cur.x;
        cur = (kd4){cur.y, cur.z, cur.w, cur.x};
        const int32_t j = jt * 16 + kq + 4 * q;
        if (j < dn && live) {
          const double u = cma_fold(__dadd_rn(sMean[j], __dmul_rn(sigma, s)));
          const double cv = sCv[j];
          const int32_t col = sPar[j].col;
          const double v = __dadd_rn(from_unit(sPar[j], u, cv), 0.0);
          out[(int64_t)col * ldo + i] = v;
          if (out_unit) out_unit[(int64_t)j * ldo + i] = u;
          same = same && d_to_bits(v) == d_to_bits(cv);
        }
      }
    }
    int sm = same ? 1 : 0;
    sm &= __shfl_xor(sm, 16);
    sm &= __shfl_xor(sm, 32);
    if (live && kq == 0) invalid[i] = (uint8_t)sm;
  }
}

// the parameters that are not moving primitives (rest[0 .. n_rest)): single-point
// primitives keep the centre's value; BOOL / ENUM / PERM move with cat_prob as
// in ut_propose_tr, without `must`
__global__ __launch_bounds__(256) void k_cma_rest(const DevParam* __restrict__ params,
                                                  const int32_t* __restrict__ rest, int32_t n_rest,
                                                  const double* __restrict__ centre, double cat_prob, uint64_t seed,
                                                  uint32_t round_, int64_t cand_base, int64_t m,
                                                  double* __restrict__ out, int64_t ldo,
                                                  uint8_t* __restrict__ invalid) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const uint64_t g = (uint64_t)(cand_base + i);
  bool moved = false;
  for (int32_t r = 0; r < n_rest; ++r) {
    const int32_t p = rest[r];
    const DevParam pr = params[p];
    if (is_primitive(pr.kind)) {
      out[(int64_t)pr.col * ldo + i] = centre[pr.col];
      continue;
    }
    const u32x4 a = draw(seed, g, (uint32_t)p, round_, OP_CMA);
    const bool pick = (double)a.z * (1.0 / 4294967296.0) < cat_prob;
    const uint32_t sb = (uint32_t)p | (1u << STREAM_SUB_SHIFT);
    if (pr.kind == UT_PERM) {
      const int32_t S = pr.psize;
      const PRow c{centre + pr.col, 1};
      WRow o{out + (int64_t)pr.col * ldo + i, ldo};
      perm_copy(o, c, S);
      if (pick) {
        PermRng R(seed, g, sb, round_, OP_CMA);
        perm_small_change(o, S, R);
        moved |= !perm_equal(o.ro(), c, S);
      }
      continue;
    }
    const double cv = centre[pr.col];
    double v = cv;
    if (pick) {
      if (pr.kind == UT_BOOL) {
        v = 1.0 - cv;
      } else if (pr.n_opt > 1) {   // ENUM: uniform over the other options
        const u32x4 b = draw(seed, g, sb, round_, OP_CMA);
        int64_t q = (int64_t)below64(u64_from(b.z, b.w), (uint64_t)(pr.n_opt - 1));
        q += (q >= (int64_t)cv) ? 1 : 0;
        v = (double)q;
      }
      moved |= d_to_bits(v) != d_to_bits(cv);
    }
    out[(int64_t)pr.col * ldo + i] = v;
  }
  if (moved) invalid[i] = 0;
}

template <int NJT>
static int launch_cma_n(ut_ctx* c, unsigned grid, size_t lds, const int32_t* feat, const double* fac, const double* mean,
                        const double* centre, int32_t dn, double sigma, uint32_t round_, int64_t cand_base, int64_t m,
                        double* out, int64_t ld, uint8_t* invalid, double* out_unit) {
  if (lds > 48 * 1024)
    UT_HIP(c, hipFuncSetAttribute(reinterpret_cast<const void*>(&k_cma<NJT>),
                                  hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
  hipLaunchKernelGGL(k_cma<NJT>, dim3(grid), dim3(CMA_NT), lds, c->stream, c->space.d_params.p, feat, fac, mean, centre,
                     dn, sigma, c->seed, round_, cand_base, m, out, ld, invalid, out_unit);
  UT_LAUNCH_CHECK(c);
  return 0;
}

// moving primitives of the space, in parameter order, then every other parameter
static int32_t cma_lists(const Space& s, std::vector<int32_t>& lists) {
  lists.assign((size_t)s.P, 0);
  int32_t dn = 0;
  for (int32_t p = 0; p < s.P; ++p) {
    const DevParam& pr = s.host_params[p];
    if (pr.kind <= UT_POW2 && pr.lo < pr.hi) lists[dn++] = p;
  }
  int32_t r = dn;
  for (int32_t p = 0; p < s.P; ++p) {
    const DevParam& pr = s.host_params[p];
    if (!(pr.kind <= UT_POW2 && pr.lo < pr.hi)) lists[r++] = p;
  }
  return dn;
}

static int launch_cma(ut_ctx* c, const ut_cma_params* a, const double* centre, const double* mean_host,
                      const double* factor_host, uint32_t round_, int64_t cand_base, int64_t m, double* out, int64_t ld,
                      uint8_t* invalid, double* out_unit) {
  const Space& s = c->space;
  const int32_t dn = a->dn, n_rest = s.P - dn;
  const size_t lds = cma_lds(dn);
  UT_CHECK(c, lds <= c->max_lds, UT_EUNSUPPORTED, "propose_cma: the factor does not fit the device's LDS");
  int rc;
  if ((rc = ensure(c, c->cma_in, (size_t)dn * dn + dn))) return rc;
  if ((rc = ensure(c, c->cma_lists, (size_t)s.P))) return rc;
  double* fac = c->cma_in.p;
  double* mean = fac + (size_t)dn * dn;
  UT_HIP(c, hipMemcpyAsync(fac, factor_host, sizeof(double) * dn * dn, hipMemcpyHostToDevice, c->stream));
  UT_HIP(c, hipMemcpyAsync(mean, mean_host, sizeof(double) * dn, hipMemcpyHostToDevice, c->stream));
  UT_HIP(c, hipMemcpyAsync(c->cma_lists.p, c->cma_lists_host.data(), sizeof(int32_t) * s.P, hipMemcpyHostToDevice,
                           c->stream));
  // persistent grid: as many workgroups as fit the CUs' LDS (at most 4 per CU), never more than tiles
  const int64_t ntiles = (m + CMA_TILE - 1) / CMA_TILE;
  const int64_t per_cu = std::max<int64_t>(1, std::min<int64_t>(4, (int64_t)(160 * 1024 / lds)));
  const unsigned grid = (unsigned)std::min<int64_t>(ntiles, per_cu * c->n_cu);
#define UT_CMA_CASE(N)                                                                                              \
  case N:                                                                                                           \
    rc = launch_cma_n<N>(c, grid, lds, c->cma_lists.p, fac, mean, centre, dn, a->sigma, round_, cand_base, m, out, ld, \
                         invalid, out_unit);                                                                        \
    break;
  switch (cma_njt(dn)) {
    UT_CMA_CASE(1) UT_CMA_CASE(2) UT_CMA_CASE(3) UT_CMA_CASE(4) UT_CMA_CASE(5) UT_CMA_CASE(6) UT_CMA_CASE(7)
    UT_CMA_CASE(8)
    default: rc = set_err(c, UT_EINVAL, "propose_cma: dn out of range");
  }
#undef UT_CMA_CASE
  if (rc) return rc;
  if (n_rest > 0) {
    hipLaunchKernelGGL(k_cma_rest, dim3(grid1(m, 256)), dim3(256), 0, c->stream, s.d_params.p, c->cma_lists.p + dn,
                       n_rest, centre, a->cat_prob, c->seed, round_, cand_base, m, out, ld, invalid);
    UT_LAUNCH_CHECK(c);
  }
  return 0;
}

}  // namespace ut

extern "C" int ut_propose_cma(ut_ctx* c, const ut_cma_params* a, const double* centre, const double* mean_host,
                              const double* factor_host, uint32_t round_, int64_t cand_base, int64_t m,
                              double* out_values, int64_t ld, uint8_t* out_invalid, double* out_unit) {
  if (!c) return UT_EINVAL;
  UT_CHECK(c, c->has_space, UT_ENOSPACE, "space not defined");
  UT_CHECK(c, a && centre && mean_host && factor_host && out_values && out_invalid, UT_EINVAL,
           "propose_cma: a NULL argument (only out_unit may be NULL)");
  UT_CHECK(c, m >= 0 && cand_base >= 0 && ld >= m, UT_EINVAL, "propose_cma: bad arguments");
  const double big = 1.7976931348623157e308;
  UT_CHECK(c, a->sigma > 0.0 && a->sigma <= big, UT_EINVAL, "propose_cma: sigma must be finite and > 0");
  UT_CHECK(c, a->cat_prob >= 0.0 && a->cat_prob <= 1.0, UT_EINVAL, "propose_cma: cat_prob must be in [0, 1]");
  UT_CHECK(c, a->dn >= 1 && a->dn <= ut::CMA_MAX_DN, UT_EINVAL, "propose_cma: dn must be in [1, 128]");
  const int32_t dn = ut::cma_lists(c->space, c->cma_lists_host);
  UT_CHECK(c, a->dn == dn, UT_EINVAL,
           "propose_cma: dn = " + std::to_string(a->dn) + " but the space has " + std::to_string(dn) +
               " moving primitive parameters");
  for (int32_t j = 0; j < dn; ++j)
    UT_CHECK(c, mean_host[j] >= -big && mean_host[j] <= big, UT_EINVAL, "propose_cma: mean is not finite");
  for (int32_t e = 0; e < dn * dn; ++e)
    UT_CHECK(c, factor_host[e] >= -big && factor_host[e] <= big, UT_EINVAL, "propose_cma: factor is not finite");
  if (m == 0) return 0;
  // a staged fit is issued after the proposal (as ut_propose_tr)
  int rc;
  if ((rc = ut::gp_fit_prefit(c))) return rc;
  if ((rc = ut::launch_cma(c, a, centre, mean_host, factor_host, round_, cand_base, m, out_values, ld, out_invalid,
                           out_unit)))
    return rc;
  return ut::gp_fit_flush(c);
}
