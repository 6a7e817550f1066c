// ssgp.hip -- the sparse-spectrum GP (uthot.h "sparse-spectrum GP" states the
// rule in full): Bayesian linear regression on D random Fourier features of
// the RBF kernel.  The fit is O(n D^2) and the state D x D whatever n is; a
// scoring round is O(m D^2).
//
//   k_ssgp_gram  A's lower 128 x 128 tiles (i >= j) and c in one pass over the
//                training rows; Phi is formed on the fly and never stored.  A
//                workgroup owns a tile pair and a contiguous run of UNITS of
//                training rows.  Per 128-row step it forms the feature tiles
//                Phi_i and Phi_j ([128 rows][128 features], one on the
//                diagonal) with gp_kstar_tile.h's kstar_contract and the
//                cos2pi epilogue (the TS path kernel's), stages them through
//                LDS in four slices of 32 rows (2 x 32 x 128 doubles = the
//                freed ring's 64 KiB; two slices of Phi_i are parked in 64 KiB
//                more while Phi_j is contracted) and accumulates Phi_i^T Phi_j on
//                v_mfma_f64_16x16x4, 2 x 2 waves of 64 x 64 outputs.  The
//                accumulators stay in registers across a unit and are then
//                written to the workspace; tile column j = 0 also sums
//                c = Phi^T ys from the staged slices.  Padding rows (n to
//                npad) are zero phi: they contribute exactly 0.
//   k_ssgp_gram_red / k_ssgp_c_red   the units' partials summed in unit order
//                (no atomics), diag added, A written whole and symmetric and
//                its lower tiles as the factorisation's input.
//   The unit length is a function of (n, D) alone -- ssgp_split below --
//   and every sum runs in a fixed order inside a unit and across units, so
//   the bits do not depend on the launch: how many units one workgroup walks
//   (ut_ctx::ssgp_units_per_wg, a debug setting) changes the grid only.
//   The factorisation is gp_fit.hip's chain (launch_factor_chain), the
//   mat-vecs its k_lower_mv / k_upper_mv.
//
//   k_ssgp_phi   Phi* [D][ldc] for a chunk of candidates, in the layout the
//                fp64 variance contraction (gp_gemm.hip k_gp_var_pp) reads K*
//                in, zero past m; mu = phi . w as per-tile column sums
//                (kstar_colsums) reduced in tile order by the finalize.
//   k_ssgp_finalize   var = diag |L^-1 phi|^2 (a sum of squares: nothing
//                cancels), then gp_post.h's EI / UCB.
//
// ut_ssgp_lml_grid (the last section; uthot.h states the rule): the model's own
// log marginal likelihood at g points (a common scale on the lengthscales and a
// noise each).  A scale only divides the phase, so the projection is the same
// for every point:
//   k_ssgp_proj  P [rows][D] = Xs Zs^T for a chunk of rows, in turns, no phase:
//                the fit's contraction with no epilogue, once for all points.
//                Row-major, so that a 128-feature tile's row is 1 KiB in one
//                piece: what one glds instruction of the Gram kernel brings in.
//   k_ssgp_gram_grid   a workgroup owns (point, tile pair, unit).  The unit's
//                rows go by in slices of 16: the slice's two P tiles ([16][128]
//                each, 32 KiB, one ring stage) arrive by glds in the stage the
//                slice before last has left, under this slice's epilogue and
//                MFMAs; the epilogue (* rs_z + b, cos2pi, amplitude, zero past
//                n) runs in place in LDS, a thread on one feature column with
//                its phase in a register; then 16 MFMAs per 4 rows into the
//                accumulators that stay in registers across the unit.  Nothing
//                is parked and no Phi tile is held in registers, so two
//                workgroups share a CU (64 KiB each) and one's epilogue runs
//                under the other's MFMAs.  The point is the fastest grid
//                dimension: the workgroups that read one P tile run together.
//                Resources (-Rpass-analysis=kernel-resource-usage, gfx950):
//                VGPRs 214, AGPRs 0, SGPRs 106, scratch 0, LDS 65536 B,
//                occupancy 2 waves per SIMD.
//   k_ssgp_gram_red_grid / k_ssgp_c_red_grid   the units' partials in unit
//                order per point, + dg_z on the diagonal, into the batched
//                matrices and right-hand sides that gp_lml.hip's panel chain
//                (launch_lml_chain) factors; k_ssgp_lml_points the value.
//   The units are the fit's (ssgp_split), the rows of a unit are summed in row
//   order and the units in unit order: the bits depend on neither the launch,
//   the row chunking nor the batching of the points.
#include "gp_kstar_tile.h"
#include "gp_post.h"
#include "gp_tiles.h"

#include <cmath>

namespace ut {

// The Gram's row split.  A unit is `steps` consecutive 128-row steps whose
// products are accumulated in registers from zero; nsteps = npad / 128 steps,
// pairs = T (T + 1) / 2 tile pairs, T = D / 128.  Enough units that pairs x
// units reaches SSGP_WG_TARGET workgroups (two per CU on 256 CUs) where the
// rows allow it:
//   want  = max(1, SSGP_WG_TARGET / pairs)
//   steps = ceil(nsteps / min(nsteps, want)),  units = ceil(nsteps / steps)
constexpr int32_t SSGP_WG_TARGET = 512;
struct SsgpSplit {
  int32_t steps, units;
};
inline SsgpSplit ssgp_split(int32_t n, int32_t D) {
  const int32_t nsteps = gp_npad(n) / K_BM, T = D / K_BM, pairs = T * (T + 1) / 2;
  const int32_t want = std::max(1, SSGP_WG_TARGET / pairs);
  const int32_t steps = (nsteps + std::min(nsteps, want) - 1) / std::min(nsteps, want);
  return {steps, (nsteps + steps - 1) / steps};
}

constexpr int SS_SL = 32;   // rows of a staged slice
constexpr int SS_PARK = 2;  // slices of Phi_i parked in LDS of their own (a third frees no more registers)

// Z [D][d] as drawn, ZT [dpad][D] = Z * INV_2PI transposed (rows >= d zero), b [D]: k_ts_draw_z's draws with
// OP_SSGP and round 0
__global__ __launch_bounds__(256) void k_ssgp_draw(uint64_t seed, int32_t D, int32_t d, int32_t dpad,
                                                   double* __restrict__ Z, double* __restrict__ ZT,
                                                   double* __restrict__ b) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)dpad * D) return;
  const int32_t k = (int32_t)(e / D), j = (int32_t)(e % D);
  double zs = 0.0;
  if (k < d) {
    const double z = normal_draw(seed, (uint64_t)j, (uint32_t)k, 0u, OP_SSGP);
    Z[(int64_t)j * d + k] = z;
    zs = z * UT_INV_2PI;
  }
  ZT[e] = zs;
  if (k == 0) {
    const u32x4 r = draw(seed, (uint64_t)j, STREAM_CAND, 0u, OP_SSGP);
    b[j] = u01_from(r.x, r.y);
  }
}

// xuT [dpad][npad] = Xs^T (rows >= d, columns >= n zero)
__global__ __launch_bounds__(256) void k_ssgp_xut(const double* __restrict__ Xs, int32_t n, int32_t npad, int32_t d,
                                                  int32_t dpad, double* __restrict__ xuT) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)dpad * npad) return;
  const int32_t k = (int32_t)(e / npad), r = (int32_t)(e % npad);
  xuT[e] = (k < d && r < n) ? Xs[(int64_t)r * d + k] : 0.0;
}

// one feature tile of one 128-row step: phi[i][jj][q] at tile row wm 64 + 16 i + (lane >> 4) + 4 q (a training
// row) and column wn 64 + 16 jj + (lane & 15) (a feature); zero from row n on
// (returned by value from a local array, as kstar_contract returns its own: by reference it spills)
struct SsgpTile {
  kd4 a[4][4];
};
__device__ __forceinline__ SsgpTile ssgp_phi_tile(const KstarOperands<double>& o, const KstarRows rows, int32_t row0,
                                                  int32_t f0, const double* __restrict__ bph, int32_t n, double amp,
                                                  double* ring, int w, int lane) {
  kd4 phi[4][4];
  const int wm = w >> 1, wn = w & 1;
  const KstarAcc<double> acc = kstar_contract<double, false>(o, rows, row0, (int64_t)f0, ring, w, lane, [] {});
  double bb[4];
#pragma unroll
  for (int jj = 0; jj < 4; ++jj) bb[jj] = bph[f0 + wn * 64 + jj * 16 + (lane & 15)];
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const bool in = row0 + wm * 64 + i * 16 + (lane >> 4) + 4 * q < n;
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const double tau = acc.a[i][jj][q] + bb[jj];   // turns
        phi[i][jj][q] = in ? amp * cos2pi(tau - __builtin_rint(tau)) : 0.0;
      }
    }
  SsgpTile out;
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) out.a[i][jj] = phi[i][jj];
  return out;
}

// slice s (tile rows 16 s .. + 15 of each wave row) of a tile into P [SS_SL][128]: local row wm 16 + (lane >> 4) + 4 q
__device__ __forceinline__ void ssgp_stage(const SsgpTile& phi, int s, double* P, int w, int lane) {
  const int wm = w >> 1, wn = w & 1;
#pragma unroll
  for (int q = 0; q < 4; ++q)
#pragma unroll
    for (int jj = 0; jj < 4; ++jj)
      P[(wm * 16 + (lane >> 4) + 4 * q) * K_BN + wn * 64 + jj * 16 + (lane & 15)] = phi.a[s][jj][q];
}

__global__ __launch_bounds__(K_NT, 1) void k_ssgp_gram(const double* __restrict__ xuT, int32_t n, int32_t npad,
                                                       const double* __restrict__ ZT, const double* __restrict__ bph,
                                                       int32_t D, int32_t dpad, double amp,
                                                       const double* __restrict__ ys, int32_t steps, int32_t units,
                                                       int32_t upw, double* __restrict__ wsA,
                                                       double* __restrict__ wsc) {
  // the contraction's ring, then the two staged slices; the first SS_PARK slices of Phi_i, parked before Phi_j's
  // contraction takes the ring (so that their registers are free under it): 128 KiB in all
  __shared__ __attribute__((aligned(16))) double lds[2 * K_STAGE + SS_PARK * SS_SL * K_BN];
  static_assert(2 * SS_SL * K_BN <= 2 * K_STAGE, "the two slices fit the ring");
  static_assert(sizeof(lds) <= 160 * 1024, "a CU's LDS");
  double* const park = lds + 2 * K_STAGE;
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = w >> 1, wn = w & 1;
  const KstarRows rows = kstar_rows_f64(lane);
  int32_t ti, tj;
  lower_tile((int32_t)blockIdx.x, ti, tj);
  const bool diagt = ti == tj, withc = tj == 0;
  KstarOperands<double> o{};
  o.AT = xuT, o.lda = npad, o.B = ZT, o.ldb = D, o.dpad = dpad;
  const int32_t nsteps = npad / K_BM;
  const int32_t u_end = min(units, ((int32_t)blockIdx.y + 1) * upw);
  for (int32_t u = (int32_t)blockIdx.y * upw; u < u_end; ++u) {
    kd4 g[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) g[i][jj] = (kd4){0.0, 0.0, 0.0, 0.0};
    double cacc = 0.0;
    const int32_t st_end = min(nsteps, (u + 1) * steps);
    for (int32_t st = u * steps; st < st_end; ++st) {
      const int32_t row0 = st * K_BM;
      // (the glds addresses afresh per step: hoisted out of the unit loop they spill, gp_kstar_tile.h)
      const int il = kstar_item_lane(lane);
      const SsgpTile pi = ssgp_phi_tile(o, rows, row0, ti * K_BM, bph, n, amp, lds, w, il);
      SsgpTile pj;
#pragma unroll
      for (int s = 0; s < SS_PARK; ++s) ssgp_stage(pi, s, park + s * SS_SL * K_BN, w, lane);
      if (!diagt) {
        __syncthreads();   // the ring is read to the end before the next tile's stage 0 lands
        pj = ssgp_phi_tile(o, rows, row0, tj * K_BM, bph, n, amp, lds, w, il);
      }
#pragma unroll
      for (int s = 0; s < 4; ++s) {
        __syncthreads();   // ring (or the previous slice) fully read
        const double* const Pi = s < SS_PARK ? park + s * SS_SL * K_BN : lds;
        const double* const Pj = diagt ? Pi : lds + SS_SL * K_BN;
        if (s >= SS_PARK) ssgp_stage(pi, s, lds, w, lane);
        if (!diagt) ssgp_stage(pj, s, lds + SS_SL * K_BN, w, lane);
        __syncthreads();
#pragma nounroll
        for (int ks = 0; ks < SS_SL / 4; ++ks) {
          const int kr = ks * 4 + (lane >> 4);
          double af[4], bf[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) af[i] = Pi[kr * K_BN + wm * 64 + i * 16 + (lane & 15)];
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) bf[jj] = Pj[kr * K_BN + wn * 64 + jj * 16 + (lane & 15)];
#pragma unroll
          for (int i = 0; i < 4; ++i)
#pragma unroll
            for (int jj = 0; jj < 4; ++jj) g[i][jj] = kstar_mfma(af[i], bf[jj], g[i][jj]);
        }
        if (withc && t < K_BM) {
          // local row lr of the slice is tile row (lr >> 4) 64 + 16 s + (lr & 15)
#pragma nounroll
          for (int lr = 0; lr < SS_SL; ++lr)
            cacc += Pi[lr * K_BN + t] * ys[row0 + (lr >> 4) * 64 + s * 16 + (lr & 15)];
        }
      }
      __syncthreads();   // the slices are read: the next step's stage 0 may land
    }
    double* const wt = wsA + ((int64_t)blockIdx.x * units + u) * (K_BM * K_BN);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          wt[(wm * 64 + i * 16 + (lane >> 4) + 4 * q) * K_BN + wn * 64 + jj * 16 + (lane & 15)] = g[i][jj][q];
    if (withc && t < K_BM) wsc[((int64_t)ti * units + u) * K_BM + t] = cacc;
  }
}

// A (whole, symmetric) and Lw (the lower tiles, the diagonal ones whole) = the units' partials in unit order, + diag I
__global__ __launch_bounds__(256) void k_ssgp_gram_red(const double* __restrict__ wsA, int32_t units, int32_t D,
                                                       double diag, double* __restrict__ A, double* __restrict__ Lw) {
  int32_t ti, tj;
  lower_tile((int32_t)blockIdx.y, ti, tj);
  const int32_t e = (int32_t)blockIdx.x * 256 + threadIdx.x;   // < 128 * 128
  const double* p = wsA + (int64_t)blockIdx.y * units * (K_BM * K_BN) + e;
  double s = 0.0;
  for (int32_t u = 0; u < units; ++u) s += p[(int64_t)u * (K_BM * K_BN)];
  const int64_t i = (int64_t)ti * K_BM + (e >> 7), j = (int64_t)tj * K_BN + (e & 127);
  if (i == j) s += diag;
  A[i * D + j] = s;
  Lw[i * D + j] = s;
  if (ti != tj) A[j * D + i] = s;
}

__global__ __launch_bounds__(128) void k_ssgp_c_red(const double* __restrict__ wsc, int32_t units,
                                                    double* __restrict__ cv) {
  const double* p = wsc + (int64_t)blockIdx.x * units * K_BM + threadIdx.x;
  double s = 0.0;
  for (int32_t u = 0; u < units; ++u) s += p[(int64_t)u * K_BM];
  cv[(int64_t)blockIdx.x * K_BM + threadIdx.x] = s;
}

// Phi* [D][ldc] of the candidates B [dpad][ldb] (columns >= m zero), and the mean partials mpart [D / 128][ldc]
__global__ __launch_bounds__(K_NT, 2) void k_ssgp_phi(const double* __restrict__ ZT, const double* __restrict__ bph,
                                                      int32_t D, int32_t dpad, const double* __restrict__ B,
                                                      int64_t ldb, int64_t m, double amp,
                                                      const double* __restrict__ wv, double* __restrict__ phi,
                                                      int64_t ldc, double* __restrict__ mpart) {
  __shared__ __attribute__((aligned(16))) double lds[2 * K_STAGE];
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = w >> 1, wn = w & 1;
  const KstarRows rows = kstar_rows_f64(lane);
  const int64_t col0 = (int64_t)blockIdx.x * K_BN;
  const int32_t row0 = (int32_t)blockIdx.y * K_BM;
  KstarOperands<double> o{};
  o.AT = ZT, o.lda = D, o.B = B, o.ldb = ldb, o.dpad = dpad;
  const KstarAcc<double> acc = kstar_contract<double, false>(o, rows, row0, col0, lds, w, lane, [] {});
  double s[1][4] = {{0.0, 0.0, 0.0, 0.0}};
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      const int32_t f = row0 + wm * 64 + i * 16 + (lane >> 4) + 4 * q;
      const double bf = bph[f], wf = wv[f];
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) {
        const int64_t col = col0 + wn * 64 + jj * 16 + (lane & 15);
        const double tau = acc.a[i][jj][q] + bf;
        const double v = col < m ? amp * cos2pi(tau - __builtin_rint(tau)) : 0.0;
        phi[(int64_t)f * ldc + col] = v;
        s[0][jj] += v * wf;
      }
    }
  __syncthreads();   // ring free: the column sums' two wave rows go there
  kstar_colsums<1>(s, lds, lane, w,
                   [&](int, double tot) { mpart[(int64_t)blockIdx.y * ldc + col0 + t] = tot; });
}

__global__ __launch_bounds__(256) void k_ssgp_finalize(int64_t m, int32_t RT, const double* __restrict__ mpart,
                                                       const double* __restrict__ vpart, int64_t ldp, double diag,
                                                       Acq a, const uint8_t* __restrict__ dup,
                                                       double* __restrict__ mu_out, double* __restrict__ var_out,
                                                       double* __restrict__ score_out) {
  const int64_t j = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (j >= m) return;
  double mu = part_sum(mpart, RT, ldp, j);
  double var = diag * part_sum(vpart, RT, ldp, j);
  double sc = a.score(mu, var);
  if (*a.fit_flag != 0) mu = var = sc = __builtin_nan("");   // A was not positive definite
  if (dup && dup[j]) sc = -1.0 / 0.0;
  if (mu_out) mu_out[j] = mu;
  if (var_out) var_out[j] = var;
  if (score_out) score_out[j] = sc;
}

int ssgp_fit_impl(ut_ctx* c, const double* X, const double* y, int32_t n, int32_t d, const ut_gp_hyper* h, int32_t D) {
  UT_CHECK(c, X && y && h && h->lengthscale_host, UT_EINVAL, "ssgp_fit: NULL X, y, hyper or lengthscale_host");
  UT_CHECK(c, n >= 1 && n <= SSGP_MAX_N, UT_EINVAL, "ssgp_fit: n = " + std::to_string(n) + " is not in [1, 65536]");
  UT_CHECK(c, D >= 128 && D <= SSGP_MAX_D && D % 128 == 0, UT_EINVAL,
           "ssgp_fit: D = " + std::to_string(D) + " is not a multiple of 128 in [128, 2048]");
  UT_CHECK(c, c->has_space && d == c->space.n_feat, UT_EINVAL,
           "ssgp_fit: d = " + std::to_string(d) + " is not the space's feature count");
  UT_CHECK(c, c->gp_prec == 64, UT_EINVAL,
           "ssgp_fit: fp64 only, and ut_gp_set_precision is " + std::to_string(c->gp_prec));
  c->ss_ready = false;   // from here a failure leaves no fit
  const int32_t npad = gp_npad(n), dpad = kstar_dpad(d), T = D / K_BM, pairs = T * (T + 1) / 2;
  const SsgpSplit sp = ssgp_split(n, D);
  const size_t DD = (size_t)D * D;
  int rc;
  if ((rc = ensure(c, c->ss_Z, (size_t)D * d))) return rc;
  if ((rc = ensure(c, c->ss_b, (size_t)D))) return rc;
  if ((rc = ensure(c, c->ss_ZT, (size_t)dpad * D))) return rc;
  if ((rc = ensure(c, c->ss_inv_ell, (size_t)d))) return rc;
  if ((rc = ensure(c, c->ss_in, (size_t)n * d + n))) return rc;
  if ((rc = ensure(c, c->ss_Xs, (size_t)npad * d))) return rc;
  if ((rc = ensure(c, c->ss_xn, (size_t)npad))) return rc;
  if ((rc = ensure(c, c->ss_xuT, (size_t)dpad * npad))) return rc;
  if ((rc = ensure(c, c->ss_ys, (size_t)npad))) return rc;
  if ((rc = ensure(c, c->ss_stats, 4))) return rc;
  if ((rc = ensure(c, c->ss_flag, 1))) return rc;
  if ((rc = ensure(c, c->ss_ws, ((size_t)pairs * K_BM * K_BN + (size_t)T * K_BM) * sp.units))) return rc;
  if ((rc = ensure(c, c->ss_A, DD))) return rc;
  if ((rc = ensure(c, c->ss_c, (size_t)D))) return rc;
  if ((rc = ensure(c, c->ss_L, DD))) return rc;
  if ((rc = ensure(c, c->ss_Linv, DD))) return rc;
  if ((rc = ensure(c, c->ss_LinvT, DD))) return rc;
  if ((rc = ensure(c, c->ss_T, DD))) return rc;
  if ((rc = ensure(c, c->ss_beta, (size_t)D))) return rc;
  if ((rc = ensure(c, c->ss_w, (size_t)D))) return rc;
  std::vector<double> inv(d);
  for (int32_t k = 0; k < d; ++k) inv[k] = 1.0 / h->lengthscale_host[k];
  // (pageable sources: such a copy has read its source when the call returns, as tpe.hip relies on)
  double* const dX = c->ss_in.p;
  double* const dy = dX + (size_t)n * d;
  hipStream_t s = c->stream;
  UT_HIP(c, hipMemcpyAsync(c->ss_inv_ell.p, inv.data(), sizeof(double) * d, hipMemcpyHostToDevice, s));
  UT_HIP(c, hipMemcpyAsync(dX, X, sizeof(double) * (size_t)n * d, hipMemcpyHostToDevice, s));
  UT_HIP(c, hipMemcpyAsync(dy, y, sizeof(double) * n, hipMemcpyHostToDevice, s));
  UT_HIP(c, hipMemsetAsync(c->ss_flag.p, 0, sizeof(int32_t), s));
  const double diag = h->sigma_n2 + h->jitter, amp = std::sqrt(2.0 * h->sigma_f2 / (double)D);
  hipLaunchKernelGGL(k_ssgp_draw, dim3(grid1((int64_t)dpad * D, 256)), dim3(256), 0, s, c->seed, D, d, dpad,
                     c->ss_Z.p, c->ss_ZT.p, c->ss_b.p);
  UT_LAUNCH_CHECK(c);
  if ((rc = launch_gp_prep_train(c, dX, n, npad, d, c->ss_inv_ell.p, c->ss_Xs.p, c->ss_xn.p))) return rc;
  if ((rc = launch_gp_ystats(c, dy, n, npad, c->ss_ys.p, c->ss_stats.p))) return rc;
  hipLaunchKernelGGL(k_ssgp_xut, dim3(grid1((int64_t)dpad * npad, 256)), dim3(256), 0, s, c->ss_Xs.p, n, npad, d,
                     dpad, c->ss_xuT.p);
  double* const wsA = c->ss_ws.p;
  double* const wsc = wsA + (size_t)pairs * sp.units * K_BM * K_BN;
  const int32_t upw = std::max(1, c->ssgp_units_per_wg);
  hipLaunchKernelGGL(k_ssgp_gram, dim3(pairs, (sp.units + upw - 1) / upw), dim3(K_NT), 0, s, c->ss_xuT.p, n, npad,
                     c->ss_ZT.p, c->ss_b.p, D, dpad, amp, c->ss_ys.p, sp.steps, sp.units, upw, wsA, wsc);
  hipLaunchKernelGGL(k_ssgp_gram_red, dim3(K_BM * K_BN / 256, pairs), dim3(256), 0, s, wsA, sp.units, D, diag,
                     c->ss_A.p, c->ss_L.p);
  hipLaunchKernelGGL(k_ssgp_c_red, dim3(T), dim3(K_BM), 0, s, wsc, sp.units, c->ss_c.p);
  UT_LAUNCH_CHECK(c);
  if ((rc = launch_factor_chain(c, c->ss_L.p, c->ss_Linv.p, c->ss_T.p, c->ss_flag.p, D))) return rc;
  if ((rc = launch_lower_mv(c, c->ss_Linv.p, D, c->ss_c.p, c->ss_beta.p))) return rc;
  if ((rc = launch_transpose(c, c->ss_Linv.p, D, c->ss_LinvT.p, nullptr))) return rc;
  if ((rc = launch_upper_mv(c, c->ss_LinvT.p, D, c->ss_beta.p, c->ss_w.p))) return rc;
  c->ss_n = n, c->ss_d = d, c->ss_D = D;
  c->ss_sf2 = h->sigma_f2, c->ss_diag = diag;
  c->ss_ready = true;
  return 0;
}

int ssgp_score_impl(ut_ctx* c, const double* values, int64_t ld, int64_t m, const ut_acq* acq, const uint8_t* dup,
                    double* mu, double* var, double* score) {
  UT_CHECK(c, c->ss_ready, UT_EINVAL, "ssgp_score: call ut_ssgp_fit first");
  UT_CHECK(c, values && acq, UT_EINVAL, "ssgp_score: NULL values or acq");
  UT_CHECK(c, m >= 1 && ld >= m, UT_EINVAL, "ssgp_score: needs m >= 1 and ld >= m");
  UT_CHECK(c, c->has_space && c->space.n_feat == c->ss_d, UT_EINVAL,
           "ssgp_score: the fit's feature count is not the space's");
  const int32_t D = c->ss_D, RT = D / K_BM, dpad = kstar_dpad(c->ss_d);
  const int64_t ldk = gp_ldk(m);
  // candidates per chunk: the Phi* workspace [D][ldc] stays within the cap (256 MiB, gp_ts.hip's rule), whole
  // 256-candidate strips, at least one
  const int64_t cap = (int64_t)std::max(1, c->ssgp_phi_mib) << 20;
  const int64_t mc_max = std::max<int64_t>(VAR_BN, cap / (8 * (int64_t)D) / VAR_BN * VAR_BN);
  const int64_t ldc = std::min(ldk, mc_max);
  int rc;
  if ((rc = ensure(c, c->ss_u, (size_t)dpad * ldk))) return rc;
  if ((rc = ensure(c, c->ss_cn, (size_t)ldk))) return rc;
  if ((rc = ensure(c, c->ss_phi, (size_t)D * ldc))) return rc;
  if ((rc = ensure(c, c->ss_mu, (size_t)RT * ldc))) return rc;
  if ((rc = ensure(c, c->ss_vpart, (size_t)RT * ldc))) return rc;
  if ((rc = ensure(c, c->ss_mscr, (size_t)RT * ldc))) return rc;
  if ((rc = ensure(c, c->gp_ctr, 32))) return rc;   // the variance contraction's tickets
  if ((rc = launch_encode_scaled(c, values, ld, m, c->ss_u.p, dpad, ldk, c->ss_cn.p, c->ss_inv_ell.p))) return rc;
  const double amp = std::sqrt(2.0 * c->ss_sf2 / (double)D);
  const Acq a{c->ss_sf2, c->ss_stats.p, c->ss_flag.p, acq->kind, acq->xi, acq->kappa};
  for (int64_t m0 = 0; m0 < m; m0 += ldc) {
    const int64_t mc = std::min(ldc, m - m0), ldm = gp_ldk(mc);
    hipLaunchKernelGGL(k_ssgp_phi, dim3((unsigned)(ldm / K_BN), RT), dim3(K_NT), 0, c->stream, c->ss_ZT.p, c->ss_b.p,
                       D, dpad, c->ss_u.p + m0, ldk, mc, amp, c->ss_w.p, c->ss_phi.p, ldc, c->ss_mu.p);
    UT_LAUNCH_CHECK(c);
    // V = L^-1 Phi*: gp_gemm.hip's fp64 contraction as it runs on (L^-1, K*); its own mean partial is unused.
    // Its k loops unsplit (the split is for pruned scoring's few strips: its chunking, and so the rounding,
    // follows the strip count): a candidate's bits then do not depend on how the pool is cut
    if ((rc = launch_gemm_var(c, 64, c->ss_LinvT.p, D, c->ss_phi.p, ldc, D, mc, c->ss_vpart.p, c->ss_beta.p,
                              c->ss_mscr.p, false)))
      return rc;
    hipLaunchKernelGGL(k_ssgp_finalize, dim3(grid1(mc, 256)), dim3(256), 0, c->stream, mc, RT, c->ss_mu.p,
                       c->ss_vpart.p, ldc, c->ss_diag, a, dup ? dup + m0 : nullptr, mu ? mu + m0 : nullptr,
                       var ? var + m0 : nullptr, score ? score + m0 : nullptr);
    UT_LAUNCH_CHECK(c);
  }
  return 0;
}

int ssgp_read_impl(ut_ctx* c, int32_t what, double* out_host, int32_t* info) {
  UT_CHECK(c, what >= 0 && what <= 6, UT_EINVAL, "ssgp_read: what is not in [0, 6]");
  UT_CHECK(c, out_host || info, UT_EINVAL, "ssgp_read: NULL out_host and info");
  UT_CHECK(c, c->ss_ready, UT_EINVAL, "ssgp_read: call ut_ssgp_fit first");
  const int32_t n = c->ss_n, d = c->ss_d, D = c->ss_D;
  const size_t DD = (size_t)D * D;
  if (info) {
    int32_t flag = 0;
    UT_HIP(c, hipMemcpyAsync(&flag, c->ss_flag.p, sizeof(int32_t), hipMemcpyDeviceToHost, c->stream));
    UT_HIP(c, hipStreamSynchronize(c->stream));
    info[0] = n, info[1] = d, info[2] = D, info[3] = flag == 0 ? 1 : 0;
  }
  if (!out_host) return 0;
  const double* src = nullptr;
  size_t cnt = 0;
  switch (what) {
    case 0: src = c->ss_Z.p, cnt = (size_t)D * d; break;
    case 1: src = c->ss_b.p, cnt = D; break;
    case 2: src = c->ss_A.p, cnt = DD; break;
    case 3: src = c->ss_c.p, cnt = D; break;
    case 4:   // (the factor keeps A's entries above its diagonal tiles' triangle: masked through the scratch)
      if (int rc = launch_fit_read_lower(c, c->ss_L.p, D, c->ss_T.p)) return rc;
      src = c->ss_T.p, cnt = DD;
      break;
    case 5: src = c->ss_Linv.p, cnt = DD; break;
    default: src = c->ss_w.p, cnt = D;
  }
  UT_HIP(c, hipMemcpyAsync(out_host, src, sizeof(double) * cnt, hipMemcpyDeviceToHost, c->stream));
  UT_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

// ---------------------------------------------------------------------------
// ut_ssgp_lml_grid
// ---------------------------------------------------------------------------
constexpr int GG_SL = 16;                    // rows of a slice: two P tiles of it are one ring stage
constexpr int GG_TILE = GG_SL * K_BN;        // doubles of one tile's slice
static_assert(2 * GG_TILE == K_STAGE && K_BM % (2 * GG_SL) == 0, "a slice pair is a stage; a unit has an even count");

// P [rows][D] of the training rows row0 .. row0 + rows - 1 (whole 128-row steps): blockIdx.x a feature tile,
// blockIdx.y a step of the chunk
__global__ __launch_bounds__(K_NT, 2) void k_ssgp_proj(const double* __restrict__ xuT, int32_t npad,
                                                       const double* __restrict__ ZT, int32_t D, int32_t dpad,
                                                       int32_t row0, double* __restrict__ P) {
  __shared__ __attribute__((aligned(16))) double ring[2 * K_STAGE];
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = w >> 1, wn = w & 1;
  KstarOperands<double> o{};
  o.AT = xuT, o.lda = npad, o.B = ZT, o.ldb = D, o.dpad = dpad;
  const int32_t f0 = (int32_t)blockIdx.x * K_BN, lr0 = (int32_t)blockIdx.y * K_BM;
  const KstarAcc<double> acc =
      kstar_contract<double, false>(o, kstar_rows_f64(lane), row0 + lr0, (int64_t)f0, ring, w, lane, [] {});
#pragma unroll
  for (int i = 0; i < 4; ++i)
#pragma unroll
    for (int q = 0; q < 4; ++q) {
      double* const pr = P + (int64_t)(lr0 + wm * 64 + i * 16 + (lane >> 4) + 4 * q) * D + f0 + wn * 64 + (lane & 15);
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) pr[jj * 16] = acc.a[i][jj][q];
    }
}

// slice rows r .. r + 15 (chunk-local) of feature tiles fi and (unless the pair is diagonal) fj into one stage:
// wave w brings rows 4 w .. 4 w + 3 of each, a 1-KiB row per glds
__device__ __forceinline__ void ssgp_p_issue(const double* __restrict__ P, int32_t D, int32_t fi, int32_t fj,
                                             bool diagt, int64_t r, double* st, int w, int lane) {
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int q = 4 * w + u;
    __builtin_amdgcn_global_load_lds(P + (r + q) * D + fi + lane * 2,
                                     (__attribute__((address_space(3))) void*)(st + q * K_BN), 16, 0, 0);
  }
  if (diagt) return;
#pragma unroll
  for (int u = 0; u < 4; ++u) {
    const int q = 4 * w + u;
    __builtin_amdgcn_global_load_lds(P + (r + q) * D + fj + lane * 2,
                                     (__attribute__((address_space(3))) void*)(st + GG_TILE + q * K_BN), 16, 0, 0);
  }
}

// the units u0 .. u1 - 1 (whole, inside the chunk that starts at row crow0) of the points z0 + blockIdx.x;
// blockIdx.y the tile pair, blockIdx.z a run of upw units.  wsA [bz][pairs][units][128][128], wsc [bz][T][units][128]
__global__ __launch_bounds__(K_NT, 2) void k_ssgp_gram_grid(
    const double* __restrict__ P, int32_t crow0, int32_t n, int32_t npad, const double* __restrict__ bph, int32_t D,
    double amp, const double* __restrict__ rs, int32_t z0, const double* __restrict__ ys, int32_t steps, int32_t units,
    int32_t u0, int32_t u1, int32_t upw, double* __restrict__ wsA, double* __restrict__ wsc) {
  __shared__ __attribute__((aligned(16))) double lds[2 * K_STAGE];
  static_assert(2 * sizeof(lds) <= 160 * 1024, "two workgroups in a CU's LDS");
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = w >> 1, wn = w & 1;
  int32_t ti, tj;
  lower_tile((int32_t)blockIdx.y, ti, tj);
  const bool diagt = ti == tj, withc = tj == 0;
  const int32_t T = D / K_BM, pairs = (int32_t)gridDim.y, fi = ti * K_BM, fj = tj * K_BN;
  const int col = t & (K_BN - 1), half = t >> 7;   // the epilogue's column, and which rows of a slice: half + 2 k
  const double rsz = rs[z0 + blockIdx.x], bi = bph[fi + col], bj = bph[fj + col];
  const int32_t nsteps = npad / K_BM;
  const int32_t ub = u0 + (int32_t)blockIdx.z * upw, ue = min(u1, ub + upw);
  for (int32_t u = ub; u < ue; ++u) {
    kd4 g[4][4];
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) g[i][jj] = (kd4){0.0, 0.0, 0.0, 0.0};
    double cacc = 0.0;
    const int32_t rbeg = u * steps * K_BM, rend = min(nsteps, (u + 1) * steps) * K_BM;
    const int32_t nsl = (rend - rbeg) / GG_SL;   // even: the last slice's stage is 1, the next unit starts in 0
    ssgp_p_issue(P, D, fi, fj, diagt, (int64_t)(rbeg - crow0), lds, w, lane);
    for (int32_t it = 0; it < nsl; ++it) {
      const int32_t r0 = rbeg + it * GG_SL;
      asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
      __builtin_amdgcn_s_barrier();   // slice it has landed everywhere; slice it - 1 is fully read
      asm volatile("" ::: "memory");
      if (it + 1 < nsl)
        ssgp_p_issue(P, D, fi, fj, diagt, (int64_t)(r0 + GG_SL - crow0), lds + ((it + 1) & 1) * K_STAGE, w, lane);
      double* const Si = lds + (it & 1) * K_STAGE;
      double* const Sj = diagt ? Si : Si + GG_TILE;
      // the point's epilogue in place: tau = P rs + b (product and sum rounded apart)
#pragma unroll
      for (int k = 0; k < GG_SL / 2; ++k) {
        const int lr = half + 2 * k;
        const bool in = r0 + lr < n;
        const double ta = Si[lr * K_BN + col] * rsz + bi;
        Si[lr * K_BN + col] = in ? amp * cos2pi(ta - __builtin_rint(ta)) : 0.0;
        if (!diagt) {
          const double tb = Sj[lr * K_BN + col] * rsz + bj;
          Sj[lr * K_BN + col] = in ? amp * cos2pi(tb - __builtin_rint(tb)) : 0.0;
        }
      }
      __syncthreads();
#pragma unroll
      for (int ks = 0; ks < GG_SL / 4; ++ks) {
        const int kr = ks * 4 + (lane >> 4);
        double af[4], bf[4];
#pragma unroll
        for (int i = 0; i < 4; ++i) af[i] = Si[kr * K_BN + wm * 64 + i * 16 + (lane & 15)];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) bf[jj] = Sj[kr * K_BN + wn * 64 + jj * 16 + (lane & 15)];
#pragma unroll
        for (int i = 0; i < 4; ++i)
#pragma unroll
          for (int jj = 0; jj < 4; ++jj) g[i][jj] = kstar_mfma(af[i], bf[jj], g[i][jj]);
      }
      if (withc && t < K_BM) {
#pragma unroll
        for (int lr = 0; lr < GG_SL; ++lr) cacc += Si[lr * K_BN + t] * ys[r0 + lr];
      }
    }
    __syncthreads();   // the last slice is read before the next unit's first one lands
    double* const wt = wsA + (((int64_t)blockIdx.x * pairs + blockIdx.y) * units + u) * (K_BM * K_BN);
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int q = 0; q < 4; ++q)
          wt[(wm * 64 + i * 16 + (lane >> 4) + 4 * q) * K_BN + wn * 64 + jj * 16 + (lane & 15)] = g[i][jj][q];
    if (withc && t < K_BM) wsc[(((int64_t)blockIdx.x * T + ti) * units + u) * K_BM + t] = cacc;
  }
}

// K [bz][D][D], whole and symmetric (the chain reads its lower 64-tiles, the read-back all of it) = the units'
// partials in unit order, + dg_z I; a diagonal tile's upper half is its lower half mirrored
__global__ __launch_bounds__(256) void k_ssgp_gram_red_grid(const double* __restrict__ wsA, int32_t units, int32_t D,
                                                            const double* __restrict__ dg, int32_t z0,
                                                            double* __restrict__ K) {
  int32_t ti, tj;
  lower_tile((int32_t)blockIdx.y, ti, tj);
  const int32_t e = (int32_t)blockIdx.x * 256 + threadIdx.x;   // < 128 * 128
  int32_t r = e >> 7, cc = e & 127;
  if (ti == tj && cc > r) {
    const int32_t x = r;
    r = cc, cc = x;
  }
  const double* p = wsA + ((int64_t)blockIdx.z * gridDim.y + blockIdx.y) * units * (K_BM * K_BN) + r * K_BN + cc;
  double s = 0.0;
  for (int32_t u = 0; u < units; ++u) s += p[(int64_t)u * (K_BM * K_BN)];
  const int64_t i = (int64_t)ti * K_BM + (e >> 7), j = (int64_t)tj * K_BN + (e & 127);
  if (i == j) s += dg[z0 + blockIdx.z];
  double* Kz = K + (int64_t)blockIdx.z * D * D;
  Kz[i * D + j] = s;
  if (ti != tj) Kz[j * D + i] = s;
}

// rhs [bz][D] = c_z; blockIdx.x a feature tile, blockIdx.y the point
__global__ __launch_bounds__(128) void k_ssgp_c_red_grid(const double* __restrict__ wsc, int32_t units, int32_t D,
                                                         double* __restrict__ rhs) {
  const double* p = wsc + ((int64_t)blockIdx.y * gridDim.x + blockIdx.x) * units * K_BM + threadIdx.x;
  double s = 0.0;
  for (int32_t u = 0; u < units; ++u) s += p[(int64_t)u * K_BM];
  rhs[(int64_t)blockIdx.y * D + (int64_t)blockIdx.x * K_BM + threadIdx.x] = s;
}

// s + t exactly as hi + lo (Knuth), and (hi, lo) += x * x or -= x * x with the product's error kept (fma)
__device__ __forceinline__ void dd_add(double& hi, double& lo, double x, double xl) {
  const double s = hi + x, bb = s - hi;
  lo += ((hi - (s - bb)) + (x - bb)) + xl;
  hi = s;
}
__device__ __forceinline__ void dd_add_sq(double& hi, double& lo, double x, double sign) {
  const double p = x * x;
  dd_add(hi, lo, sign * p, sign * __builtin_fma(x, x, -p));
}

// the values of the points z0 + blockIdx.x from their factor L (in K) and beta (in rhs); every sum by thread
// stride, then a tree: a fixed order.  q = |ys|^2 - |beta|^2 is divided by 2 dg and both norms are near n: it is
// one signed sum carried in two doubles, so that what is left of it is the elements' own error, not the sum's
__global__ __launch_bounds__(256) void k_ssgp_lml_points(const double* __restrict__ K, const double* __restrict__ rhs,
                                                         const int32_t* __restrict__ flag, const double* __restrict__ ys,
                                                         int32_t n, int32_t D, const double* __restrict__ dg,
                                                         int32_t z0, double* __restrict__ out) {
  __shared__ double red[3][256];
  const int t = threadIdx.x;
  const double* L = K + (int64_t)blockIdx.x * D * D;
  const double* beta = rhs + (int64_t)blockIdx.x * D;
  double sl = 0.0, qh = 0.0, ql = 0.0;
  for (int32_t i = t; i < D; i += 256) {
    sl += log(L[(int64_t)i * D + i]);
    dd_add_sq(qh, ql, beta[i], -1.0);
  }
  for (int32_t i = t; i < n; i += 256) dd_add_sq(qh, ql, ys[i], 1.0);
  red[0][t] = sl, red[1][t] = qh, red[2][t] = ql;
  __syncthreads();
  for (int h = 128; h > 0; h >>= 1) {
    if (t < h) {
      red[0][t] += red[0][t + h];
      dd_add(red[1][t], red[2][t], red[1][t + h], red[2][t + h]);
    }
    __syncthreads();
  }
  if (t != 0) return;
  const double d = dg[z0 + blockIdx.x];
  const double v = -(red[1][0] + red[2][0]) / (2.0 * d) - red[0][0] - 0.5 * (double)(n - D) * log(d) -
                   0.5 * (double)n * 1.8378770664093454836;   // log 2 pi
  out[z0 + blockIdx.x] = flag[z0 + blockIdx.x] != 0 ? __builtin_nan("") : v;
}

int ssgp_lml_grid_impl(ut_ctx* c, const double* X, const double* y, int32_t n, int32_t d, const ut_gp_hyper* h,
                       int32_t D, int32_t g, const double* scale, const double* noise, double* lml_host,
                       int32_t* best_host, double* A_host, double* c_host) {
  UT_CHECK(c, X && y && h && h->lengthscale_host && scale && lml_host && best_host, UT_EINVAL,
           "ssgp_lml_grid: NULL argument");
  UT_CHECK(c, n >= 1 && n <= SSGP_MAX_N, UT_EINVAL,
           "ssgp_lml_grid: n = " + std::to_string(n) + " is not in [1, 65536]");
  UT_CHECK(c, D >= 128 && D <= SSGP_MAX_D && D % 128 == 0, UT_EINVAL,
           "ssgp_lml_grid: D = " + std::to_string(D) + " is not a multiple of 128 in [128, 2048]");
  UT_CHECK(c, c->has_space && d == c->space.n_feat, UT_EINVAL,
           "ssgp_lml_grid: d = " + std::to_string(d) + " is not the space's feature count");
  UT_CHECK(c, c->gp_prec == 64, UT_EINVAL,
           "ssgp_lml_grid: fp64 only, and ut_gp_set_precision is " + std::to_string(c->gp_prec));
  UT_CHECK(c, g >= 1, UT_EINVAL, "ssgp_lml_grid: g must be at least 1");
  for (int32_t z = 0; z < g; ++z)
    UT_CHECK(c, std::isfinite(scale[z]) && scale[z] > 0.0, UT_EINVAL, "ssgp_lml_grid: scales must be finite and > 0");
  const int32_t npad = gp_npad(n), dpad = kstar_dpad(d), T = D / K_BM, pairs = T * (T + 1) / 2;
  const SsgpSplit sp = ssgp_split(n, D);
  const size_t DD = (size_t)D * D;
  // a point's partial tiles and c's; a batch of B points holds B D^2 doubles of matrices within LML_BUDGET and
  // its partials within as much again
  const size_t wsz = ((size_t)pairs * K_BM * K_BN + (size_t)T * K_BM) * sp.units;
  int64_t B = c->lml_batch > 0 ? c->lml_batch
                               : (int64_t)std::min(LML_BUDGET / (DD * sizeof(double)), LML_BUDGET / (wsz * sizeof(double)));
  B = std::max<int64_t>(1, std::min<int64_t>(B, g));
  // row chunks of whole units whose P stays within the Phi* cap, at least a unit
  const int64_t cap = (int64_t)std::max(1, c->ssgp_phi_mib) << 20;
  const int64_t urow = (int64_t)sp.steps * K_BM;
  const int32_t uchunk = (int32_t)std::min<int64_t>(sp.units, std::max<int64_t>(1, cap / (urow * D * 8)));
  const int64_t prow = std::min<int64_t>(npad, (int64_t)uchunk * urow);
  // sl_in: X | y | 1/ell | scaled rows | norms | the rows transposed | ys | stats | Z | ZT | b | 1/scale | dg | lml
  // (every block on an even offset: the glds sources are read 16 B at a time)
  auto up2 = [](size_t v) { return (v + 1) & ~(size_t)1; };
  const size_t oy = up2((size_t)n * d), oinv = up2(oy + n), oXs = up2(oinv + d), oxn = up2(oXs + (size_t)npad * d);
  const size_t oxu = up2(oxn + npad), oys = up2(oxu + (size_t)dpad * npad), ost = up2(oys + npad), oZ = ost + 4;
  const size_t oZT = up2(oZ + (size_t)D * d), ob = up2(oZT + (size_t)dpad * D), ors = up2(ob + D), odg = ors + g;
  const size_t olml = odg + g;
  int rc;
  if ((rc = ensure(c, c->sl_in, olml + g))) return rc;
  if ((rc = ensure(c, c->sl_P, (size_t)prow * D))) return rc;
  if ((rc = ensure(c, c->sl_ws, (size_t)B * wsz))) return rc;
  if ((rc = ensure(c, c->lml_k, (size_t)B * DD))) return rc;
  if ((rc = ensure(c, c->lml_li, (size_t)B * NB * D))) return rc;
  if ((rc = ensure(c, c->lml_rhs, (size_t)B * D))) return rc;
  if ((rc = ensure(c, c->lml_flag, (size_t)g))) return rc;
  double* const in = c->sl_in.p;
  std::vector<double> hp((size_t)d + 2 * g);
  for (int32_t k = 0; k < d; ++k) hp[k] = 1.0 / h->lengthscale_host[k];
  for (int32_t z = 0; z < g; ++z) {
    hp[(size_t)d + z] = 1.0 / scale[z];
    hp[(size_t)d + g + z] = (noise ? noise[z] : h->sigma_n2) + h->jitter;
  }
  const double amp = std::sqrt(2.0 * h->sigma_f2 / (double)D);
  const int32_t upw = std::max(1, c->ssgp_units_per_wg);
  hipStream_t s = c->stream;
  auto enqueue = [&]() -> int {
    UT_HIP(c, hipMemcpyAsync(in, X, sizeof(double) * (size_t)n * d, hipMemcpyHostToDevice, s));
    UT_HIP(c, hipMemcpyAsync(in + oy, y, sizeof(double) * n, hipMemcpyHostToDevice, s));
    UT_HIP(c, hipMemcpyAsync(in + oinv, hp.data(), sizeof(double) * d, hipMemcpyHostToDevice, s));
    UT_HIP(c, hipMemcpyAsync(in + ors, hp.data() + d, sizeof(double) * 2 * g, hipMemcpyHostToDevice, s));
    UT_HIP(c, hipMemsetAsync(c->lml_flag.p, 0, sizeof(int32_t) * g, s));
    hipLaunchKernelGGL(k_ssgp_draw, dim3(grid1((int64_t)dpad * D, 256)), dim3(256), 0, s, c->seed, D, d, dpad,
                       in + oZ, in + oZT, in + ob);
    UT_LAUNCH_CHECK(c);
    if ((rc = launch_gp_prep_train(c, in, n, npad, d, in + oinv, in + oXs, in + oxn))) return rc;
    if ((rc = launch_gp_ystats(c, in + oy, n, npad, in + oys, in + ost))) return rc;
    hipLaunchKernelGGL(k_ssgp_xut, dim3(grid1((int64_t)dpad * npad, 256)), dim3(256), 0, s, in + oXs, n, npad, d, dpad,
                       in + oxu);
    UT_LAUNCH_CHECK(c);
    int32_t in_P = -1;   // the chunk P holds: projected again only when another one is needed
    for (int32_t z0 = 0; z0 < g; z0 += (int32_t)B) {
      const int32_t bz = std::min<int32_t>((int32_t)B, g - z0);
      double* const wsA = c->sl_ws.p;
      double* const wsc = wsA + (size_t)bz * pairs * sp.units * K_BM * K_BN;
      for (int32_t u0 = 0; u0 < sp.units; u0 += uchunk) {
        const int32_t u1 = std::min(sp.units, u0 + uchunk);
        const int32_t crow0 = (int32_t)(u0 * urow), crows = (int32_t)std::min<int64_t>(npad, u1 * urow) - crow0;
        if (in_P != u0) {
          hipLaunchKernelGGL(k_ssgp_proj, dim3(T, crows / K_BM), dim3(K_NT), 0, s, in + oxu, npad, in + oZT, D, dpad,
                             crow0, c->sl_P.p);
          in_P = u0;
        }
        hipLaunchKernelGGL(k_ssgp_gram_grid, dim3(bz, pairs, (u1 - u0 + upw - 1) / upw), dim3(K_NT), 0, s, c->sl_P.p,
                           crow0, n, npad, in + ob, D, amp, in + ors, z0, in + oys, sp.steps, sp.units, u0, u1, upw,
                           wsA, wsc);
        UT_LAUNCH_CHECK(c);
      }
      hipLaunchKernelGGL(k_ssgp_gram_red_grid, dim3(K_BM * K_BN / 256, pairs, bz), dim3(256), 0, s, wsA, sp.units, D,
                         in + odg, z0, c->lml_k.p);
      hipLaunchKernelGGL(k_ssgp_c_red_grid, dim3(T, bz), dim3(K_BM), 0, s, wsc, sp.units, D, c->lml_rhs.p);
      UT_LAUNCH_CHECK(c);
      if (A_host)
        UT_HIP(c, hipMemcpyAsync(A_host + (size_t)z0 * DD, c->lml_k.p, sizeof(double) * bz * DD,
                                 hipMemcpyDeviceToHost, s));
      if (c_host)
        UT_HIP(c, hipMemcpyAsync(c_host + (size_t)z0 * D, c->lml_rhs.p, sizeof(double) * bz * D,
                                 hipMemcpyDeviceToHost, s));
      if ((rc = launch_lml_chain(c, c->lml_k.p, c->lml_li.p, c->lml_rhs.p, c->lml_flag.p + z0, D, bz, true)))
        return rc;
      hipLaunchKernelGGL(k_ssgp_lml_points, dim3(bz), dim3(256), 0, s, c->lml_k.p, c->lml_rhs.p, c->lml_flag.p,
                         in + oys, n, D, in + odg, z0, in + olml);
      UT_LAUNCH_CHECK(c);
    }
    UT_HIP(c, hipMemcpyAsync(lml_host, in + olml, sizeof(double) * g, hipMemcpyDeviceToHost, s));
    return 0;
  };
  // the caller's arrays and hp are read by copies in flight: wait whatever happened
  rc = enqueue();
  const hipError_t es = hipStreamSynchronize(s);
  if (rc) return rc;
  UT_HIP(c, es);
  int32_t best = -1;
  for (int32_t z = 0; z < g; ++z) {
    if (!std::isfinite(lml_host[z])) {
      lml_host[z] = std::nan("");
      continue;
    }
    if (best < 0 || lml_host[z] > lml_host[best]) best = z;
  }
  *best_host = best;
  return 0;
}

}  // namespace ut
