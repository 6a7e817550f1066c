// gp_ts.hip -- Thompson sampling (uthot.h "Thompson sampling" states the rule
// in full): q sample paths of the GP posterior over the whole candidate pool by
// pathwise conditioning, and one pick per path.
//
//   f_s(u) = sum_j Theta[s][j] phi_j(u)  +  sum_r k(x_r, u) a_s[r]
//
// Both sums are K*-shaped: a contraction of the candidates' scaled features
// with a row set (the D frequency rows Z / (2 pi), then the n training rows),
// an elementwise epilogue (cos2pi of the phase; the exp table of K*), and a
// second contraction of the tile with the paths' weights (Theta; A).
//
//   k_ts_paths  one workgroup = a 128-candidate column tile x a group of
//               TS_GROUP = 32 paths, looping over every row tile of both sets
//               with gp_kstar_tile.h's kstar_contract.  The fp64 16x16x4
//               accumulator (row = (lane >> 4) + 4 reg, col = lane & 15) is,
//               register by register, a B fragment (k = lane >> 4, n = lane &
//               15) of tile rows 4 reg .. 4 reg + 3, so the epilogue's values
//               feed out[s][col] += sum_row W[s][row] e[row][col] on the same
//               MFMA with no trip through LDS; W (A times sigma_f2, or Theta
//               times sqrt(2 sigma_f2 / D)) is staged in the freed ring.  The
//               path accumulators (32 paths x 64 columns per wave = 64 VGPRs)
//               stay in registers across all row tiles, in tile order; the
//               two waves of a column half combine once at the end through
//               LDS.  Neither K* nor a per-row-tile partial is stored.
//               Padding contributes exactly 0: -1e300 half-norms for the exp
//               set's rows and columns, zero A on its padding rows (D is a
//               multiple of 128: the frequency set has none), and columns
//               >= m are not written.
//   k_ts_solve  Out = In Mt for q rows at once on the fp64 MFMA, Mt one of
//               the triangular (L^-1)^T, L^-1: beta_s = L^-1 r_s, a_s = L^-T beta_s
//   k_ts_pick_* a pick = the partial minima of the path's row of F over the
//               free candidates (many workgroups), then their reduction, the
//               slot and the taken mark (one workgroup); chained on the stream
// Every sum runs in a fixed order and nothing is accumulated by atomics, so
// two calls on one fit and one draw return the same bits.
#include "gp_kstar_tile.h"

#include <cmath>

namespace ut {

constexpr int TS_LDW = TS_GROUP + 1;   // W in LDS: [128 rows][TS_LDW]
constexpr int32_t TS_PICK_WG = 256;
static_assert(K_BM * TS_LDW <= 2 * K_STAGE && TS_GROUP * K_BN <= 2 * K_STAGE, "W and the final sums fit the ring");
static_assert(TS_GROUP == 32, "two 16-path MFMA row blocks per group");

struct TsSets {
  const double *XsT, *xnorm;   // training rows: [dpad][npad] times KSTAR_T_SCALE, |xs|^2 [npad]
  int32_t n, npad, RT_a;       // RT_a = 0: the prior path alone (g_s)
  const double *ZT, *bph;      // frequency rows: [dpad][D] Z / (2 pi), phases [D]
  int32_t D;
  const double *A, *Theta;     // weights [q][npad], [q][D]
  double sf2, amp;
};

__global__ __launch_bounds__(K_NT, 1) void k_ts_paths(TsSets S, const double* __restrict__ B, int64_t ldb, int32_t dpad,
                                                      const double* __restrict__ cnorm, int64_t m, int32_t s_base,
                                                      int32_t q, double* __restrict__ out, int64_t ldf) {
  constexpr int MAIN = 2 * K_STAGE;
  // the ring (then W, then the final sums), the exp table, the item's row and column operands
  __shared__ __attribute__((aligned(16))) double lds[MAIN + EXP_TAB + 2 * K_BM];
  double* etab = lds + MAIN;
  double* const rowop = lds + MAIN + EXP_TAB;
  const int t = threadIdx.x, lane = t & 63;
  etab[t & (EXP_TAB - 1)] = exp2((double)(t & (EXP_TAB - 1)) / EXP_TAB);
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = w >> 1, wn = w & 1;
  const KstarRows rows = kstar_rows_f64(lane);
  const int64_t col0 = (int64_t)blockIdx.x * K_BN;
  const int32_t s0 = s_base + (int32_t)blockIdx.y * TS_GROUP;
  const int32_t RT_f = S.D / K_BM, RTt = S.RT_a + RT_f;

  kd4 pacc[2][4];
#pragma unroll
  for (int sb = 0; sb < 2; ++sb)
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) pacc[sb][jj] = (kd4){0.0, 0.0, 0.0, 0.0};

  for (int32_t it = 0; it < RTt; ++it) {
    const bool freq = it >= S.RT_a;
    const int32_t row0 = (freq ? it - S.RT_a : it) * K_BM;
    KstarOperands<double> o{};
    o.AT = freq ? S.ZT : S.XsT, o.lda = freq ? S.D : S.npad;
    o.B = B, o.ldb = ldb, o.dpad = dpad;
    const double* const rsrc = (freq ? S.bph : S.xnorm) + row0;
    const KstarAcc<double> acc = kstar_contract<double, false>(o, rows, row0, col0, lds, w, lane, [=] {
      if (w == 0)
        __builtin_amdgcn_global_load_lds(rsrc + lane * 2, (__attribute__((address_space(3))) void*)(rowop), 16, 0, 0);
      if (w == 1)
        __builtin_amdgcn_global_load_lds(cnorm + col0 + lane * 2,
                                         (__attribute__((address_space(3))) void*)(rowop + K_BM), 16, 0, 0);
    });
    __syncthreads();   // ring free: the item's weights W [128][TS_LDW] go there
    {
      const double* const W = freq ? S.Theta : S.A;
      const int64_t ldw = freq ? S.D : S.npad;
      const double sc = freq ? S.amp : S.sf2;
#pragma unroll
      for (int u = 0; u < TS_GROUP * K_BM / K_NT; ++u) {
        const int e = u * K_NT + t, sl = e >> 7, rl = e & (K_BM - 1);
        const int32_t s = s0 + sl;
        lds[rl * TS_LDW + sl] = s < q ? W[(int64_t)s * ldw + row0 + rl] * sc : 0.0;
      }
      if (!freq) {
        // the half-norms once per item; -1e300 for a padding row or column (k is then exactly 0)
        const double hv = (-0.5 * KSTAR_T_SCALE) * rowop[t];
        const bool in = t < K_BM ? row0 + t < S.n : col0 + (t - K_BM) < m;
        rowop[t] = in ? hv : -1e300;
      }
    }
    __syncthreads();
    double hc[4];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) hc[jj] = rowop[K_BM + wn * 64 + jj * 16 + (lane & 15)];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rl = wm * 64 + i * 16 + (lane >> 4) + 4 * r;
        const double hx = rowop[rl];
        double e[4];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          const double cacc = acc.a[i][jj][r];
          if (freq) {
            const double tau = cacc + hx;              // turns
            e[jj] = cos2pi(tau - __builtin_rint(tau));   // (exact reduction)
          } else {
            const double x = __builtin_fmax(__builtin_fmin((cacc + hx) + hc[jj], 0.0), KSTAR_T_MIN);
            e[jj] = sf2_exp2t_nonpos(x, etab);
          }
        }
        // accumulator register r of row group i = the B fragment of tile rows i * 16 + 4 r .. + 3
        const int wr = (wm * 64 + i * 16 + 4 * r + (lane >> 4)) * TS_LDW + (lane & 15);
        const double a0 = lds[wr], a1 = lds[wr + 16];
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          pacc[0][jj] = kstar_mfma(a0, e[jj], pacc[0][jj]);
          pacc[1][jj] = kstar_mfma(a1, e[jj], pacc[1][jj]);
        }
      }
    }
    __syncthreads();   // W and rowop read: the next item's stage 0 may land
  }
  // the two waves of a column half: wm = 1's sums through red [TS_GROUP][K_BN], added to wm = 0's
  double* const red = lds;
  if (wm == 1) {
#pragma unroll
    for (int sb = 0; sb < 2; ++sb)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int r = 0; r < 4; ++r)
          red[(sb * 16 + (lane >> 4) + 4 * r) * K_BN + wn * 64 + jj * 16 + (lane & 15)] = pacc[sb][jj][r];
  }
  __syncthreads();
  if (wm == 0) {
#pragma unroll
    for (int sb = 0; sb < 2; ++sb)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj)
#pragma unroll
        for (int r = 0; r < 4; ++r) {
          const int sl = sb * 16 + (lane >> 4) + 4 * r, cl = wn * 64 + jj * 16 + (lane & 15);
          const int32_t s = s0 + sl;
          const int64_t col = col0 + cl;
          if (s < q && col < m) out[(int64_t)(s - s_base) * ldf + col] = pacc[sb][jj][r] + red[sl * K_BN + cl];
        }
  }
}

// Z [D][d] as drawn, ZT [dpad][D] = Z * INV_2PI transposed (rows >= d zero), b [D]
__global__ __launch_bounds__(256) void k_ts_draw_z(uint64_t seed, uint32_t round_, int32_t D, int32_t d, int32_t dpad,
                                                   double* __restrict__ Z, double* __restrict__ ZT,
                                                   double* __restrict__ b) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)dpad * D) return;
  const int32_t k = (int32_t)(e / D), j = (int32_t)(e % D);
  double zs = 0.0;
  if (k < d) {
    const double z = normal_draw(seed, (uint64_t)j, (uint32_t)k, round_, OP_TS);
    Z[(int64_t)j * d + k] = z;
    zs = z * UT_INV_2PI;
  }
  ZT[e] = zs;
  if (k == 0) {
    const u32x4 r = draw(seed, (uint64_t)j, STREAM_CAND, round_, OP_TS);
    b[j] = u01_from(r.x, r.y);
  }
}

// Theta [q][D], Eps [q][npad] (0 on padding rows)
__global__ __launch_bounds__(256) void k_ts_draw_te(uint64_t seed, uint32_t round_, int32_t q, int32_t D, int32_t n,
                                                    int32_t npad, double* __restrict__ Theta,
                                                    double* __restrict__ Eps) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  const int64_t nt = (int64_t)q * D, ne = (int64_t)q * npad;
  if (e < nt) {
    const int32_t s = (int32_t)(e / D), j = (int32_t)(e % D);
    Theta[e] = normal_draw(seed, (uint64_t)j, (uint32_t)s | (1u << STREAM_SUB_SHIFT), round_, OP_TS);
  } else if (e < nt + ne) {
    const int64_t f = e - nt;
    const int32_t s = (int32_t)(f / npad), r = (int32_t)(f % npad);
    Eps[f] = r < n ? normal_draw(seed, (uint64_t)r, (uint32_t)s | (2u << STREAM_SUB_SHIFT), round_, OP_TS) : 0.0;
  }
}

// the training rows as candidates: xu [dpad][npad] = Xs^T (rows >= d, columns >= n zero)
__global__ __launch_bounds__(256) void k_ts_xu(const double* __restrict__ Xs, int32_t n, int32_t npad, int32_t d,
                                               int32_t dpad, double* __restrict__ xu) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)dpad * npad) return;
  const int32_t k = (int32_t)(e / npad), r = (int32_t)(e % npad);
  xu[e] = (k < d && r < n) ? Xs[(int64_t)r * d + k] : 0.0;
}

// r_s = ys - g_s(X) - sqrt(diag) Eps[s], 0 on padding rows; NaN after a failed fit
__global__ __launch_bounds__(256) void k_ts_resid(const double* __restrict__ ys, const double* __restrict__ G,
                                                  const double* __restrict__ Eps, int32_t q, int32_t n, int32_t npad,
                                                  double sd, const int32_t* __restrict__ fit_flag,
                                                  double* __restrict__ R) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)q * npad) return;
  const int32_t r = (int32_t)(e % npad);
  double v = 0.0;
  if (r < n) v = *fit_flag != 0 ? __builtin_nan("") : (ys[r] - G[e]) - sd * Eps[e];
  R[e] = v;
}

// Out [q][npad] = In [q][npad] Mt [npad][npad]; Mt[k][c] is taken as 0 above (upper = false: Mt = (L^-1)^T,
// nonzero for k <= c) or below (upper = true: Mt = L^-1, nonzero for k >= c) its triangle.  One wave per
// 16 x 16 output tile, k ascending in steps of 4; pad: the rows of Out from n on are written as 0
__global__ __launch_bounds__(64) void k_ts_solve(const double* __restrict__ In, const double* __restrict__ Mt,
                                                 int32_t npad, int32_t q, int32_t upper, int32_t nzero,
                                                 double* __restrict__ Out) {
  const int lane = threadIdx.x;
  const int32_t c0 = blockIdx.x * 16, sblk = blockIdx.y * 16;
  const int32_t sa = sblk + (lane & 15), cc = c0 + (lane & 15);
  const int32_t kbeg = upper ? c0 : 0, kend = upper ? npad : c0 + 16;
  kd4 acc = (kd4){0.0, 0.0, 0.0, 0.0};
  for (int32_t k0 = kbeg; k0 < kend; k0 += 4) {
    const int32_t kk = k0 + (lane >> 4);
    const double a = sa < q ? In[(int64_t)sa * npad + kk] : 0.0;
    const bool nz = upper ? kk >= cc : kk <= cc;
    const double b = nz ? Mt[(int64_t)kk * npad + cc] : 0.0;
    acc = kstar_mfma(a, b, acc);
  }
#pragma unroll
  for (int r = 0; r < 4; ++r) {
    const int32_t s = sblk + (lane >> 4) + 4 * r;
    if (s < q) Out[(int64_t)s * npad + cc] = cc < nzero ? acc[r] : 0.0;
  }
}

// (va, pa) is picked before (vb, pb): a NaN first (the minimum of a set with a NaN is NaN), then the
// smaller value, then the smaller position; pa < 0: nothing
__device__ __forceinline__ bool ts_before(double va, int64_t pa, double vb, int64_t pb) {
  if (pa < 0 || pb < 0) return pa >= 0;
  const bool na = va != va, nb = vb != vb;
  if (na || nb) return na && (!nb || pa < pb);
  return va < vb || (va == vb && pa < pb);
}

__device__ __forceinline__ void ts_wg_first(double& v, int64_t& p, double* rs, int64_t* rp) {
  const int tid = threadIdx.x;
  for (int off = 32; off > 0; off >>= 1) {
    const double vo = __shfl_xor(v, off);
    const int64_t po = __shfl_xor(p, off);
    if (ts_before(vo, po, v, p)) v = vo, p = po;
  }
  if ((tid & 63) == 0) rs[tid >> 6] = v, rp[tid >> 6] = p;
  __syncthreads();
  if (tid == 0)
    for (int w = 1; w < 4; ++w)
      if (ts_before(rs[w], rp[w], v, p)) v = rs[w], p = rp[w];
}

__global__ __launch_bounds__(256) void k_ts_pick_part(const double* __restrict__ F, int64_t m,
                                                      const uint8_t* __restrict__ dup,
                                                      const uint8_t* __restrict__ taken, double* __restrict__ pv,
                                                      int64_t* __restrict__ pp) {
  __shared__ double rs[4];
  __shared__ int64_t rp[4];
  double v = 1.0 / 0.0;
  int64_t p = -1;
  for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < m; i += (int64_t)gridDim.x * 256) {
    if (taken[i] || (dup && dup[i])) continue;
    const double f = F[i];
    if (ts_before(f, i, v, p)) v = f, p = i;
  }
  ts_wg_first(v, p, rs, rp);
  if (threadIdx.x == 0) pv[blockIdx.x] = v, pp[blockIdx.x] = p;
}

// dead = pp[TS_PICK_WG]: an earlier slot was empty
__global__ __launch_bounds__(256) void k_ts_pick_fin(int32_t nb, const double* __restrict__ pv,
                                                     int64_t* __restrict__ pp, uint8_t* __restrict__ taken,
                                                     int64_t* __restrict__ out_pos, double* __restrict__ out_f) {
  __shared__ double rs[4];
  __shared__ int64_t rp[4];
  const int tid = threadIdx.x;
  double v = tid < nb ? pv[tid] : 1.0 / 0.0;
  int64_t p = tid < nb ? pp[tid] : -1;
  ts_wg_first(v, p, rs, rp);
  if (tid == 0) {
    const bool empty = pp[TS_PICK_WG] != 0 || p < 0 || v != v;
    if (empty) pp[TS_PICK_WG] = 1;
    else taken[p] = 1;
    *out_pos = empty ? -1 : p;
    if (out_f) *out_f = empty ? 1.0 / 0.0 : v;
  }
}

// what every call on the current fit starts with: the fit's launches issued, its factor waited for on the device
static int ts_fit_ready(ut_ctx* c, const std::string& who) {
  UT_CHECK(c, c->gp_ready, UT_EINVAL, who + ": call ut_gp_fit first");
  int rc;
  if ((rc = gp_fit_flush(c))) return rc;
  UT_CHECK(c, c->has_space && c->space.n_feat == c->gp_d, UT_EINVAL,
           who + ": the fit's feature count is not the space's");
  if (c->fit_pending) UT_HIP(c, hipStreamWaitEvent(c->stream, c->ev_fit, 0));
  UT_CHECK(c, c->gp_npad_fit == gp_npad(c->gp_n) && c->gp_npad_fit % K_BM == 0, UT_EINVAL, who + ": no fitted GP");
  return 0;
}

static int ts_have_draw(ut_ctx* c, const std::string& who) {
  UT_CHECK(c, c->ts_q > 0, UT_EINVAL, who + ": call ut_gp_ts_draw first");
  UT_CHECK(c, c->ts_fit == c->fit_gen, UT_EINVAL,
           who + ": the paths were drawn for fit " + std::to_string(c->ts_fit) + " and fit " +
               std::to_string(c->fit_gen) + " is current (stale: call ut_gp_ts_draw again after every fit)");
  return 0;
}

// paths s_base .. s_base + ns - 1 at the m candidates of (B [dpad][ldb], cnorm) into out [ns][ldf]
static int ts_launch_paths(ut_ctx* c, bool data, const double* B, int64_t ldb, const double* cnorm, int64_t m,
                           int32_t s_base, int32_t ns, double* out, int64_t ldf) {
  const int32_t npad = c->gp_npad_fit, dpad = kstar_dpad(c->gp_d);
  UT_CHECK(c, ldb % K_BN == 0 && ldb >= m && dpad >= 4 && c->ts_D % K_BM == 0, UT_EINVAL, "gp_ts: bad padding");
  TsSets S{c->gp_XsT.p, c->gp_xnorm.p, c->gp_n, npad, data ? npad / K_BM : 0,
           c->ts_ZT.p,  c->ts_b.p,     c->ts_D, c->ts_A.p, c->ts_theta.p,
           c->gp_sf2,   std::sqrt(2.0 * c->gp_sf2 / (double)c->ts_D)};
  const dim3 grid((unsigned)((m + K_BN - 1) / K_BN), (unsigned)((ns + TS_GROUP - 1) / TS_GROUP));
  hipLaunchKernelGGL(k_ts_paths, grid, dim3(K_NT), 0, c->stream, S, B, ldb, dpad, cnorm, m, s_base, s_base + ns, out,
                     ldf);
  UT_LAUNCH_CHECK(c);
  return 0;
}

int gp_ts_draw_impl(ut_ctx* c, int32_t q, int32_t D, uint32_t round_) {
  UT_CHECK(c, q >= 1 && q <= TS_MAX_Q, UT_EINVAL, "gp_ts_draw: q = " + std::to_string(q) + " is not in [1, 256]");
  UT_CHECK(c, D >= 128 && D <= TS_MAX_D && D % 128 == 0, UT_EINVAL,
           "gp_ts_draw: D = " + std::to_string(D) + " is not a multiple of 128 in [128, 4096]");
  UT_CHECK(c, round_ < (1u << 24), UT_EINVAL, "gp_ts_draw: round_ does not fit 24 bits");
  int rc;
  if ((rc = ts_fit_ready(c, "gp_ts_draw"))) return rc;
  c->ts_q = 0;   // (nothing usable until every launch below is issued)
  const int32_t n = c->gp_n, d = c->gp_d, npad = c->gp_npad_fit, dpad = kstar_dpad(d);
  const size_t qn = (size_t)q * npad;
  if ((rc = ensure(c, c->ts_Z, (size_t)D * d))) return rc;
  if ((rc = ensure(c, c->ts_b, (size_t)D))) return rc;
  if ((rc = ensure(c, c->ts_ZT, (size_t)dpad * D))) return rc;
  if ((rc = ensure(c, c->ts_theta, (size_t)q * D))) return rc;
  if ((rc = ensure(c, c->ts_eps, qn))) return rc;
  if ((rc = ensure(c, c->ts_A, qn))) return rc;
  if ((rc = ensure(c, c->ts_R, 2 * qn))) return rc;
  if ((rc = ensure(c, c->ts_xu, (size_t)dpad * npad))) return rc;
  if ((rc = gp_ensure_linvt(c))) return rc;
  double* const R = c->ts_R.p;
  double* const G = R + qn;   // g_s(X), then beta_s
  hipLaunchKernelGGL(k_ts_draw_z, dim3(grid1((int64_t)dpad * D, 256)), dim3(256), 0, c->stream, c->seed, round_, D, d,
                     dpad, c->ts_Z.p, c->ts_ZT.p, c->ts_b.p);
  hipLaunchKernelGGL(k_ts_draw_te, dim3(grid1((int64_t)q * D + (int64_t)qn, 256)), dim3(256), 0, c->stream, c->seed,
                     round_, q, D, n, npad, c->ts_theta.p, c->ts_eps.p);
  hipLaunchKernelGGL(k_ts_xu, dim3(grid1((int64_t)dpad * npad, 256)), dim3(256), 0, c->stream, c->gp_Xs.p, n, npad, d,
                     dpad, c->ts_xu.p);
  UT_LAUNCH_CHECK(c);
  c->ts_D = D;
  // g_s(X): the path kernel on the training rows, the frequency rows alone
  if ((rc = ts_launch_paths(c, false, c->ts_xu.p, npad, c->gp_xnorm.p, n, 0, q, G, npad))) return rc;
  hipLaunchKernelGGL(k_ts_resid, dim3(grid1((int64_t)qn, 256)), dim3(256), 0, c->stream, c->gp_y.p, G, c->ts_eps.p, q,
                     n, npad, std::sqrt(c->gp_diag_fit), c->gp_flag.p, R);
  const dim3 sg(npad / 16, (q + 15) / 16);
  hipLaunchKernelGGL(k_ts_solve, sg, dim3(64), 0, c->stream, R, c->gp_LinvT.p, npad, q, 0, npad, G);
  hipLaunchKernelGGL(k_ts_solve, sg, dim3(64), 0, c->stream, G, c->gp_Linv.p, npad, q, 1, n, c->ts_A.p);
  UT_LAUNCH_CHECK(c);
  c->ts_q = q, c->ts_fit = c->fit_gen;
  return 0;
}

// the call's candidates as K* operands over every feature: c->ts_u [dpad][ldk], c->ts_cn [ldk]
static int ts_encode(ut_ctx* c, const double* values, int64_t ld, int64_t m, int64_t* ldk_out) {
  const int32_t dpad = kstar_dpad(c->gp_d);
  const int64_t ldk = gp_ldk(m);
  int rc;
  if ((rc = ensure(c, c->ts_u, (size_t)dpad * ldk))) return rc;
  if ((rc = ensure(c, c->ts_cn, (size_t)ldk))) return rc;
  *ldk_out = ldk;
  return launch_encode_scaled(c, values, ld, m, c->ts_u.p, dpad, ldk, c->ts_cn.p);
}

int gp_ts_eval_impl(ut_ctx* c, const double* values, int64_t ld, int64_t m, double* out_F, int64_t ldf) {
  UT_CHECK(c, values && out_F, UT_EINVAL, "gp_ts_eval: NULL values or out_F");
  UT_CHECK(c, m >= 1 && ld >= m && ldf >= m, UT_EINVAL, "gp_ts_eval: needs m >= 1, ld >= m and ldf >= m");
  int rc;
  if ((rc = ts_fit_ready(c, "gp_ts_eval"))) return rc;
  if ((rc = ts_have_draw(c, "gp_ts_eval"))) return rc;
  int64_t ldk;
  if ((rc = ts_encode(c, values, ld, m, &ldk))) return rc;
  return ts_launch_paths(c, true, c->ts_u.p, ldk, c->ts_cn.p, m, 0, c->ts_q, out_F, ldf);
}

int gp_ts_select_impl(ut_ctx* c, const double* values, int64_t ld, int64_t m, const uint8_t* dup, int32_t k,
                      int64_t* out_pos, double* out_f) {
  UT_CHECK(c, values && out_pos, UT_EINVAL, "gp_ts_select: NULL values or out_pos");
  UT_CHECK(c, m >= 1 && ld >= m, UT_EINVAL, "gp_ts_select: needs m >= 1 and ld >= m");
  int rc;
  if ((rc = ts_fit_ready(c, "gp_ts_select"))) return rc;
  if ((rc = ts_have_draw(c, "gp_ts_select"))) return rc;
  UT_CHECK(c, k >= 1 && k <= c->ts_q, UT_EINVAL,
           "gp_ts_select: k = " + std::to_string(k) + " is not in [1, q = " + std::to_string(c->ts_q) + "]");
  int64_t ldk;
  if ((rc = ts_encode(c, values, ld, m, &ldk))) return rc;
  if ((rc = ensure(c, c->ts_F, (size_t)TS_GROUP * ldk))) return rc;
  if ((rc = ensure(c, c->ts_pv, (size_t)TS_PICK_WG))) return rc;
  if ((rc = ensure(c, c->ts_pp, (size_t)TS_PICK_WG + 1))) return rc;
  if ((rc = ensure(c, c->ts_taken, (size_t)m))) return rc;
  UT_HIP(c, hipMemsetAsync(c->ts_taken.p, 0, (size_t)m, c->stream));
  UT_HIP(c, hipMemsetAsync(c->ts_pp.p + TS_PICK_WG, 0, sizeof(int64_t), c->stream));
  const int32_t nb = (int32_t)std::min<int64_t>(TS_PICK_WG, (m + 1023) / 1024);
  for (int32_t s0 = 0; s0 < k; s0 += TS_GROUP) {
    const int32_t ns = std::min(TS_GROUP, k - s0);
    if ((rc = ts_launch_paths(c, true, c->ts_u.p, ldk, c->ts_cn.p, m, s0, ns, c->ts_F.p, ldk))) return rc;
    for (int32_t s = s0; s < s0 + ns; ++s) {
      hipLaunchKernelGGL(k_ts_pick_part, dim3(nb), dim3(256), 0, c->stream, c->ts_F.p + (int64_t)(s - s0) * ldk, m, dup,
                         c->ts_taken.p, c->ts_pv.p, c->ts_pp.p);
      hipLaunchKernelGGL(k_ts_pick_fin, dim3(1), dim3(256), 0, c->stream, nb, c->ts_pv.p, c->ts_pp.p, c->ts_taken.p,
                         out_pos + s, out_f ? out_f + s : nullptr);
    }
    UT_LAUNCH_CHECK(c);
  }
  return 0;
}

int gp_ts_read_impl(ut_ctx* c, int32_t what, double* out_host, int32_t* info) {
  UT_CHECK(c, what >= 0 && what <= 4, UT_EINVAL, "gp_ts_read: what is not in [0, 4]");
  UT_CHECK(c, out_host || info, UT_EINVAL, "gp_ts_read: NULL out_host and info");
  UT_CHECK(c, c->gp_ready, UT_EINVAL, "gp_ts_read: call ut_gp_fit first");
  int rc;
  if ((rc = ts_have_draw(c, "gp_ts_read"))) return rc;
  const int32_t q = c->ts_q, D = c->ts_D, n = c->gp_n, d = c->gp_d, npad = c->gp_npad_fit;
  if (info) info[0] = q, info[1] = D, info[2] = n, info[3] = d;
  if (!out_host) return 0;
  switch (what) {
    case 0: UT_HIP(c, hipMemcpyAsync(out_host, c->ts_Z.p, sizeof(double) * D * d, hipMemcpyDeviceToHost, c->stream)); break;
    case 1: UT_HIP(c, hipMemcpyAsync(out_host, c->ts_b.p, sizeof(double) * D, hipMemcpyDeviceToHost, c->stream)); break;
    case 2:
      UT_HIP(c, hipMemcpyAsync(out_host, c->ts_theta.p, sizeof(double) * q * D, hipMemcpyDeviceToHost, c->stream));
      break;
    default: {
      const double* src = what == 3 ? c->ts_eps.p : c->ts_A.p;
      UT_HIP(c, hipMemcpy2DAsync(out_host, sizeof(double) * n, src, sizeof(double) * npad, sizeof(double) * n, q,
                                 hipMemcpyDeviceToHost, c->stream));
    }
  }
  UT_HIP(c, hipStreamSynchronize(c->stream));
  return 0;
}

}  // namespace ut
