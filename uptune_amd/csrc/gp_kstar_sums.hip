// gp_kstar_sums.hip -- the K* contraction (gp_kstar_tile.h) with a column-sum
// epilogue and no K* stored: per candidate u and row set,
//   NW = 0:  S(u)   = sum_r k(x_r, u)            (the failure vote, gp_feas.hip)
//   NW > 0:  S_q(u) = sum_r k(x_r, u) w_q[r]     (the constraint means, gp_cons.hip)
// with k(a, u) = exp(-1/2 |(a - u) / ell|^2 / s^2), s = 1 unless SCALED.
#include "gp_kstar_tile.h"

namespace ut {

// One launch covers two row sets: item j of an XCD group is row tile
// j % (RT_a + RT_b) -- a's tiles, then b's (RT_b = 0: a alone).
//   1. the item's epilogue operands go to LDS beside stage 0, one 1-KiB glds
//      each (rows < npad, columns < ldk are in range), spread over the waves:
//      rowop = [norm 128][cnorm 128][w_q 128] x NW;
//   2. SCALED: the exponent is scaled by 1 / s^2 (the categorical c0 + c1 M
//      start with it: s scales every lengthscale).  Each of its three terms is
//      scaled, not their sum, so that a padding row's or column's -1e300 stays
//      what it is whatever s (inv_s2 == 1: the same bits as K*'s (acc + hx) + hc).
//      The accumulator's product is rounded before the add;
//   3. part [RT_a + RT_b][max(NW, 1)][ldk] gets the tile's column sums
//      (sigma_f2 = 1 in the exp table: the consumer multiplies).
// Padding rows (row >= n of their set) and columns (>= m) contribute exactly
// 0: their half-norm is -1e300, and the clamp at KSTAR_T_MIN is where the
// table's 2^k' underflows to 0 (and w is 0 on padding rows).
// o: what both row sets share (B, ldb, dpad, bcat, nkc, c0, c1); the item's set fills in the rest
template <bool CAT, int NW, bool SCALED>
__global__ __launch_bounds__(K_NT, 2) void k_kstar_sums(KstarRowSet a, KstarRowSet b, int32_t RT_a, int32_t RT_b,
                                                        KstarOperands<double> o, int32_t CT,
                                                        const double* __restrict__ cnorm, int64_t m,
                                                        int32_t* __restrict__ ticket, double* __restrict__ part,
                                                        double inv_s2) {
  constexpr int MAIN = 2 * K_STAGE, NS = NW > 0 ? NW : 1;
  static_assert(K_NT == 2 * K_BM && K_BM == K_BN, "one thread per epilogue operand (rowop)");
  static_assert(NW >= 0 && NW <= UT_CONS_MAX, "weight vectors per launch");
  // the ring, the exp table, the ticket slot, the item's |row|^2 and |u_c|^2, its w_q rows
  __shared__ __attribute__((aligned(16))) double lds[MAIN + EXP_TAB + 2 + (2 + NW) * K_BM];
  double* etab = lds + MAIN;
  int32_t& s_item = *reinterpret_cast<int32_t*>(lds + MAIN + EXP_TAB);
  double* const rowop = lds + MAIN + EXP_TAB + 2;
  const int t = threadIdx.x, lane0 = t & 63;
  if (t < EXP_TAB) etab[t] = exp2((double)t / EXP_TAB);   // published by the first ticket barrier
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = w >> 1, wn = w & 1;
  const int32_t xcd = blockIdx.x & 7;
  const int32_t RTt = RT_a + RT_b;
  const KstarRows rows = kstar_rows_f64(lane0);

  int32_t nxt = 0;
  kstar_draw(nxt, ticket, xcd);
  // (j uniform: the row set's pointers stay scalar)
  for (;;) {
    int32_t j;
    const int32_t ct = kstar_item<true>(nxt, s_item, xcd, RTt, j);
    if (ct >= CT) break;
    kstar_draw(nxt, ticket, xcd);
    const int lane = kstar_item_lane(lane0);
    const int32_t rtt = j % RTt;              // the partial's row in `part`
    const bool second = rtt >= RT_a;
    const KstarRowSet& R = second ? b : a;
    const int32_t rt = second ? rtt - RT_a : rtt;
    const int32_t nrows = R.n;
    const int64_t col0 = (int64_t)ct * K_BN;
    const int32_t row0 = rt * K_BM;
    KstarOperands<double> oi = o;
    oi.AT = R.AT, oi.lda = R.npad, oi.acat = R.acat, oi.npad_a = R.npad;
    const double* const norm = R.norm;
    const double* const wq = R.w;
    const int64_t ldw = R.npad;

    const KstarAcc<double> acc = kstar_contract<double, CAT>(oi, rows, row0, col0, lds, w, lane, [=] {
#pragma unroll
      for (int op = 0; op < 2 + NW; ++op) {
        if ((op & 3) != w) continue;
        const double* src = op == 0 ? norm + row0 : op == 1 ? cnorm + col0 : wq + (int64_t)(op - 2) * ldw + row0;
        __builtin_amdgcn_global_load_lds(src + lane * 2, (__attribute__((address_space(3))) void*)(rowop + op * K_BM),
                                         16, 0, 0);
      }
    });

    __syncthreads();  // ring free: reuse as the column reduction buffer
    // the item's half-norms once per item, not once per element (as k_gp_kstar<int8_t> keeps
    // its rows'): -1e300 for a padding row (>= n of its set) or column (>= m), whose k is
    // then exactly 0 without a select in the element code
    {
      double hv = (-0.5 * KSTAR_T_SCALE) * rowop[t];
      if constexpr (SCALED) hv = hv * inv_s2;
      const bool in = t < K_BM ? row0 + t < nrows : col0 + (t - K_BM) < m;
      rowop[t] = in ? hv : -1e300;
    }
    __syncthreads();
    double hc[4];
#pragma unroll
    for (int jj = 0; jj < 4; ++jj) {
      const int cl = wn * 64 + jj * 16 + (lane & 15);
      hc[jj] = rowop[K_BM + cl];
    }
    double s[NS][4];
#pragma unroll
    for (int q = 0; q < NS; ++q)
#pragma unroll
      for (int jj = 0; jj < 4; ++jj) s[q][jj] = 0.0;
#pragma unroll
    for (int i = 0; i < 4; ++i) {
#pragma unroll
      for (int r = 0; r < 4; ++r) {
        const int rl = wm * 64 + i * 16 + (lane >> 4) + 4 * r;
        const double hx = rowop[rl];
        double wr[NS];
        if constexpr (NW > 0) {
#pragma unroll
          for (int q = 0; q < NW; ++q) wr[q] = rowop[(2 + q) * K_BM + rl];
        }
#pragma unroll
        for (int jj = 0; jj < 4; ++jj) {
          // t = (C - |x|^2/2 - |u|^2/2) [/ s^2] * 256 / ln 2, clamped to [-1000 * 256 / ln 2, 0]
          double c = acc.a[i][jj][r];
          if constexpr (SCALED) c = c * inv_s2;
          const double x = __builtin_fmax(__builtin_fmin((c + hx) + hc[jj], 0.0), KSTAR_T_MIN);
          const double k = sf2_exp2t_nonpos(x, etab);
          if constexpr (NW > 0) {
#pragma unroll
            for (int q = 0; q < NW; ++q) s[q][jj] = __builtin_fma(k, wr[q], s[q][jj]);
          } else {
            s[0][jj] += k;
          }
        }
      }
    }
    kstar_sums_done(s);
    kstar_colsums<NS>(s, lds, lane, w, [=](int q, double v) {   // red [NS][2][128]
      const int64_t col = col0 + t;
      if (col < m) part[((int64_t)rtt * NS + q) * o.ldb + col] = v;
    });
  }
}

template <bool CAT>
static void launch_sums(ut_ctx* c, int32_t nw, int32_t nb, const KstarRowSet& a, const KstarRowSet& b,
                        const KstarOperands<double>& o, int32_t CT, const double* cnorm, int64_t m, double* part,
                        double inv_s2) {
#define UT_SUMS_LAUNCH(NW, SCALED)                                                                               \
  hipLaunchKernelGGL((k_kstar_sums<CAT, NW, SCALED>), dim3(nb), dim3(K_NT), 0, c->stream, a, b, a.npad / K_BM,    \
                     b.npad / K_BM, o, CT, cnorm, m, c->gp_ctr.p + 8, part, inv_s2)
  switch (nw) {
    case 0: UT_SUMS_LAUNCH(0, true); break;
    case 1: UT_SUMS_LAUNCH(1, false); break;
    case 2: UT_SUMS_LAUNCH(2, false); break;
    case 3: UT_SUMS_LAUNCH(3, false); break;
    default: UT_SUMS_LAUNCH(4, false); break;
  }
#undef UT_SUMS_LAUNCH
}

int launch_kstar_sums(ut_ctx* c, const char* who, const ScoreShape& s, const CandOps& u, int64_t m, const double* w,
                      int32_t nw, const KstarRowSet& b, double inv_s2, double* part) {
  const KstarTrain tr = kstar_train(c, s.cat, u.bcat);
  int rc;
  if ((rc = kstar_check(c, who, s.npad, s.dpad, u.ld, m, tr.cat))) return rc;
  const KstarRowSet a{tr.XsT, tr.xnorm ? tr.xnorm : c->gp_xnorm.p, tr.cat.acat, w, s.n, s.npad};
  const int32_t CT = (int32_t)(u.ld / K_BN);
  int32_t nb;
  if ((rc = kstar_grid(c, (int64_t)(a.npad + b.npad) / K_BM * CT, true, &nb))) return rc;
  const KstarOperands<double> o = kstar_operands<double>(tr.XsT, u.ucand, tr.cat, s.npad, u.ld, s.dpad);
  if (tr.cat.nkc > 0)
    launch_sums<true>(c, nw, nb, a, b, o, CT, u.cnorm, m, part, inv_s2);
  else
    launch_sums<false>(c, nw, nb, a, b, o, CT, u.cnorm, m, part, inv_s2);
  UT_LAUNCH_CHECK(c);
  return 0;
}

}  // namespace ut
