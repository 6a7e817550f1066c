// gp_i8.hip -- the fp64-tier variance contraction on the int8 MFMA
// (ut_gp_set_precision(ctx, 8); "Ozaki" slicing with exact int32 accumulation).
//
// The variance needs |v|^2 with v = L^-1 k* for every candidate, an n x n by
// n x m contraction (gp_gemm.hip k_gp_var_pp on the fp64 MFMA).  Here both
// operands are cut into S = 6 signed 8-bit digit planes and the contraction
// runs on v_mfma_i32_32x32x32_i8 (64x the fp64 MFMA's rate per CU):
//
//   row i of L^-1:  x_ik = L^-1_ik 2^-ea_i  (power of two: |x| <= 0.49)
//   column c of K*: y_kc = k*_kc 2^-eb      (eb from sf2 >= k*: |y| <= 0.49)
//   X = rint(x 2^48) = sum_{p=1..6} a_p 256^(6-p), a_p in [-128, 127] ("balanced"
//   digits: the bytes of X + 0x808080808080, each XOR 0x80, taken from the bits
//   of the fp64 sum x + 24.50196..., whose ulp is 2^-48 -- i8_biased), Y likewise.
//   x y ~ sum_{p+q <= 7} a_p b_q 2^-8(p+q):  21 of the 36 digit products, in
//   six groups g = p + q whose int32 sums T_g = sum_k sum_{p+q=g} a_p b_q are
//   exact (|a b| <= 2^14, at most 6 pairs per group: K < 2^14 rows keep every
//   T_g below 2^31), and
//   v_ic = 2^(ea_i + eb) 2^-16 (T_2 + 2^-8 (T_3 + ... + 2^-8 T_7))   in fp64.
//
// Error (per element, in units of 2^(ea_i + eb)): the digit rounding of x and y
// (|dx|, |dy| <= 2^-49, times |y|, |x| <= 0.4901) and the dropped pairs
// p + q >= 8 (<= 2^14 (5 2^-64 + 4 2^-72 + ...) < 5.02 2^-50) stay below
// C = 3.5 2^-49, so |v_ic - v^_ic| <= e_i = (i + 1) C 2^(ea_i + eb) for every
// candidate, and |v - v^| <= E = |e|_2 (k_i8_errsum).  With s = |v^|^2 the
// exact |v|^2 lies within E (2 |v^| + E) of s, plus the fp64 rounding of the
// recombination and the sums (< s (2n + 64) 2^-53).  k_gp_finalize_i8 (gp_score.hip)
// accepts a candidate when that bound is <= tau * (sf2 - s) (tau: ut_gp_set_i8_tol,
// default 2^-20), i.e. its variance is within tau relative of the exact one;
// every other candidate -- next to a training point, where sf2 - |v|^2 is a
// cancellation -- is recomputed in fp64 (gp_score.hip gp_score_impl).  The mean
// is mu^ = v^ . L^-1 y from k_gp_var_i8's epilogue (K* computes none), with
// |mu - mu^| <= Emu = sum_r e_r |(L^-1 y)_r| (k_i8_errsum): a candidate is
// accepted only if Emu <= tau * sigma as well.
//
// Layouts (bytes): A = [6][npad/32][npad][32] (L^-1 rows), B = [6][npad/32][ldk][32]
// (written by k_gp_kstar_q, gp_kq.hip, for numeric fits; by k_gp_kstar<int8_t>
// under UT_KSTAR_Q=0 and for categorical fits); row / candidate r's 16-byte
// chunk c of a 32-k piece sits at position c ^ ((r >> 3) & 1), so the 32x32x32
// MFMA's fragment reads (32 rows x 2 chunks per ds_read_b128) hit distinct banks.
// k_gp_kstar_q also writes B's plane-occupancy mask, kmask [npad/32][ldk/32]
// bytes: bit p set iff plane p of that 32-k x 32-candidate block holds a
// non-zero digit (one k stage of a 128-candidate strip: one aligned dword).
// K* has one exponent for the whole fit, so an element below 2^-9 of sf2's
// scale has a zero top digit and one below 2^-49 six zero digits: far from the
// data (short lengthscales) whole blocks of planes are zero, and
// k_gp_var_i8<true> neither loads them nor issues their MFMAs.  A product with
// an all-zero operand adds exact zeros to an exact int32 sum: no output bit
// changes, and the error contract above is the unmasked kernel's.  The masked
// kernel's guarded MFMA groups cost a dense K* about 3 %, so it runs only
// while the last call's K* was sparse (I8Hints::var_skip, gp_i8_plan.h).
// After a screened K* (k_q_screen, gp_kq.hip) the planes behind cleared mask
// dwords were not written at all: the masked kernel always runs then.  Where
// the plan expects few live strips (I8Hints::list: 7 blocks in 8 of the
// last call all-zero, or UT_KSTAR_STRIPS=1) it is the instance <true, true>
// over the screen's list of strips with a live unit (the other strips'
// partials already hold their zeros); otherwise <true> over every strip, which
// gives the same bits and is the faster instance per live strip.  i8_plan
// (gp_i8_plan.h) chooses among the three; launch_gemm_var_i8 runs the one named.
#include "ut_internal.h"

namespace ut {

constexpr int I8_PL = I8_BM * I8_BK;   // one plane's piece of a stage: 64 rows x 32 k = 2 KiB
constexpr double I8_C = 3.5 * 0x1p-49;

// a wave-uniform 64-bit value, said so to the compiler (it then stays in SGPRs)
__device__ __forceinline__ uint64_t i8_uniform64(uint64_t v) {
  return ((uint64_t)(uint32_t)__builtin_amdgcn_readfirstlane((int32_t)(v >> 32)) << 32) |
         (uint32_t)__builtin_amdgcn_readfirstlane((int32_t)v);
}

template <int N>
__device__ __forceinline__ void i8_vm_wait() {
  static_assert(N >= 0 && N < 64, "vmcnt");
  __builtin_amdgcn_s_waitcnt((N & 15) | ((N >> 4) << 14) | (7 << 4) | (15 << 8));
}

// ---------------------------------------------------------------------------
// fit side: L^-1 -> digit planes, row scales 2^(ea_i + eb), e_i^2
// one 256-thread workgroup per padded row; thread t digitises k = 4t .. 4t + 3
// (+ 1024 j), one dword per plane
// ---------------------------------------------------------------------------
__global__ __launch_bounds__(256) void k_split_i8(const double* __restrict__ Linv, int32_t n, int32_t npad,
                                                  int32_t eb, int8_t* __restrict__ A, double* __restrict__ rs,
                                                  double* __restrict__ e2) {
  __shared__ double red[4];
  const int32_t r = blockIdx.x;
  const int t = threadIdx.x;
  const int32_t kend = r < n ? r + 1 : 0;   // L^-1 row r is zero past the diagonal
  const double* row = Linv + (int64_t)r * npad;
  double mx = 0.0;
  for (int32_t k = t; k < kend; k += 256) mx = fmax(mx, fabs(row[k]));
  for (int o = 32; o > 0; o >>= 1) mx = fmax(mx, __shfl_xor(mx, o));
  if ((t & 63) == 0) red[t >> 6] = mx;
  __syncthreads();
  mx = fmax(fmax(red[0], red[1]), fmax(red[2], red[3]));
  // 2^ea >= mx / 0.49: |x| <= 0.49 (to the rounding of the quotient)
  const int32_t ea = mx > 0.0 ? ilogb(mx / 0.49) + 1 : 0;
  const int64_t plane = (int64_t)npad * npad;
  for (int32_t k0 = 4 * t; k0 < npad; k0 += 1024) {
    uint32_t lo[4], hi[4];
#pragma unroll
    for (int u = 0; u < 4; ++u) {
      const double v = k0 + u < kend ? row[k0 + u] : 0.0;
      const uint64_t b = i8_biased(__builtin_ldexp(v, -ea));
      lo[u] = (uint32_t)b;
      hi[u] = (uint32_t)(b >> 32);
    }
    uint32_t pl[I8_S];
    i8_planes(lo, hi, pl);
    const int64_t o = i8_off(r, k0, npad);
#pragma unroll
    for (int p = 0; p < I8_S; ++p) *reinterpret_cast<uint32_t*>(A + p * plane + o) = pl[p];
  }
  if (t == 0) {
    const bool live = kend > 0 && mx > 0.0;
    const double sc = live ? __builtin_ldexp(1.0, ea + eb) : 0.0;
    rs[r] = sc;
    const double e = (double)kend * I8_C * sc;
    e2[r] = e * e;
  }
}

// E = sqrt(sum_r e2[r]) and Emu = sum_r e_r |beta_r| (beta = L^-1 y; one
// workgroup, fixed order), both rounded up.  The mean comes from the variance
// epilogue, mu^ = v^ . beta, so |mu - mu^| <= sum_r |v_r - v^_r| |beta_r| <= Emu.
__global__ __launch_bounds__(256) void k_i8_errsum(const double* __restrict__ e2, const double* __restrict__ beta,
                                                   int32_t npad, double* __restrict__ E) {
  __shared__ double red[2][4];
  const int t = threadIdx.x;
  double s = 0.0, sm = 0.0;
  for (int32_t r = t; r < npad; r += 256) {
    s += e2[r];
    sm = __builtin_fma(sqrt(e2[r]), fabs(beta[r]), sm);
  }
  for (int o = 32; o > 0; o >>= 1) {
    s += __shfl_xor(s, o);
    sm += __shfl_xor(sm, o);
  }
  if ((t & 63) == 0) {
    red[0][t >> 6] = s;
    red[1][t >> 6] = sm;
  }
  __syncthreads();
  if (t == 0) {
    E[0] = sqrt((red[0][0] + red[0][1]) + (red[0][2] + red[0][3])) * (1.0 + 0x1p-40);
    E[1] = ((red[1][0] + red[1][1]) + (red[1][2] + red[1][3])) * (1.0 + 0x1p-40);
  }
}

int alloc_split_i8(ut_ctx* c, int32_t npad) {
  int rc;
  if ((rc = ensure(c, c->gp_i8a, (size_t)I8_S * npad * npad))) return rc;
  return ensure(c, c->gp_i8rs, (size_t)2 * npad + 2);   // [rs | e2 | E | Emu]
}

int launch_split_i8(ut_ctx* c, int32_t n, int32_t npad) {
  UT_CHECK(c, c->gp_i8a.n >= (size_t)I8_S * npad * npad && c->gp_i8rs.n >= (size_t)2 * npad + 2, UT_EINVAL,
           "split_i8: planes not allocated (alloc_split_i8)");
  double* rs = c->gp_i8rs.p;
  hipLaunchKernelGGL(k_split_i8, dim3(npad), dim3(256), 0, c->stream, c->gp_Linv.p, n, npad, c->gp_i8_eb,
                     c->gp_i8a.p, rs, rs + npad);
  hipLaunchKernelGGL(k_i8_errsum, dim3(1), dim3(256), 0, c->stream, rs + npad, c->gp_beta.p, npad, rs + 2 * npad);
  UT_LAUNCH_CHECK(c);
  return 0;
}

// ---------------------------------------------------------------------------
// the contraction: part[rt][col] = sum_{rows of tile rt} v^_{row,col}^2
//
// Persistent, TWO 256-thread workgroups per CU (one's barrier waits and
// epilogue overlap the other's MFMAs, as k_gp_var_pp); a work item is the
// row-tile pair (RT - 1 - p, p) of one 128-candidate strip (every item the
// same length), handed out per XCD in groups of P pairs x Sg strips so the
// group shares each L^-1 stage through L2.  The pair's second (short) tile
// walks its k stages in descending order: at every step the strip's P
// workgroups then read at most two distinct K* stages, the rest L2 hits.
// Tile 64 rows x 128 candidates; waves 2 x 2 of 32 rows x 64 candidates (two
// 32 x 32 MFMA column tiles share the wave's A fragments; B planes streamed
// one at a time); a 2-stage ring of 32-k stages (6 A planes x 2 KiB + 6 B
// planes x 4 KiB = 36 KiB), filled by global_load_lds (9 per wave per stage).
// The wave's rows [32 wm, +32) see zeros once k passes them (L^-1 is lower
// triangular): those stages skip their MFMAs.  Probe on random digits
// (scripts/exp/i8var_probe.hip, n = 1024, m = 2^20): 9.26 ms against 10.0 for
// 64-candidate tiles with a 3-stage ring.
//
// MASK (k_gp_kstar_q's occupancy mask, npad <= I8_MASK_MAX_K): lane l of every
// wave fetches the strip's mask dword of k stage l once per item (both tiles
// of the pair share the strip) and ORs its four bytes into a 6-bit stage mask;
// a ballot gives the live stages as one 64-bit scalar set, and a live stage's
// mask comes back by readlane, so the loop stays scalar-uniform.  A tile walks
// its live stages only (ascending, the short tile descending, the next live
// one prefetched into the other ring slot).  K* is non-negative under one
// exponent, so a block's zero planes are its leading ones: a stage whose first
// plane with a digit is q0 loads and multiplies B planes q0 .. 5 only (and the
// A planes they meet: pa + qb < 6), a stage with q0 = 0 issues the unmasked
// loads and all 21 products, and a tile with no live stage writes the zeros
// that zero accumulators give.  (A zero plane behind a non-zero one is loaded
// and multiplied as the zeros it holds.)
// ---------------------------------------------------------------------------
constexpr int I8_WN = 128;                 // candidates per tile
constexpr int I8_BPL = I8_WN * I8_BK;      // one B plane's piece of a stage (4 KiB)

template <bool MASK, bool SLIST = false>
__global__ __launch_bounds__(256, 2) void k_gp_var_i8(const int8_t* __restrict__ Ad, const int8_t* __restrict__ Bd,
                                                      int32_t npad, int64_t ldk, int32_t RT, int32_t CT, int64_t m,
                                                      int32_t* __restrict__ ticket, const double* __restrict__ rs,
                                                      const double* __restrict__ beta, double* __restrict__ part,
                                                      double* __restrict__ mpart, int32_t Sg,
                                                      const uint8_t* __restrict__ kmask) {
  constexpr int STAGE = I8_S * (I8_PL + I8_BPL);
  constexpr int NW = 6 * I8_S / 4;   // glds per wave per stage
  __shared__ __attribute__((aligned(16))) int8_t lds[2 * STAGE + 4 * I8_WN * 8 + 2 * I8_BM * 8 + 16];
  double* red = reinterpret_cast<double*>(lds + 2 * STAGE);   // [2][128] sums of v^2, [2][128] of v beta
  double* srs = red + 4 * I8_WN;                               // row scales of the tile
  double* sbt = srs + I8_BM;                                   // beta of the tile's rows
  int32_t& s_item = *reinterpret_cast<int32_t*>(sbt + I8_BM);
  const int t = threadIdx.x, lane = t & 63;
  const int w = __builtin_amdgcn_readfirstlane(t >> 6);
  const int wm = w >> 1, wn = w & 1;
  const int32_t xcd = __builtin_amdgcn_readfirstlane(blockIdx.x & 7);
  const int64_t aplane = (int64_t)npad * npad, bplane = (int64_t)npad * ldk;

  // stage kt of tile (row0, col0): A planes 2 KiB (2 pieces), B planes 4 KiB (4 pieces);
  // wave w moves pieces w + 4j
  // (all_c false: only the B planes from q0 on, and the A planes pa that meet
  // one of them in a product, pa + q0 < 6)
  auto issue = [&](int32_t row0, int64_t col0, int32_t kt, int8_t* st, auto all_c, int q0) {
    constexpr bool ALL = decltype(all_c)::value;
#pragma unroll
    for (int j = 0; j < NW; ++j) {
      const int u = w + 4 * j;
      const int8_t* src;
      int8_t* dst;
      bool need;
      if (u < 2 * I8_S) {
        const int pl = u >> 1, h = u & 1;
        src = Ad + pl * aplane + ((int64_t)kt * npad + row0) * 32 + h * 1024;
        dst = st + pl * I8_PL + h * 1024;
        need = ALL || pl + q0 < I8_S;
      } else {
        const int v = u - 2 * I8_S, pl = v >> 2, h = v & 3;
        src = Bd + pl * bplane + ((int64_t)kt * ldk + col0) * 32 + h * 1024;
        dst = st + I8_S * I8_PL + pl * I8_BPL + h * 1024;
        need = ALL || pl >= q0;
      }
      if constexpr (ALL)
        __builtin_amdgcn_global_load_lds(src + lane * 16, (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
      else if (need)
        __builtin_amdgcn_global_load_lds(src + lane * 16, (__attribute__((address_space(3))) void*)dst, 16, 0, 0);
    }
  };
  constexpr std::integral_constant<bool, true> all_planes{};
  constexpr std::integral_constant<bool, false> live_planes{};

  const int32_t P = (RT + 1) / 2;
  const int c = lane >> 5;
  const int ra = wm * 32 + (lane & 31);
  const int aoff = ra * 32 + ((c ^ ((ra >> 3) & 1)) << 4);
  int boff[2];
#pragma unroll
  for (int jj = 0; jj < 2; ++jj) {
    const int cb = wn * 64 + jj * 32 + (lane & 31);
    boff[jj] = I8_S * I8_PL + cb * 32 + ((c ^ ((cb >> 3) & 1)) << 4);
  }
  for (;;) {
    if (t == 0) {
      const int32_t it = atomicAdd(&ticket[xcd], 1);
      s_item = it;
      if constexpr (SLIST) {
        // a strip list (k_q_screen's): the XCD's live strips in the list's order,
        // the others hold their zeros already; past its end CT, so that the
        // workgroup leaves (with no live strip after one ticket).  The list sits
        // behind the mask's bytes, [8 counts][8][ceil(CT / 8)] strips, and thread 0
        // looks the strip up beside the ticket, in an instance of its own: read
        // through pointer arguments by every wave it cost the plain masked kernel
        // 9 more spilled SGPRs and 18 % at ell = 0.5.
        const int32_t* tail = reinterpret_cast<const int32_t*>(kmask + (int64_t)(npad >> 5) * (ldk >> 5));
        const int32_t P_ = (RT + 1) / 2;
        const int32_t si = (it / (P_ * Sg)) * Sg + (it % (P_ * Sg)) / P_;
        (&s_item)[1] = si < tail[xcd] ? tail[8 + xcd * ((CT + 7) >> 3) + si] : CT;
      }
    }
    __syncthreads();
    // (every item quantity scalar: the glds bases and loop bounds in SGPRs)
    const int32_t j = __builtin_amdgcn_readfirstlane(s_item);
    const int32_t G = j / (P * Sg), q = j % (P * Sg), p = q % P;
    const int32_t ct =
        SLIST ? __builtin_amdgcn_readfirstlane((&s_item)[1]) : (G * Sg + q / P) * 8 + xcd;
    if (ct >= CT) break;   // uniform: the whole workgroup leaves
    const int nrt = RT - 1 - p == p ? 1 : 2;
    // lane l: the 6-bit mask of k stage l of this strip (the long tile's stages
    // include the short tile's); live: the stages with any plane
    uint32_t m6 = 0;
    uint64_t live = 0;
    uint32_t dw = 0;   // (the fetch is issued here and first read in the long tile, below)
    if constexpr (MASK) {
      const int32_t nkl = (RT - p) * (I8_BM / I8_BK);   // <= 64
      if (lane < nkl) dw = *reinterpret_cast<const uint32_t*>(kmask + (int64_t)lane * (ldk >> 5) + ct * 4);
    }
    for (int ri = 0; ri < nrt; ++ri) {
      if (ri > 0) __syncthreads();   // the previous tile's ring, red and srs are read
      const int32_t rt = __builtin_amdgcn_readfirstlane(ri == 0 ? RT - 1 - p : p);
      const int32_t row0 = rt * I8_BM;
      const int64_t col0 = (int64_t)ct * I8_WN;
      const int32_t nk = (row0 + I8_BM) / I8_BK;   // >= 2
      const bool rev = ri > 0;
      auto ktof = [&](int32_t u) -> int32_t { return rev ? nk - 1 - u : u; };
      uint64_t lv = 0;   // (MASK) the tile's live stages not yet issued
      if constexpr (MASK) {
        if (ri == 0) {   // (the fetch's first use: the wave waits for it here)
          dw |= dw >> 16;
          m6 = (dw | (dw >> 8)) & 0x3fu;
          live = i8_uniform64(__builtin_amdgcn_ballot_w64(m6 != 0));
        }
        lv = i8_uniform64(live & (nk >= 64 ? ~0ull : (1ull << nk) - 1));
        if (lv == 0) {
          // no live stage: what zero accumulators give.  (The barrier: a one-tile
          // item has none otherwise between reading s_item and the next ticket.)
          if (ri == 0) __syncthreads();
          if (t < I8_WN) {
            const int64_t col = col0 + t;
            if (col < m) {
              part[(int64_t)rt * ldk + col] = 0.0;
              mpart[(int64_t)rt * ldk + col] = 0.0;
            }
          }
          continue;
        }
      }
      i8v16 acc[2][I8_S];
#pragma unroll
      for (int jj = 0; jj < 2; ++jj)
#pragma unroll
        for (int g = 0; g < I8_S; ++g)
#pragma unroll
          for (int r = 0; r < 16; ++r) acc[jj][g][r] = 0;
      if (w < 2 && lane < 32)   // 64 row scales / betas: one 512-B glds each, retired with stage 0
        __builtin_amdgcn_global_load_lds((w == 0 ? rs : beta) + row0 + lane * 2,
                                         (__attribute__((address_space(3))) void*)(w == 0 ? srs : sbt), 16, 0, 0);
      if constexpr (!MASK) {
        issue(row0, col0, ktof(0), lds, all_planes, 0);
        for (int32_t u = 0; u < nk; ++u) {
          i8_vm_wait<0>();                        // stage u landed (this wave's pieces)
          __builtin_amdgcn_s_barrier();           // every wave's stage u landed; stage u - 1 fully read
          asm volatile("" ::: "memory");
          if (u + 1 < nk) issue(row0, col0, ktof(u + 1), lds + ((u + 1) & 1) * STAGE, all_planes, 0);
          const int32_t kt = ktof(u);
          if (kt * I8_BK >= row0 + 32 * wm + 32) continue;   // rows of this wave: all zero here
          const int8_t* st = lds + (u & 1) * STAGE;
          i8v4 af[I8_S];
#pragma unroll
          for (int pp = 0; pp < I8_S; ++pp) af[pp] = *reinterpret_cast<const i8v4*>(st + pp * I8_PL + aoff);
#pragma unroll
          for (int qb = 0; qb < I8_S; ++qb) {
            i8v4 bf[2];
#pragma unroll
            for (int jj = 0; jj < 2; ++jj) bf[jj] = *reinterpret_cast<const i8v4*>(st + qb * I8_BPL + boff[jj]);
            // digit products of group g = pa + qb (0-based): pairs with (pa + 1) + (qb + 1) <= 7
#pragma unroll
            for (int pa = 0; pa + qb < I8_S; ++pa)
#pragma unroll
              for (int jj = 0; jj < 2; ++jj)
                acc[jj][pa + qb] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[pa], bf[jj], acc[jj][pa + qb], 0, 0, 0);
          }
        }
      } else {
        // the live stages in the tile's order; q0: a stage's first plane with a
        // digit.  K* is non-negative under one exponent, so a block's zero planes
        // are its leading ones: planes q0 .. 5 are loaded and multiplied (a zero
        // plane among them as the zeros it holds), planes 0 .. q0 - 1 neither.
        auto take = [&]() -> int32_t {
          const int32_t k = rev ? 63 - __builtin_clzll(lv) : __builtin_ctzll(lv);
          lv &= ~(1ull << k);
          return k;
        };
        auto issue_live = [&](int32_t k, int8_t* st, int q0) {   // (a dense stage: the unmasked loads)
          if (q0 == 0) issue(row0, col0, k, st, all_planes, 0);
          else issue(row0, col0, k, st, live_planes, q0);
        };
        int32_t kt = take();
        int q0 = __builtin_ctz(__builtin_amdgcn_readlane(m6, kt));
        issue_live(kt, lds, q0);
        for (int32_t u = 0;; ++u) {
          i8_vm_wait<0>();                        // this live stage landed (this wave's pieces)
          __builtin_amdgcn_s_barrier();           // ... in every wave; the one before it fully read
          asm volatile("" ::: "memory");
          const bool more = lv != 0;
          int32_t ktn = 0;
          int q0n = 0;
          if (more) {
            ktn = take();
            q0n = __builtin_ctz(__builtin_amdgcn_readlane(m6, ktn));
            issue_live(ktn, lds + ((u + 1) & 1) * STAGE, q0n);
          }
          if (kt * I8_BK < row0 + 32 * wm + 32) {   // (else: rows of this wave all zero here)
            // One body for every q0, its MFMA groups under scalar guards (a second,
            // unguarded body beside it made the compiler spill the accumulators
            // inside this loop; reading a plane's fragments ahead of its guard put
            // a scratch reload into the loads of a partly live stage).  An A plane
            // that was not loaded is read as stale bytes and meets no product.
            const int8_t* st = lds + (u & 1) * STAGE;
            i8v4 af[I8_S];
#pragma unroll
            for (int pp = 0; pp < I8_S; ++pp) af[pp] = *reinterpret_cast<const i8v4*>(st + pp * I8_PL + aoff);
#pragma unroll
            for (int qb = 0; qb < I8_S; ++qb) {
              if (qb < q0) continue;   // (scalar)
              i8v4 bf[2];
#pragma unroll
              for (int jj = 0; jj < 2; ++jj) bf[jj] = *reinterpret_cast<const i8v4*>(st + qb * I8_BPL + boff[jj]);
#pragma unroll
              for (int pa = 0; pa + qb < I8_S; ++pa)
#pragma unroll
                for (int jj = 0; jj < 2; ++jj)
                  acc[jj][pa + qb] = __builtin_amdgcn_mfma_i32_32x32x32_i8(af[pa], bf[jj], acc[jj][pa + qb], 0, 0, 0);
            }
          }
          if (!more) break;
          kt = ktn;
          q0 = q0n;
        }
      }
      // epilogue: v = 2^-16 (T_2 + 2^-8 (T_3 + ...)) * 2^(ea_row + eb), column sums
      // of v^2 and of v beta (the mean, mu = (L^-1 k*) . (L^-1 y))
      // (C/D map of the 32x32 MFMA: row (r & 3) + 8 (r >> 2) + 4 (lane >> 5), column lane & 31)
#pragma unroll
      for (int jj = 0; jj < 2; ++jj) {
        double s = 0.0, sm = 0.0;
#pragma unroll
        for (int r = 0; r < 16; ++r) {
          double v = (double)acc[jj][I8_S - 1][r];
#pragma unroll
          for (int g = I8_S - 2; g >= 0; --g) v = __builtin_fma(v, 0x1p-8, (double)acc[jj][g][r]);
          const int rr = wm * 32 + (r & 3) + 8 * (r >> 2) + 4 * (lane >> 5);
          v *= 0x1p-16 * srs[rr];
          s = __builtin_fma(v, v, s);
          sm = __builtin_fma(v, sbt[rr], sm);
        }
        s += __shfl_xor(s, 32);
        sm += __shfl_xor(sm, 32);
        if (lane < 32) {
          red[wm * I8_WN + wn * 64 + jj * 32 + lane] = s;
          red[2 * I8_WN + wm * I8_WN + wn * 64 + jj * 32 + lane] = sm;
        }
      }
      __syncthreads();
      if (t < I8_WN) {
        const int64_t col = col0 + t;
        if (col < m) {
          part[(int64_t)rt * ldk + col] = red[t] + red[I8_WN + t];
          mpart[(int64_t)rt * ldk + col] = red[2 * I8_WN + t] + red[3 * I8_WN + t];
        }
      }
    }
  }
}

int launch_gemm_var_i8(ut_ctx* c, int32_t npad, const int8_t* kst8, int64_t ldk, int64_t m, double* part,
                       double* mpart, I8Var var) {
  UT_CHECK(c, npad % 128 == 0 && npad <= I8_MAX_K && ldk % I8_WN == 0 && ldk >= m, UT_EINVAL,
           "gemm_var_i8: bad padding");
  const uint8_t* kmask = c->kmask.p;
  UT_CHECK(c, var == I8Var::Unmasked || (kmask && npad <= I8_MASK_MAX_K), UT_EINVAL,
           "gemm_var_i8: a masked kernel needs K*'s mask and at most 2048 training rows");
  UT_CHECK(c, c->gp_i8a.p && c->gp_i8rs.p, UT_EINVAL, "gemm_var_i8: the fit has no int8 planes");
  const int32_t RT = npad / I8_BM, CT = (int32_t)((m + I8_WN - 1) / I8_WN);
  const int32_t P = (RT + 1) / 2;
  const int64_t items = (int64_t)P * CT;
  int32_t nb = 2 * (c->n_cu / 8) * 8;   // two workgroups per CU, a multiple of 8 (every XCD group works)
  if (items < nb) nb = (int32_t)(((items + 7) / 8) * 8);
  const int32_t W = nb / 8, Sg = W / P > 1 ? W / P : 1;
  UT_HIP(c, hipMemsetAsync(c->gp_ctr.p, 0, sizeof(int32_t) * 8, c->stream));
  if (var == I8Var::MaskedList)
    hipLaunchKernelGGL((k_gp_var_i8<true, true>), dim3(nb), dim3(256), 0, c->stream, c->gp_i8a.p, kst8, npad, ldk, RT, CT,
                       m, c->gp_ctr.p, c->gp_i8rs.p, c->gp_beta.p, part, mpart, Sg, kmask);
  else if (var == I8Var::Masked)
    hipLaunchKernelGGL(k_gp_var_i8<true>, dim3(nb), dim3(256), 0, c->stream, c->gp_i8a.p, kst8, npad, ldk, RT, CT, m,
                       c->gp_ctr.p, c->gp_i8rs.p, c->gp_beta.p, part, mpart, Sg, kmask);
  else
    hipLaunchKernelGGL(k_gp_var_i8<false>, dim3(nb), dim3(256), 0, c->stream, c->gp_i8a.p, kst8, npad, ldk, RT, CT, m,
                       c->gp_ctr.p, c->gp_i8rs.p, c->gp_beta.p, part, mpart, Sg, nullptr);
  UT_LAUNCH_CHECK(c);
  return 0;
}

// (for tests: ut_gp_kstar_read) K*'s digit planes back to doubles: element
// (training row r, candidate col) has digit p at kst8[p npad ldk + i8_off(col,
// r, ldk)], plane 0 the most significant; k* = (sum_p d_p 256^(5-p)) scale
// with scale = 2^(eb - 48): a 48-bit integer times a power of two, exact.
// out [npad][nc], columns c0 .. c0 + nc - 1.
__global__ __launch_bounds__(256) void k_i8_kstar_decode(const int8_t* __restrict__ kst8, int32_t npad, int64_t ldk,
                                                         int64_t c0, int64_t nc, double scale,
                                                         double* __restrict__ out,
                                                         const uint8_t* __restrict__ kmask) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)npad * nc) return;
  const int32_t r = (int32_t)(e / nc);
  const int64_t j = e - (int64_t)r * nc;
  const int64_t plane = (int64_t)npad * ldk, off = i8_off(c0 + j, r, ldk);
  int64_t v = 0;
  // (a plane whose mask bit is clear holds no digit: after a screened call it was not even written)
  const uint32_t mk = kmask ? kmask[(int64_t)(r >> 5) * (ldk >> 5) + ((c0 + j) >> 5)] : 0x3fu;
#pragma unroll
  for (int p = 0; p < I8_S; ++p) v = v * 256 + (((mk >> p) & 1u) ? (int64_t)kst8[p * plane + off] : 0);
  out[e] = (double)v * scale;
}

int launch_kstar_decode_i8(ut_ctx* c, const int8_t* kst8, int32_t npad, int64_t ldk, int64_t c0, int64_t nc,
                           double* out, const uint8_t* kmask) {
  UT_CHECK(c, npad % 32 == 0 && c0 >= 0 && nc >= 0 && c0 + nc <= ldk, UT_EINVAL, "kstar_decode_i8: bad range");
  if (nc == 0) return 0;
  hipLaunchKernelGGL(k_i8_kstar_decode, dim3(grid1((int64_t)npad * nc, 256)), dim3(256), 0, c->stream, kst8, npad,
                     ldk, c0, nc, ldexp(1.0, i8_kstar_exp(c->gp_sf2) - 48), out, kmask);
  UT_LAUNCH_CHECK(c);
  return 0;
}

// (for tests: ut_gp_fit_read) L^-1's digit planes back to integers: element
// (row r, k) has digit p at A[p npad^2 + i8_off(r, k, npad)], plane 0 the most
// significant; out [npad][npad] = sum_p d_p 256^(5-p), below 2^47 in magnitude: exact
__global__ __launch_bounds__(256) void k_i8_linv_decode(const int8_t* __restrict__ A, int32_t npad,
                                                        double* __restrict__ out) {
  const int64_t e = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (e >= (int64_t)npad * npad) return;
  const int32_t r = (int32_t)(e / npad), k = (int32_t)(e - (int64_t)r * npad);
  const int64_t plane = (int64_t)npad * npad, off = i8_off(r, k, npad);
  int64_t v = 0;
#pragma unroll
  for (int p = 0; p < I8_S; ++p) v = v * 256 + (int64_t)A[p * plane + off];
  out[e] = (double)v;
}

int launch_linv_decode_i8(ut_ctx* c, int32_t npad, double* out) {
  UT_CHECK(c, npad % 32 == 0 && c->gp_i8a.p && c->gp_i8a.n >= (size_t)I8_S * npad * npad, UT_EINVAL,
           "linv_decode_i8: the fit has no int8 planes");
  hipLaunchKernelGGL(k_i8_linv_decode, dim3(grid1((int64_t)npad * npad, 256)), dim3(256), 0, c->stream, c->gp_i8a.p,
                     npad, out);
  UT_LAUNCH_CHECK(c);
  return 0;
}

}  // namespace ut
