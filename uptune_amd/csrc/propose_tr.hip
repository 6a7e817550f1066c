// propose_tr.hip -- trust-region proposals (ut_propose_tr; the rule is stated
// in include/uthot.h and restated in numpy by tests/_tr_oracle.py).
//
// Every candidate lies in a box around one centre row and moves a random
// subset of the parameters.  As in propose.hip: one lane = one candidate, the
// parameter loop is wave-uniform (DevParam, the centre's value and the box
// faces are scalar loads), values are SoA columns, so each store of a wave is
// one coalesced 512-byte access.  Bound: HBM writes (8 * ncols bytes per
// candidate); nothing but the output is read per candidate.
//
// k_tr_box computes the centre's unit value and the clipped box faces once
// per call and parameter ([P] each), which keeps LOGINT's py_log2 (a table
// log plus a division) out of the per-candidate loop; a selected LOGINT still
// pays set_unit_value's exp2_cr.  Block A is drawn for every (candidate,
// parameter), block B only by the lanes that selected the parameter.
// Compiled with -ffp-contract=off, like ut_param.h.
#include "ut_param.h"
#include "ut_perm.h"

namespace ut {

// box [3][P]: h (in) | lo | hi (out)
__global__ __launch_bounds__(64) void k_tr_box(const DevParam* __restrict__ params, int32_t P,
                                               const double* __restrict__ vtab, const double* __restrict__ centre,
                                               double* __restrict__ box) {
  const int32_t p = blockIdx.x * blockDim.x + threadIdx.x;
  if (p >= P) return;
  const DevParam pr = params[p];
  double lo = 0.0, hi = 0.0;
  if (is_primitive(pr.kind)) {
    const double uc = unit_of(pr, centre[pr.col], vtab), h = box[p];
    lo = py_max(__dsub_rn(uc, h), 0.0);
    hi = py_min(__dadd_rn(uc, h), 1.0);
  }
  box[P + p] = lo;
  box[2 * P + p] = hi;
}

__global__ __launch_bounds__(256) void k_tr(const DevParam* __restrict__ params, int32_t P,
                                            const double* __restrict__ centre, const double* __restrict__ box,
                                            double prob, double cat_prob, int32_t must, uint64_t seed, uint32_t round_,
                                            int64_t cand_base, int64_t m, double* __restrict__ out, int64_t ldo,
                                            uint8_t* __restrict__ invalid) {
  const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
  if (i >= m) return;
  const uint64_t g = (uint64_t)(cand_base + i);
  double sel = 0.0;
  bool moved = false;   // some column differs bitwise from the centre's
  for (int32_t p = 0; p < P; ++p) {
    const DevParam pr = params[p];
    const bool prim = is_primitive(pr.kind);
    const u32x4 a = draw(seed, g, (uint32_t)p, round_, OP_TR);
    bool pick = false;
    if ((double)(P - p) * u01_from(a.x, a.y) < (double)must - sel) {
      sel += 1.0;
      pick = true;
    }
    pick = pick || ((double)a.z * (1.0 / 4294967296.0) < (prim ? prob : cat_prob));
    const uint32_t sb = (uint32_t)p | (1u << STREAM_SUB_SHIFT);
    if (pr.kind == UT_PERM) {
      const int32_t S = pr.psize;
      const PRow c{centre + pr.col, 1};
      WRow o{out + (int64_t)pr.col * ldo + i, ldo};
      perm_copy(o, c, S);
      if (pick) {
        PermRng R(seed, g, sb, round_, OP_TR);
        perm_small_change(o, S, R);
        moved |= !perm_equal(o.ro(), c, S);
      }
      continue;
    }
    const double cv = centre[pr.col];
    double v = cv;
    if (pick) {
      if (prim) {
        const u32x4 b = draw(seed, g, sb, round_, OP_TR);
        const double lo = box[P + p], hi = box[2 * P + p];
        const double u = __dadd_rn(lo, __dmul_rn(__dsub_rn(hi, lo), u01_from(b.x, b.y)));
        v = __dadd_rn(from_unit(pr, u, cv), 0.0);   // (+ 0.0: rint(-0.3) = -0.0 is stored as the centre's +0.0)
      } else if (pr.kind == UT_BOOL) {
        v = 1.0 - cv;
      } else if (pr.n_opt > 1) {   // ENUM: uniform over the other options
        const u32x4 b = draw(seed, g, sb, round_, OP_TR);
        int64_t r = (int64_t)below64(u64_from(b.z, b.w), (uint64_t)(pr.n_opt - 1));
        r += (r >= (int64_t)cv) ? 1 : 0;
        v = (double)r;
      }
      moved |= d_to_bits(v) != d_to_bits(cv);
    }
    out[(int64_t)pr.col * ldo + i] = v;
  }
  invalid[i] = moved ? 0 : 1;
}

int launch_tr(ut_ctx* c, const ut_tr_params* a, const double* centre, const double* half_host, uint32_t round_,
              int64_t cand_base, int64_t m, double* out, int64_t ld, uint8_t* invalid) {
  const Space& s = c->space;
  int rc = ensure(c, c->tr_box, (size_t)3 * s.P);
  if (rc) return rc;
  UT_HIP(c, hipMemcpyAsync(c->tr_box.p, half_host, sizeof(double) * s.P, hipMemcpyHostToDevice, c->stream));
  hipLaunchKernelGGL(k_tr_box, dim3(grid1(s.P, 64)), dim3(64), 0, c->stream, s.d_params.p, s.P, s.d_vtab.p, centre,
                     c->tr_box.p);
  UT_LAUNCH_CHECK(c);
  hipLaunchKernelGGL(k_tr, dim3(grid1(m, 256)), dim3(256), 0, c->stream, s.d_params.p, s.P, centre, c->tr_box.p,
                     a->prob, a->cat_prob, a->must, c->seed, round_, cand_base, m, out, ld, invalid);
  UT_LAUNCH_CHECK(c);
  return 0;
}

}  // namespace ut

extern "C" int ut_propose_tr(ut_ctx* c, const ut_tr_params* a, const double* centre, const double* half_width_host,
                             uint32_t round_, int64_t cand_base, int64_t m, double* out_values, int64_t ld,
                             uint8_t* out_invalid) {
  if (!c) return UT_EINVAL;
  UT_CHECK(c, c->has_space, UT_ENOSPACE, "space not defined");
  UT_CHECK(c, a && centre && half_width_host, UT_EINVAL, "propose_tr: params, centre or half_width_host is NULL");
  UT_CHECK(c, m >= 0 && cand_base >= 0 && ld >= m && ((out_values && out_invalid) || m == 0), UT_EINVAL,
           "propose_tr: bad arguments");
  UT_CHECK(c, a->prob >= 0.0 && a->prob <= 1.0 && a->cat_prob >= 0.0 && a->cat_prob <= 1.0, UT_EINVAL,
           "propose_tr: prob and cat_prob must be in [0, 1]");
  UT_CHECK(c, a->must >= 0 && a->must <= c->space.P, UT_EINVAL, "propose_tr: must out of range");
  for (int32_t p = 0; p < c->space.P; ++p) {
    const double h = half_width_host[p];
    UT_CHECK(c, h >= 0.0 && h <= 1.7976931348623157e308, UT_EINVAL,
             "propose_tr: half-width of parameter " + std::to_string(p) + " is negative or not finite");
  }
  if (m == 0) return 0;
  // a staged fit is issued after the proposal (as ut_propose_ga)
  int rc;
  if ((rc = ut::gp_fit_prefit(c))) return rc;
  if ((rc = ut::launch_tr(c, a, centre, half_width_host, round_, cand_base, m, out_values, ld, out_invalid))) return rc;
  return ut::gp_fit_flush(c);
}
