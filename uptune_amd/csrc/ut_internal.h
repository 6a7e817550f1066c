// ut_internal.h -- context, device-side space description and launch
// helpers shared by the libuthot translation units.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include <algorithm>
#include <functional>
#include <initializer_list>
#include <string>
#include <type_traits>
#include <utility>
#include <vector>

#include "../../include/uthot.h"
#include "gp_i8_plan.h"
#include "ut_core.h"

namespace ut {

// Per-parameter record in device memory (uniform across a wave: every lane of
// a candidate-parallel kernel reads the same record, so these become scalar
// loads).
struct DevParam {
  int32_t kind;
  int32_t hash_mode;   // HM_LUT / HM_FLOAT / HM_INT / HM_LOGINT
  int64_t lut_base;    // first digest of this param in the LUT buffer
  int64_t lut_n;       // LUT entries (indices are clamped to [0, lut_n))
  double lo, hi;       // FLOAT/INT/LOGINT: stored-value bounds (min_value, max_value);
                       // POW2: exponent bounds (its legal_range, manipulator.py:829-830)
  double u_lo, u_hi;   // unit-encoding range of the searched value (get_value):
                       // widened for integer types; LOGINT: the scaled legal_range
  double u_span;       // u_hi - u_lo, rounded as Python rounds it
  int64_t n_opt;       // ENUM/BOOL option count
  int32_t feat_col;    // first GP feature column
  int32_t n_feat;      // GP feature columns of this param
  int64_t vtab_base;   // LOGINT: first entry of get_value(v) for v = lo.. in the value table
  int64_t vtab_n;      // LOGINT: table entries; 0 = compute the log on the device
  int32_t col;         // first SoA value column (PERM: `psize` columns of item indices)
  int32_t psize;       // PERM: permutation size S; 1 for every other kind
  int32_t wcol;        // PERM: first of its S columns in the GA parent workspace
  int32_t pslot;       // PERM: slot of its inner digest in the per-round perm digest buffer
  int32_t cslot;       // HM_FLOAT / HM_INT / HM_LOGINT (inner digest computed on the device):
                       // its slot in the population inner-digest cache; -1 otherwise
  int32_t pad_;
};

enum : int32_t { HM_LUT = 0, HM_FLOAT = 1, HM_INT = 2, HM_LOGINT = 3, HM_PERM = 4 };

// One 32-bit word of the fixed-layout outer hash message: the constant bytes
// plus, when the word overlaps a digest "hole", where its hex bytes come from
// in the kernel's 32-register hex array (hole j lives in slot j % 2).  8 bytes,
// read with scalar loads (every lane of a wave uses the same word).
struct HashWord {
  uint32_t tmpl;   // constant bytes (zero where hex characters go)
  uint32_t info;   // 0 = no hole; else HW_* fields
};
enum : uint32_t {
  HW_LO_VALID = 1u << 6,   // bits 0..4: hex register of the word's first bytes
  HW_HI_POS = 8,           // bits 8..12: hex register of its last bytes
  HW_HI_VALID = 1u << 14,
  HW_SHIFT_POS = 16,       // bits 16..20: left shift of the 64-bit concatenation, in bits
  HW_HOLE = 1u << 31,
};

// every device allocation of the library goes through these two (api.hip):
// the bytes held per device are what ut_device_bytes reports (a rank's HBM
// footprint in the bench line)
hipError_t dmalloc(void** p, size_t bytes);
void dfree(void* p);

// An owning device array: the destructor frees it, so a buffer that is a
// member of the context (or of a Space, a PopSlot) or a local needs no line
// anywhere else.  Move-only; never give one static storage duration (it would
// be freed after the HIP runtime has shut down).  Kernels take b.p.
template <class T>
struct DevBuf {
  T* p = nullptr;
  size_t n = 0;   // elements
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  DevBuf(DevBuf&& o) noexcept { swap(o); }
  DevBuf& operator=(DevBuf&& o) noexcept {
    swap(o);
    return *this;
  }
  ~DevBuf() { ut::dfree(p); }
  void swap(DevBuf& o) noexcept {
    std::swap(p, o.p);
    std::swap(n, o.n);
  }
  void reset() {
    ut::dfree(p);
    p = nullptr;
    n = 0;
  }
  // exactly `count` elements in place of what it held, outside the fault
  // injection's count (ensure() and dalloc() below are the counted ways).  The
  // caller waits for the context's streams first if the old array may be in use.
  hipError_t alloc(size_t count) {
    reset();
    const hipError_t e = ut::dmalloc((void**)&p, count * sizeof(T));
    if (e == hipSuccess) n = count;
    else p = nullptr;
    return e;
  }
};
static_assert(!std::is_copy_constructible<DevBuf<double>>::value && !std::is_copy_assignable<DevBuf<double>>::value,
              "DevBuf owns its array: two owners would free it twice");
static_assert(std::is_nothrow_move_constructible<DevBuf<double>>::value &&
                  std::is_nothrow_move_assignable<DevBuf<double>>::value,
              "DevBuf moves by exchanging p and n");

struct Space {
  int32_t P = 0;                          // parameters
  int32_t ncols = 0;                      // SoA value columns (P + sum over PERM of size - 1)
  int32_t n_perm = 0;                     // PERM parameters
  int32_t perm_cols = 0;                  // sum of PERM sizes
  int32_t perm_smax = 0;                  // largest PERM size
  int32_t n_feat = 0;
  int32_t py2 = 0;
  std::vector<DevParam> host_params;
  std::vector<int32_t> host_order;        // sorted position -> param index
  int64_t outer_len = 0;
  int64_t outer_blocks = 0;
  DevBuf<DevParam> d_params;
  DevBuf<int32_t> d_order;                // sorted position -> param index
  DevBuf<HashWord> d_words;               // outer_blocks * 16
  DevBuf<int32_t> d_block_last;           // last sorted position needed by each block
  DevBuf<uint32_t> d_lut;                 // digests as hex [*][16 words]
  DevBuf<double> d_vtab;                  // LOGINT get_value tables (host-computed by CPython)
  DevBuf<int32_t> d_order_col;            // sorted position -> first value column
  DevBuf<int32_t> d_perm_params;          // PERM param indices, by digest slot
  DevBuf<uint8_t> d_perm_bytes;           // concatenated repr(item) bytes of every PERM param
  DevBuf<int32_t> d_perm_off;             // per PERM param: S + 1 offsets into d_perm_bytes
  DevBuf<int32_t> d_perm_offbase;         // per PERM slot: first entry in d_perm_off
  DevBuf<int32_t> d_perm_len;             // per PERM slot: len(repr(list)) (constant per param)
  int32_t n_comp = 0;                     // params whose inner digest is computed (cslot >= 0)
  DevBuf<int32_t> d_comp;                 // cslot -> param index
  DevBuf<int32_t> d_col_param;            // value column -> its param (first column of a non-PERM param), or -1
  // categorical K* (gp_gemm.hip): ENUM / BOOL params are one-hot blocks of the
  // GP features, so their part of |x - u|^2 is (2 or 1) / ell^2 per mismatching
  // param -- an integer dot product of one-hot codes, taken on the int8 MFMA;
  // the other ("numeric") features go through the fp64 K* contraction
  int32_t n_cat = 0;                      // ENUM + BOOL params
  int32_t cat_k = 0;                      // int8 code columns (ENUM: n_opt, BOOL: 2), padded to 128
  int32_t n_num = 0;                      // numeric features
  std::vector<int32_t> host_cat;          // the ENUM / BOOL param indices
  std::vector<int32_t> host_num_feat;     // numeric k -> feature column
  DevBuf<int32_t> d_cat_ccol;             // per param: first code column (-1: numeric param)
  DevBuf<int32_t> d_num_feat;             // numeric k -> feature column
  DevBuf<int32_t> d_feat_num;             // feature column -> numeric k, or -1 (categorical)
};

// Per-stage device time of the scoring rounds: events are recorded while the
// rounds run and read only when a stage time is asked for, so timing adds no
// host synchronisation between rounds (consecutive rounds still overlap).
struct Timing {
  struct Mark {
    std::string name;   // "" = a stream's start point in its round, not reported
    hipStream_t stream;
    hipEvent_t ev;
    int64_t round;
  };
  bool on = false;
  bool in_round = false;   // inside ut_score_round_* (its stages share one round)
  int64_t round = 0;
  std::vector<Mark> marks;  // a stage's time = its mark - the previous mark of the round on the same stream
  std::vector<std::pair<std::string, std::pair<double, int64_t>>> totals;  // name -> (sum ms, rounds)
};

// What the last dense scoring call left in ut_ctx::kst (ut_gp_kstar_read and
// the other readers in api.hip).  fmt: 64 = fp64 rows [npad][ldk], 8 = six
// digit planes, -1 = the fp32 / f16x3 formats, 0 = nothing of the current fit
// (a fit, a pruned call or a failed dense call since).  masked: ut_ctx::kmask
// describes those planes -- k_gp_kstar_q's alone; k_gp_kstar<int8_t>
// (UT_KSTAR_Q=0, categorical fits) writes no mask.  After a screened call the
// planes behind cleared mask dwords hold whatever an earlier call left: every
// reader of masked planes goes through mask_of.
struct KstDesc {
  int32_t fmt = 0, npad = 0;
  int64_t ldk = 0;
  bool masked = false;
  void invalidate() { fmt = 0, masked = false; }
  void set(int32_t fmt_, int32_t npad_, int64_t ldk_, bool masked_) {
    fmt = fmt_, npad = npad_, ldk = ldk_, masked = masked_ && fmt_ == 8;
  }
  bool valid() const { return fmt != 0; }
  bool readable() const { return fmt > 0; }   // (not the fp32 / f16x3 formats)
  bool planes() const { return fmt == 8; }
  const uint8_t* mask_of(const uint8_t* kmask) const { return masked ? kmask : nullptr; }
};

}  // namespace ut

// Every device array of a context is a DevBuf: a member here, of its Space or
// of a PopSlot.  `delete c` frees them all, so a new buffer is one declaration
// and nothing else; ut_ctx_destroy itself releases only the streams, events
// and pinned host buffers.
struct ut_ctx {
  int device = 0;
  uint64_t seed = 0;
  hipStream_t stream = nullptr;      // the caller-visible stream (ut_set_stream)
  hipStream_t own_stream = nullptr;
  // internal streams: a round's hash + dedup run on `side` beside the GP
  // contractions on `stream`; an asynchronous GP fit runs on `fit_stream`
  // beside the round's proposal / hash (joined by events, never by host waits)
  hipStream_t side = nullptr;
  hipStream_t fit_stream = nullptr;
  hipEvent_t ev_fork = nullptr, ev_join = nullptr, ev_fit = nullptr, ev_prefit = nullptr;
  hipEvent_t ev_fit_x = nullptr;     // fit stream: scaled training inputs ready (K* may start)
  bool fit_pending = false;          // scoring waits on ev_fit before touching GP state
  // fp64 variance with few candidate strips: 1 = split the k loops
  // (k_gp_var_pp<true> + k_var_split_red), 0 = one item per row tile; UT_VAR_SPLIT
  int32_t var_split = 1;
  double* fit_host = nullptr;        // pinned staging of X, y, 1/ell for the asynchronous fit
  size_t fit_host_n = 0;
  // a staged fit whose device work is not enqueued yet: gp_fit_enqueue stages
  // X, y and the host-side decisions, gp_fit_flush issues the launches.  A
  // proposal (and so every scoring round) is enqueued before the staged fit,
  // so the caller's stream is not idle while the host issues the fit's ~50
  // launches; anything that reads GP state flushes first.
  struct FitJob {
    bool on = false;
    int32_t n = 0, n0 = 0, d = 0, npad = 0, dpn = 0, xr0 = 0;
    bool app = false;
    double diag = 0.0, sf2 = 1.0;
  } fit_job;
  bool fit_prefit_set = false;   // ev_prefit already recorded for fit_job (gp_fit_prefit)
  int32_t fit_defer = 1;         // UT_FIT_DEFER=0: gp_fit_enqueue issues the launches itself
  std::string err;
  ut::Space space;
  bool has_space = false;

  // One population and what is derived from it.  The techniques of one bandit
  // share a context (its GP fit, history set, scratch) and keep one population
  // each: `cur` is the selected slot's, the others are parked in pop_slots
  // (ut_population_select swaps them).
  struct PopSlot {
    ut::DevBuf<double> pop;
    int64_t npop = 0;
    // PSO state
    ut::DevBuf<double> pso_vel;    // [P][npop]
    ut::DevBuf<double> pso_best;   // [P][npop]
    // inner digests sha256(repr(get_value)) of the population's computed-digest
    // params ([n_comp][npop][8]): a DE trial keeps most of its target's values,
    // so its hash reuses the target's inner digests and computes only the
    // changed ones (hash.hip launch_hash_de)
    ut::DevBuf<uint32_t> pop_dig;
    bool pop_dig_valid = false;
    // the cache covers members [pop_dig_lo, pop_dig_lo + pop_dig_n) only: the
    // targets of this context's candidates (a rank's shard of the global pool,
    // cand_base .. cand_base + m), not the whole replicated population
    int64_t pop_dig_lo = 0, pop_dig_n = 0;
    // member-major donor copy of the population ([npop + 1][ld], ld = ncols
    // rounded up to 16 columns = whole 128-B lines), primitive params stored
    // as their unit values (unit_of), the others raw: k_de gathers its donors'
    // rows from it in line pieces staged in LDS, with no unit_of left to
    // compute; row npop holds the best config of the current DE launch.
    // Rebuilt from pop when stale, patched by replace.
    ut::DevBuf<double> pop_aos;
    bool pop_aos_valid = false;
  };
  PopSlot cur;
  std::vector<PopSlot> pop_slots;   // [pop_slot] is empty while that slot is in `cur`
  int32_t pop_slot = 0;
  int32_t de_aos = 1;   // 0: k_de gathers donor values from the column-major population (UT_DE_AOS=0)
  // the round being enqueued holds its hash for an in-flight fit (dense fp64
  // rounds: api.hip score_round_de_impl)
  bool round_hash_hold = false;
  // the grid-stride hash kernels' workgroups per CU: > 0 at most this many, 0
  // uncapped, -1 capped while a large refit is in flight (hash.hip hash_cap);
  // UT_HASH_WG_PER_CU
  int32_t hash_wg_per_cu = -1;
  // top-k of raw scores (topk.hip): 1 threshold selection at every size, 0 the
  // tournament of sorts everywhere, -1 the selection where the tournament needs
  // more than two launches; UT_TOPK_SELECT
  int32_t topk_select = -1;
  // small-m outer hash (hash.hip): 1 one wave per row up to HASH_WIDE_M, 0 the
  // lane-per-row k_hash, -1 = 1; UT_HASH_WIDE
  int32_t hash_wide = -1;
  // refit: the next diagonal block factored inside the trailing update
  // (k_chol_update_diag). -1 = from 2048 padded rows on: the fit alone 6.5 ->
  // 5.7 ms at n = 4096, C3 pruned 60.1 -> 59.2 ms; at C2 (n = 1024, the fit
  // beside K*) the heavier update workgroups cost the round 0.25 ms. UT_CHOL_FUSE
  int32_t chol_fuse = -1;
  // L^-1 levels of 256 rows and more on k_trinv_big (128 x 128 tiles, glds
  // ring) instead of k_trinv_level (64 x 64 tiles, plain loads); UT_TRINV_BIG
  int32_t trinv_big = 1;
  // the diagonal blocks' inverse solved inside the Cholesky column loop
  // (gp_tiles.h chol_diag_core<true>); UT_CHOL_MERGED
  int32_t chol_merged = 1;

  // history set
  ut::DevBuf<uint32_t> hist_keys;   // [cap][8]
  ut::DevBuf<uint32_t> hist_state;  // [cap] 0 empty / 1 full
  int64_t hist_cap = 0;
  int64_t hist_count = 0;

  // batch dedup table
  ut::DevBuf<int32_t> batch_slots;

  // GP state
  int32_t gp_n = 0, gp_d = 0;
  bool gp_ready = false;
  uint64_t fit_gen = 0;        // counts the fits staged (gp_fit_enqueue): the key of every per-fit cache
  ut::DevBuf<double> gp_Xs;     // [n][d] scaled features
  ut::DevBuf<double> gp_xnorm;  // [n]
  ut::DevBuf<double> gp_K;      // [n][n] work / L
  ut::DevBuf<double> gp_Linv;   // [n][n]
  ut::DevBuf<double> gp_T;      // [n][n] scratch of the recursive inverse
  ut::DevBuf<double> gp_y;      // [n] standardised
  ut::DevBuf<double> gp_tmp;    // [n]
  ut::DevBuf<double> gp_alpha;  // [n]  K^-1 y
  ut::DevBuf<double> gp_beta;   // [n]  L^-1 y (mean from the variance epilogue: mu = (L^-1 k*) . beta)
  ut::DevBuf<double> gp_inv_ell;// [d]
  ut::DevBuf<double> gp_stats;  // [4]: f_best, mean, std, flag
  ut::DevBuf<int32_t> gp_flag;
  double gp_sf2 = 1.0;
  int32_t gp_prec = 64;        // precision requested for the next fit
  int32_t gp_fit_prec = 64;    // precision of the fitted factors used by scoring
  // incremental fit (gp_fit.hip gp_fit_enqueue): 1 = a fit whose training set
  // extends the previous one's extends its factor (ut_gp_set_fit_append)
  int32_t fit_append = 1;
  int32_t gp_npad_fit = 0;     // padded size of the current factor
  double gp_diag_fit = 0.0;    // its sigma_n2 + jitter
  double gp_sn2_fit = 0.0;     // ... and its sigma_n2 alone (the LML gradient's noise component)
  int32_t gp_fit_kind = 0;     // 0 = the last fit refactored, 1 = it appended rows
  int32_t gp_l_rows = 0;       // leading rows of gp_K whose off-diagonal entries are L's (appends keep B in gp_T)
  bool gp_linvt_stale = false; // gp_LinvT / gp_alpha not yet written for the current factor (gp_ensure_linvt)
  int32_t* flag_host = nullptr;  // pinned readback of the previous fit's flag
  ut::DevBuf<float> gp_Xs_f;    // fp32 copies for the fp32 MFMA path
  ut::DevBuf<double> gp_LinvT;  // (L^-1)^T [k][row]: the A operand of the variance contraction
  ut::DevBuf<double> gp_XsT;    // (X/ell)^T [dpad][npad]: the A operand of the K* contraction
  // categorical K* of the current fit (cat_on): numeric-feature operands and
  // the training rows' weighted one-hot codes; c0 + c1 * matches starts the
  // fp64 accumulator (= -|x_cat - u_cat|^2 / 2)
  bool cat_on = false;         // this fit scores with the categorical K*
  bool cat_x_ok = false;       // every training row so far has one-hot ENUM / 0-1 BOOL features
  int32_t cat_enable = 1;      // UT_CAT_KSTAR
  double cat_c0 = 0.0, cat_c1 = 0.0;
  ut::DevBuf<double> gp_XsT_num;    // [dpad_num][npad]
  ut::DevBuf<double> gp_xnorm_num;  // [npad] |x_num / ell|^2
  ut::DevBuf<int8_t> gp_acat;       // [cat_k / 128][npad][128] training codes (weights 2 ENUM, 1 BOOL)
  ut::DevBuf<int8_t> bcat;         // [cat_k / 128][ldk][128] candidate codes (one-hot 0/1)
  bool ucand_cat = false;          // ucand / cnorm / bcat hold the categorical K*'s operands (encode path)
  ut::DevBuf<int8_t> pr_bcat;      // pruned scoring: the gathered candidates' codes
  ut::DevBuf<float> gp_LinvT_f;  // fp32 (L^-1)^T; in h3 mode the fp16 hi/lo planes of L^-1 [row][k]
  // int8-sliced fp64 tier (precision 8, gp_i8.hip): L^-1 as I8_S digit planes,
  // per-row scales 2^(ea_i + eb) [npad] | e_i^2 [npad] | the bound E [1]
  ut::DevBuf<int8_t> gp_i8a;
  ut::DevBuf<double> gp_i8rs;
  // precision 8's K* on the int8 MFMA (gp_kq.hip, numeric fits): digit planes
  // of the training operand and its [amax, ea]; the round's candidate planes
  // and column scales
  ut::DevBuf<int8_t> gp_x8, u8;
  ut::DevBuf<int64_t> gp_q8;
  ut::DevBuf<double> scol;
  // k_gp_kstar_q's plane-occupancy mask [npad / 32][ldk / 32]: bit p of a byte is
  // set iff plane p of that 32-row x 32-candidate block of K* holds a non-zero
  // digit (the four bytes of a 128-candidate variance strip at one k stage: one
  // aligned dword); kst_desc.masked says whether it describes the planes now in
  // kst.  Behind the mask's bytes, the K* screen's variance strips with a live
  // unit, [8] counts and [8][scap] strips (there, so that the variance kernel
  // needs no further pointer).
  ut::DevBuf<uint8_t> kmask;
  // kmask_cnt [1]: the blocks of the last k_gp_kstar_q whose mask is not 0x3f
  // (padding included), read back with each precision-8 call's recompute count.
  ut::DevBuf<int32_t> kmask_cnt;
  // The K* screen (k_q_screen, gp_kq.hip): ks_items [8][icap] the live 64 x 64
  // K* items per XCD (64 * column tile + row tile); ks_cnt [24] = item counts
  // [0, 8), certified units [16], all-zero mask bytes of an unscreened call [17]
  // (k_q_mask_zeros).
  ut::DevBuf<int32_t> ks_items, ks_cnt;
  ut::I8Hints i8_hints;   // (gp_i8_plan.h) all that precision-8 dense scoring carries from call to call
  ut::I8Stats i8_stats;   // the last precision-8 dense call, for the API
  int32_t kstar_q = 1;  // UT_KSTAR_Q=0: precision-8 K* on k_gp_kstar<int8_t> (the fp64 MFMA)
  int32_t gp_i8_eb = 0;          // K* digit scale: y = k* 2^-eb <= 0.49
  double i8_tol = 0x1p-20;       // accepted relative variance error (ut_gp_set_i8_tol)
  ut::DevBuf<int32_t> gp_ctr;   // [32] per-XCD work tickets: [0,8) variance, [8,16) K*; [16,18) max|L^-1| bits (h3)
  int32_t n_cu = 256;
  // LDS one workgroup may hold (hipDeviceAttributeMaxSharedMemoryPerBlock): the
  // categorical K*'s code-row kernels need code_rows_lds(cat_k) of it
  size_t max_lds = 65536;
  int64_t gp_cap_n = 0;

  // scratch for GP scoring / round pipeline
  ut::DevBuf<double> kst;        // [n][ld]
  ut::KstDesc kst_desc;          // what is in kst
  ut::DevBuf<double> mu_part;    // [RT][ld]
  ut::DevBuf<double> var_part;   // [RT][ld]
  ut::DevBuf<double> cnorm;      // [ld]
  ut::DevBuf<double> ucand;      // [dpad][ld] candidate features / ell (the K* B operand)
  ut::DevBuf<double> r_values, r_feat, r_mu, r_var, r_score;
  ut::DevBuf<uint32_t> r_digest;
  ut::DevBuf<uint8_t> r_dup;
  ut::DevBuf<uint8_t> r_inval;      // GA rounds: children whose retries all reproduced a parent
  ut::DevBuf<double> tk_score[2];
  ut::DevBuf<int64_t> tk_idx[2];
  ut::DevBuf<uint32_t> tk_sel;      // top-k selection: global digit histogram + SelState (topk.hip), zero between kernels
  ut::DevBuf<uint32_t> tk_wcnt;     // top-k selection: ties of the threshold key per workgroup
  ut::DevBuf<int64_t> r_topk_idx;
  ut::DevBuf<double> tr_box;     // [3][P] trust-region call: half-widths h | box faces lo | hi (propose_tr.hip)
  ut::DevBuf<double> perm_ws;    // [2 * perm_cols + 3 * perm_smax][ld]: GA parents + crossover scratch
  ut::DevBuf<uint32_t> perm_dig; // [n_perm][m][8] inner digests of PERM values (hash pre-pass)
  ut::DevBuf<double> r_topk_score;
  ut::DevBuf<double> r_topk_vals;   // gathered top-k rows when the caller wants digests only
  ut::DevBuf<uint32_t> r_mask;      // [ceil(n_comp / 32)][ld]: bit s = trial's cslot-s value differs from its target's
  ut::DevBuf<uint32_t> r_fresh;     // [n_comp][ld][8]: inner digests of the changed values
  ut::DevBuf<uint64_t> r_pairs;     // compacted (candidate << 20 | cslot) of the changed values
  ut::DevBuf<int64_t> r_npairs;     // [1] their count
  ut::DevBuf<uint32_t> de_xbits;    // k_de's cr-test bits when they outgrow LDS (> 2048 params)
  ut::DevBuf<uint32_t> par_dig;     // [n_comp][16]: hex inner digests of ut_hash_parent's parent row
  ut::DevBuf<uint32_t> hs_mask;     // small-m ut_hash: all-ones reuse mask [ceil(n_comp / 32)][ld]
  ut::DevBuf<uint32_t> hs_fresh;    // small-m ut_hash: every inner digest, hex [n_comp][ld][16]
  // EI-bound pruned scoring (gp_prune.hip ut_gp_topk_pruned)
  ut::DevBuf<double> pr_mu, pr_ub, pr_score;   // [ld] exact mean, score bound, exact scores (-inf if pruned)
  ut::DevBuf<double> pr_mpart;                 // [RT][ldk] unused mean partials of the bound / survivor GEMMs
  ut::DevBuf<double> pr_kst, pr_vpart;         // survivors' K* columns [npad][lds] and variance partials
  ut::DevBuf<double> pr_ucand, pr_cnorm;       // survivors' scaled features [dpad][lds] and norms [lds]
  ut::DevBuf<int64_t> pr_idx;                  // [ld] survivor indices (+ the threshold set)
  ut::DevBuf<int64_t> pr_count;                // [1]
  ut::DevBuf<double> var_vbuf;                 // split variance: raw partial tiles [items][128][128]
  ut::DevBuf<double> app_ws;                   // split-K partials of the incremental fit [b][maxq][64][64]
  ut::DevBuf<double> pr_k2;                    // [RT][ldk] partials of |k*|^2 (the variance tail bound)
  ut::DevBuf<double> pr_f2;                    // [1] |L^-1|_F^2 (+ its block partials), then the f32
                                               // pass's sum |alpha|
  // the fit (fit_gen) each per-fit cache was built from; 0 = never built
  uint64_t pr_f2_gen = 0, pr_ab_gen = 0;       // pr_f2[0] and the sum |alpha|
  uint64_t pr_xf_gen = 0;                      // pr_xsT_f and max |x|^2,
  bool pr_xf_cat = false;                     // ... built from this operand (numeric block or all features)
  int32_t pr_xf_dpad = -1;                     // ... with this many rows
  ut::DevBuf<float> pr_xsT_f, pr_ucand_f;      // f32 K* operands of the f32-contraction bound pass
  ut::DevBuf<double> pr_sa;                    // [RT][ldk] partials of sum |alpha_r| k*_r (f32 bound pass)
  ut::DevBuf<double> pr_gmu;                   // [RT][ldc] fp64 mean partials of recomputed columns (f32 pass)
  int32_t prune_pass = 32;                     // ut_gp_set_prune_pass: the bound pass in f32 or fp64
  ut::DevBuf<uint8_t> pr_exact;                // [ld] the stored score is the exact score
  int32_t prune_weighted = 0;                  // ut_gp_set_prune_weighted: pruned scoring takes loaded rows / values
  ut::DevBuf<double> pr_p;                     // [ldc] the vote p of the gathered candidates (weighted pruning)
  int64_t pr_m = 0;                            // the last pruned call's m (ut_gp_prune_bounds); 0 = none yet
  int64_t r_ld = 0;
  int64_t r_m = 0;
  bool r_feat_valid = false;        // r_feat holds the last round's features (pruned rounds only)
  // lazy dense DE rounds (api.hip score_round_de_impl): only the score-sorted
  // prefix of K' >= 2k candidates is hashed and deduplicated
  ut::DevBuf<int64_t> lz_idx;       // [K'] the prefix: top-K' by unmasked score (-1 = none)
  ut::DevBuf<double> lz_score;      // [K'] their scores
  ut::DevBuf<double> lz_vals;       // [ncols][K'] their value rows
  ut::DevBuf<uint32_t> lz_dig;      // [K'][8] their digests
  ut::DevBuf<uint32_t> lz_out_dig;  // [k][8] the selections' digests when the caller wants none
  ut::DevBuf<int32_t> lz_gate;      // [1] need_full: the prefix held fewer than k distinct new configs
  ut::DevBuf<int64_t> lz_nfall;     // [1] rounds that set need_full, since context creation
  int64_t lazy_rounds = 0;          // lazy rounds enqueued, since context creation
  bool r_lazy = false;              // the last round was lazy
  // while the gated remainder of a lazy round is enqueued: the launchers of
  // hash.hip, dedup.hip, topk.hip and the row gather pass it to their kernels,
  // which return at once when it points at 0
  const int32_t* round_gate = nullptr;

  // tree-ensemble surrogate (forest.hip)
  ut::DevBuf<ut_tree_node> forest_nodes;
  ut::DevBuf<int32_t> forest_roots;
  int32_t forest_trees = 0, forest_rule = 0;
  int32_t forest_max_feat = -1;   // largest feature index of the loaded ensemble's splits
  double forest_base = 0.0, forest_scale = 1.0, forest_div = 1.0;
  // the loaded records as the device holds them: every leaf's threshold field
  // is its variance (0 until ut_forest_leaf_var; forest_score.hip reads it)
  std::vector<ut_tree_node> forest_host;

  // multi-GPU exchange (comm.hip): the RCCL communicator of this context's
  // rank and the packed top-k records of the all-gather / merge
  void* comm = nullptr;               // ncclComm_t
  int32_t comm_rank = 0, comm_size = 1;
  ut::DevBuf<uint64_t> cm_send, cm_recv;   // [k][W] / [R k][W] records (W = 6 + payload columns)
  ut::DevBuf<uint8_t> cm_keep;             // [R k] record survives the digest dedup
  ut::DevBuf<double> cm_pay;               // [n][5] broadcast payload (value + digest)
  ut::DevBuf<int64_t> cm_cnt;              // [2] broadcast count + agreement flag (allocated by ut_comm_init)
  // record capacity (uint64 words of cm_send / cm_recv) every rank agreed it
  // holds: the all-gather votes only when a call needs more (comm.hip)
  size_t cm_agreed_send = 0, cm_agreed_recv = 0;
  // log marginal likelihood (gp_lml.hip).  The grid's scratch, apart from
  // everything the fit and the scoring own:
  ut::DevBuf<double> lml_in;      // staged X [n][d] | y [n] | 1/ell [d] | scaled rows [npad][d] | norms [npad] |
                                  // ys [npad] | stats [4] | per point: 0.5 / scale^2, diagonal, lml [3 g]
  ut::DevBuf<double> lml_d2;      // [npad][npad] |xs_i - xs_j|^2 (lower 64 x 64 tiles)
  ut::DevBuf<double> lml_k;       // [B][npad][npad] K_z, then L_z
  ut::DevBuf<double> lml_li;      // [B][64][npad]: inv(L_kk) of the current panel in columns 0 .. 63
  ut::DevBuf<double> lml_rhs;     // [B][npad] ys, then beta_z = L_z^-1 ys
  ut::DevBuf<int32_t> lml_flag;   // [g] point z is not positive definite
  int32_t lml_batch = 0;          // grid points per chunk; 0 = what fits LML_BUDGET (UT_LML_BATCH)
  double* lml_host = nullptr;     // pinned: ut_gp_lml's result, written by its kernel
  // the LML gradient's scratch (gp_lml_grad.hip): alpha [npad] | the components [d + 2] |
  // the lower tiles' shares of them [tiles][d + 2]
  ut::DevBuf<double> lml_grad;
  // batch-aware selection's scratch (gp_batch.hip), p the shortlist, ldp its padding
  ut::DevBuf<double> bs_u, bs_cn;          // scaled features [dpad to 16][ldp] and norms [ldp]
  ut::DevBuf<double> bs_kst, bs_v;         // K*^T and V = L^-1 K*^T, [npad][ldp]
  ut::DevBuf<double> bs_sig;               // Sigma [p to 64][ldp], the full symmetric matrix
  ut::DevBuf<double> bs_g;                 // G [k][ldp]
  ut::DevBuf<double> bs_vec;               // mu [ldp] | var [ldp] | the launches' partial scores [2][16]
  ut::DevBuf<int32_t> bs_pos;              // ... and partial positions [2][16]
  ut::DevBuf<uint8_t> bs_picked;           // [ldp]
  // the acquisition gradient's and the polish's scratch (gp_polish.hip), beside bs_u, bs_cn, bs_kst, bs_v
  ut::DevBuf<double> bs_w;                 // W = L^-T V [npad][ldp]
  ut::DevBuf<double> bs_pu;                // unit features: current [d][ldp] | trial [d][ldp] | gradient [d][ldp]
  ut::DevBuf<double> bs_pvec;              // per candidate [ldp] each: mu, var, score, cm, cs, s, s0, eta
  ut::DevBuf<double> bs_pval;              // the decoded rows [ncols][ldp]
  ut::DevBuf<uint8_t> bs_pflag;            // free [d to 256] | active [ldp] | accepted [ldp]
  // failure-aware scoring (gp_feas.hip): the loaded failed rows, and their K*
  // operands under the current fit's lengthscales -- a per-fit cache like pr_f2
  ut::DevBuf<double> fs_X;                 // [fs_n][fs_d] features as given to ut_gp_feas_set
  int32_t fs_n = 0, fs_d = 0;              // fs_n = 0: nothing loaded, no score is weighted
  ut_feas_params fs_par{0.0, 1.0, 1.0, 1.0};
  int32_t fs_bad_row = -1;                 // the first row that is not one-hot / 0-1 in the ENUM / BOOL blocks
  uint64_t fs_gen = 0;                     // the fit (fit_gen) the operands below were built from; 0 = stale
  ut::DevBuf<double> fs_Xs, fs_norm;       // scaled rows [nfpad][d] and their norms [nfpad]
  ut::DevBuf<double> fs_XsT;               // [dpad][nfpad], every feature
  ut::DevBuf<double> fs_XsT_num, fs_norm_num;   // the numeric block [dpad_num][nfpad] and its norms (categorical fits)
  ut::DevBuf<int8_t> fs_acat;              // [cat_k / 128][nfpad][128] weighted one-hot codes
  ut::DevBuf<double> fs_part;              // [RT + RT_fail][ldk] column partials of sum k
  // constrained EI (gp_cons.hip): the measured constraint values of the fit's
  // rows, and their per-fit operands on the shared factor -- a per-fit cache
  // like the failed rows' above, but the values themselves belong to one fit
  double* cs_host = nullptr;               // pinned: C^T [cs_nc][cs_n], then the thresholds [cs_nc]
  size_t cs_host_n = 0;
  hipEvent_t cs_ev = nullptr;              // the last copy out of cs_host (recorded on the stream it ran on)
  int32_t cs_n = 0, cs_nc = 0;             // cs_nc = 0: nothing loaded, no score is weighted
  uint64_t cs_fit = 0;                     // the fit (fit_gen) the values were loaded for
  uint64_t cs_gen = 0;                     // the fit the operands below were built from; 0 = stale
  ut::DevBuf<double> cs_C;                 // [cs_nc][npad] raw values (then the thresholds [UT_CONS_MAX])
  ut::DevBuf<double> cs_chat;              // [cs_nc][npad] standardised, zero on padding rows
  ut::DevBuf<double> cs_beta;              // [cs_nc][npad] L^-1 chat_j
  ut::DevBuf<double> cs_alpha;             // [cs_nc][npad] K^-1 chat_j, zero on padding rows
  ut::DevBuf<double> cs_stats;             // [UT_CONS_MAX][4] ystats of column j, [3] = tau_j; then f_best_c, n_feasible
  ut::DevBuf<double> cs_part;              // [RT][cs_nc][ldk] column partials of sum k alpha_j
  ut::DevBuf<double> cs_mu, cs_var;        // [ldk] the posterior of a call that asked for neither
  // two objectives (gp_mo.hip): the second objective's values of the fit's rows
  // and their per-fit operands on the shared factor, kept as the constraint
  // values' are; the Pareto front of the rows in standardised units
  double* mo_host = nullptr;               // pinned: Y2 [npad], then the reference point [2]
  size_t mo_host_n = 0;
  hipEvent_t mo_ev = nullptr;              // the last copy out of mo_host
  int32_t mo_n = 0;                        // 0: nothing loaded, every score is the plain acquisition
  uint64_t mo_fit = 0;                     // the fit (fit_gen) the values were loaded for
  uint64_t mo_gen = 0;                     // the fit the operands below were built from; 0 = stale
  ut::DevBuf<double> mo_Y;                 // [npad] raw values, then the raw reference point [2]
  ut::DevBuf<double> mo_y2s;               // [npad] standardised, zero on padding rows
  ut::DevBuf<double> mo_beta, mo_alpha;    // [npad] L^-1 y2s, K^-1 y2s
  ut::DevBuf<double> mo_stats;             // [4] ystats of Y2: [1] = m_2, [2] = s_2
  ut::DevBuf<uint8_t> mo_keep;             // [npad] the row is on the front
  ut::DevBuf<double> mo_fr;                // [MO_A] r_1, r_2, hv, P | a [0 .. P + 1] | b [0 .. P] (mo_b_off)
  ut::DevBuf<int32_t> mo_rows;             // [npad] the front's rows, in its order
  ut::DevBuf<double> mo_part;              // [RT][ldk] column partials of sum k alpha_2
  // Thompson-sampling paths (gp_ts.hip): one draw of q paths for one fit
  int32_t ts_q = 0, ts_D = 0;              // ts_q = 0: nothing drawn
  uint64_t ts_fit = 0;                     // the fit (fit_gen) the draw was made for
  ut::DevBuf<double> ts_Z, ts_b;           // Z [D][d] as drawn, b [D]
  ut::DevBuf<double> ts_ZT;                // [dpad][D] Z / (2 pi), transposed: the frequency rows' A operand
  ut::DevBuf<double> ts_theta;             // [q][D]
  ut::DevBuf<double> ts_eps;               // [q][npad], 0 on padding rows
  ut::DevBuf<double> ts_A;                 // [q][npad] a_s, 0 on padding rows
  ut::DevBuf<double> ts_R;                 // [2][q][npad] the residuals r_s, then L^-1 r_s
  ut::DevBuf<double> ts_xu;                // [dpad][npad] the training rows as candidates (g_s(X))
  ut::DevBuf<double> ts_u, ts_cn;          // a call's candidates: scaled features [dpad][ldk], norms [ldk]
  ut::DevBuf<double> ts_F;                 // select: one path group's values [TS_GROUP][ldk]
  ut::DevBuf<double> ts_pv;                // select: the pick launches' partial minima [TS_PICK_WG]
  ut::DevBuf<int64_t> ts_pp;               // ... their positions [TS_PICK_WG], then [1] the dead flag
  ut::DevBuf<uint8_t> ts_taken;            // select: [m] picked by an earlier path
  int32_t dbg_fail_alloc = 0;             // ut_debug_fail_alloc: the next N growing ensure() / dalloc() calls fail
  int32_t dbg_fail_skip = 0;               // ut_debug_fail_alloc_after: ... once this many more have succeeded

  ut::Timing timing;
};

namespace ut {

int set_err(ut_ctx* c, int code, const std::string& msg);

// wait for every stream of the context (before freeing or reusing buffers)
inline hipError_t sync_all(ut_ctx* c) {
  hipError_t e = hipStreamSynchronize(c->stream);
  for (hipStream_t s : {c->side, c->fit_stream}) {
    if (!s) continue;
    const hipError_t e2 = hipStreamSynchronize(s);
    if (e == hipSuccess) e = e2;
  }
  return e;
}

// launches inside the scope go to stream s (the launch helpers all use c->stream)
struct StreamScope {
  ut_ctx* c;
  hipStream_t saved;
  StreamScope(ut_ctx* ctx, hipStream_t s) : c(ctx), saved(ctx->stream) { ctx->stream = s; }
  ~StreamScope() { c->stream = saved; }
};

#define UT_HIP(ctx, call)                                                                 \
  do {                                                                                    \
    hipError_t e_ = (call);                                                               \
    if (e_ != hipSuccess)                                                                 \
      return ::ut::set_err((ctx), UT_EHIP, std::string(#call) + ": " + hipGetErrorString(e_)); \
  } while (0)

#define UT_CHECK(ctx, cond, code, msg)                    \
  do {                                                    \
    if (!(cond)) return ::ut::set_err((ctx), (code), (msg)); \
  } while (0)

#define UT_LAUNCH_CHECK(ctx)                                                       \
  do {                                                                             \
    hipError_t e_ = hipGetLastError();                                             \
    if (e_ != hipSuccess)                                                          \
      return ::ut::set_err((ctx), UT_EHIP, std::string("launch: ") + hipGetErrorString(e_)); \
  } while (0)

// feature rows of the K* operands (Xs^T, U'): d rounded up to the f64 MFMA's k = 4
inline int32_t kstar_dpad(int32_t d) { return ((d + 3) / 4) * 4; }
// ... and of the categorical K*'s operands: the numeric features only
inline int32_t cat_dpad(const ut_ctx* c) { return kstar_dpad(c->space.n_num); }

constexpr int NPAD = 128;                  // training set padded to the GEMM row tile
constexpr int VAR_BM = 128, VAR_BN = 256;  // variance-contraction tile (rows of L^-1 x candidates)
inline int32_t gp_npad(int32_t n) { return ((n + NPAD - 1) / NPAD) * NPAD; }
// K* rows padded to whole variance column tiles: the variance kernel reads
// full 256-candidate strips (the K* kernel writes zeros past m)
inline int64_t gp_ldk(int64_t m) { return ((m + VAR_BN - 1) / VAR_BN) * VAR_BN; }

// The padded sizes of one scoring call over m candidates of the current fit:
// which K* it takes (cat) is the caller's own rule, every size that follows
// from it is taken from here.  n, d: training rows, features; RT: 128-row
// tiles; ldk: padded candidates; dpad: feature rows of the K* operands
struct ScoreShape {
  int32_t n, d, npad, RT;
  int64_t ldk;
  bool cat;
  int32_t dpad;
  size_t urows() const { return (size_t)(dpad > 0 ? dpad : 1); }   // ... to allocate (never 0)
};
inline ScoreShape score_shape(const ut_ctx* c, int64_t m, bool cat) {
  const int32_t npad = gp_npad(c->gp_n);
  return ScoreShape{c->gp_n, c->gp_d, npad, npad / NPAD, gp_ldk(m), cat, cat ? cat_dpad(c) : kstar_dpad(c->gp_d)};
}

// fault injection (tests): true when this counted allocation is to fail as
// hipMalloc would -- after dbg_fail_skip counted allocations went through, the
// next dbg_fail_alloc fail
inline bool inject_alloc_failure(ut_ctx* c) {
  if (c->dbg_fail_alloc <= 0) return false;
  if (c->dbg_fail_skip > 0) {
    --c->dbg_fail_skip;
    return false;
  }
  --c->dbg_fail_alloc;
  return true;
}

template <class T>
int ensure(ut_ctx* c, DevBuf<T>& b, size_t n) {
  if (b.n >= n && b.p) return 0;
  if (inject_alloc_failure(c)) return set_err(c, UT_ENOMEM, "hipMalloc: injected failure (ut_debug_fail_alloc)");
  // a buffer that has to grow again (sizes that follow a growing training
  // set) gets headroom, up to 2 GiB: every regrowth costs a device-wide sync
  size_t want = n;
  if (b.p) {
    want = n + std::min(n / 4, ((size_t)2 << 30) / sizeof(T));
    (void)ut::sync_all(c);
    b.reset();
  }
  hipError_t e = b.alloc(want ? want : 1);
  if (e != hipSuccess && want > n) {   // no room for the headroom: exactly n
    (void)hipGetLastError();
    want = n;
    e = b.alloc(want ? want : 1);
  }
  if (e != hipSuccess) return set_err(c, UT_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
  b.n = want;   // (an empty request holds one element and still counts as 0)
  return 0;
}

// a new array of exactly n elements under the same fault injection as
// ensure(), with neither its headroom nor its sync (the history and batch
// dedup tables): b is written only on success, so a caller allocates into
// locals and swaps them in once it has all.
template <class T>
int dalloc(ut_ctx* c, DevBuf<T>& b, size_t n) {
  if (inject_alloc_failure(c)) return set_err(c, UT_ENOMEM, "hipMalloc: injected failure (ut_debug_fail_alloc)");
  DevBuf<T> q;
  const hipError_t e = q.alloc(n ? n : 1);
  if (e != hipSuccess) {
    (void)hipGetLastError();
    return set_err(c, UT_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
  }
  b.swap(q);
  return 0;
}

void mark(ut_ctx* c, const char* name);
int gp_fit_enqueue(ut_ctx* c, const double* X, const double* y, int32_t n, int32_t d, const ut_gp_hyper* h);
int gp_wait_fit(ut_ctx* c);
int gp_fit_flush(ut_ctx* c);
int gp_ensure_linvt(ut_ctx* c);
int gp_fit_prefit(ut_ctx* c);
// gp_fit.hip's staging kernels on any buffers: scaled rows + norms, standardised y + stats
int launch_gp_prep_train(ut_ctx* c, const double* X, int32_t n, int32_t npad, int32_t d, const double* inv_ell,
                         double* Xs, double* xnorm);
int launch_gp_ystats(ut_ctx* c, const double* y, int32_t n, int32_t npad, double* ys, double* stats);
// ... and its mat-vecs over the current factor: out = L^-1 v, out = L^-T v ([npad] each)
int launch_gp_lower_mv(ut_ctx* c, const double* v, double* out);
int launch_gp_upper_mv(ut_ctx* c, const double* v, double* out);
// gp_lml.hip: the log marginal likelihood of the fit in place / at g hyperparameter points
int gp_lml_impl(ut_ctx* c, double* lml_host);
int gp_lml_grid_impl(ut_ctx* c, const double* X, const double* y, int32_t n, int32_t d, const ut_gp_hyper* h,
                     int32_t g, const double* scale, const double* noise, double* lml_host, int32_t* best_host);
// gp_lml_grad.hip: its gradient at the fit in place
int gp_lml_grad_impl(ut_ctx* c, int32_t d, double* dlog_ell_host, double* dlog_sf2_host, double* dlog_sn2_host);
// gp_fit.hip: the categorical K*'s training-side operands of rows Xs (scaled) / X (raw), as the fit builds its own
int launch_gp_cat_train(ut_ctx* c, const double* Xs, const double* X, int32_t n, int32_t npad, int32_t d, int32_t dpn,
                        double* XsT_num, double* xnorm_num, int8_t* acat);
// ... and the host check that goes with the codes: rows [r0, r1) of X [n][d] are one-hot / 0-1 there
bool cat_rows_ok(const Space& s, const double* X, int32_t d, int32_t r0, int32_t r1);
// gp_feas.hip: the feasibility vote.  feas_weight: score[i] *= p_i^gamma for the m candidates whose K*
// operands (of shape s) are in c->ucand / c->cnorm / c->bcat
int gp_feas_set_impl(ut_ctx* c, const double* X, int32_t nf, int32_t d, const ut_feas_params* p);
int gp_feas_prob_impl(ut_ctx* c, const double* values, const double* features, int64_t ld, int64_t m, double* p_out,
                      double* s_ok_out, double* s_fail_out);
int feas_weight(ut_ctx* c, const ScoreShape& s, int64_t m, double* score);
// the candidates' K* operands of a vote: the context's own (c->ucand / c->cnorm / c->bcat, padded to s.ldk)
// unless given -- pruned scoring's gathered columns (c->pr_ucand / c->pr_cnorm / c->pr_bcat, padded to ld)
struct CandOps {
  const double* ucand;
  const double* cnorm;
  const int8_t* bcat;
  int64_t ld;
};
// gp_kstar_sums.hip: the K* contraction with a column-sum epilogue, no K* stored.  One row set of a launch: the
// contraction's A operand and what goes with it
struct KstarRowSet {
  const double* AT = nullptr;     // [dpad][npad] scaled rows, transposed, times KSTAR_T_SCALE
  const double* norm = nullptr;   // [npad] |row / ell|^2 over the operand's features
  const int8_t* acat = nullptr;   // [nkc][npad][128] weighted one-hot codes (categorical)
  const double* w = nullptr;      // [nw][npad] the rows' weight vectors (nw > 0; 0 on padding rows)
  int32_t n = 0, npad = 0;        // rows, padded to 128 (0: an empty set)
};
// part [(s.npad + b.npad) / 128][max(nw, 1)][u.ld] = per row tile, the fit's training rows' then b's, the sums over
// the tile's rows r of k(r, u) (nw = 0, with every lengthscale times 1 / sqrt(inv_s2)) or of k(r, u) w_q[r]
// (q < nw <= UT_CONS_MAX, w: the training rows' weights; inv_s2 unused), for the m candidates of u (shape s)
int launch_kstar_sums(ut_ctx* c, const char* who, const ScoreShape& s, const CandOps& u, int64_t m, const double* w,
                      int32_t nw, const KstarRowSet& b, double inv_s2, double* part);
// ... p_out[j] = p of the m columns of ops (no score is touched)
int feas_prob_cols(ut_ctx* c, const ScoreShape& s, const CandOps& ops, int64_t m, double* p_out);
// gp_cons.hip: constrained EI.  cons_weight: score[i] = EI(mu_i, var_i; f_best_c, xi) P_i (P_i when no row is
// feasible) for the m candidates whose K* operands (of shape s) are in c->ucand / c->cnorm / c->bcat and whose
// posterior the dense body left in mu / var; cons_stale: UT_EINVAL when the loaded values belong to an earlier fit
int gp_cons_set_impl(ut_ctx* c, const double* C, int32_t n, int32_t nc, const double* thr);
int gp_cons_prob_impl(ut_ctx* c, const double* values, const double* features, int64_t ld, int64_t m, double* p_out,
                      double* mu_c_out);
int gp_cons_info_impl(ut_ctx* c, int32_t* n, int32_t* nc, int32_t* n_feasible, double* f_best_c);
int cons_stale(ut_ctx* c, const char* who);
int cons_weight(ut_ctx* c, const ScoreShape& s, int64_t m, double xi, const double* mu, const double* var,
                double* score);
// ... its first half alone: the per-fit operands (cs_alpha, cs_stats) and the constraint-mean partials of the m
// candidates in c->ucand / c->cnorm / c->bcat (or in ops) into c->cs_part [RT][cs_nc][ld] (k_kstar_sums)
int cons_means(ut_ctx* c, const ScoreShape& s, int64_t m, const CandOps* ops = nullptr);
constexpr int CS_INFO = 4 * UT_CONS_MAX;   // cs_stats[CS_INFO] = f_best_c, [CS_INFO + 1] = n_feasible
// gp_mo.hip: two objectives (uthot.h "two objectives").  mo_fr's layout: the header, then a with both
// sentinels, then b with its one
constexpr int MO_A = 4;
inline int64_t mo_b_off(int32_t npad) { return MO_A + (int64_t)npad + 2; }
int gp_mo_set_impl(ut_ctx* c, const double* Y2, int32_t n, const double* ref);
int gp_mo_score_impl(ut_ctx* c, const double* values, const double* features, int64_t ld, int64_t m, double* ehvi_out,
                     double* mu2_out);
int gp_mo_info_impl(ut_ctx* c, int32_t* n, int32_t* P, double* ref_std, double* hv);
int gp_mo_front_impl(ut_ctx* c, int32_t* rows_host, double* a_host, double* b_host, int32_t cap, int32_t* P);
int gp_mo_read_impl(ut_ctx* c, int32_t what, double* out_host);
// UT_EUNSUPPORTED while a second objective is loaded: `who` does not know EHVI (why: the reason's words)
int mo_refuse(ut_ctx* c, const char* who, const char* why);
// what a dense scoring call checks before it enqueues anything: UT_EINVAL when the loaded values belong to an
// earlier fit, UT_EUNSUPPORTED for a UCB score (EHVI stands in for EI only)
int mo_check(ut_ctx* c, const char* who, const ut_acq* acq);
// score[i] = EHVI_i (finite scores only) for the m candidates whose K* operands (of shape s) are in c->ucand /
// c->cnorm / c->bcat and whose posterior the dense body left in mu / var
int mo_weight(ut_ctx* c, const ScoreShape& s, int64_t m, const double* mu, const double* var, double* score);
// gp_score.hip: UT_EUNSUPPORTED for a UCB score while rows (feas) or values (cons) would weight it
int weights_refuse_ucb(ut_ctx* c, const ut_acq* acq, bool feas, bool cons);
// gp_batch.hip: k picks from a shortlist of p, each conditioned on the picks before it
int gp_select_batch_impl(ut_ctx* c, const double* values, int64_t ld, int32_t p, const ut_acq* acq,
                         const uint8_t* dup, int32_t k, int64_t* out_pos, double* out_score, double* out_var);
// ... its V = L^-1 K*^T [npad][ldp] alone (k_bs_v), CT column tiles of 64
int launch_bs_v(ut_ctx* c, int32_t CT, int32_t npad, const double* kst, int64_t ldp, double* V);
// gp_polish.hip: the acquisition's gradient in the unit features, and the projected-ascent polish of a shortlist
int gp_acq_grad_impl(ut_ctx* c, const double* values, int64_t ld, int32_t p, const ut_acq* acq, double* out_score,
                     double* out_mu, double* out_var, double* out_grad, int64_t ld_g);
int gp_polish_impl(ut_ctx* c, const double* values, int64_t ld, int32_t p, const ut_acq* acq, const uint8_t* dup,
                   const ut_polish_params* prm, double* out_values, int64_t ld_o, double* out_score,
                   double* out_score0, uint8_t* out_moved);
// gp_ts.hip: Thompson-sampling posterior paths (uthot.h states the rule)
constexpr int32_t TS_GROUP = 32;      // paths per work item of k_ts_paths, and per F workspace of ut_gp_ts_select
constexpr int32_t TS_MAX_Q = 256, TS_MAX_D = 4096;
int gp_ts_draw_impl(ut_ctx* c, int32_t q, int32_t D, uint32_t round_);
int gp_ts_eval_impl(ut_ctx* c, const double* values, int64_t ld, int64_t m, double* out_F, int64_t ldf);
int gp_ts_select_impl(ut_ctx* c, const double* values, int64_t ld, int64_t m, const uint8_t* dup, int32_t k,
                      int64_t* out_pos, double* out_f);
int gp_ts_read_impl(ut_ctx* c, int32_t what, double* out_host, int32_t* info);

// kernel launchers implemented in the .hip translation units
int launch_population_init(ut_ctx* c, uint32_t round_);
// diff = true (DE scoring rounds): k_de also writes the DE-diff mask, pairs and
// pair count (r_mask / r_pairs / r_npairs) that launch_hash_de would derive
int launch_de(ut_ctx* c, const ut_de_params* p, uint32_t round_, int64_t cand_base, int64_t m, double* out,
              int64_t ld, bool diff = false);
int launch_pso(ut_ctx* c, const ut_pso_params* a, const double* gbest, uint32_t round_, int64_t cand_base,
               int64_t m, double* out_x, double* out_v, int64_t ld);
int launch_ga(ut_ctx* c, const ut_ga_params* a, const double* parent1, const double* parent2, uint32_t round_,
              int64_t cand_base, int64_t m, double* out, int64_t ld, uint8_t* invalid);
int launch_encode(ut_ctx* c, const double* values, int64_t ld, int64_t m, double* feat, int64_t ldf);
int launch_hash(ut_ctx* c, const double* values, int64_t ld, int64_t m, uint32_t* out);
// hash_config of DE trials of the selected population (candidate g targets
// member g % npop): inner digests of values equal to the target's come from
// the population cache (rebuilt if stale), the rest are computed once
// have_diff: the mask / pairs / count were written by k_de (launch_de diff = true)
int launch_hash_de(ut_ctx* c, const double* values, int64_t ld, int64_t m, int64_t cand_base, uint32_t* out,
                   bool have_diff = false);
// hash_config of children of one parent row (ut_hash_parent): inner digests of
// the values equal to the parent's are the parent's own
int launch_hash_parent(ut_ctx* c, const double* values, int64_t ld, int64_t m, const double* parent, uint32_t* out);
// the DE-diff buffers for m candidates (ld): r_mask, r_fresh, r_pairs, r_npairs
int ensure_de_diff(ut_ctx* c, int64_t ld);
// population cache maintenance: the rows idx[0..n) after a replace (rows
// outside the cached window are skipped)
int launch_pop_digests(ut_ctx* c, const int64_t* idx, int64_t n);
// full rebuild of the cache for the members [lo, lo + wn)
int launch_pop_digests_window(ut_ctx* c, int64_t lo, int64_t wn);
// the member-major population copy: rebuilt if stale (ensure), or the rows
// idx[0..n) patched from trial after a replace
int ensure_pop_aos(ut_ctx* c);
int launch_pop_aos_rows(ut_ctx* c, const double* trial, int64_t ld, const int64_t* idx, int64_t n);
// row `row` of the donor copy = the config `src` (device, ncols values)
int launch_aos_row(ut_ctx* c, const double* src, int64_t row);
inline int64_t pop_aos_ld(const ut_ctx* c) { return ((int64_t)c->space.ncols + 15) / 16 * 16; }
int launch_hist_insert(ut_ctx* c, const uint32_t* dig, int64_t n);
// re-insert the occupied slots of the table (okeys, ostate, ocap) into (keys, state, cap)
int launch_hist_rehash(ut_ctx* c, const uint32_t* okeys, const uint32_t* ostate, int64_t ocap, uint32_t* keys,
                       uint32_t* state, int64_t cap);
int launch_dedup(ut_ctx* c, const uint32_t* dig, int64_t m, uint8_t* dup);
int launch_mask_or(ut_ctx* c, uint8_t* dst, const uint8_t* src, int64_t m);
// lazy rounds (dedup.hip).  The prefix of kp <= 1024 score-sorted candidates
// (idx, -1 = none; score; digests; value rows [ncols][kp]): entry p is a
// duplicate when its digest is in the history or an entry with a smaller
// index has it; the first k others, in prefix order, go to out_* (padded with
// index -1).  *gate = 1 when fewer than k were found and every prefix entry
// was a candidate (nfall counts those rounds), else 0.
int launch_prefix_dedup(ut_ctx* c, const int64_t* idx, const double* score, const uint32_t* dig, const double* vals,
                        int32_t kp, int64_t cand_base, int32_t k, int64_t* out_idx, double* out_score,
                        double* out_vals, uint32_t* out_dig, int32_t* gate, int64_t* nfall);
// score[i] = -inf where dup[i] (what the finalize kernels write for a duplicate)
int launch_mask_score(ut_ctx* c, double* score, const uint8_t* dup, int64_t m);
// c->round_gate for the calls inside the scope
struct GateScope {
  ut_ctx* c;
  GateScope(ut_ctx* ctx, const int32_t* gate) : c(ctx) { ctx->round_gate = gate; }
  ~GateScope() { c->round_gate = nullptr; }
};
// feat == nullptr: the candidates' scaled features and norms are already in
// c->ucand / c->cnorm (gp_encode_scaled); dup_ready: the event of the dup
// mask (the round's side stream), joined before the variance GEMM
int gp_score_impl(ut_ctx* c, const double* feat, int64_t ld, int64_t m, const ut_acq* acq, const uint8_t* dup,
                  double* mu, double* var, double* score, hipEvent_t dup_ready = nullptr);
// encode + scale in one pass into c->ucand / c->cnorm (sized for m), for gp_score_impl(feat = nullptr)
int gp_encode_scaled(ut_ctx* c, const double* values, int64_t ld, int64_t m);
int launch_encode_scaled(ut_ctx* c, const double* values, int64_t ld, int64_t m, double* u, int32_t dpad, int64_t ldu,
                         double* cn);
// gp_score.hip: fp64 K* columns of the candidates idx[0..nc) of a call of shape s
int gather_kstar_cols(ut_ctx* c, const ScoreShape& s, const int64_t* idx, int64_t base, int64_t nc, int64_t ldc,
                      double* mu_part = nullptr);
int topk_impl(ut_ctx* c, const double* score, const uint8_t* dup, int64_t m, int64_t cand_base, int32_t k,
              int64_t* out_idx, double* out_score);
int topk_pairs_impl(ut_ctx* c, const double* score, const int64_t* idx, int64_t n, int32_t k, int64_t* out_idx,
                    double* out_score);
int gp_topk_pruned_impl(ut_ctx* c, const double* feat, int64_t ld, int64_t m, const ut_acq* acq, const uint8_t* dup,
                        int64_t cand_base, int32_t k, int32_t bound_rows, int64_t* out_idx, double* out_score,
                        ut_prune_stats* stats, hipEvent_t dup_ready = nullptr);
// prec: 64 (fp64 MFMA), 32 (fp32 MFMA), 16 (f16x3: fp16 hi/lo split operands,
// three fp16 MFMA products, f32 accumulate -- see gp_gemm.hip), 8 (the fp64
// tier on the int8 MFMA: six-digit planes, a per-candidate error bound and an
// fp64 recompute of the candidates it does not clear -- gp_i8.hip)
constexpr int H3_KSCALE_EXP = 14;  // K* (<= sf2) is scaled by 2^(14 - ceil(log2 sf2)) before the split
int h3_kstar_exp(double sf2);
// K*'s training operand (Xs^T, the numeric part in categorical mode) is stored
// times 256 / ln 2: the contraction then yields the exponent in 2^(1/256) units
// (sf2_exp2t_nonpos below)
constexpr double KSTAR_T_SCALE = 369.3299304675746;   // 256 / ln 2
// sf2 * exp(x) for x <= 0, table-driven: etab[j] = sf2 * 2^(j/256) built in LDS by
// each workgroup (2 KiB); about 12 VALU ops against ~32 for the library exp with
// its range checks (the epilogue shares the SIMDs with the f64 MFMAs, so every
// op counts; a 32-entry table with a degree-6 polynomial took two more FMAs).
// Max error ~2 ulp; 2^k' underflows to exactly 0 at x = -1000.
constexpr int EXP_TAB = 256;

// The K* contraction works in units of 2^(1/256): its training operand is
// Xs^T * (256 / ln 2) (KSTAR_T_SCALE, applied where Xs^T is built, k_gp_xs_t /
// k_gp_num_train), the epilogue's norms and categorical coefficients carry the
// same factor, so the accumulator is t = -|x - u|^2 / 2 * 256 / ln 2 directly
// and the exp needs no multiply and no two-step reduction: t = 256 k' + j + f
// with kf = rint(t), f = t - kf exact (|f| <= 1/2), and
// exp = 2^k' * 2^(j/256) * e^(f ln2/256) with the same degree-4 polynomial
// (|f ln2/256| <= 1.36e-3: truncation < 4e-17).  Two DP ops fewer per k*
// than sf2_exp_nonpos, whose rounding it shares to ~1 ulp.
__device__ __forceinline__ double sf2_exp2t_nonpos(double t, const double* etab) {
  constexpr double L = 0.6931471805599453 / 256.0;    // ln 2 / 256 (exact: a power-of-two division)
  constexpr double C2 = L * L / 2.0, C3 = L * L * L / 6.0, C4 = L * L * L * L / 24.0;
  const double kf = __builtin_rint(t);
  const double f = t - kf;
  double p = __builtin_fma(C4, f, C3);
  p = __builtin_fma(p, f, C2);
  p = __builtin_fma(p, f, L);
  p = __builtin_fma(p, f, 1.0);
  const int k = (int)kf;
  return __builtin_ldexp(p * etab[k & (EXP_TAB - 1)], k >> 8);
}
constexpr double KSTAR_T_MIN = -1000.0 * KSTAR_T_SCALE;   // exp(-1000): the table's 2^k' underflows to 0
// the K* contraction's categorical operands (nkc = cat_k / 128 int8 stages; 0 = none)
struct KstarCat {
  const int8_t* acat = nullptr;
  const int8_t* bcat = nullptr;
  int32_t nkc = 0;
  double c0 = 0.0, c1 = 0.0;
};
// the training side of the K* contraction for the current fit: every feature
// (cat = false) or the numeric block, the one-hot codes (the candidates': bcat) beside it
struct KstarTrain {
  const double* XsT = nullptr;     // [dpad][npad]
  const double* xnorm = nullptr;   // training norms (nullptr: c->gp_xnorm)
  KstarCat cat;
};
inline KstarTrain kstar_train(const ut_ctx* c, bool cat, const int8_t* bcat) {
  if (!cat) return KstarTrain{c->gp_XsT.p};
  return {c->gp_XsT_num.p, c->gp_xnorm_num.p, {c->gp_acat.p, bcat, c->space.cat_k / 128, c->cat_c0, c->cat_c1}};
}
// one K* launch over the npad training rows of the current fit
struct KstarArgs {
  KstarTrain train;
  const double* ucand = nullptr;   // candidate operand [dpad][ldk] (launch_gemm_kstar_f32c: unused)
  int32_t dpad = 0;
  int64_t m = 0;
  void* kst = nullptr;             // K* [npad][ldk] in the precision's format (f32c stores none)
  int64_t ldk = 0;
  double* part = nullptr;          // mean partials k* . alpha [RT][ldk] (fp32 / h3 / f32c: required)
  double* part2 = nullptr;         // fp64 with part, f32c: also sum_r k*_r^2 partials
  double* part3 = nullptr;         // f32c: sum_r |alpha_r| k*_r partials
  int32_t store_rows = -1;         // fp64: only the first store_rows rows of K* are written
  int32_t row_tiles = -1;          // > 0: only the first row_tiles 128-row tiles
  int32_t rt0 = 0;                 // f32c: the first row tile
  const double* cn = nullptr;      // candidate norms (nullptr: c->cnorm)
};
// The persistent grid of a K* launch over `items` work items: two workgroups
// per CU, a multiple of 8 (one ticket per XCD), CUs left to an in-flight fit if
// asked; kstar_grid also zeroes the eight tickets at c->gp_ctr + 8 on c->stream.
int32_t kstar_blocks(ut_ctx* c, int64_t items, bool leave_for_fit);
int kstar_grid(ut_ctx* c, int64_t items, bool leave_for_fit, int32_t* nb);
int launch_gemm_kstar(ut_ctx* c, int prec, int32_t npad, const KstarArgs& a);
int launch_gemm_kstar_f32c(ut_ctx* c, const float* XsT_f, const float* ucand_f, int32_t npad, const KstarArgs& a);
// gp_kq.hip: K* of a numeric precision-8 fit as the distance contraction on
// the int8 MFMA (digit planes of the training operand from the fit, of the
// candidates' operand per call into u8 / scol), stored as the six digit planes
// the int8 variance reads (no mean partial, no one-hot codes; norms in
// c->gp_xnorm / c->cnorm).  launch_gemm_kstar_q also writes the planes'
// occupancy mask into c->kmask, and runs the screen / the zero-block count
// that plan (i8_plan of this npad and kstar_q_k32(dpad)) names: it decides nothing.
inline int32_t kstar_q_k32(int32_t dpad) { return (dpad + 31) / 32; }
int alloc_split_x8(ut_ctx* c, int32_t npad, int32_t K);
int launch_split_x8(ut_ctx* c, const double* XsT, int32_t K, int32_t npad);
int launch_gemm_kstar_q(ut_ctx* c, const I8Plan& plan, const double* ucand, int32_t dpad, int64_t m, void* kst,
                        int64_t ldk, DevBuf<int8_t>& u8, DevBuf<double>& scol);
// a caller's feature matrix feat [s.d][ld] becomes the K* operands of the m candidates of a call of shape s (dense
// over every feature) in c->ucand / c->cnorm, grown as needed
int prep_cand_features(ut_ctx* c, const ScoreShape& s, const double* feat, int64_t ld, int64_t m);
// categorical K*: the K* operands of the candidate side when the fit is in
// categorical mode -- numeric features / ell (dpad_num rows), their norms, and
// one-hot codes into c->bcat, from the values; cat_dpad(c) rows
// the candidates' 128-byte code rows of one 256-candidate workgroup, written
// coalesced: each thread sets its codes as bits in LDS (bits [256][stride],
// stride = cat_k / 32 + 1 dwords), then every 128-column block is expanded to
// bytes through an LDS image and stored as whole rows (propose.hip)
__device__ inline void store_code_rows(const uint32_t* bits, int32_t stride, int32_t nkb, uint32_t* img, int8_t* bcat,
                                int64_t ldu, int64_t i0) {
  const int t = threadIdx.x;
  for (int32_t kb = 0; kb < nkb; ++kb) {
    // this thread's 128 codes of block kb: bits 4w .. 4w + 3 -> the 4 bytes of dword w
#pragma unroll
    for (int w = 0; w < 32; ++w) {
      const uint32_t b = (bits[t * stride + kb * 4 + (w >> 3)] >> ((w & 7) * 4)) & 15u;
      img[t * 33 + w] = (b & 1u) | ((b & 2u) << 7) | ((b & 4u) << 14) | ((b & 8u) << 21);
    }
    __syncthreads();
    // the block's 256 rows of 128 bytes are contiguous in bcat: 16-byte stores in order
    uint4* dst = reinterpret_cast<uint4*>(bcat + ((int64_t)kb * ldu + i0) * 128);
#pragma unroll
    for (int q = 0; q < 8; ++q) {
      const int e = q * 256 + t, r = e >> 3, c = e & 7;
      const uint32_t* src = img + r * 33 + 4 * c;
      dst[e] = make_uint4(src[0], src[1], src[2], src[3]);
    }
    __syncthreads();
  }
}

inline size_t code_rows_lds(int32_t cat_k) { return sizeof(uint32_t) * 256 * ((cat_k / 32 + 1) + 33); }
int launch_encode_scaled_cat(ut_ctx* c, const double* values, int64_t ld, int64_t m, double* u, int32_t dpad,
                             int64_t ldu, double* cn, int8_t* bcat);
int launch_xs_t(ut_ctx* c, const double* Xs, int32_t npad, int32_t d, int32_t dpad, double* XsT);
int launch_gemm_var(ut_ctx* c, int prec, const void* LinvT, int64_t lda, const void* kst, int64_t ldk, int32_t npad,
                    int64_t m, double* part, const double* beta, double* mpart);
// the fp64 contraction of cnt columns against the first `rows` rows of L^-1, the mean partials into c->pr_mpart
inline int launch_gemm_var64(ut_ctx* c, int32_t npad, const double* kst, int64_t ldk, int32_t rows, int64_t cnt,
                             double* vpart) {
  return launch_gemm_var(c, 64, c->gp_LinvT.p, npad, kst, ldk, rows, cnt, vpart, c->gp_beta.p, c->pr_mpart.p);
}
int launch_transpose(ut_ctx* c, const double* src, int32_t n, double* dst, float* dst_f);
// ---- int8-sliced fp64 tier (gp_i8.hip) ----
// six balanced 8-bit digits per operand value; tiles of the variance contraction
constexpr int I8_S = 6, I8_BM = 64, I8_BN = 64, I8_BK = 32;
constexpr int32_t I8_MAX_K = 16384;   // exact int32 group sums: K * 6 * 2^14 < 2^31
// the digit scale of K*: the smallest eb with sf2 2^-eb <= 0.49 (k* <= sf2)
inline int i8_kstar_exp(double sf2) { return ilogb(sf2 / 0.49) + 1; }
// byte offset of element (r, k) in a digit plane [K / 32][ld][32]: a 32-k piece
// of row r is 32 contiguous bytes, its 16-byte chunks swizzled by bit 3 of r
__host__ __device__ inline int64_t i8_off(int64_t r, int32_t k, int64_t ld) {
  return ((int64_t)(k >> 5) * ld + r) * 32 + ((((k >> 4) & 1) ^ (int)((r >> 3) & 1)) << 4) + (k & 15);
}
// x in [-0.49, 0.49] -> bits 0..47 = rint(x 2^48) + 0x808080808080: the fp64
// sum x + 24.5019... (24 + 0x808080808080 2^-48, exact) lies in [16, 32), so
// its ulp is 2^-48, its exponent field fixed, and its mantissa's low 48 bits
// that integer (rounded to nearest even: the offset is even); its six bytes,
// each XOR 0x80, are the balanced digits (int8) of rint(x 2^48) in base 256,
// most significant = byte 5 (bits 48.. are the exponent: ignored)
__device__ __forceinline__ uint64_t i8_biased(double x) {
  return (uint64_t)__double_as_longlong(x + 0x1.8808080808080p4);
}
// four values' biased words (lo / hi dwords) -> the six digit planes' dwords
// (byte u of plane p's dword = digit p of value u; plane 0 = most significant):
// a 4 x 4 byte transpose by v_perm_b32 (byte j of perm(a, b, s) is byte
// s_j of the pair, 0..3 = b, 4..7 = a)
typedef int32_t i8v4 __attribute__((ext_vector_type(4)));
typedef int32_t i8v16 __attribute__((ext_vector_type(16)));
__device__ __forceinline__ void i8_planes(const uint32_t (&lo)[4], const uint32_t (&hi)[4], uint32_t (&pl)[I8_S]) {
  const uint32_t t0 = __builtin_amdgcn_perm(lo[1], lo[0], 0x05010400u);   // w0.b0 w1.b0 w0.b1 w1.b1
  const uint32_t t1 = __builtin_amdgcn_perm(lo[1], lo[0], 0x07030602u);   // w0.b2 w1.b2 w0.b3 w1.b3
  const uint32_t t2 = __builtin_amdgcn_perm(lo[3], lo[2], 0x05010400u);
  const uint32_t t3 = __builtin_amdgcn_perm(lo[3], lo[2], 0x07030602u);
  const uint32_t u0 = __builtin_amdgcn_perm(hi[1], hi[0], 0x05010400u);
  const uint32_t u2 = __builtin_amdgcn_perm(hi[3], hi[2], 0x05010400u);
  pl[0] = __builtin_amdgcn_perm(u2, u0, 0x07060302u) ^ 0x80808080u;      // byte 5
  pl[1] = __builtin_amdgcn_perm(u2, u0, 0x05040100u) ^ 0x80808080u;      // byte 4
  pl[2] = __builtin_amdgcn_perm(t3, t1, 0x07060302u) ^ 0x80808080u;      // byte 3
  pl[3] = __builtin_amdgcn_perm(t3, t1, 0x05040100u) ^ 0x80808080u;      // byte 2
  pl[4] = __builtin_amdgcn_perm(t2, t0, 0x07060302u) ^ 0x80808080u;      // byte 1
  pl[5] = __builtin_amdgcn_perm(t2, t0, 0x05040100u) ^ 0x80808080u;      // byte 0
}
// fit: L^-1's planes, row scales and the error bound (c->gp_i8a, c->gp_i8rs,
// allocated beforehand by alloc_split_i8; the digit scale of K* in c->gp_i8_eb)
int alloc_split_i8(ut_ctx* c, int32_t npad);
int launch_split_i8(ut_ctx* c, int32_t n, int32_t npad);
// the variance contraction from K*'s digit planes (kst8, [6][npad/32][ldk][32]):
// part [npad / 64][ldk] column partials of |v|^2
// part / mpart: per 64-row tile the column sums of v^2 and of v beta (the mean)
// var (I8Plan::var): Masked skips the all-zero blocks of the planes' occupancy mask c->kmask
// [npad / 32][ldk / 32] (k_gp_kstar_q's), neither loaded nor multiplied; MaskedList also visits only the
// strips of k_q_screen's list, which sits behind the mask's bytes ([8] counts, [8][ceil(CT / 8)] strips
// per XCD): every other strip's part / mpart already hold their zeros
int launch_gemm_var_i8(ut_ctx* c, int32_t npad, const int8_t* kst8, int64_t ldk, int64_t m, double* part,
                       double* mpart, I8Var var);
// (for tests) columns c0 .. c0 + nc - 1 of K*'s digit planes as doubles, out [npad][nc]
// kmask (nullptr: none): a digit of a plane whose mask bit is clear reads as 0 -- true by the mask's
// definition, and what a screened call's unwritten planes need
int launch_kstar_decode_i8(ut_ctx* c, const int8_t* kst8, int32_t npad, int64_t ldk, int64_t c0, int64_t nc,
                           double* out, const uint8_t* kmask = nullptr);
// (for tests) L^-1's digit planes as the integers sum_p a_p 256^(5-p), out [npad][npad] in (row, k) order
int launch_linv_decode_i8(ut_ctx* c, int32_t npad, double* out);
// (for tests, gp_fit.hip) out [npad][npad] = the lower triangle of src, zeros above; out [n] = (double)src [n]
int launch_fit_read_lower(ut_ctx* c, const double* src, int32_t npad, double* out);
int launch_fit_read_f32(ut_ctx* c, const float* src, int64_t n, double* out);
// L^-1 [row][k] (n x n, fp64) -> scaled fp16 hi/lo planes, blocked (h3 A operand, rows padded to 256);
// the scale exponent is derived on the device from max|L^-1| (kept in gp_ctr[16..17])
int launch_split_h3(ut_ctx* c, const double* Linv, int32_t n, _Float16* dst);
int launch_to_f32(ut_ctx* c, const double* src, float* dst, int64_t n);
// gp_fit.hip: the fit kernels' issue priority (UT_FIT_SETPRIO; process-wide)
int set_fit_prio(int32_t on);
int set_fit_prio_gemm(int32_t on);   // gp_gemm.hip's fit kernels
int launch_gather_rows(ut_ctx* c, const double* values, int64_t ld, const int64_t* idx, int64_t cand_base,
                       int32_t k, double* out, int64_t ldo, const uint32_t* dig, uint32_t* out_dig);
int launch_gather_prefix_rows(ut_ctx* c, const double* values, int64_t ld, const int64_t* idx, int64_t cand_base,
                              int32_t kp, double* out);
// comm.hip: release the context's communicator (ut_ctx_destroy)
void comm_release(ut_ctx* c);

inline unsigned grid1(int64_t n, int bs) { return (unsigned)((n + bs - 1) / bs); }

}  // namespace ut
