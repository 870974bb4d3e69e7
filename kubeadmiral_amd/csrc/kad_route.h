// Which kernels one kad_schedule launches, and with what shapes: decided here, once. Pure host arithmetic (no
// HIP calls, no allocation); the launchers (kad_kernels.hip) only execute a Route. Both structs are flat int32
// records: kad_route_eval / kad_last_route (include/kad_sched.h) hand them out as arrays in this field order.
#pragma once
#include "../../include/kad_sched.h"
#include "kad_layout.h"
#include <cstdint>
#include <initializer_list>

namespace kad {

struct RouteIn {
  int32_t C, clean, fold, fitfold, TW, snap_negative;               // snapshot
  int32_t W, has_current, zero_req, batch_defer, batch_many_terms;  // batch (flags_or & KAD_W_HAS_CURRENT, ...)
  int32_t filter_mask, score_mask;                                  // profile
  // launch context. n_cu: of the device the launchers first ran on (n_cus() keeps it for the process, as ever:
  // a process driving unlike devices routes, and reports, every one of them with the first one's count)
  int32_t debug_capture, side_stream, n_cu;
  // tuning (tuning_env: measurement builds only): KAD_NO_ROWS, KAD_ROWS_AFTER, KAD_ROWS_NO_INLINE, KAD_PREP_WAVE,
  // KAD_WIDE_MIN_NCH, KAD_LEAN_BLOCKS_PER_CU (< 1: as many lean blocks per CU as the occupancy query answers)
  int32_t no_rows = 0, rows_after = 0, rows_no_inline = 0, prep_wave = 1, wide_min_nch = 5, lean_blocks_per_cu = 0;
  // the rows prep_kernel reads and writes all start on 16-byte boundaries (rows_aligned16 of BatchDev::req_mask, sw,
  // cw and SnapDev::fit_rows, taint_tab, slices): with whole lanes (nch % PREP_CPL == 0) the PREP_VEC route
  int32_t rows16 = 0;
};
static_assert(sizeof(RouteIn) == 4 * KAD_ROUTE_IN_FIELDS, "RouteIn is a flat int32 record");

// Every kernel instantiation a schedule launch can name, with its kernel (read by kad_kernels.hip's table
// alone). Families are contiguous: full, row, wide, lean (kad_k_full.h, kad_k_row.h, kad_k_wide.h, kad_k_lean.h).
#define KAD_VARIANTS(X)                                                   \
  X(FULL_LDS, schedule_kernel<false>)                                     \
  X(FULL_GSCR, schedule_kernel<true>)                                     \
  X(ROW_DEFAULT, schedule_row_kernel<SM_DEFAULT>)                         \
  X(ROW, schedule_row_kernel<-1>)                                         \
  X(WIDE_ZR, schedule_wide_kernel<WIDE_MAX_NCH, 0, -1, true>)             \
  X(WIDE, schedule_wide_kernel<WIDE_MAX_NCH, 0, -1>)                      \
  X(WIDE_LEAST_ZR, schedule_wide_kernel<WIDE_MAX_NCH, 0, SM_LEAST, true>) \
  X(WIDE_LEAST, schedule_wide_kernel<WIDE_MAX_NCH, 0, SM_LEAST>)          \
  X(WIDE8_DEFAULT_ZR, schedule_wide_kernel<8, 8, SM_DEFAULT, true>)       \
  X(WIDE8_DEFAULT, schedule_wide_kernel<8, 8, SM_DEFAULT>)                \
  X(LEAN1_CLEAN, schedule_lean_kernel<1, true>)                           \
  X(LEAN1, schedule_lean_kernel<1, false>)                                \
  X(LEAN2_CLEAN, schedule_lean_kernel<2, true>)                           \
  X(LEAN2, schedule_lean_kernel<2, false>)                                \
  X(LEAN3_CLEAN, schedule_lean_kernel<3, true>)                           \
  X(LEAN3, schedule_lean_kernel<3, false>)                                \
  X(LEAN4_CLEAN_LEAST, schedule_lean_kernel<4, true, SM_LEAST>)           \
  X(LEAN4_CLEAN, schedule_lean_kernel<4, true>)                           \
  X(LEAN4, schedule_lean_kernel<4, false>)                                \
  X(LEAN0_DEFAULT, schedule_lean_kernel<0, false, SM_DEFAULT>)            \
  X(LEAN0, schedule_lean_kernel<0, false>)
#define X(n, ...) KV_##n,
enum Variant : int32_t { KAD_VARIANTS(X) KV_COUNT };
#undef X
inline const char* variant_name(int v) {
#define X(n, ...) #n,
  static const char* const names[KV_COUNT] = {KAD_VARIANTS(X)};
#undef X
  return v >= 0 && v < KV_COUNT ? names[v] : "?";
}
enum : int32_t { PREP = 0, PREP_WAVE2, PREP_WAVE3, PREP_WAVE4, PREP_VEC, PREP_COUNT };  // PREP_VEC: prep_kernel<true>
enum : int32_t { FAMILY_LEAN = 0, FAMILY_WIDE };
enum : int32_t { ROWS_NONE = 0, ROWS_INLINE, ROWS_BESIDE, ROWS_AFTER };

constexpr int32_t SM_LEAST = 1 << KAD_PL_LEAST_ALLOCATED;
constexpr int32_t SM_DEFAULT = (1 << KAD_PL_TAINT_TOLERATION) | (1 << KAD_PL_BALANCED_ALLOCATION) |
                               (1 << KAD_PL_LEAST_ALLOCATED) | (1 << KAD_PL_CLUSTER_AFFINITY);

struct Route {
  int32_t prep, prep_lanes;  // PREP*; prep_kernel lanes per unit
  int32_t family, variant;   // FAMILY_*; the main kernel
  int32_t row_variant, full_variant;  // the row kernel's and the defer pass's, where they run
  int32_t use_rows, early_rows, may_defer;  // BatchDev's flags of the same names
  int32_t rows, defer_pass;  // ROWS_*; schedule_kernel over the defer list afterwards
  int32_t cache_ne, cache_pn, cache_zs;
  int32_t wpb, threads, lds, wave_bytes;  // the main kernel's waves per block, block size, dynamic LDS, of it per wave
  int32_t grid, batch, row_grid;  // by route_grids; all 0 at W == 0, row_grid 0 unless ROWS_BESIDE / ROWS_AFTER
};
static_assert(sizeof(Route) == 4 * KAD_ROUTE_FIELDS, "Route is a flat int32 record");

inline int route_nch(int C) { return (C + 63) >> 6; }
// prep_kernel lanes per unit (a power of two <= 64 lets it count a unit's feasible clusters in one wave)
inline int prep_lanes_per_unit(int C) { return C > 0 ? (route_nch(C) + PREP_CPL - 1) / PREP_CPL : 1; }
// RouteIn::rows16: 1 if every address is a multiple of 16 bytes (a null pointer, a table this snapshot or batch
// does not have, is never read and counts as aligned)
inline int32_t rows_aligned16(std::initializer_list<const void*> bases) {
  uintptr_t any = 0;
  for (const void* p : bases) any |= reinterpret_cast<uintptr_t>(p);
  return (any & 15) == 0;
}
// prep_kernel's 16-byte row accesses need every lane to own PREP_CPL whole chunks (so a row's words at a lane
// are PREP_CPL consecutive ones at a multiple of PREP_CPL, no clamped tail) and 16-byte aligned bases
inline bool prep_vec_ok(int nch, int rows16) { return PREP_CPL % 2 == 0 && nch > 0 && nch % PREP_CPL == 0 && rows16 != 0; }
// the wide kernel takes clean snapshots with min_nch <= nch <= WIDE_MAX_NCH
// (KAD_WIDE_MIN_NCH overrides the lower bound, for A/B runs of C <= 256)
inline bool route_wide(int C, int clean, int min_nch) {
  const int nch = route_nch(C);
  return clean && nch >= min_nch && nch >= 1 && nch <= WIDE_MAX_NCH;
}
inline bool row_kernel_fits(int C) { return C > 0 && C <= ROW_MAX_C; }
inline size_t row_kernel_lds(int C) { return rowk_layout(C).bytes; }

inline Route route_schedule(const RouteIn& in) {
  Route r{};
  const int nch = route_nch(in.C);
  // wide snapshots (more than 64 chunks, up to 256): prep takes one unit per wave
  const int cw = (nch + 63) / 64;
  r.prep = (nch > 64 && cw <= 4 && in.prep_wave) ? PREP_WAVE2 + (cw - 2) : (prep_vec_ok(nch, in.rows16) ? PREP_VEC : PREP);
  const int per = r.prep_lanes = prep_lanes_per_unit(in.C);
  const bool wide = route_wide(in.C, in.clean, in.wide_min_nch);
  // long feasible lists go to schedule_row_kernel when every filter is in the static words
  r.use_rows = !in.no_rows && in.clean && in.fold && in.fitfold && row_kernel_fits(in.C);
  r.early_rows = r.use_rows && !in.rows_after && wide && (per & (per - 1)) == 0 && per <= 64 && !in.debug_capture;
  // can any unit reach the defer list (schedule_kernel)? The wide kernel with early routing (every filter in
  // the static words, long lists routed by prep) defers only the units batch_defer names; the row path also
  // those with more preferred terms than it holds. Otherwise the lean kernel's own reasons, and on the wide
  // path without early routing, lists past WIDE_P.
  const bool rows_defer = in.batch_many_terms && (in.score_mask & (1 << KAD_PL_CLUSTER_AFFINITY));
  r.may_defer = in.batch_defer || in.debug_capture ||
                (wide ? !r.early_rows || rows_defer : in.snap_negative || in.TW > 1);
  r.row_variant = in.score_mask == SM_DEFAULT ? KV_ROW_DEFAULT : KV_ROW;  // the default set's scores as constants (C5)
  r.full_variant = row_layout(in.C).bytes <= (size_t)LDS_BUDGET ? KV_FULL_LDS : KV_FULL_GSCR;
  r.cache_ne = (in.filter_mask & (1 << KAD_PL_TAINT_TOLERATION)) && in.has_current;
  r.cache_pn = (in.score_mask >> KAD_PL_TAINT_TOLERATION) & 1;
  if (wide) {
    r.family = FAMILY_WIDE;
    const size_t per_wave = r.wave_bytes = (int32_t)wide_layout().bytes;
    const bool s_res = in.score_mask & ((1 << KAD_PL_LEAST_ALLOCATED) | (1 << KAD_PL_MOST_ALLOCATED) |
                                        (1 << KAD_PL_BALANCED_ALLOCATION));
    // zero-request batches: the resource-score column, when it costs no wave (LDS beside the 16 wave regions)
    r.cache_zs = KAD_WIDE_ZS && s_res && in.zero_req &&
                 wide_cache_bytes(in.C, r.cache_ne, r.cache_pn, 1) + (size_t)(WIDE_THREADS / 64) * per_wave <= (size_t)LDS_MAX;
    const size_t cache = wide_cache_bytes(in.C, r.cache_ne, r.cache_pn, r.cache_zs);
    const int wpb = (int)(((size_t)LDS_MAX - cache) / per_wave);
    r.wpb = wpb > WIDE_THREADS / 64 ? WIDE_THREADS / 64 : wpb;
    r.lds = (int32_t)(cache + (size_t)r.wpb * per_wave);
    // the instantiation: the score set of the bench profiles (C2/C3: LeastAllocated alone, which compiles the
    // folded filter only; C4: the default set, also at its exact 8 chunks — 16 exact chunks unroll past the
    // 128-VGPR budget and spill), else generic; each with and without the zero-request column
    const int sel = in.fold && in.fitfold && nch == 16 && in.score_mask == SM_LEAST ? 1
                                                                                     : (nch == 8 && in.score_mask == SM_DEFAULT ? 2 : 0);
    r.variant = KV_WIDE_ZR + 2 * sel + (r.cache_zs ? 0 : 1);
    // the routed long units inside the wide kernel (its opening phase) when the row body's LDS fits below
    // the cluster cache (it needs >= 2 waves: wave 1 dequeues and prefetches while wave 0 replays); else the
    // row kernel beside it on a second stream, else after it
    const bool fits = !in.rows_no_inline && r.wpb >= 2 && row_kernel_lds(in.C) <= (size_t)r.wpb * per_wave;
    r.rows = r.early_rows && fits ? ROWS_INLINE
                                  : (r.early_rows && in.side_stream ? ROWS_BESIDE : (r.use_rows ? ROWS_AFTER : ROWS_NONE));
    // the defer pass only when some unit can reach the defer list (may_defer, host-checked: REC_FULL units,
    // requests or affinity weights outside the exact path, rows with more preferred terms than ROW_MAX_TERMS,
    // or units past WIDE_P without early routing)
    r.defer_pass = r.may_defer;
  } else {
    r.family = FAMILY_LEAN;
    const bool cl = in.clean && nch >= 1 && nch <= 4;
    r.wpb = 4;
    r.wave_bytes = (int32_t)lean_layout(in.C, lean_qmax(nch <= 4 ? nch : 0)).bytes;
    r.lds = r.wave_bytes * r.wpb + (nch <= 4 ? (int32_t)lean_cache_bytes(in.C, 6 + r.cache_ne + r.cache_pn + (cl ? 1 : 0)) : 0);
    // score-set specialisations of the bench profiles: C2 (4 clean chunks, LeastAllocated alone), C5 (long
    // lists, the default set)
    if (nch >= 1 && nch <= 3)
      r.variant = KV_LEAN1_CLEAN + 2 * (nch - 1) + (cl ? 0 : 1);
    else if (nch == 4)
      r.variant = cl ? (in.score_mask == SM_LEAST ? KV_LEAN4_CLEAN_LEAST : KV_LEAN4_CLEAN) : KV_LEAN4;
    else
      r.variant = in.score_mask == SM_DEFAULT && nch > 4 ? KV_LEAN0_DEFAULT : KV_LEAN0;
    r.rows = nch > 4 && r.use_rows ? ROWS_AFTER : ROWS_NONE;
    // nch <= 4: nothing can be deferred without may_defer (host-checked: every unit and cluster is in the lean
    // kernel's range and every feasible list fits its registers)
    r.defer_pass = nch > 4 || r.may_defer;
  }
  r.threads = 64 * r.wpb;
  return r;
}

// The grids and the work-queue batch size. per_cu / row_per_cu: hipOccupancyMaxActiveBlocksPerMultiprocessor's
// answers (< 1: failed, taken as 1) for the main kernel — the lean family only: the wide kernel runs one block
// per CU — and for the row kernel.
inline void route_grids(const RouteIn& in, Route& r, int per_cu, int row_per_cu) {
  if (in.W == 0) return;
  const long need = ((long)in.W + r.wpb - 1) / r.wpb;  // at least one unit per wave
  long grid = in.n_cu;
  if (r.family == FAMILY_LEAN)  // one wave per resident slot: contiguous equal shares, no tail of late blocks
    grid *= in.lean_blocks_per_cu >= 1 ? in.lean_blocks_per_cu : (per_cu < 1 ? 1 : per_cu);
  r.grid = (int32_t)(grid > need ? need : grid);
  const long upw = ((long)in.W + (long)r.grid * r.wpb - 1) / ((long)r.grid * r.wpb);  // units per wave
  // wide: 4 units, 3 when the waves take fewer than 64 units each (a 125k-unit shard: the last batches are the
  // tail; at 1M units 3-unit batches cost more in dequeue atomics than they save: profiles/r05/ab_wide_batch_c3.txt)
  // lean: at most LEAN_BATCH (one VGPR of UnitRecs), small enough that every wave takes >= 12 batches, so the
  // waves run out of work together (C2: 16 units per wave → 1-unit batches)
  if (r.family == FAMILY_WIDE)
    r.batch = upw < 64 ? 3 : WQ_BATCH;
  else
    r.batch = upw / 6 < 1 ? 1 : (upw / 6 > LEAN_BATCH ? LEAN_BATCH : (int32_t)(upw / 6));
  if (r.rows == ROWS_BESIDE || r.rows == ROWS_AFTER) {
    const long rg = (long)in.n_cu * (row_per_cu < 1 ? 1 : row_per_cu);
    r.row_grid = (int32_t)(rg > ROW_MAX_BLOCKS ? ROW_MAX_BLOCKS : rg);
    if (r.row_grid > in.W) r.row_grid = in.W;
  }
}

}  // namespace kad
