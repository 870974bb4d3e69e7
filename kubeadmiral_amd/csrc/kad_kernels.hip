// The schedule kernels' translation unit of libkad.so for gfx950 (MI355X, CDNA4): the kernels, one family per
// header (kad_k_*.h, with kad_prof.h, kad_score.h, kad_kargs.h and kad_wq.h between them), and their launchers.
//
// schedule_kernel — one 64-lane wavefront per SchedulingUnit:
//   filters (ballot bitmask) → raw scores → per-row max → normalisation →
//   totals → MaxCluster first-k set (radix select + restricted pdqsort replay)
//   → ascending cluster-id output via ballot compaction.
//   Reference: genericScheduler.Schedule, core/generic_scheduler.go:92-150.
// plan_kernel — one wavefront per Divide-mode unit with ≥1 selected cluster:
//   ClusterCapacityWeight (rsp.go:65-181) + planner.Plan (planner.go:83-366).
//
// Nothing here is a dense contraction (no MFMA). Cluster attributes are read
// attribute-major (attr[i*C + c]) so each wave's 64 lanes read 64 consecutive
// clusters: one coalesced 512-B access per i64 attribute. Per-row state lives
// in LDS (per-wave region) when it fits, else in a per-wave global scratch slab.
#include <cstdlib>

#include <type_traits>

#include "kad_affinity.h"
#include "kad_device.h"
#include "kad_plan.h"
#include "kad_select.h"
#include "kad_wave.h"
// the kernels in definition order, which the code object's layout follows (as it does the order of the
// includes above: kad_plan.h and kad_select.h define device functions that are not inlined)
#include "kad_kargs.h"
#include "kad_prof.h"
#include "kad_k_rows.h"
#include "kad_score.h"
#include "kad_k_full.h"
#include "kad_k_prep.h"
#include "kad_wq.h"
#include "kad_k_lean.h"
#include "kad_k_wide.h"
#include "kad_k_row.h"
#include "kad_k_plan.h"
#include "kad_k_stage.h"

namespace kad {

size_t select_wave_bytes(int C) { return row_layout(C).bytes; }
size_t plan_wave_bytes(int K) { return plan_layout(K).bytes; }

// ================================================================ launchers
int debug_phase_counters(uint64_t* out, int reset) {
#ifdef KAD_PHASE_PROF
  if (reset == -3 || reset == -4) {  // the wide kernel's per-unit trace: out holds 2^20 entries
    const hipError_t e = reset == -3 ? hipMemcpyFromSymbol(out, HIP_SYMBOL(g_ustart), sizeof(unsigned long long) * KAD_UTRACE_MAX)
                                     : hipMemcpyFromSymbol(out, HIP_SYMBOL(g_uinfo), sizeof(unsigned long long) * KAD_UTRACE_MAX);
    return e == hipSuccess ? KAD_UTRACE_MAX : -1;
  }
  if (reset == -2) {  // the wide kernel's per-wave extras: out holds 8192 * 6 entries
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wavex), sizeof(unsigned long long) * 8192 * 6) != hipSuccess) return -1;
    return 8192;
  }
  if (reset < 0) {  // the lean kernel's per-wave (start, end) timestamps: out holds 8192 * 2 entries
    if (hipMemcpyFromSymbol(out, HIP_SYMBOL(g_wavetime), sizeof(unsigned long long) * 8192 * 2) != hipSuccess) return -1;
    return 8192;
  }
  static unsigned long long h[256 * KAD_PSLOTS];
  if (hipMemcpyFromSymbol(h, HIP_SYMBOL(g_phase), sizeof h) != hipSuccess) return -1;
  for (int i = 0; i < KAD_PSLOTS; ++i) {
    out[i] = 0;
    for (int s = 0; s < 256; ++s) out[i] += h[s * KAD_PSLOTS + i];
  }
  if (reset) {
    static const unsigned long long z[256 * KAD_PSLOTS] = {};
    if (hipMemcpyToSymbol(HIP_SYMBOL(g_phase), z, sizeof z) != hipSuccess) return -1;
  }
  return KAD_PSLOTS;
#else
  (void)out;
  (void)reset;
  return 0;
#endif
}

static constexpr int MAX_RESIDENT_WAVES = 256 * 32;

hipError_t launch_req_masks(const SnapDev& s, const BatchDev& b, hipStream_t st, bool zero_rows, bool* zeroed) {
  (void)hipGetLastError();
  const int nch = (s.C + 63) >> 6;
  const long lanes = (long)b.n_rowreq * ((nch + REQ_RC - 1) / REQ_RC);
  *zeroed = zero_rows && lanes > 0;
  if (lanes > 0)
    hipLaunchKernelGGL(req_row_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, s, b, zero_rows ? 1 : 0);
  const int ngrp = (nch + REQ_G - 1) / REQ_G;
  const long waves = (long)b.n_seg * ngrp;
  if (waves > 0) hipLaunchKernelGGL(req_mask_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, s, b, ngrp);
  return hipGetLastError();
}

hipError_t launch_value_rows(const SnapDev& s, uint64_t* vrows, hipStream_t st) {
  (void)hipGetLastError();
  const long waves = (long)s.K * ((s.C + 63) >> 6);
  if (waves == 0) return hipSuccess;
  hipLaunchKernelGGL(value_rows_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, s, vrows);
  return hipGetLastError();
}

hipError_t launch_res_cols(const SnapDev& s, void* buf, hipStream_t st) {
  (void)hipGetLastError();
  if (s.C <= 0) return hipSuccess;
  double4* r4 = static_cast<double4*>(buf);
  ulonglong4* p4 = s.TW <= 4 ? reinterpret_cast<ulonglong4*>(static_cast<char*>(buf) + res_cols_pns4_offset(s.C)) : nullptr;
  hipLaunchKernelGGL(res_cols_kernel, dim3((unsigned)((s.C + 255) / 256)), dim3(256), 0, st, s, r4,
                     reinterpret_cast<float2*>(r4 + s.C), p4);
  return hipGetLastError();
}

hipError_t launch_slices(const SnapDev& s, uint64_t* slices, hipStream_t st) {
  (void)hipGetLastError();
  const int nch = (s.C + 63) >> 6;
  const long waves = (128L * s.TW + 64L * s.GW) * nch;
  if (waves == 0) return hipSuccess;
  hipLaunchKernelGGL(slice_kernel, dim3((unsigned)((waves + 3) / 4)), dim3(256), 0, st, s, slices);
  const long lanes = 2L * 8 * s.TW * 256 * nch;
  hipLaunchKernelGGL(taint_table_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, s,
                     slices + (128L * s.TW + 64L * s.GW) * nch);
  return hipGetLastError();
}

// The prep and schedule kernels by route id (kad_route.h: PREP*, KAD_VARIANTS): the one list of their
// instantiations, for the LDS attribute, the occupancy queries and the launches.
static void (*const PREP_FN[PREP_COUNT])(SnapDev, BatchDev, ProfDev, int) = {
    prep_kernel<false>, prep_wave_kernel<2>, prep_wave_kernel<3>, prep_wave_kernel<4>, prep_kernel<true>};
#define X(n, ...) (const void*)__VA_ARGS__,
static const void* const VARIANT_FN[KV_COUNT] = {KAD_VARIANTS(X)};
#undef X
// the argument struct the launchers cast each family's entries back to
template <int V>
using VariantArgs = std::conditional_t<V <= KV_FULL_GSCR, SchedArgs, std::conditional_t<V <= KV_ROW, RowArgs,
                    std::conditional_t<V <= KV_WIDE8_DEFAULT, WideArgs, LeanArgs>>>;
#define X(n, ...) static_assert(std::is_same<decltype(&__VA_ARGS__), void (*)(VariantArgs<KV_##n>)>::value, #n);
KAD_VARIANTS(X)
#undef X

hipError_t launch_prep(const SnapDev& s, const BatchDev& b, const ProfDev& p, bool force_full, const Route& r,
                       hipStream_t st) {
  (void)hipGetLastError();
  // prep_kernel: prep_lanes lanes per unit; prep_wave_kernel: one unit per wave (not persistent: C5's prep is
  // L2-miss bound and took 587 -> 729 us with the resident grid, profiles/r06/ab_c5_prep_persistent.txt)
  if (r.prep < 0 || r.prep >= PREP_COUNT) return hipErrorInvalidValue;
  const long grid = r.prep == PREP || r.prep == PREP_VEC ? ((long)b.W * r.prep_lanes + 255) / 256 : ((long)b.W + 3) / 4;
  // (one block at W = 0 still resets defer_n)
  hipLaunchKernelGGL(PREP_FN[r.prep], dim3((unsigned)(grid > 0 ? grid : 1)), dim3(256), 0, st, s, b, p, force_full ? 1 : 0);
  return hipGetLastError();
}

int n_cus() {
  static int n_cu = 0;
  int dev = 0;
  if (n_cu == 0 && (hipGetDevice(&dev) != hipSuccess || hipDeviceGetAttribute(&n_cu, hipDeviceAttributeMultiprocessorCount, dev) != hipSuccess || n_cu <= 0)) n_cu = 256;
  return n_cu;
}

// schedule_kernel over the defer list: its length is only known on the device, so the grid strides over it
// (waves past its end exit at once)
static hipError_t launch_defer_pass(const SnapDev& s, const BatchDev& b, const OutDev& o, const ProfDev& p, const Route& r,
                                    void* gscr, size_t scr_bytes, hipStream_t st) {
  const size_t wb = row_layout(s.C).bytes;
  const auto fn = (void (*)(SchedArgs))VARIANT_FN[r.full_variant];
  if (r.full_variant == KV_FULL_LDS) {
    int wpb2 = (int)(LDS_BUDGET / wb);
    wpb2 = wpb2 > 4 ? 4 : (wpb2 < 1 ? 1 : wpb2);
    long waves2 = b.W < 256 * 16 ? b.W : 256 * 16;
    const int grid2 = (int)((waves2 + wpb2 - 1) / wpb2);
    const SchedArgs A2{s, b, o, p, nullptr, (int)wb, wpb2, grid2 * wpb2, b.defer, b.defer_n};
    hipLaunchKernelGGL(fn, dim3(grid2), dim3(64 * wpb2), wb * wpb2, st, A2);
  } else {  // rows too large for LDS: per-wave global scratch slabs
    size_t slots = scr_bytes / wb;
    if (slots < 1) return hipErrorInvalidValue;
    if (slots > (size_t)MAX_RESIDENT_WAVES) slots = MAX_RESIDENT_WAVES;
    if (slots > (size_t)b.W) slots = b.W;
    const SchedArgs A2{s, b, o, p, (char*)gscr, (int)wb, 1, (int)slots, b.defer, b.defer_n};
    hipLaunchKernelGGL(fn, dim3((int)slots), dim3(64), small_layout(s.C).bytes, st, A2);
  }
  return hipGetLastError();
}

// schedule_row_kernel over BatchDev::rows (its length is only known on the device: the persistent
// workgroups dequeue until the list is drained)
static hipError_t launch_rows(const SnapDev& s, const BatchDev& b, const OutDev& o, const ProfDev& p, const Route& r,
                              hipStream_t st) {
  static const int exp = tuning_env("KAD_ROW_EXPERIMENT", 0);
  const RowArgs A{s, b, o, p, b.row_slabs, exp};
  hipLaunchKernelGGL((void (*)(RowArgs))VARIANT_FN[r.row_variant], dim3((unsigned)r.row_grid), dim3(ROW_THREADS),
                     row_kernel_lds(s.C), st, A);
  return hipGetLastError();
}

hipError_t launch_schedule(const SnapDev& s, const BatchDev& b, const OutDev& o, const ProfDev& p, const RouteIn& in,
                           Route& r, void* gscr, size_t scr_bytes, hipStream_t st, hipEvent_t after_main,
                           hipEvent_t after_rows, hipStream_t side, hipEvent_t fork, hipEvent_t join) {
  auto rec = [&](hipEvent_t ev) { return ev ? hipEventRecord(ev, st) : hipSuccess; };
  (void)hipGetLastError();  // clear any stale error so the check below is this launch's
  if (b.W == 0) return hipSuccess;
  if (r.wpb < 1) return hipErrorInvalidValue;
  const bool beside = r.rows == ROWS_BESIDE, row_launch = beside || r.rows == ROWS_AFTER;
  // Up front, where the parent did them beside each launch: the row and wide kernels' LDS limit (all eight at the
  // first launch that runs one), the slab check and both occupancy queries — before any kernel is launched.
  static bool attr = false;
  if (!attr && (row_launch || r.family == FAMILY_WIDE)) {
    for (int v = KV_ROW_DEFAULT; v <= KV_WIDE8_DEFAULT; ++v)
      if (hipError_t e = hipFuncSetAttribute(VARIANT_FN[v], hipFuncAttributeMaxDynamicSharedMemorySize, LDS_MAX)) return e;
    attr = true;
  }
  if (row_launch && !b.row_slabs) return hipErrorInvalidValue;
  auto per_cu = [](const void* fn, int threads, size_t lds) {  // (a failed query: 0, which route_grids takes as 1)
    int n = 0;
    return hipOccupancyMaxActiveBlocksPerMultiprocessor(&n, fn, threads, lds) == hipSuccess ? n : 0;
  };
  route_grids(in, r, r.family == FAMILY_LEAN ? per_cu(VARIANT_FN[r.variant], r.threads, r.lds) : 0,
              row_launch ? per_cu(VARIANT_FN[r.row_variant], ROW_THREADS, row_kernel_lds(s.C)) : 0);
  if (beside) {  // the row kernel on the side stream, from the end of prep_kernel, beside the wide kernel
    if (hipError_t e = hipEventRecord(fork, st)) return e;
    if (hipError_t e = hipStreamWaitEvent(side, fork, 0)) return e;
    if (hipError_t e = launch_rows(s, b, o, p, r, side)) return e;
    if (hipError_t e = hipEventRecord(join, side)) return e;
  }
  if (r.family == FAMILY_WIDE) {
    static const int exp = tuning_env("KAD_WIDE_EXPERIMENT", 0);
    const WideArgs A{s, b, o, p, r.wpb, r.cache_ne, r.cache_pn, r.cache_zs, r.rows == ROWS_INLINE ? 1 : 0, r.batch, exp};
    hipLaunchKernelGGL((void (*)(WideArgs))VARIANT_FN[r.variant], dim3((unsigned)r.grid), dim3(r.threads), r.lds, st, A);
  } else {
    const LeanArgs A{s, b, o, p, r.wave_bytes, r.wpb, r.batch, r.cache_ne, r.cache_pn};
    hipLaunchKernelGGL((void (*)(LeanArgs))VARIANT_FN[r.variant], dim3((unsigned)r.grid), dim3(r.threads), r.lds, st, A);
  }
  hipError_t e = hipGetLastError();
  if (e == hipSuccess) e = rec(after_main);
  if (beside) {
    // joined even when the main launch failed: the row kernel on the side stream must finish before
    // anything later on st (the next batch upload) can overwrite what it reads
    const hipError_t j = hipStreamWaitEvent(st, join, 0);
    if (e == hipSuccess) e = j;
  } else if (e == hipSuccess && row_launch) {
    e = launch_rows(s, b, o, p, r, st);
  }
  if (e != hipSuccess) return e;
  if (hipError_t e2 = rec(after_rows)) return e2;
  return r.defer_pass ? launch_defer_pass(s, b, o, p, r, gscr, scr_bytes, st) : hipSuccess;
}

hipError_t launch_plan_hdr(const BatchDev& b, const int32_t* rows, int n_rows, PlanRowHdr* out, hipStream_t st) {
  (void)hipGetLastError();
  if (n_rows <= 0) return hipSuccess;
  hipLaunchKernelGGL(plan_hdr_kernel, dim3((unsigned)((n_rows + 255) / 256)), dim3(256), 0, st, b, rows, n_rows, out);
  return hipGetLastError();
}

constexpr int PLAN_OVERSUB = 8;  // register planners' grid over the resident block count (launch_plan)
hipError_t launch_plan(const SnapDev& s, const BatchDev& b, const OutDev& o, const ProfDev& p, const PlanRowHdr* rows,
                       int n_rows, int kmax, void* gscr, size_t scr_bytes, hipStream_t st, int32_t* big, int32_t* big_n) {
  (void)hipGetLastError();  // clear any stale error so the check below is this launch's
  (void)p;
  if (n_rows == 0 || kmax <= 0) return hipSuccess;
  const int cp = (s.C + 63) & ~63;
  // grid: `over` times the resident block count, rows round-robin (r += grid). The pair planner takes up to
  // PLAN_OVERSUB = 8 (at least 16 rows per wave): each wave's rows are an eighth of a persistent wave's, and the
  // hardware starts the next waves as earlier ones finish — with a fixed stride per resident wave, the waves
  // whose rows held the most rounds set the kernel's end (C4: planner 1.463 -> 1.276 ms, step 2.29 -> 2.10 ms;
  // 16x equal, 32x / 64x slower: profiles/r06/ab_c4_plan_grid.txt). Small row sets (C5's) and the list kernel
  // (its rows are known on the device only) keep the resident grid: extra waves there only start and exit.
  auto persistent = [&](const void* fn, size_t lds, int over = 1) {
    int per_cu = 0;
    if (hipOccupancyMaxActiveBlocksPerMultiprocessor(&per_cu, fn, 64, lds) != hipSuccess || per_cu < 1) per_cu = 8;
    const long res = (long)n_cus() * per_cu;
    long grid = res * over;
    if (over > 1 && grid > n_rows / 16) grid = n_rows / 16 > res ? n_rows / 16 : res;
    return (int)(grid > n_rows ? n_rows : grid);
  };
  static const int over = tuning_env("KAD_PLAN_GRID_MULT", PLAN_OVERSUB);
  // rows of K <= 64: the register planners, lookup tables only in LDS. Two rows per wave for K <= 32
  // (plan_pair_kernel: u16 tables, 8 B per cluster for the two segments), then the rows of 32 < K <= 64 it
  // listed, one per wave (plan_kernel<false, true>: u32 tables, 8 B per cluster)
  {
    const int tbl_cp = cp <= 1024 ? cp : 0;
    const size_t lds = (size_t)tbl_cp * 8 + 64 * 8;  // tables + sort keys
    static const int pairs = tuning_env("KAD_PLAN_PAIRS", 1);
    if (pairs && big) {
      if (hipError_t e = hipMemsetAsync(big_n, 0, sizeof(int32_t), st)) return e;
      const int grid = persistent((const void*)plan_pair_kernel, lds, over);
      hipLaunchKernelGGL(plan_pair_kernel, dim3((unsigned)grid), dim3(64), lds, st, s, b, o, rows, n_rows, grid, tbl_cp,
                         big, big_n);
      if (hipError_t e = hipGetLastError()) return e;
      const int grid2 = persistent((const void*)plan_kernel<false, true>, lds);
      hipLaunchKernelGGL((plan_kernel<false, true>), dim3((unsigned)grid2), dim3(64), lds, st, s, b, o, rows, n_rows,
                         kmax, (char*)nullptr, 0, grid2, tbl_cp, (const int32_t*)big, (const int32_t*)big_n);
    } else {
      const int grid = persistent((const void*)plan_kernel<false, true>, lds, over);
      hipLaunchKernelGGL((plan_kernel<false, true>), dim3((unsigned)grid), dim3(64), lds, st, s, b, o, rows, n_rows,
                         kmax, (char*)nullptr, 0, grid, tbl_cp, (const int32_t*)nullptr, (const int32_t*)nullptr);
    }
    if (hipError_t e = hipGetLastError()) return e;
  }
  if (kmax <= WAVE) return hipSuccess;
  // rows of K > 64: the workspace planner
  const size_t wb = plan_layout(kmax).bytes;
  // per-wave lookup tables (8 B per cluster) when they fit beside the row state
  const int tbl_cp = (cp <= 1024 && wb + (size_t)cp * 8 <= (size_t)LDS_BUDGET) ? cp : 0;
  const size_t wbt = wb + (size_t)tbl_cp * 8;
  if (wbt <= (size_t)LDS_BUDGET) {
    const int grid = persistent((const void*)plan_kernel<false, false>, wbt);
    hipLaunchKernelGGL((plan_kernel<false, false>), dim3((unsigned)grid), dim3(64), wbt, st, s, b, o, rows, n_rows,
                       kmax, (char*)nullptr, (int)wb, grid, tbl_cp);
  } else {
    size_t slots = scr_bytes / wb;
    if (slots < 1) return hipErrorInvalidValue;
    if (slots > (size_t)MAX_RESIDENT_WAVES) slots = MAX_RESIDENT_WAVES;
    if (slots > (size_t)n_rows) slots = n_rows;
    hipLaunchKernelGGL((plan_kernel<true, false>), dim3(slots), dim3(64), 0, st, s, b, o, rows, n_rows, kmax,
                       (char*)gscr, (int)wb, (int)slots, 0);
  }
  return hipGetLastError();
}

hipError_t launch_select_rows(int n_rows, const int32_t* row_off, const int64_t* scores, const int64_t* maxc,
                              uint32_t pflags, int kmax, int32_t* out_count, int32_t* out_sel, int32_t* out_status,
                              void* gscr, size_t scr_bytes, hipStream_t st) {
  (void)hipGetLastError();  // clear any stale error so the check below is this launch's
  if (n_rows == 0) return hipSuccess;
  const size_t wb = row_layout(kmax < 1 ? 1 : kmax).bytes;
  if (wb <= (size_t)LDS_BUDGET) {
    hipLaunchKernelGGL(select_rows_kernel<false>, dim3(n_rows), dim3(64), wb, st, n_rows, row_off, scores, maxc,
                       pflags, out_count, out_sel, out_status, (char*)nullptr, (int)wb, kmax < 1 ? 1 : kmax, n_rows);
  } else {
    size_t slots = scr_bytes / wb;
    if (slots < 1) return hipErrorInvalidValue;
    if (slots > (size_t)n_rows) slots = n_rows;
    hipLaunchKernelGGL(select_rows_kernel<true>, dim3(slots), dim3(64), 0, st, n_rows, row_off, scores, maxc, pflags,
                       out_count, out_sel, out_status, (char*)gscr, (int)wb, kmax, (int)slots);
  }
  return hipGetLastError();
}

hipError_t launch_plan_rows(const PlanRowsDev& r, int kmax, int force_ws, void* gscr, size_t scr_bytes,
                            hipStream_t st) {
  (void)hipGetLastError();  // clear any stale error so the check below is this launch's
  if (r.n_rows == 0 || kmax <= 0) return hipSuccess;
  const size_t wb = plan_layout(kmax).bytes;
  // force_ws (kad_debug_plan_force_workspace, tests): rows of K <= 64 through the LDS-workspace planner too
  if (wb <= (size_t)LDS_BUDGET) {
    hipLaunchKernelGGL(plan_rows_kernel<false>, dim3(r.n_rows), dim3(64), wb, st, r, (char*)nullptr, (int)wb,
                       r.n_rows, force_ws);
  } else {
    size_t slots = scr_bytes / wb;
    if (slots < 1) return hipErrorInvalidValue;
    if (slots > (size_t)r.n_rows) slots = r.n_rows;
    hipLaunchKernelGGL(plan_rows_kernel<true>, dim3(slots), dim3(64), 0, st, r, (char*)gscr, (int)wb, (int)slots,
                       force_ws);
  }
  return hipGetLastError();
}

}  // namespace kad
