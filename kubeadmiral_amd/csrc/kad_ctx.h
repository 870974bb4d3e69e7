// The context behind the C ABI (include/kad_sched.h) and the host helpers every entry point shares: each
// stage's host half (kad_api.hip, and every consumer's .hip below its kernels) includes this; it includes no
// consumer's header. The first part needs no HIP (KAD_HOST_ONLY stops there: tests/arena_main.cpp).
#pragma once

#include <atomic>
#include <climits>
#include <cstdint>

#include "kad_pool.h"

// [lo, hi) pieces of n on up to 16 host threads
template <class F>
inline void host_parallel(int n, F f, int serial_below = 4096) {
  const int T = n < serial_below ? 1 : kadpool::pool().threads();
  if (T <= 1) {
    f(0, n);
    return;
  }
  kadpool::run_checks(T, [&](int t) { f((int)((int64_t)n * t / T), (int)((int64_t)n * (t + 1) / T)); });
}
// the smallest i in [0, n) with bad(i), or -1: pieces checked on up to 16 host threads, each
// stopping at its first failure or once an earlier one is known — the same index, so the same
// error, as one serial pass
template <class F>
inline int64_t first_bad(int64_t n, F bad) {
  if (n < 65536) {
    for (int64_t i = 0; i < n; i++)
      if (bad(i)) return i;
    return -1;
  }
  std::atomic<int64_t> best{INT64_MAX};
  const int T = kadpool::pool().threads();
  kadpool::run_checks(T, [&](int t) {
    const int64_t lo = n * t / T, hi = n * (t + 1) / T;
    for (int64_t i = lo; i < hi; i++) {
      if ((i & 1023) == 0 && i > best.load(std::memory_order_relaxed)) return;
      if (bad(i)) {
        int64_t cur = best.load();
        while (i < cur && !best.compare_exchange_weak(cur, i)) {
        }
        return;
      }
    }
  });
  const int64_t r = best.load();
  return r == INT64_MAX ? -1 : r;
}
// offsets off[0 .. n] of a CSR: missing, not starting at 0, or decreasing somewhere
template <class O>
inline bool off_bad(const O* off, int64_t n) {
  if (!off || off[0] != 0) return true;
  return first_bad(n, [off](int64_t i) { return off[i + 1] < off[i]; }) >= 0;
}
// a CSR of n rows whose entries lie in [lo, hi): bad offsets, data missing when non-empty, or an entry outside
template <class O>
inline bool csr_bad(const O* off, const int32_t* data, int64_t n, int64_t lo, int64_t hi) {
  if (off_bad(off, n)) return true;
  const int64_t m = off[n];
  if (m && !data) return true;
  return first_bad(m, [=](int64_t j) { return data[j] < lo || data[j] >= hi; }) >= 0;
}

#ifndef KAD_HOST_ONLY
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cstring>
#include <mutex>
#include <string>
#include <vector>

#include "../../include/kad_sched.h"
#include "kad_device.h"
#include "kad_groups.h"

// A device buffer that grows on demand (grow) and frees itself: a ctx member is released by kad_ctx_destroy's
// delete, a per-call one at the end of its scope — no list of buffers to keep.
struct DevBuf {
  void* p = nullptr;
  size_t cap = 0;
  DevBuf() = default;
  DevBuf(const DevBuf&) = delete;
  DevBuf& operator=(const DevBuf&) = delete;
  ~DevBuf() { release(); }
  void release() {
    if (p) (void)hipFree(p);
    p = nullptr;
    cap = 0;
  }
  template <class T>
  T* as() const { return static_cast<T*>(p); }
};

// One consumer of the scheduler's results: its staging buffer (kad_arena.h), the events
// recorded around its kernels (ev[0] the start), whether they hold a run (stage_timing), what that run launched
// (the call's route record as it stands in include/kad_sched.h: stage_ran / stage_last_route) and what its
// kad_*_debug_route forces on the next ones.
struct Stage {
  DevBuf buf;
  hipEvent_t ev[4] = {nullptr, nullptr, nullptr, nullptr};
  bool ran = false;
  int32_t route[8] = {0, 0, 0, 0, 0, 0, 0, 0};
  int route_n = 0;  // fields of `route` in use
  kad::GroupForce force;
};
enum StageId { STG_DIFF, STG_EXPLAIN, STG_OVERRIDE, STG_FOLLOWER, STG_MIGRATE, STG_TRIGGER, STG_CSTAT, STG_SAGG,
               STG_ROLLOUT, STG_DISPATCH, STG_POLICYRC, STG_SYNCNU, STG_SYNCFIN, STG_MONREC, STG_MONREP, STG_MONIO, STG_REVISION,
               STG_DELPLAN, STG_DELFIN, STG_COUNT };

// The monitor's meters (kad_monitor_*, DESIGN.md §7 "monitor"): the one consumer state that stays on the device
// between calls. One slot per meter, a column per field; allocated in steps of kad_monitor.h's MON_BTILE slots and
// zeroed, so that the report reads whole steps. live / n_slots / max_type: the host's shadow of what the calls'
// validation needs (the slot's LIVE flag, one past the highest slot ever written, the highest type id stored).
struct MonTable {
  DevBuf col[5], type_id, flags;
  int64_t cap = 0, n_slots = 0, n_live = 0;
  int32_t max_type = -1;
  std::vector<uint8_t> live;
};

struct kad_ctx {
  int device = 0;
  hipStream_t stream = nullptr;
  hipStream_t side = nullptr;                   // schedule_row_kernel beside the wide kernel (BatchDev::early_rows)
  hipEvent_t fork_ev = nullptr, join_ev = nullptr;
  // stage events: 0 start, 3 after req_mask, 4 after prep, 5 after the main schedule kernel, 1 after the
  // defer pass, 2 after the planner
  hipEvent_t ev[8] = {nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr, nullptr};
  std::mutex mu;
  std::string err;
  // snapshot
  DevBuf d_snap;
  kad_snapshot_header snap_hdr{};
  kad::SnapDev sd{};
  // batch
  DevBuf d_batch;
  kad_batch_header batch_hdr{};
  kad::BatchDev bd{};
  std::vector<int32_t> plan_rows;
  DevBuf d_plan_rows;  // i32: plan_rows
  DevBuf d_plan_hdr;   // PlanRowHdr per planner row (plan_hdr_kernel at upload)
  DevBuf d_plan_big;   // i32[rows + 1]: plan_pair_kernel's list of rows for the 64-lane planner + its length
  // outputs
  int32_t *d_status = nullptr, *d_count = nullptr, *d_cluster = nullptr;
  uint32_t* d_flags = nullptr;
  int64_t* d_replicas = nullptr;
  size_t out_w_cap = 0, out_slot_cap = 0;
  DevBuf d_req_mask;  // u64
  std::vector<int32_t> h_reqseg;  // BatchDev::req_perm [NR][8] then req_seg [n_seg][4] (host copy until the next upload)
  DevBuf d_reqseg;
  int n_seg_reqs = 0;  // requirements on req_mask_kernel's segment path (the rest: value rows)
  DevBuf d_vrows;      // SnapDev::vrows
  DevBuf d_rescols;    // SnapDev::res4 / res_iv
  DevBuf d_rowslab;    // BatchDev::row_slabs
  DevBuf d_rec;        // UnitRec[W] (prep_kernel)
  DevBuf d_sw;         // u64[W][nch] static filter words (prep_kernel)
  DevBuf d_cw;         // u64[W][nch] current-cluster words (prep_kernel)
  DevBuf d_defer;      // i32[2W + 4]: defer_n, work_n, rows_n, rows_head, the defer list, the row list
  DevBuf d_wq;         // u32[WQ_HEADS * WQ_STRIDE]: schedule kernels' work heads
  // scratch (per-wave slabs for rows that do not fit LDS)
  DevBuf d_scratch;
  bool have_snapshot = false, have_batch = false, ran = false;
  // the resident batch's units this ctx schedules: all of them, or a kad_group member's contiguous shard
  // [unit_lo, unit_lo + unit_n) whose output slots are [slot_lo, slot_lo + slot_n) of the batch's
  int64_t unit_lo = 0, unit_n = 0, slot_lo = 0, slot_n = 0;
  int inject_fault = 0;  // kad_debug_inject_fault: 1 = the next refresh_derived fails (tests)
  int plan_force_ws = 0;  // kad_debug_plan_force_workspace: kad_plan_rows through the workspace planner (tests)
  // the consumers of the results, one Stage each (StageId): a call's inputs and outputs in its buffer, its
  // last route and forced route beside them
  Stage stage[STG_COUNT];
  MonTable mon;
  // override policies (kad_override_*): the resident policy-set blob, its requirement routing (the layout of
  // h_reqseg) and its rows (requirement rows [NR][nch], then M and E [R][nch] each)
  DevBuf d_ovr;
  kad_override_header ovr_hdr{};
  bool have_ovr = false;
  std::vector<int32_t> h_ovr_pro;  // POL_RULE_OFF (host copy: rule counts per object are checked per call)
  std::vector<int32_t> h_ovr_reqseg;
  DevBuf d_ovr_reqseg;
  int ovr_n_seg = 0, ovr_n_rowreq = 0, ovr_n_seg_reqs = 0;
  DevBuf d_ovr_rows;
  int32_t cur_lo = 0, cur_n = 0;  // the resident batch's (shard's) range of KAD_B_CUR_ID entries
  std::vector<uint8_t> di_host;    // kad_dispatch_plan: the entries as they come back, before each object's count is known
  bool group_member = false;   // owned by a kad_group: its resident results are a shard's
  // HIP event records around the stages (kad_set_timing); timed = the last
  // kad_schedule recorded them
  bool timing = false, timed = false;
  bool snap_negative = false;  // some allocatable / used cpu or memory < 0 or >= 2^46 (odd score ranges)
  int clean_kind = 0;          // res_clean of the resident snapshot: 2 strict, 1 relaxed, 0 generic
  std::vector<int64_t> h_res;  // host shadow of alloc/used cpu/mem [4][C] (snap_negative after deltas)
  std::vector<uint64_t> h_ns;  // host shadow of the NoSchedule|NoExecute taint words [TW][C] (SnapDev::present_taints)
  DevBuf d_slices;             // SnapDev::slices [128*TW + 64*GW][nch], then SnapDev::taint_tab [2][8*TW][256][nch]
  std::vector<int64_t> h_fit;  // SnapDev::fit_vals / fit_rows (host copy the upload reads from)
  DevBuf d_fit;
  DevBuf d_delta;              // kad_snapshot_update: resident delta blob
  bool batch_defer = false;    // some unit uses a feature the lean kernel defers
  bool batch_zero_req = false;  // no unit has a ResourceRequest (BatchDev::zero_req)
  bool batch_many_terms = false;  // some unit has more than ROW_MAX_TERMS preferred terms (the row path defers it)
  kad::Route route{};          // what the last kad_schedule launched (kad_last_route)
  // scheduling-trigger hashes (kad_trigger_*)
  DevBuf t_suffix;
  int64_t t_suffix_len = -1;   // -1: no suffix uploaded
  DevBuf t_prefix;
  DevBuf t_tabs;               // segment / composed tables + powers of the suffix
  int t_n = -1;                // -1: no prefixes uploaded
  kad::TriggerDev td{};
};

inline int fail(kad_ctx* c, int code, const std::string& msg) {
  if (c) c->err = msg;
  return code;
}
#define HIPCHK(ctx, x)                                                                             \
  do {                                                                                             \
    hipError_t e_ = (x);                                                                           \
    if (e_ != hipSuccess) return fail(ctx, KAD_EHIP, std::string(#x ": ") + hipGetErrorString(e_)); \
  } while (0)

// Nothing unwinds through the C ABI: a host-side exception (std::bad_alloc from a check's or a planner
// row's vectors, rethrown by the worker pool once all its workers are done) becomes an error code.
template <class F>
inline int guarded(kad_ctx* c, F f) {
  try {
    return f();
  } catch (const std::bad_alloc&) {
    return fail(c, KAD_ENOMEM, "host allocation failed");
  } catch (const std::exception& e) {  // e.g. std::system_error from a pool thread's creation
    return fail(c, KAD_EHOST, std::string("host error: ") + e.what());
  } catch (...) {
    return fail(c, KAD_EHOST, "host error: unknown exception");
  }
}

// Every ctx-taking entry point: guarded, KAD_EINVAL without a ctx or with bad arguments (args_ok must not
// read through c), then f() under the ctx's lock.
template <class F>
inline int entry(kad_ctx* c, bool args_ok, F f) {
  return guarded(c, [&]() -> int {
    if (!c || !args_ok) return KAD_EINVAL;
    std::lock_guard<std::mutex> g(c->mu);
    return f();
  });
}

template <class T>
inline const T* at(const void* base, const uint64_t* off, int i) {
  return reinterpret_cast<const T*>(static_cast<const char*>(base) + off[i]);
}

inline int grow(kad_ctx* c, DevBuf& b, size_t need) {
  if (need <= b.cap && b.p) return 0;
  b.release();
  if (need == 0) need = 256;
  hipError_t e = hipMalloc(&b.p, need);
  if (e != hipSuccess) return fail(c, KAD_ENOMEM, std::string("hipMalloc: ") + hipGetErrorString(e));
  b.cap = need;
  return 0;
}

// ---- the ABI glue of a consumer call: kad_*_timing, kad_*_route_eval, kad_*_last_route, kad_*_debug_route and
// kad_*_check are one line each over these
// ms[i] = the time between a stage's events i and i + 1, for its n intervals; KAD_ESTATE (none_ran) before
// its first run
inline int stage_timing(kad_ctx* c, StageId id, int n, float* ms, const char* none_ran) {
  return entry(c, ms != nullptr, [&]() -> int {
    const Stage& s = c->stage[id];
    if (!s.ran) return fail(c, KAD_ESTATE, none_ran);
    HIPCHK(c, hipEventSynchronize(s.ev[n]));
    for (int i = 0; i < n; i++) HIPCHK(c, hipEventElapsedTime(&ms[i], s.ev[i], s.ev[i + 1]));
    return KAD_OK;
  });
}
// a route struct as the FIELDS int32_t of its record in include/kad_sched.h
template <int FIELDS, class R>
inline int route_record(int32_t* out, const R& r) {
  static_assert(sizeof(R) == 4 * FIELDS && FIELDS <= 8, "a route record: the struct's int32_t fields, 8 at most");
  memcpy(out, &r, sizeof r);
  return KAD_OK;
}
// the stage's events hold a run that launched r
template <class R>
inline void stage_ran(Stage& s, const R& r) {
  s.ran = true;
  s.route_n = (int)(sizeof(R) / 4);
  route_record<sizeof(R) / 4>(s.route, r);
}
inline int stage_last_route(kad_ctx* c, StageId id, int32_t* out, const char* none_ran) {
  return entry(c, out != nullptr, [&]() -> int {
    const Stage& s = c->stage[id];
    if (!s.ran) return fail(c, KAD_ESTATE, none_ran);
    memcpy(out, s.route, 4 * (size_t)s.route_n);
    return KAD_OK;
  });
}
inline int stage_debug_route(kad_ctx* c, StageId id, bool args_ok, const kad::GroupForce& f) {
  return entry(c, args_ok && f.long_min >= 0, [&]() -> int {
    c->stage[id].force = f;
    return KAD_OK;
  });
}
// a host-only kad_*_check: nothing unwinds through the C ABI, and there is no ctx to keep a message
template <class F>
inline int check_guarded(F f) {
  try {
    return f();
  } catch (...) {
    return KAD_EHOST;
  }
}

inline kad::OutDev out_dev(kad_ctx* c) {
  kad::OutDev o{};
  o.status = c->d_status;
  o.count = c->d_count;
  o.flags = c->d_flags;
  // the kernels write slot out_off[w] (batch-wide): a shard's buffer holds slots [slot_lo, slot_lo + slot_n)
  o.cluster = reinterpret_cast<int32_t*>(reinterpret_cast<uintptr_t>(c->d_cluster) - 4 * (uintptr_t)c->slot_lo);
  o.replicas = reinterpret_cast<int64_t*>(reinterpret_cast<uintptr_t>(c->d_replicas) - 8 * (uintptr_t)c->slot_lo);
  return o;
}

// kad_api.hip
int validate_profile(kad_ctx* c, const kad_profile* p);
struct ReqRouting {
  int n_seg = 0, n_rowreq = 0, n_seg_reqs = 0;
};
ReqRouting route_requirements(int NR, const int32_t* ro, const int32_t* rq, int K, size_t nch, bool vr,
                              std::vector<int32_t>& out);
#endif  // KAD_HOST_ONLY
