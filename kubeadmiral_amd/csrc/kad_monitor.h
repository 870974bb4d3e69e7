// kad_monitor_* (kad_monitor.hip): the monitor controller's per-object meters as a device-resident table, a batch of
// object events against it, and the report's one pass over it; the device arrays, the launch decisions, the launches.
//
// Time on the device (declared here, checked against an exact model of Go's time by tests/monitor_ref.py): int64
// nanoseconds since the Unix epoch for a real time, which lies in [0, 2^62); Go's zero time.Time (year 1, which no
// int64 of Unix nanoseconds holds) is the sentinel MON_ZERO = -2^62, and a time the reference derives from it by
// Add (zero - 10 ms, zero + ReportInterval) is MON_ZERO plus that duration: every such value lies below -2^61 and
// compares as Go's does (before zero, zero, after zero, all before any real time). After is >, IsZero is == MON_ZERO,
// Add is +, and Sub saturates at MinInt64 / MaxInt64 whenever exactly one operand lies below -2^61 (Go: the operands
// are more than 292 years apart), else it is the plain difference.
//
// The reference ranges over a sync.Map, whose order is unspecified; the report's two timer lists come out in ascending
// slot order instead, so that the output is deterministic.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kad_groups.h"

namespace kad {

constexpr int64_t MON_ZERO = -(1ll << 62);   // KAD_MON_TIME_ZERO
constexpr int64_t MON_NEAR = -(1ll << 61);   // below: the zero time, or derived from it
constexpr int64_t MON_TIME_END = 1ll << 62;  // real times end here
constexpr int64_t MON_MS = 1000000ll, MON_SECOND = 1000000000ll, MON_MINUTE = 60 * MON_SECOND;
constexpr int64_t MON_REPORT_INTERVAL = MON_MINUTE;  // monitor_controller.go:47
constexpr int MON_MAX_CLUSTERS = 16384;              // KAD_DISPATCH_MAX_CLUSTERS
constexpr int MON_THREADS = 256;
constexpr int MON_COLS = 5;  // creation, last_update, sync_success, last_status_synced, out_of_sync_ns
enum { MON_CR, MON_LU, MON_SS, MON_LST, MON_OOS };
constexpr uint8_t MON_LIVE = 1;  // KAD_MON_LIVE

// ---- kad_monitor_reconcile
// Objects whose longest list has more entries than this take a whole block (kad_sync_finish's value); a lane of a
// group compares this many entries of a mean object (a compare is two loads and no search: kad_statusagg's 8).
constexpr int MON_LONG_MIN = 512;
constexpr int MON_PER_LANE = 8;
constexpr uint16_t MON_DELETED = 1, MON_NEW = 2, MON_SS_PARSED = 4, MON_LASTGEN_PRESENT = 8, MON_LASTGEN_EQUAL = 16,
                   MON_LSSG_PRESENT = 32, MON_LSSG_EQUAL = 64, MON_STATUS_ENABLED = 128, MON_STATUS_ABSENT = 256,
                   MON_FED_MISSING = 512, MON_CLUSTER_ERR = 1024, MON_HAS_LAST = 2048, MON_OBJ_ALL = 4095;  // KAD_MON_OBJ_*
constexpr uint8_t MON_ALL_OK = 0, MON_STATUS_ERROR = 1, MON_REQUEUE = 2;  // KAD_MON_RESULT_*
constexpr uint8_t MON_METER_DELETED = 1, MON_UPDATE_ANNOTATION = 2, MON_STATUS_STORED = 4, MON_REPLACE_LAST = 8,
                  MON_MISSING_OG = 16, MON_LOG_LAST_CLUSTER = 32;  // KAD_MON_BIT_*

struct MonList {
  const int32_t *off, *cluster;
  const int64_t* gen;
};

struct MonTableDev {
  int64_t* col[MON_COLS];
  int32_t* type_id;
  uint8_t* flags;
};

struct MonRecDev {
  int O, n_long;
  int64_t now;
  const int32_t* slot;
  const uint16_t* obj_flags;
  const int32_t* type_id;
  const int64_t *creation, *sync_success;
  MonList fed, mem, last;
  const uint8_t* obj_long;   // [O] 1: the object is on the long path (built on the host while it validates)
  const int32_t* long_list;  // [n_long] ascending
  MonTableDev t;
  uint8_t *result, *bits;
  int64_t *meter, *would;  // [O][5], [O][2]
};

// The launch decision of one kad_monitor_reconcile (kad_sync_finish's shape): a wave is 64 / width lane groups, every
// group takes one object at a time and its lanes stride over the object's lists; the width is the mean size of a
// short object (its longest list) over MON_PER_LANE, rounded up to a power of two in [1, 64]. Objects larger than
// long_min go one per block.
struct MonRecRoute {
  int32_t width, long_min, threads, grid, long_grid, stride;
};
inline MonRecRoute route_monitor_reconcile(int O, int n_long, int64_t short_items, int n_cu) {
  MonRecRoute r{};
  const int n_short = O - n_long;
  r.width = group_width(short_items, n_short, 1, MON_PER_LANE);
  r.long_min = MON_LONG_MIN;
  r.threads = MON_THREADS;
  r.grid = n_short > 0 ? group_grid(O, r.width, n_cu) : 0;
  r.long_grid = n_long;
  r.stride = group_stride(r.grid, r.width);
  return r;
}

// ---- kad_monitor_report
constexpr int MON_VEC = 4;                                // consecutive slots a lane takes per step
constexpr int MON_WTILE = 64 * MON_VEC;                   // slots of a wave's step: the unit of the timer lists' counts
constexpr int MON_BTILE = MON_THREADS * MON_VEC;          // slots of a block's step; the table is allocated in these
constexpr int MON_COUNTERS = 14;                          // sync buckets [6], status buckets [6], the two throughputs
constexpr int MON_BUCKETS = 6;
constexpr int MON_SLOT_BYTES = MON_COLS * 8 + 4 + 1;      // what the report reads of a slot: 45 B
// The largest n_types whose two histograms a block keeps in LDS: 2 * n_types int32 bins, 32 KiB at the limit, so that
// four blocks (16 waves) stay resident on a CU's 160 KiB (DESIGN.md §7 "monitor" holds the reasoning and the
// measurement).
constexpr int MON_LDS_TYPES = 4096;
constexpr int MON_PATH_LDS = 0, MON_PATH_GLOBAL = 1;

struct MonRepDev {
  int64_t n_slots, now;
  int n_types, n_wtiles, timer_cap;
  MonTableDev t;
  int32_t* counters;  // [MON_COUNTERS], zeroed before the scan kernel
  int32_t* hist;      // [2 * n_types]: five-minute sync count per type, then status; zeroed before
  int32_t* tile_cnt;  // [n_wtiles] timers of a wave tile: sync | status << 16
  int32_t* tile_off;  // [2][n_wtiles + 1] their exclusive sums
  int32_t *sync_slot, *status_slot;
  int64_t *sync_ms, *status_ms;
  int32_t* n_timers;  // [2]
};

// The launch decision of one kad_monitor_report, taken here and nowhere else. The scan kernel's blocks stride over
// the table MON_BTILE slots at a time: one block per step, capped by what stays resident: on the LDS-private path the
// 160 KiB of a CU over a block's 2 * n_types bins (8 blocks at most), on the global path 8 blocks (32 waves) a CU.
struct MonRepRoute {
  int32_t path;     // MON_PATH_*
  int32_t bins;     // MON_LDS_TYPES
  int32_t threads;  // per block
  int32_t grid;     // blocks of the scan and of the scatter kernel (0 without slots)
  int32_t vec;      // slots per lane per step
  int32_t wtiles;   // wave tiles: the entries of the timer lists' count
};
// force_path: 0 the route's own, 1 LDS-private (the caller rejects it above the bins limit), 2 global; force_grid: 0
// the route's own, else the blocks (at most one per step)
inline MonRepRoute route_monitor_report(int64_t n_slots, int n_types, int n_cu, int force_path = 0, int force_grid = 0) {
  MonRepRoute r{};
  r.path = force_path == 1 ? MON_PATH_LDS : force_path == 2 ? MON_PATH_GLOBAL : n_types <= MON_LDS_TYPES ? MON_PATH_LDS : MON_PATH_GLOBAL;
  r.bins = MON_LDS_TYPES;
  r.threads = MON_THREADS;
  r.vec = MON_VEC;
  const int64_t lds = r.path == MON_PATH_LDS ? 2 * (int64_t)n_types * 4 : 0;
  const int64_t by_lds = lds > 0 ? (160 * 1024) / (lds + 256) : 8, per_cu = by_lds < 1 ? 1 : by_lds < 8 ? by_lds : 8;
  const int64_t want = (n_slots + MON_BTILE - 1) / MON_BTILE, cap = (int64_t)n_cu * per_cu;
  int64_t g = want < cap ? want : cap;
  if (force_grid > 0) g = force_grid < want ? force_grid : want;
  r.grid = (int32_t)g;
  r.wtiles = (int32_t)((n_slots + MON_WTILE - 1) / MON_WTILE);
  return r;
}

// ---- the table's gather / scatter (kad_monitor_load / kad_monitor_read)
struct MonIoDev {
  int n;
  const int32_t* slots;
  int64_t* col[MON_COLS];  // staged values [n]
  int32_t* type_id;
  uint8_t* flags;
  MonTableDev t;
};

hipError_t launch_monitor_reconcile(const MonRecDev& d, const MonRecRoute& r, hipStream_t st);
hipError_t launch_monitor_report(const MonRepDev& d, const MonRepRoute& r, hipStream_t st);
hipError_t launch_monitor_timers(const MonRepDev& d, const MonRepRoute& r, hipStream_t st);
hipError_t launch_monitor_io(const MonIoDev& d, bool load, hipStream_t st);

}  // namespace kad
