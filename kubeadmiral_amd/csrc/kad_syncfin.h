// kad_sync_needs_update / kad_sync_finish (kad_syncfin.hip): the version check of a batch of updates and the close
// of a batch of reconciles; the device arrays, the launch decisions, the launches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kad_groups.h"

namespace kad {

constexpr int SF_MAX_CLUSTERS = 16384;  // KAD_DISPATCH_MAX_CLUSTERS
constexpr int SF_THREADS = 256;
// Objects whose longest list has more entries than this take a whole block (kad_statusagg's value, which the
// measured rows do not contradict), and a lane of a group takes this many elements of a mean object (measured: every
// element costs binary searches, so fewer per lane than kad_statusagg's 8): DESIGN §7.2 has the table.
constexpr int SF_LONG_MIN = 512;
constexpr int SF_PER_LANE = 2;
constexpr uint8_t SF_ST_OK = 1, SF_ST_WAITING = 2, SF_ST_CREATION_TO = 20, SF_ST_UPDATE_TO = 21, SF_ST_DELETION_TO = 22,
                  SF_ST_LABEL_TO = 23, SF_ST_MAX = 23;                                                  // KAD_SYNC_ST_*
constexpr uint8_t SF_VER_HAS_GEN = 1, SF_VER_IS_GEN = 2;                                                // KAD_SYNC_VER_*
constexpr uint8_t SF_ROW_REPLICAS = 1, SF_ROW_SURGE = 2, SF_ROW_UNAVAILABLE = 4, SF_ROW_META = 8;       // KAD_SYNC_ROW_*
constexpr uint16_t SF_OBJ_EXISTS = 1, SF_OBJ_CURRENT = 2, SF_OBJ_OLDV_NIL = 4, SF_OBJ_OLDV_IRREGULAR = 8, SF_OBJ_UPDATED = 16,
                   SF_OBJ_SCALARS = 32, SF_OBJ_COND_EXISTS = 64, SF_OBJ_COND_TRUE = 128, SF_OBJ_ON_HOST = 256;  // KAD_SYNC_OBJ_*
constexpr uint8_t SF_OUT_CLUSTERS = 1, SF_OUT_PROPAGATED = 2, SF_OUT_TRANSITION = 4, SF_OUT_REQUIRED = 8, SF_OUT_WRITE = 16;

// Wait()'s transition of one recorded status (managed.go:137-155); 0: the entry leaves the status map
__host__ __device__ inline uint8_t sf_transition(uint8_t s) {
  if (s == SF_ST_CREATION_TO || s == SF_ST_UPDATE_TO) return SF_ST_OK;
  if (s == SF_ST_DELETION_TO) return SF_ST_WAITING;
  if (s == SF_ST_LABEL_TO) return 0;
  return s;
}

struct SyncRowsDev {
  int n_rows;
  const int32_t *row_obj, *row_cluster, *row_target;
  const uint8_t *row_flags, *obj_flags;
  const int32_t *rec_off, *rec_cluster, *rec_version;
  const uint8_t* ver_flags;
  uint8_t* needs_update;
  int32_t* recorded;
};

struct SyncFinDev {
  int O, n_long, reason_check;
  const uint16_t* obj_flags;
  const int32_t *reason_in, *cond_reason;
  const int32_t *sel_off, *sel_cluster;
  const int32_t *ent_off, *ent_cluster;
  const uint8_t* ent_status;
  const int32_t* ent_version;
  const int32_t *oldv_off, *oldv_cluster, *oldv_version;
  const int32_t *olds_off, *olds_cluster;
  const uint8_t* olds_status;
  const int64_t *olds_gen, *ver_gen;
  const uint8_t* ver_flags;
  const int64_t *ver_off, *st_off;
  // built on the host while it validates
  const uint8_t* obj_long;   // [O] 1: the object is on the long path
  const int32_t* long_list;  // [n_long] ascending
  // scratch: per object the exclusive counts of emitted entries, one more slot than the list has entries (object o's
  // start at off[o] + o)
  int32_t *ent_pre, *oldv_pre;
  int32_t *out_ver_cluster, *out_ver_id, *ver_count;
  uint8_t* ver_write;
  int32_t* out_st_cluster;
  uint8_t* out_st_status;
  int64_t* out_st_gen;
  int32_t* st_count;
  uint8_t* obj_out;
  int32_t* reason_out;
};

// The launch decision of one kad_sync_needs_update: a lane per row, the lanes of a grid striding over the rows.
struct SyncRowsRoute {
  int32_t threads, grid, stride;
};
inline SyncRowsRoute route_sync_rows(int64_t n_rows, int n_cu) {
  SyncRowsRoute r{};
  r.threads = SF_THREADS;
  r.grid = group_grid(n_rows, 1, n_cu);
  r.stride = group_stride(r.grid, 1);
  return r;
}

// The launch decision of one kad_sync_finish, taken here and nowhere else (kad_sync_finish_route_eval /
// _last_route show it). Group path: a wave is 64 / width lane groups, every group takes one object at a time and its
// lanes stride over the object's lists; the width is the mean size of a short object (its longest list of ent, oldv,
// olds) over SF_PER_LANE, rounded up to a power of two in [1, 64]. Objects larger than long_min go one per block.
struct SyncFinRoute {
  int32_t width, long_min, threads, grid, long_grid, stride;
};
inline SyncFinRoute route_sync_finish(int O, int n_long, int64_t short_items, int n_cu) {
  SyncFinRoute r{};
  const int n_short = O - n_long;
  r.width = group_width(short_items, n_short, 1, SF_PER_LANE);
  r.long_min = SF_LONG_MIN;
  r.threads = SF_THREADS;
  r.grid = n_short > 0 ? group_grid(O, r.width, n_cu) : 0;
  r.long_grid = n_long;
  r.stride = group_stride(r.grid, r.width);
  return r;
}

hipError_t launch_sync_rows(const SyncRowsDev& d, const SyncRowsRoute& r, hipStream_t st);
hipError_t launch_sync_finish(const SyncFinDev& d, const SyncFinRoute& r, hipStream_t st);

}  // namespace kad
