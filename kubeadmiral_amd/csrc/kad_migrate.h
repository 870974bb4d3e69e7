// kad_migrate_estimate (kad_migrate.hip): one batch of objects, (object, cluster) segments and pod records,
// the launch decision, the launches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kad_groups.h"

namespace kad {

constexpr int MIG_MAX_IDS = 131072;    // the id space of kad_follower_union
constexpr int MIG_LONG_MIN = 1024;     // segments with more pods than this take the long path (a starting value,
                                       // see DESIGN §7 for the measured comparison)
constexpr int MIG_MIN_WIDTH = 8;       // lane-group widths: powers of two in [8, 64]
constexpr uint8_t MIG_SEG_SKIP = 1, MIG_SEG_BACKOFF = 2;                  // KAD_MIG_SEG_*
constexpr uint8_t MIG_POD_DELETING = 1, MIG_POD_UNSCHED = 2, MIG_POD_TZERO = 4;  // KAD_MIG_POD_*

struct MigrateDev {
  int O, S;
  int64_t now;
  int width, obj_width;          // lanes per segment (group path) / per object
  int long_min, n_long;
  const int32_t* obj_seg_off;    // [O + 1]
  const int64_t* obj_thr;        // [O]
  const int32_t* seg_obj;        // [S] the object of each segment (built on the host while it validates)
  const int32_t* seg_cluster;    // [S]
  const int64_t* seg_desired;    // [S]
  const uint8_t* seg_flags;      // [S]
  const int64_t* seg_pod_off;    // [S + 1]
  const int64_t* pod_t;          // [P]
  const uint8_t* pod_flags;      // [P]
  const int32_t* long_list;      // [n_long] the segments of the long path, ascending
  const int32_t* old_off;        // [O + 1]
  const int32_t* old_cluster;    // [old_off[O]]
  const int64_t* old_cap;        // [old_off[O]]
  int32_t* uns;                  // [S]
  int64_t* next_cross;           // [S]
  int64_t* cap;                  // [S]
  uint8_t* changed;              // [O]
  int32_t* n_written;            // [O]
  int64_t* retry_after;          // [O]
  uint8_t* backoff;              // [O]
};

// The launch decision of one kad_migrate_estimate, taken here and nowhere else (kad_migrate_route_eval /
// kad_migrate_last_route show it). Group path: a wave is 64 / width lane groups and every group reduces one
// segment at a time, the groups of a grid striding over the segments; width is the batch's mean segment
// length rounded up to a power of two in [8, 64], so that a group covers a typical segment in one step and
// short segments share a wave. Segments with more than long_min pods (the caller counts them: n_long) are
// left out there and go one per 256-thread block. The object kernel does the same per object with the mean
// number of segments per object.
struct MigrateRoute {
  int32_t width;       // lanes per segment on the group path
  int32_t long_min;    // a segment with more pods than this is on the long path
  int32_t threads;     // per block, every kernel
  int32_t grid;        // blocks of the group path (0 at S = 0)
  int32_t long_grid;   // blocks of the long path = n_long
  int32_t stride;      // segments between two consecutive segments of one lane group
  int32_t obj_width;   // lanes per object
  int32_t obj_grid;    // blocks of the object kernel
};

inline MigrateRoute route_migrate(int S, int64_t P, int n_long, int O, int n_cu) {
  MigrateRoute r{};
  r.width = group_width(P, S, MIG_MIN_WIDTH, 1);
  r.long_min = MIG_LONG_MIN;
  r.threads = 256;
  // no LDS on the group path
  r.grid = group_grid(S, r.width, n_cu);
  r.long_grid = n_long;
  r.stride = group_stride(r.grid, r.width);
  r.obj_width = group_width(S, O, MIG_MIN_WIDTH, 1);
  r.obj_grid = group_grid(O, r.obj_width, n_cu);
  return r;
}

}  // namespace kad
