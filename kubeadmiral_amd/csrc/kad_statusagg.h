// kad_status_aggregate (kad_statusagg.hip): one batch of source objects and their (object, member cluster)
// segments, the launch decision, the launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kad_groups.h"

namespace kad {

constexpr int SAGG_DEPLOYMENT = 0, SAGG_JOB = 1;  // KAD_SAGG_DEPLOYMENT / KAD_SAGG_JOB
constexpr int SAGG_NV_DEP = 5, SAGG_NV_JOB = 3;   // summed int32 rows of a segment
constexpr int SAGG_NOLD_DEP = 6, SAGG_NOLD_JOB = 5;  // int64 rows of an object's old status
constexpr int SAGG_LONG_MIN = 512;  // objects with more segments than this take the long path (a starting value,
                                    // see DESIGN §7 for the measured comparison)
constexpr uint8_t SAGG_OBJ_UPTODATE = 1, SAGG_OBJ_ERROR = 2, SAGG_OBJ_OLD_OTHER = 4;                      // KAD_SAGG_OBJ_*
constexpr uint8_t SAGG_SEG_NIL = 1, SAGG_SEG_SYNCED = 2, SAGG_SEG_START = 4, SAGG_SEG_DONE = 8, SAGG_SEG_FAILED = 16;  // KAD_SAGG_SEG_*

struct SaggDev {
  int O, S;
  int n_long;
  const int32_t* obj_seg_off;   // [O + 1]
  const uint8_t* obj_flags;     // [O]
  const int64_t* obj_generation;  // [O] Deployment
  const int64_t* obj_observed;  // [O] Deployment
  const int64_t* old_vals;      // [NOLD][O]
  const int32_t* seg_vals;      // [NV][S]
  const uint8_t* seg_flags;     // [S]
  const int64_t* seg_a;         // [S] Deployment: status.observedGeneration; Job: startTime
  const int64_t* seg_b;         // [S] Deployment: the synced generation; Job: completionTime
  // built on the host while it validates
  const uint8_t* obj_long;      // [O] 1: the object is on the long path
  const int32_t* long_list;     // [n_long] the objects of the long path, ascending
  int32_t* sums;                // [NV][O]
  int64_t* observed;            // [O] Deployment
  int64_t* start_min;           // [O] Job
  int64_t* done_max;            // [O] Job
  int32_t* n_done;              // [O] Job
  int32_t* n_failed;            // [O] Job
  uint8_t* finished;            // [O] Job
  uint8_t* changed;             // [O]
};

// The launch decision of one kad_status_aggregate, taken here and nowhere else (kad_sagg_route_eval /
// kad_sagg_last_route show it). Group path: a wave is 64 / width lane groups, every group takes one object at a
// time and its lanes stride over the object's segments; the groups of a grid stride over the objects. The width
// is the mean segments per short object / 8, rounded up to a power of two in [1, 64]: several segments in flight
// per wave (what the auto-migration sweep measured), down to a lane per object. Objects with more than long_min
// segments (the caller counts them: n_long, and the short objects' segments) are left out there and go one per
// 256-thread block.
struct SaggRoute {
  int32_t width;      // lanes per object on the group path
  int32_t long_min;   // an object with more segments than this is on the long path
  int32_t threads;    // per block
  int32_t grid;       // blocks of the group path (0 when every object is long)
  int32_t long_grid;  // blocks of the long path = n_long
  int32_t stride;     // objects between two consecutive objects of one lane group
};

inline SaggRoute route_sagg(int O, int n_long, int64_t short_segments, int n_cu) {
  SaggRoute r{};
  const int n_short = O - n_long;
  r.width = group_width(short_segments, n_short, 1, 8);
  r.long_min = SAGG_LONG_MIN;
  r.threads = 256;
  // the groups stride over all O objects and skip the long ones; no LDS on the group path
  r.grid = n_short > 0 ? group_grid(O, r.width, n_cu) : 0;
  r.long_grid = n_long;
  r.stride = group_stride(r.grid, r.width);
  return r;
}

hipError_t launch_sagg(int kind, const SaggDev& d, const SaggRoute& r, hipStream_t st);

}  // namespace kad
