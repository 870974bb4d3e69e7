// kad_follower_union (kad_follower.hip): one batch of leaders and followers, the launch decision, the launches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kad {

constexpr int FOL_WAVE_MAX_IDS = 8192;     // the wave path's per-wave bitmaps: 256 u32 words each
constexpr int FOL_MAX_IDS = 131072;        // the block path's block-shared bitmaps: 4096 u32 words each
constexpr int FOL_WAVE_WORDS = FOL_WAVE_MAX_IDS / 32;
constexpr int FOL_BLOCK_WORDS = FOL_MAX_IDS / 32;
constexpr int FOL_SCAN_ITEMS = 8;          // followers per thread of the offset scan (2048 per block)

struct FollowerDev {
  int n_ids, nw;                 // id space; u32 bitmap words = ceil(n_ids / 32)
  int F, n_leaders;
  // explicit leaders (resident == 0): leader l holds lead_cluster[lead_off[l] .. lead_off[l + 1])
  const int32_t *lead_off, *lead_cluster;
  // resident leaders (resident == 1): leader l < W is unit l of the last schedule — status OK: count[l]
  // output slots from out_off[l]; sticky: its KAD_B_CUR_ID entries (-1 entries skipped); an error class:
  // sched_cluster[sched_off[l] .. sched_off[l + 1]) (sched_off may be null: nothing); leaders >= W: keep only
  int resident, W;
  const int64_t* out_off;        // [W + 1] (BatchDev::out_off)
  const int32_t* cur_off;        // [W + 1] (BatchDev::cur_off)
  const int32_t *res_status, *res_count, *res_cluster, *cur_id;
  int64_t slot_lo;
  const int32_t *sched_off, *sched_cluster;
  const int32_t *keep_off, *keep_cluster;  // [n_leaders + 1] or null: unioned in for every leader
  // followers
  const int32_t *fol_off, *fol_leader;     // [F + 1], indices into the leaders (-1: skipped)
  const int32_t *fcur_off, *fcur_cluster;  // [F + 1], the follower's current placement
  const uint8_t* fcur_has;                 // [F]
  int emit_all;
  int64_t capacity;              // elements of out_cluster
  uint8_t* changed;              // [F]
  int32_t* count;                // [F]
  int64_t* fout_off;             // [F + 1]
  int32_t* out_cluster;          // [capacity]
  int64_t* scan_sums;            // [ceil(F / (256 * FOL_SCAN_ITEMS))] block sums of the offset scan
};

// The launch decision of one kad_follower_union, taken here and nowhere else (kad_follower_route_eval /
// kad_follower_last_route show it): followers whose id space fits two 1-KiB bitmaps per wave go one per
// wave, four waves a block, the waves striding over the followers; larger id spaces take one 256-thread
// block per follower at a time with block-shared bitmaps.
struct FollowerRoute {
  int32_t path;       // 0 wave, 1 block
  int32_t words;      // u32 words per bitmap
  int32_t threads;    // per block
  int32_t grid;       // blocks of the union and of the emit kernel (0 at F = 0)
  int32_t lds;        // static LDS bytes per block
  int32_t stride;     // followers between two consecutive followers of one wave (wave path) / block
};

inline FollowerRoute route_follower(int n_ids, int F, int n_cu) {
  FollowerRoute r{};
  r.path = n_ids > FOL_WAVE_MAX_IDS ? 1 : 0;
  r.words = (n_ids + 31) / 32;
  r.threads = 256;
  if (r.path == 0) {
    // 8 KiB of LDS a block: 8 blocks (32 waves) a CU
    const int64_t want = ((int64_t)F + 3) / 4, cap = (int64_t)n_cu * 8;
    r.grid = (int32_t)(want < cap ? want : cap);
    r.lds = 4 * 2 * FOL_WAVE_WORDS * 4;
    r.stride = r.grid * 4;
  } else {
    // 32 KiB of LDS a block: 4 blocks a CU
    const int64_t cap = (int64_t)n_cu * 4;
    r.grid = (int32_t)(F < cap ? F : cap);
    r.lds = 2 * FOL_BLOCK_WORDS * 4;
    r.stride = r.grid;
  }
  return r;
}

}  // namespace kad
