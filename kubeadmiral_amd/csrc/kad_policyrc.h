// kad_policyrc_count (kad_policyrc.hip): the policy reference counter's two maps as one dense table, a batch of
// references removed and added as two id lists; the device arrays, the launch decision, the launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kad {

// The largest P whose two histograms a block keeps in LDS: 2 * P int32 bins, 64 KiB at the limit, so that two
// blocks stay resident on a CU's 160 KiB (DESIGN.md §7 "policy reference counts" holds the measurement behind it).
constexpr int PRC_LDS_BINS = 8192;
constexpr int PRC_THREADS = 256;
constexpr int PRC_VEC = 4;  // ids a lane reads per step: 16 B
constexpr int PRC_PATH_LDS = 0, PRC_PATH_GLOBAL = 1;
constexpr uint8_t PRC_POL_EXISTS = 1, PRC_POL_ENQUEUED = 2;          // KAD_PRC_POL_*
constexpr uint8_t PRC_FLAGGED = 1, PRC_UPDATE = 2, PRC_NEGATIVE = 4;  // KAD_PRC_*

struct PolicyrcDev {
  int P, n_dec, n_inc;
  const int32_t *dec_ids, *inc_ids;  // [n_dec], [n_inc], every id in [0, P) (checked on the host)
  const int64_t *count, *stored_typed, *stored_rest, *stored_total;  // [P]
  const uint8_t* pol_flags;          // [P]
  int32_t* hist;                     // [2 * P]: removals per policy, then additions; zeroed before the count kernel
  int64_t *new_count, *new_total;    // [P]
  uint8_t* state;                    // [P]
  int32_t* n_negative;               // [1], zeroed before the apply kernel
};

// The launch decision of one kad_policyrc_count, taken here and nowhere else (kad_policyrc_route_eval /
// kad_policyrc_last_route show it). The count kernel's blocks stride over each list, PRC_THREADS * PRC_VEC ids to a
// block and step: one block per step of the n_ids = n_dec + n_inc ids, capped by what stays resident: on the
// LDS-private path the 160 KiB of a CU over a block's 2 * P bins (8 blocks at most), on the global path 8 blocks
// (32 waves) a CU.
struct PolicyrcRoute {
  int32_t path;        // PRC_PATH_*
  int32_t bins;        // PRC_LDS_BINS
  int32_t threads;     // per block
  int32_t grid;        // count-kernel blocks (0 without ids)
  int32_t vec;         // ids per lane per step
  int32_t apply_grid;  // apply-kernel blocks
};

// force_path: 0 the route's own, 1 LDS-private (the caller rejects it above the bins limit), 2 global
inline PolicyrcRoute route_policyrc(int P, int64_t n_ids, int n_cu, int force_path = 0) {
  PolicyrcRoute r{};
  r.path = force_path == 1 ? PRC_PATH_LDS : force_path == 2 ? PRC_PATH_GLOBAL : P <= PRC_LDS_BINS ? PRC_PATH_LDS : PRC_PATH_GLOBAL;
  r.bins = PRC_LDS_BINS;
  r.threads = PRC_THREADS;
  r.vec = PRC_VEC;
  const int64_t lds = r.path == PRC_PATH_LDS ? 2 * (int64_t)P * 4 : 0;
  const int64_t by_lds = lds > 0 ? (160 * 1024) / lds : 8, per_cu = by_lds < 1 ? 1 : by_lds < 8 ? by_lds : 8;
  const int64_t per_step = (int64_t)PRC_THREADS * PRC_VEC, want = (n_ids + per_step - 1) / per_step, cap = (int64_t)n_cu * per_cu;
  r.grid = (int32_t)(want < cap ? want : cap);
  r.apply_grid = (int32_t)(((int64_t)P + PRC_THREADS - 1) / PRC_THREADS);
  return r;
}

hipError_t launch_policyrc_count(const PolicyrcDev& d, const PolicyrcRoute& r, hipStream_t st);
hipError_t launch_policyrc_apply(const PolicyrcDev& d, const PolicyrcRoute& r, hipStream_t st);

}  // namespace kad
