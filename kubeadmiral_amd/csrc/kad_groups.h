// The lane-group launch rule the consumer calls share (kad_migrate / kad_cstat / kad_statusagg / kad_rollout):
// a wave is 64 / width lane groups, every group takes one row (a segment, a cluster, an object) at a time and
// the groups of a grid stride over the rows. Each call's route_* (its own header) stays the place where its
// decision is taken; the arithmetic is here, once. Plain C++: no HIP header is needed.
#pragma once

#include <cstdint>
#include <type_traits>

namespace kad {

// lanes per row: the mean items per row (rounded up), per_lane of them to a lane (rounded up), rounded up to a
// power of two in [min_width, 64]
inline int group_width(int64_t items, int64_t rows, int min_width, int per_lane) {
  const int64_t mean = rows > 0 ? (items + rows - 1) / rows : 0;
  const int64_t want = (mean + per_lane - 1) / per_lane;
  int w = min_width;
  while (w < 64 && w < want) w <<= 1;
  return w;
}

// blocks of 256 threads for `rows` rows, 256 / width of them a block: 8 blocks (32 waves) a CU at most, each
// lane group striding
inline int32_t group_grid(int64_t rows, int width, int n_cu) {
  const int64_t per_block = 256 / width, want = (rows + per_block - 1) / per_block, cap = (int64_t)n_cu * 8;
  return (int32_t)(want < cap ? want : cap);
}

// rows between two consecutive rows of one lane group
inline int32_t group_stride(int32_t grid, int width) { return (int32_t)((int64_t)grid * (256 / width)); }

// 0 (the route's own) or a power of two in [min_width, 64]
inline bool group_width_ok(int w, int min_width) { return w == 0 || (w >= min_width && w <= 64 && (w & (w - 1)) == 0); }

// What a call's kad_*_debug_route forces on its following runs (0: the route's own). Measurement only.
struct GroupForce {
  int32_t width = 0, long_min = 0, serial = 0;  // serial: kad_rollout_plan alone
  int32_t path = 0;                             // kad_policyrc_count, kad_monitor_report: 1 LDS-private, 2 global
  int32_t grid = 0;                             // kad_monitor_report alone: the scan kernel's blocks
  int long_min_or(int own) const { return long_min > 0 ? long_min : own; }
};

// A forced width replaces the route's own on a group path over `rows` rows, with the grid (and the stride, where
// the route records one) that follow from it. on_path: the path has rows to take (a call whose rows are all long
// leaves its group path empty; kad_migrate_estimate applies the width all the same and passes true).
inline void group_force_apply(const GroupForce& f, bool on_path, int64_t rows, int n_cu, int32_t& width, int32_t& grid,
                              int32_t* stride = nullptr) {
  if (f.width <= 0 || !on_path) return;
  width = f.width;
  grid = group_grid(rows, width, n_cu);
  if (stride) *stride = group_stride(grid, width);
}

// f(std::integral_constant<int, W>{}) for the power of two w in [MIN, 64] (anything else: 64), so that a launch
// names its kernel template once. MIN is 1 or 8; the cases ascend, as the kernels are instantiated.
template <int MIN, class F>
inline void with_width(int w, F f) {
  static_assert(MIN == 1 || MIN == 8, "lane-group widths start at 1 or at 8");
  if constexpr (MIN == 1) {
    switch (w) {
      case 1: return f(std::integral_constant<int, 1>{});
      case 2: return f(std::integral_constant<int, 2>{});
      case 4: return f(std::integral_constant<int, 4>{});
      default: break;
    }
  }
  switch (w) {
    case 8: return f(std::integral_constant<int, 8>{});
    case 16: return f(std::integral_constant<int, 16>{});
    case 32: return f(std::integral_constant<int, 32>{});
    default: return f(std::integral_constant<int, 64>{});
  }
}

}  // namespace kad
