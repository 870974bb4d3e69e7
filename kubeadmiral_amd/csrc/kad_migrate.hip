// Auto-migration (kad_migrate_estimate): the estimated capacity of every (object, cluster) pair from its pods.
//
// The auto-migration controller walks, per object with the unschedulable threshold annotation, the pods of
// every member cluster (estimateCapacity, pkg/controllers/automigration/controller.go:292-378), counts those
// that have been unschedulable for longer than the threshold (countUnschedulablePods, util.go:29-64) and
// writes the clusters whose capacity falls short of the desired replicas into the auto-migration annotation,
// if the map differs from the one the object holds (reconcile, controller.go:237-255). On the device that is a
// segmented reduction over the pod records, then a short merge per object:
//
//   migrate_segment_kernel<W>  blocks below n_long: one listed long segment per 256-thread block (strided
//                              loads, DPP reduce per wave, LDS combine); the other blocks: a wave is 64 / W
//                              lane groups, each group reduces one segment at a time (count: i32 sum,
//                              nextCrossIn: i64 min of the positive crossings) and one lane of the group
//                              derives the capacity and stores the three outputs
//   migrate_object_kernel<W>   one lane group per object: retryAfter = min nextCrossIn, backoff = OR of the
//                              segment flags, the number of written entries, and DeepEqual of the written
//                              (cluster, capacity) pairs with the existing annotation's, both ascending
//
// No atomics, no state that kad_schedule reads.
#include "kad_migrate.h"
#include "kad_wave.h"

namespace kad {

// one pod (util.go:34-61): deleting pods and pods whose first PodScheduled condition is not
// False / Unschedulable are skipped; crossing = (lastTransitionTime + threshold) - now, <= 0 counts, > 0
// feeds the minimum. The host bounds |t|, |threshold| and now by 2^61, so the sum cannot overflow; a pod
// whose lastTransitionTime is Go's zero time (MIG_POD_TZERO) always counts (Time.Sub saturates to the
// minimum duration there).
__device__ __forceinline__ void pod_step(uint8_t f, int64_t t, int64_t cut, int& cnt, int64_t& next) {
  if ((f & (MIG_POD_DELETING | MIG_POD_UNSCHED)) != MIG_POD_UNSCHED) return;
  const int64_t crossing = wsub(t, cut);  // cut = now - threshold (t is unchecked under MIG_POD_TZERO)
  if ((f & MIG_POD_TZERO) || crossing <= 0)
    ++cnt;
  else
    next = crossing < next ? crossing : next;
}

// controller.go:345-366 for a segment of n pods, uns of them counted: the capacity, or -1 for no entry
__device__ __forceinline__ int64_t segment_cap(int64_t n, int64_t desired, int uns) {
  int64_t cap = n >= desired ? n - uns : desired - uns;
  if (cap >= desired) return -1;
  // unreachable for consistent inputs (uns <= n, so either branch above is >= 0); kept as the reference has it
  if (cap < 0) cap = 0;
  return cap;
}

__device__ __forceinline__ void store_segment(const MigrateDev& d, int s, int64_t n, int cnt, int64_t next) {
  d.uns[s] = cnt;
  d.next_cross[s] = next;
  d.cap[s] = segment_cap(n, d.seg_desired[s], cnt);
}

// segments the reference leaves before it counts (controller.go:310-330): no entry, nothing to retryAfter
__device__ __forceinline__ void store_skipped(const MigrateDev& d, int s) {
  d.uns[s] = 0;
  d.next_cross[s] = I64_MAX;
  d.cap[s] = -1;
}

// sum / min over the W lanes of a group: xor butterflies below W never leave the group
template <int W>
__device__ __forceinline__ int group_sum_i32(int v) {
#pragma unroll
  for (int m = W / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}
template <int W>
__device__ __forceinline__ int64_t group_min_i64(int64_t v) {
#pragma unroll
  for (int m = W / 2; m >= 1; m >>= 1) {
    const int64_t o = shfl_xor_i64(v, m);
    v = o < v ? o : v;
  }
  return v;
}
// this group's lanes of a wave mask
template <int W>
__device__ __forceinline__ uint64_t group_mask(int lane) {
  if (W == 64) return ~0ull;
  return ((1ull << W) - 1ull) << (lane & ~(W - 1));
}

template <int W>
__global__ __launch_bounds__(256) void migrate_segment_kernel(MigrateDev d) {
  if ((int)blockIdx.x < d.n_long) {
    // ---- long path: one listed segment per block
    __shared__ int s_cnt[4];
    __shared__ int64_t s_next[4];
    const int s = d.long_list[blockIdx.x], t = threadIdx.x;
    const int64_t lo = d.seg_pod_off[s], hi = d.seg_pod_off[s + 1];
    const int64_t cut = d.now - d.obj_thr[d.seg_obj[s]];
    int cnt = 0;
    int64_t next = I64_MAX;
    int64_t k = lo + t;
    for (; k + 768 < hi; k += 1024) {  // four independent loads a lane in flight
      const int64_t t0 = d.pod_t[k], t1 = d.pod_t[k + 256], t2 = d.pod_t[k + 512], t3 = d.pod_t[k + 768];
      const uint8_t f0 = d.pod_flags[k], f1 = d.pod_flags[k + 256], f2 = d.pod_flags[k + 512], f3 = d.pod_flags[k + 768];
      pod_step(f0, t0, cut, cnt, next);
      pod_step(f1, t1, cut, cnt, next);
      pod_step(f2, t2, cut, cnt, next);
      pod_step(f3, t3, cut, cnt, next);
    }
    for (; k < hi; k += 256) pod_step(d.pod_flags[k], d.pod_t[k], cut, cnt, next);
    cnt = wave_sum_i32(cnt);
    next = wave_min_i64(next);
    if ((t & 63) == 0) {
      s_cnt[t >> 6] = cnt;
      s_next[t >> 6] = next;
    }
    __syncthreads();
    if (t == 0) {
      int c = 0;
      int64_t m = I64_MAX;
      for (int q = 0; q < 4; ++q) {
        c += s_cnt[q];
        m = s_next[q] < m ? s_next[q] : m;
      }
      store_segment(d, s, hi - lo, c, m);
    }
    return;
  }
  // ---- group path: the loop is uniform over the wave (groups past S idle), so every shuffle sees its group whole
  constexpr int GPB = 256 / W;  // groups a block
  const int lane = lane_id_h(), gl = lane & (W - 1);
  const int g = (int)threadIdx.x / W;
  const int64_t stride = (int64_t)(gridDim.x - d.n_long) * GPB;
  const int64_t first = (int64_t)(blockIdx.x - d.n_long) * GPB;
  for (int64_t base = first; base < d.S; base += stride) {
    const int64_t s64 = base + g;
    const bool live = s64 < d.S;
    const int s = live ? (int)s64 : 0;
    int cnt = 0;
    int64_t next = I64_MAX, n = 0;
    uint8_t sf = MIG_SEG_SKIP;
    if (live) {
      sf = d.seg_flags[s];
      const int64_t lo = d.seg_pod_off[s], hi = d.seg_pod_off[s + 1];
      n = hi - lo;
      if (!(sf & MIG_SEG_SKIP) && n <= d.long_min) {
        const int64_t cut = d.now - d.obj_thr[d.seg_obj[s]];
        // consecutive lanes read consecutive pods; consecutive groups hold consecutive segments
        for (int64_t k = lo + gl; k < hi; k += W) pod_step(d.pod_flags[k], d.pod_t[k], cut, cnt, next);
      }
    }
    cnt = group_sum_i32<W>(cnt);
    next = group_min_i64<W>(next);
    if (live && gl == 0) {
      if (sf & MIG_SEG_SKIP)
        store_skipped(d, s);
      else if (n <= d.long_min)
        store_segment(d, s, n, cnt, next);
    }
  }
}

template <int W>
__global__ __launch_bounds__(256) void migrate_object_kernel(MigrateDev d) {
  constexpr int GPB = 256 / W;
  const int lane = lane_id_h(), gl = lane & (W - 1);
  const int g = (int)threadIdx.x / W;
  const uint64_t gm = group_mask<W>(lane);
  const uint64_t below = gm & ((1ull << lane) - 1ull);  // this group's lanes below this one
  const int64_t stride = (int64_t)gridDim.x * GPB;
  for (int64_t base = (int64_t)blockIdx.x * GPB; base < d.O; base += stride) {
    const int64_t o64 = base + g;
    const bool live = o64 < d.O;
    const int o = live ? (int)o64 : 0;
    const int s0 = live ? d.obj_seg_off[o] : 0, s1 = live ? d.obj_seg_off[o + 1] : 0;
    const int q0 = live ? d.old_off[o] : 0, n_old = live ? d.old_off[o + 1] - q0 : 0;
    // the widest object of the wave decides the steps, so that the ballots below see every lane
    const int steps = wave_max_u_i32((s1 - s0 + W - 1) / W);
    int64_t retry = I64_MAX;
    int written = 0;  // entries of the groups' earlier steps (uniform over the group)
    bool bo = false, differ = false;
    for (int it = 0; it < steps; ++it) {
      const int s = s0 + it * W + gl;
      bool w = false;
      if (s < s1) {
        const uint8_t sf = d.seg_flags[s];
        bo |= (sf & MIG_SEG_BACKOFF) != 0;
        if (!(sf & MIG_SEG_SKIP)) {  // a skipped segment feeds neither retryAfter nor the map
          const int64_t nx = d.next_cross[s];
          retry = nx < retry ? nx : retry;
          w = d.cap[s] >= 0;
        }
      }
      const uint64_t m = ballot(w);
      if (w) {
        // both sides ascend by cluster: the maps are equal iff they are equal entry by entry
        const int rank = written + popc64(m & below);
        differ |= rank >= n_old || d.old_cluster[q0 + rank] != d.seg_cluster[s] || d.old_cap[q0 + rank] != d.cap[s];
      }
      written += popc64(m & gm);
    }
    retry = group_min_i64<W>(retry);
    const bool any_bo = (ballot(bo) & gm) != 0, any_differ = (ballot(differ) & gm) != 0;
    if (live && gl == 0) {
      // equality.Semantic.DeepEqual of the two maps; nil and empty are equal (controller.go:247)
      d.changed[o] = (any_differ || written != n_old) ? 1 : 0;
      d.n_written[o] = written;
      d.retry_after[o] = retry;
      d.backoff[o] = any_bo ? 1 : 0;
    }
  }
}

hipError_t launch_migrate_segments(const MigrateDev& d, const MigrateRoute& r, hipStream_t st) {
  (void)hipGetLastError();
  const unsigned grid = (unsigned)(r.grid + r.long_grid);
  if (grid > 0) {
    switch (r.width) {
      case 8: hipLaunchKernelGGL(migrate_segment_kernel<8>, dim3(grid), dim3(256), 0, st, d); break;
      case 16: hipLaunchKernelGGL(migrate_segment_kernel<16>, dim3(grid), dim3(256), 0, st, d); break;
      case 32: hipLaunchKernelGGL(migrate_segment_kernel<32>, dim3(grid), dim3(256), 0, st, d); break;
      default: hipLaunchKernelGGL(migrate_segment_kernel<64>, dim3(grid), dim3(256), 0, st, d); break;
    }
  }
  return hipGetLastError();
}

hipError_t launch_migrate_objects(const MigrateDev& d, const MigrateRoute& r, hipStream_t st) {
  (void)hipGetLastError();
  const unsigned grid = (unsigned)r.obj_grid;
  if (grid > 0) {
    switch (r.obj_width) {
      case 8: hipLaunchKernelGGL(migrate_object_kernel<8>, dim3(grid), dim3(256), 0, st, d); break;
      case 16: hipLaunchKernelGGL(migrate_object_kernel<16>, dim3(grid), dim3(256), 0, st, d); break;
      case 32: hipLaunchKernelGGL(migrate_object_kernel<32>, dim3(grid), dim3(256), 0, st, d); break;
      default: hipLaunchKernelGGL(migrate_object_kernel<64>, dim3(grid), dim3(256), 0, st, d); break;
    }
  }
  return hipGetLastError();
}

}  // namespace kad
