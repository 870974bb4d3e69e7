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
  if (grid > 0)
    with_width<MIG_MIN_WIDTH>(r.width, [&](auto W) {
      hipLaunchKernelGGL(migrate_segment_kernel<decltype(W)::value>, dim3(grid), dim3(256), 0, st, d);
    });
  return hipGetLastError();
}

hipError_t launch_migrate_objects(const MigrateDev& d, const MigrateRoute& r, hipStream_t st) {
  (void)hipGetLastError();
  const unsigned grid = (unsigned)r.obj_grid;
  if (grid > 0)
    with_width<MIG_MIN_WIDTH>(r.obj_width, [&](auto W) {
      hipLaunchKernelGGL(migrate_object_kernel<decltype(W)::value>, dim3(grid), dim3(256), 0, st, d);
    });
  return hipGetLastError();
}

}  // namespace kad

// ------------------------------------------------------ host half: kad_migrate_*
#include "kad_arena.h"

using namespace kad;

extern "C" {

// ------------------------------------------------------ auto-migration
// Every offset array monotone from 0 and ending at its count, every id in [0, n_ids) and strictly ascending
// within its object, every flag known, every time inside the domain: all of it on the host, before anything is
// copied or launched. With seg_obj / long_list (kad_migrate_estimate) the same pass leaves the object of
// every segment and the segments of the long path (not skipped, more than long_min pods), ascending.
static int validate_migrate(const kad_migrate_batch* b, const kad_migrate_view* out, int C, int long_min,
                            std::vector<int32_t>* seg_obj, std::vector<int32_t>* long_list, std::string* err) {
  auto bad = [&](const char* m) {
    *err = m;
    return KAD_EINVAL;
  };
  const int64_t n_ids = b->n_ids, O = b->n_objects, S = b->n_segments, P = b->n_pods, N = b->n_old;
  constexpr int64_t TMAX = KAD_MIG_TIME_MAX;
  if (n_ids < C || n_ids > MIG_MAX_IDS) return bad("n_ids must lie in [the snapshot's clusters, 131072]");
  if (O < 0 || S < 0 || P < 0 || N < 0) return bad("negative count");
  if (b->now_ns < 0 || b->now_ns > TMAX) return bad("now_ns outside [0, 2^61]");
  if (!b->obj_seg_off || !b->old_off || !b->seg_pod_off) return bad("offset array missing");
  if ((O && !b->obj_threshold_ns) || (S && (!b->seg_cluster || !b->seg_desired || !b->seg_flags)) ||
      (P && (!b->pod_t_ns || !b->pod_flags)) || (N && (!b->old_cluster || !b->old_cap)))
    return bad("input array missing");
  {
    const int32_t *so = b->obj_seg_off, *oo = b->old_off;
    if (off_bad(so, O) || off_bad(oo, O)) return bad("obj_seg_off / old_off not monotone from 0");
    if (so[O] != S || oo[O] != N) return bad("obj_seg_off / old_off does not end at n_segments / n_old");
    const int64_t* po = b->seg_pod_off;
    if (po[0] != 0 || first_bad(S, [&](int64_t i) { return po[i + 1] < po[i] || po[i + 1] - po[i] > INT32_MAX; }) >= 0)
      return bad("seg_pod_off not monotone from 0, or a segment of more than 2^31 - 1 pods");
    if (po[S] != P) return bad("seg_pod_off does not end at n_pods");
  }
  {
    const int64_t* th = b->obj_threshold_ns;
    if (first_bad(O, [&](int64_t i) { return th[i] < -TMAX || th[i] > TMAX; }) >= 0)
      return bad("obj_threshold_ns beyond 2^61 in magnitude");
    // ids in range and strictly ascending within each object, on both sides
    const int32_t *so = b->obj_seg_off, *sc = b->seg_cluster, *oo = b->old_off, *oc = b->old_cluster;
    auto asc_bad = [&](const int32_t* off, const int32_t* id, int64_t i) {
      for (int32_t j = off[i]; j < off[i + 1]; ++j)
        if (id[j] < 0 || id[j] >= n_ids || (j > off[i] && id[j] <= id[j - 1])) return true;
      return false;
    };
    if (first_bad(O, [&](int64_t i) { return asc_bad(so, sc, i); }) >= 0)
      return bad("seg_cluster out of range or not strictly ascending within an object");
    if (first_bad(O, [&](int64_t i) { return asc_bad(oo, oc, i); }) >= 0)
      return bad("old_cluster out of range or not strictly ascending within an object");
    const uint8_t* sf = b->seg_flags;
    if (first_bad(S, [&](int64_t i) {
          return (sf[i] & ~(KAD_MIG_SEG_SKIP | KAD_MIG_SEG_BACKOFF)) || ((sf[i] & KAD_MIG_SEG_BACKOFF) && !(sf[i] & KAD_MIG_SEG_SKIP));
        }) >= 0)
      return bad("seg_flags: unknown flag, or BACKOFF without SKIP");
    const uint8_t* pf = b->pod_flags;
    const int64_t* pt = b->pod_t_ns;
    if (first_bad(P, [&](int64_t i) {
          if (pf[i] & ~(KAD_MIG_POD_DELETING | KAD_MIG_POD_UNSCHED | KAD_MIG_POD_TZERO)) return true;
          return !(pf[i] & KAD_MIG_POD_TZERO) && (pt[i] < -TMAX || pt[i] > TMAX);
        }) >= 0)
      return bad("pod_flags: unknown flag, or pod_t_ns beyond 2^61 in magnitude");
  }
  if (!out || (S && (!out->uns || !out->next_cross || !out->cap)) ||
      (O && (!out->changed || !out->n_written || !out->retry_after || !out->backoff)))
    return bad("output view missing");
  if (seg_obj) {
    seg_obj->resize((size_t)S);
    int32_t* so = seg_obj->data();
    const int32_t* off = b->obj_seg_off;
    host_parallel((int)O, [&](int lo, int hi) {
      for (int i = lo; i < hi; ++i)
        for (int32_t j = off[i]; j < off[i + 1]; ++j) so[j] = i;
    });
  }
  if (long_list) {
    long_list->clear();
    const int64_t* po = b->seg_pod_off;
    const uint8_t* sf = b->seg_flags;
    for (int64_t i = 0; i < S; ++i)
      if (po[i + 1] - po[i] > long_min && !(sf[i] & KAD_MIG_SEG_SKIP)) long_list->push_back((int32_t)i);
  }
  return KAD_OK;
}

static int migrate_estimate_locked(kad_ctx* c, const kad_migrate_batch* b, const kad_migrate_view* out) {
  if (!c->have_snapshot) return fail(c, KAD_ESTATE, "a snapshot must be uploaded first");
  Stage& stg = c->stage[STG_MIGRATE];
  const int long_min = stg.force.long_min_or(MIG_LONG_MIN);
  std::string err;
  std::vector<int32_t> seg_obj, long_list;
  if (int r = validate_migrate(b, out, c->sd.C, long_min, &seg_obj, &long_list, &err)) return fail(c, r, err);
  const int O = b->n_objects, S = b->n_segments, N = b->n_old;
  const int64_t P = b->n_pods;
  if (O == 0) return KAD_OK;
  HIPCHK(c, hipSetDevice(c->device));
  MigrateRoute route = route_migrate(S, P, (int)long_list.size(), O, n_cus());
  group_force_apply(stg.force, true, S, n_cus(), route.width, route.grid, &route.stride);  // even when every segment is long
  route.long_min = long_min;
  // one buffer: the inputs, then the outputs
  const size_t o = (size_t)O, sg = (size_t)S, pd = (size_t)P, n = (size_t)N, nl = long_list.size();
  MigrateDev md{};
  md.O = O;
  md.S = S;
  md.now = b->now_ns;
  md.width = route.width;
  md.obj_width = route.obj_width;
  md.long_min = route.long_min;
  md.n_long = (int)nl;
  Arena a;
  a.in(md.obj_seg_off, b->obj_seg_off, o + 1);
  a.in(md.obj_thr, b->obj_threshold_ns, o);
  a.in(md.seg_obj, seg_obj.data(), sg);
  a.in(md.seg_cluster, b->seg_cluster, sg);
  a.in(md.seg_desired, b->seg_desired, sg);
  a.in(md.seg_flags, b->seg_flags, sg);
  a.in(md.seg_pod_off, b->seg_pod_off, sg + 1);
  a.in(md.pod_t, b->pod_t_ns, pd);
  a.in(md.pod_flags, b->pod_flags, pd);
  a.in(md.long_list, long_list.data(), nl);
  a.in(md.old_off, b->old_off, o + 1);
  a.in(md.old_cluster, b->old_cluster, n);
  a.in(md.old_cap, b->old_cap, n);
  a.out(md.uns, out->uns, sg);
  a.out(md.next_cross, out->next_cross, sg);
  a.out(md.cap, out->cap, sg);
  a.out(md.changed, out->changed, o);
  a.out(md.n_written, out->n_written, o);
  a.out(md.retry_after, out->retry_after, o);
  a.out(md.backoff, out->backoff, o);
  if (int r = a.commit(c, stg.buf)) return r;
  HIPCHK(c, hipEventRecord(stg.ev[0], c->stream));
  HIPCHK(c, launch_migrate_segments(md, route, c->stream));
  HIPCHK(c, hipEventRecord(stg.ev[1], c->stream));
  HIPCHK(c, launch_migrate_objects(md, route, c->stream));
  HIPCHK(c, hipEventRecord(stg.ev[2], c->stream));
  stage_ran(stg, route);
  if (int r = a.fetch(c)) return r;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return KAD_OK;
}

int kad_migrate_check(const kad_migrate_batch* b, const kad_migrate_view* out, int32_t n_clusters) {
  return check_guarded([&]() -> int {
    if (!b || n_clusters < 0) return KAD_EINVAL;
    std::string err;
    return validate_migrate(b, out, n_clusters, MIG_LONG_MIN, nullptr, nullptr, &err);
  });
}

int kad_migrate_estimate(kad_ctx* c, const kad_migrate_batch* b, const kad_migrate_view* out) {
  return entry(c, b != nullptr, [&]() -> int {
    return migrate_estimate_locked(c, b, out);
  });
}

int kad_migrate_timing(kad_ctx* c, float ms[2]) { return stage_timing(c, STG_MIGRATE, 2, ms, "no kad_migrate_estimate ran"); }

int kad_migrate_route_eval(int32_t n_segments, int64_t n_pods, int32_t n_long, int32_t n_objects, int32_t n_cu,
                           int32_t* out) {
  if (!out || n_segments < 0 || n_pods < 0 || n_long < 0 || n_long > n_segments || n_objects < 0 || n_cu < 1)
    return KAD_EINVAL;
  return route_record<KAD_MIG_ROUTE_FIELDS>(out, route_migrate(n_segments, n_pods, n_long, n_objects, n_cu));
}

int kad_migrate_last_route(kad_ctx* c, int32_t* out) { return stage_last_route(c, STG_MIGRATE, out, "no kad_migrate_estimate ran"); }

int kad_migrate_debug_route(kad_ctx* c, int32_t force_width, int32_t force_long_min) {
  return stage_debug_route(c, STG_MIGRATE, group_width_ok(force_width, MIG_MIN_WIDTH), GroupForce{force_width, force_long_min, 0});
}

}  // extern "C"
