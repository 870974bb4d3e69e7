// Status aggregation (kad_status_aggregate): the aggregated status of every source object from its member
// clusters' copies.
//
// The status aggregator folds, per source object and on every member-object event, the statuses of the object's
// copies in the member clusters into the source object's status (reconcile, pkg/controllers/statusaggregator/
// controller.go:249-348): for a Deployment the five replica counts summed and the observed generation
// (plugins/deployment.go:42-186), for a Job the three pod counts summed, the earliest start time, the latest
// completion time and how many members completed or failed (plugins/job.go:43-163); the status is written if it
// differs from the one the object holds. On the device that is one segmented reduction over (object, member
// cluster) segments held in columns, and the compare with the old status' columns:
//
//   sagg_kernel<W, KIND>  blocks below n_long: one listed long object per 256-thread block (four strided loads a
//                         lane in flight, DPP reduce per wave, LDS combine); the other blocks: a wave is 64 / W
//                         lane groups, each group reduces one object at a time (xor shuffles below W) and one
//                         lane of the group derives the outputs and stores them
//
// The sums are Go int32 and wrap: they are accumulated as uint32. No atomics, no state that kad_schedule reads.
#include "kad_statusagg.h"
#include "kad_wave.h"

namespace kad {

// what one lane has folded of an object's segments
template <int KIND>
struct SaggAcc {
  uint32_t sum[KIND == SAGG_DEPLOYMENT ? SAGG_NV_DEP : SAGG_NV_JOB];
  // Deployment: a = 1 once needUpdateObservedGeneration is cleared. Job: a / b = completed / failed members
  int a, b;
  int64_t start, done;  // Job
};

template <int KIND>
__device__ __forceinline__ void acc_init(SaggAcc<KIND>& x) {
  constexpr int NV = KIND == SAGG_DEPLOYMENT ? SAGG_NV_DEP : SAGG_NV_JOB;
#pragma unroll
  for (int v = 0; v < NV; ++v) x.sum[v] = 0;
  x.a = x.b = 0;
  x.start = I64_MAX;
  x.done = I64_MIN;
}

// one member cluster's copy: flags f, the two int64 columns a / b, the int32 columns at index s
template <int KIND>
__device__ __forceinline__ void seg_step(const SaggDev& d, int64_t s, uint8_t f, int64_t a, int64_t b, SaggAcc<KIND>& x) {
  constexpr int NV = KIND == SAGG_DEPLOYMENT ? SAGG_NV_DEP : SAGG_NV_JOB;
  if (f & SAGG_SEG_NIL) {  // a nil status is skipped (deployment.go:89-92, job.go:68-70)
    if (KIND == SAGG_DEPLOYMENT) x.a = 1;
    return;
  }
  if (KIND == SAGG_DEPLOYMENT) {
    // the cluster's controller has not observed the synced generation (deployment.go:100-102)
    if (!(f & SAGG_SEG_SYNCED) || a != b) x.a = 1;
  } else {
    if ((f & SAGG_SEG_START) && a < x.start) x.start = a;  // a nil start time never replaces a set one (job.go:78-80)
    if (f & SAGG_SEG_DONE) {
      ++x.a;
      x.done = b > x.done ? b : x.done;
    } else if (f & SAGG_SEG_FAILED) {
      ++x.b;
    }
  }
#pragma unroll
  for (int v = 0; v < NV; ++v) x.sum[v] += (uint32_t)d.seg_vals[(int64_t)v * d.S + s];
}

template <int KIND>
__device__ __forceinline__ void seg_load_step(const SaggDev& d, int64_t s, SaggAcc<KIND>& x) {
  seg_step<KIND>(d, s, d.seg_flags[s], d.seg_a[s], d.seg_b[s], x);
}

// the outputs of object o with n segments from its folded segments (one lane)
template <int KIND>
__device__ __forceinline__ void store_object(const SaggDev& d, int o, int n, uint8_t of, const SaggAcc<KIND>& x) {
  constexpr int NV = KIND == SAGG_DEPLOYMENT ? SAGG_NV_DEP : SAGG_NV_JOB;
  const int64_t O = d.O;
  bool differ = (of & SAGG_OBJ_OLD_OTHER) != 0;
  // zero fields are omitted from the new status and an absent old field is a 0 column: DeepEqual of the numeric
  // part is equality of the columns
#pragma unroll
  for (int v = 0; v < NV; ++v) {
    const int32_t sum = (int32_t)x.sum[v];
    d.sums[(int64_t)v * O + o] = sum;
    differ |= (int64_t)sum != d.old_vals[(int64_t)v * O + o];
  }
  if (KIND == SAGG_DEPLOYMENT) {
    const bool keep = (of & SAGG_OBJ_UPTODATE) && !x.a;  // needUpdateObservedGeneration (deployment.go:131-135)
    const int64_t obs = keep ? d.obj_generation[o] : d.obj_observed[o];
    d.observed[o] = obs;
    differ |= obs != d.old_vals[(int64_t)NV * O + o];
  } else {
    const int fin = x.a + x.b;
    const bool finished = fin > 0 && fin == n;  // a nil-status member counts in len(clusterObjs) (job.go:96)
    d.start_min[o] = x.start;
    d.done_max[o] = x.done;
    d.n_done[o] = x.a;
    d.n_failed[o] = x.b;
    d.finished[o] = finished ? 1 : 0;
    // completionTime is written only when every member completed (job.go:109-113)
    const int64_t done = finished && x.b == 0 ? x.done : I64_MIN;
    differ |= x.start != d.old_vals[(int64_t)NV * O + o] || done != d.old_vals[(int64_t)(NV + 1) * O + o];
  }
  d.changed[o] = differ ? 1 : 0;
}

// an object the host found in error: every output zero
template <int KIND>
__device__ __forceinline__ void store_error(const SaggDev& d, int o) {
  constexpr int NV = KIND == SAGG_DEPLOYMENT ? SAGG_NV_DEP : SAGG_NV_JOB;
#pragma unroll
  for (int v = 0; v < NV; ++v) d.sums[(int64_t)v * d.O + o] = 0;
  if (KIND == SAGG_DEPLOYMENT) {
    d.observed[o] = 0;
  } else {
    d.start_min[o] = 0;
    d.done_max[o] = 0;
    d.n_done[o] = 0;
    d.n_failed[o] = 0;
    d.finished[o] = 0;
  }
  d.changed[o] = 0;
}

__device__ __forceinline__ uint32_t wave_sum_u32(uint32_t v) {  // wrapping; every lane active
  v += (uint32_t)dpp32<0x111, 0xf>(0, (int)v);
  v += (uint32_t)dpp32<0x112, 0xf>(0, (int)v);
  v += (uint32_t)dpp32<0x114, 0xf>(0, (int)v);
  v += (uint32_t)dpp32<0x118, 0xf>(0, (int)v);
  v += (uint32_t)dpp32<0x142, 0xa>(0, (int)v);
  v += (uint32_t)dpp32<0x143, 0xc>(0, (int)v);
  return (uint32_t)__builtin_amdgcn_readlane((int)v, 63);
}

template <int W>
__device__ __forceinline__ int64_t sagg_group_min(int64_t v) {
#pragma unroll
  for (int m = W / 2; m >= 1; m >>= 1) {
    const int64_t o = shfl_xor_i64(v, m);
    v = o < v ? o : v;
  }
  return v;
}
template <int W>
__device__ __forceinline__ int64_t sagg_group_max(int64_t v) {
#pragma unroll
  for (int m = W / 2; m >= 1; m >>= 1) {
    const int64_t o = shfl_xor_i64(v, m);
    v = o > v ? o : v;
  }
  return v;
}

template <int W, int KIND>
__global__ __launch_bounds__(256) void sagg_kernel(SaggDev d) {
  constexpr int NV = KIND == SAGG_DEPLOYMENT ? SAGG_NV_DEP : SAGG_NV_JOB;
  SaggAcc<KIND> x;
  acc_init<KIND>(x);
  if ((int)blockIdx.x < d.n_long) {
    // ---- long path: one listed object per block
    __shared__ uint32_t s_sum[4][NV];
    __shared__ int s_a[4], s_b[4];
    __shared__ int64_t s_start[4], s_done[4];
    const int o = d.long_list[blockIdx.x], t = threadIdx.x;
    const int64_t lo = d.obj_seg_off[o], hi = d.obj_seg_off[o + 1];
    int64_t k = lo + t;
    for (; k + 768 < hi; k += 1024) {  // four independent loads a lane and column in flight
      const uint8_t f0 = d.seg_flags[k], f1 = d.seg_flags[k + 256], f2 = d.seg_flags[k + 512], f3 = d.seg_flags[k + 768];
      const int64_t a0 = d.seg_a[k], a1 = d.seg_a[k + 256], a2 = d.seg_a[k + 512], a3 = d.seg_a[k + 768];
      const int64_t b0 = d.seg_b[k], b1 = d.seg_b[k + 256], b2 = d.seg_b[k + 512], b3 = d.seg_b[k + 768];
      seg_step<KIND>(d, k, f0, a0, b0, x);
      seg_step<KIND>(d, k + 256, f1, a1, b1, x);
      seg_step<KIND>(d, k + 512, f2, a2, b2, x);
      seg_step<KIND>(d, k + 768, f3, a3, b3, x);
    }
    for (; k < hi; k += 256) seg_load_step<KIND>(d, k, x);
#pragma unroll
    for (int v = 0; v < NV; ++v) x.sum[v] = wave_sum_u32(x.sum[v]);
    x.a = wave_sum_i32(x.a);
    if (KIND == SAGG_JOB) {
      x.b = wave_sum_i32(x.b);
      x.start = wave_min_i64(x.start);
      x.done = wave_max_i64(x.done);
    }
    if ((t & 63) == 0) {
#pragma unroll
      for (int v = 0; v < NV; ++v) s_sum[t >> 6][v] = x.sum[v];
      s_a[t >> 6] = x.a;
      s_b[t >> 6] = x.b;
      s_start[t >> 6] = x.start;
      s_done[t >> 6] = x.done;
    }
    __syncthreads();
    if (t == 0) {
      for (int q = 1; q < 4; ++q) {
#pragma unroll
        for (int v = 0; v < NV; ++v) x.sum[v] += s_sum[q][v];
        x.a += s_a[q];
        x.b += s_b[q];
        x.start = s_start[q] < x.start ? s_start[q] : x.start;
        x.done = s_done[q] > x.done ? s_done[q] : x.done;
      }
      store_object<KIND>(d, o, (int)(hi - lo), d.obj_flags[o], x);
    }
    return;
  }
  // ---- group path: the loop is uniform over the wave (groups past O idle), so every shuffle sees its group whole
  constexpr int GPB = 256 / W;  // groups a block
  const int gl = (int)threadIdx.x & (W - 1), g = (int)threadIdx.x / W;
  const int64_t stride = (int64_t)(gridDim.x - d.n_long) * GPB;
  for (int64_t base = (int64_t)(blockIdx.x - d.n_long) * GPB; base < d.O; base += stride) {
    const int64_t o64 = base + g;
    const bool live = o64 < d.O;
    const int o = live ? (int)o64 : 0;
    uint8_t of = SAGG_OBJ_ERROR;
    bool reduce = false;
    int n = 0;
    acc_init<KIND>(x);
    if (live) {
      of = d.obj_flags[o];
      reduce = !(of & SAGG_OBJ_ERROR) && !d.obj_long[o];
      if (reduce) {
        const int lo = d.obj_seg_off[o], hi = d.obj_seg_off[o + 1];
        n = hi - lo;
        // consecutive lanes read consecutive segments; consecutive groups hold consecutive objects
        for (int s = lo + gl; s < hi; s += W) seg_load_step<KIND>(d, s, x);
      }
    }
    if (W > 1) {
#pragma unroll
      for (int m = W / 2; m >= 1; m >>= 1) {
#pragma unroll
        for (int v = 0; v < NV; ++v) x.sum[v] += (uint32_t)__shfl_xor((int)x.sum[v], m);
        x.a += __shfl_xor(x.a, m);
        if (KIND == SAGG_JOB) x.b += __shfl_xor(x.b, m);
      }
      if (KIND == SAGG_JOB) {
        x.start = sagg_group_min<W>(x.start);
        x.done = sagg_group_max<W>(x.done);
      }
    }
    if (live && gl == 0) {
      if (reduce)
        store_object<KIND>(d, o, n, of, x);
      else if (of & SAGG_OBJ_ERROR)
        store_error<KIND>(d, o);
    }
  }
}

template <int KIND>
static void launch_kind(const SaggDev& d, int width, unsigned grid, hipStream_t st) {
  with_width<1>(width, [&](auto W) {
    hipLaunchKernelGGL((sagg_kernel<decltype(W)::value, KIND>), dim3(grid), dim3(256), 0, st, d);
  });
}

hipError_t launch_sagg(int kind, const SaggDev& d, const SaggRoute& r, hipStream_t st) {
  (void)hipGetLastError();
  const unsigned grid = (unsigned)(r.grid + r.long_grid);
  if (grid > 0) {
    if (kind == SAGG_DEPLOYMENT)
      launch_kind<SAGG_DEPLOYMENT>(d, r.width, grid, st);
    else
      launch_kind<SAGG_JOB>(d, r.width, grid, st);
  }
  return hipGetLastError();
}

}  // namespace kad

// ------------------------------------------------------ host half: kad_sagg_* / kad_status_aggregate
#include "kad_arena.h"

using namespace kad;

namespace {

// what the validation leaves for the launch: the objects of the long path and the short objects' segments
struct SaggPlan {
  std::vector<uint8_t> obj_long;
  std::vector<int32_t> long_list;
  int64_t short_segments = 0;
};

}  // namespace

extern "C" {

// The kind, the offset array monotone from 0 and ending at n_segments, every flag known and consistent with the
// kind, every time a set flag makes count inside the domain: all of it on the host, before anything is copied or
// launched. With a plan (kad_status_aggregate) the same pass leaves the objects of the long path (not in error,
// more than long_min segments).
static int validate_sagg(const kad_sagg_batch* b, const kad_sagg_view* out, int long_min, SaggPlan* plan, std::string* err) {
  auto bad = [&](const char* m) {
    *err = m;
    return KAD_EINVAL;
  };
  if (b->kind != KAD_SAGG_DEPLOYMENT && b->kind != KAD_SAGG_JOB) return bad("kind is neither KAD_SAGG_DEPLOYMENT nor KAD_SAGG_JOB");
  const bool dep = b->kind == KAD_SAGG_DEPLOYMENT;
  const int64_t O = b->n_objects, S = b->n_segments;
  if (O < 0 || S < 0) return bad("negative count");
  if (!b->obj_seg_off) return bad("offset array missing");
  if (O && (!b->obj_flags || !b->old_vals || (dep && (!b->obj_generation || !b->obj_observed))))
    return bad("input array missing");
  if (S && (!b->seg_vals || !b->seg_flags || (dep ? !b->seg_observed || !b->seg_synced : !b->seg_start || !b->seg_done)))
    return bad("input array missing");
  const int32_t* so = b->obj_seg_off;
  if (off_bad(so, O)) return bad("obj_seg_off not monotone from 0");
  if (so[O] != S) return bad("obj_seg_off does not end at n_segments");
  {
    const uint8_t *of = b->obj_flags, *sf = b->seg_flags;
    constexpr uint8_t OBJ_ALL = KAD_SAGG_OBJ_UPTODATE | KAD_SAGG_OBJ_ERROR | KAD_SAGG_OBJ_OLD_OTHER;
    if (first_bad(O, [&](int64_t i) { return (of[i] & ~OBJ_ALL) != 0; }) >= 0) return bad("obj_flags: unknown flag");
    const uint8_t known = dep ? (KAD_SAGG_SEG_NIL | KAD_SAGG_SEG_SYNCED)
                              : (KAD_SAGG_SEG_NIL | KAD_SAGG_SEG_START | KAD_SAGG_SEG_DONE | KAD_SAGG_SEG_FAILED);
    if (first_bad(S, [&](int64_t i) {
          const uint8_t f = sf[i];
          if (f & ~known) return true;
          // a nil status has no times and no condition; a completed member is not also counted as failed
          if ((f & KAD_SAGG_SEG_NIL) && (f & (KAD_SAGG_SEG_START | KAD_SAGG_SEG_DONE | KAD_SAGG_SEG_FAILED))) return true;
          return (f & KAD_SAGG_SEG_DONE) && (f & KAD_SAGG_SEG_FAILED);
        }) >= 0)
      return bad("seg_flags: a flag unknown to the kind, NIL with START / DONE / FAILED, or DONE with FAILED");
    if (!dep) {
      constexpr int64_t TMAX = KAD_SAGG_TIME_MAX;
      const int64_t *ts = b->seg_start, *td = b->seg_done;
      auto out_of_domain = [](int64_t t) { return t < -TMAX || t > TMAX || t == KAD_SAGG_TIME_ZERO; };
      if (first_bad(S, [&](int64_t i) {
            return ((sf[i] & KAD_SAGG_SEG_START) && out_of_domain(ts[i])) || ((sf[i] & KAD_SAGG_SEG_DONE) && out_of_domain(td[i]));
          }) >= 0)
        return bad("seg_start / seg_done beyond 2^61 in magnitude, or Go's zero time");
    }
  }
  if (!out || (O && (!out->sums || !out->changed)) ||
      (O && (dep ? !out->observed : !out->start_min || !out->done_max || !out->n_done || !out->n_failed || !out->finished)))
    return bad("output view missing");
  if (plan) {
    plan->obj_long.assign((size_t)O, 0);
    for (int64_t i = 0; i < O; ++i) {
      if (b->obj_flags[i] & KAD_SAGG_OBJ_ERROR) continue;
      const int64_t n = so[i + 1] - so[i];
      if (n <= long_min) {
        plan->short_segments += n;
        continue;
      }
      plan->obj_long[(size_t)i] = 1;
      plan->long_list.push_back((int32_t)i);
    }
  }
  return KAD_OK;
}

static int status_aggregate_locked(kad_ctx* c, const kad_sagg_batch* b, const kad_sagg_view* out) {
  Stage& stg = c->stage[STG_SAGG];
  const int long_min = stg.force.long_min_or(SAGG_LONG_MIN);
  std::string err;
  SaggPlan plan;
  if (int r = validate_sagg(b, out, long_min, &plan, &err)) return fail(c, r, err);
  const int O = b->n_objects, S = b->n_segments;
  if (O == 0) return KAD_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const bool dep = b->kind == KAD_SAGG_DEPLOYMENT;
  const int n_long = (int)plan.long_list.size();
  SaggRoute route = route_sagg(O, n_long, plan.short_segments, n_cus());
  group_force_apply(stg.force, n_long < O, O, n_cus(), route.width, route.grid, &route.stride);
  route.long_min = long_min;
  // one buffer: the inputs, then the outputs (the other kind's arrays are absent)
  const size_t o = (size_t)O, sg = (size_t)S, nl = (size_t)n_long;
  const size_t nv = dep ? SAGG_NV_DEP : SAGG_NV_JOB, nold = dep ? SAGG_NOLD_DEP : SAGG_NOLD_JOB;
  SaggDev d{};
  d.O = O;
  d.S = S;
  d.n_long = n_long;
  Arena a;
  a.in(d.obj_seg_off, b->obj_seg_off, o + 1);
  a.in(d.obj_flags, b->obj_flags, o);
  if (dep) {
    a.in(d.obj_generation, b->obj_generation, o);
    a.in(d.obj_observed, b->obj_observed, o);
  } else {
    a.absent(d.obj_generation);
    a.absent(d.obj_observed);
  }
  a.in(d.old_vals, b->old_vals, nold * o);
  a.in(d.seg_vals, b->seg_vals, nv * sg);
  a.in(d.seg_flags, b->seg_flags, sg);
  a.in(d.seg_a, dep ? b->seg_observed : b->seg_start, sg);
  a.in(d.seg_b, dep ? b->seg_synced : b->seg_done, sg);
  a.in(d.obj_long, plan.obj_long.data(), o);
  a.in(d.long_list, plan.long_list.data(), nl);
  a.out(d.sums, out->sums, nv * o);
  a.out(d.changed, out->changed, o);
  if (dep) {
    a.out(d.observed, out->observed, o);
    a.absent(d.start_min);
    a.absent(d.done_max);
    a.absent(d.n_done);
    a.absent(d.n_failed);
    a.absent(d.finished);
  } else {
    a.absent(d.observed);
    a.out(d.start_min, out->start_min, o);
    a.out(d.done_max, out->done_max, o);
    a.out(d.n_done, out->n_done, o);
    a.out(d.n_failed, out->n_failed, o);
    a.out(d.finished, out->finished, o);
  }
  if (int r = a.commit(c, stg.buf)) return r;
  HIPCHK(c, hipEventRecord(stg.ev[0], c->stream));
  HIPCHK(c, launch_sagg(b->kind, d, route, c->stream));
  HIPCHK(c, hipEventRecord(stg.ev[1], c->stream));
  stage_ran(stg, route);
  if (int r = a.fetch(c)) return r;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return KAD_OK;
}

int kad_sagg_check(const kad_sagg_batch* b, const kad_sagg_view* out) {
  return check_guarded([&]() -> int {
    if (!b) return KAD_EINVAL;
    std::string err;
    return validate_sagg(b, out, SAGG_LONG_MIN, nullptr, &err);
  });
}

int kad_status_aggregate(kad_ctx* c, const kad_sagg_batch* b, const kad_sagg_view* out) {
  return entry(c, b != nullptr, [&]() -> int {
    return status_aggregate_locked(c, b, out);
  });
}

int kad_sagg_timing(kad_ctx* c, float ms[1]) { return stage_timing(c, STG_SAGG, 1, ms, "no kad_status_aggregate ran"); }

int kad_sagg_route_eval(int32_t n_objects, int32_t n_long, int64_t short_segments, int32_t n_cu, int32_t* out) {
  if (!out || n_objects < 0 || n_long < 0 || n_long > n_objects || short_segments < 0 || n_cu < 1) return KAD_EINVAL;
  return route_record<KAD_SAGG_ROUTE_FIELDS>(out, route_sagg(n_objects, n_long, short_segments, n_cu));
}

int kad_sagg_last_route(kad_ctx* c, int32_t* out) { return stage_last_route(c, STG_SAGG, out, "no kad_status_aggregate ran"); }

int kad_sagg_debug_route(kad_ctx* c, int32_t force_width, int32_t force_long_min) {
  return stage_debug_route(c, STG_SAGG, group_width_ok(force_width, 1), GroupForce{force_width, force_long_min, 0});
}

}  // extern "C"
