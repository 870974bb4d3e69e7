// Policy reference counts (kad_policyrc_count): per policy, the number of federated objects that reference it after
// a batch of reference changes, and whether its status is to be written.
//
// Counter.Update (pkg/controllers/policyrc/counter.go:50-80) takes one object at a time under one mutex: every
// previously known policy of the object loses a reference (:67-74), every new one gains one (:76-78), both are
// flagged for persisting; reconcilePersist (controller.go:280-366) then compares the count with the policy's stored
// typed count and the sum of its typed counts with its stored total. Over a batch that is a signed histogram over
// the policy ids and a row-wise comparison:
//
//   prc_count_kernel   two non-negative int32 histograms, removals and additions (so that "named by either list"
//                      needs no bitmap of its own), zeroed on the stream before the launch. Ids are read 16 B a
//                      lane, the blocks striding over each list, the last n % 4 ids one to a lane of block 0.
//                      LDS-private (P <= PRC_LDS_BINS): a block counts into 2 * P bins of its own with LDS atomics
//                      and adds its non-zero bins to the histograms. Global: a wave merges the runs of equal
//                      neighbouring ids within its 4 x 64 ids (batches arrive grouped by namespace, hence by policy)
//                      and adds one global atomic per run.
//   prc_apply_kernel   one thread per policy: new_count, new_total, state, n_negative.
//
// Everything is integer and every atomic is a relaxed add whose result nobody reads before the kernel ends, so the
// outputs do not depend on the order of arrival. Nothing here writes state that kad_schedule reads.
#include "kad_device.h"
#include "kad_policyrc.h"
#include "kad_wave.h"

namespace kad {

namespace {

// relaxed, agent scope: the sums are read by the next kernel on the stream
__device__ __forceinline__ void prc_add(int32_t* p, int v) {
  __hip_atomic_fetch_add(p, v, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
}
__device__ __forceinline__ void prc_lds_inc(int32_t* p) {
  __hip_atomic_fetch_add(p, 1, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_WORKGROUP);
}

// one list into a block's own bins
__device__ __forceinline__ void prc_list_lds(const int32_t* ids, int n, int32_t* bins) {
  const int n4 = n / PRC_VEC, stride = gridDim.x * PRC_THREADS;
  const int4* v4 = reinterpret_cast<const int4*>(ids);
  for (int k = blockIdx.x * PRC_THREADS + threadIdx.x; k < n4; k += stride) {
    const int4 v = v4[k];
    prc_lds_inc(bins + v.x);
    prc_lds_inc(bins + v.y);
    prc_lds_inc(bins + v.z);
    prc_lds_inc(bins + v.w);
  }
  const int tail = n - n4 * PRC_VEC;
  if (blockIdx.x == 0 && (int)threadIdx.x < tail) prc_lds_inc(bins + ids[n4 * PRC_VEC + threadIdx.x]);
}

// One list into the global histogram g. A wave's step is 4 x 64 consecutive ids, id j of it in lane j / 4; id j
// heads a run when it differs from id j - 1 (or j is 0), and the head adds the distance to the next head (or to the
// end of the step's ids). The heads of every lane as four wave masks, so that a lane finds the next head above it
// with bit operations alone.
__device__ __forceinline__ void prc_list_runs(const int32_t* ids, int n, int32_t* g) {
  const int n4 = n / PRC_VEC, stride = gridDim.x * PRC_THREADS, t = lane_id_h();
  const int4* v4 = reinterpret_cast<const int4*>(ids);
  const int first = __builtin_amdgcn_readfirstlane((int)(blockIdx.x * PRC_THREADS + (threadIdx.x & ~(WAVE - 1))));
  for (int base = first; base < n4; base += stride) {
    const bool valid = base + t < n4;  // the lanes with ids are a prefix of the wave
    const int4 v = valid ? v4[base + t] : make_int4(-1, -1, -1, -1);
    const int prev = __shfl_up(v.w, 1);
    const bool h0 = valid && (t == 0 || v.x != prev), h1 = valid && v.y != v.x, h2 = valid && v.z != v.y,
               h3 = valid && v.w != v.z;
    const uint64_t b0 = ballot(h0), b1 = ballot(h1), b2 = ballot(h2), b3 = ballot(h3);
    const int end = PRC_VEC * popc64(ballot(valid));
    const uint64_t above = (b0 | b1 | b2 | b3) & ~((2ull << t) - 1ull);  // heads in the lanes above this one
    int next = end;
    if (above) {
      const int l = __builtin_ctzll(above);
      const uint64_t m = 1ull << l;
      next = PRC_VEC * l + ((b0 & m) ? 0 : (b1 & m) ? 1 : (b2 & m) ? 2 : 3);
    }
    const int at = PRC_VEC * t;
    if (h3) {
      prc_add(g + v.w, next - (at + 3));
      next = at + 3;
    }
    if (h2) {
      prc_add(g + v.z, next - (at + 2));
      next = at + 2;
    }
    if (h1) {
      prc_add(g + v.y, next - (at + 1));
      next = at + 1;
    }
    if (h0) prc_add(g + v.x, next - at);
  }
  const int tail = n - n4 * PRC_VEC;
  if (blockIdx.x == 0 && (int)threadIdx.x < tail) prc_add(g + ids[n4 * PRC_VEC + threadIdx.x], 1);
}

}  // namespace

template <int PATH>
__global__ __launch_bounds__(PRC_THREADS) void prc_count_kernel(PolicyrcDev d) {
  if constexpr (PATH == PRC_PATH_LDS) {
    extern __shared__ int32_t prc_bins[];  // [2 * P]: removals, then additions
    const int nb = 2 * d.P;
    for (int i = threadIdx.x; i < nb; i += PRC_THREADS) prc_bins[i] = 0;
    __syncthreads();
    prc_list_lds(d.dec_ids, d.n_dec, prc_bins);
    prc_list_lds(d.inc_ids, d.n_inc, prc_bins + d.P);
    __syncthreads();
    for (int i = threadIdx.x; i < nb; i += PRC_THREADS) {
      const int v = prc_bins[i];
      if (v) prc_add(d.hist + i, v);
    }
  } else {
    prc_list_runs(d.dec_ids, d.n_dec, d.hist);
    prc_list_runs(d.inc_ids, d.n_inc, d.hist + d.P);
  }
}

__global__ __launch_bounds__(PRC_THREADS) void prc_apply_kernel(PolicyrcDev d) {
  const int i = blockIdx.x * PRC_THREADS + threadIdx.x;
  if (i >= d.P) return;
  const int32_t dec = d.hist[i], inc = d.hist[d.P + i];
  const int64_t nc = wsub(wadd(d.count[i], inc), dec), nt = wadd(d.stored_rest[i], nc);
  const uint8_t pf = d.pol_flags[i];
  uint8_t st = (dec | inc) ? PRC_FLAGGED : (uint8_t)0;
  // reconcilePersist's hasChange (controller.go:337-353), for a policy that is in the store (:307-310)
  if ((pf & PRC_POL_EXISTS) && (st || (pf & PRC_POL_ENQUEUED)) && (nc != d.stored_typed[i] || nt != d.stored_total[i]))
    st |= PRC_UPDATE;
  if (nc < 0) {
    st |= PRC_NEGATIVE;
    atomicAdd(d.n_negative, 1);
  }
  d.new_count[i] = nc;
  d.new_total[i] = nt;
  d.state[i] = st;
}

hipError_t launch_policyrc_count(const PolicyrcDev& d, const PolicyrcRoute& r, hipStream_t st) {
  (void)hipGetLastError();
  if (r.grid > 0) {
    if (r.path == PRC_PATH_LDS)
      hipLaunchKernelGGL(prc_count_kernel<PRC_PATH_LDS>, dim3((unsigned)r.grid), dim3((unsigned)r.threads),
                         (size_t)2 * d.P * sizeof(int32_t), st, d);
    else
      hipLaunchKernelGGL(prc_count_kernel<PRC_PATH_GLOBAL>, dim3((unsigned)r.grid), dim3((unsigned)r.threads), 0, st, d);
  }
  return hipGetLastError();
}

hipError_t launch_policyrc_apply(const PolicyrcDev& d, const PolicyrcRoute& r, hipStream_t st) {
  (void)hipGetLastError();
  if (r.apply_grid > 0)
    hipLaunchKernelGGL(prc_apply_kernel, dim3((unsigned)r.apply_grid), dim3((unsigned)r.threads), 0, st, d);
  return hipGetLastError();
}

}  // namespace kad

// ------------------------------------------------------ host half: kad_policyrc_*
#include "kad_arena.h"

using namespace kad;

extern "C" {

// The counts, every array that its count needs, every id in [0, P), every flag known, reserved == 0, the output
// view: all of it on the host, before anything is copied or launched.
static int validate_policyrc(const kad_policyrc_batch* b, const kad_policyrc_view* out, std::string* err) {
  auto bad = [&](const char* m) {
    *err = m;
    return KAD_EINVAL;
  };
  const int64_t P = b->n_policies, nd = b->n_dec, ni = b->n_inc;
  if (P < 0 || nd < 0 || ni < 0) return bad("negative count");
  if (b->reserved != 0) return bad("reserved is not 0");
  if ((nd && !b->dec_ids) || (ni && !b->inc_ids)) return bad("id list missing");
  if (P && (!b->count || !b->stored_typed || !b->stored_rest || !b->stored_total || !b->pol_flags))
    return bad("input array missing");
  const int32_t *di = b->dec_ids, *ii = b->inc_ids;
  if (first_bad(nd, [&](int64_t k) { return di[k] < 0 || di[k] >= P; }) >= 0) return bad("dec_ids: id outside [0, n_policies)");
  if (first_bad(ni, [&](int64_t k) { return ii[k] < 0 || ii[k] >= P; }) >= 0) return bad("inc_ids: id outside [0, n_policies)");
  constexpr uint8_t POL_ALL = KAD_PRC_POL_EXISTS | KAD_PRC_POL_ENQUEUED;
  const uint8_t* pf = b->pol_flags;
  if (first_bad(P, [&](int64_t i) { return (pf[i] & ~POL_ALL) != 0; }) >= 0) return bad("pol_flags: unknown flag");
  if (!out || !out->n_negative || (P && (!out->new_count || !out->new_total || !out->state))) return bad("output view missing");
  return KAD_OK;
}

static int policyrc_count_locked(kad_ctx* c, const kad_policyrc_batch* b, const kad_policyrc_view* out) {
  std::string err;
  if (int r = validate_policyrc(b, out, &err)) return fail(c, r, err);
  const int P = b->n_policies;
  Stage& stg = c->stage[STG_POLICYRC];
  if (stg.force.path == 1 && P > PRC_LDS_BINS)
    return fail(c, KAD_EINVAL, "kad_policyrc_debug_route: the LDS-private path forced on more policies than its bins");
  if (P == 0) {
    *out->n_negative = 0;
    return KAD_OK;
  }
  HIPCHK(c, hipSetDevice(c->device));
  const PolicyrcRoute route = route_policyrc(P, (int64_t)b->n_dec + b->n_inc, n_cus(), stg.force.path);
  const size_t p = (size_t)P;
  PolicyrcDev d{};
  d.P = P;
  d.n_dec = b->n_dec;
  d.n_inc = b->n_inc;
  Arena a;
  a.in(d.dec_ids, b->dec_ids, (size_t)b->n_dec);
  a.in(d.inc_ids, b->inc_ids, (size_t)b->n_inc);
  a.in(d.count, b->count, p);
  a.in(d.stored_typed, b->stored_typed, p);
  a.in(d.stored_rest, b->stored_rest, p);
  a.in(d.stored_total, b->stored_total, p);
  a.in(d.pol_flags, b->pol_flags, p);
  a.out(d.hist, 2 * p);
  a.out(d.new_count, out->new_count, p);
  a.out(d.new_total, out->new_total, p);
  a.out(d.state, out->state, p);
  a.out(d.n_negative, out->n_negative, 1);
  HIPCHK(c, hipEventRecord(stg.ev[0], c->stream));
  if (int r = a.commit(c, stg.buf)) return r;
  HIPCHK(c, hipEventRecord(stg.ev[1], c->stream));
  HIPCHK(c, hipMemsetAsync(d.hist, 0, 2 * p * sizeof *d.hist, c->stream));
  HIPCHK(c, hipMemsetAsync(d.n_negative, 0, sizeof *d.n_negative, c->stream));
  HIPCHK(c, launch_policyrc_count(d, route, c->stream));
  HIPCHK(c, hipEventRecord(stg.ev[2], c->stream));
  HIPCHK(c, launch_policyrc_apply(d, route, c->stream));
  HIPCHK(c, hipEventRecord(stg.ev[3], c->stream));
  if (int r = a.fetch(c)) return r;
  stage_ran(stg, route);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return KAD_OK;
}

int kad_policyrc_check(const kad_policyrc_batch* b, const kad_policyrc_view* out) {
  return check_guarded([&]() -> int {
    if (!b) return KAD_EINVAL;
    std::string err;
    return validate_policyrc(b, out, &err);
  });
}

int kad_policyrc_count(kad_ctx* c, const kad_policyrc_batch* b, const kad_policyrc_view* out) {
  return entry(c, b != nullptr, [&]() -> int {
    return policyrc_count_locked(c, b, out);
  });
}

int kad_policyrc_timing(kad_ctx* c, float ms[3]) { return stage_timing(c, STG_POLICYRC, 3, ms, "no kad_policyrc_count ran"); }

int kad_policyrc_route_eval(int32_t n_policies, int64_t n_ids, int32_t n_cu, int32_t* out) {
  if (!out || n_policies < 0 || n_ids < 0 || n_cu < 1) return KAD_EINVAL;
  return route_record<KAD_PRC_ROUTE_FIELDS>(out, route_policyrc(n_policies, n_ids, n_cu));
}

int kad_policyrc_last_route(kad_ctx* c, int32_t* out) { return stage_last_route(c, STG_POLICYRC, out, "no kad_policyrc_count ran"); }

int kad_policyrc_debug_route(kad_ctx* c, int32_t force_path) {
  return stage_debug_route(c, STG_POLICYRC, force_path >= 0 && force_path <= 2, GroupForce{0, 0, 0, force_path});
}

}  // extern "C"
