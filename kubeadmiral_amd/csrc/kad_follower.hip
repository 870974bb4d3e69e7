// Follower scheduling (kad_follower_union): the union of the leaders' placements, per follower.
//
// The follower controller sets every follower's placement to the union of ClusterNameUnion() over its
// leaders (leaderPlacementUnion, pkg/controllers/follower/controller.go:532-550) through SetPlacementNames
// (pkg/apis/types/v1alpha1/extensions_placements.go:78-103), whose hasChange is a set comparison with the
// placement the follower holds. Per follower that is a gather of a few short id lists, a set union, a set
// comparison and an ascending listing; the sets are bitmaps over the id space, kept in LDS only:
//
//   follower_union_wave_kernel   n_ids <= 8192: one follower per wave at a time, two 1-KiB bitmaps per wave
//                                (union, current), zeroed once; after each follower the wave walks the same
//                                ids again and clears just the words it set
//   follower_union_block_kernel  larger id spaces: one follower per 256-thread block at a time, block-shared
//                                bitmaps zeroed in full
//   follower_scan_*_kernel       out_off = exclusive scan of the emitted counts (changed followers, or all)
//   follower_emit_*_kernel       re-derives the union of every follower that emits by the same walk and lists
//                                its bits in ascending order at out_off[f]; nothing of size F x n_ids is ever
//                                in global memory
//
// Nothing here writes state that kad_schedule reads.
#include "kad_device.h"
#include "kad_follower.h"
#include "kad_wave.h"

namespace kad {

// T threads walk one id list, one id per thread and step (coalesced within the list)
template <int T, class Op>
__device__ __forceinline__ void walk_ids(const int32_t* p, int n, int t, Op op) {
  for (int k = t; k < n; k += T) op(p[k]);
}

// every id of follower f's leaders, duplicates included: op(id) once per list entry. f is uniform over the
// T threads, so the leader loop and the choice of lists are too.
template <int T, class Op>
__device__ __forceinline__ void walk_union(const FollowerDev& d, int f, int t, Op op) {
  const int j1 = d.fol_off[f + 1];
  for (int j = d.fol_off[f]; j < j1; ++j) {
    const int l = d.fol_leader[j];
    if (l < 0) continue;  // a leader absent from the store (controller.go:541-543)
    if (!d.resident) {
      walk_ids<T>(d.lead_cluster + d.lead_off[l], d.lead_off[l + 1] - d.lead_off[l], t, op);
    } else if (l < d.W) {
      const int st = d.res_status[l];
      if (st == KAD_ST_OK)
        walk_ids<T>(d.res_cluster + (d.out_off[l] - d.slot_lo), d.res_count[l], t, op);
      else if (st == KAD_ST_STICKY)
        walk_ids<T>(d.cur_id + d.cur_off[l], d.cur_off[l + 1] - d.cur_off[l], t, op);
      else if (st != KAD_ST_NO_FEASIBLE && d.sched_off)  // nothing was applied (scheduler.go:505-517)
        walk_ids<T>(d.sched_cluster + d.sched_off[l], d.sched_off[l + 1] - d.sched_off[l], t, op);
    }
    if (d.keep_off) walk_ids<T>(d.keep_cluster + d.keep_off[l], d.keep_off[l + 1] - d.keep_off[l], t, op);
  }
}

template <int T, class Op>
__device__ __forceinline__ void walk_current(const FollowerDev& d, int f, int t, Op op) {
  walk_ids<T>(d.fcur_cluster + d.fcur_off[f], d.fcur_off[f + 1] - d.fcur_off[f], t, op);
}

// the bitmap ops of the walks; ids outside the id space (the -1 of a sticky unit's cluster that left the
// snapshot; the host rejects every other) touch nothing
struct SetBit {
  uint32_t* bm;
  int n_ids;
  __device__ __forceinline__ void operator()(int id) const {
    if ((uint32_t)id < (uint32_t)n_ids) atomicOr(&bm[id >> 5], 1u << (id & 31));
  }
};
struct ClearWord {
  uint32_t* bm;
  int n_ids;
  __device__ __forceinline__ void operator()(int id) const {
    if ((uint32_t)id < (uint32_t)n_ids) bm[id >> 5] = 0;
  }
};

// SetPlacementNames' hasChange: an empty union deletes the placement (changed iff it exists)
__device__ __forceinline__ bool has_change(const FollowerDev& d, int f, int cnt, bool differ) {
  return cnt == 0 ? d.fcur_has[f] != 0 : differ;
}

__device__ __forceinline__ bool emits(const FollowerDev& d, int f) {
  return d.count[f] > 0 && (d.emit_all || d.changed[f]);
}

// lists the set bits of v (word w of a bitmap) from out[pos] on
__device__ __forceinline__ void list_bits(int32_t* out, int64_t pos, int w, uint32_t v) {
  while (v) {
    out[pos++] = w * 32 + (__ffs(v) - 1);
    v &= v - 1;
  }
}

__global__ __launch_bounds__(256) void follower_union_wave_kernel(FollowerDev d) {
  __shared__ uint32_t bm[4][2][FOL_WAVE_WORDS];
  const int wv = threadIdx.x >> 6, t = lane_id_h();
  uint32_t* U = bm[wv][0];
  uint32_t* Cb = bm[wv][1];
  for (int k = t; k < 2 * FOL_WAVE_WORDS; k += WAVE) U[k] = 0;  // both bitmaps, once
  wave_sync();
  const int stride = gridDim.x * 4;
  for (int f0 = blockIdx.x * 4 + wv; f0 < d.F; f0 += stride) {
    const int f = __builtin_amdgcn_readfirstlane(f0);
    walk_union<WAVE>(d, f, t, SetBit{U, d.n_ids});
    walk_current<WAVE>(d, f, t, SetBit{Cb, d.n_ids});
    wave_sync();
    int cnt = 0;
    bool differ = false;
    for (int w = t; w < d.nw; w += WAVE) {
      const uint32_t u = U[w], c = Cb[w];
      cnt += __builtin_popcount(u);
      differ |= u != c;
    }
    cnt = wave_sum_i32(cnt);
    const bool any = ballot(differ) != 0;
    if (t == 0) {
      d.changed[f] = has_change(d, f, cnt, any) ? 1 : 0;
      d.count[f] = cnt;
    }
    wave_sync();
    // only the words this follower set
    walk_union<WAVE>(d, f, t, ClearWord{U, d.n_ids});
    walk_current<WAVE>(d, f, t, ClearWord{Cb, d.n_ids});
    wave_sync();
  }
}

__global__ __launch_bounds__(256) void follower_emit_wave_kernel(FollowerDev d) {
  __shared__ uint32_t bm[4][FOL_WAVE_WORDS];
  if (d.fout_off[d.F] > d.capacity) return;  // the caller retries with fout_off[F] slots
  const int wv = threadIdx.x >> 6, t = lane_id_h();
  uint32_t* U = bm[wv];
  for (int k = t; k < FOL_WAVE_WORDS; k += WAVE) U[k] = 0;
  wave_sync();
  const int stride = gridDim.x * 4;
  for (int f0 = blockIdx.x * 4 + wv; f0 < d.F; f0 += stride) {
    const int f = __builtin_amdgcn_readfirstlane(f0);
    if (!emits(d, f)) continue;
    walk_union<WAVE>(d, f, t, SetBit{U, d.n_ids});
    wave_sync();
    int64_t base = d.fout_off[f];
    for (int w0 = 0; w0 < d.nw; w0 += WAVE) {
      const int w = w0 + t;
      const uint32_t v = w < d.nw ? U[w] : 0u;
      const int pc = __builtin_popcount(v);
      const int incl = wave_incl_sum_i32(pc);
      list_bits(d.out_cluster, base + (incl - pc), w, v);
      base += __builtin_amdgcn_readlane(incl, 63);
    }
    wave_sync();
    walk_union<WAVE>(d, f, t, ClearWord{U, d.n_ids});
    wave_sync();
  }
}

__global__ __launch_bounds__(256) void follower_union_block_kernel(FollowerDev d) {
  __shared__ uint32_t bm[2][FOL_BLOCK_WORDS];
  __shared__ int s_cnt, s_diff;
  const int t = threadIdx.x;
  uint32_t* U = bm[0];
  uint32_t* Cb = bm[1];
  for (int f = blockIdx.x; f < d.F; f += gridDim.x) {
    for (int k = t; k < d.nw; k += 256) {
      U[k] = 0;
      Cb[k] = 0;
    }
    if (t == 0) {
      s_cnt = 0;
      s_diff = 0;
    }
    __syncthreads();
    walk_union<256>(d, f, t, SetBit{U, d.n_ids});
    walk_current<256>(d, f, t, SetBit{Cb, d.n_ids});
    __syncthreads();
    int cnt = 0;
    bool differ = false;
    for (int w = t; w < d.nw; w += 256) {
      const uint32_t u = U[w], c = Cb[w];
      cnt += __builtin_popcount(u);
      differ |= u != c;
    }
    cnt = wave_sum_i32(cnt);
    const bool any = ballot(differ) != 0;
    if ((t & 63) == 0) {
      atomicAdd(&s_cnt, cnt);
      if (any) atomicOr(&s_diff, 1);
    }
    __syncthreads();
    if (t == 0) {
      d.changed[f] = has_change(d, f, s_cnt, s_diff != 0) ? 1 : 0;
      d.count[f] = s_cnt;
    }
    __syncthreads();  // s_cnt / s_diff are read before the next follower resets them
  }
}

__global__ __launch_bounds__(256) void follower_emit_block_kernel(FollowerDev d) {
  __shared__ uint32_t U[FOL_BLOCK_WORDS];
  __shared__ int wsum[4];
  if (d.fout_off[d.F] > d.capacity) return;
  const int t = threadIdx.x, wv = t >> 6;
  for (int f = blockIdx.x; f < d.F; f += gridDim.x) {
    if (!emits(d, f)) continue;
    for (int k = t; k < d.nw; k += 256) U[k] = 0;
    __syncthreads();
    walk_union<256>(d, f, t, SetBit{U, d.n_ids});
    __syncthreads();
    int64_t base = d.fout_off[f];
    for (int w0 = 0; w0 < d.nw; w0 += 256) {
      const int w = w0 + t;
      const uint32_t v = w < d.nw ? U[w] : 0u;
      const int pc = __builtin_popcount(v);
      const int incl = wave_incl_sum_i32(pc);
      if ((t & 63) == 63) wsum[wv] = incl;
      __syncthreads();
      int before = 0, total = 0;
      for (int q = 0; q < 4; ++q) {
        if (q < wv) before += wsum[q];
        total += wsum[q];
      }
      list_bits(d.out_cluster, base + before + (incl - pc), w, v);
      base += total;
      __syncthreads();  // wsum is rewritten by the next chunk; U by the next follower
    }
  }
}

// ---- out_off = exclusive scan over the followers of (emits ? count : 0), as i64
__device__ __forceinline__ int emit_n(const FollowerDev& d, int64_t i) {
  return (d.emit_all || d.changed[i]) ? d.count[i] : 0;
}

__global__ __launch_bounds__(256) void follower_scan_sums_kernel(FollowerDev d) {
  __shared__ int64_t ws[4];
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * FOL_SCAN_ITEMS;
  int64_t s = 0;
  for (int k = 0; k < FOL_SCAN_ITEMS; ++k)
    if (i0 + k < d.F) s += emit_n(d, i0 + k);
  s = wave_sum_i64(s);
  if ((threadIdx.x & 63) == 0) ws[threadIdx.x >> 6] = s;
  __syncthreads();
  if (threadIdx.x == 0) d.scan_sums[blockIdx.x] = ws[0] + ws[1] + ws[2] + ws[3];
}

// one block: the block sums to their exclusive prefixes, in place
__global__ __launch_bounds__(256) void follower_scan_top_kernel(int64_t* sums, int nb) {
  __shared__ int64_t part[256];
  const int t = threadIdx.x, per = (nb + 255) / 256;
  const int lo = min(nb, t * per), hi = min(nb, lo + per);
  int64_t s = 0;
  for (int i = lo; i < hi; ++i) s += sums[i];
  part[t] = s;
  __syncthreads();
  if (t == 0) {
    int64_t run = 0;
    for (int q = 0; q < 256; ++q) {
      const int64_t v = part[q];
      part[q] = run;
      run += v;
    }
  }
  __syncthreads();
  int64_t run = part[t];
  for (int i = lo; i < hi; ++i) {
    const int64_t v = sums[i];
    sums[i] = run;
    run += v;
  }
}

__global__ __launch_bounds__(256) void follower_scan_apply_kernel(FollowerDev d) {
  __shared__ int64_t ws[4];
  const int wv = threadIdx.x >> 6;
  const int64_t i0 = ((int64_t)blockIdx.x * 256 + threadIdx.x) * FOL_SCAN_ITEMS;
  int v[FOL_SCAN_ITEMS];
  int64_t s = 0;
  for (int k = 0; k < FOL_SCAN_ITEMS; ++k) {
    v[k] = i0 + k < d.F ? emit_n(d, i0 + k) : 0;
    s += v[k];
  }
  const int64_t incl = wave_incl_sum_i64(s);
  if ((threadIdx.x & 63) == 63) ws[wv] = incl;
  __syncthreads();
  int64_t run = d.scan_sums[blockIdx.x] + (incl - s);
  for (int q = 0; q < wv; ++q) run += ws[q];
  for (int k = 0; k < FOL_SCAN_ITEMS; ++k) {
    const int64_t i = i0 + k;
    if (i < d.F) {
      d.fout_off[i] = run;
      run += v[k];
      if (i == d.F - 1) d.fout_off[d.F] = run;
    }
  }
}

hipError_t launch_follower_union(const FollowerDev& d, const FollowerRoute& r, hipStream_t st) {
  (void)hipGetLastError();
  if (r.grid > 0) {
    if (r.path == 0)
      hipLaunchKernelGGL(follower_union_wave_kernel, dim3((unsigned)r.grid), dim3(256), 0, st, d);
    else
      hipLaunchKernelGGL(follower_union_block_kernel, dim3((unsigned)r.grid), dim3(256), 0, st, d);
  }
  return hipGetLastError();
}

hipError_t launch_follower_scan(const FollowerDev& d, hipStream_t st) {
  (void)hipGetLastError();
  if (d.F > 0) {
    const int per = 256 * FOL_SCAN_ITEMS, nb = (int)(((int64_t)d.F + per - 1) / per);
    hipLaunchKernelGGL(follower_scan_sums_kernel, dim3((unsigned)nb), dim3(256), 0, st, d);
    hipLaunchKernelGGL(follower_scan_top_kernel, dim3(1), dim3(256), 0, st, d.scan_sums, nb);
    hipLaunchKernelGGL(follower_scan_apply_kernel, dim3((unsigned)nb), dim3(256), 0, st, d);
  }
  return hipGetLastError();
}

hipError_t launch_follower_emit(const FollowerDev& d, const FollowerRoute& r, hipStream_t st) {
  (void)hipGetLastError();
  if (r.grid > 0) {
    if (r.path == 0)
      hipLaunchKernelGGL(follower_emit_wave_kernel, dim3((unsigned)r.grid), dim3(256), 0, st, d);
    else
      hipLaunchKernelGGL(follower_emit_block_kernel, dim3((unsigned)r.grid), dim3(256), 0, st, d);
  }
  return hipGetLastError();
}

}  // namespace kad

// ------------------------------------------------------ host half: kad_follower_*
#include "kad_arena.h"

using namespace kad;

extern "C" {

// ------------------------------------------------------ follower scheduling
// Every offset array monotone from 0, every id in [0, n_ids), every leader index in [-1, n_leaders): all of
// it on the host, before anything is copied or launched. C = the snapshot's clusters; W = the resident
// units a resident-mode batch reads (ignored in explicit mode).
static int validate_follower(const kad_follower_batch* b, const kad_follower_view* out, int C, int64_t W,
                             std::string* err) {
  auto bad = [&](const char* m) {
    *err = m;
    return KAD_EINVAL;
  };
  const int64_t n_ids = b->n_ids, L = b->n_leaders, F = b->n_followers;
  if (n_ids < C || n_ids > FOL_MAX_IDS) return bad("n_ids must lie in [the snapshot's clusters, 131072]");
  if (L < 0 || F < 0 || b->out_capacity < 0) return bad("negative count or capacity");
  if (b->flags & ~(uint32_t)KAD_FOL_EMIT_ALL) return bad("unknown flag");
  const bool resident = b->lead_off == nullptr;
  if (!resident) {
    if (csr_bad(b->lead_off, b->lead_cluster, L, 0, n_ids)) return bad("lead_off / lead_cluster malformed or id out of range");
  } else {
    if (L < W) return bad("resident mode: n_leaders is less than the resident batch's units");
    if (b->sched_off && csr_bad(b->sched_off, b->sched_cluster, W, 0, n_ids))
      return bad("sched_off / sched_cluster malformed or id out of range");
  }
  if (b->keep_off && csr_bad(b->keep_off, b->keep_cluster, L, 0, n_ids))
    return bad("keep_off / keep_cluster malformed or id out of range");
  if (csr_bad(b->fol_off, b->fol_leader, F, -1, L)) return bad("fol_off / fol_leader malformed or leader index out of range");
  if (csr_bad(b->cur_off, b->cur_cluster, F, 0, n_ids)) return bad("cur_off / cur_cluster malformed or id out of range");
  if (F && !b->cur_has) return bad("cur_has missing");
  {
    const int32_t* co = b->cur_off;
    const uint8_t* ch = b->cur_has;
    if (first_bad(F, [&](int64_t i) { return !ch[i] && co[i + 1] > co[i]; }) >= 0)
      return bad("cur_has = 0 with a non-empty cur range: a placement entry that does not exist holds no clusters");
  }
  if (!out || !out->out_off || (F && (!out->changed || !out->count)) || (b->out_capacity && !out->out_cluster))
    return bad("output view missing");
  return KAD_OK;
}

static int follower_union_locked(kad_ctx* c, const kad_follower_batch* b, const kad_follower_view* out) {
  if (!c->have_snapshot) return fail(c, KAD_ESTATE, "a snapshot must be uploaded first");
  const bool resident = b->lead_off == nullptr;
  if (resident && c->group_member)
    return fail(c, KAD_EUNSUPPORTED, "resident mode on a kad_group member: a follower's leaders may live in other shards");
  if (resident && (!c->have_batch || !c->ran)) return fail(c, KAD_ESTATE, "nothing has been scheduled");
  const int64_t W = resident ? c->unit_n : 0;
  std::string err;
  if (int r = validate_follower(b, out, c->sd.C, W, &err)) return fail(c, r, err);
  const int F = b->n_followers, L = b->n_leaders;
  out->out_off[0] = 0;
  if (F == 0) return KAD_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const FollowerRoute route = route_follower(b->n_ids, F, n_cus());
  // one buffer: the inputs, then changed / count / out_off / the scan's block sums / out_cluster
  const size_t f = (size_t)F, l = (size_t)L, n_lead = resident ? 0 : (size_t)b->lead_off[L],
               n_sched = resident && b->sched_off ? (size_t)b->sched_off[W] : 0, n_keep = b->keep_off ? (size_t)b->keep_off[L] : 0;
  FollowerDev fd{};
  fd.n_ids = b->n_ids;
  fd.nw = route.words;
  fd.F = F;
  fd.n_leaders = L;
  fd.resident = resident ? 1 : 0;
  fd.W = (int)W;
  if (resident) {
    fd.out_off = c->bd.out_off;
    fd.cur_off = c->bd.cur_off;
    fd.cur_id = c->bd.cur_id;
    fd.res_status = c->d_status;
    fd.res_count = c->d_count;
    fd.res_cluster = c->d_cluster;
    fd.slot_lo = c->slot_lo;
  }
  fd.emit_all = (b->flags & KAD_FOL_EMIT_ALL) ? 1 : 0;
  fd.capacity = b->out_capacity;
  // an offset array the caller left out is absent; its id list keeps an (empty) slot
  Arena a;
  if (resident)
    a.absent(fd.lead_off);
  else
    a.in(fd.lead_off, b->lead_off, l + 1);
  a.in(fd.lead_cluster, b->lead_cluster, n_lead);
  if (resident && b->sched_off)
    a.in(fd.sched_off, b->sched_off, (size_t)W + 1);
  else
    a.absent(fd.sched_off);
  a.in(fd.sched_cluster, b->sched_cluster, n_sched);
  if (b->keep_off)
    a.in(fd.keep_off, b->keep_off, l + 1);
  else
    a.absent(fd.keep_off);
  a.in(fd.keep_cluster, b->keep_cluster, n_keep);
  a.in(fd.fol_off, b->fol_off, f + 1);
  a.in(fd.fol_leader, b->fol_leader, (size_t)b->fol_off[F]);
  a.in(fd.fcur_off, b->cur_off, f + 1);
  a.in(fd.fcur_cluster, b->cur_cluster, (size_t)b->cur_off[F]);
  a.in(fd.fcur_has, b->cur_has, f);
  a.out(fd.changed, out->changed, f);
  a.out(fd.count, out->count, f);
  a.out(fd.fout_off, out->out_off, f + 1);
  a.out(fd.scan_sums, (f + 256 * FOL_SCAN_ITEMS - 1) / (256 * FOL_SCAN_ITEMS));  // the scan's block sums
  a.out(fd.out_cluster, (size_t)b->out_capacity);  // copied below, once out_off[F] is known
  Stage& stg = c->stage[STG_FOLLOWER];
  if (int r = a.commit(c, stg.buf)) return r;
  HIPCHK(c, hipEventRecord(stg.ev[0], c->stream));
  HIPCHK(c, launch_follower_union(fd, route, c->stream));
  HIPCHK(c, hipEventRecord(stg.ev[1], c->stream));
  HIPCHK(c, launch_follower_scan(fd, c->stream));
  HIPCHK(c, launch_follower_emit(fd, route, c->stream));
  HIPCHK(c, hipEventRecord(stg.ev[2], c->stream));
  stage_ran(stg, route);
  if (int r = a.fetch(c)) return r;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int64_t n_out = out->out_off[F];
  if (n_out > b->out_capacity)
    return fail(c, KAD_ENOSPC, "out_capacity " + std::to_string(b->out_capacity) + " < " + std::to_string(n_out) +
                                   " emitted ids: retry with out_off[n_followers] slots");
  if (n_out) {
    HIPCHK(c, hipMemcpyAsync(out->out_cluster, fd.out_cluster, sizeof *fd.out_cluster * (size_t)n_out, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipStreamSynchronize(c->stream));
  }
  return KAD_OK;
}

int kad_follower_check(const kad_follower_batch* b, const kad_follower_view* out, int32_t n_clusters, int32_t n_units) {
  return check_guarded([&]() -> int {
    if (!b || n_clusters < 0) return KAD_EINVAL;
    if (!b->lead_off && n_units < 0) return KAD_ESTATE;
    std::string err;
    return validate_follower(b, out, n_clusters, b->lead_off ? 0 : n_units, &err);
  });
}

int kad_follower_union(kad_ctx* c, const kad_follower_batch* b, const kad_follower_view* out) {
  return entry(c, b != nullptr, [&]() -> int {
    return follower_union_locked(c, b, out);
  });
}

int kad_follower_timing(kad_ctx* c, float ms[2]) { return stage_timing(c, STG_FOLLOWER, 2, ms, "no kad_follower_union ran"); }

int kad_follower_route_eval(int32_t n_ids, int32_t n_followers, int32_t n_cu, int32_t* out) {
  if (!out || n_ids < 0 || n_ids > FOL_MAX_IDS || n_followers < 0 || n_cu < 1) return KAD_EINVAL;
  return route_record<KAD_FOL_ROUTE_FIELDS>(out, route_follower(n_ids, n_followers, n_cu));
}

int kad_follower_last_route(kad_ctx* c, int32_t* out) { return stage_last_route(c, STG_FOLLOWER, out, "no kad_follower_union ran"); }

}  // extern "C"
