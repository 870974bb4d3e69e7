// Cluster status (kad_cluster_resources): the resources of every member cluster from its nodes and pods.
//
// The federated-cluster controller re-derives, every collection interval and per ready member cluster
// (updateClusterResources, pkg/controllers/federatedcluster/clusterstatus.go:162-202), Allocatable as the sum of
// the schedulable nodes' allocatable lists, Available as Allocatable minus the requests of every non-terminal
// pod, and the number of schedulable nodes (aggregateResources, util.go:178-214). On the device that is a
// segmented integer reduction in two passes, the second of which needs the first one's complete result (a
// request counts only for a name some schedulable node of the cluster lists):
//
//   cstat_node_kernel<W>   blocks below n_long: one listed long cluster per 256-thread block; the other blocks:
//                          a wave is 64 / W lane groups, each group takes one cluster at a time. The lanes of
//                          a team stride over the cluster's nodes; a lane walks its schedulable node's entries
//                          and adds them to the team's per-resource sums in LDS (R x 8 B, integer LDS atomics),
//                          ORs the presence bits and counts the node. Then the team stores alloc, avail =
//                          alloc, has and sched_nodes of the cluster.
//   cstat_pod_kernel<W>    the same two paths over pods: a lane walks its non-terminal pod's entries, which
//                          ascend by (resource, kind), as runs of one resource — sum of the containers, max with
//                          every init container, plus the overhead — and adds the request to the team's sums
//                          where the cluster has the name. Group path: avail = alloc - sum. Long path: blocks
//                          below n_chunks take CS_POD_CHUNK pods of a long cluster each and store partial sums.
//   cstat_combine_kernel   one thread per (long cluster, resource): avail = alloc - the sum of its chunks.
//
// Integer adds commute and the host bounds every sum by 2^62, so the results are exact whatever the order.
// No global atomics, no state that kad_schedule reads.
#include "kad_cstat.h"
#include "kad_wave.h"

namespace kad {

// the lanes of a team meet: a lane group lies inside one wave, whose LDS operations execute in order
template <int T>
__device__ __forceinline__ void team_sync() {
  if (T == 256)
    __syncthreads();
  else
    wave_sync();
}

// one cluster's node pass by a team of T lanes (tl: this lane's index in it); every lane of the team calls it,
// live or not, so that the team's meetings are uniform
template <int T>
__device__ __forceinline__ void node_team(const CstatDev& d, int k, bool live, unsigned long long* slab, int tl) {
  const int R = d.R;
  if (live)
    for (int r = tl; r < R + 2; r += T) slab[r] = 0;
  team_sync<T>();
  if (live) {
    const int64_t lo = d.cl_node_off[k], hi = d.cl_node_off[k + 1];
    unsigned long long has = 0, cnt = 0;
    // consecutive lanes take consecutive nodes, whose entries are adjacent
    for (int64_t n = lo + tl; n < hi; n += T) {
      if (!(d.node_flags[n] & CS_NODE_SCHEDULABLE)) continue;  // isNodeSchedulable (util.go:114-132), on the host
      ++cnt;
      const int64_t e1 = d.node_ent_off[n + 1];
      for (int64_t e = d.node_ent_off[n]; e < e1; ++e) {
        const int r = d.nent_res[e];
        const unsigned long long v = (unsigned long long)d.nent_val[e];
        has |= 1ull << r;  // present as soon as one schedulable node lists it, even with 0 (addResources)
        if (v) atomicAdd(&slab[r], v);
      }
    }
    if (has) atomicOr(&slab[R], has);
    if (cnt) atomicAdd(&slab[R + 1], cnt);
  }
  team_sync<T>();
  if (live) {
    const unsigned long long has = slab[R];
    const int64_t row = (int64_t)k * R;
    for (int r = tl; r < R; r += T) {
      const int64_t v = (has >> r) & 1 ? (int64_t)slab[r] : 0;
      d.alloc[row + r] = v;
      d.avail[row + r] = v;  // available starts as a copy of allocatable (util.go:194-197)
    }
    if (tl == 0) {
      d.has[k] = has;
      d.sched_nodes[k] = (int64_t)slab[R + 1];
    }
  }
  team_sync<T>();  // the slab serves the team's next cluster
}

// getPodResourceRequests for one resource of one pod (util.go:155-173) under values >= 0: the containers' sum,
// max with each init container (an absent name starts at 0), plus the overhead
__device__ __forceinline__ void flush_run(unsigned long long* slab, unsigned long long has, int res,
                                          unsigned long long csum, unsigned long long imax, unsigned long long ovh) {
  if (res < 0 || !((has >> res) & 1)) return;  // a name no schedulable node offers is ignored (util.go:206)
  const unsigned long long req = (csum > imax ? csum : imax) + ovh;
  if (req) atomicAdd(&slab[res], req);
}

// pods [lo, hi) of cluster k summed into the team's slab (which the caller reads after the closing meeting)
template <int T>
__device__ __forceinline__ void pod_team(const CstatDev& d, int k, bool live, int64_t lo, int64_t hi,
                                         unsigned long long* slab, int tl) {
  const int R = d.R;
  if (live)
    for (int r = tl; r < R; r += T) slab[r] = 0;
  team_sync<T>();
  if (live) {
    const unsigned long long has = d.has[k];
    for (int64_t p = lo + tl; p < hi; p += T) {
      if (d.pod_flags[p] & CS_POD_TERMINAL) continue;  // Succeeded / Failed (util.go:200)
      const int64_t e1 = d.pod_ent_off[p + 1];
      int cur = -1;
      unsigned long long csum = 0, imax = 0, ovh = 0;
      for (int64_t e = d.pod_ent_off[p]; e < e1; ++e) {
        const int r = d.pent_res[e], kind = d.pent_kind[e];
        const unsigned long long v = (unsigned long long)d.pent_val[e];
        if (r != cur) {
          flush_run(slab, has, cur, csum, imax, ovh);
          cur = r;
          csum = imax = ovh = 0;
        }
        if (kind == 0)
          csum += v;
        else if (kind == 1)
          imax = v > imax ? v : imax;
        else
          ovh += v;
      }
      flush_run(slab, has, cur, csum, imax, ovh);
    }
  }
  team_sync<T>();
}

template <int W>
__global__ __launch_bounds__(256) void cstat_node_kernel(CstatDev d) {
  constexpr int GPB = 256 / W;  // groups a block
  __shared__ unsigned long long s_slab[GPB * CS_SLAB];
  if ((int)blockIdx.x < d.n_long) {  // ---- long path: one listed cluster per block
    node_team<256>(d, d.long_list[blockIdx.x], true, s_slab, (int)threadIdx.x);
    return;
  }
  // ---- group path: the loop is uniform over the block (groups past K or on a long cluster idle)
  const int g = (int)threadIdx.x / W, gl = (int)threadIdx.x & (W - 1);
  const int64_t stride = (int64_t)(gridDim.x - d.n_long) * GPB;
  for (int64_t base = (int64_t)(blockIdx.x - d.n_long) * GPB; base < d.K; base += stride) {
    const int64_t k64 = base + g;
    const int k = k64 < d.K ? (int)k64 : 0;
    const bool live = k64 < d.K && !d.cl_long[k];
    node_team<W>(d, k, live, s_slab + g * CS_SLAB, gl);
  }
}

template <int W>
__global__ __launch_bounds__(256) void cstat_pod_kernel(CstatDev d) {
  constexpr int GPB = 256 / W;
  __shared__ unsigned long long s_slab[GPB * CS_SLAB];
  const int R = d.R;
  if ((int)blockIdx.x < d.n_chunks) {  // ---- long path: one chunk of a long cluster's pods per block
    const int c = (int)blockIdx.x, t = (int)threadIdx.x;
    pod_team<256>(d, d.chunk_cluster[c], true, d.chunk_pod_lo[c], d.chunk_pod_hi[c], s_slab, t);
    for (int r = t; r < R; r += 256) d.partial[(int64_t)c * R + r] = s_slab[r];
    return;
  }
  const int g = (int)threadIdx.x / W, gl = (int)threadIdx.x & (W - 1);
  unsigned long long* slab = s_slab + g * CS_SLAB;
  const int64_t stride = (int64_t)(gridDim.x - d.n_chunks) * GPB;
  for (int64_t base = (int64_t)(blockIdx.x - d.n_chunks) * GPB; base < d.K; base += stride) {
    const int64_t k64 = base + g;
    const int k = k64 < d.K ? (int)k64 : 0;
    const bool live = k64 < d.K && !d.cl_long[k];
    pod_team<W>(d, k, live, live ? d.cl_pod_off[k] : 0, live ? d.cl_pod_off[k + 1] : 0, slab, gl);
    if (live) {
      const unsigned long long has = d.has[k];
      const int64_t row = (int64_t)k * R;
      for (int r = gl; r < R; r += W)
        if ((has >> r) & 1) d.avail[row + r] = wsub(d.alloc[row + r], (int64_t)slab[r]);  // may go negative
    }
    team_sync<W>();  // the slab serves the group's next cluster
  }
}

__global__ __launch_bounds__(256) void cstat_combine_kernel(CstatDev d) {
  const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (i >= (int64_t)d.n_long * d.R) return;
  const int j = (int)(i / d.R), r = (int)(i % d.R);
  const int k = d.long_list[j];
  if (!((d.has[k] >> r) & 1)) return;
  unsigned long long sum = 0;
  for (int c = d.long_chunk_off[j]; c < d.long_chunk_off[j + 1]; ++c) sum += d.partial[(int64_t)c * d.R + r];
  const int64_t at = (int64_t)k * d.R + r;
  d.avail[at] = wsub(d.alloc[at], (int64_t)sum);
}

hipError_t launch_cstat_nodes(const CstatDev& d, const CstatRoute& r, hipStream_t st) {
  (void)hipGetLastError();
  const unsigned grid = (unsigned)(r.node_grid + r.long_grid);
  if (grid > 0)
    with_width<CS_MIN_WIDTH>(r.node_width, [&](auto W) {
      hipLaunchKernelGGL(cstat_node_kernel<decltype(W)::value>, dim3(grid), dim3(256), 0, st, d);
    });
  return hipGetLastError();
}

hipError_t launch_cstat_pods(const CstatDev& d, const CstatRoute& r, hipStream_t st) {
  (void)hipGetLastError();
  const unsigned grid = (unsigned)(r.pod_grid + r.chunk_grid);
  if (grid > 0)
    with_width<CS_MIN_WIDTH>(r.pod_width, [&](auto W) {
      hipLaunchKernelGGL(cstat_pod_kernel<decltype(W)::value>, dim3(grid), dim3(256), 0, st, d);
    });
  const int64_t n = (int64_t)d.n_long * d.R;
  if (n > 0) hipLaunchKernelGGL(cstat_combine_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, d);
  return hipGetLastError();
}

}  // namespace kad

// ------------------------------------------------------ host half: kad_cstat_* / kad_cluster_resources
#include "kad_arena.h"

using namespace kad;

namespace {

// what the validation leaves for the launch: the long path's lists and the short clusters' sizes
struct CstatPlan {
  std::vector<uint8_t> cl_long;
  std::vector<int32_t> long_list, long_chunk_off, chunk_cluster;
  std::vector<int64_t> chunk_lo, chunk_hi;
  int64_t short_nodes = 0, short_pods = 0;
};

// min and max of n values (0 and 0 for none)
void min_max(const int64_t* v, int64_t n, int64_t& mn, int64_t& mx) {
  mn = mx = 0;
  for (int64_t i = 0; i < n; ++i) {
    mn = v[i] < mn ? v[i] : mn;
    mx = v[i] > mx ? v[i] : mx;
  }
}

// max value x max entries of one cluster <= 2^62: no sum of a cluster's entries can wrap
bool sum_may_wrap(int64_t vmax, int64_t emax) {
  return (unsigned __int128)(uint64_t)vmax * (unsigned __int128)(uint64_t)emax > ((unsigned __int128)1 << 62);
}

}  // namespace

extern "C" {

// Every offset array monotone from 0 and ending at its count, every resource id below R, every kind known, a
// pod's entries ascending by (resource, kind), every flag known and every value inside the domain: all of it on
// the host, before anything is copied or launched. With a plan (kad_cluster_resources) the same pass leaves
// the clusters of the long path (more than long_min entries) and their pod chunks.
static int validate_cstat(const kad_cstat_batch* b, const kad_cstat_view* out, int long_min, CstatPlan* plan,
                          std::string* err) {
  auto bad = [&](const char* m) {
    *err = m;
    return KAD_EINVAL;
  };
  const int64_t K = b->n_clusters, R = b->n_res, N = b->n_nodes, P = b->n_pods, EN = b->n_node_ents, EP = b->n_pod_ents;
  if (R < 1 || R > CS_MAX_RES) return bad("n_res must lie in [1, 64]");
  if (K < 0 || N < 0 || P < 0 || EN < 0 || EP < 0) return bad("negative count");
  if (!b->cl_node_off || !b->node_ent_off || !b->cl_pod_off || !b->pod_ent_off) return bad("offset array missing");
  if ((N && !b->node_flags) || (EN && (!b->nent_res || !b->nent_val)) || (P && !b->pod_flags) ||
      (EP && (!b->pent_res || !b->pent_kind || !b->pent_val)))
    return bad("input array missing");
  const int64_t *cn = b->cl_node_off, *ne = b->node_ent_off, *cp = b->cl_pod_off, *pe = b->pod_ent_off;
  if (off_bad(cn, K) || cn[K] != N) return bad("cl_node_off not monotone from 0 to n_nodes");
  if (off_bad(ne, N) || ne[N] != EN) return bad("node_ent_off not monotone from 0 to n_node_ents");
  if (off_bad(cp, K) || cp[K] != P) return bad("cl_pod_off not monotone from 0 to n_pods");
  if (off_bad(pe, P) || pe[P] != EP) return bad("pod_ent_off not monotone from 0 to n_pod_ents");
  {
    const uint8_t *nf = b->node_flags, *pf = b->pod_flags, *nr = b->nent_res, *pr = b->pent_res, *pk = b->pent_kind;
    if (first_bad(N, [&](int64_t i) { return (nf[i] & ~KAD_CS_NODE_SCHEDULABLE) != 0; }) >= 0)
      return bad("node_flags: unknown flag");
    if (first_bad(P, [&](int64_t i) { return (pf[i] & ~KAD_CS_POD_TERMINAL) != 0; }) >= 0)
      return bad("pod_flags: unknown flag");
    if (first_bad(EN, [&](int64_t i) { return nr[i] >= R; }) >= 0) return bad("nent_res out of range");
    if (first_bad(EP, [&](int64_t i) { return pr[i] >= R; }) >= 0) return bad("pent_res out of range");
    if (first_bad(EP, [&](int64_t i) { return pk[i] > 2; }) >= 0) return bad("pent_kind: unknown kind");
    if (first_bad(P, [&](int64_t i) {
          for (int64_t e = pe[i] + 1; e < pe[i + 1]; ++e)
            if (pr[e] * 4 + pk[e] < pr[e - 1] * 4 + pk[e - 1]) return true;
          return false;
        }) >= 0)
      return bad("a pod's entries do not ascend by (resource, kind)");
  }
  {
    int64_t mn, nmax, pmax;
    min_max(b->nent_val, EN, mn, nmax);
    if (mn < 0) return bad("nent_val: negative value");
    min_max(b->pent_val, EP, mn, pmax);
    if (mn < 0) return bad("pent_val: negative value");
    int64_t en_max = 0, ep_max = 0;
    for (int64_t k = 0; k < K; ++k) {
      const int64_t a = ne[cn[k + 1]] - ne[cn[k]], p = pe[cp[k + 1]] - pe[cp[k]];
      en_max = a > en_max ? a : en_max;
      ep_max = p > ep_max ? p : ep_max;
    }
    if (sum_may_wrap(nmax, en_max)) return bad("node entries: max value x max entries of one cluster exceeds 2^62");
    if (sum_may_wrap(pmax, ep_max)) return bad("pod entries: max value x max entries of one cluster exceeds 2^62");
  }
  if (!out || (K && (!out->alloc || !out->avail || !out->has || !out->sched_nodes))) return bad("output view missing");
  if (plan) {
    plan->cl_long.assign((size_t)K, 0);
    plan->long_chunk_off.assign(1, 0);
    for (int64_t k = 0; k < K; ++k) {
      const int64_t ents = (ne[cn[k + 1]] - ne[cn[k]]) + (pe[cp[k + 1]] - pe[cp[k]]);
      if (ents <= long_min) {
        plan->short_nodes += cn[k + 1] - cn[k];
        plan->short_pods += cp[k + 1] - cp[k];
        continue;
      }
      plan->cl_long[(size_t)k] = 1;
      plan->long_list.push_back((int32_t)k);
      for (int64_t lo = cp[k]; lo < cp[k + 1]; lo += CS_POD_CHUNK) {
        plan->chunk_cluster.push_back((int32_t)k);
        plan->chunk_lo.push_back(lo);
        plan->chunk_hi.push_back(lo + CS_POD_CHUNK < cp[k + 1] ? lo + CS_POD_CHUNK : cp[k + 1]);
      }
      if (plan->chunk_cluster.size() > (size_t)INT32_MAX / CS_MAX_RES) return bad("too many pods on the long path");
      plan->long_chunk_off.push_back((int32_t)plan->chunk_cluster.size());
    }
  }
  return KAD_OK;
}

static int cluster_resources_locked(kad_ctx* c, const kad_cstat_batch* b, const kad_cstat_view* out) {
  Stage& stg = c->stage[STG_CSTAT];
  const int long_min = stg.force.long_min_or(CS_LONG_MIN);
  std::string err;
  CstatPlan plan;
  if (int r = validate_cstat(b, out, long_min, &plan, &err)) return fail(c, r, err);
  const int K = b->n_clusters, R = b->n_res;
  if (K == 0) return KAD_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const int n_long = (int)plan.long_list.size(), n_chunks = (int)plan.chunk_cluster.size();
  CstatRoute route = route_cstat(K, n_long, plan.short_nodes, plan.short_pods, n_chunks, n_cus());
  group_force_apply(stg.force, n_long < K, K, n_cus(), route.node_width, route.node_grid);
  group_force_apply(stg.force, n_long < K, K, n_cus(), route.pod_width, route.pod_grid);
  route.long_min = long_min;
  // one buffer: the inputs, then the partial sums and the outputs
  const size_t k = (size_t)K, n = (size_t)b->n_nodes, p = (size_t)b->n_pods, en = (size_t)b->n_node_ents,
               ep = (size_t)b->n_pod_ents, nl = (size_t)n_long, nc = (size_t)n_chunks, kr = k * (size_t)R;
  CstatDev d{};
  d.K = K;
  d.R = R;
  d.n_long = n_long;
  d.n_chunks = n_chunks;
  Arena a;
  a.in(d.cl_node_off, b->cl_node_off, k + 1);
  a.in(d.node_flags, b->node_flags, n);
  a.in(d.node_ent_off, b->node_ent_off, n + 1);
  a.in(d.nent_res, b->nent_res, en);
  a.in(d.nent_val, b->nent_val, en);
  a.in(d.cl_pod_off, b->cl_pod_off, k + 1);
  a.in(d.pod_flags, b->pod_flags, p);
  a.in(d.pod_ent_off, b->pod_ent_off, p + 1);
  a.in(d.pent_res, b->pent_res, ep);
  a.in(d.pent_kind, b->pent_kind, ep);
  a.in(d.pent_val, b->pent_val, ep);
  a.in(d.cl_long, plan.cl_long.data(), k);
  a.in(d.long_list, plan.long_list.data(), nl);
  a.in(d.long_chunk_off, plan.long_chunk_off.data(), nl + 1);
  a.in(d.chunk_cluster, plan.chunk_cluster.data(), nc);
  a.in(d.chunk_pod_lo, plan.chunk_lo.data(), nc);
  a.in(d.chunk_pod_hi, plan.chunk_hi.data(), nc);
  a.out(d.partial, nc * (size_t)R);
  a.out(d.alloc, out->alloc, kr);
  a.out(d.avail, out->avail, kr);
  a.out(d.has, out->has, k);
  a.out(d.sched_nodes, out->sched_nodes, k);
  if (int r = a.commit(c, stg.buf)) return r;
  HIPCHK(c, hipEventRecord(stg.ev[0], c->stream));
  HIPCHK(c, launch_cstat_nodes(d, route, c->stream));
  HIPCHK(c, hipEventRecord(stg.ev[1], c->stream));
  HIPCHK(c, launch_cstat_pods(d, route, c->stream));
  HIPCHK(c, hipEventRecord(stg.ev[2], c->stream));
  stage_ran(stg, route);
  if (int r = a.fetch(c)) return r;
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return KAD_OK;
}

int kad_cstat_check(const kad_cstat_batch* b, const kad_cstat_view* out) {
  return check_guarded([&]() -> int {
    if (!b) return KAD_EINVAL;
    std::string err;
    return validate_cstat(b, out, CS_LONG_MIN, nullptr, &err);
  });
}

int kad_cluster_resources(kad_ctx* c, const kad_cstat_batch* b, const kad_cstat_view* out) {
  return entry(c, b != nullptr, [&]() -> int {
    return cluster_resources_locked(c, b, out);
  });
}

int kad_cstat_timing(kad_ctx* c, float ms[2]) { return stage_timing(c, STG_CSTAT, 2, ms, "no kad_cluster_resources ran"); }

int kad_cstat_route_eval(int32_t n_clusters, int32_t n_long, int64_t short_nodes, int64_t short_pods, int32_t n_chunks,
                         int32_t n_cu, int32_t* out) {
  if (!out || n_clusters < 0 || n_long < 0 || n_long > n_clusters || short_nodes < 0 || short_pods < 0 || n_chunks < 0 ||
      n_cu < 1)
    return KAD_EINVAL;
  return route_record<KAD_CS_ROUTE_FIELDS>(out, route_cstat(n_clusters, n_long, short_nodes, short_pods, n_chunks, n_cu));
}

int kad_cstat_last_route(kad_ctx* c, int32_t* out) { return stage_last_route(c, STG_CSTAT, out, "no kad_cluster_resources ran"); }

int kad_cstat_debug_route(kad_ctx* c, int32_t force_width, int32_t force_long_min) {
  return stage_debug_route(c, STG_CSTAT, group_width_ok(force_width, CS_MIN_WIDTH), GroupForce{force_width, force_long_min, 0});
}

}  // extern "C"
