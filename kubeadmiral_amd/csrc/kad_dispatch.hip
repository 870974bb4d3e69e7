// Sync dispatch planning (kad_dispatch_plan): per federated object and joined cluster, the operation the sync
// controller starts and the propagation status it records before anything is dispatched.
//
// syncToClusters (pkg/controllers/sync/controller.go:425-544) computes the object's placement — the union of every
// controller's cluster names, cut down to the joined clusters and to the federated namespace's placement
// (sync/placement.go:45-116) — and walks every joined cluster. Per object that is a set union and intersection
// over small-integer cluster ids, a table lookup per (object, cluster) and an ascending, compacted listing; the
// sets are bitmaps over the cluster ids, kept in LDS only:
//
//   dispatch_wave_kernel   C <= 16384: one object per wave at a time, three bitmaps per wave (selected, namespace,
//                          observed) in dynamic LDS, zeroed once; after each object the wave walks the same id
//                          lists again and clears just the words it set. The emit walks selected | observed a word
//                          per lane: di_decide (kad_dispatch.h) per set bit, a wave prefix sum of the emitted
//                          entries' popcounts for the output position, so that an object's entries come out
//                          ascending and compacted without global atomics. An observation's flags sit at its
//                          cluster's rank in the observed bitmap, because the list is ascending.
//
// Nothing here writes state that kad_schedule reads.
#include "kad_device.h"
#include "kad_dispatch.h"
#include "kad_wave.h"

namespace kad {

namespace {

// the lanes of a wave walk one id list, one id per lane and step; ids outside [0, C) (the -1 of a name that is
// not a joined cluster; the host rejects every other) touch nothing
__device__ __forceinline__ void di_set(const int32_t* p, int n, int t, uint32_t* bm, int C) {
  for (int k = t; k < n; k += WAVE) {
    const int id = p[k];
    if ((uint32_t)id < (uint32_t)C) atomicOr(&bm[id >> 5], 1u << (id & 31));
  }
}
__device__ __forceinline__ void di_clear(const int32_t* p, int n, int t, uint32_t* bm, int C) {
  for (int k = t; k < n; k += WAVE) {
    const int id = p[k];
    if ((uint32_t)id < (uint32_t)C) bm[id >> 5] = 0;
  }
}

// bit b of word w: cluster w * 32 + b, selected per `sel`, observed per `obs`, whose first observation is `ob_at`
__device__ __forceinline__ DiDecision di_bit(const DispatchDev& d, int w, int b, uint32_t sel, uint32_t obs, int ob_at,
                                             uint8_t of) {
  const uint32_t m = 1u << b;
  const uint8_t ob = (obs & m) ? d.ob_flags[ob_at + __builtin_popcount(obs & (m - 1u))] : (uint8_t)0;
  return di_decide(d.cluster_flags[w * 32 + b], (sel & m) != 0, ob, of);
}

}  // namespace

__global__ __launch_bounds__(256) void dispatch_wave_kernel(DispatchDev d) {
  extern __shared__ uint32_t di_bm[];  // [4 waves][DI_BITMAPS][nw]
  const int wv = threadIdx.x >> 6, t = lane_id_h();
  uint32_t* S = di_bm + (size_t)wv * DI_BITMAPS * d.nw;
  uint32_t* N = S + d.nw;
  uint32_t* B = N + d.nw;
  for (int k = t; k < DI_BITMAPS * d.nw; k += WAVE) S[k] = 0;  // the three bitmaps, once
  wave_sync();
  const int stride = gridDim.x * 4;
  for (int o0 = blockIdx.x * 4 + wv; o0 < d.O; o0 += stride) {
    const int o = __builtin_amdgcn_readfirstlane(o0);
    const uint8_t of = d.obj_flags[o];
    if (of & DI_OBJ_ERROR) {  // ComputePlacementFailed (:437-444): nothing is walked
      if (t == 0) {
        d.count[o] = 0;
        d.n_ops[o] = 0;
        d.n_selected[o] = 0;
        d.obj_result[o] = DI_RES_PLACEMENT_FAILED;
      }
      continue;
    }
    const int ns = d.obj_ns[o];
    const int p0 = d.obj_pl_off[o], pn = ns == DI_NS_UNFEDERATED ? 0 : d.obj_pl_off[o + 1] - p0;
    const int n0 = ns >= 0 ? d.ns_pl_off[ns] : 0, nn = ns >= 0 ? d.ns_pl_off[ns + 1] - n0 : 0;
    const int b0 = d.obj_ob_off[o], bn = d.obj_ob_off[o + 1] - b0;
    di_set(d.pl_cluster + p0, pn, t, S, d.C);
    di_set(d.ns_cluster + n0, nn, t, N, d.C);
    di_set(d.ob_cluster + b0, bn, t, B, d.C);
    wave_sync();
    int64_t base = d.out_off[o];
    const int64_t first = base;
    int ob_at = b0, n_sel = 0, n_ops = 0;
    bool recheck = false;
    for (int w0 = 0; w0 < d.nw; w0 += WAVE) {
      const int w = w0 + t;
      uint32_t sel = 0, obs = 0;
      if (w < d.nw) {
        sel = ns >= 0 ? (S[w] & N[w]) : S[w];
        obs = B[w];
      }
      n_sel += __builtin_popcount(sel);
      const int opc = __builtin_popcount(obs), oincl = wave_incl_sum_i32(opc);
      const int my_ob = ob_at + (oincl - opc);
      uint32_t em = 0;
      for (uint32_t v = sel | obs; v; v &= v - 1) {
        const int b = __ffs(v) - 1;
        const DiDecision x = di_bit(d, w, b, sel, obs, my_ob, of);
        if (x.op != DI_OP_NONE || x.status != DI_ST_NONE) em |= 1u << b;
        n_ops += x.op != DI_OP_NONE;
        recheck |= x.recheck != 0;
      }
      const int pc = __builtin_popcount(em), incl = wave_incl_sum_i32(pc);
      int64_t pos = base + (incl - pc);
      for (uint32_t v = em; v; v &= v - 1) {
        const int b = __ffs(v) - 1;
        const DiDecision x = di_bit(d, w, b, sel, obs, my_ob, of);
        d.out_cluster[pos] = w * 32 + b;
        d.out_op[pos] = x.op;
        d.out_status[pos] = x.status;
        ++pos;
      }
      base += __builtin_amdgcn_readlane(incl, 63);
      ob_at += __builtin_amdgcn_readlane(oincl, 63);
    }
    n_sel = wave_sum_i32(n_sel);
    n_ops = wave_sum_i32(n_ops);
    const bool any_recheck = ballot(recheck) != 0;
    if (t == 0) {
      d.count[o] = (int32_t)(base - first);
      d.n_ops[o] = n_ops;
      d.n_selected[o] = n_sel;
      d.obj_result[o] = any_recheck ? DI_RES_RECHECK : 0;
    }
    wave_sync();
    // only the words this object set
    di_clear(d.pl_cluster + p0, pn, t, S, d.C);
    di_clear(d.ns_cluster + n0, nn, t, N, d.C);
    di_clear(d.ob_cluster + b0, bn, t, B, d.C);
    wave_sync();
  }
}

hipError_t launch_dispatch(const DispatchDev& d, const DispatchRoute& r, hipStream_t st) {
  (void)hipGetLastError();
  if (r.grid > 0)
    hipLaunchKernelGGL(dispatch_wave_kernel, dim3((unsigned)r.grid), dim3((unsigned)r.threads), (size_t)r.lds, st, d);
  return hipGetLastError();
}

}  // namespace kad

// ------------------------------------------------------ host half: kad_dispatch_*
#include "kad_arena.h"

using namespace kad;

extern "C" {

// The counts, every offset array monotone from 0, every id in range, the observations strictly ascending per
// object, every flag known and consistent, obj_ns in [-2, N), every object's output capacity at least its
// placement entries plus its observations: all of it on the host, before anything is copied or launched.
static int validate_dispatch(const kad_dispatch_batch* b, const kad_dispatch_view* out, std::string* err) {
  auto bad = [&](const char* m) {
    *err = m;
    return KAD_EINVAL;
  };
  const int64_t C = b->n_clusters, O = b->n_objects, N = b->n_namespaces;
  if (C < 0 || O < 0 || N < 0) return bad("negative count");
  if (C > DI_MAX_CLUSTERS) {
    *err = "more than 16384 joined clusters: the per-wave bitmaps do not hold them";
    return KAD_EUNSUPPORTED;
  }
  if (C && !b->cluster_flags) return bad("cluster_flags missing");
  if (O && (!b->obj_flags || !b->obj_ns)) return bad("input array missing");
  constexpr uint8_t CL_ALL = KAD_DISPATCH_CL_READY | KAD_DISPATCH_CL_TERMINATING | KAD_DISPATCH_CL_CASCADING | KAD_DISPATCH_CL_FINALIZER;
  constexpr uint8_t OBJ_ALL = KAD_DISPATCH_OBJ_ERROR | KAD_DISPATCH_OBJ_ORPHAN_ALL | KAD_DISPATCH_OBJ_ORPHAN_ADOPTED;
  constexpr uint8_t OB_ALL = KAD_DISPATCH_OB_EXISTS | KAD_DISPATCH_OB_DELETING | KAD_DISPATCH_OB_ADOPTED | KAD_DISPATCH_OB_RETRIEVAL_FAILED;
  const uint8_t *cf = b->cluster_flags, *of = b->obj_flags;
  if (first_bad(C, [&](int64_t i) { return (cf[i] & ~CL_ALL) != 0; }) >= 0) return bad("cluster_flags: unknown flag");
  if (first_bad(O, [&](int64_t i) {
        constexpr uint8_t both = KAD_DISPATCH_OBJ_ORPHAN_ALL | KAD_DISPATCH_OBJ_ORPHAN_ADOPTED;
        return (of[i] & ~OBJ_ALL) != 0 || (of[i] & both) == both;
      }) >= 0)
    return bad("obj_flags: unknown flag, or ORPHAN_ALL together with ORPHAN_ADOPTED");
  const int32_t* ns = b->obj_ns;
  if (first_bad(O, [&](int64_t i) { return ns[i] < KAD_DISPATCH_NS_UNFEDERATED || ns[i] >= N; }) >= 0)
    return bad("obj_ns outside [-2, n_namespaces)");
  if (csr_bad(b->obj_pl_off, b->pl_cluster, O, -1, C)) return bad("obj_pl_off / pl_cluster malformed or id outside [-1, n_clusters)");
  if (csr_bad(b->ns_pl_off, b->ns_cluster, N, -1, C)) return bad("ns_pl_off / ns_cluster malformed or id outside [-1, n_clusters)");
  if (csr_bad(b->obj_ob_off, b->ob_cluster, O, 0, C)) return bad("obj_ob_off / ob_cluster malformed or id outside [0, n_clusters)");
  const int32_t *oo = b->obj_ob_off, *oc = b->ob_cluster;
  const int64_t B = oo[O];
  if (B && !b->ob_flags) return bad("ob_flags missing");
  if (first_bad(O, [&](int64_t i) {
        for (int64_t k = (int64_t)oo[i] + 1; k < oo[i + 1]; ++k)
          if (oc[k] <= oc[k - 1]) return true;
        return false;
      }) >= 0)
    return bad("ob_cluster is not strictly ascending within an object");
  const uint8_t* bf = b->ob_flags;
  if (first_bad(B, [&](int64_t k) {
        const uint8_t f = bf[k];
        if (f & ~OB_ALL) return true;
        const bool exists = (f & KAD_DISPATCH_OB_EXISTS) != 0, failed = (f & KAD_DISPATCH_OB_RETRIEVAL_FAILED) != 0;
        if (exists == failed) return true;  // both, or an entry that says nothing
        return !exists && (f & (KAD_DISPATCH_OB_DELETING | KAD_DISPATCH_OB_ADOPTED)) != 0;
      }) >= 0)
    return bad("ob_flags: unknown flag, DELETING or ADOPTED without EXISTS, or not exactly one of EXISTS and RETRIEVAL_FAILED");
  const int64_t* fo = b->out_off;
  if (off_bad(fo, O)) return bad("out_off not monotone from 0");
  const int32_t* po = b->obj_pl_off;
  if (first_bad(O, [&](int64_t i) { return fo[i + 1] - fo[i] < (int64_t)(po[i + 1] - po[i]) + (oo[i + 1] - oo[i]); }) >= 0)
    return bad("out_off: an object's capacity is below its placement entries plus its observations");
  if (!out || (O && (!out->count || !out->n_ops || !out->n_selected || !out->obj_result)) ||
      (fo[O] && (!out->out_cluster || !out->out_op || !out->out_status)))
    return bad("output view missing");
  return KAD_OK;
}

static int dispatch_plan_locked(kad_ctx* c, const kad_dispatch_batch* b, const kad_dispatch_view* out) {
  std::string err;
  if (int r = validate_dispatch(b, out, &err)) return fail(c, r, err);
  const int O = b->n_objects, N = b->n_namespaces, C = b->n_clusters;
  if (O == 0) return KAD_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const DispatchRoute route = route_dispatch(C, O, n_cus());
  // one buffer: the inputs, then the outputs
  const size_t o = (size_t)O, n = (size_t)N, np = (size_t)b->obj_pl_off[O], nn = (size_t)b->ns_pl_off[N],
               nb = (size_t)b->obj_ob_off[O], cap = (size_t)b->out_off[O];
  Stage& stg = c->stage[STG_DISPATCH];
  DispatchDev d{};
  d.C = C;
  d.nw = route.words;
  d.O = O;
  Arena a;
  a.in(d.cluster_flags, b->cluster_flags, (size_t)C);
  a.in(d.obj_flags, b->obj_flags, o);
  a.in(d.obj_ns, b->obj_ns, o);
  a.in(d.obj_pl_off, b->obj_pl_off, o + 1);
  a.in(d.pl_cluster, b->pl_cluster, np);
  a.in(d.ns_pl_off, b->ns_pl_off, n + 1);
  a.in(d.ns_cluster, b->ns_cluster, nn);
  a.in(d.obj_ob_off, b->obj_ob_off, o + 1);
  a.in(d.ob_cluster, b->ob_cluster, nb);
  a.in(d.ob_flags, b->ob_flags, nb);
  a.in(d.out_off, b->out_off, o + 1);
  a.out(d.count, out->count, o);
  a.out(d.n_ops, out->n_ops, o);
  a.out(d.n_selected, out->n_selected, o);
  a.out(d.obj_result, out->obj_result, o);
  // the entries come back into a host staging area (below), not into the caller's arrays
  a.out(d.out_cluster, cap);
  a.out(d.out_op, cap);
  a.out(d.out_status, cap);
  HIPCHK(c, hipEventRecord(stg.ev[0], c->stream));
  if (int r = a.commit(c, stg.buf)) return r;
  HIPCHK(c, hipEventRecord(stg.ev[1], c->stream));
  HIPCHK(c, launch_dispatch(d, route, c->stream));
  HIPCHK(c, hipEventRecord(stg.ev[2], c->stream));
  // the entries come back into a host staging area: only an object's first count[o] slots reach the caller's
  // arrays, the slack behind them stays as the caller left it
  std::vector<uint8_t>& hs = c->di_host;
  const size_t cl_bytes = sizeof *d.out_cluster * cap;
  if (hs.size() < cl_bytes + 2 * cap) hs.resize(cl_bytes + 2 * cap);
  int32_t* h_cl = reinterpret_cast<int32_t*>(hs.data());
  uint8_t *h_op = hs.data() + cl_bytes, *h_st = h_op + cap;
  if (int r = a.fetch(c)) return r;
  if (cap) {
    HIPCHK(c, hipMemcpyAsync(h_cl, d.out_cluster, cl_bytes, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h_op, d.out_op, cap, hipMemcpyDeviceToHost, c->stream));
    HIPCHK(c, hipMemcpyAsync(h_st, d.out_status, cap, hipMemcpyDeviceToHost, c->stream));
  }
  HIPCHK(c, hipEventRecord(stg.ev[3], c->stream));
  stage_ran(stg, route);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  const int64_t* fo = b->out_off;
  const int32_t* cnt = out->count;
  if (first_bad(O, [&](int64_t i) { return cnt[i] < 0 || cnt[i] > fo[i + 1] - fo[i]; }) >= 0)
    return fail(c, KAD_EHIP, "kad_dispatch_plan: a count outside its object's capacity came back from the device");
  host_parallel(O, [&](int lo, int hi) {
    for (int i = lo; i < hi; ++i) {
      const size_t at = (size_t)fo[i], k = (size_t)cnt[i];
      if (!k) continue;
      memcpy(out->out_cluster + at, h_cl + at, sizeof *h_cl * k);
      memcpy(out->out_op + at, h_op + at, k);
      memcpy(out->out_status + at, h_st + at, k);
    }
  });
  return KAD_OK;
}

int kad_dispatch_check(const kad_dispatch_batch* b, const kad_dispatch_view* out) {
  return check_guarded([&]() -> int {
    if (!b) return KAD_EINVAL;
    std::string err;
    return validate_dispatch(b, out, &err);
  });
}

int kad_dispatch_plan(kad_ctx* c, const kad_dispatch_batch* b, const kad_dispatch_view* out) {
  return entry(c, b != nullptr, [&]() -> int {
    return dispatch_plan_locked(c, b, out);
  });
}

int kad_dispatch_decide(uint32_t cluster_flags, int32_t selected, uint32_t ob_flags, uint32_t obj_flags, uint8_t out[3]) {
  if (!out || (cluster_flags & ~15u) || (ob_flags & ~15u) || (obj_flags & ~7u)) return KAD_EINVAL;
  const DiDecision x = di_decide((uint8_t)cluster_flags, selected != 0, (uint8_t)ob_flags, (uint8_t)obj_flags);
  out[0] = x.op;
  out[1] = x.status;
  out[2] = x.recheck;
  return KAD_OK;
}

int kad_dispatch_timing(kad_ctx* c, float ms[3]) { return stage_timing(c, STG_DISPATCH, 3, ms, "no kad_dispatch_plan ran"); }

int kad_dispatch_route_eval(int32_t n_clusters, int32_t n_objects, int32_t n_cu, int32_t* out) {
  if (!out || n_clusters < 0 || n_objects < 0 || n_cu < 1) return KAD_EINVAL;
  if (n_clusters > DI_MAX_CLUSTERS) return KAD_EUNSUPPORTED;
  return route_record<KAD_DISPATCH_ROUTE_FIELDS>(out, route_dispatch(n_clusters, n_objects, n_cu));
}

int kad_dispatch_last_route(kad_ctx* c, int32_t* out) { return stage_last_route(c, STG_DISPATCH, out, "no kad_dispatch_plan ran"); }

}  // extern "C"
