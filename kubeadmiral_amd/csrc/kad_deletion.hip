// Sync deletion (kad_deletion_plan, kad_deletion_finish): the arm of the sync controller's reconcile that runs for a
// federated object with a deletion timestamp, or for a target without a federated object.
//
// ensureDeletion / removeManagedLabel (pkg/controllers/sync/controller.go:723-817) walk the joined clusters in
// handleDeletionInClusters (:923-979): per (object, observed cluster) one table lookup (the cluster's readiness) and
// del_decide (kad_deletion.h), per object a few counts and what follows from them (del_plan_obj, del_finish_obj).
// Unobserved clusters contribute nothing but the batch-wide count of unready ones, so the kernels never walk C.
//
//   deletion_count_kernel    one block: the unready clusters of cluster_flags (and, for finish, of
//                            chk_cluster_flags), 16 bytes a load, into n_unready[2]; every object reads them
//   deletion_kernel<W, FIN>  every block first stages a byte per cluster (bit 0: ready; FIN, bit 1: ready at the
//                            second listing) into dynamic LDS with 16-byte loads. Blocks below long_grid: four waves,
//                            each one listed long object. The other blocks: a wave is 64 / W lane groups, each group
//                            takes one object at a time, its lanes striding over the object's observations (FIN: then
//                            its check rows); ob_cluster / ob_flags / op_ok loads and out_op stores are consecutive
//                            over the group, and over the wave's groups, because consecutive objects' entries are.
//                            The counts fold by __shfl_xor within the group, two 16-bit counts to a register (an
//                            object has at most 16384 entries), and the group's first lane writes the object's row.
//
// gfx950 code object (-Rpass-analysis=kernel-resource-usage), every instantiation: deletion_kernel<W, false> 46 VGPRs
// and 62 to 70 SGPRs, <W, true> 42 VGPRs and 80 to 92 SGPRs, deletion_count_kernel 21 and 30; scratch 0, no VGPR or
// SGPR spills; static LDS 0 (count kernel: 32 B), dynamic LDS = the clusters rounded up to 16 B (16 KiB at most);
// occupancy 8 waves a SIMD, so the 8 blocks (32 waves) a CU that group_grid launches are resident together
// (8 x 16 KiB <= 160 KiB).
// Plain vector stores, no atomics, no inline assembly, no state that kad_schedule reads.
#include "kad_deletion.h"

namespace kad {

namespace {

constexpr uint32_t DEL_LSB = 0x01010101u;

// bytes of word `w` (the clusters base .. base + 3) that belong to [0, C) and are not ready
__device__ __forceinline__ int del_unready_in(uint32_t w, int base, int C) {
  const int nv = C - base;
  if (nv <= 0) return 0;
  const uint32_t m = nv >= 4 ? DEL_LSB : (DEL_LSB & ((1u << (8 * nv)) - 1u));
  return __builtin_popcount(~w & m);
}
__device__ __forceinline__ int del_unready_in(const uint4& v, int q, int C) {
  return del_unready_in(v.x, q * 16, C) + del_unready_in(v.y, q * 16 + 4, C) + del_unready_in(v.z, q * 16 + 8, C) +
         del_unready_in(v.w, q * 16 + 12, C);
}

template <int W>
__device__ __forceinline__ int del_group_sum(int v) {  // to every lane of the group
#pragma unroll
  for (int m = W / 2; m >= 1; m >>= 1) v += __shfl_xor(v, m);
  return v;
}

// One object (o < 0: none) by the W lanes of a group, gl the lane's index in it; cl: the staged cluster bytes.
// Every lane of the wave comes here together.
template <int W, bool FIN>
__device__ __forceinline__ void del_object(const DeletionDev& d, const uint8_t* cl, int o, int gl, int n_un, int n_un2) {
  int lo = 0, n = 0, klo = 0, kn = 0;
  uint8_t of = 0;
  if (o >= 0) {
    lo = d.obj_ob_off[o];
    n = d.obj_ob_off[o + 1] - lo;
    of = d.obj_flags[o];
    if (FIN) {
      klo = d.chk_off[o];
      kn = d.chk_off[o + 1] - klo;
    }
  }
  int ops_rem = 0, rf_fail = 0, fc = 0;  // n_ops | n_remaining << 16, n_retrieval_failed | n_failed_ops << 16
  for (int i = gl; i < n; i += W) {
    const int c = d.ob_cluster[lo + i];
    const DelDecision x = del_decide(of, (cl[c] & 1) != 0, d.ob_flags[lo + i]);
    ops_rem += (x.op != DEL_OP_NONE) | (int)x.remaining << 16;
    rf_fail += x.failed;
    if (FIN)
      rf_fail += (int)(x.op != DEL_OP_NONE && d.op_ok[lo + i] == 0) << 16;
    else
      d.out_op[lo + i] = x.op;
  }
  if (FIN) {
    for (int i = gl; i < kn; i += W) {
      const int c = d.chk_cluster[klo + i];
      fc += (cl[c] & 2) != 0 && d.chk_flags[klo + i] != DEL_CHK_UNLABELLED;
    }
  }
  if (W > 1) {
    ops_rem = del_group_sum<W>(ops_rem);
    rf_fail = del_group_sum<W>(rf_fail);
    if (FIN) fc = del_group_sum<W>(fc);
  }
  if (o < 0 || gl != 0) return;
  const bool walks = del_walks(of);
  const DelCounts k{ops_rem & 0xffff, ops_rem >> 16, rf_fail & 0xffff, rf_fail >> 16, fc};
  if (!FIN) {
    const DelPlanObj p = del_plan_obj(of, k, n_un);
    d.n_ops[o] = k.n_ops;
    d.n_remaining[o] = k.n_remaining;
    d.n_retrieval_failed[o] = k.n_failed_rf;
    d.obj_pre[o] = p.pre;
    d.obj_first[o] = p.first;
  } else {
    const DelFinishObj f = del_finish_obj(of, d.obj_wait[o], k, n_un, n_un2, d.C);
    d.obj_status[o] = f.status;
    d.obj_reason[o] = f.reason;
    d.obj_then[o] = f.then;
    d.n_failed_ops[o] = walks ? k.n_failed_ops : 0;
    d.n_failed_checks[o] = f.checked ? k.n_failed_checks : 0;
  }
}

}  // namespace

__global__ __launch_bounds__(256) void deletion_count_kernel(DeletionDev d, int finish) {
  __shared__ int part[2][4];
  const int nq = (d.C + 15) >> 4;
  const uint4* a4 = reinterpret_cast<const uint4*>(d.cluster_flags);
  const uint4* b4 = reinterpret_cast<const uint4*>(d.chk_cluster_flags);
  int a = 0, b = 0;
  for (int q = (int)threadIdx.x; q < nq; q += 256) {
    a += del_unready_in(a4[q], q, d.C);
    if (finish) b += del_unready_in(b4[q], q, d.C);
  }
  a = del_group_sum<64>(a);
  b = del_group_sum<64>(b);
  if (((int)threadIdx.x & 63) == 0) {
    part[0][(int)threadIdx.x >> 6] = a;
    part[1][(int)threadIdx.x >> 6] = b;
  }
  __syncthreads();
  if (threadIdx.x < 2) d.n_unready[threadIdx.x] = part[threadIdx.x][0] + part[threadIdx.x][1] + part[threadIdx.x][2] + part[threadIdx.x][3];
}

template <int W, bool FIN>
__global__ __launch_bounds__(256) void deletion_kernel(DeletionDev d, int long_grid) {
  extern __shared__ uint4 del_cl4[];  // a byte per cluster, rounded up to 16
  {
    const int nq = (d.C + 15) >> 4;
    const uint4* a4 = reinterpret_cast<const uint4*>(d.cluster_flags);
    const uint4* b4 = reinterpret_cast<const uint4*>(d.chk_cluster_flags);
    for (int q = (int)threadIdx.x; q < nq; q += 256) {
      uint4 v = a4[q];
      v.x &= DEL_LSB, v.y &= DEL_LSB, v.z &= DEL_LSB, v.w &= DEL_LSB;
      if (FIN) {
        const uint4 b = b4[q];
        v.x |= (b.x & DEL_LSB) << 1, v.y |= (b.y & DEL_LSB) << 1, v.z |= (b.z & DEL_LSB) << 1, v.w |= (b.w & DEL_LSB) << 1;
      }
      del_cl4[q] = v;
    }
  }
  __syncthreads();
  const uint8_t* cl = reinterpret_cast<const uint8_t*>(del_cl4);
  const int n_un = d.n_unready[0], n_un2 = FIN ? d.n_unready[1] : 0;
  if ((int)blockIdx.x < long_grid) {
    // ---- long path: one listed object per wave
    const int w = (int)blockIdx.x * 4 + ((int)threadIdx.x >> 6);
    del_object<64, FIN>(d, cl, w < d.n_long ? d.long_list[w] : -1, (int)threadIdx.x & 63, n_un, n_un2);
    return;
  }
  // ---- group path: the loop is uniform over the wave (groups past O, and those whose object is long, idle)
  constexpr int GPB = 256 / W;
  const int gl = (int)threadIdx.x & (W - 1), g = (int)threadIdx.x / W;
  const int64_t stride = (int64_t)((int)gridDim.x - long_grid) * GPB;
  for (int64_t base = (int64_t)((int)blockIdx.x - long_grid) * GPB; base < d.O; base += stride) {
    const int64_t o64 = base + g;
    int o = o64 < d.O ? (int)o64 : -1;
    if (o >= 0) {
      int64_t n = (int64_t)d.obj_ob_off[o + 1] - d.obj_ob_off[o];
      if (FIN) n += (int64_t)d.chk_off[o + 1] - d.chk_off[o];
      if (n > d.long_min) o = -1;
    }
    del_object<W, FIN>(d, cl, o, gl, n_un, n_un2);
  }
}

hipError_t launch_deletion(const DeletionDev& d, const DeletionRoute& r, bool finish, hipStream_t st) {
  (void)hipGetLastError();
  const unsigned grid = (unsigned)(r.grid + r.long_grid);
  if (grid == 0) return hipSuccess;
  hipLaunchKernelGGL(deletion_count_kernel, dim3(1), dim3(256), 0, st, d, finish ? 1 : 0);
  with_width<1>(r.width, [&](auto W) {
    if (finish)
      hipLaunchKernelGGL((deletion_kernel<decltype(W)::value, true>), dim3(grid), dim3((unsigned)r.threads), (size_t)r.lds, st, d,
                         r.long_grid);
    else
      hipLaunchKernelGGL((deletion_kernel<decltype(W)::value, false>), dim3(grid), dim3((unsigned)r.threads), (size_t)r.lds, st, d,
                         r.long_grid);
  });
  return hipGetLastError();
}

}  // namespace kad

// ------------------------------------------------------ host half: kad_deletion_*
#include "kad_arena.h"

using namespace kad;

namespace {

// what the validation leaves for the launch: the objects of the long path, the other objects' entries
struct DeletionHost {
  std::vector<int32_t> long_list;
  int64_t short_items = 0;
};

}  // namespace

extern "C" {

// The counts, both offset arrays monotone from 0, every id in range and strictly ascending per object, every flag
// known and consistent, the object flags exclusive where they must be, op_ok 0 or 1, a check row exactly one answer,
// the outputs: all of it on the host, before anything is copied or launched. res / fout: the finish call's (null for
// the plan, which takes out). With `host` the same pass leaves the long path's list.
static int validate_deletion(const kad_deletion_batch* b, const kad_deletion_view* out, const kad_deletion_results* res,
                             const kad_deletion_finish_view* fout, bool finish, int long_min, DeletionHost* host,
                             std::string* err) {
  auto bad = [&](const char* m) {
    *err = m;
    return KAD_EINVAL;
  };
  const int64_t C = b->n_clusters, O = b->n_objects;
  if (C < 0 || O < 0) return bad("negative count");
  if (C > DEL_MAX_CLUSTERS) {
    *err = "more than 16384 joined clusters: a block's LDS table does not hold them";
    return KAD_EUNSUPPORTED;
  }
  if (C && !b->cluster_flags) return bad("cluster_flags missing");
  if (O && !b->obj_flags) return bad("obj_flags missing");
  const uint8_t *cf = b->cluster_flags, *of = b->obj_flags;
  if (first_bad(C, [&](int64_t i) { return (cf[i] & ~DEL_CL_ALL) != 0; }) >= 0) return bad("cluster_flags: unknown flag");
  constexpr uint8_t OBJ_ALL = KAD_DEL_OBJ_HAS_FINALIZER | KAD_DEL_OBJ_ORPHAN_ALL | KAD_DEL_OBJ_ORPHAN_ADOPTED | KAD_DEL_OBJ_POSSIBLE_ORPHAN;
  if (first_bad(O, [&](int64_t i) { return (of[i] & ~OBJ_ALL) != 0; }) >= 0) return bad("obj_flags: unknown flag");
  if (first_bad(O, [&](int64_t i) {
        constexpr uint8_t both = KAD_DEL_OBJ_ORPHAN_ALL | KAD_DEL_OBJ_ORPHAN_ADOPTED;
        return (of[i] & both) == both;
      }) >= 0)
    return bad("obj_flags: ORPHAN_ALL together with ORPHAN_ADOPTED");
  if (first_bad(O, [&](int64_t i) { return (of[i] & KAD_DEL_OBJ_POSSIBLE_ORPHAN) && of[i] != KAD_DEL_OBJ_POSSIBLE_ORPHAN; }) >= 0)
    return bad("obj_flags: POSSIBLE_ORPHAN together with another flag");
  if (csr_bad(b->obj_ob_off, b->ob_cluster, O, 0, C)) return bad("obj_ob_off / ob_cluster malformed or id outside [0, n_clusters)");
  const int32_t *oo = b->obj_ob_off, *oc = b->ob_cluster;
  const int64_t B = oo[O];
  if (B && !b->ob_flags) return bad("ob_flags missing");
  auto ascending = [&](const int32_t* off, const int32_t* id) {
    return first_bad(O, [&](int64_t i) {
             for (int64_t k = (int64_t)off[i] + 1; k < off[i + 1]; ++k)
               if (id[k] <= id[k - 1]) return true;
             return false;
           }) < 0;
  };
  if (!ascending(oo, oc)) return bad("ob_cluster is not strictly ascending within an object");
  const uint8_t* bf = b->ob_flags;
  constexpr uint8_t OB_ALL = KAD_DISPATCH_OB_EXISTS | KAD_DISPATCH_OB_DELETING | KAD_DISPATCH_OB_ADOPTED | KAD_DISPATCH_OB_RETRIEVAL_FAILED;
  if (first_bad(B, [&](int64_t k) {
        const uint8_t f = bf[k];
        if (f & ~OB_ALL) return true;
        const bool exists = (f & KAD_DISPATCH_OB_EXISTS) != 0, failed = (f & KAD_DISPATCH_OB_RETRIEVAL_FAILED) != 0;
        if (exists == failed) return true;  // both, or an entry that says nothing
        return !exists && (f & (KAD_DISPATCH_OB_DELETING | KAD_DISPATCH_OB_ADOPTED)) != 0;
      }) >= 0)
    return bad("ob_flags: unknown flag, DELETING or ADOPTED without EXISTS, or not exactly one of EXISTS and RETRIEVAL_FAILED");
  const int32_t* ko = nullptr;
  if (!finish) {
    if (!out || (O && (!out->n_ops || !out->n_remaining || !out->n_retrieval_failed || !out->obj_pre || !out->obj_first)) ||
        (B && !out->out_op))
      return bad("output view missing");
  } else {
    if (!res) return bad("results missing");
    if (B && !res->op_ok) return bad("op_ok missing");
    if (O && !res->obj_wait) return bad("obj_wait missing");
    if (C && !res->chk_cluster_flags) return bad("chk_cluster_flags missing");
    const uint8_t *ok = res->op_ok, *wt = res->obj_wait, *ccf = res->chk_cluster_flags;
    if (first_bad(B, [&](int64_t k) { return ok[k] > 1; }) >= 0) return bad("op_ok: a value other than 0 and 1");
    constexpr uint8_t WAIT_ALL = KAD_DEL_WAIT_TIMED_OUT | KAD_DEL_WAIT_CHECK_TIMED_OUT;
    if (first_bad(O, [&](int64_t i) { return (wt[i] & ~WAIT_ALL) != 0; }) >= 0) return bad("obj_wait: unknown flag");
    if (first_bad(C, [&](int64_t i) { return (ccf[i] & ~DEL_CL_ALL) != 0; }) >= 0) return bad("chk_cluster_flags: unknown flag");
    if (csr_bad(res->chk_off, res->chk_cluster, O, 0, C)) return bad("chk_off / chk_cluster malformed or id outside [0, n_clusters)");
    ko = res->chk_off;
    const int64_t K = ko[O];
    if (K && !res->chk_flags) return bad("chk_flags missing");
    if (!ascending(ko, res->chk_cluster)) return bad("chk_cluster is not strictly ascending within an object");
    const uint8_t* kf = res->chk_flags;
    if (first_bad(K, [&](int64_t k) {
          const uint8_t f = kf[k];
          return f != KAD_DEL_CHK_GET_FAILED && f != KAD_DEL_CHK_DELETING && f != KAD_DEL_CHK_LABELLED && f != KAD_DEL_CHK_UNLABELLED;
        }) >= 0)
      return bad("chk_flags: not exactly one of GET_FAILED, DELETING, LABELLED and UNLABELLED");
    if (!fout || (O && (!fout->obj_status || !fout->obj_reason || !fout->obj_then || !fout->n_failed_ops || !fout->n_failed_checks)))
      return bad("output view missing");
  }
  if (host)
    for (int64_t i = 0; i < O; ++i) {
      const int64_t n = (int64_t)(oo[i + 1] - oo[i]) + (ko ? ko[i + 1] - ko[i] : 0);
      if (n > long_min)
        host->long_list.push_back((int32_t)i);
      else
        host->short_items += n;
    }
  return KAD_OK;
}

static int deletion_locked(kad_ctx* c, const kad_deletion_batch* b, const kad_deletion_view* out, const kad_deletion_results* res,
                           const kad_deletion_finish_view* fout, bool finish) {
  Stage& stg = c->stage[finish ? STG_DELFIN : STG_DELPLAN];
  const int long_min = stg.force.long_min_or(DEL_LONG_MIN);
  std::string err;
  DeletionHost host;
  if (int r = validate_deletion(b, out, res, fout, finish, long_min, &host, &err)) return fail(c, r, err);
  const int O = b->n_objects, C = b->n_clusters;
  if (O == 0) return KAD_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const int n_long = (int)host.long_list.size();
  DeletionRoute route = route_deletion(C, O, n_long, host.short_items, n_cus());
  group_force_apply(stg.force, n_long < O, O, n_cus(), route.width, route.grid, &route.stride);
  route.long_min = long_min;
  // one buffer: the inputs, then the outputs. The kernels read both cluster arrays 16 bytes at a time.
  const size_t o = (size_t)O, cl = (size_t)C, nb = (size_t)b->obj_ob_off[O], pad16 = (16 - cl % 16) % 16;
  DeletionDev d{};
  d.C = C;
  d.O = O;
  d.n_long = n_long;
  d.long_min = long_min;
  Arena a;
  a.in(d.cluster_flags, b->cluster_flags, cl, pad16);
  a.in(d.obj_flags, b->obj_flags, o);
  a.in(d.obj_ob_off, b->obj_ob_off, o + 1);
  a.in(d.ob_cluster, b->ob_cluster, nb);
  a.in(d.ob_flags, b->ob_flags, nb);
  a.in(d.long_list, host.long_list.data(), (size_t)n_long);
  a.out(d.n_unready, 2);
  if (!finish) {
    a.out(d.out_op, out->out_op, nb);
    a.out(d.n_ops, out->n_ops, o);
    a.out(d.n_remaining, out->n_remaining, o);
    a.out(d.n_retrieval_failed, out->n_retrieval_failed, o);
    a.out(d.obj_pre, out->obj_pre, o);
    a.out(d.obj_first, out->obj_first, o);
  } else {
    const size_t nk = (size_t)res->chk_off[O];
    a.in(d.op_ok, res->op_ok, nb);
    a.in(d.obj_wait, res->obj_wait, o);
    a.in(d.chk_off, res->chk_off, o + 1);
    a.in(d.chk_cluster, res->chk_cluster, nk);
    a.in(d.chk_flags, res->chk_flags, nk);
    a.in(d.chk_cluster_flags, res->chk_cluster_flags, cl, pad16);
    a.out(d.obj_status, fout->obj_status, o);
    a.out(d.obj_reason, fout->obj_reason, o);
    a.out(d.obj_then, fout->obj_then, o);
    a.out(d.n_failed_ops, fout->n_failed_ops, o);
    a.out(d.n_failed_checks, fout->n_failed_checks, o);
  }
  HIPCHK(c, hipEventRecord(stg.ev[0], c->stream));
  if (int r = a.commit(c, stg.buf)) return r;
  HIPCHK(c, hipEventRecord(stg.ev[1], c->stream));
  HIPCHK(c, launch_deletion(d, route, finish, c->stream));
  HIPCHK(c, hipEventRecord(stg.ev[2], c->stream));
  if (int r = a.fetch(c)) return r;
  HIPCHK(c, hipEventRecord(stg.ev[3], c->stream));
  stage_ran(stg, route);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return KAD_OK;
}

int kad_deletion_check(const kad_deletion_batch* b, const kad_deletion_view* out) {
  return check_guarded([&]() -> int {
    if (!b) return KAD_EINVAL;
    std::string err;
    return validate_deletion(b, out, nullptr, nullptr, false, DEL_LONG_MIN, nullptr, &err);
  });
}

int kad_deletion_finish_check(const kad_deletion_batch* b, const kad_deletion_finish_view* out, const kad_deletion_results* res) {
  return check_guarded([&]() -> int {
    if (!b) return KAD_EINVAL;
    std::string err;
    return validate_deletion(b, nullptr, res, out, true, DEL_LONG_MIN, nullptr, &err);
  });
}

int kad_deletion_plan(kad_ctx* c, const kad_deletion_batch* b, const kad_deletion_view* out) {
  return entry(c, b != nullptr, [&]() -> int {
    return deletion_locked(c, b, out, nullptr, nullptr, false);
  });
}

int kad_deletion_finish(kad_ctx* c, const kad_deletion_batch* b, const kad_deletion_results* res, const kad_deletion_finish_view* out) {
  return entry(c, b != nullptr, [&]() -> int {
    return deletion_locked(c, b, nullptr, res, out, true);
  });
}

int kad_deletion_decide(uint32_t obj_flags, int32_t cluster_ready, uint32_t ob_flags, uint8_t out[3]) {
  if (!out || (obj_flags & ~15u) || (ob_flags & ~15u)) return KAD_EINVAL;
  const DelDecision x = del_decide((uint8_t)obj_flags, cluster_ready != 0, (uint8_t)ob_flags);
  out[0] = x.op;
  out[1] = x.remaining;
  out[2] = x.failed;
  return KAD_OK;
}

int kad_deletion_timing(kad_ctx* c, float ms[3]) { return stage_timing(c, STG_DELPLAN, 3, ms, "no kad_deletion_plan ran"); }
int kad_deletion_finish_timing(kad_ctx* c, float ms[3]) { return stage_timing(c, STG_DELFIN, 3, ms, "no kad_deletion_finish ran"); }

static int deletion_route_eval(int32_t n_clusters, int32_t n_objects, int32_t n_long, int64_t short_items, int32_t n_cu, int32_t* out) {
  if (!out || n_clusters < 0 || n_objects < 0 || n_long < 0 || n_long > n_objects || short_items < 0 || n_cu < 1) return KAD_EINVAL;
  if (n_clusters > DEL_MAX_CLUSTERS) return KAD_EUNSUPPORTED;
  return route_record<KAD_DEL_ROUTE_FIELDS>(out, route_deletion(n_clusters, n_objects, n_long, short_items, n_cu));
}
int kad_deletion_route_eval(int32_t n_clusters, int32_t n_objects, int32_t n_long, int64_t short_items, int32_t n_cu, int32_t* out) {
  return deletion_route_eval(n_clusters, n_objects, n_long, short_items, n_cu, out);
}
int kad_deletion_finish_route_eval(int32_t n_clusters, int32_t n_objects, int32_t n_long, int64_t short_items, int32_t n_cu,
                                   int32_t* out) {
  return deletion_route_eval(n_clusters, n_objects, n_long, short_items, n_cu, out);
}

int kad_deletion_last_route(kad_ctx* c, int32_t* out) { return stage_last_route(c, STG_DELPLAN, out, "no kad_deletion_plan ran"); }
int kad_deletion_finish_last_route(kad_ctx* c, int32_t* out) {
  return stage_last_route(c, STG_DELFIN, out, "no kad_deletion_finish ran");
}

int kad_deletion_debug_route(kad_ctx* c, int32_t force_width, int32_t force_long_min) {
  return stage_debug_route(c, STG_DELPLAN, group_width_ok(force_width, 1), GroupForce{force_width, force_long_min});
}
int kad_deletion_finish_debug_route(kad_ctx* c, int32_t force_width, int32_t force_long_min) {
  return stage_debug_route(c, STG_DELFIN, group_width_ok(force_width, 1), GroupForce{force_width, force_long_min});
}

}  // extern "C"
