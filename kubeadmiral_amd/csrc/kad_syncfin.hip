// Sync completion (kad_sync_needs_update, kad_sync_finish): the second half of the sync controller's syncToClusters
// for a batch of federated objects.
//
// After kad_dispatch_plan has decided the operations, the reference checks every update against the propagated
// versions (ObjectNeedsUpdate, util/propagatedversion.go:54-119, with VersionForCluster, sync/version/
// manager.go:119-148) and, once dispatcher.Wait() returns, closes the reconcile (sync/controller.go:546-596):
// Wait's status transitions (dispatch/managed.go:137-155), the new cluster versions and whether the
// PropagatedVersion object is written (manager.go:152-210, 448-479), the generation map
// (propagatedversion.go:138-157) and status.update (sync/status/status.go:87-229). Per object these are joins of
// sparse lists that ascend by cluster id:
//
//   syncfin_rows_kernel  a lane per update row: binary search of the object's recorded versions, the decision
//   syncfin_kernel<W>    blocks below n_long: one listed long object per 256-thread block; the other blocks: a wave is
//                        64 / W lane groups, each group takes one object at a time. The lanes stride over a list,
//                        membership in another list is a binary search in global memory, and an entry's place in an
//                        output is its emitted rank in its own list (ballot + popcount below the lane, carried from
//                        pass to pass) plus the emitted entries of the other list below its cluster, read from that
//                        list's exclusive counts in scratch (written in the first phase, read after a fence).
//
// Integers only, no atomics, ordinary vector stores: nothing depends on an order.
#include "kad_syncfin.h"
#include "kad_wave.h"

namespace kad {

// the first index in [lo, hi) of the ascending a whose value is not below key
__device__ __forceinline__ int sf_lower(const int32_t* a, int lo, int hi, int key) {
  while (lo < hi) {
    const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
    if (a[mid] < key)
      lo = mid + 1;
    else
      hi = mid;
  }
  return lo;
}

__global__ __launch_bounds__(SF_THREADS) void syncfin_rows_kernel(SyncRowsDev d) {
  const int64_t stride = (int64_t)gridDim.x * SF_THREADS;
  for (int64_t r = (int64_t)blockIdx.x * SF_THREADS + threadIdx.x; r < d.n_rows; r += stride) {
    const int o = d.row_obj[r], c = d.row_cluster[r], target = d.row_target[r];
    const uint8_t rf = d.row_flags[r];
    int rec = 0;
    if (d.obj_flags[o] & 1) {  // the stored versions are still valid (manager.go:140-146)
      const int lo = d.rec_off[o], hi = d.rec_off[o + 1], p = sf_lower(d.rec_cluster, lo, hi, c);
      if (p < hi && d.rec_cluster[p] == c) rec = d.rec_version[p];
    }
    constexpr uint8_t EQ = SF_ROW_REPLICAS | SF_ROW_SURGE | SF_ROW_UNAVAILABLE;
    // propagatedversion.go:61-63, 65-114, 118
    const bool need = rec != target || (rf & EQ) != EQ || ((d.ver_flags[target] & SF_VER_IS_GEN) && !(rf & SF_ROW_META));
    d.recorded[r] = rec;
    d.needs_update[r] = need ? 1 : 0;
  }
}

// The W lanes that share an object: a lane group of a wave (W <= 64) or a block (W == 256). Every lane of them calls
// scan3 / any / sync together.
template <int W>
struct Lanes {
  int gl;           // this lane among them
  uint32_t* s_cnt;  // W == 256: [2][4] in LDS
  int par;
  __device__ __forceinline__ uint64_t mask(bool p) const {
    const uint64_t m = ballot(p);
    if (W == 64) return m;
    return (m >> (lane_id_h() & ~(W - 1) & 63)) & ((1ull << (W & 63)) - 1);
  }
  // of three predicates, packed 10 bits each: how many lanes below this one hold them, and how many in all
  __device__ __forceinline__ void scan3(bool a, bool b, bool c, uint32_t& excl, uint32_t& total) {
    if constexpr (W <= 64) {
      const uint64_t ma = mask(a), mb = mask(b), mc = mask(c), below = (1ull << gl) - 1;
      excl = (uint32_t)popc64(ma & below) | (uint32_t)popc64(mb & below) << 10 | (uint32_t)popc64(mc & below) << 20;
      total = (uint32_t)popc64(ma) | (uint32_t)popc64(mb) << 10 | (uint32_t)popc64(mc) << 20;
    } else {
      const uint64_t ma = ballot(a), mb = ballot(b), mc = ballot(c);
      const int w = (int)threadIdx.x >> 6;
      if ((threadIdx.x & 63) == 0)
        s_cnt[par * 4 + w] = (uint32_t)popc64(ma) | (uint32_t)popc64(mb) << 10 | (uint32_t)popc64(mc) << 20;
      __syncthreads();  // the other parity is written next: one barrier a call
      excl = (uint32_t)mbcnt(ma) | (uint32_t)mbcnt(mb) << 10 | (uint32_t)mbcnt(mc) << 20;
      total = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const uint32_t t = s_cnt[par * 4 + q];
        if (q < w) excl += t;
        total += t;
      }
      par ^= 1;
    }
  }
  __device__ __forceinline__ bool any(bool p) {
    if constexpr (W <= 64) {
      return mask(p) != 0;
    } else {
      uint32_t e, t;
      scan3(p, false, false, e, t);
      return t != 0;
    }
  }
  // the scratch written before is read after
  __device__ __forceinline__ void sync() {
    if constexpr (W <= 64)
      wave_sync_global();
    else
      __syncthreads();
  }
};

// One object, by its W lanes. Every loop below has the same trip count on all of them.
template <int W>
__device__ __forceinline__ void sf_object(const SyncFinDev& d, const int o, Lanes<W>& L) {
  const uint16_t f = d.obj_flags[o];
  const bool cur = (f & SF_OBJ_CURRENT) != 0, on_host = (f & SF_OBJ_ON_HOST) != 0;
  const int s_lo = d.sel_off[o], s_hi = d.sel_off[o + 1];
  const int e_lo = d.ent_off[o], e_hi = d.ent_off[o + 1], n_ent = e_hi - e_lo;
  const int v_lo = d.oldv_off[o], n_oldv = d.oldv_off[o + 1] - v_lo;
  // the stored versions are kept only while the template and override versions match (manager.go:175-177)
  const int n_ov = cur ? n_oldv : 0, v_hi = v_lo + n_ov;
  const int t_lo = d.olds_off[o], n_olds = d.olds_off[o + 1] - t_lo;
  const int64_t ver_at = d.ver_off[o], st_at = d.st_off[o];
  int32_t* const e_pre = d.ent_pre + e_lo + o;
  int32_t* const v_pre = d.oldv_pre + v_lo + o;
  uint32_t ex, tot;

  // ---- phase 1a: the dispatcher's records. Wait's transitions, the status entries (their place needs this list
  // alone), the counts of the three maps
  int cv = 0, cs = 0, cg = 0;  // entries with a version / a status / a generation so far
  bool notok = false;
  for (int b = 0; b < n_ent; b += W) {
    const int i = b + L.gl;
    const bool live = i < n_ent;
    int c = 0, v = 0;
    uint8_t s = 0;
    if (live) {
      c = d.ent_cluster[e_lo + i];
      s = sf_transition(d.ent_status[e_lo + i]);
      v = d.ent_version[e_lo + i];
    }
    const bool has_v = v != 0, has_s = s != 0;
    const bool has_g = has_v && (d.ver_flags[v] & SF_VER_HAS_GEN);
    L.scan3(has_v, has_s, has_g, ex, tot);
    if (live) e_pre[i] = cv + (int)(ex & 1023);
    if (has_s && !on_host) {  // setClusters (status.go:139-153)
      const int64_t r = st_at + cs + (int)((ex >> 10) & 1023);
      d.out_st_cluster[r] = c;
      d.out_st_status[r] = s;
      d.out_st_gen[r] = has_g ? d.ver_gen[v] : 0;
    }
    notok |= has_s && s != SF_ST_OK;
    cv += (int)(tot & 1023);
    cs += (int)((tot >> 10) & 1023);
    cg += (int)(tot >> 20);
  }
  if (L.gl == 0) e_pre[n_ent] = cv;
  const bool any_notok = L.any(notok);

  // ---- phase 1b: the stored versions that are retained: the cluster is selected and the dispatcher recorded no
  // version for it (updateClusterVersions, manager.go:452-460)
  int cr = 0;
  for (int b = 0; b < n_ov; b += W) {
    const int j = b + L.gl;
    const bool live = j < n_ov;
    bool keep = false;
    if (live) {
      const int c = d.oldv_cluster[v_lo + j];
      const int ps = sf_lower(d.sel_cluster, s_lo, s_hi, c);
      if (ps < s_hi && d.sel_cluster[ps] == c) {
        const int pe = sf_lower(d.ent_cluster, e_lo, e_hi, c);
        keep = !(pe < e_hi && d.ent_cluster[pe] == c && d.ent_version[pe] != 0);
      }
    }
    L.scan3(keep, false, false, ex, tot);
    if (live) v_pre[j] = cr + (int)(ex & 1023);
    cr += (int)(tot & 1023);
  }
  if (L.gl == 0) v_pre[n_ov] = cr;

  // ---- phase 1c: clustersDiffers (status.go:159-179): both lengths, then every stored entry against the maps
  bool differs = false;
  if (!on_host) {
    differs = n_olds != cs || n_olds != cg;
    if (!differs) {
      bool dl = false;
      for (int b = 0; b < n_olds; b += W) {
        const int k = b + L.gl;
        if (k < n_olds) {
          const int c = d.olds_cluster[t_lo + k];
          const int pe = sf_lower(d.ent_cluster, e_lo, e_hi, c);
          uint8_t s = 0;
          int64_t g = 0;
          if (pe < e_hi && d.ent_cluster[pe] == c) {
            s = sf_transition(d.ent_status[pe]);
            const int v = d.ent_version[pe];
            if (v != 0 && (d.ver_flags[v] & SF_VER_HAS_GEN)) g = d.ver_gen[v];
          }
          dl |= s != d.olds_status[t_lo + k] || g != d.olds_gen[t_lo + k];
        }
      }
      differs = L.any(dl);
    }
  }

  L.sync();

  // ---- phase 2: the new cluster versions, ascending: an entry's place is its rank among the emitted entries of
  // its own list plus the other list's emitted entries below its cluster. PropagatedVersionStatusEquivalent on the
  // way: the entry at place r must be oldv's r-th.
  bool mism = false;
  for (int b = 0; b < n_ent; b += W) {
    const int i = b + L.gl;
    if (i < n_ent) {
      const int v = d.ent_version[e_lo + i];
      if (v != 0) {
        const int c = d.ent_cluster[e_lo + i];
        const int p = sf_lower(d.oldv_cluster, v_lo, v_hi, c) - v_lo;
        const int r = e_pre[i] + v_pre[p];
        d.out_ver_cluster[ver_at + r] = c;
        d.out_ver_id[ver_at + r] = v;
        if (cur) mism |= r >= n_ov || d.oldv_cluster[v_lo + r] != c || d.oldv_version[v_lo + r] != v;
      }
    }
  }
  for (int b = 0; b < n_ov; b += W) {
    const int j = b + L.gl;
    if (j < n_ov) {
      const int at = v_pre[j];
      if (v_pre[j + 1] != at) {
        const int c = d.oldv_cluster[v_lo + j];
        const int p = sf_lower(d.ent_cluster, e_lo, e_hi, c) - e_lo;
        const int r = at + e_pre[p];
        d.out_ver_cluster[ver_at + r] = c;
        d.out_ver_id[ver_at + r] = d.oldv_version[v_lo + j];
        mism |= r != j;
      }
    }
  }
  const int n_new = cv + cr;
  const bool any_mism = L.any(mism);

  if (L.gl == 0) {
    // manager.go:189: no stored status, or one that is not equivalent to the new
    const bool write = !(f & SF_OBJ_EXISTS) || !cur || (f & SF_OBJ_OLDV_IRREGULAR) || ((f & SF_OBJ_OLDV_NIL) && n_new == 0) ||
                       n_new != n_oldv || any_mism;
    d.ver_count[o] = n_new;
    d.ver_write[o] = write ? 1 : 0;
    if (on_host) {
      d.st_count[o] = 0;
      d.obj_out[o] = 0;
      d.reason_out[o] = 0;
    } else {
      int reason = d.reason_in[o];
      if (reason == 0 && any_notok) reason = d.reason_check;  // status.go:106-113
      const bool propagated = differs || (cs > 0 && (f & SF_OBJ_UPDATED));  // status.go:120
      // setPropagationCondition (status.go:189-228)
      const bool transition = !(f & SF_OBJ_COND_EXISTS) || ((f & SF_OBJ_COND_TRUE) != 0) != (reason == 0) || d.cond_reason[o] != reason;
      const bool required = propagated || transition;
      const bool status_write = (f & SF_OBJ_SCALARS) || required;  // status.go:124
      d.st_count[o] = cs;
      d.obj_out[o] = (uint8_t)((differs ? SF_OUT_CLUSTERS : 0) | (propagated ? SF_OUT_PROPAGATED : 0) |
                               (transition ? SF_OUT_TRANSITION : 0) | (required ? SF_OUT_REQUIRED : 0) |
                               (status_write ? SF_OUT_WRITE : 0));
      d.reason_out[o] = reason;
    }
  }
}

template <int W>
__global__ __launch_bounds__(SF_THREADS) void syncfin_kernel(SyncFinDev d) {
  __shared__ uint32_t s_cnt[8];
  if ((int)blockIdx.x < d.n_long) {
    // ---- long path: one listed object per block
    Lanes<256> L{(int)threadIdx.x, s_cnt, 0};
    sf_object<256>(d, d.long_list[blockIdx.x], L);
    return;
  }
  // ---- group path: the lanes of a group stay together; groups past O, and those whose object is long, idle
  constexpr int GPB = SF_THREADS / W;
  Lanes<W> L{(int)threadIdx.x & (W - 1), nullptr, 0};
  const int g = (int)threadIdx.x / W;
  const int64_t stride = (int64_t)(gridDim.x - d.n_long) * GPB;
  for (int64_t base = (int64_t)(blockIdx.x - d.n_long) * GPB; base < d.O; base += stride) {
    const int64_t o = base + g;
    if (o < d.O && !d.obj_long[o]) sf_object<W>(d, (int)o, L);
  }
}

hipError_t launch_sync_rows(const SyncRowsDev& d, const SyncRowsRoute& r, hipStream_t st) {
  (void)hipGetLastError();
  if (r.grid > 0) hipLaunchKernelGGL(syncfin_rows_kernel, dim3((unsigned)r.grid), dim3((unsigned)r.threads), 0, st, d);
  return hipGetLastError();
}

hipError_t launch_sync_finish(const SyncFinDev& d, const SyncFinRoute& r, hipStream_t st) {
  (void)hipGetLastError();
  const unsigned grid = (unsigned)(r.grid + r.long_grid);
  if (grid > 0)
    with_width<1>(r.width, [&](auto W) {
      hipLaunchKernelGGL((syncfin_kernel<decltype(W)::value>), dim3(grid), dim3(SF_THREADS), 0, st, d);
    });
  return hipGetLastError();
}

}  // namespace kad

// ------------------------------------------------------ host half: kad_sync_needs_update / kad_sync_finish
#include "kad_arena.h"

using namespace kad;

namespace {

// what the validation leaves for the launch: the objects of the long path and the short objects' sizes
struct FinPlan {
  std::vector<uint8_t> obj_long;
  std::vector<int32_t> long_list;
  int64_t short_items = 0;
};

// a CSR of O rows of cluster ids in [0, C), strictly ascending within a row
inline bool list_bad(const int32_t* off, const int32_t* cl, int64_t O, int64_t C) {
  if (csr_bad(off, cl, O, 0, C)) return true;
  return first_bad(O, [=](int64_t i) {
           for (int64_t k = (int64_t)off[i] + 1; k < off[i + 1]; ++k)
             if (cl[k] <= cl[k - 1]) return true;
           return false;
         }) >= 0;
}

}  // namespace

extern "C" {

static int validate_sync_nu(const kad_sync_nu_batch* b, const kad_sync_nu_view* out, std::string* err) {
  auto bad = [&](const char* m) {
    *err = m;
    return KAD_EINVAL;
  };
  const int64_t C = b->n_clusters, O = b->n_objects, N = b->n_rows, V = b->n_versions;
  if (C < 0 || O < 0 || N < 0 || V < 1) return bad("negative count, or no version table");
  if (C > SF_MAX_CLUSTERS) {
    *err = "more than KAD_DISPATCH_MAX_CLUSTERS clusters";
    return KAD_EUNSUPPORTED;
  }
  if (!b->ver_flags || (O && !b->obj_flags)) return bad("input array missing");
  if (N && (!b->row_obj || !b->row_cluster || !b->row_target || !b->row_flags)) return bad("row array missing");
  const uint8_t *vf = b->ver_flags, *of = b->obj_flags, *rf = b->row_flags;
  if (vf[0] != 0 || first_bad(V, [=](int64_t i) { return (vf[i] & ~(KAD_SYNC_VER_HAS_GEN | KAD_SYNC_VER_IS_GEN)) != 0; }) >= 0)
    return bad("ver_flags: unknown flag, or flags on id 0");
  if (first_bad(O, [=](int64_t i) { return (of[i] & ~KAD_SYNC_VERSIONS_CURRENT) != 0; }) >= 0) return bad("obj_flags: unknown flag");
  if (list_bad(b->rec_off, b->rec_cluster, O, C)) return bad("rec_off / rec_cluster malformed, id outside [0, n_clusters) or not strictly ascending");
  const int64_t M = b->rec_off[O];
  const int32_t* rv = b->rec_version;
  if (M && !rv) return bad("rec_version missing");
  if (first_bad(M, [=](int64_t k) { return rv[k] < 0 || rv[k] >= V; }) >= 0) return bad("rec_version outside [0, n_versions)");
  const int32_t *ro = b->row_obj, *rc = b->row_cluster, *rt = b->row_target;
  if (first_bad(N, [=](int64_t r) {
        return ro[r] < 0 || ro[r] >= O || rc[r] < 0 || rc[r] >= C || rt[r] < 0 || rt[r] >= V || (rf[r] & ~15u) != 0;
      }) >= 0)
    return bad("a row's object, cluster or target outside its table, or an unknown row flag");
  if (!out || (N && (!out->needs_update || !out->recorded))) return bad("output view missing");
  return KAD_OK;
}

static int sync_nu_locked(kad_ctx* c, const kad_sync_nu_batch* b, const kad_sync_nu_view* out) {
  std::string err;
  if (int r = validate_sync_nu(b, out, &err)) return fail(c, r, err);
  if (b->n_rows == 0 || b->n_objects == 0) return KAD_OK;
  HIPCHK(c, hipSetDevice(c->device));
  Stage& stg = c->stage[STG_SYNCNU];
  const SyncRowsRoute route = route_sync_rows(b->n_rows, n_cus());
  const size_t n = (size_t)b->n_rows, o = (size_t)b->n_objects, m = (size_t)b->rec_off[b->n_objects];
  SyncRowsDev d{};
  d.n_rows = b->n_rows;
  Arena a;
  a.in(d.row_obj, b->row_obj, n);
  a.in(d.row_cluster, b->row_cluster, n);
  a.in(d.row_target, b->row_target, n);
  a.in(d.row_flags, b->row_flags, n);
  a.in(d.obj_flags, b->obj_flags, o);
  a.in(d.rec_off, b->rec_off, o + 1);
  a.in(d.rec_cluster, b->rec_cluster, m);
  a.in(d.rec_version, b->rec_version, m);
  a.in(d.ver_flags, b->ver_flags, (size_t)b->n_versions);
  a.out(d.needs_update, out->needs_update, n);
  a.out(d.recorded, out->recorded, n);
  HIPCHK(c, hipEventRecord(stg.ev[0], c->stream));
  if (int r = a.commit(c, stg.buf)) return r;
  HIPCHK(c, hipEventRecord(stg.ev[1], c->stream));
  HIPCHK(c, launch_sync_rows(d, route, c->stream));
  HIPCHK(c, hipEventRecord(stg.ev[2], c->stream));
  if (int r = a.fetch(c)) return r;
  HIPCHK(c, hipEventRecord(stg.ev[3], c->stream));
  stage_ran(stg, route);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return KAD_OK;
}

// With a plan (kad_sync_finish) the same pass leaves the objects of the long path.
static int validate_sync_fin(const kad_sync_fin_batch* b, const kad_sync_fin_view* out, int long_min, FinPlan* plan, std::string* err) {
  auto bad = [&](const char* m) {
    *err = m;
    return KAD_EINVAL;
  };
  const int64_t C = b->n_clusters, O = b->n_objects, V = b->n_versions, R = b->n_reasons;
  if (C < 0 || O < 0 || V < 1 || R < 3) return bad("negative count, no version table, or fewer than three reasons");
  if (C > SF_MAX_CLUSTERS) {
    *err = "more than KAD_DISPATCH_MAX_CLUSTERS clusters";
    return KAD_EUNSUPPORTED;
  }
  const int32_t rcc = b->reason_check_clusters, rnn = b->reason_ns_not_federated;
  if (rcc < 1 || rcc >= R || rnn < 1 || rnn >= R || rcc == rnn) return bad("reason_check_clusters / reason_ns_not_federated outside [1, n_reasons) or equal");
  if (!b->ver_flags || !b->ver_gen || (O && (!b->obj_flags || !b->reason_in || !b->cond_reason))) return bad("input array missing");
  const uint8_t* vf = b->ver_flags;
  if (vf[0] != 0 || first_bad(V, [=](int64_t i) { return (vf[i] & ~(KAD_SYNC_VER_HAS_GEN | KAD_SYNC_VER_IS_GEN)) != 0; }) >= 0)
    return bad("ver_flags: unknown flag, or flags on id 0");
  if (list_bad(b->sel_off, b->sel_cluster, O, C)) return bad("sel malformed, id outside [0, n_clusters) or not strictly ascending");
  if (list_bad(b->ent_off, b->ent_cluster, O, C)) return bad("ent malformed, id outside [0, n_clusters) or not strictly ascending");
  if (list_bad(b->oldv_off, b->oldv_cluster, O, C)) return bad("oldv malformed, id outside [0, n_clusters) or not strictly ascending");
  if (list_bad(b->olds_off, b->olds_cluster, O, C)) return bad("olds malformed, id outside [0, n_clusters) or not strictly ascending");
  const int32_t *eo = b->ent_off, *vo = b->oldv_off, *to = b->olds_off;
  const int64_t NE = eo[O], NV = vo[O], NT = to[O];
  if ((NE && (!b->ent_status || !b->ent_version)) || (NV && !b->oldv_version) || (NT && (!b->olds_status || !b->olds_gen)))
    return bad("list array missing");
  const uint8_t *es = b->ent_status, *ts = b->olds_status;
  const int32_t *ev = b->ent_version, *ov = b->oldv_version;
  if (first_bad(NE, [=](int64_t k) { return es[k] > KAD_SYNC_ST_MAX || ev[k] < 0 || ev[k] >= V; }) >= 0)
    return bad("ent_status: unknown code, or ent_version outside [0, n_versions)");
  if (first_bad(NV, [=](int64_t k) { return ov[k] < 1 || ov[k] >= V; }) >= 0) return bad("oldv_version outside [1, n_versions)");
  if (first_bad(NT, [=](int64_t k) { return ts[k] < 1 || ts[k] > KAD_SYNC_ST_MAX; }) >= 0) return bad("olds_status: unknown code");
  const uint16_t* of = b->obj_flags;
  const int32_t *ri = b->reason_in, *cr = b->cond_reason;
  if (first_bad(O, [=](int64_t i) {
        const uint16_t f = of[i];
        if (f & ~511u) return true;
        if ((f & KAD_SYNC_OBJ_VERSIONS_CURRENT) && !(f & KAD_SYNC_OBJ_VERSION_EXISTS)) return true;
        if ((f & KAD_SYNC_OBJ_COND_TRUE) && !(f & KAD_SYNC_OBJ_COND_EXISTS)) return true;
        if ((!(f & KAD_SYNC_OBJ_VERSION_EXISTS) || (f & KAD_SYNC_OBJ_OLDV_NIL)) && vo[i + 1] != vo[i]) return true;
        if ((f & KAD_SYNC_OBJ_STATUS_ON_HOST) && to[i + 1] != to[i]) return true;
        return ri[i] < 0 || ri[i] >= R || cr[i] < -1 || cr[i] >= R;
      }) >= 0)
    return bad("obj_flags: unknown or inconsistent flag, a list that its flags exclude, or a reason id outside its table");
  const int64_t *fo = b->ver_off, *so = b->st_off;
  if (off_bad(fo, O) || off_bad(so, O)) return bad("ver_off / st_off not monotone from 0");
  if (first_bad(O, [=](int64_t i) {
        const int64_t ne = eo[i + 1] - eo[i];
        return fo[i + 1] - fo[i] < ne + (vo[i + 1] - vo[i]) || so[i + 1] - so[i] < ne;
      }) >= 0)
    return bad("ver_off / st_off: an object's capacity is below |ent| + |oldv| / |ent|");
  if (fo[O] > INT32_MAX || so[O] > INT32_MAX) return bad("ver_off / st_off beyond 2^31 - 1 entries");
  if (!out || (O && (!out->ver_count || !out->ver_write || !out->st_count || !out->obj_out || !out->reason_out)) ||
      (fo[O] && (!out->out_ver_cluster || !out->out_ver_id)) || (so[O] && (!out->out_st_cluster || !out->out_st_status || !out->out_st_gen)))
    return bad("output view missing");
  if (plan) {
    plan->obj_long.assign((size_t)O, 0);
    for (int64_t i = 0; i < O; ++i) {
      const int64_t n = std::max<int64_t>({eo[i + 1] - eo[i], vo[i + 1] - vo[i], to[i + 1] - to[i]});
      if (n <= long_min) {
        plan->short_items += n;
        continue;
      }
      plan->obj_long[(size_t)i] = 1;
      plan->long_list.push_back((int32_t)i);
    }
  }
  return KAD_OK;
}

static int sync_fin_locked(kad_ctx* c, const kad_sync_fin_batch* b, const kad_sync_fin_view* out) {
  Stage& stg = c->stage[STG_SYNCFIN];
  const int long_min = stg.force.long_min_or(SF_LONG_MIN);
  std::string err;
  FinPlan plan;
  if (int r = validate_sync_fin(b, out, long_min, &plan, &err)) return fail(c, r, err);
  const int O = b->n_objects;
  if (O == 0) return KAD_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const int n_long = (int)plan.long_list.size();
  SyncFinRoute route = route_sync_finish(O, n_long, plan.short_items, n_cus());
  group_force_apply(stg.force, n_long < O, O, n_cus(), route.width, route.grid, &route.stride);
  route.long_min = long_min;
  const size_t o = (size_t)O, ns = (size_t)b->sel_off[O], ne = (size_t)b->ent_off[O], nv = (size_t)b->oldv_off[O],
               nt = (size_t)b->olds_off[O], V = (size_t)b->n_versions, vcap = (size_t)b->ver_off[O], scap = (size_t)b->st_off[O];
  SyncFinDev d{};
  d.O = O;
  d.n_long = n_long;
  d.reason_check = b->reason_check_clusters;
  Arena a;
  a.in(d.obj_flags, b->obj_flags, o);
  a.in(d.reason_in, b->reason_in, o);
  a.in(d.cond_reason, b->cond_reason, o);
  a.in(d.sel_off, b->sel_off, o + 1);
  a.in(d.sel_cluster, b->sel_cluster, ns);
  a.in(d.ent_off, b->ent_off, o + 1);
  a.in(d.ent_cluster, b->ent_cluster, ne);
  a.in(d.ent_status, b->ent_status, ne);
  a.in(d.ent_version, b->ent_version, ne);
  a.in(d.oldv_off, b->oldv_off, o + 1);
  a.in(d.oldv_cluster, b->oldv_cluster, nv);
  a.in(d.oldv_version, b->oldv_version, nv);
  a.in(d.olds_off, b->olds_off, o + 1);
  a.in(d.olds_cluster, b->olds_cluster, nt);
  a.in(d.olds_status, b->olds_status, nt);
  a.in(d.olds_gen, b->olds_gen, nt);
  a.in(d.ver_gen, b->ver_gen, V);
  a.in(d.ver_flags, b->ver_flags, V);
  a.in(d.ver_off, b->ver_off, o + 1);
  a.in(d.st_off, b->st_off, o + 1);
  a.in(d.obj_long, plan.obj_long.data(), o);
  a.in(d.long_list, plan.long_list.data(), (size_t)n_long);
  a.out(d.ent_pre, ne + o);
  a.out(d.oldv_pre, nv + o);
  a.out(d.out_ver_cluster, out->out_ver_cluster, vcap);
  a.out(d.out_ver_id, out->out_ver_id, vcap);
  a.out(d.ver_count, out->ver_count, o);
  a.out(d.ver_write, out->ver_write, o);
  a.out(d.out_st_cluster, out->out_st_cluster, scap);
  a.out(d.out_st_status, out->out_st_status, scap);
  a.out(d.out_st_gen, out->out_st_gen, scap);
  a.out(d.st_count, out->st_count, o);
  a.out(d.obj_out, out->obj_out, o);
  a.out(d.reason_out, out->reason_out, o);
  HIPCHK(c, hipEventRecord(stg.ev[0], c->stream));
  if (int r = a.commit(c, stg.buf)) return r;
  HIPCHK(c, hipEventRecord(stg.ev[1], c->stream));
  HIPCHK(c, launch_sync_finish(d, route, c->stream));
  HIPCHK(c, hipEventRecord(stg.ev[2], c->stream));
  if (int r = a.fetch(c)) return r;
  HIPCHK(c, hipEventRecord(stg.ev[3], c->stream));
  stage_ran(stg, route);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return KAD_OK;
}

int kad_sync_needs_update_check(const kad_sync_nu_batch* b, const kad_sync_nu_view* out) {
  return check_guarded([&]() -> int {
    if (!b) return KAD_EINVAL;
    std::string err;
    return validate_sync_nu(b, out, &err);
  });
}

int kad_sync_needs_update(kad_ctx* c, const kad_sync_nu_batch* b, const kad_sync_nu_view* out) {
  return entry(c, b != nullptr, [&]() -> int {
    return sync_nu_locked(c, b, out);
  });
}

int kad_sync_needs_update_timing(kad_ctx* c, float ms[3]) { return stage_timing(c, STG_SYNCNU, 3, ms, "no kad_sync_needs_update ran"); }

int kad_sync_needs_update_route_eval(int32_t n_rows, int32_t n_cu, int32_t* out) {
  if (!out || n_rows < 0 || n_cu < 1) return KAD_EINVAL;
  return route_record<KAD_SYNC_NU_ROUTE_FIELDS>(out, route_sync_rows(n_rows, n_cu));
}

int kad_sync_needs_update_last_route(kad_ctx* c, int32_t* out) {
  return stage_last_route(c, STG_SYNCNU, out, "no kad_sync_needs_update ran");
}

int kad_sync_finish_check(const kad_sync_fin_batch* b, const kad_sync_fin_view* out) {
  return check_guarded([&]() -> int {
    if (!b) return KAD_EINVAL;
    std::string err;
    return validate_sync_fin(b, out, SF_LONG_MIN, nullptr, &err);
  });
}

int kad_sync_finish(kad_ctx* c, const kad_sync_fin_batch* b, const kad_sync_fin_view* out) {
  return entry(c, b != nullptr, [&]() -> int {
    return sync_fin_locked(c, b, out);
  });
}

int kad_sync_finish_timing(kad_ctx* c, float ms[3]) { return stage_timing(c, STG_SYNCFIN, 3, ms, "no kad_sync_finish ran"); }

int kad_sync_finish_route_eval(int32_t n_objects, int32_t n_long, int64_t short_items, int32_t n_cu, int32_t* out) {
  if (!out || n_objects < 0 || n_long < 0 || n_long > n_objects || short_items < 0 || n_cu < 1) return KAD_EINVAL;
  return route_record<KAD_SYNC_FIN_ROUTE_FIELDS>(out, route_sync_finish(n_objects, n_long, short_items, n_cu));
}

int kad_sync_finish_last_route(kad_ctx* c, int32_t* out) { return stage_last_route(c, STG_SYNCFIN, out, "no kad_sync_finish ran"); }

int kad_sync_finish_debug_route(kad_ctx* c, int32_t force_width, int32_t force_long_min) {
  return stage_debug_route(c, STG_SYNCFIN, group_width_ok(force_width, 1), GroupForce{force_width, force_long_min, 0});
}

}  // extern "C"
