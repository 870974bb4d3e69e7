// Result application diff (§8 f3) on gfx950: which units' results change their federated object.
//
// applySchedulingResult (pkg/controllers/scheduler/scheduler.go:632-695) rewrites the scheduler's placement
// when the result's cluster SET differs from the placement's (SetPlacementNames, reflect.DeepEqual of two
// map[string]struct{}, types/v1alpha1/extensions_placements.go:78-103; an empty result deletes the placement,
// a change iff it existed) and the replicas overrides when OverrideUpdateNeeded (scheduler/util.go:154-185)
// finds a replicas-path patch whose value is not a float64, whose cluster has no replica count in the result,
// or whose int64(value) differs from it, or when the number of matching patches is not the number of result
// entries with a replica count. One lane per unit: the result slots of a unit are ascending cluster
// positions (every schedule / plan kernel writes them so), the canonical placement ids too (host-sorted,
// unique), so the set test is one pass and each patch a binary search.
#include "kad_device.h"

namespace kad {

__global__ __launch_bounds__(256) void result_diff_kernel(ResultDiffDev d) {
  const int w = (int)(blockIdx.x * 256 + threadIdx.x);
  if (w >= d.W) return;
  const int32_t st = d.status[w];
  uint32_t f = 0;
  if (st == KAD_ST_ERR_SCORE || st == KAD_ST_ERR_SELECT || st == KAD_ST_ERR_REPLICAS) {
    d.out[w] = KAD_DIFF_SKIP;  // Schedule returned an error: nothing is applied
    return;
  }
  if (st == KAD_ST_STICKY) {
    d.out[w] = KAD_DIFF_STICKY;
    return;
  }
  const int n = st == KAD_ST_OK ? d.count[w] : 0;  // NO_FEASIBLE: the nil map
  const int32_t* cl = d.cluster + d.out_off[w];
  const int64_t* rp = d.replicas + d.out_off[w];
  // ---- placement: SetPlacementNames(controller, result cluster set)
  const uint8_t uf = d.uflag[w];
  const int p0 = d.pl_off[w], np = d.pl_off[w + 1] - p0;
  bool pc;
  if (n == 0) {
    pc = uf & 1;  // DeletePlacement: a change iff the placement existed
  } else {
    pc = (uf & 2) || np != n;  // a name outside the snapshot never is in the result
    for (int i = 0; !pc && i < n; ++i) pc = d.pl_id[p0 + i] != cl[i];
  }
  if (pc) f |= KAD_DIFF_PLACEMENT;
  // ---- overrides: OverrideUpdateNeeded(typeConfig, overrides, {cluster: replicas} of the non-nil counts)
  int nres = 0;
  for (int i = 0; i < n; ++i) nres += rp[i] >= 0;  // Duplicate results carry nil (-1) counts
  const int o0 = d.ov_off[w], o1 = d.ov_off[w + 1];
  bool oc = false;
  int checked = 0;
  for (int o = o0; o < o1 && !oc; ++o) {
    if (d.ov_kind[o] != 0) {
      oc = true;  // the value is not a float64
      break;
    }
    const int id = d.ov_id[o];
    int lo = 0, hi = n;  // first slot with cluster >= id
    while (lo < hi) {
      const int mid = (lo + hi) >> 1;
      if (cl[mid] < id)
        lo = mid + 1;
      else
        hi = mid;
    }
    if (id < 0 || lo >= n || cl[lo] != id || rp[lo] < 0 || rp[lo] != d.ov_val[o]) oc = true;
    ++checked;
  }
  if (oc || checked != nres) f |= KAD_DIFF_OVERRIDES;
  d.out[w] = f;
}

hipError_t launch_result_diff(const ResultDiffDev& d, hipStream_t st) {
  if (d.W <= 0) return hipSuccess;
  result_diff_kernel<<<(unsigned)((d.W + 255) / 256), 256, 0, st>>>(d);
  return hipGetLastError();
}

}  // namespace kad

// ------------------------------------------------------ host half: kad_result_diff
#include "kad_arena.h"

using namespace kad;

extern "C" {

int kad_result_diff(kad_ctx* c, const kad_result_state* st, uint32_t* out) {
  return entry(c, st && out, [&]() -> int {
    if (!c->ran || !c->have_batch) return fail(c, KAD_ESTATE, "no scheduled batch resident");
    // this ctx's units (a kad_group member: its shard, whose out_off keeps the batch-wide slot numbers that
    // out_dev's shifted slot arrays are indexed by)
    const int W = (int)c->unit_n, C = c->sd.C;
    if (st->n_units != W) return fail(c, KAD_EINVAL, "state n_units differs from the resident batch");
    if (W == 0) return KAD_OK;
    if (!st->place_off || !st->place_has || !st->ovr_off) return fail(c, KAD_EINVAL, "null state array");
    if (off_bad(st->place_off, W) || off_bad(st->ovr_off, W)) return fail(c, KAD_EINVAL, "state offsets not monotone from 0");
    const int64_t NP = st->place_off[W], NO = st->ovr_off[W];
    if ((NP && !st->place_cluster) || (NO && (!st->ovr_cluster || !st->ovr_value || !st->ovr_kind)))
      return fail(c, KAD_EINVAL, "null state array");
    if (csr_bad(st->place_off, st->place_cluster, W, -1, C)) return fail(c, KAD_EINVAL, "placement cluster out of range");
    if (csr_bad(st->ovr_off, st->ovr_cluster, W, -1, C)) return fail(c, KAD_EINVAL, "override cluster out of range");
    // canonical placements: sorted unique snapshot positions; names outside the snapshot → uflag bit 1
    std::vector<int32_t> cnt((size_t)W + 1, 0);
    std::vector<uint8_t> uflag((size_t)W);
    std::vector<int32_t> ids((size_t)NP);
    host_parallel(W, [&](int lo, int hi) {
      for (int w = lo; w < hi; w++) {
        int32_t* b = ids.data() + st->place_off[w];
        const int m = st->place_off[w + 1] - st->place_off[w];
        std::copy(st->place_cluster + st->place_off[w], st->place_cluster + st->place_off[w + 1], b);
        std::sort(b, b + m);
        const int u = (int)(std::unique(b, b + m) - b);
        const bool unknown = u > 0 && b[0] < 0;
        cnt[(size_t)w + 1] = unknown ? u - 1 : u;
        if (unknown) std::copy(b + 1, b + u, b);  // drop the -1
        uflag[w] = (uint8_t)((st->place_has[w] ? 1 : 0) | (unknown ? 2 : 0));
      }
    });
    std::vector<int32_t> pl_off((size_t)W + 1, 0);
    for (int w = 0; w < W; w++) pl_off[(size_t)w + 1] = pl_off[w] + cnt[(size_t)w + 1];
    std::vector<int32_t> pl_id((size_t)pl_off[W] + 1);
    host_parallel(W, [&](int lo, int hi) {
      for (int w = lo; w < hi; w++)
        std::copy(ids.data() + st->place_off[w], ids.data() + st->place_off[w] + cnt[(size_t)w + 1], pl_id.data() + pl_off[w]);
    });
    // one device buffer: [pl_off | pl_id | ov_off | ov_id | ov_val | uflag | ov_kind | out]; the kernel may read
    // one element past pl_id, ov_id, ov_val and ov_kind
    const size_t w = (size_t)W, no = (size_t)NO;
    ResultDiffDev dd{};
    dd.W = W;
    dd.status = c->d_status;
    dd.count = c->d_count;
    const OutDev od = out_dev(c);
    dd.cluster = od.cluster;
    dd.replicas = od.replicas;
    dd.out_off = c->bd.out_off;
    Arena a;
    a.in(dd.pl_off, pl_off.data(), w + 1);
    a.in(dd.pl_id, pl_id.data(), (size_t)pl_off[W], 1);
    a.in(dd.ov_off, st->ovr_off, w + 1);
    a.in(dd.ov_id, st->ovr_cluster, no, 1);
    a.in(dd.ov_val, st->ovr_value, no, 1);
    a.in(dd.uflag, uflag.data(), w);
    a.in(dd.ov_kind, st->ovr_kind, no, 1);
    a.out(dd.out, out, w);
    HIPCHK(c, hipSetDevice(c->device));
    if (int r = a.commit(c, c->stage[STG_DIFF].buf)) return r;
    HIPCHK(c, launch_result_diff(dd, c->stream));
    if (int r = a.fetch(c)) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));  // the caller's state arrays are free on return
    return KAD_OK;
  });
}

}  // extern "C"
