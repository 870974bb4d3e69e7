// Filter diagnosis (kad_explain): which filter plugin rejects which cluster for the listed units.
//
// filter_explain_kernel — one 64-lane wavefront per listed unit. Same predicates as schedule_kernel's
// phase A (findClustersThatFitWorkload, core/generic_scheduler.go:152-169), but the five filters stay apart:
// RunFilterPlugins stops at the first plugin that does not succeed, in the framework's filter order
// (framework/runtime/framework.go:114-126), so each cluster is attributed to that plugin. The order is the
// one thing kad_profile does not carry (its filters are a mask); it travels in the kernel's arguments.
// Nothing here writes state that kad_schedule reads.
#include "kad_affinity.h"
#include "kad_device.h"
#include "kad_wave.h"

namespace kad {

constexpr int EXPLAIN_WAVES = 4;            // waves (units) per block while their bitmaps fit EXPLAIN_LDS
constexpr size_t EXPLAIN_LDS = 32 * 1024;   // else one wave per block: 16 KB at the 65535-cluster limit

// The argument block is read through the kernarg segment pointer, laundered per unit and per chunk (as
// schedule_kernel's kargs()): argument loads then sit next to their uses instead of being hoisted to the
// entry, where the ~80 pointers of the snapshot and batch views overflow the SGPR file.
typedef const __attribute__((address_space(4))) ExplainArgs* XArgs;
__device__ __forceinline__ XArgs xargs() {
  return (XArgs)opq((uintptr_t)__builtin_amdgcn_kernarg_segment_ptr());
}

__global__ __launch_bounds__(256) void filter_explain_kernel(ExplainArgs args) {
  (void)args;  // read through xargs()
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = lane_id();
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  const int wpb = blockDim.x >> 6;
  int C, TW, n_units, n_order;
  uint32_t fm, order;
  {
    XArgs a = xargs();
    C = a->s.C;
    TW = a->s.TW;
    n_units = a->n_units;
    n_order = a->n_order;
    fm = a->filter_mask;
    order = a->order;
  }
  const int nch = (C + 63) >> 6;
  // per wave: PlacementFilter's ClusterNames and the unit's CurrentClusters as cluster bitmaps
  uint64_t* plb = reinterpret_cast<uint64_t*>(smem) + (size_t)wv * 2 * nch;
  uint64_t* curb = plb + nch;
  const bool f_api = fm & (1u << KAD_PL_API_RESOURCES), f_taint = fm & (1u << KAD_PL_TAINT_TOLERATION);
  const bool f_fit = fm & (1u << KAD_PL_CLUSTER_RESOURCES_FIT), f_place = fm & (1u << KAD_PL_PLACEMENT_FILTER);
  const bool f_aff = fm & (1u << KAD_PL_CLUSTER_AFFINITY);

  for (int i = blockIdx.x * wpb + wv; i < n_units; i += gridDim.x * wpb) {
    XArgs a = xargs();
    const int w = ldc(a->units + i);
    const uint32_t f = ldc(a->b.flags + w);
    uint8_t* ff = a->first_fail ? a->first_fail + (size_t)i * C : nullptr;
    // wave-uniform counters (ballot popcounts): scalar registers, written once by lane 0
    int rej[5] = {0, 0, 0, 0, 0}, fit[3] = {0, 0, 0}, feas = 0;
    if (f & KAD_W_STICKY) {  // generic_scheduler.go:101-104: the unit keeps its clusters, no filter runs
      feas = -1;
      if (ff)
        for (int c = lane; c < C; c += WAVE) ff[c] = 0xFF;
    } else {
      const bool use_place = f_place && (f & KAD_W_HAS_PLACEMENT);
      const bool use_cur = f_taint && (f & KAD_W_HAS_CURRENT);
      if (use_place || use_cur) {
        wave_sync();  // the previous unit's reads of the bitmaps
        for (int j = lane; j < nch; j += WAVE) {
          plb[j] = 0;
          curb[j] = 0;
        }
        wave_sync();
        if (use_place)
          for (int j = ldc(a->b.place_off + w) + lane; j < ldc(a->b.place_off + w + 1); j += WAVE) {
            const int c = ldg(a->b.place, (uint32_t)j);
            atomicOr((unsigned long long*)&plb[c >> 6], 1ull << (c & 63));
          }
        if (use_cur)
          for (int j = ldc(a->b.cur_off + w) + lane; j < ldc(a->b.cur_off + w + 1); j += WAVE) {
            const int c = ldg(a->b.cur_id, (uint32_t)j);
            atomicOr((unsigned long long*)&curb[c >> 6], 1ull << (c & 63));
          }
        wave_sync();
      }
      const int gv = ldc(a->b.gvk + w);
      const uint64_t* tolA = a->b.tol_all + (size_t)ldc(a->b.tolset + w) * TW;
      const int64_t rq_cpu = ldc(a->b.req_cpu + w), rq_mem = ldc(a->b.req_mem + w);
      const bool fit_on = f_fit && (f & KAD_W_FIT_NONZERO);  // fit.go:82-87: a zero request fits everywhere
      const int s0 = ldc(a->b.sreq_off + w), s1 = ldc(a->b.sreq_off + w + 1);
      ProgRegs FP{nullptr, 0};
      if (f_aff) {
        const int fo = ldc(a->b.fprog_off + w), fl = ldc(a->b.fprog_off + w + 1) - fo;
        FP = load_prog(a->b.fprog + fo, fl);
      }
      uint64_t affv = ~0ull;
      for (int ch = 0; ch < nch; ++ch) {
        XArgs a = xargs();
        // lane l of affinity_filter_chunks holds chunk ch + l: one evaluation serves 64 chunks
        if (f_aff && (ch & 63) == 0) affv = affinity_filter_chunks(a->b.req_mask, FP, nch, ch);
        const int c = ch * WAVE + lane;
        const uint32_t cl = c < C ? (uint32_t)c : 0u;
        bool bad_api = false, bad_taint = false, bad_place = false, bad_aff = false;
        bool no_cpu = false, no_mem = false, no_scalar = false;
        if (f_api) {  // api_resources.go:42-63 (gv < 0: no cluster lists the unit's GroupVersionKind)
          bad_api = true;
          if (gv >= 0) bad_api = !((ldg(a->s.gvk, (uint32_t)((gv >> 6) * C) + cl) >> (gv & 63)) & 1);
        }
        if (f_taint) {  // taint_toleration.go:50-77: NoExecute only on the clusters the unit is already in
          const bool sch = use_cur && ((curb[ch] >> lane) & 1);
          for (int t = 0; t < TW; ++t) {
            uint64_t x = ldg(a->s.nsne, (uint32_t)(t * C) + cl);
            if (use_cur) {
              const uint64_t y = ldg(a->s.ne, (uint32_t)(t * C) + cl);
              x = sch ? y : x;
            }
            bad_taint |= (x & ~ldc(tolA + t)) != 0;
          }
        }
        if (fit_on) {  // fit.go:73-134 collects every short resource (Go's wrapping add)
          no_cpu = ldg(a->s.alloc_cpu, cl) < wadd(rq_cpu, ldg(a->s.used_cpu, cl));
          no_mem = ldg(a->s.alloc_mem, cl) < wadd(rq_mem, ldg(a->s.used_mem, cl));
          for (int j = s0; j < s1; ++j) {
            const int sid = ldc(a->b.sreq_id + j);
            const int64_t v = ldc(a->b.sreq_val + j);
            int64_t al = 0, us = 0;  // a scalar no cluster has (id -1): allocatable 0, used 0
            if (sid >= 0) {
              al = ldg(a->s.alloc_s, (uint32_t)(sid * C) + cl);
              us = ldg(a->s.used_s, (uint32_t)(sid * C) + cl);
            }
            no_scalar |= al < wadd(v, us);
          }
        }
        if (use_place) bad_place = !((plb[ch] >> lane) & 1);
        if (f_aff) bad_aff = !((readlane64(affv, ch & 63) >> lane) & 1);
        const bool bad_fit = no_cpu | no_mem | no_scalar;

        uint64_t remaining = ballot(c < C);
        int code = 0xFF;
        for (int k = 0; k < n_order; ++k) {
          const int pl = (int)((order >> (4 * k)) & 15u);
          const bool bad = pl == KAD_PL_API_RESOURCES           ? bad_api
                           : pl == KAD_PL_TAINT_TOLERATION      ? bad_taint
                           : pl == KAD_PL_CLUSTER_RESOURCES_FIT ? bad_fit
                           : pl == KAD_PL_PLACEMENT_FILTER      ? bad_place
                                                                : bad_aff;
          const uint64_t m = ballot(bad) & remaining;
          const int n = popc64(m);
#pragma unroll
          for (int p = 0; p < 5; ++p) rej[p] += pl == p ? n : 0;
          if (pl == KAD_PL_CLUSTER_RESOURCES_FIT) {
            fit[0] += popc64(ballot(no_cpu) & m);
            fit[1] += popc64(ballot(no_mem) & m);
            fit[2] += popc64(ballot(no_scalar) & m);
          }
          if ((m >> lane) & 1) code = pl;
          remaining &= ~m;
        }
        feas += popc64(remaining);
        if (ff && c < C) ff[c] = (uint8_t)code;
      }
    }
    if (lane == 0) {
#pragma unroll
      for (int p = 0; p < 5; ++p) a->rejected[(size_t)i * 5 + p] = rej[p];
      a->feasible[i] = feas;
      if (a->fit_detail) {
#pragma unroll
        for (int k = 0; k < 3; ++k) a->fit_detail[(size_t)i * 3 + k] = fit[k];
      }
    }
  }
}

hipError_t launch_explain(const ExplainArgs& a, hipStream_t st) {
  (void)hipGetLastError();
  if (a.n_units <= 0) return hipSuccess;
  const size_t per_wave = 2 * 8 * (size_t)((a.s.C + 63) >> 6);
  const int wpb = EXPLAIN_WAVES * per_wave <= EXPLAIN_LDS ? EXPLAIN_WAVES : 1;
  const int blocks = (a.n_units + wpb - 1) / wpb;
  hipLaunchKernelGGL(filter_explain_kernel, dim3((unsigned)(blocks < 2048 ? blocks : 2048)), dim3(64 * wpb),
                     wpb * per_wave, st, a);
  return hipGetLastError();
}

}  // namespace kad

// ------------------------------------------------------ host half: kad_explain
#include "kad_arena.h"

using namespace kad;

extern "C" {

// The filter diagnosis of the listed units (kad_explain.hip). Reads the resident snapshot and batch and the
// requirement rows (rebuilt here by the launch schedule_locked uses: ~10 us at the bench sizes, and no
// currency flag to keep through every upload and update path); writes only its own buffer.
int kad_explain(kad_ctx* c, const kad_profile* p, const int32_t* order, int n_order, const int32_t* unit_idx,
                int n_units, const kad_explain_view* out) {
  return entry(c, true, [&]() -> int {
    if (!c->have_snapshot || !c->have_batch) return fail(c, KAD_ESTATE, "snapshot and batch must be uploaded first");
    if (int r = validate_profile(c, p)) return r;
    if (p->filter_mask != c->batch_hdr.packed_filter_mask)
      return fail(c, KAD_EINVAL, "profile differs from the one the batch was packed for");
    if (n_order < 0 || n_order > 5 || (n_order && !order)) return fail(c, KAD_EINVAL, "filter order: 0..5 plugin ids");
    uint32_t seen = 0, packed = 0;
    for (int k = 0; k < n_order; k++) {
      if (order[k] < 0 || order[k] > KAD_PL_CLUSTER_AFFINITY || (seen >> order[k] & 1))
        return fail(c, KAD_EINVAL, "filter order: not a filter plugin id, or listed twice");
      seen |= 1u << order[k];
      packed |= (uint32_t)order[k] << (4 * k);
    }
    if (seen != p->filter_mask) return fail(c, KAD_EINVAL, "filter order is not a permutation of the profile's filter mask");
    if (n_units < 0 || (n_units && (!unit_idx || !out || !out->rejected || !out->feasible)))
      return fail(c, KAD_EINVAL, "unit list or output view missing");
    const int W = c->bd.W;
    for (int i = 0; i < n_units; i++)
      if (unit_idx[i] < 0 || unit_idx[i] >= W)
        return fail(c, KAD_EINVAL, "unit_idx[" + std::to_string(i) + "] = " + std::to_string(unit_idx[i]) +
                                       " outside the batch's " + std::to_string(W) + " units");
    if (n_units == 0) return KAD_OK;
    HIPCHK(c, hipSetDevice(c->device));
    const size_t n = (size_t)n_units, C = (size_t)c->sd.C;
    ExplainArgs a{};
    a.s = c->sd;
    a.b = c->bd;
    a.filter_mask = p->filter_mask;
    a.order = packed;
    a.n_order = n_order;
    a.n_units = n_units;
    Arena ar;
    ar.in(a.units, unit_idx, n);
    ar.out(a.rejected, out->rejected, 5 * n);
    ar.out(a.feasible, out->feasible, n);
    if (out->fit_detail)
      ar.out(a.fit_detail, out->fit_detail, 3 * n);
    else
      ar.absent(a.fit_detail);
    if (out->first_fail)
      ar.out(a.first_fail, out->first_fail, n * C);
    else
      ar.absent(a.first_fail);
    Stage& stg = c->stage[STG_EXPLAIN];
    if (int r = ar.commit(c, stg.buf)) return r;
    HIPCHK(c, hipEventRecord(stg.ev[0], c->stream));
    bool zeroed = false;
    HIPCHK(c, launch_req_masks(c->sd, c->bd, c->stream, false, &zeroed));
    HIPCHK(c, hipEventRecord(stg.ev[1], c->stream));
    HIPCHK(c, launch_explain(a, c->stream));
    HIPCHK(c, hipEventRecord(stg.ev[2], c->stream));
    stg.ran = true;
    if (int r = ar.fetch(c)) return r;
    HIPCHK(c, hipStreamSynchronize(c->stream));
    return KAD_OK;
  });
}

int kad_explain_timing(kad_ctx* c, float ms[2]) { return stage_timing(c, STG_EXPLAIN, 2, ms, "no kad_explain ran"); }

}  // extern "C"
