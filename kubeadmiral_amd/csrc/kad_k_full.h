// schedule_kernel: the full kernel, one wavefront per unit, every feature (the defer list's consumer).
// Part of kad_kernels.hip's translation unit, which includes the kernels' headers in definition order.
#pragma once

#include "kad_affinity.h"
#include "kad_device.h"
#include "kad_kargs.h"
#include "kad_prof.h"
#include "kad_score.h"
#include "kad_select.h"
#include "kad_wave.h"

namespace kad {

struct SchedArgs {
  SnapDev s;
  BatchDev b;
  OutDev o;
  ProfDev p;
  char* gscratch;
  int wave_bytes, waves_per_block, w_stride;
  const int32_t* list;    // non-null: schedule units list[0 .. *list_n) (the lean kernel's defer list)
  const int32_t* list_n;
};
typedef const __attribute__((address_space(4))) SchedArgs* KArgs;

template <bool GSCR>
__global__ __launch_bounds__(256) void schedule_kernel(SchedArgs args) {
  (void)args;  // read through kernarg<SchedArgs>()
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = lane_id();
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);  // wave-uniform: per-unit loads go scalar
  int gw, w_stride, C, TW, W;
  char* region;
  uint32_t fm, sm;
  int xs_b, xs_c;
  {
    KArgs a = kernarg<SchedArgs>();
    const int wpb = a->waves_per_block, wbytes = a->wave_bytes;
    gw = blockIdx.x * wpb + wv;
    w_stride = a->w_stride;
    region = GSCR ? a->gscratch + (size_t)gw * wbytes : smem + (size_t)wv * wbytes;
    C = a->s.C;
    TW = a->s.TW;
    W = a->list ? *a->list_n : a->b.W;  // (no host launch leaves the list out any more: launch_defer_pass alone)
    fm = a->p.filter_mask;
    sm = a->p.score_mask;
    xs_b = (a->p.flags & KAD_PROFILE_XORSHIFT_GO121) ? 7 : 17;
    xs_c = (a->p.flags & KAD_PROFILE_XORSHIFT_GO121) ? 17 : 5;
  }
  const RowLayout L = row_layout(C);
  int64_t* tot = (int64_t*)(region + L.tot);
  uint32_t* fx = (uint32_t*)(region + L.fx);
  uint16_t* idx = (uint16_t*)(region + L.idx);
  uint16_t* perm = (uint16_t*)(region + L.perm);
  const SmallLayout SL = small_layout(C);
  uint64_t* selb = (uint64_t*)(GSCR ? smem + SL.sel : region + L.sel);
  uint64_t* plb = (uint64_t*)(GSCR ? smem + SL.place : region + L.place);
  uint64_t* curb = (uint64_t*)(GSCR ? smem + SL.cur : region + L.cur);
  uint32_t* hist = (uint32_t*)(GSCR ? smem + SL.hist : region + L.hist);
  uint16_t* posl = (uint16_t*)(region + L.posl);
  uint16_t* posr = (uint16_t*)(region + L.posr);
  const int nch = (C + 63) >> 6;
  const bool f_taint = fm & BIT(KAD_PL_TAINT_TOLERATION), f_api = fm & BIT(KAD_PL_API_RESOURCES);
  const bool f_aff = fm & BIT(KAD_PL_CLUSTER_AFFINITY), f_place = fm & BIT(KAD_PL_PLACEMENT_FILTER);

  KAD_PACC;
  for (int wi = gw; wi < W; wi += w_stride) {
    KAD_PT(t0);
    KArgs a = kernarg<SchedArgs>();
    const int w = a->list ? ldc(a->list + wi) : wi;
    const uint32_t f = ldc(a->b.flags + w);
    if (f & KAD_W_STICKY) {  // generic_scheduler.go:101-104
      unit_status(a, w, KAD_ST_STICKY);
      continue;
    }
    const bool use_place = f_place && (f & KAD_W_HAS_PLACEMENT);
    const bool use_cur = f_taint && (f & KAD_W_HAS_CURRENT);
    if (use_place || use_cur) {
      for (int i = lane; i < nch; i += WAVE) {
        plb[i] = 0;
        curb[i] = 0;
      }
      wsync<GSCR>();
      if (use_place) {
        const int32_t* pl = a->b.place;
        for (int j = ldc(a->b.place_off + w) + lane; j < ldc(a->b.place_off + w + 1); j += WAVE) {
          const int c = ldg(pl, (uint32_t)j);
          atomicOr((unsigned long long*)&plb[c >> 6], 1ull << (c & 63));
        }
      }
      if (use_cur) {
        const int32_t* cu = a->b.cur_id;
        for (int j = ldc(a->b.cur_off + w) + lane; j < ldc(a->b.cur_off + w + 1); j += WAVE) {
          const int c = ldg(cu, (uint32_t)j);
          atomicOr((unsigned long long*)&curb[c >> 6], 1ull << (c & 63));
        }
      }
      wsync<GSCR>();
    }
    const int gv = ldc(a->b.gvk + w);
    const int ts = ldc(a->b.tolset + w);
    const int64_t rq_cpu = ldc(a->b.req_cpu + w), rq_mem = ldc(a->b.req_mem + w);
    const bool fit_on = (fm & BIT(KAD_PL_CLUSTER_RESOURCES_FIT)) && (f & KAD_W_FIT_NONZERO);
    const int s0 = ldc(a->b.sreq_off + w), s1 = ldc(a->b.sreq_off + w + 1);
    ProgRegs FP{nullptr, 0};
    if (f_aff) {
      const int fo = ldc(a->b.fprog_off + w), fl = ldc(a->b.fprog_off + w + 1) - fo;
      FP = load_prog(a->b.fprog + fo, fl);
    }

    // ---------------- A: filters → compacted feasible list (findClustersThatFitWorkload, :152-169)
    // Per chunk of 64 clusters every attribute load is unconditional, so one
    // memory round trip serves all filters; ClusterAffinity comes from the
    // lane-per-chunk bitmask evaluation.
    int n = 0;
    uint64_t affv = ~0ull;
    for (int ch = 0; ch < nch; ++ch) {
      KArgs ac = kernarg<SchedArgs>();
      if (f_aff && (ch & 63) == 0) affv = affinity_filter_chunks(ac->b.req_mask, FP, nch, ch);
      const int c = ch * WAVE + lane;
      const uint32_t cl = c < C ? (uint32_t)c : 0u;
      bool ok = c < C;
      if (f_aff) ok &= (readlane64(affv, ch & 63) >> lane) & 1;
      if (use_place) ok &= (plb[ch] >> lane) & 1;
      if (f_taint) {  // taint_toleration.go:50-77: NoSchedule/NoExecute (NoExecute only if not yet scheduled)
        const uint64_t* tolA = ac->b.tol_all + (size_t)ts * TW;
        const uint64_t* nsne = ac->s.nsne;
        const uint64_t* ne = ac->s.ne;
        const bool sch = use_cur && ((curb[ch] >> lane) & 1);
        for (int t = 0; t < TW; ++t) {
          uint64_t x = ldg(nsne, (uint32_t)(t * C) + cl);
          if (use_cur) {
            const uint64_t y = ldg(ne, (uint32_t)(t * C) + cl);
            x = sch ? y : x;
          }
          ok &= (x & ~ldc(tolA + t)) == 0;
        }
      }
      if (f_api) {  // api_resources.go:42-63
        if (gv >= 0)
          ok &= (ldg(ac->s.gvk, (uint32_t)((gv >> 6) * C) + cl) >> (gv & 63)) & 1;
        else
          ok = false;
      }
      if (fit_on) {  // cluster_resources_fit.go:48-90
        const int64_t acpu = ldg(ac->s.alloc_cpu, cl), ucpu = ldg(ac->s.used_cpu, cl);
        const int64_t amem = ldg(ac->s.alloc_mem, cl), umem = ldg(ac->s.used_mem, cl);
        ok &= (int)(acpu >= wadd(rq_cpu, ucpu)) & (int)(amem >= wadd(rq_mem, umem));
        for (int j = s0; j < s1; ++j) {
          KArgs aj = kernarg<SchedArgs>();
          const int sid = ldc(aj->b.sreq_id + j);
          const int64_t v = ldc(aj->b.sreq_val + j);
          int64_t al = 0, us = 0;
          if (sid >= 0) {
            al = ldg(aj->s.alloc_s, (uint32_t)(sid * C) + cl);
            us = ldg(aj->s.used_s, (uint32_t)(sid * C) + cl);
          }
          ok &= al >= wadd(v, us);
        }
      }
      const uint64_t m = ballot(ok);
      if (ok) idx[n + mbcnt(m)] = (uint16_t)c;  // compact feasible clusters, snapshot order
      n += popc64(m);
      uint8_t* dbg = ac->o.dbg_feas;
      if (dbg && c < C) dbg[(size_t)w * C + c] = ok;
    }
    KAD_PT(t1);
    KAD_PADD(0, t1 - t0);
    if (n == 0) {  // generic_scheduler.go:112-114
      unit_status(kernarg<SchedArgs>(), w, KAD_ST_NO_FEASIBLE);
      continue;
    }
    if ((sm & BIT(KAD_PL_CLUSTER_AFFINITY)) && (f & KAD_W_SCORE_ERROR)) {  // framework.go:149-159
      unit_status(kernarg<SchedArgs>(), w, KAD_ST_ERR_SCORE);
      continue;
    }
    wsync<GSCR>();

    // ---------------- B: raw scores on the compacted feasible list (RunScorePlugins, framework.go:139-181)
    int ttmax = 0;
    int64_t affmax = 0;
    {
      KArgs ab = kernarg<SchedArgs>();
      const uint64_t* tolP = ab->b.tol_pns + (size_t)ts * TW;
      const int32_t* sp = ab->b.sprog + ldc(ab->b.sprog_off + w);
      for (int j = lane; j < n; j += WAVE) {
        const uint32_t c = idx[j];
        int64_t fixed = 0;
        if (sm & (BIT(KAD_PL_LEAST_ALLOCATED) | BIT(KAD_PL_MOST_ALLOCATED) | BIT(KAD_PL_BALANCED_ALLOCATION))) {
          const int64_t rc = wadd(ldg(ab->s.used_cpu, c), rq_cpu), rm = wadd(ldg(ab->s.used_mem, c), rq_mem);
          const int64_t cc = ldg(ab->s.alloc_cpu, c), cm = ldg(ab->s.alloc_mem, c);
          if (sm & BIT(KAD_PL_LEAST_ALLOCATED))
            fixed += go_div(wadd(least_requested(rm, cm), least_requested(rc, cc)), 2);
          if (sm & BIT(KAD_PL_MOST_ALLOCATED))
            fixed += go_div(wadd(most_requested(rm, cm), most_requested(rc, cc)), 2);
          if (sm & BIT(KAD_PL_BALANCED_ALLOCATION)) fixed += balanced(rc, cc, rm, cm);
        }
        int tt = 0;
        if (sm & BIT(KAD_PL_TAINT_TOLERATION))
          for (int t = 0; t < TW; ++t) tt += popc64(ldg(ab->s.pns, (uint32_t)(t * C) + c) & ~ldc(tolP + t));
        int64_t aff = 0;
        if (sm & BIT(KAD_PL_CLUSTER_AFFINITY)) aff = affinity_score(ab->b.req_mask, sp, nch, c);
        fx[j] = (uint32_t)fixed | ((uint32_t)tt << 16);
        tot[j] = aff;
        ttmax = tt > ttmax ? tt : ttmax;
        affmax = aff > affmax ? aff : affmax;
      }
    }
    if (sm & BIT(KAD_PL_TAINT_TOLERATION)) ttmax = wave_max_u_i32(ttmax);
    if (sm & BIT(KAD_PL_CLUSTER_AFFINITY)) affmax = wave_max_u_i64(affmax);
    wsync<GSCR>();
    KAD_PT(t2);
    KAD_PADD(1, t2 - t1);

    // ---------------- C: DefaultNormalizeScore (framework/util.go:455-483) + sum
    int64_t rmin = I64_MAX, rmax = I64_MIN;
    {
      int64_t* dbt = kernarg<SchedArgs>()->o.dbg_total;
      for (int j = lane; j < n; j += WAVE) {
        const uint32_t x = fx[j];
        int64_t t = (int64_t)(x & 0xFFFF);
        if (sm & BIT(KAD_PL_TAINT_TOLERATION))
          t += ttmax == 0 ? 100 : 100 - (int64_t)small_quot(100 * (int)(x >> 16), ttmax);
        if (sm & BIT(KAD_PL_CLUSTER_AFFINITY)) {
          const int64_t av = tot[j];
          t = wadd(t, affmax == 0 ? av : div_fast(wmul(100, av), affmax));
        }
        tot[j] = t;
        rmin = t < rmin ? t : rmin;
        rmax = t > rmax ? t : rmax;
        if (dbt) dbt[(size_t)w * C + idx[j]] = t;
      }
    }
    rmin = wave_min_u_i64(rmin);
    rmax = wave_max_u_i64(rmax);
    wsync<GSCR>();
    KAD_PT(t3);
    KAD_PADD(2, t3 - t2);

    // ---------------- D: select (framework.go:183-209, max_cluster.go:42-66)
    int64_t k = n;
    {
      KArgs ad = kernarg<SchedArgs>();
      if (ad->p.select_plugin == KAD_PL_MAX_CLUSTER) {
        const bool hm = f & KAD_W_HAS_MAX_CLUSTERS;
        const int64_t mc = ldc(ad->b.maxc + w);
        if (hm && mc < 0) {
          unit_status(ad, w, KAD_ST_ERR_SELECT);
          continue;
        }
        if (hm && mc < k) k = mc;
      }
    }
    SelWs ws{tot, selb, perm, hist, posl, posr};
    const uint32_t rflags = select_topk<GSCR>(ws, n, k, rmin, rmax, xs_b, xs_c);
    KAD_PT(t4);
    KAD_PADD(3, t4 - t3);
    KAD_PADD(6, 1);
    KAD_PADD(7, n);
    if (rflags & KAD_RF_TIE_STRADDLE) {
      KAD_PADD(5, 1);
      KAD_PADD(8, t4 - t3);
    }

    // ---------------- E: output, ascending cluster id (idx is ascending in j)
    {
      KArgs ae = kernarg<SchedArgs>();
      const bool dup = f & KAD_W_DUPLICATE;
      const bool replicas = !dup && ae->p.replicas_plugin == KAD_PL_CLUSTER_CAPACITY_WEIGHT &&
                            (f & KAD_W_HAS_DESIRED) && ldc(ae->b.desired + w) > 0 && k > 0;
      if (dup || replicas) {
        const int64_t off = ldc(ae->b.out_off + w);
        int32_t* oc = ae->o.cluster + off;
        int64_t* orp = ae->o.replicas + off;
        int base = 0;
        for (int jc = 0; jc < ((n + 63) >> 6); ++jc) {
          const uint64_t m = selb[jc];
          if ((m >> lane) & 1) {
            const uint32_t at = (uint32_t)(base + mbcnt(m));
            stg(oc, at, (int32_t)idx[jc * WAVE + lane]);
            stg(orp, at, (int64_t)(dup ? -1 : 0));
          }
          base += popc64(m);
        }
      }
      if (lane == 0) {
        ae->o.status[w] = KAD_ST_OK;
        ae->o.count[w] = (dup || replicas) ? (int32_t)k : 0;  // Divide without replicas plugin: empty map
        ae->o.flags[w] = rflags;
      }
    }
    wsync<GSCR>();
    KAD_PT(t5);
    KAD_PADD(4, t5 - t4);
  }
  KAD_PFLUSH;
}

}  // namespace kad
