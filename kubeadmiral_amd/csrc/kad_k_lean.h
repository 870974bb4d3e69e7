// schedule_lean_kernel.
// Part of kad_kernels.hip's translation unit, which includes the kernels' headers in definition order.
#pragma once

#include "kad_affinity.h"
#include "kad_device.h"
#include "kad_kargs.h"
#include "kad_prof.h"
#include "kad_score.h"
#include "kad_select.h"
#include "kad_wave.h"
#include "kad_wq.h"

namespace kad {

// schedule_lean_kernel<NCH, CL> — the common case: every snapshot the wide kernel
// does not take (kad_route.h route_schedule). Each wave owns a run of consecutive units.
// For NCH > 0 (C <= 64*NCH) the block first copies the cluster attributes the
// path reads (fit resources, taint words, GVK word) into an LDS cache shared
// by its waves; a unit's record and static filter words arrive in VGPRs with
// one vector load per 4-unit batch (issued a batch ahead) and are read with
// v_readlane. CL (clean snapshot, SnapDev::clean, NCH > 0): the resource
// columns are cached as exact f64 (capacity, available) + f32 100/cap and
// every total fits 32 bits (see quot100).
// The feasible list is compacted into LDS (snapshot order = the reference's
// feasible list, generic_scheduler.go:152-169); then each lane owns
// positions lane + 64q (q < QMAX), and scores, normalisation and MaxCluster's
// first-k set are computed in registers:
//   * the k-th largest total T from an LDS histogram when the totals span
//     < 128 (one wave prefix sum), else by ballot bisection over [min, max];
//   * cut takes every tie (k - #(>T) == #(==T)): selection = {total >= T};
//   * n <= 12: Go's pdqsort is one stable insertionSort, so the selection is
//     {> T} plus the first k - #(>T) ties in input order;
//   * otherwise the restricted pdqsort replay (kad_select.h PdqWave) on u32
//     keys (total - row minimum) in the wave's LDS region.
// Units routed REC_FULL by prep go to the defer list and schedule_kernel
// afterwards; those (NCH == 0) with more than 64*QMAX feasible clusters to
// the row kernel's list where it runs, else to the defer list too.

struct LeanArgs {
  SnapDev s;
  BatchDev b;
  OutDev o;
  ProfDev p;
  int wave_bytes, waves_per_block, units_per_wave;  // units_per_wave: work-queue batch size (<= LEAN_BATCH)
  int cache_ne, cache_pn;  // optional cache arrays present
};
typedef const __attribute__((address_space(4))) LeanArgs* LArgs;

// CL (clean snapshot, host-checked SnapDev::clean, NCH > 0): resources as exact
// f64 columns, every total in [-2^28, 2^28] (units with wide affinity weights
// or requests outside [0, 2^46) are deferred), so totals live in 32 bits
template <typename TT>
__device__ __forceinline__ TT tadd(TT a, int64_t b) {
  if constexpr (sizeof(TT) == 8)
    return wadd(a, b);
  else
    return a + (TT)b;
}
// SM >= 0: specialised for that score-plugin mask (as schedule_wide_kernel)
template <int NCH, bool CL, int SM = -1>
__global__ __launch_bounds__(256, 6) void schedule_lean_kernel(LeanArgs args) {
  using TT = typename std::conditional<CL, int, int64_t>::type;
  (void)args;  // read through kernarg<LeanArgs>()
  constexpr int Q = lean_qmax(NCH);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = lane_id();
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int C, W, TWs;
  uint32_t fm, sm;
  char* region;
  {
    LArgs a = kernarg<LeanArgs>();
    region = smem + (size_t)wv * a->wave_bytes;
    C = a->s.C;
    TWs = a->s.TW;
    W = a->b.W;
    fm = a->p.filter_mask;
    sm = SM >= 0 ? (uint32_t)SM : a->p.score_mask;
  }
  const int nch = (C + 63) >> 6;
  const LeanLayout L = lean_layout(C, Q);
  constexpr int P = Q * 64;
  const int Cp = nch * 64;
  uint32_t* key = (uint32_t*)(region + L.key);
  uint16_t* idx = (uint16_t*)(region + L.idx);
  uint16_t* pid = (uint16_t*)(region + L.pid);
  uint16_t* posl = (uint16_t*)(region + L.posl);
  uint16_t* posr = (uint16_t*)(region + L.posr);
  uint16_t* inv = posl;  // ranks after the replay
  const bool f_taint = fm & BIT(KAD_PL_TAINT_TOLERATION), f_api = fm & BIT(KAD_PL_API_RESOURCES);
  // static filter words carry ClusterAffinity + PlacementFilter, and with SnapDev::fold also TaintToleration
  // + APIResources (prep_kernel)
  const bool fold = kernarg<LeanArgs>()->s.fold;
  const bool fitf = kernarg<LeanArgs>()->s.fitfold;  // cpu / memory fit in the static words too
  // the static words are always read: they also clear the last chunk's lanes past C (prep_kernel)
  constexpr bool f_sw = true;
  const bool f_fit = fm & BIT(KAD_PL_CLUSTER_RESOURCES_FIT);
  const bool s_res =
      sm & (BIT(KAD_PL_LEAST_ALLOCATED) | BIT(KAD_PL_MOST_ALLOCATED) | BIT(KAD_PL_BALANCED_ALLOCATION));
  const bool s_tt = sm & BIT(KAD_PL_TAINT_TOLERATION);

  // block-shared LDS cache of the cluster attributes (NCH > 0), after the wave regions
  int64_t* cache = (int64_t*)(smem + (size_t)blockDim.x / 64 * kernarg<LeanArgs>()->wave_bytes);
  int64_t* c_ac = cache;
  int64_t* c_uc = cache + Cp;
  int64_t* c_am = cache + 2 * Cp;
  int64_t* c_um = cache + 3 * Cp;
  uint64_t* c_ns = (uint64_t*)(cache + 4 * Cp);
  uint64_t* c_gv = (uint64_t*)(cache + 5 * Cp);
  uint64_t* c_ne = nullptr;
  uint64_t* c_pn = nullptr;
  float2* c_iv = nullptr;
  // clean snapshot (host-checked, SnapDev::clean): the resource columns are
  // cached as exact f64 capacity / available (alloc - used) plus f32 100/cap,
  // and fit / Least / Most / Balanced run in f64 compares and one correction
  constexpr bool clean = CL && NCH > 0;
  {
    LArgs a = kernarg<LeanArgs>();
    int nx = 6;
    if (a->cache_ne) c_ne = (uint64_t*)(cache + (nx++) * Cp);
    if (a->cache_pn) c_pn = (uint64_t*)(cache + (nx++) * Cp);
    if (clean) c_iv = (float2*)(cache + (nx++) * Cp);
  }
  if constexpr (NCH > 0) {
    LArgs a = kernarg<LeanArgs>();
    for (int c = threadIdx.x; c < Cp; c += blockDim.x) {
      const bool in = c < C;
      const uint32_t cl = in ? (uint32_t)c : 0u;
      const int64_t ac = in ? ldg(a->s.alloc_cpu, cl) : 1, uc = in ? ldg(a->s.used_cpu, cl) : 0;
      const int64_t am = in ? ldg(a->s.alloc_mem, cl) : 1, um = in ? ldg(a->s.used_mem, cl) : 0;
      if (clean) {
        double capc, avc, capm, avm;  // (relaxed clusters: only with the fit rows, MODE 3 below)
        score_res(ac, uc, capc, avc);
        score_res(am, um, capm, avm);
        c_ac[c] = __builtin_bit_cast(int64_t, capc);
        c_uc[c] = __builtin_bit_cast(int64_t, avc);
        c_am[c] = __builtin_bit_cast(int64_t, capm);
        c_um[c] = __builtin_bit_cast(int64_t, avm);
        c_iv[c] = make_float2((float)(100.0 / capc), (float)(100.0 / capm));
      } else {
        c_ac[c] = in ? ac : 0;
        c_uc[c] = uc;
        c_am[c] = in ? am : 0;
        c_um[c] = um;
      }
      c_ns[c] = in ? ldg(a->s.nsne, cl) : 0;
      c_gv[c] = in ? ldg(a->s.gvk, cl) : 0;
      if (c_ne) c_ne[c] = in ? ldg(a->s.ne, cl) : 0;
      if (c_pn) c_pn[c] = in ? ldg(a->s.pns, cl) : 0;
    }
    __syncthreads();
  }
  constexpr int NR = NCH > 0 ? NCH : 1;

  // UnitRecs and static filter words of a batch of up to 8 units, loaded
  // with two vector loads at the batch start into VGPRs (record dword d of
  // batch unit u in lane 16*(u&3)+d of rvA/rvB; filter word ch of unit u in
  // lanes 2*(u*nch+ch)+{0,1} of svv) and read per unit with v_readlane: no
  // scalar or vector memory round trip per unit (an SMEM load would be
  // waited by the next LDS wait; a vector load by the last unit's stores).
  // Units are dequeued in batches of LEAN_BATCH from the work heads (WorkTicket: one returning atomicAdd
  // per batch, resolved one batch later); the grid is the resident wave count (launch_schedule) and
  // every wave runs until all heads are drained, so no wave idles on a static share while others work.
  const UnitRec* recs = kernarg<LeanArgs>()->b.rec;
  const uint64_t* sws = kernarg<LeanArgs>()->b.sw;
  uint32_t* heads = kernarg<LeanArgs>()->b.wq;
  WorkTicket tk = wq_start((int)(blockDim.x >> 6), kernarg<LeanArgs>()->units_per_wave);
#ifdef KAD_PHASE_PROF
  const unsigned long long wt_start = __builtin_amdgcn_s_memrealtime();  // 100 MHz, device-wide
#endif
  // the next batch's records are loaded one batch ahead (nrvA/nsvv): the
  // wait at a batch start then only covers the previous unit's stores
  uint32_t rvA = 0, svv = ~0u, nrvA = 0, nsvv = ~0u;
  auto fetch = [&](int wb, int nb) {
    nrvA = lane < nb * 16 ? ldg((const uint32_t*)(recs + wb), (uint32_t)lane) : 0u;
    if (NCH > 0 && f_sw) nsvv = lane < nb * 2 * nch ? ldg((const uint32_t*)(sws + (size_t)wb * nch), (uint32_t)lane) : ~0u;
  };
  int2 cb = wq_resolve(heads, W, tk);  // the static first batch; then the ticket of the one after
  if (cb.y > 0) {
    wq_issue(heads, tk);
    fetch(cb.x, cb.y);
  }
  int w = -1, bend = 0, u = 0;
  KAD_PACC;
  for (;;) {
    ++w;
    ++u;
    if (w >= bend) {  // next batch
      if (cb.y <= 0) break;
      w = cb.x;
      bend = cb.x + cb.y;
      u = 0;
      rvA = nrvA;
      svv = nsvv;
      cb = wq_resolve(heads, W, tk);
      if (cb.y > 0) {
        wq_issue(heads, tk);
        fetch(cb.x, cb.y);
      }
    }
    KAD_PT(t0);
    auto fld = [&](int d) -> uint32_t { return (uint32_t)__builtin_amdgcn_readlane((int)rvA, (u << 4) + d); };
    auto fld64 = [&](int d) -> int64_t { return (int64_t)(((uint64_t)fld(d + 1) << 32) | fld(d)); };
    const uint32_t fc = fld(0);
    const int gvc = (int)fld(1);
    const int tsc = (int)fld(2);
    const int64_t rqc = fld64(4), rqm = fld64(6);
    const uint64_t tolc = (uint64_t)fld64(12);
    uint64_t swc[NR];
#pragma unroll
    for (int ch = 0; ch < NR; ++ch) {
      const int l = 2 * (u * nch + ch);
      swc[ch] = ((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)svv, l + 1) << 32) |
                (uint32_t)__builtin_amdgcn_readlane((int)svv, l);
    }
    if (fc & KAD_W_STICKY) {  // generic_scheduler.go:101-104
      unit_status<LeanArgs>(w, KAD_ST_STICKY);
      continue;
    }
    if ((fc & REC_FULL) ||
        (clean && ((uint64_t)rqc >= (1ull << 46) || (uint64_t)rqm >= (1ull << 46) || (fc & KAD_W_WIDE_SCORES)))) {
      unit_defer<LeanArgs>(w);  // (requests outside [0, 2^46) and wide weights set the host's batch_defer)
      continue;
    }
    const double rqcd = (double)rqc, rqmd = (double)rqm;  // exact on the clean path
    const int spo = (int)fld(3);
    const int64_t mc = fld64(8), ooff = fld64(10);
    const uint64_t tolp0 = (uint64_t)fld64(14);
    const bool use_cur = f_taint && (fc & KAD_W_HAS_CURRENT);
    const bool fit_on = f_fit && (fc & KAD_W_FIT_NONZERO);
    const uint64_t o_sw = 0ull, o_taint = f_taint ? 0ull : ~0ull, o_fit = fit_on ? 0ull : ~0ull;
    const uint64_t o_api = f_api ? 0ull : ~0ull, a_api = gvc >= 0 ? ~0ull : 0ull;  // no GVK id: no cluster has it
    const double fcpu = fit_on ? rqcd : -1.0, fmem = fit_on ? rqmd : -1.0;  // clean fit compare operands
    uint64_t dsw = ~0ull, dcw = 0;  // dynamic-NCH path: words of chunks 64g..64g+63 in lanes
    auto load_words = [&](int ch0) {
      LArgs a = kernarg<LeanArgs>();
      const int ch = ch0 + lane;
      dsw = (f_sw && ch < nch) ? ldg(a->b.sw, (uint32_t)(w * nch + ch)) : ~0ull;
      dcw = (use_cur && ch < nch) ? ldg(a->b.cw, (uint32_t)(w * nch + ch)) : 0ull;
    };
    if constexpr (NCH == 0) load_words(0);
    // (NCH == 0, every filter in the static words: the words of chunks 64..191 load in the same round trip)
    uint64_t dsw1 = 0, dsw2 = 0;
    if constexpr (NCH == 0) {
      if (fold && fitf && f_sw && nch > WAVE) {
        LArgs a = kernarg<LeanArgs>();
        const int c1 = WAVE + lane, c2 = 2 * WAVE + lane;
        dsw1 = ldg(a->b.sw, (uint32_t)(w * nch + (c1 < nch ? c1 : nch - 1)));
        dsw2 = ldg(a->b.sw, (uint32_t)(w * nch + (c2 < nch ? c2 : nch - 1)));
      }
    }

    // ---------------- filters → compacted feasible list (findClustersThatFitWorkload, :152-169)
    int n = 0;
    uint64_t mk[NR];
    const int NC = NCH > 0 ? NCH : nch;
    // NCH == 0 (no LDS cache): the attributes of chunk ch+1 are loaded while
    // chunk ch is filtered (software pipeline; one exposed round trip per unit)
    int64_t p_ac = 0, p_uc = 0, p_am = 0, p_um = 0;
    uint64_t p_ns = 0, p_ne = 0, p_gv = 0;
    // NCH == 0: the attributes of chunk cn (lanes = its clusters) that the mode's filters read: none
    // when every filter is in the static words (FITF), the resources only with FOLD
    auto load_attrs = [&](auto mode_t, int cn) {
      constexpr int MODE = decltype(mode_t)::value;
      if constexpr (MODE != 3) {
        LArgs a = kernarg<LeanArgs>();
        const uint32_t cl = cn < C ? (uint32_t)cn : 0u;
        p_ac = ldg(a->s.alloc_cpu, cl);
        p_uc = ldg(a->s.used_cpu, cl);
        p_am = ldg(a->s.alloc_mem, cl);
        p_um = ldg(a->s.used_mem, cl);
        if constexpr (MODE < 2) {
          p_ns = ldg(a->s.nsne, cl);
          p_ne = ldg(a->s.ne, cl);
          p_gv = ldg(a->s.gvk, cl);
        }
      }
    };
    // the chunk loop twice: FAST (no CurrentClusters, one taint word) has no
    // uniform branch inside, so the cache reads of every chunk issue together
    // MODE 2 (FOLD): taint and API filters already in the static words (prep_kernel, SnapDev::fold);
    // 1 (FAST): one taint word, no CurrentClusters; 0: general
    auto filter_chunks = [&](auto mode_t) {
      constexpr int MODE = decltype(mode_t)::value;
      constexpr bool FAST = MODE >= 1, FOLD = MODE >= 2, FITF = MODE == 3;
      if constexpr (NCH == 0 && FITF) {
        // every filter is in the static words: only the non-zero words of each 64-chunk group (one per
        // lane) are compacted — C5's median unit has 2 feasible clusters of 10 000
        for (int g = 0; g < nch; g += WAVE) {
          if (g == WAVE) dsw = f_sw ? dsw1 : ~0ull;
          else if (g == 2 * WAVE) dsw = f_sw ? dsw2 : ~0ull;
          else if (g > 0) load_words(g);
          uint64_t nz = ballot(g + lane < nch && dsw != 0);
          while (nz) {
            const int l = __builtin_ctzll(nz);
            nz &= nz - 1;
            const uint64_t m = readlane64(dsw, l);
            if (lane_on(m)) {
              const int pos = n + mbcnt(m);
              if (pos < P) idx[pos] = (uint16_t)((g + l) * WAVE + lane);  // more than P: deferred
            }
            n += popc64(m);
            if (n > P) return;
          }
        }
        return;
      }
      const bool ucur = !FAST && use_cur;
      if constexpr (NCH == 0) load_attrs(mode_t, lane);
#pragma unroll
      for (int ch = 0; ch < NC; ++ch) {
        const int c = ch * WAVE + lane;
        int64_t acpu, ucpu, amem, umem;
        uint64_t ns0, ne0, pn0, gv0, sw0, cw0;
        if constexpr (NCH > 0) {
          acpu = (clean || FITF) ? 0 : c_ac[c];
          ucpu = FITF ? 0 : c_uc[c];  // clean: available cpu as f64
          amem = (clean || FITF) ? 0 : c_am[c];
          umem = FITF ? 0 : c_um[c];
          ns0 = FOLD ? 0ull : c_ns[c];
          ne0 = ucur ? c_ne[c] : 0ull;
          pn0 = 0;
          gv0 = FOLD ? 0ull : c_gv[c];
          sw0 = swc[ch];
          cw0 = ucur ? ldc(kernarg<LeanArgs>()->b.cw + (size_t)w * nch + ch) : 0ull;
        } else {
          acpu = p_ac;
          ucpu = p_uc;
          amem = p_am;
          umem = p_um;
          ns0 = p_ns;
          ne0 = p_ne;
          gv0 = p_gv;
          pn0 = 0;
          if (ch + 1 < NC) load_attrs(mode_t, c + WAVE);
          if (ch > 0 && (ch & 63) == 0) load_words(ch);
          sw0 = readlane64(dsw, ch & 63);
          cw0 = readlane64(dcw, ch & 63);
        }
        // each filter as a lane mask (v_cmp → SGPR pair), combined with scalar
        // ANDs under uniform selects (no branches inside the unrolled loop)
        uint64_t m = ~0ull;  // lanes past C: cleared in the static word
        const bool sch = ucur && ((cw0 >> lane) & 1);
        const uint64_t x = sch ? ne0 : ns0;
        bool tok = (x & ~tolc) == 0;
        for (int tw = 1; tw < (FAST ? 1 : TWs); ++tw) {  // more than 64 taint ids (C5): words 1.. from global
          LArgs a = kernarg<LeanArgs>();
          const uint32_t cl = c < C ? (uint32_t)c : 0u;
          const uint64_t xt = sch ? ldg(a->s.ne, (uint32_t)(tw * C) + cl) : ldg(a->s.nsne, (uint32_t)(tw * C) + cl);
          tok &= (xt & ~ldc(a->b.tol_all + (size_t)tsc * TWs + tw)) == 0;
        }
        // fit.go:73-134: alloc >= req + used (clean: available - req >= 0, exact in f64; with the filter
        // off the compare is against -1, true everywhere)
        const uint64_t m_fit = FITF    ? ~0ull  // in the static words (SnapDev::fitfold)
                               : clean ? ballot(__builtin_bit_cast(double, ucpu) >= fcpu) & ballot(__builtin_bit_cast(double, umem) >= fmem)
                                       : ballot((acpu >= wadd(rqc, ucpu)) & (amem >= wadd(rqm, umem)));
        if constexpr (FOLD) {
          (void)tok;
          m &= sw0 & (clean ? m_fit : (m_fit | o_fit));
        } else {
          const uint64_t m_taint = ballot(tok);      // taint_toleration.go:50-77
          const uint64_t m_api = ballot((gv0 >> (gvc & 63)) & 1);  // apiresources.go:25-43
          // disabled filters OR in an all-ones mask (per-unit constants: two SALU ops per filter)
          m &= (sw0 | o_sw) & (m_taint | o_taint) & ((m_api & a_api) | o_api) & (m_fit | o_fit);
        }
        (void)pn0;
        if constexpr (NCH > 0) {
          mk[ch] = m;  // compaction after every chunk's mask: no LDS store between the cache reads
        } else {
          if ((m >> lane) & 1) {
            const int pos = n + mbcnt(m);
            if (pos < P) idx[pos] = (uint16_t)c;  // more than P feasible: the unit is deferred
          }
          n += popc64(m);
          if (n > P) break;  // deferred whatever the remaining chunks hold
        }
      }
    };
    if (fold && fitf)
      filter_chunks(std::integral_constant<int, 3>{});
    else if (fold)
      filter_chunks(std::integral_constant<int, 2>{});
    else if (!use_cur && TWs == 1)
      filter_chunks(std::integral_constant<int, 1>{});
    else
      filter_chunks(std::integral_constant<int, 0>{});
    if constexpr (NCH > 0) {
#pragma unroll
      for (int ch = 0; ch < NCH; ++ch) {
        // every lane stores (no exec branch): infeasible lanes into pid[], rewritten before use
        idx[lane_on(mk[ch]) ? n + mbcnt(mk[ch]) : P + lane] = (uint16_t)(ch * WAVE + lane);
        n += popc64(mk[ch]);
      }
    }
    KAD_PT(t1);
    KAD_PADD(0, t1 - t0);
    if (n == 0) {  // generic_scheduler.go:112-114
      unit_status<LeanArgs>(w, KAD_ST_NO_FEASIBLE);
      continue;
    }
    if (NCH == 0 && n > P) {  // more feasible clusters than registers: the row kernel (or the full kernel)
      unit_row_or_defer<LeanArgs>(w);
      continue;
    }
    if ((sm & BIT(KAD_PL_CLUSTER_AFFINITY)) && (fc & KAD_W_SCORE_ERROR)) {  // framework.go:149-159
      unit_status<LeanArgs>(w, KAD_ST_ERR_SCORE);
      continue;
    }
    wave_sync();

    // ---------------- scores of positions 64q + lane (RunScorePlugins, framework.go:139-181)
    const int nq = (n + 63) >> 6;
    TT t[Q];
    uint32_t cid[Q];
    int ttv[Q];
    int ttmax = 0;
#pragma unroll
    for (int q = 0; q < Q; ++q) {
      t[q] = 0;
      cid[q] = 0;
      ttv[q] = 0;
      if (q >= nq) continue;
      const int p = q * 64 + lane;
      const bool v = p < n;
      cid[q] = v ? idx[p] : 0u;
      const uint32_t cq = cid[q];
      if (s_res && clean) {
        // x = cap - req = available - request (exact); req > cap <=> x < 0 (score 0)
        const double capc = __builtin_bit_cast(double, c_ac[cq]), capm = __builtin_bit_cast(double, c_am[cq]);
        const double xc = __builtin_bit_cast(double, c_uc[cq]) - rqcd, xm = __builtin_bit_cast(double, c_um[cq]) - rqmd;
        const float2 iv = c_iv[cq];
        // branch-free: quotients of max(x, 0) (= 0 when x <= 0), masked to 0 where req > cap
        const double xcp = fmax(xc, 0.0), xmp = fmax(xm, 0.0);
        const int okc = -(int)(xc >= 0.0), okm = -(int)(xm >= 0.0);
        int x = 0;
        if (sm & BIT(KAD_PL_LEAST_ALLOCATED)) x += (quot100(xcp, capc, iv.x) + quot100(xmp, capm, iv.y)) >> 1;
        if (sm & BIT(KAD_PL_MOST_ALLOCATED))
          x += ((quot100(capc - xcp, capc, iv.x) & okc) + (quot100(capm - xmp, capm, iv.y) & okm)) >> 1;
        if (sm & BIT(KAD_PL_BALANCED_ALLOCATION)) x += (int)balanced_d((capc - xc) / capc, (capm - xm) / capm);
        t[q] = (TT)x;
      } else if (s_res) {
        int64_t cc, cm, uc, um;
        if constexpr (NCH > 0) {
          cc = c_ac[cq];
          cm = c_am[cq];
          uc = c_uc[cq];
          um = c_um[cq];
        } else {
          LArgs a = kernarg<LeanArgs>();
          cc = ldg(a->s.alloc_cpu, cq);
          cm = ldg(a->s.alloc_mem, cq);
          uc = ldg(a->s.used_cpu, cq);
          um = ldg(a->s.used_mem, cq);
        }
        if (!v) {
          cc = cm = 1;
          uc = um = 0;
        }
        const int64_t rc = wadd(uc, rqc), rm = wadd(um, rqm);
        int64_t x = 0;
        if (sm & BIT(KAD_PL_LEAST_ALLOCATED))
          x = wadd(x, go_div(wadd(least_requested(rm, cm), least_requested(rc, cc)), 2));
        if (sm & BIT(KAD_PL_MOST_ALLOCATED))
          x = wadd(x, go_div(wadd(most_requested(rm, cm), most_requested(rc, cc)), 2));
        if (sm & BIT(KAD_PL_BALANCED_ALLOCATION)) x = wadd(x, balanced(rc, cc, rm, cm));
        t[q] = x;
      }
      if (s_tt) {  // taint_toleration.go:91-118: PreferNoSchedule taints not tolerated
        uint64_t pn;
        if constexpr (NCH > 0)
          pn = c_pn[cq];
        else
          pn = ldg(kernarg<LeanArgs>()->s.pns, cq);
        int tc = popc64(pn & ~tolp0);
        for (int tw = 1; tw < TWs; ++tw) {
          LArgs a = kernarg<LeanArgs>();
          tc += popc64(ldg(a->s.pns, (uint32_t)(tw * C) + cq) & ~ldc(a->b.tol_pns + (size_t)tsc * TWs + tw));
        }
        ttv[q] = v ? tc : 0;
        ttmax = ttv[q] > ttmax ? ttv[q] : ttmax;
      }
    }
    if (s_tt) {  // DefaultNormalizeScore(100, reverse=true), framework/util.go:455-483
      ttmax = wave_max_u_i32(ttmax);
#pragma unroll
      for (int q = 0; q < Q; ++q)
        if (q < nq) t[q] = tadd(t[q], ttmax == 0 ? 100 : 100 - (int64_t)small_quot(100 * ttv[q], ttmax));
    }
    if (sm & BIT(KAD_PL_CLUSTER_AFFINITY)) {  // cluster_affinity.go:96-140 + DefaultNormalizeScore(100, false)
      LArgs a = kernarg<LeanArgs>();
      const int32_t* sp = a->b.sprog + spo;
      const uint32_t pv = ldg((const uint32_t*)sp, (uint32_t)lane);  // program words 0..63 (slack past the blob)
      if (__builtin_amdgcn_readfirstlane((int)pv) > 0) {  // units without preferred terms score 0 everywhere
        TT afs[Q];  // CL: |raw| <= sum |weight| <= 2^20 (wider units are deferred)
        TT amax = 0;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          afs[q] = 0;
          if (q < nq && q * 64 + lane < n) afs[q] = (TT)affinity_score_pv(a->b.req_mask, pv, sp, nch, (int)cid[q]);
          amax = afs[q] > amax ? afs[q] : amax;
        }
        if constexpr (CL) {
          amax = wave_max_u_i32(amax);
#pragma unroll
          for (int q = 0; q < Q; ++q)
            if (q < nq) {
              const int num = 100 * afs[q];
              t[q] += amax == 0 ? afs[q] : (num >= 0 && num < (1 << 24) ? (int)small_quot(num, amax) : num / amax);
            }
        } else {
          amax = wave_max_u_i64(amax);
#pragma unroll
          for (int q = 0; q < Q; ++q)
            if (q < nq) t[q] = wadd(t[q], amax == 0 ? afs[q] : div_fast(wmul(100, afs[q]), amax));
        }
      }
    }
    KAD_PT(t2);
    KAD_PADD(1, t2 - t1);

    // ---------------- select (framework.go:183-209, max_cluster.go:42-66)
    LArgs ad = kernarg<LeanArgs>();
    int k = n;  // <= n <= 64 * Q: 32-bit counts
    if (ad->p.select_plugin == KAD_PL_MAX_CLUSTER) {
      const bool hm = fc & KAD_W_HAS_MAX_CLUSTERS;
      if (hm && mc < 0) {
        unit_status<LeanArgs>(w, KAD_ST_ERR_SELECT);
        continue;
      }
      if (hm && mc < k) k = (int)mc;
    }
    uint64_t sel[Q];
    uint32_t rflags = 0;
#pragma unroll
    for (int q = 0; q < Q; ++q) sel[q] = 0;
    if (k >= n) {
#pragma unroll
      for (int q = 0; q < Q; ++q) sel[q] = ballot(q * 64 + lane < n);
    } else if (k > 0) {
      // lanes holding a total, per position chunk
      uint64_t vm[Q];
      TT mn = CL ? (TT)INT32_MAX : (TT)I64_MAX, mx = CL ? (TT)INT32_MIN : (TT)I64_MIN;
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        const int r = n - q * 64;
        vm[q] = q < nq ? (r >= 64 ? ~0ull : ((1ull << r) - 1)) : 0ull;
        const bool vq = lane_on(vm[q]);
        mn = (vq && t[q] < mn) ? t[q] : mn;
        mx = (vq && t[q] > mx) ? t[q] : mx;
      }
      // k-th largest total T: the largest T with #(total >= T) >= k, by
      // bisection over [min, max] — in 32 bits when every total fits (the
      // usual case: totals are sums of 0..100 plugin scores)
      const bool hv = lane < n;
      int64_t rmin, rmax, lo;
      if (!ballot(hv && (mn < INT32_MIN || mx > INT32_MAX))) {
        int mn32, mx32;
        wave_minmax_u_i32(hv ? (int)mn : INT32_MAX, hv ? (int)mx : INT32_MIN, mn32, mx32);
        int t32[Q];
#pragma unroll
        for (int q = 0; q < Q; ++q) t32[q] = (int)t[q];
        int lo32 = mn32, hi32 = mx32;
        if (Q >= 2 && (uint32_t)mx32 - (uint32_t)mn32 < 128u) {
          // totals within 128 of each other (the usual case: sums of 0..100
          // plugin scores): LDS histogram in descending bin order, one
          // prefix sum over the wave, the k-th largest from one ballot —
          // instead of a ballot-count bisection step per bit of the range
          uint32_t* hist = key;  // 128 u32; the replay rewrites key[] afterwards
          *(uint2*)(hist + 2 * lane) = make_uint2(0u, 0u);
          wave_sync();
#pragma unroll
          for (int q = 0; q < Q; ++q)
            if (q < nq) {  // exec-free: lanes past n add 0 to bin `lane` (not all to one bin)
              const bool vq = lane_on(vm[q]);
              atomicAdd(hist + (vq ? 127 - (t32[q] - mn32) : lane), vq ? 1u : 0u);
            }
          wave_sync();
          const uint2 hh = *(const uint2*)(hist + 2 * lane);  // bins 127-2l, 126-2l
          const int pre = wave_incl_sum_i32((int)(hh.x + hh.y));  // #(total >= mn + 126 - 2l)
          const int kk = (int)k;
          const int l0 = (int)__builtin_ctzll(ballot(pre >= kk));
          const int pl = __builtin_amdgcn_readlane(pre, l0);
          const int h1 = __builtin_amdgcn_readlane((int)hh.y, l0);
          lo32 = mn32 + (pl - h1 >= kk ? 127 - 2 * l0 : 126 - 2 * l0);
          hi32 = lo32;
          wave_sync();
        }
        if (nq == 1) {  // one position per lane: one ballot per step
          while (lo32 < hi32) {
            const uint32_t d = (uint32_t)hi32 - (uint32_t)lo32;
            const int mid = (int)((uint32_t)lo32 + (d >> 1) + (d & 1));
            if (popc64(ballot(t32[0] >= mid) & vm[0]) >= k)
              lo32 = mid;
            else
              hi32 = mid - 1;
          }
        } else {
          while (lo32 < hi32) {
            const uint32_t d = (uint32_t)hi32 - (uint32_t)lo32;
            const int mid = (int)((uint32_t)lo32 + (d >> 1) + (d & 1));
            int cnt = 0;
#pragma unroll
            for (int q = 0; q < Q; ++q)
              if (q < nq) cnt += popc64(ballot(t32[q] >= mid) & vm[q]);
            if (cnt >= k)
              lo32 = mid;
            else
              hi32 = mid - 1;
          }
        }
        rmin = mn32;
        rmax = mx32;
        lo = lo32;
      } else {
        rmin = wave_min_u_i64(mn);
        rmax = wave_max_u_i64(mx);
        lo = rmin;
        int64_t hi = rmax;
        while (lo < hi) {
          const uint64_t d = (uint64_t)hi - (uint64_t)lo;
          const int64_t mid = (int64_t)((uint64_t)lo + (d >> 1) + (d & 1));
          int64_t cnt = 0;
#pragma unroll
          for (int q = 0; q < Q; ++q)
            if (q < nq) cnt += popc64(ballot(t[q] >= mid) & vm[q]);
          if (cnt >= k)
            lo = mid;
          else
            hi = (int64_t)((uint64_t)mid - 1);
        }
      }
      uint64_t gm[Q], em[Q];
      int g = 0, e = 0;
#pragma unroll
      for (int q = 0; q < Q; ++q) {
        gm[q] = ballot(t[q] > lo) & vm[q];
        em[q] = ballot(t[q] == lo) & vm[q];
        g += popc64(gm[q]);
        e += popc64(em[q]);
      }
      const int need = k - g;
      if (need == e) {  // the cut takes every tie: no sort needed
#pragma unroll
        for (int q = 0; q < Q; ++q) sel[q] = gm[q] | em[q];
      } else {
        rflags = KAD_RF_TIE_STRADDLE;
        const int xs_b = (ad->p.flags & KAD_PROFILE_XORSHIFT_GO121) ? 7 : 17;
        const int xs_c = (ad->p.flags & KAD_PROFILE_XORSHIFT_GO121) ? 17 : 5;
        if (n <= 12) {  // pdqsort_func: a single (stable) insertionSort
          sel[0] = gm[0] | ballot(lane < n && t[0] == lo && mbcnt(em[0]) < need);
        } else {
          // restricted pdqsort replay, wave-parallel (kad_select.h PdqWave), on
          // u32 keys t - min (order-preserving); rows spanning >= 2^32 go to schedule_kernel
          if ((uint64_t)rmax - (uint64_t)rmin > 0xFFFFFFFFull) {
            unit_defer<LeanArgs>(w);
            continue;
          }
          if ((uint64_t)rmax - (uint64_t)rmin < 65536u) {  // packed replay: key << 16 | position
#pragma unroll
            for (int q = 0; q < Q; ++q)
              if (q < nq && q * 64 + lane < n)
                key[q * 64 + lane] = ((uint32_t)((uint64_t)t[q] - (uint64_t)rmin) << 16) | (uint32_t)(q * 64 + lane);
            wave_sync();
            PdqWaveP<> pw{key, posl, posr, xs_b, xs_c};
            pw.select(n, (int)k);
            for (int r = lane; r < n; r += WAVE) inv[key[r] & 0xFFFFu] = (uint16_t)r;
          } else {
#pragma unroll
            for (int q = 0; q < Q; ++q)
              if (q < nq && q * 64 + lane < n) {
                key[q * 64 + lane] = (uint32_t)((uint64_t)t[q] - (uint64_t)rmin);
                pid[q * 64 + lane] = (uint16_t)(q * 64 + lane);
              }
            wave_sync();
            PdqWave<uint32_t> pw{key, pid, posl, posr, xs_b, xs_c};
            pw.select(n, (int)k);
            for (int r = lane; r < n; r += WAVE) inv[pid[r]] = (uint16_t)r;
          }
          wave_sync();
#pragma unroll
          for (int q = 0; q < Q; ++q)
            if (q < nq) {
              const int p = q * 64 + lane;
              sel[q] = ballot(p < n && inv[p] < k);
            }
        }
      }
    }
    KAD_PT(t3);
    KAD_PADD(2, t3 - t2);
    if (rflags) {
      KAD_PADD(4, 1);
      KAD_PADD(5, t3 - t2);
    }

    // ---------------- output, ascending cluster id (= ascending position)
    {
      LArgs ae = kernarg<LeanArgs>();
      const bool dup = fc & KAD_W_DUPLICATE;
      const bool replicas =
          !dup && ae->p.replicas_plugin == KAD_PL_CLUSTER_CAPACITY_WEIGHT && (fc & REC_DESIRED_POS) && k > 0;
      int base = 0;
      if (dup || replicas) {
        int32_t* oc = ae->o.cluster + ooff;
        int64_t* orp = ae->o.replicas + ooff;
#pragma unroll
        for (int q = 0; q < Q; ++q) {
          if ((sel[q] >> lane) & 1) {
            const uint32_t at = (uint32_t)(base + mbcnt(sel[q]));
            stg(oc, at, (int32_t)cid[q]);
            stg(orp, at, (int64_t)(dup ? -1 : 0));
          }
          base += popc64(sel[q]);
        }
      }
      if (lane == 0) {
        ae->o.status[w] = KAD_ST_OK;
        ae->o.count[w] = base;  // Divide without replicas plugin: empty map
        ae->o.flags[w] = rflags;
      }
    }
    wave_sync();
    KAD_PT(t4);
    KAD_PADD(3, t4 - t3);
  }
#ifdef KAD_PHASE_PROF
  {
    const int gwv = blockIdx.x * (int)(blockDim.x >> 6) + wv;
    if (lane == 0 && gwv < 8192) {
      g_wavetime[2 * gwv] = wt_start;
      g_wavetime[2 * gwv + 1] = __builtin_amdgcn_s_memrealtime();
    }
  }
#endif
  KAD_PFLUSH_LEAN;
}

}  // namespace kad
