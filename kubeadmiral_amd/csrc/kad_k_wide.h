// schedule_wide_kernel.
// Part of kad_kernels.hip's translation unit, which includes the kernels' headers in definition order.
#pragma once

#include "kad_device.h"
#include "kad_kargs.h"
#include "kad_prof.h"
#include "kad_score.h"
#include "kad_select.h"
#include "kad_wave.h"
#include "kad_wq.h"

namespace kad {

// schedule_wide_kernel<NCH> — 256 < C <= 64*NCH (C3: 1 000 clusters, 16
// chunks) on a clean snapshot. The lean kernel's register-resident positions
// do not scale to feasible lists of several hundred clusters (C3: 20 % of the
// units have n > 256), so here:
//   * one 1024-thread workgroup per CU (persistent grid = #CUs): ONE block-
//     shared LDS copy of the cluster attributes (C = 1000: ~56 KB) serves 16
//     waves, and each wave's region (positions, replay scratch: 6 KB at
//     P = 512) fits beside it in the 160 KB LDS;
//   * units are dequeued dynamically from the work queue (kad_wq.h: WQ_HEADS
//     heads, WideArgs::batch units per ticket, one batch ahead of use), so
//     every wave runs until the whole batch is drained (no static-share tail);
//   * each unit's 64-B record and static filter words arrive in ONE VGPR,
//     loaded one unit ahead (lanes 0-15: UnitRec, lanes 16..16+2*nch: sw);
//   * filter per 64-cluster chunk: two ds_read_b128 (available cpu/mem as
//     exact f64; NS|NE taint word + GVK word) → lane masks ANDed in SALU →
//     compaction into the wave's position list (u16 cluster ids);
//   * scores and totals for positions 64q + lane (q < WIDE_Q) in registers,
//     normalisation by DPP wave max; MaxCluster's k-th largest total by LDS
//     histogram (span < 128) or ballot bisection; the same tie rules as the
//     lean kernel (all ties / n <= 12 insertionSort / PdqWave replay).
// REC_FULL units and requests outside the exact-f64 range go to the defer list
// (schedule_kernel). Units with more than WIDE_P feasible clusters: prep routes
// them to the row path up front (BatchDev::early_rows); without that they go to
// the row kernel's list where it runs afterwards, else to the defer list.
#ifndef KAD_DUMMY_STRIDE
#define KAD_DUMMY_STRIDE 1  // u16 dummy slots of the wide kernel's compaction: P + stride * lane (<= 2: inside idx / pid)
#endif
#ifndef KAD_WIDE_C8
#define KAD_WIDE_C8 0  // compaction at exactly 8 chunks: 0 chunk loop, 1 8-cluster lane pieces, 2 16-cluster pieces
#endif
// the row path's body (defined with schedule_row_kernel, kad_k_row.h), run by the wide kernel's opening phase
template <int SM, int NT, class ArgsOf>
__device__ __forceinline__ void row_units(ArgsOf args, char* smem, int rexp);
// the wide kernel's row phase as a separate (not inlined) function: its register demand stays out of the
// unit loop's allocation
template <int SM>
__device__ __attribute__((noinline)) void wide_rows(char* smem, const __attribute__((address_space(4))) struct WideArgs* a);


struct WideArgs {
  SnapDev s;
  BatchDev b;
  OutDev o;
  ProfDev p;
  int waves_per_block;
  int cache_ne, cache_pn;
  int cache_zs;     // the resource scores of a zero request per cluster (c_zs, below)
  int rows_inline;  // the units prep_kernel routed to rows run in this kernel's opening phase (row_units)
  int batch;        // units per work-queue batch (launch_schedule: by units per wave)
  int exp;  // measurement-only variants (KAD_WIDE_EXPERIMENT, never set by default; results differ from
            // the reference): bit 0 skips the pdqsort replay (ties taken by position), bit 1 ends each unit
            // after the filters, bit 2 after the scores (no selection), bit 3 skips the output pass
};
typedef const __attribute__((address_space(4))) WideArgs* WArgs;
// experiment bits: compiled out of product builds
#if defined(KAD_PHASE_PROF) || defined(KAD_TUNING)
#define WIDE_EXP(bits) ((kernarg<WideArgs>()->exp & (bits)) != 0)
#else
#define WIDE_EXP(bits) false
#endif

// XN > 0: the kernel is specialised for exactly XN chunks; SM >= 0: for the score-plugin mask SM (the
// profile's plugins as compile-time constants: every runtime plugin test of the hot loops folds away, and
// with it the 64-bit condition masks the compiler otherwise keeps live — and spills — across the loop)
// ZR: every unit of the batch has a zero ResourceRequest (BatchDev::zero_req): the resource scores are the
// per-cluster column c_zs. (A per-unit test inside the one instantiation cost C3's units, which all carry
// requests, 31 us of 1.13 ms for the zero-request units' 24 us: profiles/r06/ab_c3_zero_request_kernel.txt)
template <int NCH, int XN, int SM, bool ZR = false>
__global__ __launch_bounds__(WIDE_THREADS, 4) void schedule_wide_kernel(WideArgs args) {
  (void)args;  // read through kernarg<WideArgs>()
  constexpr int Q = WIDE_Q;
  constexpr int P = WIDE_P;
  static_assert(XN <= NCH, "exact chunk count within the template bound");
  extern __shared__ __attribute__((aligned(16))) char smem[];
  // the units prep_kernel routed to the row path (more than P feasible clusters, BatchDev::early_rows):
  // the first blocks take them, one unit per block at a time, before their own work queue — in the LDS
  // of the waves' regions (the cluster cache above is loaded afterwards); the queue's dynamic batches
  // absorb the delay of these blocks' static first batches. First in the kernel, so that nothing of the
  // unit loop is live across the row body (its register pressure does not spill the loop's values).
  if (kernarg<WideArgs>()->rows_inline) {
    const int rn = __hip_atomic_load(kernarg<WideArgs>()->b.rows_n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    if ((int)blockIdx.x < rn) {
      wide_rows<SM>(smem, kernarg<WideArgs>());  // (a callee cannot read the kernarg segment pointer itself: pass it)
      __syncthreads();  // the row body's LDS reads are done before the waves' regions are reused
    }
  }
  const int lane = lane_id();
  const int wv = __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
  int C, W, TWs;
  uint32_t fm, sm;
  {
    WArgs a = kernarg<WideArgs>();
    C = a->s.C;
    TWs = a->s.TW;
    W = a->b.W;
    fm = a->p.filter_mask;
    sm = SM >= 0 ? (uint32_t)SM : a->p.score_mask;
  }
  const int nch = XN > 0 ? XN : (C + 63) >> 6;
  const int Cp = nch * 64;
  const WideLayout L = wide_layout();
  const int nwaves = blockDim.x >> 6;
  char* region = smem + (size_t)wv * L.bytes;
  uint32_t* key = (uint32_t*)(region + L.key);
  uint16_t* idx = (uint16_t*)(region + L.idx);
  uint16_t* pid = (uint16_t*)(region + L.pid);
  uint16_t* posl = (uint16_t*)(region + L.posl);
  uint16_t* posr = (uint16_t*)(region + L.posr);
  uint16_t* inv = posl;
  char* cache = smem + (size_t)nwaves * L.bytes;
  double2* c_av = (double2*)cache;
  ulonglong2* c_tg = (ulonglong2*)(cache + (size_t)16 * Cp);
  double2* c_cap = (double2*)(cache + (size_t)32 * Cp);
  float2* c_iv = (float2*)(cache + (size_t)48 * Cp);
  uint64_t* c_ne = nullptr;
  uint64_t* c_pn = nullptr;
  // the sum of the profile's resource scores for a ZERO request per cluster: the live controller never sets
  // ResourceRequest (schedulingtriggers.go:188-191), so Least / Most / Balanced are per-cluster constants
  // there — one LDS read per position instead of the exact-f64 quotients
  int32_t* c_zs = nullptr;
  {
    WArgs a = kernarg<WideArgs>();
    size_t o = (size_t)56 * Cp;
    if (a->cache_ne) {
      c_ne = (uint64_t*)(cache + o);
      o += (size_t)8 * Cp;
    }
    if (a->cache_pn) {
      c_pn = (uint64_t*)(cache + o);
      o += (size_t)8 * Cp;
    }
    if (a->cache_zs) c_zs = (int32_t*)(cache + o);
  }
  const bool f_taint = fm & BIT(KAD_PL_TAINT_TOLERATION), f_api = fm & BIT(KAD_PL_API_RESOURCES);
  const bool fold = kernarg<WideArgs>()->s.fold;  // taint + API filters in the static words (prep_kernel)
  const bool fitf = kernarg<WideArgs>()->s.fitfold;  // and the cpu / memory fit test
  // the static words are always read: they also clear the last chunk's lanes past C (prep_kernel)
  const bool f_fit = fm & BIT(KAD_PL_CLUSTER_RESOURCES_FIT);
  const bool s_res =
      sm & (BIT(KAD_PL_LEAST_ALLOCATED) | BIT(KAD_PL_MOST_ALLOCATED) | BIT(KAD_PL_BALANCED_ALLOCATION));
  const bool s_tt = sm & BIT(KAD_PL_TAINT_TOLERATION);
  {
    WArgs a = kernarg<WideArgs>();
    for (int c = threadIdx.x; c < Cp; c += blockDim.x) {
      const bool in = c < C;
      const uint32_t cl = in ? (uint32_t)c : 0u;
      const int64_t ac = in ? ldg(a->s.alloc_cpu, cl) : 1, uc = in ? ldg(a->s.used_cpu, cl) : 0;
      const int64_t am = in ? ldg(a->s.alloc_mem, cl) : 1, um = in ? ldg(a->s.used_mem, cl) : 0;
      double capc, avc, capm, avm;
      score_res(ac, uc, capc, avc);
      score_res(am, um, capm, avm);
      c_av[c] = make_double2(avc, avm);
      c_cap[c] = make_double2(capc, capm);
      const float ivc = (float)(100.0 / capc), ivm = (float)(100.0 / capm);
      c_iv[c] = make_float2(ivc, ivm);
      c_tg[c] = make_ulonglong2(in ? ldg(a->s.nsne, cl) : 0ull, in ? ldg(a->s.gvk, cl) : 0ull);
      if (c_ne) c_ne[c] = in ? ldg(a->s.ne, cl) : 0;
      if (c_pn) c_pn[c] = in ? ldg(a->s.pns, cl) : 0;
      if (c_zs) {  // the score expressions below with request 0: x = available
        const double xcp = fmax(avc, 0.0), xmp = fmax(avm, 0.0);
        const int okc = -(int)(avc >= 0.0), okm = -(int)(avm >= 0.0);
        int x = 0;
        if (sm & BIT(KAD_PL_LEAST_ALLOCATED)) x += (quot100(xcp, capc, ivc) + quot100(xmp, capm, ivm)) >> 1;
        if (sm & BIT(KAD_PL_MOST_ALLOCATED))
          x += ((quot100(capc - xcp, capc, ivc) & okc) + (quot100(capm - xmp, capm, ivm) & okm)) >> 1;
        if (sm & BIT(KAD_PL_BALANCED_ALLOCATION)) x += (int)balanced_d((capc - avc) / capc, (capm - avm) / capm);
        c_zs[c] = x;
      }
    }
    __syncthreads();
  }

  uint32_t* heads;
  const UnitRec* recs;
  const uint64_t* sws;
  {
    WArgs a = kernarg<WideArgs>();
    heads = a->b.wq;
    recs = a->b.rec;
    sws = a->b.sw;
  }
  WorkTicket tk = wq_start(nwaves, kernarg<WideArgs>()->batch);
#ifdef KAD_PHASE_PROF
  const unsigned long long wt_start = __builtin_amdgcn_s_memrealtime();  // 100 MHz, device-wide
  unsigned long long wx_units = 0, wx_max = 0, wx_deq = wt_start, wx_str = 0;
#endif
  // one VGPR per unit: lanes 0-15 its UnitRec dwords, lanes 16..16+2*nch its static filter words
  auto fetch = [&](int w) -> uint32_t {
    if (w < 0) return 0u;
    if (lane < 16) return ldg((const uint32_t*)(recs + w), (uint32_t)lane);
    if (lane < 16 + 2 * nch) return ldg((const uint32_t*)(sws + (size_t)w * nch), (uint32_t)(lane - 16));
    return 0u;  // chunks past nch: nothing feasible
  };
  int2 cb = wq_resolve(heads, W, tk);  // the static first batch
  if (cb.y > 0) wq_issue(heads, tk);   // the next batch's ticket, resolved when this batch ends
  int w = cb.y > 0 ? cb.x : -1;
  uint32_t cur = fetch(w);
  int bend = cb.x + cb.y;
  KAD_PACC;
  while (w >= 0) {
    // per unit, opaque copies of the loop invariants its conditions derive from: the conditions are then
    // evaluated inside the unit (a few scalar compares) instead of hoisted out of the unit loop and kept
    // live — and spilled — across it as 64-bit masks
    const int nch_o = XN > 0 ? nch : opq(nch);
#define nch nch_o
    // the next unit: within this batch, else the head of the next batch
    int wn = -1;
    if (w + 1 < bend) {
      wn = w + 1;
    } else {
      const int2 nb = wq_resolve(heads, W, tk);
      if (nb.y > 0) {
        wn = nb.x;
        bend = nb.x + nb.y;
        wq_issue(heads, tk);  // resolved one batch later
#ifdef KAD_PHASE_PROF
        wx_deq = __builtin_amdgcn_s_memrealtime();
#endif
      }
    }
    const uint32_t nxt = fetch(wn);
    KAD_PT(t0);
#ifdef KAD_PHASE_PROF
    const unsigned long long ut0 = __builtin_amdgcn_s_memrealtime();
    int ut_n = 0;
    uint32_t ut_fl = 0;
#endif

    auto fld = [&](int d) -> uint32_t { return (uint32_t)__builtin_amdgcn_readlane((int)cur, d); };
    auto fld64 = [&](int d) -> int64_t { return (int64_t)(((uint64_t)fld(d + 1) << 32) | fld(d)); };
    const uint32_t fc = fld(0);
    const int gvc = (int)fld(1);
    const int tsc = (int)fld(2);
    const int64_t rqc = fld64(4), rqm = fld64(6);
    const uint64_t tolc = (uint64_t)fld64(12);
    do {  // one unit; `break` = done with it
      if (fc & REC_ROW) break;  // prep_kernel routed it to schedule_row_kernel
      if (fc & KAD_W_STICKY) {  // generic_scheduler.go:101-104
        unit_status<WideArgs>(w, KAD_ST_STICKY);
        break;
      }
      if ((fc & REC_FULL) || (uint64_t)rqc >= (1ull << 46) || (uint64_t)rqm >= (1ull << 46) ||
          (fc & KAD_W_WIDE_SCORES)) {
        unit_defer<WideArgs>(w);
        break;
      }
      const double rqcd = (double)rqc, rqmd = (double)rqm;  // exact: 0 <= request < 2^46
      const int spo = (int)fld(3);
      const int64_t mc = fld64(8), ooff = fld64(10);
      const uint64_t tolp0 = (uint64_t)fld64(14);
      const bool use_cur = f_taint && (fc & KAD_W_HAS_CURRENT);
      const bool fit_on = f_fit && (fc & KAD_W_FIT_NONZERO);
      const uint64_t o_taint = f_taint ? 0ull : ~0ull;
      const uint64_t o_api = f_api ? 0ull : ~0ull, a_api = gvc >= 0 ? ~0ull : 0ull;
      const double fcpu = fit_on ? rqcd : -1.0, fmem = fit_on ? rqmd : -1.0;  // fit off: compare against -1

      // ---------------- filters → compacted feasible list (findClustersThatFitWorkload, :152-169)
      int n = 0;
      // the chunk loop twice: FAST (one taint word, no CurrentClusters) has no branch inside a
      // 4-chunk group, so the 8 LDS reads of a group issue together; compaction stores are
      // exec-free (infeasible lanes and overflow positions write into pid[], rewritten before use)
      // MODE 2 (FOLD): taint + API already in the static words; 1 (FAST): one taint word, no
      // CurrentClusters; 0: general
      auto filter_chunks = [&](auto mode_t) {
        constexpr int MODE = decltype(mode_t)::value;
        constexpr bool FAST = MODE >= 1, FOLD = MODE >= 2, FITF = MODE == 3;
        // exactly 8 chunks (C4's instantiation): KAD_WIDE_C8 0 keeps the unrolled chunk loop below, 1 gives
        // each lane 8 clusters (all 64 lanes hold bits), 2 the 16-cluster pieces of the general case (half the
        // lanes idle at 512 clusters; 5a66d20 took C4's wide kernel 665 -> 688 us: profiles/r06/bisect_c4.txt)
        constexpr int C8 = KAD_WIDE_C8;
        constexpr bool PIECES = FITF && !(XN == 8 && C8 == 0);
        if constexpr (PIECES) {
          // the static words are the whole filter: compact them with each lane owning B = 16 (8) clusters
          // instead of a chunk loop (per chunk two readlanes, a 64-bit rank and a store — ~9 VALU + 4 SALU, 16
          // chunks at C3). Lane L takes clusters B·L .. B·L+B-1 (its B bits of the dword in lane 16 + L·B/32 of
          // `cur`), its first position is the wave's exclusive prefix of the piece popcounts (cluster order),
          // and the lanes write their set bits one per trip — as many trips as the densest piece holds
          // (C3: ~6); lanes out of bits write their dummy slot P + lane (no exec-mask branch)
          constexpr bool B8 = XN == 8 && C8 == 1;
          constexpr int B = B8 ? 8 : 16;
          const uint32_t dw = (uint32_t)__builtin_amdgcn_ds_bpermute((16 + (B8 ? lane >> 2 : lane >> 1)) << 2, (int)cur);
          uint32_t x = B8 ? (dw >> ((lane & 3) << 3)) & 0xFFu : (dw >> ((lane & 1) << 4)) & 0xFFFFu;
          const int c = __builtin_popcount(x);
          const int incl = wave_incl_sum_i32(c);
          n = __builtin_amdgcn_readlane(incl, 63);
          if (n > P) return;  // (positions past P are never written: the unit goes to rows / defer)
          int pos = incl - c;
          const int base = B * lane;
          while (ballot(x != 0)) {
            const bool on = x != 0;
            const int bit = __builtin_ctz(x | (1u << B));
            idx[on ? pos : P + KAD_DUMMY_STRIDE * lane] = (uint16_t)(base + bit);
            pos += on ? 1 : 0;
            x &= x - 1u;
          }
          return;
        }
        // FOLD: fully unrolled (constant readlane lanes for the static words); else one 4-chunk group per trip
#pragma unroll
        for (int g = 0; g < (FOLD ? NCH : nch); g += 4) {
          if (FOLD && g >= nch) break;
          uint64_t mk[4];
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            const int ch = g + j;
            const int c = ch * WAVE + lane;
            uint64_t m = ~0ull;  // lanes past C and chunks past nch: cleared in the static words
            const int cc = c < Cp ? c : 0;
            const double2 av = FITF ? make_double2(0.0, 0.0) : c_av[cc];
            const ulonglong2 tg = FOLD ? make_ulonglong2(0ull, 0ull) : c_tg[cc];
            const uint64_t sw0 = (((uint64_t)(uint32_t)__builtin_amdgcn_readlane((int)cur, 17 + 2 * ch)) << 32) |
                                 (uint32_t)__builtin_amdgcn_readlane((int)cur, 16 + 2 * ch);
            bool tok;
            if constexpr (FAST) {
              tok = (tg.x & ~tolc) == 0;
            } else {
              WArgs a = kernarg<WideArgs>();
              const bool sch = use_cur && ch < nch && ((ldc(a->b.cw + (size_t)w * nch + ch) >> lane) & 1);
              tok = ((sch ? c_ne[cc] : tg.x) & ~tolc) == 0;
              for (int tw = 1; tw < TWs; ++tw) {  // more than 64 taint ids: words 1.. from global
                const uint32_t cl = c < C ? (uint32_t)c : 0u;
                const uint64_t xt = sch ? ldg(a->s.ne, (uint32_t)(tw * C) + cl) : ldg(a->s.nsne, (uint32_t)(tw * C) + cl);
                tok &= (xt & ~ldc(a->b.tol_all + (size_t)tsc * TWs + tw)) == 0;
              }
            }
            // fit.go:73-134 on exact f64: available - request >= 0 (FITF: in the static words)
            const uint64_t m_fit = FITF ? ~0ull : ballot(av.x >= fcpu) & ballot(av.y >= fmem);
            if constexpr (FOLD) {
              (void)tok;
              m &= sw0 & m_fit;
            } else {
              const uint64_t m_taint = ballot(tok);                    // taint_toleration.go:50-77
              const uint64_t m_api = ballot((tg.y >> (gvc & 63)) & 1);  // apiresources.go:25-43
              m &= sw0 & (m_taint | o_taint) & ((m_api & a_api) | o_api) & m_fit;
            }
            mk[j] = m;
          }
#pragma unroll
          for (int j = 0; j < 4; ++j) {
            // positions past P (the unit is then deferred) stay inside the wave's region (pid, posl); the
            // rank is computed by every lane (pinned in a VGPR) so the address is one v_cndmask, not an
            // exec-mask branch
            int r = n + mbcnt(mk[j]);
            asm volatile("" : "+v"(r));
            idx[lane_on(mk[j]) ? r : P + lane] = (uint16_t)((g + j) * WAVE + lane);
            n += popc64(mk[j]);
          }
        }
      };
      // (the wide kernel runs on clean snapshots of C <= 1024: fold implies fitf; the general mode is
      // correct for any snapshot, re-testing what the static words hold)
      // (the LeastAllocated instantiation runs only on folded, fit-folded snapshots: the host checks; at C3
      // dropping the other modes takes its spilled SGPRs 27 -> 1, while the C4 instantiation ran 0.7 % slower
      // without them)
      if (SM == (1 << KAD_PL_LEAST_ALLOCATED) || (fold && fitf))
        filter_chunks(std::integral_constant<int, 3>{});
      else if (!fold && !use_cur && TWs == 1)
        filter_chunks(std::integral_constant<int, 1>{});
      else
        filter_chunks(std::integral_constant<int, 0>{});
      KAD_PT(t1);
      KAD_PADD(0, t1 - t0);
#ifdef KAD_PHASE_PROF
      ut_n = n;
#endif
      if (n == 0) {  // generic_scheduler.go:112-114
        unit_status<WideArgs>(w, KAD_ST_NO_FEASIBLE);
        break;
      }
      if (n > P) {
        unit_row_or_defer<WideArgs, true>(w);
        break;
      }
      if ((sm & BIT(KAD_PL_CLUSTER_AFFINITY)) && (fc & KAD_W_SCORE_ERROR)) {  // framework.go:149-159
        unit_status<WideArgs>(w, KAD_ST_ERR_SCORE);
        break;
      }
      if (WIDE_EXP(2)) {
        unit_status<WideArgs>(w, KAD_ST_OK);
        break;
      }
      wave_sync();

      // ---------------- scores of positions 64q + lane (RunScorePlugins, framework.go:139-181)
      const int nq = (n + 63) >> 6;
      int t[Q];
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
        const uint32_t raw = idx[p];  // (p < 512 = P: inside the wave's region, no exec branch; past n discarded)
        cid[q] = v ? raw : 0u;
        const uint32_t cq = cid[q];
        if (ZR) {  // (s_res: ZR launches only with a resource score in the profile)
          t[q] = c_zs[cq];
        } else if (s_res) {
          // x = cap - req = available - request (exact); req > cap <=> x < 0 (score 0)
          const double2 cap = c_cap[cq], av = c_av[cq];
          const double xc = av.x - rqcd, xm = av.y - rqmd;
          const float2 iv = c_iv[cq];
          const double xcp = fmax(xc, 0.0), xmp = fmax(xm, 0.0);
          const int okc = -(int)(xc >= 0.0), okm = -(int)(xm >= 0.0);
          int x = 0;
          if (sm & BIT(KAD_PL_LEAST_ALLOCATED)) x += (quot100(xcp, cap.x, iv.x) + quot100(xmp, cap.y, iv.y)) >> 1;
          if (sm & BIT(KAD_PL_MOST_ALLOCATED))
            x += ((quot100(cap.x - xcp, cap.x, iv.x) & okc) + (quot100(cap.y - xmp, cap.y, iv.y) & okm)) >> 1;
          if (sm & BIT(KAD_PL_BALANCED_ALLOCATION)) x += (int)balanced_d((cap.x - xc) / cap.x, (cap.y - xm) / cap.y);
          t[q] = x;
        }
        if (s_tt) {  // taint_toleration.go:91-118: PreferNoSchedule taints not tolerated
          int tc = popc64(c_pn[cq] & ~tolp0);
          for (int tw = 1; tw < TWs; ++tw) {
            WArgs a = kernarg<WideArgs>();
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
          if (q < nq) t[q] += ttmax == 0 ? 100 : 100 - (int)small_quot(100 * ttv[q], ttmax);
      }
      // units without preferred terms (C4's) score 0 everywhere: one scalar load of the term count decides
      // before the 64-word window's vector load (2ef3455 loaded the window for every unit: C4's wide kernel
      // 688 -> 728 us, profiles/r06/bisect_c4.txt)
      if ((sm & BIT(KAD_PL_CLUSTER_AFFINITY)) && ldc(kernarg<WideArgs>()->b.sprog + spo) > 0) {  // cluster_affinity.go:96-140
        WArgs a = kernarg<WideArgs>();
        const int32_t* sp = a->b.sprog + spo;
        const uint32_t pv = ldg((const uint32_t*)sp, (uint32_t)lane);  // program words 0..63 (slack past the blob)
        {
          int afs[Q];  // |raw| <= sum |weight| <= 2^20 (wider units are deferred)
          int amax = 0;
#pragma unroll
          for (int q = 0; q < Q; ++q) {
            afs[q] = 0;
            if (q < nq && q * 64 + lane < n) afs[q] = (int)affinity_score_pv(a->b.req_mask, pv, sp, nch, (int)cid[q]);
            amax = afs[q] > amax ? afs[q] : amax;
          }
          amax = wave_max_u_i32(amax);
#pragma unroll
          for (int q = 0; q < Q; ++q)
            if (q < nq) {
              const int num = 100 * afs[q];
              t[q] += amax == 0 ? afs[q] : (num >= 0 && num < (1 << 24) ? (int)small_quot(num, amax) : num / amax);
            }
        }
      }

      KAD_PT(t2);
      KAD_PADD(1, t2 - t1);
      // ---------------- select (framework.go:183-209, max_cluster.go:42-66)
      WArgs ad = kernarg<WideArgs>();
      int k = n;
      if (ad->p.select_plugin == KAD_PL_MAX_CLUSTER && !WIDE_EXP(4)) {
        const bool hm = fc & KAD_W_HAS_MAX_CLUSTERS;
        if (hm && mc < 0) {
          unit_status<WideArgs>(w, KAD_ST_ERR_SELECT);
          break;
        }
        if (hm && mc < k) k = (int)mc;
      }
      // selection rule for the output pass: 0 all, 1 total >= T, 2 first ties (n <= 12), 3 replay ranks
      int mode = 0, T = 0, need = 0;
      uint32_t rflags = 0;
      if (k < n && k > 0) {
        int mn = INT32_MAX, mx = INT32_MIN;
#pragma unroll
        for (int q = 0; q < Q; ++q)
          if (q < nq) {
            const bool vq = q * 64 + lane < n;
            mn = (vq && t[q] < mn) ? t[q] : mn;
            mx = (vq && t[q] > mx) ? t[q] : mx;
          }
        int mn32, mx32;
        wave_minmax_u_i32(mn, mx, mn32, mx32);
        int lo32 = mn32, hi32 = mx32;
        int gcount = -1, e = 0;  // #(total > T), #(total == T); -1: count them below
        if ((uint32_t)mx32 - (uint32_t)mn32 < 128u) {
          // LDS histogram in descending bin order + one wave prefix sum: the k-th largest total, and the
          // counts above / at it from the same prefix (no per-position ballots)
          uint32_t* hist = key;
          *(uint2*)(hist + 2 * lane) = make_uint2(0u, 0u);
          wave_sync();
#pragma unroll
          for (int q = 0; q < Q; ++q)
            if (q < nq) {  // exec-free: lanes past n add 0 to bin `lane` (one shared bin: 26M of C3's 78M
              // LDS bank-conflict cycles, 0.5 % of the kernel; profiles/r06/ab_c3_lds_conflicts.txt)
              const bool vq = q * 64 + lane < n;
              atomicAdd(hist + (vq ? 127 - (t[q] - mn32) : lane), vq ? 1u : 0u);
            }
          wave_sync();
          const uint2 hh = *(const uint2*)(hist + 2 * lane);  // bins 127-2l, 126-2l
          const int pre = wave_incl_sum_i32((int)(hh.x + hh.y));
          const int l0 = (int)__builtin_ctzll(ballot(pre >= k));
          const int pl = __builtin_amdgcn_readlane(pre, l0);
          const int h0 = __builtin_amdgcn_readlane((int)hh.x, l0);
          const int h1 = __builtin_amdgcn_readlane((int)hh.y, l0);
          const bool first = pl - h1 >= k;  // T is the higher bin of lane l0's pair
          lo32 = mn32 + (first ? 127 - 2 * l0 : 126 - 2 * l0);
          e = first ? h0 : h1;
          gcount = first ? pl - h1 - h0 : pl - h1;
          wave_sync();
        } else {
          while (lo32 < hi32) {  // the largest T with #(total >= T) >= k
            const uint32_t d = (uint32_t)hi32 - (uint32_t)lo32;
            const int mid = (int)((uint32_t)lo32 + (d >> 1) + (d & 1));
            int cnt = 0;
#pragma unroll
            for (int q = 0; q < Q; ++q)
              if (q < nq) cnt += popc64(ballot(q * 64 + lane < n && t[q] >= mid));
            if (cnt >= k)
              lo32 = mid;
            else
              hi32 = mid - 1;
          }
        }
        T = lo32;
        if (gcount < 0) {
          gcount = 0;
#pragma unroll
          for (int q = 0; q < Q; ++q)
            if (q < nq) {
              const bool v = q * 64 + lane < n;
              gcount += popc64(ballot(v && t[q] > T));
              e += popc64(ballot(v && t[q] == T));
            }
        }
        need = k - gcount;
        if (need == e) {  // the cut takes every tie: no sort needed
          mode = 1;
        } else {
          rflags = KAD_RF_TIE_STRADDLE;
          if (n <= 12 || WIDE_EXP(1)) {  // pdqsort_func: a single (stable) insertionSort
            mode = 2;
          } else {
            // restricted pdqsort replay, wave-parallel, on u32 keys total - min (order-preserving)
            const int xs_b = (ad->p.flags & KAD_PROFILE_XORSHIFT_GO121) ? 7 : 17;
            const int xs_c = (ad->p.flags & KAD_PROFILE_XORSHIFT_GO121) ? 17 : 5;
            KAD_PT(r0);
            if ((uint32_t)mx32 - (uint32_t)mn32 < 65536u) {
              // packed replay: key << 16 | position (n <= 512), one LDS word per element
#pragma unroll
              for (int q = 0; q < Q; ++q)
                if (q < nq && q * 64 + lane < n)
                  key[q * 64 + lane] = ((uint32_t)(t[q] - mn32) << 16) | (uint32_t)(q * 64 + lane);
              wave_sync();
              PdqWaveP<> pw{key, posl, posr, xs_b, xs_c};
              KAD_PT(r1);
              pw.select(n, k);
              KAD_PT(r2);
              for (int r = lane; r < n; r += WAVE) inv[key[r] & 0xFFFFu] = (uint16_t)r;
              wave_sync();
              KAD_PT(r3);
              KAD_PADD(6, (r1 - r0) + (r3 - r2));
#ifdef KAD_PHASE_PROF
              KAD_PADD(7, pw.pr[0]);
              KAD_PADD(8, pw.pr[1]);
              KAD_PADD(9, pw.pr[2]);
              KAD_PADD(10, pw.pr[3]);
              KAD_PADD(11, n);
#endif
            } else {
#pragma unroll
              for (int q = 0; q < Q; ++q)
                if (q < nq && q * 64 + lane < n) {
                  key[q * 64 + lane] = (uint32_t)(t[q] - mn32);
                  pid[q * 64 + lane] = (uint16_t)(q * 64 + lane);
                }
              wave_sync();
              PdqWave<uint32_t> pw{key, pid, posl, posr, xs_b, xs_c};
              KAD_PT(r1);
              pw.select(n, k);
              KAD_PT(r2);
              for (int r = lane; r < n; r += WAVE) inv[pid[r]] = (uint16_t)r;
              wave_sync();
              KAD_PT(r3);
              KAD_PADD(6, (r1 - r0) + (r3 - r2));
            }
            mode = 3;
          }
        }
      } else if (k <= 0) {
        mode = -1;  // nothing selected
      }

      KAD_PT(t3);
      KAD_PADD(2, t3 - t2);
      if (rflags) {
        KAD_PADD(4, 1);
        KAD_PADD(5, t3 - t2);
      }
#ifdef KAD_PHASE_PROF
      ut_fl = rflags ? 1u : 0u;
#endif
      // ---------------- output, ascending cluster id (= ascending position)
      {
        WArgs ae = kernarg<WideArgs>();
        const bool dup = fc & KAD_W_DUPLICATE;
        const bool replicas =
            !dup && ae->p.replicas_plugin == KAD_PL_CLUSTER_CAPACITY_WEIGHT && (fc & REC_DESIRED_POS) && k > 0;
        int base = 0;
        if ((dup || replicas) && mode >= 0 && !WIDE_EXP(8)) {
          int32_t* oc = ae->o.cluster + ooff;
          int64_t* orp = ae->o.replicas + ooff;
          const int64_t rv = dup ? -1 : 0;
          // the selection mode is uniform: one branch per unit, then a branch-free predicate per position
          auto emit = [&](int q, bool s) {
            const uint64_t sel = ballot(s);
            const uint32_t at = (uint32_t)(base + mbcnt(sel));
            if (s) {
              stg(oc, at, (int32_t)cid[q]);
              stg(orp, at, rv);
            }
            base += popc64(sel);
          };
          if (mode == 3) {  // the replay's ranks
#pragma unroll
            for (int q = 0; q < Q; ++q)
              if (q < nq) {
                const int p = q * 64 + lane;
                const uint32_t rk = inv[p];  // (p < P + 64: inside the region, no exec branch; past n discarded)
                emit(q, p < n && rk < (uint32_t)k);
              }
          } else if (mode == 2) {  // every total > T, then the first `need` ties by position
            int eq_before = 0;
#pragma unroll
            for (int q = 0; q < Q; ++q)
              if (q < nq) {
                const bool v = q * 64 + lane < n;
                const uint64_t eqm = ballot(v && t[q] == T);
                emit(q, v && (t[q] > T || (t[q] == T && mbcnt(eqm) + eq_before < need)));
                eq_before += popc64(eqm);
              }
          } else {  // 0: every position; 1: total >= T
            const int Tlo = mode == 0 ? INT32_MIN : T;
#pragma unroll
            for (int q = 0; q < Q; ++q)
              if (q < nq) emit(q, q * 64 + lane < n && t[q] >= Tlo);
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
    } while (false);
#ifdef KAD_PHASE_PROF
    {
      KAD_PT(tz);
      wx_units++;
      wx_max = (tz - t0) > wx_max ? (tz - t0) : wx_max;
      const unsigned long long ut1 = __builtin_amdgcn_s_memrealtime();
      if (lane == 0 && w < KAD_UTRACE_MAX) {
        const unsigned long long gw = (unsigned long long)(blockIdx.x * nwaves + wv) & 0xFFFFull;
        g_ustart[w] = ut0;
        g_uinfo[w] = (ut1 - ut0) | ((unsigned long long)(ut_n & 0x7FFF) << 32) | ((unsigned long long)ut_fl << 47) |
                     (gw << 48);
      }
    }
#endif
    cur = nxt;
    w = wn;
#undef nch
  }
#ifdef KAD_PHASE_PROF
  {
    const int gwv = blockIdx.x * nwaves + wv;
    if (lane == 0 && gwv < 8192) {
      g_wavetime[2 * gwv] = wt_start;
      g_wavetime[2 * gwv + 1] = __builtin_amdgcn_s_memrealtime();
      g_wavex[6 * gwv] = wx_units;
      g_wavex[6 * gwv + 1] = wx_max;
      g_wavex[6 * gwv + 2] = wx_deq;
      g_wavex[6 * gwv + 3] = pacc[4];
      g_wavex[6 * gwv + 4] = __builtin_amdgcn_s_getreg((31 << 11) | 4);   // HW_ID
      g_wavex[6 * gwv + 5] = __builtin_amdgcn_s_getreg((31 << 11) | 20);  // XCC_ID
    }
  }
#endif
  KAD_PFLUSH_LEAN;
}

}  // namespace kad
