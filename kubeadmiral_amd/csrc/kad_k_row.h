// schedule_row_kernel, and the row body that schedule_wide_kernel's opening phase runs (row_units, wide_rows).
// Part of kad_kernels.hip's translation unit, which includes the kernels' headers in definition order.
#pragma once

#include "kad_device.h"
#include "kad_k_wide.h"
#include "kad_kargs.h"
#include "kad_prof.h"
#include "kad_score.h"
#include "kad_select.h"
#include "kad_wave.h"

namespace kad {

// schedule_row_kernel — the units whose feasible list is longer than the lean / wide kernels' register
// positions (C5: 16 % of the units, a few thousand feasible clusters of 10 000), on snapshots where
// every filter is in the static words (BatchDev::use_rows: clean, SnapDev::fold and ::fitfold,
// C <= ROW_MAX_C). One 512-thread workgroup per unit, two per CU (LDS: 6 B per cluster + the preferred-
// term words, which the replay scratch reuses), persistent (units dequeued from BatchDev::rows):
//   * compaction: the unit's static words → per-chunk popcounts → block prefix → cluster ids in LDS
//     (findClustersThatFitWorkload order, generic_scheduler.go:152-169);
//   * scores spread over the 8 waves (RunScorePlugins, framework.go:139-181), the clean-snapshot
//     arithmetic of the wide kernel (exact f64 quotients, 32-bit totals), block maxima for
//     DefaultNormalizeScore (framework/util.go:455-483);
//   * MaxCluster (max_cluster.go:42-66): the k-th largest total by a block-wide 8-bit radix histogram;
//     the cut takes every tie, or wave 0 replays Go's pdqsort restricted to k (PdqWave) on the LDS keys,
//     its position scratch in LDS up to ROW_NREP positions, else in the block's global slab;
//   * output in ascending cluster id by per-chunk ballots and a block prefix.
// Units outside the clean-f64 range (requests >= 2^46, wide affinity weights) or with more than
// ROW_MAX_TERMS preferred terms go on to the defer list.
#ifndef KAD_ROW_RU
#define KAD_ROW_RU 2
#endif
#ifndef KAD_ROW_MINW
#define KAD_ROW_MINW 2  // waves per SIMD the row kernel's VGPR budget is sized for (2 blocks of 8 waves / CU: 4)
#endif
// scoring: positions per thread trip, their gathers issued together. 3 cut the score phase's cycles per row
// by 29 % (profiling build, profiles/r03/q6_c5_ru*.json) but at 127 VGPRs the kernel ran 1.5 % longer (C5
// rows 1.28 -> 1.30 ms, two product builds on one box); 4 spills and drops to one block per CU
constexpr int ROW_RU = KAD_ROW_RU;
static_assert(ROW_MAX_BLOCKS >= 1, "row kernel slabs");
// per-block global slab for replays longer than ROW_NREP: pid u16[Cp], posl u16[Cp + 64], posr u16[Cp]
__host__ __device__ size_t row_slab_bytes(int C) { return ((size_t)6 * ((C + 63) & ~63) + 128 + 255) & ~(size_t)255; }

struct RowArgs {
  SnapDev s;
  BatchDev b;
  OutDev o;
  ProfDev p;
  char* slabs;  // [grid][row_slab_bytes(C)]
  int exp;      // measurement-only variants (profiling builds, KAD_ROW_EXPERIMENT; results differ): bit 0 no
                // resource scores, bit 1 no PreferNoSchedule counts, bit 2 no affinity scores
};

// block-wide reductions of one i32 per thread: wave partials in red[nw], every thread reads all (NW > 0: the
// wave count as a constant)
template <int NW>
__device__ __forceinline__ int row_block_max(int v, int* red, int nw) {
  const int r = wave_max_u_i32(v);
  if (lane_id() == 0) red[threadIdx.x >> 6] = r;
  __syncthreads();
  int m = red[0];
  if constexpr (NW > 0) {
#pragma unroll
    for (int i = 1; i < NW; ++i) m = red[i] > m ? red[i] : m;
  } else {
    for (int i = 1; i < nw; ++i) m = red[i] > m ? red[i] : m;
  }
  __syncthreads();
  return m;
}
template <int NW>
__device__ __forceinline__ int row_block_min(int v, int* red, int nw) { return -row_block_max<NW>(-v, red, nw); }
template <int NW>
__device__ __forceinline__ int row_block_sum(int v, int* red, int nw) {
  const int r = wave_sum_u_i32(v);
  if (lane_id() == 0) red[threadIdx.x >> 6] = r;
  __syncthreads();
  int m = 0;
  if constexpr (NW > 0) {
#pragma unroll
    for (int i = 0; i < NW; ++i) m += red[i];
  } else {
    for (int i = 0; i < nw; ++i) m += red[i];
  }
  __syncthreads();
  return m;
}
// exclusive prefix of cnt[0..m) in place by wave `by`, total in cnt[m]; callers sync before and after
__device__ __forceinline__ void row_exclusive_scan(int* cnt, int m, int by = 0) {
  if ((int)(threadIdx.x >> 6) != by) return;
  const int lane = lane_id();
  int carry = 0;
  for (int c0 = 0; c0 < m; c0 += WAVE) {
    const int i = c0 + lane;
    const int v = i < m ? cnt[i] : 0;
    const int inc = wave_incl_sum_i32(v);
    if (i < m) cnt[i] = carry + inc - v;
    carry += __builtin_amdgcn_readlane(inc, 63);
  }
  if (lane == 0) cnt[m] = carry;
}

// The row path over BatchDev::rows, for one workgroup: schedule_row_kernel's body (NT = ROW_THREADS) and
// schedule_wide_kernel's opening phase (NT = 0: the wide block's blockDim.x threads, up to ROW_MAX_WAVES
// waves) — the wide kernel's blocks take the units prep_kernel routed to rows before their own work
// queue, so no second stream, fork or join is needed. `rargs` returns the kernel's arguments (SnapDev s,
// BatchDev b, OutDev o, ProfDev p in the constant address space); smem: row_kernel_lds(C) bytes of LDS.
// SM >= 0: specialised for that score-plugin mask (as schedule_wide_kernel).
template <int SM, int NT, class ArgsOf>
__device__ __forceinline__ void row_units(ArgsOf rargs, char* smem, int rexp_arg) {
  constexpr int NW = NT / 64;
  const int NTH = NT > 0 ? NT : (int)blockDim.x;
  const int NWV = NT > 0 ? NW : NTH >> 6;
  const int tid = threadIdx.x, lane = lane_id();
  const int wv = __builtin_amdgcn_readfirstlane(tid >> 6);
  int C, TW;
  uint32_t fm, sm;
  {
    auto a = rargs();
    C = a->s.C;
    TW = a->s.TW;
    fm = a->p.filter_mask;
    sm = SM >= 0 ? (uint32_t)SM : a->p.score_mask;
  }
  (void)fm;
  const int nch = (C + 63) >> 6;
  const RowKLayout L = rowk_layout(C);
  uint32_t* key = (uint32_t*)(smem + L.key);
  uint16_t* idx = (uint16_t*)(smem + L.idx);
  uint16_t* pid_l = (uint16_t*)(smem + L.pid);
  uint16_t* posl_l = (uint16_t*)(smem + L.posl);
  uint16_t* posr_l = (uint16_t*)(smem + L.posr);
  uint64_t* termw = (uint64_t*)(smem + L.x);  // preferred-term words (scoring and normalisation only)
  uint16_t* pid_g;  // the block's global slab (replays longer than ROW_NREP)
  pid_g = (uint16_t*)(rargs()->b.row_slabs + (size_t)blockIdx.x * row_slab_bytes(C));
  uint64_t* const swl0 = (uint64_t*)(smem + L.sw);
  int32_t* const cnt0 = (int32_t*)(smem + L.cnt);
  uint32_t* hist = (uint32_t*)(smem + L.hist);
  int32_t* red = (int32_t*)(smem + L.red);
  int32_t* bc = red + 4 * ROW_MAX_WAVES;  // broadcasts
#if defined(KAD_PHASE_PROF) || defined(KAD_TUNING)
  const int rexp = rexp_arg;
#else
  constexpr int rexp = 0;
  (void)rexp_arg;
#endif
  const bool s_res =
      (sm & (BIT(KAD_PL_LEAST_ALLOCATED) | BIT(KAD_PL_MOST_ALLOCATED) | BIT(KAD_PL_BALANCED_ALLOCATION))) && !(rexp & 1);
  const bool s_tt = (sm & BIT(KAD_PL_TAINT_TOLERATION)) && !(rexp & 2);

  KAD_PACC;
  // the next unit's list index is dequeued one unit ahead (thread 64, wave 1's lane 0), so the returning
  // atomic's latency overlaps the current unit. While wave 0 replays (or before the output pass) wave 1
  // also prefetches the next unit: its static words, chunk counts and their prefix into the other LDS
  // buffer (bc[20]: the prefetched unit, -1 the list is drained, -2 nothing prefetched); the list is
  // complete before this kernel starts (prep_kernel's early routing, or the lean kernel before it)
  // thread 64 holds the list length (complete before this kernel starts), its ticket and the unit the ticket
  // names, loaded one dequeue ahead: a dequeue returns a unit already in a register and only issues the next
  // ticket's atomic and list load (waited for at the next dequeue, a unit later)
  int ticket = 0, rn = 0, nxt_u = -1;
  if (tid == 64) {
    auto a = rargs();
    rn = __hip_atomic_load(a->b.rows_n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    ticket = atomicAdd(a->b.rows_head, 1);
    nxt_u = ticket < rn ? a->b.rows[ticket] : -1;
  }
#ifdef KAD_PHASE_PROF
  const unsigned long long rt_start = __builtin_amdgcn_s_memrealtime();
  unsigned long long rt_units = 0;
#endif
  if (tid == 0) bc[20] = -2;
  int par = 0;  // the current unit's buffers
  uint32_t* const pre0 = (uint32_t*)(smem + L.pre);
  // one wave: unit u's UnitRec dwords (lanes 0-15), its score-program length and first ROW_PRE_PROG words into
  // pr — the unit's scalars are then LDS reads, not a chain of scalar loads (record → program → each term)
  auto stage_unit = [&](int u, uint32_t* pr) {
    auto a = rargs();
    const uint32_t rd = lane < 16 ? ldg((const uint32_t*)(a->b.rec + u), (uint32_t)lane) : 0u;
    const int so = ldg(a->b.sprog_off, (uint32_t)u), se = ldg(a->b.sprog_off, (uint32_t)u + 1u);
    const int len = se - so;
    const int32_t pw = lane < len ? ldg(a->b.sprog, (uint32_t)(so + lane)) : 0;
    if (lane < 16) pr[lane] = rd;
    if (lane == 0) pr[16] = (uint32_t)len;
    pr[17 + lane] = (uint32_t)pw;
  };
  auto next_unit = [&]() -> int {  // thread 64 only
    const int nx = nxt_u;
    if (nx >= 0) {
      auto a = rargs();
      ticket = atomicAdd(a->b.rows_head, 1);
      nxt_u = ticket < rn ? a->b.rows[ticket] : -1;
    }
    return nx;
  };
  auto prefetch = [&]() {  // wave 1
    if (lane == 0) bc[20] = next_unit();
    wave_sync();
    const int nx = __builtin_amdgcn_readfirstlane(bc[20]);
    if (nx < 0) return;
    stage_unit(nx, pre0 + (size_t)(par ^ 1) * ROW_PRE_DW);
    uint64_t* sw2 = swl0 + (size_t)(par ^ 1) * nch;
    int32_t* c2 = cnt0 + (size_t)(par ^ 1) * (nch + 1);
    const uint64_t* src = rargs()->b.sw + (size_t)nx * nch;
    for (int ch = lane; ch < nch; ch += WAVE) {
      const uint64_t m = ldg(src, (uint32_t)ch);
      sw2[ch] = m;
      c2[ch] = popc64(m);
    }
    wave_sync();
    row_exclusive_scan(c2, nch, 1);
  };
  for (;;) {
    __syncthreads();  // the previous unit's LDS reads (and wave 1's prefetch) are done
    KAD_PT(t0);
    if (tid == 64) {
      const int pf = bc[20];
      bc[21] = pf != -2 ? 1 : 0;
      bc[0] = pf != -2 ? pf : next_unit();
      bc[20] = -2;
    }
    __syncthreads();
    const int w = __builtin_amdgcn_readfirstlane(bc[0]);
    const bool pre = __builtin_amdgcn_readfirstlane(bc[21]) != 0;
    if (w < 0) break;
#ifdef KAD_PHASE_PROF
    rt_units++;
#endif
    if (pre) par ^= 1;
    uint64_t* const swl = swl0 + (size_t)par * nch;
    int32_t* const cnt = cnt0 + (size_t)par * (nch + 1);
    uint32_t* const pr = pre0 + (size_t)par * ROW_PRE_DW;
    bool did_pf = false;  // wave 1 prefetched the next unit during this one (uniform)
    auto a = rargs();
    if (!pre) {  // not prefetched: record, program and static words now (the chunk counts' prefix below)
      if (wv == 0) stage_unit(w, pr);
      for (int ch = tid; ch < nch; ch += NTH) {
        const uint64_t m = ldg(a->b.sw, (uint32_t)(w * nch + ch));
        swl[ch] = m;
        cnt[ch] = popc64(m);
      }
      __syncthreads();
      row_exclusive_scan(cnt, nch);
    }
    __syncthreads();
    auto prd = [&](int d) -> uint32_t { return (uint32_t)__builtin_amdgcn_readfirstlane((int)pr[d]); };
    auto prd64 = [&](int d) -> int64_t { return (int64_t)(((uint64_t)prd(d + 1) << 32) | prd(d)); };
    const uint32_t fc = prd(0);
    const int64_t rqc = prd64(4), rqm = prd64(6);
    const int spo = (int)prd(3);
    const int plen = (int)prd(16);
    // score program word i: staged in LDS (programs of up to ROW_PRE_PROG words, every bench unit's), else global
    auto spw = [&](int i) -> int32_t {
      return plen <= ROW_PRE_PROG ? (int32_t)prd(17 + i) : ldc(rargs()->b.sprog + spo + i);
    };
    const bool many_terms = (sm & BIT(KAD_PL_CLUSTER_AFFINITY)) && plen > 0 && spw(0) > ROW_MAX_TERMS;
    if ((uint64_t)rqc >= (1ull << 46) || (uint64_t)rqm >= (1ull << 46) || (fc & KAD_W_WIDE_SCORES) || many_terms) {
      if (tid == 0) {  // outside the exact clean-f64 range: the full kernel
        const int slot = atomicAdd(a->b.defer_n, 1);
        a->b.defer[slot] = w;
      }
      continue;
    }
    const int tsc = (int)prd(2);
    const int64_t mc = prd64(8), ooff = prd64(10);
    auto status = [&](int32_t st) {
      if (tid == 0) {
        auto ao = rargs();
        ao->o.status[w] = st;
        ao->o.count[w] = 0;
        ao->o.flags[w] = 0;
      }
    };

    // ---------------- compaction of the static words (every filter folded by prep_kernel)
    const int n = __builtin_amdgcn_readfirstlane(cnt[nch]);
    {
      // four chunks per trip, their words and offsets read together; every lane stores (infeasible lanes
      // into a dummy slot of the term-word region, unused until the term words below): no exec branch
      // between the LDS reads of consecutive chunks
      uint16_t* const dmy = (uint16_t*)(smem + L.x) + lane;
      for (int ch0 = wv; ch0 < nch; ch0 += 4 * NWV) {
        uint64_t mm[4];
        int co[4];
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const int ch = ch0 + u * NWV;
          const int cl = ch < nch ? ch : nch - 1;
          const uint64_t m = swl[cl];
          mm[u] = ch < nch ? m : 0ull;
          co[u] = cnt[cl];
        }
#pragma unroll
        for (int u = 0; u < 4; ++u) {
          const bool on = lane_on(mm[u]);
          uint16_t* const dst = on ? idx + co[u] + mbcnt(mm[u]) : dmy;
          *dst = (uint16_t)((ch0 + u * NWV) * WAVE + lane);
        }
      }
    }
    KAD_PADD(0, 1);
    if (n == 0) {  // generic_scheduler.go:112-114
      status(KAD_ST_NO_FEASIBLE);
      continue;
    }
    if ((sm & BIT(KAD_PL_CLUSTER_AFFINITY)) && (fc & KAD_W_SCORE_ERROR)) {  // framework.go:149-159
      status(KAD_ST_ERR_SCORE);
      continue;
    }
    int k = n;
    if (a->p.select_plugin == KAD_PL_MAX_CLUSTER) {
      const bool hm = fc & KAD_W_HAS_MAX_CLUSTERS;
      if (hm && mc < 0) {
        status(KAD_ST_ERR_SELECT);
        continue;
      }
      if (hm && mc < k) k = (int)mc;
    }
    __syncthreads();
    KAD_PT(t1);
    KAD_PADD(1, t1 - t0);

    // ---------------- raw scores (RunScorePlugins, framework.go:139-181)
    const int32_t* sp = a->b.sprog + spo;
    const int n_terms = plen > 0 ? spw(0) : 0;
    const bool s_aff = (sm & BIT(KAD_PL_CLUSTER_AFFINITY)) && n_terms > 0 && !(rexp & 4);  // no terms: 0 everywhere
    // ClusterAffinity preferred terms (cluster_affinity.go:96-135) as per-chunk words in LDS (<= ROW_MAX_TERMS,
    // checked above): word (t, ch) = AND of the term's requirement rows — once per chunk instead of once per
    // feasible position; a position's raw score is then a sum of weights over LDS bit tests, recomputed
    // where it is needed (no per-position array)
    // the term list parsed once: weights in SGPRs (constant indices after unrolling), each term's
    // expression count and id offset in LDS for the (term, chunk) word pass
    int32_t wt[ROW_MAX_TERMS];
    int32_t* tdesc = bc + 4;  // [2][ROW_MAX_TERMS]: expression count, id offset (broadcast slots 4..19)
    {
      int pc = 1;
#pragma unroll
      for (int t = 0; t < ROW_MAX_TERMS; ++t) {
        wt[t] = 0;
        if (t < n_terms) {
          wt[t] = spw(pc);
          const int ne = spw(pc + 1);
          if (tid == 0) {
            tdesc[t] = ne;
            tdesc[ROW_MAX_TERMS + t] = pc + 2;
          }
          pc += 2 + ne;
        }
      }
    }
    int wabs = 0;  // sum of |weight|: bounds |raw affinity score|
#pragma unroll
    for (int t = 0; t < ROW_MAX_TERMS; ++t) wabs += t < n_terms ? (wt[t] < 0 ? -wt[t] : wt[t]) : 0;
    const bool apack = s_aff && wabs <= 4095;
    auto raw_aff = [&](uint32_t c) {
      int af = 0;
#pragma unroll
      for (int t = 0; t < ROW_MAX_TERMS; ++t)
        if (t < n_terms) af += ((termw[t * nch + (c >> 6)] >> (c & 63)) & 1) ? wt[t] : 0;
      return af;
    };
    if (s_aff) {
      __syncthreads();  // tdesc
      for (int x = tid; x < n_terms * nch; x += NTH) {
        const int t = x / nch, ch = x - t * nch;
        const int ne = tdesc[t], io = tdesc[ROW_MAX_TERMS + t];
        uint64_t m = ~0ull;
        if (plen <= ROW_PRE_PROG && ne >= 1 && ne <= 4) {  // the rows' loads together (ids repeat past ne: AND is idempotent)
          uint64_t r[4];
#pragma unroll
          for (int i = 0; i < 4; ++i) {
            const int id = (int)pr[17 + io + (i < ne ? i : ne - 1)];
            r[i] = ldg(a->b.req_mask, (uint32_t)id * (uint32_t)nch + (uint32_t)ch);
          }
          m = r[0] & r[1] & r[2] & r[3];
        } else {
          for (int i = 0; i < ne; ++i) {
            const int id = plen <= ROW_PRE_PROG ? (int)pr[17 + io + i] : ldg(sp, (uint32_t)(io + i));
            m &= ldg(a->b.req_mask, (uint32_t)id * (uint32_t)nch + (uint32_t)ch);
          }
        }
        termw[x] = m;
      }
      __syncthreads();
    }
    KAD_PT(t1a);
    KAD_PADD(6, t1a - t1);
    const double rqcd = (double)rqc, rqmd = (double)rqm;
    int ttmax = 0, amax = 0;
    // the unit's tolerated PreferNoSchedule words, once (scalar)
    uint64_t tpn[TFOLD_MAX_TW];
#pragma unroll
    for (int tw = 0; tw < TFOLD_MAX_TW; ++tw) tpn[tw] = (s_tt && tw < TW) ? ldc(a->b.tol_pns + (size_t)tsc * TW + tw) : 0ull;
    // ROW_RU positions per trip: every gather of all of them is issued before any is used (the phase is
    // latency-bound: its resource, taint and affinity parts cost cycles in proportion to their load chains)
    constexpr int RU = ROW_RU;
    for (int j0 = tid; j0 < n; j0 += RU * NTH) {
      auto as = rargs();
      double4 r4[RU];
      float2 iv[RU];
      uint64_t pn[RU][TFOLD_MAX_TW];
      uint32_t cs[RU];
#pragma unroll
      for (int u = 0; u < RU; ++u) {
        const int j = j0 + u * NTH;
        cs[u] = idx[j < n ? j : j0];
      }
#pragma unroll
      for (int u = 0; u < RU; ++u) {
        r4[u] = make_double4(0.0, 0.0, 1.0, 1.0);
        iv[u] = make_float2(0.f, 0.f);
        if (s_res) {  // (available cpu, available mem, cap cpu, cap mem) as f64, f32 100 / cap
          r4[u] = as->s.res4[cs[u]];
          iv[u] = as->s.res_iv[cs[u]];
        }
        if (s_tt) {  // one 32-B gather (SnapDev::pns4: the row kernel runs on clean snapshots, TW <= 4)
          const ulonglong4 q = as->s.pns4[cs[u]];
          pn[u][0] = q.x;
          pn[u][1] = q.y;
          pn[u][2] = q.z;
          pn[u][3] = q.w;
        } else {
#pragma unroll
          for (int tw = 0; tw < TFOLD_MAX_TW; ++tw) pn[u][tw] = 0ull;
        }
      }
#pragma unroll
      for (int u = 0; u < RU; ++u) {
        const int j = j0 + u * NTH;
        if (j >= n) break;
        const uint32_t c = cs[u];
        int x = 0;
        if (s_res) {  // the wide kernel's clean path: x = available - request, exact in f64
          const double capc = r4[u].z, capm = r4[u].w;
          const double xc = r4[u].x - rqcd, xm = r4[u].y - rqmd;
          const float ivc = iv[u].x, ivm = iv[u].y;
          const double xcp = fmax(xc, 0.0), xmp = fmax(xm, 0.0);
          const int okc = -(int)(xc >= 0.0), okm = -(int)(xm >= 0.0);
          if (sm & BIT(KAD_PL_LEAST_ALLOCATED)) x += (quot100(xcp, capc, ivc) + quot100(xmp, capm, ivm)) >> 1;
          if (sm & BIT(KAD_PL_MOST_ALLOCATED))
            x += ((quot100(capc - xcp, capc, ivc) & okc) + (quot100(capm - xmp, capm, ivm) & okm)) >> 1;
          if (sm & BIT(KAD_PL_BALANCED_ALLOCATION)) x += (int)balanced_d((capc - xc) / capc, (capm - xm) / capm);
        }
        int tc = 0;
        if (s_tt)  // taint_toleration.go:91-118: PreferNoSchedule taints not tolerated
#pragma unroll
          for (int tw = 0; tw < TFOLD_MAX_TW; ++tw)
            if (tw < TW) tc += popc64(pn[u][tw] & ~tpn[tw]);
        int af = 0;
        if (s_aff) {  // |raw| <= 2^20 (wider units were deferred above)
          af = raw_aff(c);
          amax = af > amax ? af : amax;
        }
        // x <= 300 (three resource scores), tc <= 256 (TW <= 4); the raw affinity score rides along when the
        // unit's weights keep it within 13 signed bits, so the normalisation does not recompute it
        key[j] = (uint32_t)x | ((uint32_t)tc << 10) | (apack ? ((uint32_t)af & 0x1FFFu) << 19 : 0u);
        ttmax = tc > ttmax ? tc : ttmax;
      }
    }
    KAD_PT(t1b);
    KAD_PADD(7, t1b - t1a);
    if (s_tt) ttmax = row_block_max<NW>(ttmax, red, NWV);
    if (s_aff) amax = row_block_max<NW>(amax, red, NWV);
    __syncthreads();
    KAD_PT(t2);
    KAD_PADD(2, t2 - t1);

    // ---------------- DefaultNormalizeScore + totals, stored order-preserving as u32 (total ^ 2^31)
    int mn = INT32_MAX, mx = INT32_MIN;
    for (int j = tid; j < n; j += NTH) {
      const uint32_t x = key[j];
      int t = (int)(x & 0x3FFu);
      if (s_tt) t += ttmax == 0 ? 100 : 100 - (int)small_quot(100 * (int)((x >> 10) & 0x1FFu), ttmax);
      if (s_aff) {
        const int af = apack ? ((int32_t)x >> 19) : raw_aff(idx[j]);
        const int num = 100 * af;
        t += amax == 0 ? af : (num >= 0 && num < (1 << 24) ? (int)small_quot(num, amax) : num / amax);
      }
      key[j] = (uint32_t)t ^ 0x80000000u;
      mn = t < mn ? t : mn;
      mx = t > mx ? t : mx;
    }
    mn = row_block_min<NW>(mn, red, NWV);
    mx = row_block_max<NW>(mx, red, NWV);
    KAD_PT(t3);
    KAD_PADD(3, t3 - t2);

    // ---------------- select (framework.go:183-209, max_cluster.go:42-66)
    uint16_t* inv = nullptr;  // ranks after a replay (LDS or the block's slab)
    // mode: -1 nothing, 0 all, 1 total >= T, 3 replay ranks < k
    int mode = k >= n ? 0 : (k <= 0 ? -1 : 1);
    uint32_t rflags = 0;
    uint32_t Tk = 0;  // the k-th largest total, sign-flipped
    if (mode == 1) {
      const uint32_t base = (uint32_t)mn ^ 0x80000000u;
      const uint32_t span = (uint32_t)mx - (uint32_t)mn;
      uint32_t prefix = 0, pmask = 0;
      int kk = k;
      if (span != 0) {
        const int bits = 32 - __builtin_clz(span);
        // digits from the top: the first pass takes the span's top 8 bits (C5's totals span ~9 bits: 8-bit
        // digits aligned at bit 8 put every position into 2 bins, thousands of LDS atomics on two words)
        for (int hi = bits; hi > 0; hi -= 8) {
          const int shift = hi > 8 ? hi - 8 : 0;
          const uint32_t dmask = (1u << (hi - shift)) - 1u;
          for (int i = tid; i < 256; i += NTH) hist[i] = 0;  // (NTH >= 256 on every caller; any NTH is correct)
          __syncthreads();
          for (int j = tid; j < n; j += NTH) {
            const uint32_t d = key[j] - base;
            if ((d & pmask) == prefix) atomicAdd(&hist[(d >> shift) & dmask], 1u);
          }
          __syncthreads();
          if (wv == 0) {  // lane l owns digits 255-4l .. 252-4l (descending)
            int h[4], s4 = 0;
#pragma unroll
            for (int q = 0; q < 4; ++q) {
              h[q] = (int)hist[255 - 4 * lane - q];
              s4 += h[q];
            }
            const int incl = wave_incl_sum_i32(s4);
            const int excl = incl - s4;
            if (excl < kk && kk <= incl) {
              int cum = excl;
#pragma unroll
              for (int q = 0; q < 4; ++q) {
                if (cum + h[q] >= kk) {
                  bc[1] = 255 - 4 * lane - q;
                  bc[2] = cum;
                  break;
                }
                cum += h[q];
              }
            }
          }
          __syncthreads();
          const int digit = __builtin_amdgcn_readfirstlane(bc[1]), above = __builtin_amdgcn_readfirstlane(bc[2]);
          kk -= above;
          prefix |= (uint32_t)digit << shift;
          pmask |= dmask << shift;
        }
      }
      Tk = base + prefix;
      int g = 0, e = 0;
      for (int j = tid; j < n; j += NTH) {
        const uint32_t t = key[j];
        g += t > Tk;
        e += t == Tk;
      }
      g = row_block_sum<NW>(g, red, NWV);
      e = row_block_sum<NW>(e, red, NWV);
      KAD_PT(t4);
      KAD_PADD(4, t4 - t3);
      if (k - g != e) {  // ties straddle the cut: Go's pdqsort decides which tied clusters stay (n > 256)
        rflags = KAD_RF_TIE_STRADDLE;
        mode = 3;
        const bool in_lds = n <= ROW_NREP;
        const size_t Cp = (size_t)nch * 64;
        uint16_t* pid = in_lds ? pid_l : pid_g;
        uint16_t* posl = in_lds ? posl_l : pid_g + Cp;
        uint16_t* posr = in_lds ? posr_l : pid_g + 2 * Cp + 64;
        inv = posl;
        // packed replay (key - min << 16 | position: every C5 row, n <= C < 2^16) unless the totals span 2^16
        const bool packed = (uint32_t)mx - (uint32_t)mn < 65536u;
        for (int j = tid; j < n; j += NTH) {
          if (packed)
            key[j] = (((key[j] ^ 0x80000000u) - (uint32_t)mn) << 16) | (uint32_t)j;
          else
            pid[j] = (uint16_t)j;
        }
        __syncthreads();
        const int xs_b = (a->p.flags & KAD_PROFILE_XORSHIFT_GO121) ? 7 : 17;
        const int xs_c = (a->p.flags & KAD_PROFILE_XORSHIFT_GO121) ? 17 : 5;
        // packed: the partitions of ranges longer than ROW_BLOCK_PART run on all 8 waves, then wave 0 goes
        // on alone (red[] is free scratch here)
        did_pf = true;  // wave 1 prefetches the next unit while wave 0 finishes the replay alone
        if (packed && in_lds) {
          PdqWaveP<> pw{key, posl, posr, xs_b, xs_c};
          const auto st = pw.select_block(n, k, ROW_BLOCK_PART, NWV, wv, red);
          if (wv == 0) pw.select_from(st, k);
          else if (wv == 1) prefetch();
        } else if (packed) {  // elements stay in LDS; stopper scratch in the slab (workgroup fences order both)
          PdqWaveP<true> pw{key, posl, posr, xs_b, xs_c};
          const auto st = pw.select_block(n, k, ROW_BLOCK_PART, NWV, wv, red);
          if (wv == 0) pw.select_from(st, k);
          else if (wv == 1) prefetch();
        } else if (wv == 1) {
          prefetch();
        } else if (wv == 0) {
          if (in_lds) {
            PdqWave<uint32_t> pw{key, pid, posl, posr, xs_b, xs_c};
            pw.select(n, k);
          } else {  // keys stay in LDS; positions in the slab (workgroup-scope fences order both)
            PdqWave<uint32_t, true> pw{key, pid, posl, posr, xs_b, xs_c};
            pw.select(n, k);
          }
        }
        __syncthreads();
        for (int r = tid; r < n; r += NTH) inv[packed ? (key[r] & 0xFFFFu) : pid[r]] = (uint16_t)r;
        __syncthreads();
        KAD_PT(t5);
        KAD_PADD(5, t5 - t4);
      }
    }

    // ---------------- output, ascending cluster id (= ascending position)
    if (!did_pf && wv == 1) prefetch();  // (into the other buffers: the output pass uses this unit's cnt)
    const bool dup = fc & KAD_W_DUPLICATE;
    const bool replicas =
        !dup && a->p.replicas_plugin == KAD_PL_CLUSTER_CAPACITY_WEIGHT && (fc & REC_DESIRED_POS) && k > 0;
    int total = 0;
    if ((dup || replicas) && mode >= 0) {
      const int nq = (n + 63) >> 6;
      auto selected = [&](int p) -> bool {
        if (p >= n) return false;
        if (mode == 0) return true;
        if (mode == 1) return key[p] >= Tk;
        return inv[p] < k;
      };
      for (int q = wv; q < nq; q += NWV) {
        const uint64_t m = ballot(selected(q * WAVE + lane));
        if (lane == 0) cnt[q] = popc64(m);
      }
      __syncthreads();
      row_exclusive_scan(cnt, nq);
      __syncthreads();
      total = __builtin_amdgcn_readfirstlane(cnt[nq]);
      auto ao = rargs();
      int32_t* oc = ao->o.cluster + ooff;
      int64_t* orp = ao->o.replicas + ooff;
      for (int q = wv; q < nq; q += NWV) {
        const int p = q * WAVE + lane;
        const bool s = selected(p);
        const uint64_t m = ballot(s);
        if (s) {
          const uint32_t at = (uint32_t)(cnt[q] + mbcnt(m));
          stg(oc, at, (int32_t)idx[p]);
          stg(orp, at, (int64_t)(dup ? -1 : 0));
        }
      }
    }
    if (tid == 0) {
      auto ao = rargs();
      ao->o.status[w] = KAD_ST_OK;
      ao->o.count[w] = total;  // Divide without replicas plugin: empty map
      ao->o.flags[w] = rflags;
    }
  }
#ifdef KAD_PHASE_PROF
  // per-block (start, end, units) of the last launch in g_wavetime / g_wavex (the wide kernel's slots)
  if (tid == 0 && blockIdx.x < 8192) {
    g_wavetime[2 * blockIdx.x] = rt_start;
    g_wavetime[2 * blockIdx.x + 1] = __builtin_amdgcn_s_memrealtime();
    g_wavex[6 * blockIdx.x] = rt_units;
  }
#endif
  KAD_PFLUSH_ROW;
}

template <int SM>
__device__ __attribute__((noinline)) void wide_rows(char* smem, WArgs a) {
  row_units<SM, 0>([a] { return a; }, smem, 0);
}

template <int SM = -1>
__global__ __launch_bounds__(ROW_THREADS, KAD_ROW_MINW) void schedule_row_kernel(RowArgs args) {
  (void)args;  // read through kernarg<RowArgs>()
  extern __shared__ __attribute__((aligned(16))) char smem[];
#if defined(KAD_PHASE_PROF) || defined(KAD_TUNING)
  const int rexp = kernarg<RowArgs>()->exp;
#else
  constexpr int rexp = 0;
#endif
  row_units<SM, ROW_THREADS>([] { return kernarg<RowArgs>(); }, smem, rexp);
}

}  // namespace kad
