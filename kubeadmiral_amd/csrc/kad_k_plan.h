// plan_hdr_kernel, plan_kernel, plan_pair_kernel: replica planning of Divide-mode units.
// Part of kad_kernels.hip's translation unit, which includes the kernels' headers in definition order.
#pragma once

#include "kad_device.h"
#include "kad_plan.h"
#include "kad_prof.h"
#include "kad_wave.h"

namespace kad {

struct PlanLayout {
  size_t cid, hash, w, mn, mx, cap, cur, fl, plan, over, ofl, w2, mx2, adj, plan2, over2, ofl2, ord, act, act2, bytes;
};
__host__ __device__ inline PlanLayout plan_layout(int K) {
  const size_t Kp = (size_t)((K + 63) & ~63);
  PlanLayout L;
  size_t o = 0;
  auto take = [&](size_t n) {
    size_t r = o;
    o += (n + 15) & ~(size_t)15;
    return r;
  };
  L.w = take(8 * Kp);
  L.mn = take(8 * Kp);
  L.mx = take(8 * Kp);
  L.cap = take(8 * Kp);
  L.cur = take(8 * Kp);
  L.plan = take(8 * Kp);
  L.over = take(8 * Kp);
  L.w2 = take(8 * Kp);
  L.mx2 = take(8 * Kp);
  L.adj = take(8 * Kp);
  L.plan2 = take(8 * Kp);
  L.over2 = take(8 * Kp);
  L.cid = take(4 * Kp);
  L.hash = take(4 * Kp);
  L.fl = take(4 * Kp);
  L.ofl = take(4 * Kp);
  L.ofl2 = take(4 * Kp);
  L.ord = take(4 * Kp);
  L.act = take(4 * Kp);
  L.act2 = take(4 * Kp);
  L.bytes = o;
  return L;
}

__device__ PlanWs plan_ws(char* region, int K) {
  const PlanLayout L = plan_layout(K);
  PlanWs ws;
  ws.cid = (int32_t*)(region + L.cid);
  ws.hash = (uint32_t*)(region + L.hash);
  ws.w = (int64_t*)(region + L.w);
  ws.mn = (int64_t*)(region + L.mn);
  ws.mx = (int64_t*)(region + L.mx);
  ws.cap = (int64_t*)(region + L.cap);
  ws.cur = (int64_t*)(region + L.cur);
  ws.fl = (uint32_t*)(region + L.fl);
  ws.plan = (int64_t*)(region + L.plan);
  ws.over = (int64_t*)(region + L.over);
  ws.ofl = (uint32_t*)(region + L.ofl);
  ws.w2 = (int64_t*)(region + L.w2);
  ws.mx2 = (int64_t*)(region + L.mx2);
  ws.adj = (int64_t*)(region + L.adj);
  ws.plan2 = (int64_t*)(region + L.plan2);
  ws.over2 = (int64_t*)(region + L.over2);
  ws.ofl2 = (uint32_t*)(region + L.ofl2);
  ws.ord = (int32_t*)(region + L.ord);
  ws.act = (int32_t*)(region + L.act);
  ws.act2 = (int32_t*)(region + L.act2);
  return ws;
}

// binary search of cluster id c in a sorted CSR slice [lo, hi)
__device__ __forceinline__ int find_sorted(const int32_t* a, int lo, int hi, int c) {
  while (lo < hi) {
    const int mid = (lo + hi) >> 1;
    const int v = a[mid];
    if (v == c) return mid;
    if (v < c)
      lo = mid + 1;
    else
      hi = mid;
  }
  return -1;
}

// LANES: rows of K <= 64 only, the planner in registers (8 waves / SIMD: <= 64 VGPRs); else rows of
// K > 64 only, with the LDS / global-scratch workspace (GSCR). launch_plan runs the first and, when
// some row may exceed 64 clusters, the second; each skips the other's rows.
// PlanRowHdr of every planner row (once per batch upload): one lane per row
__global__ __launch_bounds__(256) void plan_hdr_kernel(BatchDev b, const int32_t* rows, int n_rows, PlanRowHdr* out) {
  const int r = blockIdx.x * 256 + threadIdx.x;
  if (r >= n_rows) return;
  const int w = rows[r];
  PlanRowHdr h;
  h.w = w;
  h.flags = b.flags[w];
  h.off = b.out_off[w];
  h.slots = (int32_t)(b.out_off[w + 1] - b.out_off[w]);
  h.p0 = b.pref_off[w];
  h.p1 = b.pref_off[w + 1];
  h.c0 = b.cur_off[w];
  h.c1 = b.cur_off[w + 1];
  h.k0 = b.key_off[w];
  h.k1 = b.key_off[w + 1];
  h.pad = 0;
  h.desired = b.desired[w];
  h.pad2 = 0;
  out[r] = h;
}

template <bool GSCR, bool LANES>
__global__ __launch_bounds__(64, LANES ? 8 : 1) void plan_kernel(SnapDev s, BatchDev b, OutDev o, const PlanRowHdr* rows,
                                                                 int n_rows, int kmax, char* gscratch, int wave_bytes,
                                                                 int r_stride, int tbl_cp, const int32_t* list = nullptr,
                                                                 const int32_t* list_n = nullptr) {
  // list (LANES only): the rows plan_pair_kernel left to the 64-lane planner (32 < K <= 64): row list[i] for
  // i < *list_n instead of row i
  if (list) n_rows = __hip_atomic_load(list_n, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = lane_id_h();
  const int gw = blockIdx.x;
  // LDS: the row workspace of rows with K > 64 (kmax > 64 only), then the lookup tables
  char* region = GSCR ? gscratch + (size_t)gw * wave_bytes : smem;
  const size_t ws_bytes = (GSCR || LANES || kmax <= WAVE) ? 0 : plan_layout(kmax).bytes;
  // cluster id → (row tag << 16 | preference / current-cluster index + 1) lookup tables in LDS
  // (tbl_cp > 0), written per row and never cleared: an entry counts only with the row's tag (the wave's
  // row counter; the tables are zeroed when it wraps). Replaces two binary searches in global memory per
  // selected cluster.
  uint32_t* tbl_p = (uint32_t*)(smem + ws_bytes);
  uint32_t* tbl_c = tbl_p + tbl_cp;
  uint64_t* kbuf = LANES ? (uint64_t*)(smem + ws_bytes + (size_t)tbl_cp * 8) : nullptr;  // sort keys (64)
  const bool use_tbl = !GSCR && tbl_cp > 0;
  uint32_t tag = 0;
  if (use_tbl) {  // LDS starts undefined: no entry may carry a tag before its row writes it
    for (int i = lane; i < 2 * tbl_cp; i += WAVE) tbl_p[i] = 0;
    wsync<GSCR>();
  }
  KAD_PACC;
  // XCD-aware row ranges (grid a multiple of 8; blocks go round-robin over the 8 XCDs): the blocks of XCD
  // x walk the x-th contiguous eighth of the rows, so neighbouring rows — which share the cache lines of
  // the per-unit columns (status, count, flags, headers, slot ids, preference columns) — are read through
  // one L2 instead of once by each XCD's L2 (C4: FETCH_SIZE per launch 1.09 -> 0.54 GB, time unchanged)
  int r_lo = gw, r_hi = n_rows, r_st = r_stride;
  if ((r_stride & 7) == 0 && r_stride >= 8) {
    const int x = gw & 7;
    r_lo = (int)((int64_t)n_rows * x / 8) + (gw >> 3);
    r_hi = (int)((int64_t)n_rows * (x + 1) / 8);
    r_st = r_stride >> 3;
  }
  // the row's PlanRowHdr in lanes 0..15 (one 64-B line), loaded one row ahead
  auto fetch_hdr = [&](int r) -> uint32_t {
    if (r >= r_hi) return 0u;
    const int rr = list ? ldc(list + r) : r;
    return lane < 16 ? ldg((const uint32_t*)(rows + rr), (uint32_t)lane) : 0u;
  };
  uint32_t hn = fetch_hdr(r_lo);
  for (int r = r_lo; r < r_hi; r += r_st) {
    KAD_PT(t0);
    const uint32_t hc = hn;
    hn = fetch_hdr(r + r_st);
    auto hf = [&](int d) -> uint32_t { return (uint32_t)__builtin_amdgcn_readlane((int)hc, d); };
    const int w = (int)hf(0);
    const uint32_t f = hf(1);
    const int64_t off = (int64_t)(((uint64_t)hf(3) << 32) | hf(2));
    const int slots = (int)hf(4);
    const int p0 = (int)hf(5), p1 = (int)hf(6);
    const int c0 = (int)hf(7), c1 = (int)hf(8);
    const int ko0 = (int)hf(9), ko1 = (int)hf(10);
    const int64_t desired = (int64_t)(((uint64_t)hf(13) << 32) | hf(12));
    // everything this row reads next issues together (one memory round trip): the schedule stage's status,
    // count and flags, the unit's slot ids (within its bound, whatever the count), key bytes, and (K <= 64)
    // the preference / current-cluster ids for the lookup tables
    const int st = o.status[w];
    const int K = o.count[w];
    const uint32_t rflags0 = o.flags[w];
    const uint8_t* key = b.key + ko0;
    const int klen = ko1 - ko0;
    // su.Key() bytes in lanes (uniform): the FNV-1 continuation of every element
    // reads them with v_readlane instead of one dependent load per byte
    const uint32_t kb0 = lane < klen ? (uint32_t)key[lane] : 0u;
    int c_l = 0;
    if (LANES && slots > 0) c_l = o.cluster[off + (lane < slots ? lane : 0)];  // (no slot: nothing to read)
    // the lookup tables' first 64 preference / current-cluster ids (uniform guards, clamped lanes: no
    // exec branch), so that the name hashes and the preference columns below share the next round trip
    int pid_l = 0, cid_l = 0;
    if (use_tbl && p1 > p0) pid_l = b.pref_id[p0 + (p0 + lane < p1 ? lane : 0)];
    if (use_tbl && c1 > c0) cid_l = b.cur_id[c0 + (c0 + lane < c1 ? lane : 0)];
    if (st != KAD_ST_OK || K <= 0 || (K <= WAVE) != LANES) continue;
    const int64_t total = (f & KAD_W_HAS_DESIRED) ? desired : 0;
    // rows of K <= 64: element `lane`'s name hash (and cores) are loaded before the lookup tables are
    // filled, so those loads and the tables' index loads share one memory round trip
    uint32_t h_l = 0;
    int64_t ac_l = 0, av_l = 0;  // cores for dynamic weights (rsp.go:183-272)
    if constexpr (LANES) {
      const int first_c = __builtin_amdgcn_readfirstlane(c_l);  // (every lane active: lane 0 holds element 0)
      if (lane >= K) c_l = first_c;  // past K: element 0 (masked off later)
      h_l = s.name_fnv[c_l];
      if (f & KAD_W_DYNAMIC_WEIGHTS) {
        ac_l = s.alloc_cores[c_l];
        av_l = s.avail_cores[c_l];
      }
    }
    // preferences (rsp.go:99-126)
    if (use_tbl) {
      tag = (tag + 1) & 0xFFFFu;
      if (tag == 0) {  // wrapped: no stale entry may carry a live tag
        for (int i = lane; i < 2 * tbl_cp; i += WAVE) tbl_p[i] = 0;
        wsync<GSCR>();
        tag = 1;
      }
      if (p0 + lane < p1) tbl_p[pid_l] = (tag << 16) | (uint32_t)(lane + 1);
      if (c0 + lane < c1) tbl_c[cid_l] = (tag << 16) | (uint32_t)(lane + 1);
      for (int j = p0 + WAVE + lane; j < p1; j += WAVE) tbl_p[b.pref_id[j]] = (tag << 16) | (uint32_t)(j - p0 + 1);
      for (int j = c0 + WAVE + lane; j < c1; j += WAVE) tbl_c[b.cur_id[j]] = (tag << 16) | (uint32_t)(j - c0 + 1);
      wsync<GSCR>();
    }
    // element i: cluster id, hash, preference columns, current replicas
    auto gather = [&](int i, int& c, PlanLane& e) {
      uint32_t h;
      if constexpr (LANES) {
        c = c_l;  // i == lane (or 0 past K)
        h = h_l;
      } else {
        c = o.cluster[off + i];
        h = s.name_fnv[c];
      }
      int pi, ci;
      if (use_tbl) {
        const uint32_t tp = tbl_p[c], tc = tbl_c[c];
        pi = (tp >> 16) == tag ? p0 + (int)(tp & 0xFFFFu) - 1 : -1;
        ci = (tc >> 16) == tag ? c0 + (int)(tc & 0xFFFFu) - 1 : -1;
      } else {
        pi = find_sorted(b.pref_id, p0, p1, c);
        ci = find_sorted(b.cur_id, c0, c1, c);
      }
      e.fl = 0;
      e.w = e.mn = e.mx = e.cap = 0;
      if (pi >= 0) {
        // all five columns in one round trip (pi is in bounds), flags select after
        const uint32_t pf = b.pref_fl[pi];
        int64_t pw, pmx, pcp;
        if (b.pref_narrow) {  // i32 columns (KAD_BATCH_NARROW_PREFS)
          pw = b.pref_w32[pi];
          pmx = b.pref_max32[pi];
          pcp = b.pref_cap32[pi];
          e.mn = b.pref_min32[pi];
        } else {
          pw = b.pref_w[pi];
          pmx = b.pref_max[pi];
          pcp = b.pref_cap[pi];
          e.mn = b.pref_min[pi];
        }
        if (pf & KAD_PREF_HAS_WEIGHT) e.w = pw;
        if (pf & KAD_PREF_HAS_MAX) {
          e.fl |= EF_HAS_MAX;
          e.mx = pmx;
        }
        if (pf & KAD_PREF_HAS_CAP) {
          e.fl |= EF_HAS_CAP;
          e.cap = pcp;
        }
      }
      e.cur = ci >= 0 ? b.cur_rep[ci] : 0;
      // the FNV-1 continuation after the column loads are issued: the name hash's load and theirs share
      // one round trip
      for (int k0 = 0; k0 < klen; k0 += WAVE) {
        const uint32_t kb = k0 == 0 ? kb0 : (k0 + lane < klen ? (uint32_t)key[k0 + lane] : 0u);
        const int m = klen - k0 < WAVE ? klen - k0 : WAVE;
        for (int q = 0; q < m; ++q) {
          h *= 16777619u;
          h ^= (uint32_t)__builtin_amdgcn_readlane((int)kb, q);
        }
      }
      e.hash = h;
    };
    const bool avoid = f & KAD_W_AVOID_DISRUPTION;
    const bool keep = f & KAD_W_KEEP_UNSCHED;
    uint32_t rflags = rflags0;
    if constexpr (LANES) {
      // ---------------- one element per lane, the planner in registers (kad_plan.h plan_row_lanes)
      const bool v = lane < K;
      // every lane runs the gather (its FNV loop reads the key bytes of all lanes with v_readlane, so the
      // lanes that hold them must be live); lanes past K take element 0 and are masked off
      int c = 0;
      PlanLane e;
      gather(v ? lane : 0, c, e);
      if (!v) {
        e = PlanLane{0, 0, 0, 0, 0, 0u, 0u};
        c = 0;
      }
      wsync<GSCR>();  // the next row's table writes follow this row's reads
      KAD_PT(t1);
      KAD_PADD(0, t1 - t0);
      KAD_PADD(5, 1);
      if (f & KAD_W_DYNAMIC_WEIGHTS) {
        // CalcWeightLimit (rsp.go:183-213) + AvailableToPercentage (rsp.go:215-272)
        const int64_t ac = v ? ac_l : 0, av = v ? av_l : 0;
        const double sum = wave_sum_f64(v ? (double)ac : 0.0);
        const double suma = wave_sum_f64((v && av > 0) ? (double)av : 0.0);
        if (suma == 0) {
          e.w = v ? go_f2i(round(1000.0 / (double)K)) : 0;
        } else {
          const int64_t lim = sum == 0 ? go_f2i(round(1000.0 / (double)K))
                                       : go_f2i(round((double)ac / sum * 1000.0 * 1.4));
          const double avd = av < 0 ? 0.0 : (double)av;
          int64_t wt = go_f2i(round(avd / suma * 1000.0));
          if (wt > lim) wt = lim;
          const int64_t sumtmp = wave_sum_i64(v ? wt : 0);
          wt = go_f2i(round((double)wt / (double)sumtmp * 1000.0));
          const int64_t other = wave_sum_i64(v ? wt : 0);
          const int64_t maxw = wave_max_i64(v ? wt : 0);
          e.w = v ? wt : 0;
          if (maxw > 0) {  // remainder → first strict maximum (lowest cluster id among ties)
            const uint64_t tm = ballot(v && wt == maxw);
            const int first = (int)__builtin_ctzll(tm);
            if (popc64(tm) > 1) rflags |= KAD_RF_REMAINDER_TIE;
            if (lane == first) e.w = wadd(e.w, wsub(1000, other));
          }
        }
      }
      KAD_PT(t2);
      KAD_PADD(1, t2 - t1);
      PlanOut po;
      rflags |= plan_row_lanes(e, K, total, avoid, keep, po, kbuf);
      KAD_PT(t3);
      KAD_PADD(2, t3 - t2);
      // result = plan + overflow, zeros dropped (rsp.go:162-179), ascending cluster id
      const int64_t rr = v ? wadd(po.plan, (po.ofl & EF_HAS_OVER) ? po.over : 0) : 0;
      const bool nz = v && rr != 0;
      const uint64_t m = ballot(nz);
      if (nz) {
        const int64_t at = off + mbcnt(m);
        o.cluster[at] = c;
        o.replicas[at] = rr;
      }
      if (lane == 0) {
        o.count[w] = popc64(m);
        o.flags[w] = rflags;
      }
      KAD_PT(t4);
      KAD_PADD(3, t4 - t3);
      continue;
    } else {
    // ---------------- K > 64: the row state in the LDS / global-scratch workspace (kad_plan.h plan_row)
    PlanWs ws = plan_ws(region, K);
    for (int i0 = 0; i0 < K; i0 += WAVE) {
      const int i = i0 + lane;
      int c;
      PlanLane e;
      gather(i < K ? i : 0, c, e);  // every lane (see the K <= 64 path)
      if (i < K) {
        ws.cid[i] = c;
        ws.hash[i] = e.hash;
        ws.w[i] = e.w;
        ws.mn[i] = e.mn;
        ws.mx[i] = e.mx;
        ws.cap[i] = e.cap;
        ws.fl[i] = e.fl;
        ws.cur[i] = e.cur;
      }
    }
    wsync<GSCR>();
    KAD_PT(t1);
    KAD_PADD(0, t1 - t0);
    KAD_PADD(5, 1);
    if (f & KAD_W_DYNAMIC_WEIGHTS) {
      // CalcWeightLimit (rsp.go:183-213) + AvailableToPercentage (rsp.go:215-272)
      double sum = 0.0, suma = 0.0;
      for (int i = lane; i < K; i += WAVE) {
        const int c = ws.cid[i];
        sum += (double)s.alloc_cores[c];
        const int64_t av = s.avail_cores[c];
        if (av > 0) suma += (double)av;
      }
      sum = wave_sum_f64(sum);
      suma = wave_sum_f64(suma);
      if (suma == 0) {
        const int64_t even = go_f2i(round(1000.0 / (double)K));
        for (int i = lane; i < K; i += WAVE) ws.w[i] = even;
      } else {
        int64_t sumtmp = 0;
        for (int i = lane; i < K; i += WAVE) {
          const int c = ws.cid[i];
          const int64_t lim = sum == 0 ? go_f2i(round(1000.0 / (double)K))
                                       : go_f2i(round((double)s.alloc_cores[c] / sum * 1000.0 * 1.4));
          double v = (double)s.avail_cores[c];
          if (v < 0.0) v = 0.0;
          int64_t wt = go_f2i(round(v / suma * 1000.0));
          if (wt > lim) wt = lim;
          ws.w[i] = wt;
          sumtmp = wadd(sumtmp, wt);
        }
        sumtmp = wave_sum_i64(sumtmp);
        int64_t other = 0, maxw = 0;
        for (int i = lane; i < K; i += WAVE) {
          const int64_t wt = go_f2i(round((double)ws.w[i] / (double)sumtmp * 1000.0));
          ws.w[i] = wt;
          other = wadd(other, wt);
          maxw = wt > maxw ? wt : maxw;
        }
        other = wave_sum_i64(other);
        maxw = wave_max_i64(maxw);
        wsync<GSCR>();
        if (maxw > 0) {  // remainder → first strict maximum (lowest cluster id among ties)
          int first = K, ties = 0;
          for (int i = lane; i < K; i += WAVE) {
            if (ws.w[i] == maxw) {
              first = i < first ? i : first;
              ties++;
            }
          }
          for (int m = 32; m >= 1; m >>= 1) {
            const int of = __shfl_xor(first, m);
            first = of < first ? of : first;
          }
          ties = wave_sum_i32(ties);
          if (ties > 1) rflags |= KAD_RF_REMAINDER_TIE;
          if (lane == 0) ws.w[first] = wadd(ws.w[first], wsub(1000, other));
        }
      }
      wsync<GSCR>();
    }
    KAD_PT(t2);
    KAD_PADD(1, t2 - t1);
    rflags |= plan_row<GSCR>(ws, K, total, avoid, keep);
    KAD_PT(t3);
    KAD_PADD(2, t3 - t2);
    // result = plan + overflow, zeros dropped (rsp.go:162-179), ascending cluster id
    int base = 0;
    for (int i0 = 0; i0 < K; i0 += WAVE) {
      const int i = i0 + lane;
      int64_t r = 0;
      if (i < K) r = wadd(ws.plan[i], (ws.ofl[i] & EF_HAS_OVER) ? ws.over[i] : 0);
      const bool nz = i < K && r != 0;
      const uint64_t m = ballot(nz);
      if (nz) {
        const int64_t at = off + base + mbcnt(m);
        o.cluster[at] = ws.cid[i];
        o.replicas[at] = r;
      }
      base += popc64(m);
    }
    if (lane == 0) {
      o.count[w] = base;
      o.flags[w] = rflags;
    }
    wsync<GSCR>();
    KAD_PT(t4);
    KAD_PADD(3, t4 - t3);
    }
  }
  KAD_PFLUSH_PLAN;
}

// plan_pair_kernel — rows of K <= 32, two per wave (kad_plan.h plan_row_pair): row A (the wave's r-th row) in
// lanes 0-31, row B (the next row of its range) in lanes 32-63; C4's rows hold 15 selected clusters on
// average, so the 64-lane planner (one row per wave) left three quarters of its lanes idle. The same steps as
// plan_kernel<false, true> per segment: the row's header line, the schedule stage's status / count / flags,
// the slot ids, key bytes and preference / current-cluster ids in one round trip; name hashes and cores; the
// lookup tables (u16 per segment: (tag << 10) | (index + 1), rows of more than 1022 ids search the sorted
// lists instead); the preference columns; the FNV-1 continuation; dynamic weights; the plan. Rows with
// 32 < K <= 64 go to `big` (plan_kernel<false, true> runs them next); K > 64 rows are the workspace planner's.
#ifndef KAD_PAIR_MINW
#define KAD_PAIR_MINW 6  // waves per SIMD plan_pair_kernel's VGPR budget is sized for (6: 80 VGPRs; 8 spills, 5 / 7
                         // slower: profiles/r06/ab_c4_pair_planner.txt, ab_c4_planner_occupancy_classes.txt)
#endif
__global__ __launch_bounds__(64, KAD_PAIR_MINW) void plan_pair_kernel(SnapDev s, BatchDev b, OutDev o, const PlanRowHdr* rows,
                                                          int n_rows, int r_stride, int tbl_cp, int32_t* big,
                                                          int32_t* big_n) {
  extern __shared__ __attribute__((aligned(16))) char smem[];
  const int lane = lane_id_h();
  const int sl = lane & 31;
  const bool hi = lane >= 32;
  const int gw = blockIdx.x;
  uint16_t* const tbl = (uint16_t*)smem;  // [kind: pref, cur][segment][tbl_cp]
  uint16_t* const tbl_p = tbl + (hi ? tbl_cp : 0);
  uint16_t* const tbl_c = tbl + 2 * (size_t)tbl_cp + (hi ? tbl_cp : 0);
  uint64_t* const kbuf = (uint64_t*)(smem + (size_t)tbl_cp * 8);
  const bool use_tbl = tbl_cp > 0;
  constexpr int TAG_MAX = 63, IDX_MAX = 1022;
  uint32_t tag = 0;
  auto clear_tables = [&]() {
    for (int i = lane; i < 2 * tbl_cp; i += WAVE) ((uint32_t*)tbl)[i] = 0u;  // 4 tables of tbl_cp u16
    wave_sync();
  };
  if (use_tbl) clear_tables();
  int r_lo = gw, r_hi = n_rows, r_st = r_stride;
  if ((r_stride & 7) == 0 && r_stride >= 8) {  // XCD-contiguous ranges (plan_kernel)
    const int x = gw & 7;
    r_lo = (int)((int64_t)n_rows * x / 8) + (gw >> 3);
    r_hi = (int)((int64_t)n_rows * (x + 1) / 8);
    r_st = r_stride >> 3;
  }
  for (int r = r_lo; r < r_hi; r += 2 * r_st) {
    const int rr = hi ? r + r_st : r;  // this segment's row
    const bool has = rr < r_hi;
    const uint32_t hc = (has && sl < 16) ? ldg((const uint32_t*)(rows + rr), (uint32_t)sl) : 0u;
    auto hf = [&](int d) -> uint32_t { return (uint32_t)seg_read32((int)hc, d); };
    const int w = has ? (int)hf(0) : 0;
    const uint32_t f = hf(1);
    const int64_t off = (int64_t)(((uint64_t)hf(3) << 32) | hf(2));
    const int p0 = (int)hf(5), p1 = (int)hf(6);
    const int c0 = (int)hf(7), c1 = (int)hf(8);
    const int ko0 = (int)hf(9), ko1 = (int)hf(10);
    const int64_t desired = (int64_t)(((uint64_t)hf(13) << 32) | hf(12));
    // the schedule stage's outputs, the slot ids, key bytes and the first 32 preference / current ids together
    const int st = has ? o.status[w] : -1;
    const int Kr = has ? o.count[w] : 0;
    const uint32_t rflags0 = has ? o.flags[w] : 0u;
    const int klen = ko1 - ko0;
    const bool ok = st == KAD_ST_OK && Kr > 0;
    const bool pok = ok && Kr <= 32;
    const int K = pok ? Kr : 0;
    const uint8_t* key = b.key + ko0;
    const uint32_t kb0 = (pok && sl < klen) ? (uint32_t)key[sl] : 0u;
    int c_l = pok ? o.cluster[off + (sl < K ? sl : 0)] : 0;
    const bool tbl_row = use_tbl && p1 - p0 <= IDX_MAX && c1 - c0 <= IDX_MAX;
    int pid_l = 0, cid_l = 0;
    if (pok && tbl_row && p1 > p0) pid_l = b.pref_id[p0 + (p0 + sl < p1 ? sl : 0)];
    if (pok && tbl_row && c1 > c0) cid_l = b.cur_id[c0 + (c0 + sl < c1 ? sl : 0)];
    if (ok && Kr > 32 && Kr <= WAVE && sl == 0) big[atomicAdd(big_n, 1)] = rr;  // the 64-lane planner's
    if (!ballot(pok)) continue;
    const int64_t total = (f & KAD_W_HAS_DESIRED) ? desired : 0;
    const bool dyn = f & KAD_W_DYNAMIC_WEIGHTS;
    const uint32_t h_l = s.name_fnv[c_l];
    int64_t ac_l = 0, av_l = 0;
    if (ballot(pok && dyn)) {
      ac_l = s.alloc_cores[c_l];
      av_l = s.avail_cores[c_l];
    }
    if (use_tbl) {
      if (++tag > TAG_MAX) {  // wrapped: no stale entry may carry a live tag
        clear_tables();
        tag = 1;
      }
      const uint16_t tg = (uint16_t)(tag << 10);
      if (pok && tbl_row) {
        if (p0 + sl < p1) tbl_p[pid_l] = (uint16_t)(tg | (sl + 1));
        if (c0 + sl < c1) tbl_c[cid_l] = (uint16_t)(tg | (sl + 1));
        for (int j = p0 + 32 + sl; j < p1; j += 32) tbl_p[b.pref_id[j]] = (uint16_t)(tg | (j - p0 + 1));
        for (int j = c0 + 32 + sl; j < c1; j += 32) tbl_c[b.cur_id[j]] = (uint16_t)(tg | (j - c0 + 1));
      }
      wave_sync();
    }
    // element sl of this segment's row (lanes past K: element 0, masked off below)
    const bool v = sl < K;
    const int c = c_l;
    PlanLane e;
    {
      int pi, ci;
      if (pok && tbl_row) {
        const uint32_t tp = tbl_p[c], tcc = tbl_c[c];
        pi = (tp >> 10) == tag ? p0 + (int)(tp & 1023u) - 1 : -1;
        ci = (tcc >> 10) == tag ? c0 + (int)(tcc & 1023u) - 1 : -1;
      } else if (pok) {
        pi = find_sorted(b.pref_id, p0, p1, c);
        ci = find_sorted(b.cur_id, c0, c1, c);
      } else {
        pi = ci = -1;
      }
      e.fl = 0;
      e.w = e.mn = e.mx = e.cap = 0;
      if (pi >= 0) {
        const uint32_t pf = b.pref_fl[pi];
        int64_t pw, pmx, pcp;
        if (b.pref_narrow) {
          pw = b.pref_w32[pi];
          pmx = b.pref_max32[pi];
          pcp = b.pref_cap32[pi];
          e.mn = b.pref_min32[pi];
        } else {
          pw = b.pref_w[pi];
          pmx = b.pref_max[pi];
          pcp = b.pref_cap[pi];
          e.mn = b.pref_min[pi];
        }
        if (pf & KAD_PREF_HAS_WEIGHT) e.w = pw;
        if (pf & KAD_PREF_HAS_MAX) {
          e.fl |= EF_HAS_MAX;
          e.mx = pmx;
        }
        if (pf & KAD_PREF_HAS_CAP) {
          e.fl |= EF_HAS_CAP;
          e.cap = pcp;
        }
      }
      e.cur = ci >= 0 ? b.cur_rep[ci] : 0;
      // FNV-1 continuation with su.Key() (planner.go:185-195): the segment's key bytes by readlane
      uint32_t h = h_l;
      const int kmax = wave_max_u_i32(pok ? klen : 0);
      for (int k0 = 0; k0 < kmax; k0 += 32) {
        const uint32_t kb = k0 == 0 ? kb0 : ((pok && k0 + sl < klen) ? (uint32_t)key[k0 + sl] : 0u);
        const int m = kmax - k0 < 32 ? kmax - k0 : 32;
        for (int q = 0; q < m; ++q) {
          const uint32_t byte = (uint32_t)seg_read32((int)kb, q);
          if (k0 + q < klen) h = (h * 16777619u) ^ byte;
        }
      }
      e.hash = h;
    }
    if (use_tbl) wave_sync();  // the next pair's table writes follow these reads
    if (!v) e = PlanLane{0, 0, 0, 0, 0, 0u, 0u};
    uint32_t rflags = rflags0;
    if (ballot(pok && dyn)) {
      // CalcWeightLimit (rsp.go:183-213) + AvailableToPercentage (rsp.go:215-272), per segment
      const int64_t ac = v ? ac_l : 0, av = v ? av_l : 0;
      const double sum = seg_sum_f64(v ? (double)ac : 0.0);
      const double suma = seg_sum_f64((v && av > 0) ? (double)av : 0.0);
      int64_t wdyn;
      uint32_t tf = 0;
      // (segment-uniform branches: a segment's reductions read only its own lanes, so the two segments may
      // take different ones)
      if (suma == 0) {
        wdyn = v ? go_f2i(round(1000.0 / (double)(K > 0 ? K : 1))) : 0;
      } else {
        const int64_t lim = sum == 0 ? go_f2i(round(1000.0 / (double)(K > 0 ? K : 1)))
                                     : go_f2i(round((double)ac / sum * 1000.0 * 1.4));
        const double avd = av < 0 ? 0.0 : (double)av;
        int64_t wt = go_f2i(round(avd / suma * 1000.0));
        if (wt > lim) wt = lim;
        const int64_t sumtmp = seg_sum_i64(v ? wt : 0);
        wt = go_f2i(round((double)wt / (double)sumtmp * 1000.0));
        const int64_t other = seg_sum_i64(v ? wt : 0);
        const int64_t maxw = seg_max_i64(v ? wt : 0);
        wdyn = v ? wt : 0;
        const uint32_t tm = seg_ballot(v && wt == maxw);
        if (maxw > 0) {  // remainder → first strict maximum (lowest cluster id among ties)
          const int first = (int)__builtin_ctz(tm | 0x80000000u);
          if (__builtin_popcount(tm) > 1) tf = KAD_RF_REMAINDER_TIE;
          if (sl == first) wdyn = wadd(wdyn, wsub(1000, other));
        }
      }
      if (dyn) {
        e.w = wdyn;
        rflags |= tf;
      }
    }
    PlanOut po;
    rflags |= plan_row_pair(e, K, total, (f & KAD_W_AVOID_DISRUPTION) != 0, (f & KAD_W_KEEP_UNSCHED) != 0, po, kbuf);
    // result = plan + overflow, zeros dropped (rsp.go:162-179), ascending cluster id
    const int64_t res = v ? wadd(po.plan, (po.ofl & EF_HAS_OVER) ? po.over : 0) : 0;
    const bool nz = v && res != 0;
    const uint32_t m = seg_ballot(nz);
    if (nz) {
      const int64_t at = off + seg_mbcnt(m);
      o.cluster[at] = c;
      o.replicas[at] = res;
    }
    if (pok && sl == 0) {
      o.count[w] = __builtin_popcount(m);
      o.flags[w] = rflags;
    }
  }
}

}  // namespace kad
