// prep_kernel / prep_wave_kernel: unit records and static filter words, and the snapshot's slice kernels.
// Part of kad_kernels.hip's translation unit, which includes the kernels' headers in definition order.
#pragma once

#include "kad_device.h"
#include "kad_wave.h"

namespace kad {

// Words i .. i+CPL-1 of `base` as CPL/2 16-byte accesses. Only on the PREP_VEC route (kad_route.h): the host
// launches it where nch % PREP_CPL == 0 (no lane has a clamped tail, and every row offset is a multiple of
// CPL words) and every base is 16-byte aligned, so i is even and the address a multiple of 16.
template <int CPL>
__device__ __forceinline__ void ld_words(const uint64_t* base, uint32_t i, uint64_t (&r)[CPL]) {
  static_assert(CPL % 2 == 0, "16-byte accesses hold two words");
  ulonglong2 v[CPL / 2];
#pragma unroll
  for (int k = 0; k < CPL / 2; k++) v[k] = ldg(reinterpret_cast<const ulonglong2*>(base), (i >> 1) + (uint32_t)k);
#pragma unroll
  for (int k = 0; k < CPL / 2; k++) r[2 * k] = v[k].x, r[2 * k + 1] = v[k].y;
}
template <int CPL>
__device__ __forceinline__ void st_words(uint64_t* p, const uint64_t (&r)[CPL]) {
  static_assert(CPL % 2 == 0, "16-byte accesses hold two words");
#pragma unroll
  for (int k = 0; k < CPL / 2; k++) reinterpret_cast<ulonglong2*>(p)[k] = make_ulonglong2(r[2 * k], r[2 * k + 1]);
}

// One lane per (unit, PREP_CPL consecutive 64-cluster chunks), every launch,
// before the schedule kernel:
//  * the unit's first lanes write its 64-B UnitRec (16 B each), routing units that use a
//    feature the lean kernel leaves out (scalar resource requests, more than
//    64 taint ids or GVKs, debug capture) to schedule_kernel (REC_FULL);
//  * every lane writes the unit's static filter words for its chunks: the
//    ClusterAffinity filter (cluster_affinity.go:50-94,
//    MatchClusterSelectorTerms clusterselector/util.go:97-132) evaluated over
//    the requirement rows, ANDed with the PlacementFilter's ClusterNames
//    bitmap (placement/filter.go:37-57); and, for units with
//    CurrentClusters, the current-cluster word (TaintToleration's NoExecute
//    rule, taint_toleration.go:64-78).
// This takes the program → requirement-row load chain off every unit's
// critical path in the schedule kernel.
// p(i): word i of the unit's filter program (prep_kernel stages the first words in LDS). The CPL
// chunks ch0 .. ch0+CPL-1 are evaluated together (their row loads are independent); chunks past
// nch read chunk nch-1 and are never stored. VEC (prep_kernel<true>): no chunk is past nch and a row's CPL
// words are read as 16-byte loads (ld_words).
template <int CPL, class Prog, bool WAVE_ANY = false, bool VEC = false>
__device__ __forceinline__ void affinity_words(const uint64_t* rows, Prog p, uint32_t nch, uint32_t ch0,
                                               uint64_t (&out)[CPL], uint32_t cst = 1) {
  uint32_t cc[CPL];
#pragma unroll
  for (int k = 0; k < CPL; k++) cc[k] = ch0 + k * cst < nch ? ch0 + k * cst : nch - 1;
  auto and_row = [&](uint64_t (&v)[CPL], int id) {
    uint64_t r[CPL];
    if constexpr (VEC) {
      ld_words<CPL>(rows, (uint32_t)id * nch + ch0, r);
    } else {
#pragma unroll
      for (int k = 0; k < CPL; k++) r[k] = ldg(rows, (uint32_t)id * nch + cc[k]);
    }
#pragma unroll
    for (int k = 0; k < CPL; k++) v[k] &= r[k];
  };
  auto any = [](const uint64_t (&v)[CPL]) {
    uint64_t o = 0;
#pragma unroll
    for (int k = 0; k < CPL; k++) o |= v[k];
    if constexpr (WAVE_ANY) return ballot(o != 0) != 0;  // (one unit per wave: uniform control flow)
    return o != 0;
  };
  int pc = 0;
  const int n_sel = p(pc++);
  uint64_t m[CPL];  // SelectorFromSet: AND of the ClusterSelector entries
#pragma unroll
  for (int k = 0; k < CPL; k++) m[k] = ~0ull;
  for (int i = 0; i < n_sel; i++) and_row(m, p(pc + i));
  pc += n_sel;
#pragma unroll
  for (int k = 0; k < CPL; k++) out[k] = m[k];
  if (!p(pc++)) return;  // Required == nil: Success
  const int n_terms = p(pc++);
  uint64_t matched[CPL], undecided[CPL], cand[CPL];
#pragma unroll
  for (int k = 0; k < CPL; k++) matched[k] = 0, undecided[k] = m[k];
  for (int t = 0; t < n_terms && any(undecided); t++) {
    const int tf = p(pc), ne = p(pc + 1), nf = p(pc + 2);
    const int at = pc + 3;
    pc += 3 + ne + nf;
    if (!(tf & (KAD_TERM_HAS_EXPR | KAD_TERM_HAS_FIELD))) continue;  // nil/empty term selects nothing
#pragma unroll
    for (int k = 0; k < CPL; k++) cand[k] = undecided[k];
    if (tf & KAD_TERM_HAS_EXPR) {
      if (!(tf & KAD_TERM_EXPR_VALID)) break;  // invalid selector reached: false for every undecided cluster
      for (int i = 0; i < ne; i++) and_row(cand, p(at + i));
    }
    if (tf & KAD_TERM_HAS_FIELD) {
      if (!(tf & KAD_TERM_FIELD_VALID)) {  // reached only where the expressions matched
#pragma unroll
        for (int k = 0; k < CPL; k++) undecided[k] &= ~cand[k];
        continue;
      }
      for (int i = 0; i < nf; i++) and_row(cand, p(at + ne + i));
    }
#pragma unroll
    for (int k = 0; k < CPL; k++) matched[k] |= cand[k], undecided[k] &= ~cand[k];
  }
#pragma unroll
  for (int k = 0; k < CPL; k++) out[k] = matched[k];
}


// the words of chunks ch0 .. ch0+CPL-1 of the sorted cluster-id list ids[lo, hi): one lower bound of the
// first chunk's base, then the ids inside the CPL chunks four at a time (independent loads)
template <int CPL>
__device__ __forceinline__ void id_list_words(const int32_t* ids, int lo, int hi, uint32_t ch0, uint64_t (&out)[CPL]) {
#pragma unroll
  for (int k = 0; k < CPL; k++) out[k] = 0;
  const int base = (int)ch0 * WAVE, end = base + CPL * WAVE;
  int a = lo, b = hi;
  while (a < b) {  // lower bound of base
    const int mid = (a + b) >> 1;
    if (ids[mid] < base)
      a = mid + 1;
    else
      b = mid;
  }
  for (int j = a; j < hi; j += 4) {
    int v[4];
#pragma unroll
    for (int u = 0; u < 4; u++) v[u] = j + u < hi ? ids[j + u] : INT32_MAX;
    bool past = false;
#pragma unroll
    for (int u = 0; u < 4; u++) {
      const int d = v[u] - base;
      if (d >= 0 && d < CPL * WAVE) {
#pragma unroll
        for (int k = 0; k < CPL; k++)
          if ((d >> 6) == k) out[k] |= 1ull << (d & 63);
      }
      past |= v[u] >= end;
    }
    if (past) break;
  }
}

// the words of chunks ch0 + k*cst (k < CPL) of the sorted cluster-id list ids[lo, hi): per chunk one lower
// bound of its base, then the ids inside it four at a time (prep_wave_kernel's strided chunks)
template <int CPL>
__device__ __forceinline__ void id_list_words_strided(const int32_t* ids, int lo, int hi, uint32_t ch0, uint32_t cst,
                                                      uint64_t (&out)[CPL]) {
#pragma unroll
  for (int k = 0; k < CPL; k++) {
    out[k] = 0;
    const int base = (int)(ch0 + k * cst) * WAVE, end = base + WAVE;
    int a = lo, b = hi;
    while (a < b) {
      const int mid = (a + b) >> 1;
      if (ids[mid] < base)
        a = mid + 1;
      else
        b = mid;
    }
    for (int j = a; j < hi; j += 4) {
      int v[4];
#pragma unroll
      for (int u = 0; u < 4; u++) v[u] = j + u < hi ? ids[j + u] : INT32_MAX;
      bool past = false;
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int d = v[u] - base;
        if (d >= 0 && d < WAVE) out[k] |= 1ull << d;
        past |= v[u] >= end;
      }
      if (past) break;
    }
  }
}

// SnapDev::slices row r (r < 64*TW: NoSchedule|NoExecute taint id r; r < 128*TW: NoExecute taint id
// r - 64*TW; else GVK id r - 128*TW, any of the GW words), chunk ch: one wave per (row, ch), lane = cluster
__global__ __launch_bounds__(256) void slice_kernel(SnapDev s, uint64_t* out) {
  const int lane = lane_id();
  const int nch = (s.C + 63) >> 6;
  const int TW = s.TW;
  const long gw = (long)blockIdx.x * 4 + (threadIdx.x >> 6);
  if (gw >= (128L * TW + 64L * s.GW) * nch) return;
  const int ch = (int)(gw % nch), r = (int)(gw / nch);
  const int c = ch * WAVE + lane;
  const uint32_t cl = c < s.C ? (uint32_t)c : 0u;
  uint64_t word;
  int bit;
  if (r < 128 * TW) {
    const int t = r % (64 * TW);
    const uint32_t at = (uint32_t)(t >> 6) * (uint32_t)s.C + cl;
    word = r < 64 * TW ? ldg(s.nsne, at) : ldg(s.ne, at);
    bit = t & 63;
  } else {
    const int g = r - 128 * TW;
    word = ldg(s.gvk, (uint32_t)(g >> 6) * (uint32_t)s.C + cl);
    bit = g & 63;
  }
  const uint64_t m = ballot(c < s.C && ((word >> bit) & 1));
  if (lane == 0) out[(size_t)r * nch + ch] = m;
}

// SnapDev::taint_tab: lane per (tbl, g, sub, ch); OR over the set bits of sub of slice 8g + b of table tbl
__global__ __launch_bounds__(256) void taint_table_kernel(SnapDev s, uint64_t* tab) {
  const uint32_t nch = (uint32_t)((s.C + 63) >> 6);
  const uint32_t ng = 8u * (uint32_t)s.TW;  // 8-id groups per table
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g >= 2u * ng * 256 * nch) return;
  const uint32_t ch = g % nch, e = g / nch, sub = e & 255u, grp = (e >> 8) % ng, tbl = (e >> 8) / ng;
  uint64_t m = 0;
  for (uint32_t r = sub; r; r &= r - 1) m |= s.slices[((size_t)tbl * 8 * ng + grp * 8 + __builtin_ctz(r)) * nch + ch];
  tab[g] = m;
}

// TaintToleration.Filter (taint_toleration.go:44-89) and APIResources.Filter (apiresources.go:25-43) of
// unit w on chunks cc[0..CPL) (TW <= TFOLD_MAX_TW): clusters with a NoSchedule|NoExecute taint the unit
// does not tolerate are out — only NoExecute ones on its CurrentClusters (cw) — and clusters without its
// GVK. The untolerated present taints are looked up 8 ids at a time in SnapDev::taint_tab, each lookup
// serving the lane's CPL chunks (independent loads). VEC: cc[k] = cc[0] + k, read as 16-byte loads.
template <int CPL, bool VEC = false>
__device__ __forceinline__ void folded_words(const SnapDev& s, uint32_t fm, uint32_t f, int gvk, const uint64_t* tol,
                                             const uint64_t (&cw)[CPL], uint32_t nch, const uint32_t (&cc)[CPL],
                                             uint64_t (&out)[CPL]) {
#pragma unroll
  for (int k = 0; k < CPL; k++) out[k] = ~0ull;
  if (fm & (1u << KAD_PL_TAINT_TOLERATION)) {
    const bool cur = f & KAD_W_HAS_CURRENT;
    const int TW = s.TW;
    const size_t ng = (size_t)8 * TW;
    uint64_t bad_ns[CPL], bad_ne[CPL];
#pragma unroll
    for (int k = 0; k < CPL; k++) bad_ns[k] = bad_ne[k] = 0;
    for (int tw = 0; tw < TW; tw++) {
      const uint64_t u = s.present_taints[tw] & ~tol[tw];
#pragma unroll
      for (int gi = 0; gi < 8; gi++) {
        const uint32_t sub = (uint32_t)(u >> (8 * gi)) & 255u;
        if (sub) {
          const uint64_t* rn = s.taint_tab + ((size_t)(8 * tw + gi) * 256 + sub) * nch;
          uint64_t x[CPL];
          if constexpr (VEC) {
            ld_words<CPL>(rn, cc[0], x);
          } else {
#pragma unroll
            for (int k = 0; k < CPL; k++) x[k] = rn[cc[k]];
          }
#pragma unroll
          for (int k = 0; k < CPL; k++) bad_ns[k] |= x[k];
          if (cur) {
            const uint64_t* re = s.taint_tab + ((ng + 8 * tw + gi) * 256 + sub) * nch;
            if constexpr (VEC) {
              ld_words<CPL>(re, cc[0], x);
            } else {
#pragma unroll
              for (int k = 0; k < CPL; k++) x[k] = re[cc[k]];
            }
#pragma unroll
            for (int k = 0; k < CPL; k++) bad_ne[k] |= x[k];
          }
        }
      }
    }
#pragma unroll
    for (int k = 0; k < CPL; k++) out[k] = cur ? ((cw[k] & ~bad_ne[k]) | (~cw[k] & ~bad_ns[k])) : ~bad_ns[k];
  }
  if (fm & (1u << KAD_PL_API_RESOURCES)) {  // any GVK id of the snapshot's GW words (-1: no cluster has it)
    const bool has = gvk >= 0 && gvk < 64 * s.GW;
    const uint64_t* rg = s.slices + ((size_t)128 * s.TW + (has ? gvk : 0)) * nch;
    if constexpr (VEC) {
      uint64_t x[CPL];
      ld_words<CPL>(rg, cc[0], x);
#pragma unroll
      for (int k = 0; k < CPL; k++) out[k] &= has ? x[k] : 0ull;
    } else {
#pragma unroll
      for (int k = 0; k < CPL; k++) out[k] &= has ? rg[cc[k]] : 0ull;
    }
  }
}

// #(fit_vals[r] < x) for r = 0, 1 (x0, x1): 8 levels over the LDS fences (SnapDev::fit_fences: fence i =
// value (i+1)*S - 1, S = fit_mp / FIT_FENCES), then log2(S) levels in global memory; both searches interleaved
__device__ __forceinline__ int2 fit_ranks(const SnapDev& s, const int64_t (*fences)[FIT_FENCES], int64_t x0, int64_t x1) {
  int f0 = 0, f1 = 0;
#pragma unroll
  for (int st = FIT_FENCES / 2; st >= 1; st >>= 1) {
    f0 = fences[0][f0 + st - 1] < x0 ? f0 + st : f0;
    f1 = fences[1][f1 + st - 1] < x1 ? f1 + st : f1;
  }
  const int S = s.fit_mp / FIT_FENCES;
  int b0 = f0 * S, b1 = f1 * S;  // the answer lies in [b, b + S - 1]: value b + S - 1 >= x
  for (int st = S >> 1; st >= 1; st >>= 1) {
    const int64_t v0 = ldg(s.fit_vals[0], (uint32_t)(b0 + st - 1)), v1 = ldg(s.fit_vals[1], (uint32_t)(b1 + st - 1));
    b0 = v0 < x0 ? b0 + st : b0;
    b1 = v1 < x1 ? b1 + st : b1;
  }
  return make_int2(b0, b1);
}

#ifndef KAD_PREP_MINW
#define KAD_PREP_MINW 1
#endif
// VEC (route PREP_VEC, decided per launch on the host: nch % PREP_CPL == 0 and req_mask, fit_rows, taint_tab,
// slices, sw and cw all 16-byte aligned): every lane owns CPL whole chunks, and the CPL words of each row it
// reads or stores are moved as 16-byte accesses — the same bytes in half the vector memory instructions.
template <bool VEC>
__global__ __launch_bounds__(256, VEC ? 5 : KAD_PREP_MINW) void prep_kernel(SnapDev s, BatchDev b, ProfDev p, int force_full) {
  constexpr int CPL = PREP_CPL;
  __shared__ int32_t prog_words[256 * CPL];  // words CPL*l .. CPL*l+CPL-1 of its unit's filter program, per lane
  const uint32_t nch = (uint32_t)((s.C + 63) >> 6);
  const uint32_t per = nch > 0 ? (nch + CPL - 1) / CPL : 1u;  // lanes per unit
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g == 0) {
    *b.defer_n = 0;
    *b.work_n = 0;
    if (!b.early_rows) {  // early_rows: this kernel appends to rows (the host zeroes both before it runs)
      *b.rows_n = 0;
      *b.rows_head = 0;
    }
  }
  if (g < (uint32_t)WQ_HEADS) b.wq[g * WQ_STRIDE] = 0u;  // the schedule kernels' work heads
  // one block per 256 lanes (a persistent grid striding over the batch measured equal at C3, 188 vs 187 us,
  // and its loop cost C4's 2-lane units 17 us: profiles/r06/ab_c3_prep_persistent.txt)
  const bool live = g < (uint32_t)b.W * per;
  const uint32_t w = live ? g / per : 0u, l = g - w * per, ch0 = l * CPL;
  if (b.W <= 0) return;  // (the one block of an empty batch: the resets above are all it does)
  // every per-unit load is issued up front by every lane (the lanes of a unit share its cache lines), and
  // before the barrier (none of them reads LDS): the batch columns and the program offsets are one round of
  // loads in flight together with the fences, the program words and the toleration words (which wait for
  // fprog_off and tolset) a second, and the record's chain and the affinity chain below overlap instead of
  // running one after the other. The loads are unconditional (a select per load would become a branch and
  // a wait per load): the last block's dead lanes read unit 0's columns.
  const int32_t fpo = b.fprog_off[w], fpo1 = b.fprog_off[w + 1];
  const int32_t plen = live ? fpo1 - fpo : 0;
  // SnapDev::fitfold: every S-th fit value per resource, from the snapshot's fence table (built at upload /
  // update): one coalesced 16-B load per lane, 4 KB per block
  __shared__ __attribute__((aligned(16))) int64_t fences[2][FIT_FENCES];
  static_assert(2 * FIT_FENCES % 512 == 0, "the fence copy moves 2 values per lane of a 256-lane block");
  longlong2 fv[FIT_FENCES / 256];
  if (s.fitfold) {
#pragma unroll
    for (int i = 0; i < FIT_FENCES / 256; i++) fv[i] = reinterpret_cast<const longlong2*>(s.fit_fences)[i * 256 + threadIdx.x];
  }
  const uint32_t f = b.flags[w];
  const uint32_t fm = p.filter_mask;
  const int32_t gvk = b.gvk[w], tolset = b.tolset[w], sprog = b.sprog_off[w];
  const int64_t rqc = b.req_cpu[w], rqm = b.req_mem[w], maxc = b.maxc[w], desired = b.desired[w];
  const int64_t oo = b.out_off[w];
  const int32_t so0 = b.sreq_off[w], so1 = b.sreq_off[w + 1];
  // the unit's lanes load its program words 0 .. CPL*per-1 with coalesced loads into LDS: the interpreter's
  // word → row chain then runs on LDS reads, not on dependent global loads (words past the program read
  // the unit's word 0 and are stored as 0)
  int32_t pwv[CPL];
#pragma unroll
  for (int k = 0; k < CPL; k++) {
    const int i = (int)ch0 + k;
    const int32_t v = b.fprog[fpo + (i < plen ? i : 0)];
    pwv[k] = i < plen ? v : 0;
  }
  const uint64_t tol0 = b.tol_all[(size_t)tolset * b.TW], tolp0 = b.tol_pns[(size_t)tolset * b.TW];
  if (s.fitfold) {
#pragma unroll
    for (int i = 0; i < FIT_FENCES / 256; i++) reinterpret_cast<longlong2*>(&fences[0][0])[i * 256 + threadIdx.x] = fv[i];
  }
#pragma unroll
  for (int k = 0; k < CPL; k++) prog_words[threadIdx.x * CPL + k] = pwv[k];
  __syncthreads();
  if (!live) return;
  bool full = force_full != 0;
  // the unfolded schedule kernels cache GVK word 0 only; folded snapshots take every GVK id from the slices
  if ((fm & (1u << KAD_PL_API_RESOURCES)) && gvk >= 64 && !s.fold) full = true;
  if ((fm & (1u << KAD_PL_CLUSTER_RESOURCES_FIT)) && (f & KAD_W_FIT_NONZERO) && so0 < so1) full = true;
  const uint32_t rflags = f | (((f & KAD_W_HAS_DESIRED) && desired > 0) ? REC_DESIRED_POS : 0u) | (full ? REC_FULL : 0u);
  const bool act = ch0 < nch && !(f & KAD_W_STICKY);
  int cnt = 0;  // feasible clusters among this lane's chunks (early_rows)
  if (act) {
    uint64_t m[CPL];
#pragma unroll
    for (int k = 0; k < CPL; k++) m[k] = ~0ull;
    if (fm & (1u << KAD_PL_CLUSTER_AFFINITY)) {
      const int32_t* gp = b.fprog + fpo;
      const int base = ((int)threadIdx.x - (int)l) * CPL;  // the unit's program word 0 in this block (may be < 0)
      auto word = [&](int i) -> int32_t {
        const int t = base + i;
        return (i < (int)(per * CPL) && t >= 0 && t < 256 * CPL) ? prog_words[t] : gp[i];
      };
      affinity_words<CPL, decltype(word), false, VEC>(b.req_mask, word, nch, ch0, m);
    }
    if (s.fitfold && (fm & (1u << KAD_PL_CLUSTER_RESOURCES_FIT)) && (f & KAD_W_FIT_NONZERO)) {
      // fit.go:73-134 (cpu, memory) by threshold rows: clusters whose available amount >= the request
      const int2 j = fit_ranks(s, fences, rqc, rqm);
      const int jc = j.x, jm = j.y;
      if constexpr (VEC) {
        uint64_t rc[CPL], rm[CPL];
        ld_words<CPL>(s.fit_rows[0], (uint32_t)jc * nch + ch0, rc);
        ld_words<CPL>(s.fit_rows[1], (uint32_t)jm * nch + ch0, rm);
#pragma unroll
        for (int k = 0; k < CPL; k++) m[k] &= rc[k] & rm[k];
      } else {
#pragma unroll
        for (int k = 0; k < CPL; k++) {
          const uint32_t ch = ch0 + k < nch ? ch0 + k : nch - 1;
          m[k] &= ldg(s.fit_rows[0], (uint32_t)jc * nch + ch) & ldg(s.fit_rows[1], (uint32_t)jm * nch + ch);
        }
      }
    }
    const bool place = (fm & (1u << KAD_PL_PLACEMENT_FILTER)) && (f & KAD_W_HAS_PLACEMENT);
    const bool curw = (fm & (1u << KAD_PL_TAINT_TOLERATION)) && (f & KAD_W_HAS_CURRENT);
    uint64_t pw[CPL], cwv[CPL];
    if (place) {
      id_list_words<CPL>(b.place, b.place_off[w], b.place_off[w + 1], ch0, pw);
#pragma unroll
      for (int k = 0; k < CPL; k++) m[k] &= pw[k];
    }
#pragma unroll
    for (int k = 0; k < CPL; k++) cwv[k] = 0;
    if (curw) id_list_words<CPL>(b.cur_id, b.cur_off[w], b.cur_off[w + 1], ch0, cwv);
    if (s.fold) {
      uint32_t cc[CPL];
#pragma unroll
      for (int k = 0; k < CPL; k++) cc[k] = ch0 + k < nch ? ch0 + k : nch - 1;
      uint64_t tw[TFOLD_MAX_TW];
      tw[0] = tol0;
      for (int t = 1; t < s.TW && t < TFOLD_MAX_TW; t++) tw[t] = b.tol_all[(size_t)tolset * b.TW + t];
      uint64_t fw[CPL];
      folded_words<CPL, VEC>(s, fm, f, gvk, tw, cwv, nch, cc, fw);
#pragma unroll
      for (int k = 0; k < CPL; k++) m[k] &= fw[k];
    }
    if constexpr (VEC) {  // chunks ch0 .. ch0+CPL-1 all exist
      if (ch0 + CPL == nch && (s.C & 63)) m[CPL - 1] &= (1ull << (s.C & 63)) - 1;  // clusters past C: never feasible
      if (curw) st_words<CPL>(b.cw + (size_t)w * nch + ch0, cwv);
      st_words<CPL>(b.sw + (size_t)w * nch + ch0, m);
#pragma unroll
      for (int k = 0; k < CPL; k++) cnt += popc64(m[k]);
    } else {
#pragma unroll
      for (int k = 0; k < CPL; k++) {
        const uint32_t ch = ch0 + k;
        if (ch >= nch) break;
        if (curw) b.cw[(size_t)w * nch + ch] = cwv[k];
        if (ch == nch - 1 && (s.C & 63)) m[k] &= (1ull << (s.C & 63)) - 1;  // clusters past C: never feasible
        b.sw[(size_t)w * nch + ch] = m[k];
        cnt += popc64(m[k]);
      }
    }
  }
  // early_rows: in the wide kernel's FITF mode (fold + fitfold) the static words are the whole filter, so
  // the unit's feasible count is their popcount (summed over its `per` lanes: a power of two, one wave);
  // a unit the wide kernel would hand to rows (past its sticky / defer checks, more than WIDE_P clusters)
  // is routed here, before the wide kernel starts
  bool route = false;
  if (b.early_rows) {
    for (uint32_t o = 1; o < per; o <<= 1) cnt += __shfl_xor(cnt, (int)o);
    route = act && !(rflags & REC_FULL) && !(f & KAD_W_WIDE_SCORES) && (uint64_t)rqc < (1ull << 46) &&
            (uint64_t)rqm < (1ull << 46) && cnt > WIDE_P;
  }
  // the record is stored by the unit's lanes, 16-B piece q by lane q (every lane holds every column, and
  // route is the same in all of them): with 4 or more lanes per unit a wave's store writes one contiguous
  // 1 KB (C3: 16 units), where the first lane alone took four stores of 16 lanes at a 64-B stride. 3 lanes:
  // the third stores two pieces; 2 lanes: two each; 1 lane: the whole record, as before.
  const auto u64x2 = [](uint64_t a, uint64_t c) { return make_uint4((uint32_t)a, (uint32_t)(a >> 32), (uint32_t)c, (uint32_t)(c >> 32)); };
  const uint4 p0 = make_uint4(rflags | (route ? REC_ROW : 0u), (uint32_t)gvk, (uint32_t)tolset, (uint32_t)sprog);
  const uint4 p1 = u64x2((uint64_t)rqc, (uint64_t)rqm), p2 = u64x2((uint64_t)maxc, (uint64_t)oo), p3 = u64x2(tol0, tolp0);
  const auto sel = [](bool c, const uint4& a, const uint4& o) { return make_uint4(c ? a.x : o.x, c ? a.y : o.y, c ? a.z : o.z, c ? a.w : o.w); };
  const auto pick = [&](uint32_t q) { return sel(q < 2, sel(q == 0, p0, p1), sel(q == 2, p2, p3)); };
  uint4* rp = reinterpret_cast<uint4*>(b.rec + w);
  if (per >= 3) {
    if (l < 4) rp[l] = pick(l);
    if (per == 3 && l == 2) rp[3] = p3;
  } else if (per == 2) {
    rp[2 * l] = sel(l == 0, p0, p2);
    rp[2 * l + 1] = sel(l == 0, p1, p3);
  } else {
    rp[0] = p0, rp[1] = p1, rp[2] = p2, rp[3] = p3;
  }
  if (l == 0 && route) b.rows[atomicAdd(b.rows_n, 1)] = (int32_t)w;
}

// prep_wave_kernel<CW> — prep_kernel for wide snapshots (64 < ceil(C/64) <= 64*CW chunks, C5's 10 000
// clusters): one unit per wave, lane l owning chunks l, l+64, ... (CW of them). prep_kernel's lanes pack
// CPL consecutive chunks and ceil(nch/CPL) lanes per unit, so a wave holds parts of two or three units whose
// filter programs diverge (every loop runs the longest unit's trips under exec masks) and a load
// instruction reads every CPL-th word of a row; here the unit's program, tolerations and taint groups are
// wave-uniform (scalar branches; the program words are v_readlane reads of one window load) and every row
// load reads 64 consecutive words. Same outputs as prep_kernel.
template <int CW>
__global__ __launch_bounds__(256) void prep_wave_kernel(SnapDev s, BatchDev b, ProfDev p, int force_full) {
  const uint32_t nch = (uint32_t)((s.C + 63) >> 6);
  const int lane = lane_id();
  const uint32_t g = blockIdx.x * 256u + threadIdx.x;
  if (g == 0) {
    *b.defer_n = 0;
    *b.work_n = 0;
    if (!b.early_rows) {
      *b.rows_n = 0;
      *b.rows_head = 0;
    }
  }
  if (g < (uint32_t)WQ_HEADS) b.wq[g * WQ_STRIDE] = 0u;
  __shared__ __attribute__((aligned(16))) int64_t fences[2][FIT_FENCES];  // the snapshot's fence table, 16 B per lane
  if (s.fitfold) {
    const longlong2* src = reinterpret_cast<const longlong2*>(s.fit_fences);
    longlong2* dst = reinterpret_cast<longlong2*>(&fences[0][0]);
    for (int i = threadIdx.x; i < FIT_FENCES; i += 256) dst[i] = src[i];
  }
  __syncthreads();
  // one unit per wave, grid = units / 4 (a unit loop here, even at one trip per wave, took C5's prep
  // 540 -> 588 us: profiles/r06/bisect_c5_prep.txt)
  const int w = __builtin_amdgcn_readfirstlane((int)(g >> 6));
  if (w >= b.W) return;
  const uint32_t f = (uint32_t)ldc(b.flags + w);
  const uint32_t fm = p.filter_mask;
  const int32_t gvk = ldc(b.gvk + w), tolset = ldc(b.tolset + w), sprog = ldc(b.sprog_off + w);
  const int64_t rqc = ldc(b.req_cpu + w), rqm = ldc(b.req_mem + w), maxc = ldc(b.maxc + w), desired = ldc(b.desired + w);
  const int64_t oo = ldc(b.out_off + w);
  const int32_t so0 = ldc(b.sreq_off + w), so1 = ldc(b.sreq_off + w + 1);
  const int32_t fpo = ldc(b.fprog_off + w), plen = ldc(b.fprog_off + w + 1) - fpo;
  const uint64_t tol0 = ldc(b.tol_all + (size_t)tolset * b.TW), tolp0 = ldc(b.tol_pns + (size_t)tolset * b.TW);
  bool full = force_full != 0;
  if ((fm & (1u << KAD_PL_API_RESOURCES)) && gvk >= 64 && !s.fold) full = true;
  if ((fm & (1u << KAD_PL_CLUSTER_RESOURCES_FIT)) && (f & KAD_W_FIT_NONZERO) && so0 < so1) full = true;
  const uint32_t rflags = f | (((f & KAD_W_HAS_DESIRED) && desired > 0) ? REC_DESIRED_POS : 0u) | (full ? REC_FULL : 0u);
  const bool act = !(f & KAD_W_STICKY);
  int cnt = 0;
  if (act) {
    uint32_t cc[CW];
#pragma unroll
    for (int k = 0; k < CW; k++) cc[k] = (uint32_t)(lane + 64 * k) < nch ? (uint32_t)(lane + 64 * k) : nch - 1;
    uint64_t m[CW];
#pragma unroll
    for (int k = 0; k < CW; k++) m[k] = ~0ull;
    if (fm & (1u << KAD_PL_CLUSTER_AFFINITY)) {
      // program words 0..63 in the lanes (one load; the batch buffer's slack covers a window past the blob)
      const int32_t* gp = b.fprog + fpo;
      const int32_t pv = ldg(gp, (uint32_t)lane);
      auto word = [&](int i) -> int32_t { return i < WAVE ? __builtin_amdgcn_readlane(pv, i) : ldc(gp + i); };
      affinity_words<CW, decltype(word), true>(b.req_mask, word, nch, (uint32_t)lane, m, 64u);
    }
    if (s.fitfold && (fm & (1u << KAD_PL_CLUSTER_RESOURCES_FIT)) && (f & KAD_W_FIT_NONZERO)) {
      const int2 j = fit_ranks(s, fences, rqc, rqm);
      const int jc = __builtin_amdgcn_readfirstlane(j.x), jm = __builtin_amdgcn_readfirstlane(j.y);
#pragma unroll
      for (int k = 0; k < CW; k++)
        m[k] &= ldg(s.fit_rows[0], (uint32_t)jc * nch + cc[k]) & ldg(s.fit_rows[1], (uint32_t)jm * nch + cc[k]);
    }
    const bool place = (fm & (1u << KAD_PL_PLACEMENT_FILTER)) && (f & KAD_W_HAS_PLACEMENT);
    const bool curw = (fm & (1u << KAD_PL_TAINT_TOLERATION)) && (f & KAD_W_HAS_CURRENT);
    uint64_t cwv[CW];
#pragma unroll
    for (int k = 0; k < CW; k++) cwv[k] = 0;
    if (place) {
      uint64_t pw[CW];
      id_list_words_strided<CW>(b.place, ldc(b.place_off + w), ldc(b.place_off + w + 1), (uint32_t)lane, 64u, pw);
#pragma unroll
      for (int k = 0; k < CW; k++) m[k] &= pw[k];
    }
    if (curw) id_list_words_strided<CW>(b.cur_id, ldc(b.cur_off + w), ldc(b.cur_off + w + 1), (uint32_t)lane, 64u, cwv);
    if (s.fold) {
      uint64_t tw[TFOLD_MAX_TW];
      tw[0] = tol0;
      for (int t = 1; t < s.TW && t < TFOLD_MAX_TW; t++) tw[t] = ldc(b.tol_all + (size_t)tolset * b.TW + t);
      uint64_t fw[CW];
      folded_words<CW>(s, fm, f, gvk, tw, cwv, nch, cc, fw);
#pragma unroll
      for (int k = 0; k < CW; k++) m[k] &= fw[k];
    }
#pragma unroll
    for (int k = 0; k < CW; k++) {
      const uint32_t ch = (uint32_t)(lane + 64 * k);
      if (ch >= nch) break;
      if (curw) b.cw[(size_t)w * nch + ch] = cwv[k];
      if (ch == nch - 1 && (s.C & 63)) m[k] &= (1ull << (s.C & 63)) - 1;
      b.sw[(size_t)w * nch + ch] = m[k];
      cnt += popc64(m[k]);
    }
  }
  bool route = false;
  if (b.early_rows) {
    cnt = wave_sum_i32(cnt);
    route = act && !(rflags & REC_FULL) && !(f & KAD_W_WIDE_SCORES) && (uint64_t)rqc < (1ull << 46) &&
            (uint64_t)rqm < (1ull << 46) && cnt > WIDE_P;
  }
  if (lane == 0) {
    UnitRec r;
    r.flags = rflags | (route ? REC_ROW : 0u);
    r.gvk = gvk;
    r.tolset = tolset;
    r.sprog_off = sprog;
    r.req_cpu = rqc;
    r.req_mem = rqm;
    r.maxc = maxc;
    r.out_off = oo;
    r.tol0 = tol0;
    r.tolp0 = tolp0;
    b.rec[w] = r;
    if (route) b.rows[atomicAdd(b.rows_n, 1)] = (int32_t)w;
  }
}

}  // namespace kad
