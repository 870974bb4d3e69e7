// Score arithmetic shared by the schedule kernels: affinity scores, resource quotients, BalancedAllocation.
// Part of kad_kernels.hip's translation unit, which includes the kernels' headers in definition order.
#pragma once

#include "kad_wave.h"

namespace kad {

// ClusterAffinity.Score raw (cluster_affinity.go:96-135) for cluster c (per lane).
__device__ int64_t affinity_score(const uint64_t* rows, const int32_t* p, int nch, int c) {
  int pc = 0;
  const int n_terms = ldc(p + pc++);
  int64_t score = 0;
  const int ch = c >> 6, bit = c & 63;
  for (int t = 0; t < n_terms; t++) {
    const int32_t wgt = ldc(p + pc), ne = ldc(p + pc + 1);
    const int32_t* ids = p + pc + 2;
    pc += 2 + ne;
    bool m = true;
    for (int i = 0; i < ne; i++) m = m && ((ldg(rows, (uint32_t)ldc(ids + i) * (uint32_t)nch + ch) >> bit) & 1);
    if (m) score = wadd(score, wgt);
  }
  return score;
}

// The same score with the unit's program words 0..63 in the lanes of `pv` (one vector load of the window at
// the program's offset; the batch buffer has 256 B of slack past the blob, BatchDev): the program is parsed
// with v_readlane, and each term's expression rows load together, four at a time (the AND of a term's rows
// at c is the AND of their bits) — one memory round trip per term instead of a scalar load chain through
// the program plus one load per expression. Words past 63 are read from memory (sp = the program).
__device__ __forceinline__ int64_t affinity_score_pv(const uint64_t* rows, uint32_t pv, const int32_t* sp, int nch,
                                                     int c) {
  auto pw = [&](int i) -> int { return i < WAVE ? __builtin_amdgcn_readlane((int)pv, i) : ldc(sp + i); };
  const int n_terms = pw(0);
  int pc = 1;
  int64_t score = 0;
  const uint32_t ch = (uint32_t)(c >> 6);
  const int bit = c & 63;
  for (int t = 0; t < n_terms; t++) {
    const int32_t wgt = pw(pc), ne = pw(pc + 1);
    const int at = pc + 2;
    pc += 2 + ne;
    uint64_t all = ~0ull;
    for (int i0 = 0; i0 < ne; i0 += 4) {
      uint64_t r[4];
#pragma unroll
      for (int u = 0; u < 4; u++) {
        const int i = i0 + u < ne ? i0 + u : ne - 1;  // (repeats past ne: AND is idempotent)
        r[u] = ldg(rows, (uint32_t)pw(at + i) * (uint32_t)nch + ch);
      }
      all &= r[0] & r[1] & r[2] & r[3];
    }
    if ((all >> bit) & 1) score = wadd(score, wgt);
  }
  return score;
}

// least_allocated.go:88-94 / most_allocated.go:90-97:
//   capacity == 0 || requested > capacity ? 0 : (x * 100) / capacity
// with x = capacity - requested (least) or requested (most). Fast path for
// 0 <= requested <= capacity < 2^46 (every real cluster): x*100 < 2^53 and the
// quotient is in [0, 100], so an f64 reciprocal estimate corrected twice with
// exact f64 products gives the exact integer quotient; anything else takes the
// Go-wrapping int64 path.
__device__ __forceinline__ int64_t alloc_score(int64_t req, int64_t cap, bool most) {
  if (cap == 0 || req > cap) return 0;
  if (cap > 0 && req >= 0 && cap < (1ll << 46)) {
    const double cd = (double)cap;
    const double ad = (double)(most ? req : cap - req) * 100.0;  // exact
    int q = (int)(ad * __builtin_amdgcn_rcp(cd));
    double r = ad - (double)q * cd;  // exact: q * cd < 2^53
    q += (r >= cd) - (r < 0.0);
    r = ad - (double)q * cd;
    q += (r >= cd) - (r < 0.0);
    return q;
  }
  const int64_t num = wmul(most ? req : wsub(cap, req), 100);
  return go_div(num, cap);
}
// floor(100 x / cap) for integer-valued 0 <= x <= cap, 1 <= cap < 2^46 (the
// lean kernel's clean-snapshot path): the f32 estimate x * (100/cap) is within
// 1e-4 of the quotient (<= 100), so one exact f64 correction (100x and q*cap
// are integers < 2^53) gives the exact Go integer quotient
__device__ __forceinline__ int quot100(double x, double cap, float inv100) {
  int q = (int)((float)x * inv100);
  const double r = __builtin_fma(-(double)q, cap, x * 100.0);
  q += (int)(r >= cap) - (int)(r < 0.0);
  return q;
}
__device__ __forceinline__ int64_t least_requested(int64_t req, int64_t cap) { return alloc_score(req, cap, false); }
__device__ __forceinline__ int64_t most_requested(int64_t req, int64_t cap) { return alloc_score(req, cap, true); }
// balanced_allocation.go:45-88 — IEEE float64, no contraction (-ffp-contract=off)
__device__ __forceinline__ int64_t balanced_d(double cf, double mf) {
  if (cf >= 1 || mf >= 1) return 0;
  const double diff = fabs(cf - mf);
  const double one_minus = 1 - diff;
  return go_f2i(one_minus * 100.0);
}
__device__ __forceinline__ int64_t balanced(int64_t rc, int64_t cc, int64_t rm, int64_t cm) {
  const double cf = cc == 0 ? 1.0 : (double)rc / (double)cc;
  const double mf = cm == 0 ? 1.0 : (double)rm / (double)cm;
  if (cf >= 1 || mf >= 1) return 0;
  const double diff = fabs(cf - mf);
  const double one_minus = 1 - diff;
  return go_f2i(one_minus * 100.0);
}

constexpr uint32_t BIT(int pl) { return 1u << pl; }
// q = num / den for Go int64 when 0 <= num < 2^24, den > 0 (f32 path), else go_div
__device__ __forceinline__ int64_t div_fast(int64_t num, int64_t den) {
  if (num >= 0 && num < (1 << 24) && den > 0) return small_quot(num, den);
  return go_div(num, den);
}

}  // namespace kad
