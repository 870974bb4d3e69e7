// Device helpers shared by the schedule kernels (kad_k_full.h, kad_k_lean.h) and the filter diagnosis
// (kad_explain.hip): a unit's predicate program in VGPR lanes and ClusterAffinity's filter over the
// requirement bitmask rows.
#pragma once
#include "kad_device.h"
#include "kad_wave.h"

namespace kad {

// A unit's program (filter / score words) held in VGPR lanes: word i < 64 is
// read with v_readlane (no memory latency on the interpretation chain);
// longer programs fall back to scalar loads for the tail.
struct ProgRegs {
  const int32_t* p;
  int v;  // lane l holds p[l] (l < len)
  __device__ __forceinline__ int operator[](int i) const {
    return i < WAVE ? __builtin_amdgcn_readlane(v, i) : ldc(p + i);
  }
};
__device__ __forceinline__ ProgRegs load_prog(const int32_t* p, int len) {
  const int l = lane_id();
  return ProgRegs{p, l < len ? ldg(p, (uint32_t)l) : 0};
}

// ClusterAffinity.Filter (cluster_affinity.go:50-94) with
// clusterselector.MatchClusterSelectorTerms (clusterselector/util.go:97-132)
// over requirement bitmask rows, one lane per 64-cluster chunk: lane l
// returns the affinity word of chunk ch0 + l (every cluster evaluated
// independently, so the result ANDs with the other filters afterwards).
__device__ uint64_t affinity_filter_chunks(const uint64_t* rows, const ProgRegs& P, int nch, int ch0) {
  const int ch = ch0 + lane_id();
  const uint32_t chc = ch < nch ? (uint32_t)ch : 0u;
  auto row = [&](int id) { return ldg(rows, (uint32_t)id * (uint32_t)nch + chc); };
  auto and_rows = [&](uint64_t m, int at, int n) {
    int i = 0;
    for (; i + 4 <= n; i += 4) {  // four independent loads in flight
      const uint64_t r0 = row(P[at + i]), r1 = row(P[at + i + 1]), r2 = row(P[at + i + 2]), r3 = row(P[at + i + 3]);
      m &= r0 & r1 & r2 & r3;
    }
    for (; i < n; ++i) m &= row(P[at + i]);
    return m;
  };
  int pc = 0;
  const int n_sel = P[pc++];
  uint64_t m = and_rows(~0ull, pc, n_sel);  // SelectorFromSet
  pc += n_sel;
  if (!P[pc++]) return m;  // Required == nil: Success
  const int n_terms = P[pc++];
  uint64_t matched = 0, undecided = m;
  for (int t = 0; t < n_terms; t++) {
    if (!ballot(undecided != 0)) break;
    const int tf = P[pc], ne = P[pc + 1], nf = P[pc + 2];
    const int at = pc + 3;
    pc += 3 + ne + nf;
    if (!(tf & (KAD_TERM_HAS_EXPR | KAD_TERM_HAS_FIELD))) continue;  // nil/empty term selects nothing
    uint64_t cand = undecided;
    if (tf & KAD_TERM_HAS_EXPR) {
      if (!(tf & KAD_TERM_EXPR_VALID)) break;  // invalid selector reached: false for every undecided cluster
      cand = and_rows(cand, at, ne);
    }
    if (tf & KAD_TERM_HAS_FIELD) {
      if (!(tf & KAD_TERM_FIELD_VALID)) {  // reached only where the expressions matched
        undecided &= ~cand;
        continue;
      }
      cand = and_rows(cand, at + ne, nf);
    }
    matched |= cand;
    undecided &= ~cand;
  }
  return matched;
}

__device__ __forceinline__ uint64_t readlane64(uint64_t v, int l) {
  const uint32_t lo = __builtin_amdgcn_readlane((int)(uint32_t)v, l);
  const uint32_t hi = __builtin_amdgcn_readlane((int)(uint32_t)(v >> 32), l);
  return ((uint64_t)hi << 32) | lo;
}

}  // namespace kad
