// Override policies (kad_override_match): which override rules match which placed cluster, per object.
//
// The reference asks isClusterMatched (pkg/controllers/override/util.go:154-221) once per (object, placed
// cluster, rule) from parseOverrides (util.go:99-140). A rule's answer depends on the cluster alone, so it is
// computed once per (rule, cluster) into two bitmask rows over the policy set's requirement rows —
// M (matches) and E (isClusterMatched returns an error) — and a batch of objects then only gathers bits:
//
//   override_rule_rows_kernel   one lane per (rule, 64-cluster chunk): the names word, the selector's AND,
//                               the term-by-term walk of MatchClusterSelectorTerms
//                               (util/clusterselector/util.go:97-132) with its error cases kept apart
//   override_status_kernel      one lane per object: does any rule of its first, then of its second policy
//                               have an E bit at a placed cluster (parseOverrides returns on the first error)
//   override_match_kernel       one lane per placed slot: the M bit of every rule of the object's one or two
//                               policies at the slot's cluster, packed into the slot's RW output words
//
// Nothing here writes state that kad_schedule reads.
#include "kad_device.h"
#include "kad_wave.h"

namespace kad {

// M and E of rule r on chunk ch. Lanes of one rule are consecutive chunks, so the requirement-row loads
// are coalesced and the rule's program words (any length: plain loads at pc, no register window) are one
// address per wave, served as a broadcast.
__global__ __launch_bounds__(256) void override_rule_rows_kernel(OverrideDev o) {
  const int nch = (o.C + 63) >> 6;
  const long g = (long)blockIdx.x * 256 + threadIdx.x;
  if (g >= (long)o.R * nch) return;
  const int r = (int)(g / nch), ch = (int)(g - (long)r * nch);
  // clusters past C: never
  const uint64_t all = (ch == nch - 1 && (o.C & 63)) ? (1ull << (o.C & 63)) - 1 : ~0ull;
  const uint32_t f = o.rule_flags[r];
  uint64_t m = 0, e = 0;
  if (!(f & KAD_OVR_HAS_TARGET)) {
    m = all;  // util.go:156-158
  } else {
    // isClusterMatchedByClusterNames (util.go:180-194): the sorted id list's entries inside this chunk
    uint64_t names = all;
    if (f & KAD_OVR_HAS_NAMES) {
      names = 0;
      const int end = o.name_off[r + 1], c0 = ch * WAVE;
      int lo = o.name_off[r], hi = end;
      while (lo < hi) {
        const int mid = lo + ((hi - lo) >> 1);
        if (o.name[mid] < c0)
          lo = mid + 1;
        else
          hi = mid;
      }
      for (int j = lo; j < end; ++j) {
        const int c = o.name[j];
        if (c >= c0 + WAVE) break;
        names |= 1ull << (c - c0);
      }
    }
    if (f & KAD_OVR_SEL_INVALID) {
      e = names;  // util.go:202-207: reached by every cluster that passed the names
    } else {
      const int32_t* P = o.prog + o.prog_off[r];
      const uint64_t* rows = o.req_mask + ch;
      auto row = [&](int id) { return rows[(size_t)id * nch]; };
      int pc = 0;
      const int n_sel = P[pc++];
      uint64_t live = names;
      for (int i = 0; i < n_sel; ++i) live &= row(P[pc++]);
      if (!P[pc++]) {
        m = live;  // util.go:216-218: no ClusterAffinity
      } else {
        // `live`: clusters still walking the terms
        const int n_terms = P[pc++];
        for (int t = 0; t < n_terms && live; ++t) {
          const int tf = P[pc], ne = P[pc + 1], nf = P[pc + 2];
          const int at = pc + 3;
          pc += 3 + ne + nf;
          if (!(tf & (KAD_TERM_HAS_EXPR | KAD_TERM_HAS_FIELD))) continue;  // clusterselector/util.go:103-106
          uint64_t x = live;
          if (tf & KAD_TERM_HAS_EXPR) {
            if (!(tf & KAD_TERM_EXPR_VALID)) {  // :109-112: every cluster that reaches the term
              e |= live;
              break;
            }
            for (int i = 0; i < ne; ++i) x &= row(P[at + i]);
          }
          if (tf & KAD_TERM_HAS_FIELD) {
            if (!(tf & KAD_TERM_FIELD_VALID)) {  // :119-122: only where the expressions matched
              e |= x;
              live &= ~x;
              continue;
            }
            for (int i = 0; i < nf; ++i) x &= row(P[at + ne + i]);
          }
          m |= x;
          live &= ~x;
        }
      }
    }
  }
  if (f & KAD_OVR_BAD_VALUE) e |= m;  // util.go:125-131: unmarshalled only where the rule matched
  o.M[g] = m;
  o.E[g] = e;
}

// the largest i in [0, n) with off[i] <= key (off[0] <= key < off[n])
template <class T>
__device__ __forceinline__ int owner_of(const T* off, int n, int64_t key) {
  int lo = 0, hi = n;  // off[lo] <= key < off[hi]
  while (hi - lo > 1) {
    const int mid = lo + ((hi - lo) >> 1);
    if ((int64_t)off[mid] <= key)
      lo = mid;
    else
      hi = mid;
  }
  return lo;
}

__device__ __forceinline__ bool bit_at(const uint64_t* rows, int nch, int r, int c) {
  return (rows[(size_t)r * nch + (c >> 6)] >> (c & 63)) & 1;
}

__global__ __launch_bounds__(256) void override_status_kernel(OverrideDev o) {
  const int i = blockIdx.x * 256 + threadIdx.x;
  if (i >= o.n_obj) return;
  const int nch = (o.C + 63) >> 6;
  const int32_t* src = nullptr;
  int n = 0;
  if (!o.from_results) {
    src = o.place_cluster + o.place_off[i];
    n = o.place_off[i + 1] - o.place_off[i];
  } else {
    const int st = o.res_status[i];
    if (st == KAD_ST_OK) {
      src = o.res_cluster + (o.out_off[i] - o.slot_lo);
      n = o.res_count[i];
    } else if (st == KAD_ST_STICKY) {
      src = o.cur_id + o.cur_off[i];
      n = o.cur_off[i + 1] - o.cur_off[i];
    }
  }
  int status = 0;
  for (int q = 0; q < 2 && !status; ++q) {
    const int pol = o.obj_policy[2 * (size_t)i + q];
    if (pol < 0) continue;
    bool err = false;
    for (int r = o.pol_rule_off[pol]; r < o.pol_rule_off[pol + 1]; ++r)
      for (int k = 0; k < n; ++k) {
        const int c = src[k];
        if (c >= 0) err |= bit_at(o.E, nch, r, c);
      }
    if (err) status = q + 1;
  }
  o.status[i] = status;
}

// Slot reads and row writes are one element per lane in lane order (coalesced); the object's policies and
// their rule ranges differ from lane to lane, so they are vector loads (the rule rows they lead to are
// R x nch x 16 B and stay in L2).
__global__ __launch_bounds__(256) void override_match_kernel(OverrideDev o) {
  const int64_t s = (int64_t)blockIdx.x * 256 + threadIdx.x;
  if (s >= o.n_slots) return;
  const int nch = (o.C + 63) >> 6;
  int i, c;
  bool placed = true;
  if (!o.from_results) {
    i = owner_of(o.place_off, o.n_obj, s);
    c = o.place_cluster[s];
  } else if (s < o.n_out) {
    const int64_t key = s + o.slot_lo;
    i = owner_of(o.out_off, o.n_obj, key);
    placed = o.res_status[i] == KAD_ST_OK && key - o.out_off[i] < (int64_t)o.res_count[i];
    c = placed ? o.res_cluster[s] : -1;
  } else {
    const int64_t j = s - o.n_out + o.cur_lo;
    i = owner_of(o.cur_off, o.n_obj, j);
    placed = o.res_status[i] == KAD_ST_STICKY;
    c = o.cur_id[j];
  }
  placed = placed && c >= 0 && o.status[i] == 0;
  uint32_t* out = o.matched + (size_t)s * o.RW;
  int j = 0, w = 0;
  uint32_t acc = 0;
  if (placed)
    for (int q = 0; q < 2; ++q) {
      const int pol = o.obj_policy[2 * (size_t)i + q];
      if (pol < 0) continue;
      for (int r = o.pol_rule_off[pol]; r < o.pol_rule_off[pol + 1]; ++r) {  // <= 32 * RW rules (host check)
        acc |= (uint32_t)bit_at(o.M, nch, r, c) << (j & 31);
        if ((++j & 31) == 0) {
          out[w++] = acc;
          acc = 0;
        }
      }
    }
  if (w < o.RW) out[w++] = acc;
  while (w < o.RW) out[w++] = 0;
}

hipError_t launch_override_rule_rows(const OverrideDev& o, hipStream_t st) {
  (void)hipGetLastError();
  const long lanes = (long)o.R * ((o.C + 63) >> 6);
  if (lanes > 0)
    hipLaunchKernelGGL(override_rule_rows_kernel, dim3((unsigned)((lanes + 255) / 256)), dim3(256), 0, st, o);
  return hipGetLastError();
}

hipError_t launch_override_match(const OverrideDev& o, hipStream_t st) {
  (void)hipGetLastError();
  if (o.n_obj > 0)
    hipLaunchKernelGGL(override_status_kernel, dim3((unsigned)((o.n_obj + 255) / 256)), dim3(256), 0, st, o);
  if (o.n_slots > 0)
    hipLaunchKernelGGL(override_match_kernel, dim3((unsigned)((o.n_slots + 255) / 256)), dim3(256), 0, st, o);
  return hipGetLastError();
}

}  // namespace kad
