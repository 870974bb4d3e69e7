// Revision history (kad_revision_plan): the sync controller's syncRevisions (pkg/controllers/sync/history.go:36-120,
// with pkg/controllers/util/history/controller_history.go:91-176) for a batch of federated objects.
//
// Per object the reference hashes the patch of its pod template (HashControllerRevision: FNV-1 32 over the patch
// bytes, then over the decimal of the collision count), compares the patch with the data of every listed
// ControllerRevision (EqualRevision), splits the list into current and old, dedups the current ones, renumbers or
// relabels the kept one, sorts the old ones, deletes those beyond the history limit and relabels the rest. The API
// calls are the caller's: the product is the ordered action plan.
//
//   hr_hash_kernel        a lane per object (the FNV chain is serial), objects in the host's order of descending patch
//                         length. A wave stages HR_TILE bytes of each of its 64 objects in LDS with 16-byte loads (four
//                         lanes cover one object's tile, one load instruction 16 objects), then every lane folds its
//                         own tile four bytes a step.
//   hr_compare_kernel<W>  a lane group per (object, revision) pair: the lengths, the hash labels, then a 16-byte
//                         strided compare that the group leaves at the first differing chunk (ballot). One byte a pair.
//   hr_plan_kernel<W>     blocks below n_long: one listed long object per block; the others: a lane group per object.
//                         Maximum, kept revision, the stable rank of every old revision (a count of smaller keys, ties
//                         by list index), the truncation prefix, the label subset tests (binary searches), the actions
//                         compacted in the reference's order (ballot + popcount below the lane, carried over passes).
//
// Integers only, no atomics, ordinary vector stores: nothing depends on an order.
#include "kad_history.h"

#include "kad_fnv.h"
#include "kad_wave.h"

namespace kad {

// the rest of a patch inside one 32-bit word: the whole word, or its first rem bytes (none for rem <= 0)
__device__ __forceinline__ uint32_t hr_fold(uint32_t h, uint32_t w, int rem) {
  if (rem >= 4) return fnv_word(h, w);
  for (int t = 0; t < rem; ++t) {
    h = (h * kFnvPrime) ^ (w & 0xffu);
    w >>= 8;
  }
  return h;
}

__global__ __launch_bounds__(HR_THREADS) void hr_hash_kernel(RevisionDev d) {
  constexpr int STRIDE4 = HR_TILE_STRIDE / 16, TILE4 = HR_TILE / 16;
  static_assert(TILE4 == 4 && HR_THREADS == 256, "four lanes load one object's tile, four waves a block");
  __shared__ uint4 s_tiles[HR_THREADS / 64][64 * STRIDE4];
  const int lane = (int)threadIdx.x & 63;
  uint4* const tile = s_tiles[threadIdx.x >> 6];
  const int64_t g = (int64_t)blockIdx.x * HR_THREADS + threadIdx.x;
  const bool live = g < d.n_hash;
  const int o = live ? d.hash_order[g] : 0;
  const int64_t off = live ? d.patch_off[o] : 0;
  const int len = live ? d.patch_len[o] : 0;
  // the four objects whose tiles this lane helps to load: object 16 k + lane / 4 of the wave, chunk lane % 4
  const int sub = lane >> 2, chunk = lane & 3;
  const uint8_t* src[4];
  int left[4];  // bytes of that object from this lane's chunk of step 0 on
#pragma unroll
  for (int k = 0; k < 4; ++k) {
    const int j = k * 16 + sub;
    src[k] = d.blob + shfl_i64(off, j) + chunk * 16;
    left[k] = __shfl(len, j) - chunk * 16;
  }
  const int steps = (wave_max_u_i32(len) + HR_TILE - 1) / HR_TILE;  // (every lane of the wave is active)
  uint32_t h = kFnvOffset;
  for (int s = 0; s < steps; ++s) {
    const int at = s * HR_TILE;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
      uint4 v = make_uint4(0, 0, 0, 0);
      // up to 15 bytes past the patch's end: its zero padding in the blob, which the host has checked is there
      if (left[k] - at > 0) v = *reinterpret_cast<const uint4*>(src[k] + at);
      tile[(k * 16 + sub) * STRIDE4 + chunk] = v;
    }
    wave_sync();
    int rem = len - at;
    if (rem > 0) {
#pragma unroll
      for (int q = 0; q < TILE4; ++q) {
        const uint4 v = tile[lane * STRIDE4 + q];
        h = hr_fold(h, v.x, rem);
        h = hr_fold(h, v.y, rem - 4);
        h = hr_fold(h, v.z, rem - 8);
        h = hr_fold(h, v.w, rem - 12);
        rem -= 16;
      }
    }
    wave_sync();
  }
  if (live) {
    if (d.obj_flags[o] & HR_OBJ_COLLISION) h = hr_fnv_i32(h, d.collision[o]);
    uint32_t val;
    const bool parsed = hr_update_label(h, &val);
    d.hash[o] = h;
    d.upd_hash[o] = val;
    d.upd_parsed[o] = parsed ? 1 : 0;
  }
}

// this group's bits of a ballot among the lanes that run it (W <= 64)
template <int W>
__device__ __forceinline__ uint64_t hr_mask(bool p) {
  const uint64_t m = ballot(p);
  if (W == 64) return m;
  return (m >> (lane_id_h() & ~(W - 1) & 63)) & ((1ull << (W & 63)) - 1);
}

template <int W>
__device__ __forceinline__ void hr_pair(const RevisionDev& d, const int64_t r, const int gl) {
  const int o = d.rev_obj[r];
  bool differ = true;
  if (d.limit[o] != 0) {
    const int32_t dl = d.rev_data_len[r];
    differ = !hr_equal_pre(dl, d.patch_len[o], (d.rev_flags[r] & HR_REV_HASH_PARSED) != 0, d.rev_hash[r], d.upd_parsed[o] != 0,
                           d.upd_hash[o]);
    if (!differ) {
      const uint4* const a = reinterpret_cast<const uint4*>(d.blob + d.rev_data_off[r]);
      const uint4* const b = reinterpret_cast<const uint4*>(d.blob + d.patch_off[o]);
      const int chunks = (dl + 15) >> 4, tail = dl & 15;
      for (int cb = 0; cb < chunks; cb += W) {  // the same trips on every lane of the group
        const int c = cb + gl;
        bool df = false;
        if (c < chunks) {
          const uint4 va = a[c], vb = b[c];
          uint32_t x[4] = {va.x ^ vb.x, va.y ^ vb.y, va.z ^ vb.z, va.w ^ vb.w};
          if (c == chunks - 1 && tail) {  // the bytes behind the end are padding: not compared
#pragma unroll
            for (int w = 0; w < 4; ++w) {
              const int valid = tail - 4 * w;
              if (valid < 4) x[w] &= valid <= 0 ? 0u : (1u << (8 * valid)) - 1u;
            }
          }
          df = (x[0] | x[1] | x[2] | x[3]) != 0;
        }
        if (hr_mask<W>(df) != 0) {
          differ = true;
          break;
        }
      }
    }
  }
  if (gl == 0) d.equal[r] = differ ? 0 : 1;
}

template <int W>
__global__ __launch_bounds__(HR_THREADS) void hr_compare_kernel(RevisionDev d) {
  constexpr int GPB = HR_THREADS / W;
  const int gl = (int)threadIdx.x & (W - 1), g = (int)threadIdx.x / W;
  const int64_t stride = (int64_t)gridDim.x * GPB;
  for (int64_t base = (int64_t)blockIdx.x * GPB; base < d.R; base += stride) {
    const int64_t r = base + g;
    if (r < d.R) hr_pair<W>(d, r, gl);
  }
}

// The W lanes that share an object: a lane group of a wave (W <= 64) or a block (W == 256). Every lane of them calls
// scan / any / max / sum / sync together.
template <int W>
struct HrLanes {
  int gl;          // this lane among them
  int64_t* s_red;  // W == 256: [2][4] in LDS
  int par;
  // how many lanes below this one hold p, and how many in all
  __device__ __forceinline__ void scan(bool p, int& excl, int& total) {
    if constexpr (W <= 64) {
      const uint64_t m = hr_mask<W>(p);
      excl = popc64(m & ((1ull << gl) - 1));
      total = popc64(m);
    } else {
      const uint64_t m = ballot(p);
      const int w = (int)threadIdx.x >> 6;
      if ((threadIdx.x & 63) == 0) s_red[par * 4 + w] = popc64(m);
      __syncthreads();  // the other parity is written next: one barrier a call
      excl = mbcnt(m);
      total = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int t = (int)s_red[par * 4 + q];
        if (q < w) excl += t;
        total += t;
      }
      par ^= 1;
    }
  }
  __device__ __forceinline__ bool any(bool p) {
    int e, t;
    scan(p, e, t);
    return t != 0;
  }
  __device__ __forceinline__ int64_t max(int64_t v) {
#pragma unroll
    for (int m = 1; m < (W < 64 ? W : 64); m <<= 1) {
      const int64_t u = shfl_xor_i64(v, m);
      v = u > v ? u : v;
    }
    if constexpr (W > 64) {
      if ((threadIdx.x & 63) == 0) s_red[par * 4 + (threadIdx.x >> 6)] = v;
      __syncthreads();
#pragma unroll
      for (int q = 0; q < 4; ++q) {
        const int64_t u = s_red[par * 4 + q];
        v = u > v ? u : v;
      }
      par ^= 1;
    }
    return v;
  }
  __device__ __forceinline__ int sum(int v) {
#pragma unroll
    for (int m = 1; m < (W < 64 ? W : 64); m <<= 1) v += __shfl_xor(v, m);
    if constexpr (W > 64) {
      if ((threadIdx.x & 63) == 0) s_red[par * 4 + (threadIdx.x >> 6)] = v;
      __syncthreads();
      v = 0;
#pragma unroll
      for (int q = 0; q < 4; ++q) v += (int)s_red[par * 4 + q];
      par ^= 1;
    }
    return v;
  }
  // the scratch written before is read after
  __device__ __forceinline__ void sync() {
    if constexpr (W <= 64)
      wave_sync_global();
    else
      __syncthreads();
  }
};

// IsLabelSubset(revision labels, wanted) (sync/history.go:122-136) over interned (key, value) pair ids, both lists
// ascending: an empty wanted set is a subset, no label holds none, else every wanted pair is searched for. (A wanted
// pair with an empty value equals a missing key in the reference: such objects are decided on the host.)
__device__ __forceinline__ bool hr_subset(const RevisionDev& d, const int r, const int w_lo, const int w_hi) {
  if (w_hi == w_lo) return true;
  const int l_lo = d.rev_lab_off[r], l_hi = d.rev_lab_off[r + 1];
  if (l_hi == l_lo) return false;
  for (int w = w_lo; w < w_hi; ++w) {
    const int key = d.want_lab[w];
    int lo = l_lo, hi = l_hi;
    while (lo < hi) {
      const int mid = (int)(((unsigned)lo + (unsigned)hi) >> 1);
      if (d.rev_lab[mid] < key)
        lo = mid + 1;
      else
        hi = mid;
    }
    if (lo >= l_hi || d.rev_lab[lo] != key) return false;
  }
  return true;
}

// One object, by its W lanes. Every loop with a group operation in it has the same trip count on all of them.
template <int W>
__device__ __forceinline__ void hr_object(const RevisionDev& d, const int o, HrLanes<W>& L) {
  const int64_t limit = d.limit[o];
  if (limit == 0) {  // history.go:47-50: no revision is read
    if (L.gl == 0) {
      d.hash[o] = 0;
      d.upd_hash[o] = 0;
      d.upd_parsed[o] = 0;
      d.n_old[o] = 0;
      d.keep[o] = -1;
      d.n_actions[o] = 0;
      d.last[o] = -1;
      d.rev_number[o] = 0;
    }
    return;
  }
  const int lo = d.rev_off[o], n = d.rev_off[o + 1] - lo;
  const int w_lo = d.want_off[o], w_hi = d.want_off[o + 1];
  const bool on_host = (d.obj_flags[o] & HR_OBJ_LABELS_ON_HOST) != 0;
  uint8_t* const act_kind = d.act_kind + d.out_off[o];
  int32_t* const act_rev = d.act_rev + d.out_off[o];
  int ex, tot;

  // ---- the split (history.go:62-68), maxRevision of the old ones (:71), the first current one with the largest
  // Revision (dedupCurRevisions, :221-228)
  int64_t my_old = 0, my_cur = I64_MIN;
  int my_keep = -1, my_n_old = 0;
  for (int b = 0; b < n; b += W) {
    const int i = b + L.gl;
    if (i < n) {
      const int64_t rev = d.rev_revision[lo + i];
      if (d.equal[lo + i]) {
        if (my_keep < 0 || rev > my_cur) {
          my_cur = rev;
          my_keep = i;
        }
      } else {
        ++my_n_old;
        if (rev > my_old) my_old = rev;
      }
    }
  }
  const int64_t revision_number = hr_revision_number(L.max(my_old));
  const int n_old = L.sum(my_n_old);
  const bool has_cur = n_old < n;
  const int64_t max_cur = L.max(my_cur);
  const int keep = has_cur ? (int)-L.max(my_keep >= 0 && my_cur == max_cur ? -(int64_t)my_keep : I64_MIN) : -1;

  // ---- the duplicates' deletes in list order (:231-238), then the kept one's action, or the create (:72-94)
  int pos = 0;
  uint8_t ka = HR_ACT_CREATE;
  if (has_cur) {
    const int keep_name = d.rev_name_rank[lo + keep];
    for (int b = 0; b < n; b += W) {
      const int i = b + L.gl;
      const bool del = i < n && d.equal[lo + i] && d.rev_name_rank[lo + i] != keep_name;
      L.scan(del, ex, tot);
      if (del) {
        act_kind[pos + ex] = HR_ACT_DELETE;
        act_rev[pos + ex] = i;
      }
      pos += tot;
    }
    ka = hr_keep_action(d.rev_revision[lo + keep], revision_number, on_host || hr_subset(d, lo + keep, w_lo, w_hi));
  }
  if (ka) {
    if (L.gl == 0) {
      act_kind[pos] = ka;
      act_rev[pos] = keep;
    }
    ++pos;
  }

  // ---- sort.Stable(byRevision) of the old ones (:165): an old revision's place is the number of old revisions
  // with a smaller key
  for (int b = 0; b < n; b += W) {
    const int i = b + L.gl;
    if (i < n && !d.equal[lo + i]) {
      const int64_t rev = d.rev_revision[lo + i], t = d.rev_time[lo + i];
      const int name = d.rev_name_rank[lo + i];
      int rank = 0;
      for (int j = 0; j < n; ++j)
        if (!d.equal[lo + j] && hr_key_less(d.rev_revision[lo + j], d.rev_time[lo + j], d.rev_name_rank[lo + j], j, rev, t, name, i)) ++rank;
      d.order[lo + rank] = i;
    }
  }
  L.sync();

  // ---- truncateRevisions' deletes (:166-181), then a relabel for every old one whose labels lack a wanted pair, the
  // deleted ones included (:114-118)
  const int kill = hr_kill(n_old, limit), base_b = pos, base_c = pos + kill;
  int carry = 0;
  for (int b = 0; b < n_old; b += W) {
    const int r = b + L.gl;
    const bool live = r < n_old;
    const int i = live ? d.order[lo + r] : 0;
    if (live && r < kill) {
      act_kind[base_b + r] = HR_ACT_DELETE;
      act_rev[base_b + r] = i;
    }
    const bool relabel = live && !on_host && !hr_subset(d, lo + i, w_lo, w_hi);
    L.scan(relabel, ex, tot);
    if (relabel) {
      act_kind[base_c + carry + ex] = HR_ACT_RELABEL;
      act_rev[base_c + carry + ex] = i;
    }
    carry += tot;
  }
  if (L.gl == 0) {
    d.n_old[o] = n_old;
    d.keep[o] = keep;
    d.n_actions[o] = base_c + carry;
    d.last[o] = n_old >= 1 && limit >= 1 ? d.order[lo + n_old - 1] : -1;  // :103-105
    d.rev_number[o] = revision_number;
  }
}

template <int W>
__global__ __launch_bounds__(HR_THREADS) void hr_plan_kernel(RevisionDev d) {
  __shared__ int64_t s_red[8];
  if ((int)blockIdx.x < d.n_long) {
    // ---- long path: one listed object per block
    HrLanes<256> L{(int)threadIdx.x, s_red, 0};
    hr_object<256>(d, d.long_list[blockIdx.x], L);
    return;
  }
  // ---- group path: the lanes of a group stay together; groups past O, and those whose object is long, idle
  constexpr int GPB = HR_THREADS / W;
  HrLanes<W> L{(int)threadIdx.x & (W - 1), nullptr, 0};
  const int g = (int)threadIdx.x / W;
  const int64_t stride = (int64_t)(gridDim.x - d.n_long) * GPB;
  for (int64_t base = (int64_t)(blockIdx.x - d.n_long) * GPB; base < d.O; base += stride) {
    const int64_t o = base + g;
    if (o < d.O && !d.obj_long[o]) hr_object<W>(d, (int)o, L);
  }
}

hipError_t launch_revision_hash(const RevisionDev& d, const RevisionRoute& r, hipStream_t st) {
  (void)hipGetLastError();
  if (r.hash_grid > 0) hipLaunchKernelGGL(hr_hash_kernel, dim3((unsigned)r.hash_grid), dim3(HR_THREADS), 0, st, d);
  return hipGetLastError();
}

hipError_t launch_revision_compare(const RevisionDev& d, const RevisionRoute& r, hipStream_t st) {
  (void)hipGetLastError();
  if (r.cmp_grid > 0)
    with_width<1>(r.cmp_width, [&](auto W) {
      hipLaunchKernelGGL((hr_compare_kernel<decltype(W)::value>), dim3((unsigned)r.cmp_grid), dim3(HR_THREADS), 0, st, d);
    });
  return hipGetLastError();
}

hipError_t launch_revision_plan(const RevisionDev& d, const RevisionRoute& r, hipStream_t st) {
  (void)hipGetLastError();
  const unsigned grid = (unsigned)(r.grid + r.long_grid);
  if (grid > 0)
    with_width<1>(r.width, [&](auto W) {
      hipLaunchKernelGGL((hr_plan_kernel<decltype(W)::value>), dim3(grid), dim3(HR_THREADS), 0, st, d);
    });
  return hipGetLastError();
}

}  // namespace kad

// ------------------------------------------------------ host half: kad_revision_plan
#include <numeric>

#include "kad_arena.h"

using namespace kad;

namespace {

// what the validation leaves for the launch
struct RevPlan {
  std::vector<int32_t> hash_order, rev_obj, long_list;
  std::vector<uint8_t> obj_long;
  std::vector<int64_t> out_off;
  int64_t short_revs = 0, pair_chunks = 0;
};

inline bool ascending_ids_bad(const int32_t* off, const int32_t* ids, int64_t rows, int64_t P) {
  if (csr_bad(off, ids, rows, 0, P)) return true;
  return first_bad(rows, [=](int64_t i) {
           for (int64_t k = (int64_t)off[i] + 1; k < off[i + 1]; ++k)
             if (ids[k] <= ids[k - 1]) return true;
           return false;
         }) >= 0;
}

}  // namespace

extern "C" {

// With a plan (kad_revision_plan) the same pass leaves the hash order, every revision's object, the long objects and
// the action offsets.
static int validate_revision(const kad_revision_batch* b, const kad_revision_view* out, int long_min, RevPlan* plan, std::string* err) {
  auto bad = [&](const char* m) {
    *err = m;
    return KAD_EINVAL;
  };
  const int64_t O = b->n_objects, P = b->n_pairs, BL = b->blob_len;
  if (O < 0 || P < 0 || BL < 0 || b->action_capacity < 0) return bad("negative count");
  if (O && (!b->limit || !b->collision || !b->obj_flags || !b->patch_off || !b->patch_len)) return bad("object array missing");
  if (BL && !b->blob) return bad("blob missing");
  if (off_bad(b->rev_off, O)) return bad("rev_off not monotone from 0");
  const int64_t R = b->rev_off[O];
  const int32_t* ro = b->rev_off;
  if (first_bad(O, [=](int64_t i) { return ro[i + 1] - ro[i] > HR_MAX_REVS; }) >= 0) {
    *err = "more than KAD_REV_MAX_REVISIONS revisions on one object";
    return KAD_EUNSUPPORTED;
  }
  if (R && (!b->rev_data_off || !b->rev_data_len || !b->rev_revision || !b->rev_time || !b->rev_name_rank || !b->rev_flags || !b->rev_hash))
    return bad("revision array missing");
  const uint8_t* of = b->obj_flags;
  const int64_t* po = b->patch_off;
  const int32_t* pl = b->patch_len;
  if (first_bad(O, [=](int64_t i) {
        if (of[i] & ~3u) return true;
        return pl[i] < 0 || po[i] < 0 || (po[i] & 15) != 0 || po[i] > BL || (((int64_t)pl[i] + 15) & ~(int64_t)15) > BL - po[i];
      }) >= 0)
    return bad("obj_flags: unknown flag, or a patch not 16-byte aligned or not inside the blob with its padding");
  const int64_t* dof = b->rev_data_off;
  const int32_t *dl = b->rev_data_len, *nr = b->rev_name_rank;
  const uint8_t* rf = b->rev_flags;
  if (first_bad(R, [=](int64_t r) {
        if (rf[r] & ~1u) return true;
        return dl[r] < 0 || dof[r] < 0 || (dof[r] & 15) != 0 || dof[r] > BL || (((int64_t)dl[r] + 15) & ~(int64_t)15) > BL - dof[r];
      }) >= 0)
    return bad("rev_flags: unknown flag, or a revision's data not 16-byte aligned or not inside the blob with its padding");
  if (first_bad(O, [=](int64_t i) {
        for (int64_t r = ro[i]; r < ro[i + 1]; ++r)
          if (nr[r] < 0 || nr[r] >= ro[i + 1] - ro[i]) return true;
        return false;
      }) >= 0)
    return bad("rev_name_rank outside [0, the object's revisions)");
  if (ascending_ids_bad(b->rev_lab_off, b->rev_lab, R, P)) return bad("rev_lab malformed, pair id outside [0, n_pairs) or not strictly ascending");
  if (ascending_ids_bad(b->want_off, b->want_lab, O, P)) return bad("want_lab malformed, pair id outside [0, n_pairs) or not strictly ascending");
  int64_t need = 0;
  for (int64_t i = 0; i < O; ++i) need += hr_action_cap(ro[i + 1] - ro[i]);
  if (need > INT32_MAX) return bad("more than 2^31 - 1 action slots");
  if (need > b->action_capacity) {
    *err = "action_capacity below the sum of 2 n + 1 over the objects";
    return KAD_ENOSPC;
  }
  if (!out || !out->out_off || (O && (!out->hash || !out->upd_hash || !out->upd_parsed || !out->n_old || !out->keep || !out->n_actions ||
                                      !out->last || !out->rev_number)) ||
      (R && (!out->equal || !out->order)) || (need && (!out->act_kind || !out->act_rev)))
    return bad("output view missing");
  if (plan) {
    plan->obj_long.assign((size_t)O, 0);
    plan->rev_obj.resize((size_t)R);
    plan->out_off.resize((size_t)O + 1);
    plan->out_off[0] = 0;
    for (int64_t i = 0; i < O; ++i) {
      const int64_t n = ro[i + 1] - ro[i];
      plan->out_off[(size_t)i + 1] = plan->out_off[(size_t)i] + hr_action_cap(n);
      for (int64_t r = ro[i]; r < ro[i + 1]; ++r) {
        plan->rev_obj[(size_t)r] = (int32_t)i;
        plan->pair_chunks += ((int64_t)dl[r] + 15) >> 4;
      }
      if (b->limit[i] != 0) plan->hash_order.push_back((int32_t)i);
      if (n <= long_min) {
        plan->short_revs += n;
        continue;
      }
      plan->obj_long[(size_t)i] = 1;
      plan->long_list.push_back((int32_t)i);
    }
    // the route sorts by length: tiles descending, the object index among equals (a unique order)
    std::stable_sort(plan->hash_order.begin(), plan->hash_order.end(),
                     [pl](int32_t x, int32_t y) { return (pl[x] + HR_TILE - 1) / HR_TILE > (pl[y] + HR_TILE - 1) / HR_TILE; });
  }
  return KAD_OK;
}

static int revision_locked(kad_ctx* c, const kad_revision_batch* b, const kad_revision_view* out) {
  Stage& stg = c->stage[STG_REVISION];
  const int long_min = stg.force.long_min_or(HR_LONG_MIN);
  std::string err;
  RevPlan plan;
  if (int r = validate_revision(b, out, long_min, &plan, &err)) return fail(c, r, err);
  const int O = b->n_objects;
  memcpy(out->out_off, plan.out_off.data(), sizeof(int64_t) * ((size_t)O + 1));
  if (O == 0) return KAD_OK;
  HIPCHK(c, hipSetDevice(c->device));
  const int n_long = (int)plan.long_list.size(), n_hash = (int)plan.hash_order.size();
  const int64_t R = b->rev_off[O];
  RevisionRoute route = route_revision(O, n_hash, n_long, plan.short_revs, R, plan.pair_chunks, n_cus());
  group_force_apply(stg.force, n_long < O, O, n_cus(), route.width, route.grid);
  group_force_apply(stg.force, R > 0, R, n_cus(), route.cmp_width, route.cmp_grid);  // one forced width: both group kernels
  route.long_min = long_min;
  const size_t o = (size_t)O, nr = (size_t)R, cap = (size_t)plan.out_off[o];
  RevisionDev d{};
  d.O = O;
  d.n_hash = n_hash;
  d.n_long = n_long;
  d.R = R;
  Arena a;
  a.in(d.limit, b->limit, o);
  a.in(d.collision, b->collision, o);
  a.in(d.obj_flags, b->obj_flags, o);
  a.in(d.patch_off, b->patch_off, o);
  a.in(d.patch_len, b->patch_len, o);
  a.in(d.blob, b->blob, (size_t)b->blob_len);
  a.in(d.rev_off, b->rev_off, o + 1);
  a.in(d.rev_data_off, b->rev_data_off, nr);
  a.in(d.rev_data_len, b->rev_data_len, nr);
  a.in(d.rev_revision, b->rev_revision, nr);
  a.in(d.rev_time, b->rev_time, nr);
  a.in(d.rev_name_rank, b->rev_name_rank, nr);
  a.in(d.rev_flags, b->rev_flags, nr);
  a.in(d.rev_hash, b->rev_hash, nr);
  a.in(d.rev_lab_off, b->rev_lab_off, nr + 1);
  a.in(d.rev_lab, b->rev_lab, (size_t)b->rev_lab_off[R]);
  a.in(d.want_off, b->want_off, o + 1);
  a.in(d.want_lab, b->want_lab, (size_t)b->want_off[O]);
  a.in(d.hash_order, plan.hash_order.data(), (size_t)n_hash);
  a.in(d.rev_obj, plan.rev_obj.data(), nr);
  a.in(d.obj_long, plan.obj_long.data(), o);
  a.in(d.long_list, plan.long_list.data(), (size_t)n_long);
  a.in(d.out_off, plan.out_off.data(), o + 1);
  a.out(d.hash, out->hash, o);
  a.out(d.upd_hash, out->upd_hash, o);
  a.out(d.upd_parsed, out->upd_parsed, o);
  a.out(d.equal, out->equal, nr);
  a.out(d.order, out->order, nr);
  a.out(d.n_old, out->n_old, o);
  a.out(d.keep, out->keep, o);
  a.out(d.n_actions, out->n_actions, o);
  a.out(d.last, out->last, o);
  a.out(d.rev_number, out->rev_number, o);
  a.out(d.act_kind, out->act_kind, cap);
  a.out(d.act_rev, out->act_rev, cap);
  if (int r = a.commit(c, stg.buf)) return r;
  HIPCHK(c, hipEventRecord(stg.ev[0], c->stream));
  HIPCHK(c, launch_revision_hash(d, route, c->stream));
  HIPCHK(c, hipEventRecord(stg.ev[1], c->stream));
  HIPCHK(c, launch_revision_compare(d, route, c->stream));
  HIPCHK(c, hipEventRecord(stg.ev[2], c->stream));
  HIPCHK(c, launch_revision_plan(d, route, c->stream));
  HIPCHK(c, hipEventRecord(stg.ev[3], c->stream));
  if (int r = a.fetch(c)) return r;
  stage_ran(stg, route);
  HIPCHK(c, hipStreamSynchronize(c->stream));
  return KAD_OK;
}

int kad_revision_plan_check(const kad_revision_batch* b, const kad_revision_view* out) {
  return check_guarded([&]() -> int {
    if (!b) return KAD_EINVAL;
    std::string err;
    return validate_revision(b, out, HR_LONG_MIN, nullptr, &err);
  });
}

int kad_revision_plan(kad_ctx* c, const kad_revision_batch* b, const kad_revision_view* out) {
  return entry(c, b != nullptr, [&]() -> int {
    return revision_locked(c, b, out);
  });
}

int kad_revision_plan_timing(kad_ctx* c, float ms[3]) { return stage_timing(c, STG_REVISION, 3, ms, "no kad_revision_plan ran"); }

int kad_revision_plan_route_eval(int32_t n_objects, int32_t n_hash, int32_t n_long, int64_t short_revs, int64_t n_pairs,
                                 int64_t pair_chunks, int32_t n_cu, int32_t* out) {
  if (!out || n_objects < 0 || n_hash < 0 || n_hash > n_objects || n_long < 0 || n_long > n_objects || short_revs < 0 || n_pairs < 0 ||
      pair_chunks < 0 || n_cu < 1)
    return KAD_EINVAL;
  return route_record<KAD_REV_ROUTE_FIELDS>(out, route_revision(n_objects, n_hash, n_long, short_revs, n_pairs, pair_chunks, n_cu));
}

int kad_revision_plan_last_route(kad_ctx* c, int32_t* out) { return stage_last_route(c, STG_REVISION, out, "no kad_revision_plan ran"); }

int kad_revision_plan_debug_route(kad_ctx* c, int32_t force_width, int32_t force_long_min) {
  return stage_debug_route(c, STG_REVISION, group_width_ok(force_width, 1), GroupForce{force_width, force_long_min, 0});
}

}  // extern "C"
