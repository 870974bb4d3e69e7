// kad_revision_plan (kad_history.hip): the sync controller's syncRevisions for a batch of federated objects; the
// decisions the host and the device share, the device arrays, the launch decisions, the launches.
// The first part is plain C++ (KAD_HOST_ONLY stops after it: tests/history_main.cpp).
#pragma once
#include <stdint.h>

#include "kad_groups.h"

#ifdef KAD_HOST_ONLY
#define KAD_HD inline
#else
#include <hip/hip_runtime.h>
#define KAD_HD __host__ __device__ inline
#endif

namespace kad {

constexpr int HR_THREADS = 256;
// More listed ControllerRevisions than this on one object: KAD_EUNSUPPORTED (KAD_REV_MAX_REVISIONS). The plan
// kernel ranks an object's old revisions by counting smaller keys, n^2 key reads: 4096 is 16 i's a thread of a block.
constexpr int HR_MAX_REVS = 4096;
// A lane of a plan-kernel group takes HR_PER_LANE revisions of a mean object and a lane of a compare-kernel group
// HR_CMP_PER_LANE 16-byte chunks of a mean revision; objects with more listed revisions than HR_LONG_MIN take a
// whole block of the plan kernel. Chosen from DESIGN §7.4's table (every width forced through
// kad_revision_plan_debug_route, 1.8 KB patches, 3.2 revisions an object): the compare kernel at the width that 4
// chunks a lane give (32) is within 4 % of the best forced width at 10 000 and 100 000 objects (1 chunk a lane, width
// 64, is 23 % slower at 100 000; width 4 is 34 % slower); the plan kernel at 1 revision a lane (width 4) is within
// 4 % of the best forced width at 10 000 and 9 % behind width 1 at 100 000, and width 16 is 2.9 times slower there. The table
// has no object beyond 7 revisions, so it does not place HR_LONG_MIN: a block on 3 revisions is 25 times slower than a
// 4-lane group, which only says the threshold must stay well above the common case. 256 is four passes of a 64-lane
// group.
constexpr int HR_LONG_MIN = 256;
constexpr int HR_PER_LANE = 1;
constexpr int HR_CMP_PER_LANE = 4;
// the hash kernel: a lane per object, a wave stages HR_TILE bytes of each of its 64 objects a step, every tile
// HR_TILE_STRIDE bytes from the next in LDS (16-byte aligned, and 16 bytes off a multiple of the bank row so that
// the lanes' own 16-byte reads spread over the banks)
constexpr int HR_TILE = 64;
constexpr int HR_TILE_STRIDE = HR_TILE + 16;

constexpr uint8_t HR_OBJ_COLLISION = 1, HR_OBJ_LABELS_ON_HOST = 2;  // KAD_REV_OBJ_*
constexpr uint8_t HR_REV_HASH_PARSED = 1;                            // KAD_REV_HASH_PARSED
constexpr uint8_t HR_ACT_CREATE = 1, HR_ACT_DELETE = 2, HR_ACT_RENUMBER = 3, HR_ACT_RELABEL = 4;  // KAD_REV_ACT_*

// FNV-1 32 over bytes, one at a time: the host's restatement of the hash kernel's fold
KAD_HD uint32_t hr_fnv_bytes(uint32_t h, const uint8_t* p, int64_t n) {
  for (int64_t i = 0; i < n; ++i) h = (h * 16777619u) ^ p[i];
  return h;
}
// ... continued over the ASCII of strconv.FormatInt(int64(v), 10): HashControllerRevision's probe
// (controller_history.go:101-103). A negative value writes its '-'.
KAD_HD uint32_t hr_fnv_i32(uint32_t h, int32_t v) {
  uint32_t m = v < 0 ? 0u - (uint32_t)v : (uint32_t)v;  // |INT32_MIN| = 2^31 fits
  if (v < 0) h = (h * 16777619u) ^ (uint32_t)'-';
  uint32_t div = 1;
  while (m / div >= 10) div *= 10;
  for (; div > 0; div /= 10) h = (h * 16777619u) ^ (uint32_t)('0' + (m / div) % 10);
  return h;
}

// The update revision's hash label as EqualRevision reads it (controller_history.go:132-138): the label is
// rand.SafeEncodeString(fmt.Sprint(sum)), every byte b of the decimal replaced by "bcdfghjklmnpqrstvwxz2456789"[b % 27].
// '0' .. '5' (48 .. 53) land on '4' .. '9' and '6' .. '9' (54 .. 57) on 'b', 'c', 'd', 'f', so strconv.ParseInt(label,
// 10, 32) succeeds exactly when the decimal holds no digit above 5 and the number re-read with every digit raised by
// 4 is at most 2^31 - 1. Returns whether it parses; *val = uint32 of the parsed number.
KAD_HD bool hr_update_label(uint32_t sum, uint32_t* val) {
  uint64_t v = 0, scale = 1;
  bool ok = true;
  do {
    const uint32_t d = sum % 10;
    ok = ok && d <= 5;
    v += (uint64_t)(d + 4) * scale;
    scale *= 10;
    sum /= 10;
  } while (sum);
  ok = ok && v <= 2147483647ull;
  *val = ok ? (uint32_t)v : 0u;
  return ok;
}

// EqualRevision before any byte is read (controller_history.go:139-142), in the order the compare kernel tests:
// the lengths (bytes.Equal of different lengths is false whatever the labels say), then the two hash labels, which
// count only if both parsed. 0: not equal; 1: the bytes decide.
KAD_HD int hr_equal_pre(int32_t data_len, int32_t patch_len, bool rev_parsed, uint32_t rev_hash, bool upd_parsed, uint32_t upd_hash) {
  if (data_len != patch_len) return 0;
  if (rev_parsed && upd_parsed && rev_hash != upd_hash) return 0;
  return 1;
}

// maxRevision(old) + 1 (sync/history.go:71, 242-250): the maximum starts at 0; Go's int64 wraps
KAD_HD int64_t hr_revision_number(int64_t max_old) { return (int64_t)((uint64_t)(max_old > 0 ? max_old : 0) + 1u); }

// truncateRevisions (history.go:164-183): toKill = len(old) - int(limit) in Go's wrapping int, the first toKill of
// the sorted list are deleted
KAD_HD int32_t hr_kill(int32_t n_old, int64_t limit) {
  const int64_t k = (int64_t)((uint64_t)(int64_t)n_old - (uint64_t)limit);
  return k <= 0 ? 0 : (k >= n_old ? n_old : (int32_t)k);
}

// what follows dedupCurRevisions for the kept revision (history.go:83-93): RENUMBER below the revision number,
// else RELABEL unless its labels already hold the wanted ones; 0: nothing
KAD_HD uint8_t hr_keep_action(int64_t keep_revision, int64_t revision_number, bool label_subset) {
  if (keep_revision < revision_number) return HR_ACT_RENUMBER;
  return label_subset ? 0 : HR_ACT_RELABEL;
}

// byRevision.Less (controller_history.go:168-176) with the list index last: sort.Stable's order is the order of
// these keys. Names compare through the object's name ranks.
KAD_HD bool hr_key_less(int64_t rev_a, int64_t t_a, int32_t name_a, int32_t idx_a, int64_t rev_b, int64_t t_b, int32_t name_b, int32_t idx_b) {
  if (rev_a != rev_b) return rev_a < rev_b;
  if (t_a != t_b) return t_a < t_b;
  if (name_a != name_b) return name_a < name_b;
  return idx_a < idx_b;
}

// the most actions one object of n listed revisions can get: the currents' deletes and the kept one's action (or the
// create), then a delete and a relabel for every old one
KAD_HD int64_t hr_action_cap(int64_t n) { return 2 * n + 1; }

// The launch decision of one kad_revision_plan, taken here and nowhere else (kad_revision_plan_route_eval /
// _last_route show it). Hash kernel: a lane per object with a history limit, in the host's order of descending
// patch length (the route SORTS by length: the 64 objects of a wave then run the same number of tiles, and one very
// long patch waits for its 63 neighbours in length, not for 63 short ones). Compare kernel: a wave is 64 / cmp_width
// lane groups, a group takes one (object, revision) pair at a time; the width is the mean data length in 16-byte
// chunks over HR_CMP_PER_LANE. Plan kernel: a lane group per object over its revisions, the width their mean over
// HR_PER_LANE; objects with more than long_min revisions take a block each.
struct RevisionRoute {
  int32_t width, long_min, cmp_width, hash_grid, cmp_grid, grid, long_grid, threads;
};
inline RevisionRoute route_revision(int O, int n_hash, int n_long, int64_t short_revs, int64_t n_pairs, int64_t pair_chunks, int n_cu) {
  RevisionRoute r{};
  const int n_short = O - n_long;
  r.width = group_width(short_revs, n_short, 1, HR_PER_LANE);
  r.long_min = HR_LONG_MIN;
  r.cmp_width = group_width(pair_chunks, n_pairs, 1, HR_CMP_PER_LANE);
  r.hash_grid = (int32_t)(((int64_t)n_hash + HR_THREADS - 1) / HR_THREADS);
  r.cmp_grid = n_pairs > 0 ? group_grid(n_pairs, r.cmp_width, n_cu) : 0;
  r.grid = n_short > 0 ? group_grid(O, r.width, n_cu) : 0;
  r.long_grid = n_long;
  r.threads = HR_THREADS;
  return r;
}

}  // namespace kad

#ifndef KAD_HOST_ONLY
namespace kad {

struct RevisionDev {
  int O, n_hash, n_long;
  int64_t R;
  const int64_t* limit;
  const int32_t* collision;
  const uint8_t* obj_flags;
  const int64_t* patch_off;
  const int32_t* patch_len;
  const uint8_t* blob;
  const int32_t* rev_off;
  const int64_t* rev_data_off;
  const int32_t* rev_data_len;
  const int64_t *rev_revision, *rev_time;
  const int32_t* rev_name_rank;
  const uint8_t* rev_flags;
  const uint32_t* rev_hash;
  const int32_t *rev_lab_off, *rev_lab, *want_off, *want_lab;
  // built on the host while it validates
  const int32_t* hash_order;  // [n_hash] the objects with a history limit, by descending patch length
  const int32_t* rev_obj;     // [R] a revision's object
  const uint8_t* obj_long;    // [O] 1: the object is on the plan kernel's long path
  const int32_t* long_list;   // [n_long] ascending
  const int64_t* out_off;     // [O + 1] where an object's actions go
  // outputs
  uint32_t *hash, *upd_hash;  // [O]
  uint8_t* upd_parsed;        // [O]
  uint8_t* equal;             // [R]
  int32_t* order;             // [R] per object its old revisions in sorted order (indices within the object)
  int32_t *n_old, *keep, *n_actions, *last;  // [O]
  int64_t* rev_number;        // [O]
  uint8_t* act_kind;          // [out_off[O]]
  int32_t* act_rev;
};

hipError_t launch_revision_hash(const RevisionDev& d, const RevisionRoute& r, hipStream_t st);
hipError_t launch_revision_compare(const RevisionDev& d, const RevisionRoute& r, hipStream_t st);
hipError_t launch_revision_plan(const RevisionDev& d, const RevisionRoute& r, hipStream_t st);

}  // namespace kad
#endif  // KAD_HOST_ONLY
