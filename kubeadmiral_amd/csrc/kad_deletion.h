// kad_deletion_plan / kad_deletion_finish (kad_deletion.hip): the deletion arm of the sync controller's reconcile for
// a batch of federated objects, the per-(object, observed cluster) decision shared by the device and the host, the
// launch decision, the launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kad_groups.h"

namespace kad {

constexpr int DEL_MAX_CLUSTERS = 16384;  // KAD_DISPATCH_MAX_CLUSTERS: a byte per cluster in LDS, 16 KiB a block at most
constexpr int DEL_THREADS = 256;
// Objects with more entries than this go one per wave (kad_rollout's value; no generated batch has such an object,
// so the cost table does not place it), and a lane of a group takes this many entries of a mean object: an entry
// is 5 to 10 bytes and a table lookup, the per-object part (two offsets, the flags, five stores) weighs more, so
// few lanes per object keep more objects in a wave (DESIGN §7.5 has the table).
constexpr int DEL_LONG_MIN = 256;
constexpr int DEL_PER_LANE = 4;
constexpr uint8_t DEL_CL_READY = 1;                                                             // KAD_DISPATCH_CL_READY
constexpr uint8_t DEL_CL_ALL = 15;                                                              // KAD_DISPATCH_CL_*
constexpr uint8_t DEL_OB_EXISTS = 1, DEL_OB_DELETING = 2, DEL_OB_ADOPTED = 4, DEL_OB_RETRIEVAL_FAILED = 8;  // KAD_DISPATCH_OB_*
constexpr uint8_t DEL_OP_NONE = 0, DEL_OP_DELETE = 3, DEL_OP_REMOVE_LABEL = 4;                  // KAD_DISPATCH_OP_*
constexpr uint8_t DEL_OBJ_HAS_FINALIZER = 1, DEL_OBJ_ORPHAN_ALL = 2, DEL_OBJ_ORPHAN_ADOPTED = 4,
                  DEL_OBJ_POSSIBLE_ORPHAN = 8;                                                  // KAD_DEL_OBJ_*
constexpr uint8_t DEL_PRE_RETRIEVAL_FAILED = 1, DEL_PRE_NOT_READY = 2;                          // KAD_DEL_PRE_*
constexpr uint8_t DEL_ACT_DELETE_HISTORY = 1, DEL_ACT_REMOVE_FINALIZER = 2, DEL_ACT_NOTHING = 4,
                  DEL_ACT_RECORD_ERROR = 8;                                                     // KAD_DEL_ACT_*
constexpr uint8_t DEL_WAIT_TIMED_OUT = 1, DEL_WAIT_CHECK_TIMED_OUT = 2;                         // KAD_DEL_WAIT_*
constexpr uint8_t DEL_CHK_GET_FAILED = 1, DEL_CHK_DELETING = 2, DEL_CHK_LABELLED = 4, DEL_CHK_UNLABELLED = 8;  // KAD_DEL_CHK_*
enum DelStatus { DEL_ST_OK, DEL_ST_ERROR, DEL_ST_RECHECK };                                     // KAD_DEL_ST_*
enum DelReason { DEL_RSN_NONE, DEL_RSN_TIMED_OUT, DEL_RSN_RETRIEVAL_FAILED, DEL_RSN_NOT_READY, DEL_RSN_OPS_FAILED,
                 DEL_RSN_WAITING, DEL_RSN_CHECK_TIMED_OUT, DEL_RSN_CHECK_NOT_READY, DEL_RSN_CHECKS_FAILED };  // KAD_DEL_RSN_*

struct DeletionDev {
  int C, O, n_long, long_min;
  const uint8_t* cluster_flags;  // [C], read 16 bytes at a time (the arena pads the part)
  const uint8_t* obj_flags;      // [O]
  const int32_t *obj_ob_off, *ob_cluster;  // [O + 1], [B]
  const uint8_t* ob_flags;       // [B]
  const int32_t* long_list;      // [n_long] the objects of the long path, ascending (built on the host)
  int32_t* n_unready;            // [2] scratch: unready clusters of cluster_flags, of chk_cluster_flags
  // plan
  uint8_t* out_op;               // [B]
  int32_t *n_ops, *n_remaining, *n_retrieval_failed;  // [O]
  uint8_t *obj_pre, *obj_first;  // [O]
  // finish
  const uint8_t *op_ok, *obj_wait;           // [B], [O]
  const int32_t *chk_off, *chk_cluster;      // [O + 1], [K]
  const uint8_t *chk_flags, *chk_cluster_flags;  // [K], [C] (16 bytes at a time)
  uint8_t *obj_status, *obj_reason, *obj_then;   // [O]
  int32_t *n_failed_ops, *n_failed_checks;   // [O]
};

// an object walks the clusters (handleDeletionInClusters): it has the finalizer, or no federated object exists
__host__ __device__ __forceinline__ bool del_walks(uint8_t of) {
  return (of & (DEL_OBJ_HAS_FINALIZER | DEL_OBJ_POSSIBLE_ORPHAN)) != 0;
}
// removeManagedLabel's arms (:741, :350) against deleteFromClusters'
__host__ __device__ __forceinline__ bool del_label_arm(uint8_t of) {
  return (of & (DEL_OBJ_ORPHAN_ALL | DEL_OBJ_POSSIBLE_ORPHAN)) != 0;
}

// What handleDeletionInClusters' loop (pkg/controllers/sync/controller.go:938-964) and the arm's deletionFunc do with
// one observed cluster: of = the object's DEL_OBJ_* bits, ready = the cluster is ready, ob = the observation's
// DEL_OB_* bits.
struct DelDecision {
  uint8_t op, remaining, failed;
};
__host__ __device__ __forceinline__ DelDecision del_decide(uint8_t of, bool ready, uint8_t ob) {
  if (!del_walks(of) || !ready) return DelDecision{DEL_OP_NONE, 0, 0};           // :735-739, :941-944
  if (ob & DEL_OB_RETRIEVAL_FAILED) return DelDecision{DEL_OP_NONE, 0, 1};       // :953-958
  if (!(ob & DEL_OB_EXISTS)) return DelDecision{DEL_OP_NONE, 0, 0};              // :959-961
  if (del_label_arm(of))                                                        // :802-807
    return DelDecision{(uint8_t)((ob & DEL_OB_DELETING) ? DEL_OP_NONE : DEL_OP_REMOVE_LABEL), 0, 0};
  // :856-859, deleteFromCluster with respectOrphaningBehavior (:834-843; orphan-all never comes here)
  const bool orphan = (of & DEL_OBJ_ORPHAN_ADOPTED) && (ob & DEL_OB_ADOPTED);
  return DelDecision{(uint8_t)(orphan ? DEL_OP_REMOVE_LABEL : DEL_OP_DELETE), 1, 0};
}

// The counts of one object's walk and what follows from them.
struct DelCounts {
  int32_t n_ops, n_remaining, n_failed_rf, n_failed_ops, n_failed_checks;
};
struct DelPlanObj {
  uint8_t pre, first;
};
__host__ __device__ __forceinline__ DelPlanObj del_plan_obj(uint8_t of, const DelCounts& k, int n_unready) {
  if (!del_walks(of)) return DelPlanObj{0, DEL_ACT_NOTHING};
  const uint8_t pre = (uint8_t)((k.n_failed_rf ? DEL_PRE_RETRIEVAL_FAILED : 0) | (n_unready ? DEL_PRE_NOT_READY : 0));
  const bool orphan_all = !(of & DEL_OBJ_POSSIBLE_ORPHAN) && (of & DEL_OBJ_ORPHAN_ALL);
  return DelPlanObj{pre, (uint8_t)(orphan_all ? DEL_ACT_DELETE_HISTORY | DEL_ACT_REMOVE_FINALIZER : 0)};
}
struct DelFinishObj {
  uint8_t status, reason, then;
  bool checked;  // ensureRemovedOrUnmanaged ran
};
// wait = the object's DEL_WAIT_* bits, n_unready / n_unready2 = the unready clusters of the first and the second
// listing, C = the joined clusters. k.n_failed_checks counts the object's failed check rows on ready clusters.
__host__ __device__ __forceinline__ DelFinishObj del_finish_obj(uint8_t of, uint8_t wait, const DelCounts& k, int n_unready,
                                                                int n_unready2, int C) {
  if (!del_walks(of)) return DelFinishObj{DEL_ST_OK, DEL_RSN_NONE, 0, false};
  const uint8_t err_then = del_label_arm(of) ? 0 : DEL_ACT_RECORD_ERROR;  // :771-776 (the label arms only return the error)
  // handleDeletionInClusters' tail (:965-978), then its callers' `!ok` (:813-815, :864-866)
  uint8_t reason = DEL_RSN_NONE;
  if ((wait & DEL_WAIT_TIMED_OUT) && k.n_ops > 0) reason = DEL_RSN_TIMED_OUT;
  else if (k.n_failed_rf) reason = DEL_RSN_RETRIEVAL_FAILED;
  else if (n_unready) reason = DEL_RSN_NOT_READY;
  else if (k.n_failed_ops) reason = DEL_RSN_OPS_FAILED;
  if (reason) return DelFinishObj{DEL_ST_ERROR, reason, err_then, false};
  if (del_label_arm(of)) return DelFinishObj{DEL_ST_OK, DEL_RSN_NONE, 0, false};
  if (k.n_remaining > 0) return DelFinishObj{DEL_ST_RECHECK, DEL_RSN_WAITING, 0, false};  // :867-871, :777-779
  // ensureRemovedOrUnmanaged (:889-919)
  if ((wait & DEL_WAIT_CHECK_TIMED_OUT) && n_unready2 < C) reason = DEL_RSN_CHECK_TIMED_OUT;
  else if (n_unready2) reason = DEL_RSN_CHECK_NOT_READY;
  else if (k.n_failed_checks) reason = DEL_RSN_CHECKS_FAILED;
  if (reason) return DelFinishObj{DEL_ST_ERROR, reason, err_then, true};
  return DelFinishObj{DEL_ST_OK, DEL_RSN_NONE, DEL_ACT_DELETE_HISTORY | DEL_ACT_REMOVE_FINALIZER, true};  // :877-881, :780
}

// The launch decision of one kad_deletion_plan / kad_deletion_finish, taken here and nowhere else
// (kad_deletion*_route_eval / _last_route show it). Group path: a wave is 64 / width lane groups, every group takes
// one object at a time and its lanes stride over the object's entries (observations; for finish the check rows
// after them); the width is the mean entries of a short object over DEL_PER_LANE, rounded up to a power of two in
// [1, 64]. Objects with more than long_min entries go one per wave, four waves a block. Every block keeps the
// clusters' flags, a byte each, in dynamic LDS.
struct DeletionRoute {
  int32_t width, long_min, threads, grid, long_grid, stride, lds;
};
inline DeletionRoute route_deletion(int C, int O, int n_long, int64_t short_items, int n_cu) {
  DeletionRoute r{};
  const int n_short = O - n_long;
  r.width = group_width(short_items, n_short, 1, DEL_PER_LANE);
  r.long_min = DEL_LONG_MIN;
  r.threads = DEL_THREADS;
  r.grid = n_short > 0 ? group_grid(O, r.width, n_cu) : 0;  // 16 KiB of LDS a block at most: 8 blocks a CU fit
  r.long_grid = (n_long + 3) / 4;
  r.stride = group_stride(r.grid, r.width);
  r.lds = (C + 15) / 16 * 16;
  return r;
}

hipError_t launch_deletion(const DeletionDev& d, const DeletionRoute& r, bool finish, hipStream_t st);

}  // namespace kad
