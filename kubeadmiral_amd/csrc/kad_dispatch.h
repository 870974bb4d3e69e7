// kad_dispatch_plan (kad_dispatch.hip): one batch of federated objects against every joined cluster, the decision
// of syncToClusters' cluster loop shared by the device and the host, the launch decision, the launch.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kad {

constexpr int DI_MAX_CLUSTERS = 16384;  // the wave path's per-wave bitmaps: 512 u32 words each at most
constexpr int DI_BITMAPS = 3;           // selected, namespace, observed
constexpr uint8_t DI_CL_READY = 1, DI_CL_TERMINATING = 2, DI_CL_CASCADING = 4, DI_CL_FINALIZER = 8;  // KAD_DISPATCH_CL_*
constexpr uint8_t DI_OBJ_ERROR = 1, DI_OBJ_ORPHAN_ALL = 2, DI_OBJ_ORPHAN_ADOPTED = 4;                // KAD_DISPATCH_OBJ_*
constexpr uint8_t DI_OB_EXISTS = 1, DI_OB_DELETING = 2, DI_OB_ADOPTED = 4, DI_OB_RETRIEVAL_FAILED = 8;  // KAD_DISPATCH_OB_*
constexpr int32_t DI_NS_NONE = -1, DI_NS_UNFEDERATED = -2;                                            // KAD_DISPATCH_NS_*
enum DiOp { DI_OP_NONE, DI_OP_CREATE, DI_OP_UPDATE, DI_OP_DELETE, DI_OP_REMOVE_LABEL };                // KAD_DISPATCH_OP_*
enum DiStatus { DI_ST_NONE, DI_ST_CLUSTER_NOT_READY, DI_ST_CACHED_RETRIEVAL_FAILED, DI_ST_WAITING_FOR_REMOVAL,
                DI_ST_LABEL_REMOVAL_TIMED_OUT, DI_ST_DELETION_TIMED_OUT, DI_ST_CLUSTER_TERMINATING,
                DI_ST_FINALIZER_CHECK_FAILED, DI_ST_CREATION_TIMED_OUT, DI_ST_UPDATE_TIMED_OUT };      // KAD_DISPATCH_ST_*
constexpr uint8_t DI_RES_RECHECK = 1, DI_RES_PLACEMENT_FAILED = 2;                                    // KAD_DISPATCH_RES_*

struct DispatchDev {
  int C, nw;  // joined clusters; u32 bitmap words = ceil(C / 32)
  int O;
  const uint8_t* cluster_flags;              // [C]
  const uint8_t* obj_flags;                  // [O]
  const int32_t* obj_ns;                     // [O]
  const int32_t *obj_pl_off, *pl_cluster;    // [O + 1], entries in [-1, C)
  const int32_t *ns_pl_off, *ns_cluster;     // [N + 1], entries in [-1, C)
  const int32_t *obj_ob_off, *ob_cluster;    // [O + 1], strictly ascending per object, in [0, C)
  const uint8_t* ob_flags;                   // [B]
  const int64_t* out_off;                    // [O + 1]
  int32_t* out_cluster;                      // [out_off[O]]
  uint8_t *out_op, *out_status;              // [out_off[O]]
  int32_t *count, *n_ops, *n_selected;       // [O]
  uint8_t* obj_result;                       // [O]
};

// What syncToClusters does with one (object, joined cluster) pair before anything is dispatched
// (pkg/controllers/sync/controller.go:458-544): cf = the cluster's DI_CL_* bits, sel = the cluster is in the
// computed placement, ob = the observation's DI_OB_* bits (0: the informer holds no target there and the lookup
// did not fail), of = the object's DI_OBJ_* bits. op == DI_OP_NONE and status == DI_ST_NONE: the loop `continue`s
// without recording anything.
struct DiDecision {
  uint8_t op, status, recheck;
};
__host__ __device__ __forceinline__ DiDecision di_decide(uint8_t cf, bool sel, uint8_t ob, uint8_t of) {
  const bool terminating = (cf & DI_CL_TERMINATING) != 0;
  const bool casc = terminating && (cf & DI_CL_CASCADING);  // isCascadingDeletionTriggered (:461)
  const bool del = !sel || casc;                            // shouldBeDeleted (:462)
  if (!(cf & DI_CL_READY))                                  // :464-472
    return DiDecision{DI_OP_NONE, (uint8_t)(del ? DI_ST_NONE : DI_ST_CLUSTER_NOT_READY), 0};
  if (ob & DI_OB_RETRIEVAL_FAILED) return DiDecision{DI_OP_NONE, DI_ST_CACHED_RETRIEVAL_FAILED, 0};  // :481-485
  const bool exists = (ob & DI_OB_EXISTS) != 0;
  if (del) {  // :488-511
    if (!exists) return DiDecision{DI_OP_NONE, DI_ST_NONE, 0};
    if (ob & DI_OB_DELETING) return DiDecision{DI_OP_NONE, DI_ST_WAITING_FOR_REMOVAL, 0};
    if (terminating && !(cf & DI_CL_CASCADING)) return DiDecision{DI_OP_NONE, DI_ST_NONE, 0};
    // deleteFromCluster (:819-844): orphaning is respected under cascading deletion only
    const bool orphan = casc && ((of & DI_OBJ_ORPHAN_ALL) || ((of & DI_OBJ_ORPHAN_ADOPTED) && (ob & DI_OB_ADOPTED)));
    if (orphan) return DiDecision{DI_OP_REMOVE_LABEL, DI_ST_LABEL_REMOVAL_TIMED_OUT, 0};
    return DiDecision{DI_OP_DELETE, DI_ST_DELETION_TIMED_OUT, 0};
  }
  if (terminating) return DiDecision{DI_OP_NONE, DI_ST_CLUSTER_TERMINATING, 0};               // :514-522
  if (!(cf & DI_CL_FINALIZER)) return DiDecision{DI_OP_NONE, DI_ST_FINALIZER_CHECK_FAILED, 1};  // :529-538
  if (!exists) return DiDecision{DI_OP_CREATE, DI_ST_CREATION_TIMED_OUT, 0};                  // :539-540
  return DiDecision{DI_OP_UPDATE, DI_ST_UPDATE_TIMED_OUT, 0};                                 // :541-543
}

// The launch decision of one kad_dispatch_plan, taken here and nowhere else (kad_dispatch_route_eval /
// kad_dispatch_last_route show it): one object per wave at a time, four waves a block, the waves striding over
// the objects; every wave owns three bitmaps of `words` u32 words in dynamic LDS.
struct DispatchRoute {
  int32_t words;    // u32 words per bitmap
  int32_t threads;  // per block
  int32_t grid;     // blocks (0 at O = 0)
  int32_t lds;      // dynamic LDS bytes per block
  int32_t stride;   // objects between two consecutive objects of one wave
};

inline DispatchRoute route_dispatch(int C, int O, int n_cu) {
  DispatchRoute r{};
  r.words = (C + 31) / 32;
  r.threads = 256;
  r.lds = 4 * DI_BITMAPS * r.words * 4;
  // 160 KiB of LDS a CU, at most 8 blocks (32 waves) of them resident
  const int64_t by_lds = r.lds > 0 ? (160 * 1024) / r.lds : 8, per_cu = by_lds < 8 ? by_lds : 8;
  const int64_t want = ((int64_t)O + 3) / 4, cap = (int64_t)n_cu * per_cu;
  r.grid = (int32_t)(want < cap ? want : cap);
  r.stride = r.grid * 4;
  return r;
}

hipError_t launch_dispatch(const DispatchDev& d, const DispatchRoute& r, hipStream_t st);

}  // namespace kad
