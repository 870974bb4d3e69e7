/*
 * kad_sched.h — C ABI of the MI355X-native batch scheduler for KubeAdmiral's
 * scheduling framework (libkad.so).
 *
 * Drop-in boundary. The reference runs, per SchedulingUnit and on one Go
 * goroutine,
 *
 *   core.ScheduleAlgorithm.Schedule(ctx, framework.Framework,
 *       framework.SchedulingUnit, []*FederatedCluster) (ScheduleResult, error)
 *   (pkg/controllers/scheduler/core/generic_scheduler.go:37-44, installed at
 *    pkg/controllers/scheduler/scheduler.go:208, called at scheduler.go:507).
 *
 * This library evaluates the same Filter → Score → Select → Replicas pipeline
 * for a whole batch of SchedulingUnits against one cluster snapshot on the GPU.
 * A cgo shim implements ScheduleAlgorithm on top of it:
 *
 *   kad_snapshot_upload   ← the []*FederatedCluster argument, packed once per
 *                           snapshot version (clusters are read-only informer
 *                           cache objects, generic_scheduler.go:96)
 *   kad_batch_upload      ← a batch of framework.SchedulingUnit values
 *                           (framework/types.go:33-69), packed
 *   kad_schedule          ← genericScheduler.Schedule for every unit
 *                           (generic_scheduler.go:92-150) under the plugin set
 *                           of the framework (kad_profile ← EnabledPlugins,
 *                           pkg/apis/core/types.go:21-43, built by
 *                           scheduler/profile.go:84-113)
 *   kad_results_download  ← ScheduleResult.SuggestedClusters per unit
 *                           (generic_scheduler.go:48-53) + error class
 *
 * Conventions: every function returns 0 on success or a negative KAD_E* code;
 * kad_last_error() gives the message. Inputs are caller-owned host buffers,
 * read only during the call; the library owns all device memory and never
 * keeps caller pointers. A kad_ctx is bound to one HIP device and one HIP
 * stream and is internally serialised (a mutex), so concurrent worker
 * goroutines (worker.go:132-134) may share it.
 *
 * Packed layouts: a snapshot blob and a batch blob are single contiguous byte
 * buffers — a header followed by 256-byte aligned arrays located by byte
 * offsets in the header — so one H2D copy (or one RCCL broadcast) moves them.
 * The host-side packer is kubeadmiral_amd/pack.py; the layout below is the
 * contract a Go packer would reproduce.
 */
#ifndef KAD_SCHED_H
#define KAD_SCHED_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define KAD_ABI_VERSION 2

/* ---------------------------------------------------------------- errors */
#define KAD_OK 0
#define KAD_EINVAL -1       /* malformed blob / profile / argument          */
#define KAD_EHIP -2         /* HIP runtime error (caller falls back)        */
#define KAD_ENOMEM -3       /* device allocation failed                     */
#define KAD_ESTATE -4       /* e.g. schedule before snapshot/batch upload   */
#define KAD_EUNSUPPORTED -5 /* plugin not in the in-tree set (webhook)      */
#define KAD_EHOST -6        /* other host-side failure (e.g. a pool thread could not start) */
#define KAD_ENOSPC -7       /* kad_follower_union: out_capacity is less than the ids to emit */

/* ------------------------------------------------------------- plugins
 * In-tree plugin ids = bit positions in kad_profile masks.
 * Names: pkg/controllers/scheduler/framework/plugins/names/names.go:19-30;
 * registry: pkg/controllers/scheduler/profile.go:39-50.                    */
enum kad_plugin {
  KAD_PL_API_RESOURCES = 0,          /* APIResources                       */
  KAD_PL_TAINT_TOLERATION = 1,       /* TaintToleration (filter + score)   */
  KAD_PL_CLUSTER_RESOURCES_FIT = 2,  /* ClusterResourcesFit                */
  KAD_PL_PLACEMENT_FILTER = 3,       /* PlacementFilter                    */
  KAD_PL_CLUSTER_AFFINITY = 4,       /* ClusterAffinity (filter + score)   */
  KAD_PL_BALANCED_ALLOCATION = 5,    /* ClusterResourcesBalancedAllocation */
  KAD_PL_LEAST_ALLOCATED = 6,        /* ClusterResourcesLeastAllocated     */
  KAD_PL_MOST_ALLOCATED = 7,         /* ClusterResourcesMostAllocated      */
  KAD_PL_MAX_CLUSTER = 8,            /* MaxCluster (select)                */
  KAD_PL_CLUSTER_CAPACITY_WEIGHT = 9 /* ClusterCapacityWeight (replicas)   */
};

/* kad_profile.flags */
#define KAD_PROFILE_XORSHIFT_GO121 (1u << 0) /* pdqsort breakPatterns with the
                                                 13/7/17 xorshift triple instead of go1.19's 13/17/5 */

/* The framework: which in-tree plugin runs at which extension point.
 * Filters are an AND (runtime/framework.go:114-126) and score sums are
 * order-independent (core/generic_scheduler.go:182-190), so masks suffice;
 * only the FIRST select / replicas plugin runs (framework.go:194-207,
 * 234-247). Framework construction errors (unknown / duplicate / wrong-type
 * plugin, framework.go:70-95) are raised by the host before this call.      */
typedef struct kad_profile {
  uint32_t filter_mask;    /* bits of KAD_PL_* filter plugins                  */
  uint32_t score_mask;     /* bits of KAD_PL_* score plugins                   */
  int32_t select_plugin;   /* -1 = none (all feasible selected), KAD_PL_MAX_CLUSTER */
  int32_t replicas_plugin; /* -1 = none, KAD_PL_CLUSTER_CAPACITY_WEIGHT        */
  uint32_t flags;          /* KAD_PROFILE_*                                    */
  uint32_t reserved[3];
} kad_profile;

/* ------------------------------------------------------ snapshot blob
 * C clusters in snapshot order (the order of the []*FederatedCluster slice;
 * MaxCluster's tie behaviour is defined relative to it).
 * Array element [i][c] is stored at i*C + c ("row-major by attribute"), so a
 * wavefront reading 64 consecutive clusters is one coalesced access.        */
#define KAD_SNAPSHOT_MAGIC 0x5344414Bu /* "KADS" */
enum kad_snapshot_array {
  KAD_S_ALLOC_CPU = 0, /* i64[C]  Allocatable cpu MilliValue (framework/util.go:106)      */
  KAD_S_ALLOC_MEM,     /* i64[C]  Allocatable memory Value()                            */
  KAD_S_USED_CPU,      /* i64[C]  (Allocatable − Available) cpu via Resource.Sub
                                  (clusterresources/fit.go:140-147)                      */
  KAD_S_USED_MEM,      /* i64[C]                                                         */
  KAD_S_ALLOC_SCALAR,  /* i64[S][C] scalar resources (IsScalarResourceName) allocatable  */
  KAD_S_USED_SCALAR,   /* i64[S][C] scalar resources used                                */
  KAD_S_ALLOC_CORES,   /* i64[C]  Value() of (0 + Allocatable cpu) (rsp.go:305-325)      */
  KAD_S_AVAIL_CORES,   /* i64[C]  Value() of (0 + Available cpu)   (rsp.go:286-304)      */
  KAD_S_GVK,           /* u64[GW][C] bit g set ⇔ cluster lists APIResource g             */
  KAD_S_TAINT_NSNE,    /* u64[TW][C] taints with effect NoSchedule|NoExecute             */
  KAD_S_TAINT_NE,      /* u64[TW][C] taints with effect NoExecute                        */
  KAD_S_TAINT_PNS,     /* u64[TW][C] PreferNoSchedule taints (one id per occurrence)     */
  KAD_S_LABEL_VAL,     /* i32[K][C] value id of label key k (-1 = absent)                */
  KAD_S_LABEL_INT,     /* i64[K][C] strconv.ParseInt(value,10,64)                        */
  KAD_S_LABEL_INT_OK,  /* u8[K][C]  1 if the parse succeeded                             */
  KAD_S_NAME_FNV,      /* u32[C]  FNV-1 32 state after the cluster name bytes
                                  (util/planner/planner.go:185-195)                      */
  KAD_S_CFLAGS,        /* u32[C]  bit0: Resource.Sub error (map-order dependent input)   */
  KAD_S_NARRAYS
};

typedef struct kad_snapshot_header {
  uint32_t magic;
  uint32_t abi_version;
  int32_t n_clusters;    /* C  */
  int32_t n_gvk_words;   /* GW */
  int32_t n_taint_words; /* TW */
  int32_t n_label_keys;  /* K  */
  int32_t n_scalar;      /* S  */
  int32_t reserved0;
  uint64_t total_bytes;
  uint64_t fingerprint; /* vocabulary fingerprint (cluster names in order and
                           the interned label / taint / API-resource / scalar
                           ids a batch is packed against); batches carry it */
  uint64_t off[KAD_S_NARRAYS];
} kad_snapshot_header;

/* ----------------------------------------------- snapshot delta blob
 * Cluster informer updates (scheduler.go:157-177) that change existing
 * clusters without growing the vocabulary — resources (the common case:
 * status collection), a label to an already-interned value, a known taint —
 * are applied to the resident snapshot in place: the delta carries the
 * changed clusters' columns of every snapshot array, so batches packed
 * against the snapshot stay valid. Anything else (cluster join/leave, a new
 * label value, taint, API resource or scalar name) needs a full upload.
 * Layout: header, i32 idx[n_changed] (snapshot positions, strictly
 * increasing), then for each snapshot array a its rows for the changed
 * clusters, element [r][j] at off[a] + (r*n_changed + j)*elem_size(a), rows
 * and element sizes as in the snapshot (1 / S / GW / TW / K rows).          */
#define KAD_DELTA_MAGIC 0x4441444Bu /* "KADD" */
typedef struct kad_snapshot_delta_header {
  uint32_t magic;
  uint32_t abi_version;
  int32_t n_clusters;   /* must equal the resident snapshot's C            */
  int32_t n_changed;    /* clusters rewritten                              */
  uint64_t total_bytes;
  uint64_t fingerprint; /* must equal the resident snapshot's fingerprint  */
  uint64_t idx_off;     /* i32[n_changed]                                  */
  uint64_t off[KAD_S_NARRAYS];
} kad_snapshot_delta_header;

/* --------------------------------------------------------- batch blob
 * W scheduling units; CSR arrays are indexed by *_OFF[w] .. *_OFF[w+1].    */
#define KAD_BATCH_MAGIC 0x4241444Bu /* "KADB" */

/* per-unit flags (KAD_B_FLAGS) */
#define KAD_W_DUPLICATE (1u << 0)         /* SchedulingMode == Duplicate (generic_scheduler.go:130)  */
#define KAD_W_STICKY (1u << 1)            /* StickyCluster && len(CurrentClusters)>0 (:101-104)      */
#define KAD_W_AVOID_DISRUPTION (1u << 2)  /* AvoidDisruption (planner.go:116-176)                   */
#define KAD_W_KEEP_UNSCHED (1u << 3)      /* AutoMigration.KeepUnschedulableReplicas (rsp.go:128-139)*/
#define KAD_W_HAS_DESIRED (1u << 4)       /* DesiredReplicas != nil                                  */
#define KAD_W_HAS_MAX_CLUSTERS (1u << 5)  /* MaxClusters != nil (max_cluster.go:48-58)               */
#define KAD_W_FIT_NONZERO (1u << 6)       /* fit.go:82-87 early return NOT taken                     */
#define KAD_W_HAS_PLACEMENT (1u << 7)     /* len(ClusterNames) > 0 (placement/filter.go:47)          */
#define KAD_W_SCORE_ERROR (1u << 8)       /* ClusterAffinity.Score errors (cluster_affinity.go:121)  */
#define KAD_W_DYNAMIC_WEIGHTS (1u << 9)   /* len(Weights) == 0 (rsp.go:69)                           */
#define KAD_W_HAS_CURRENT (1u << 10)      /* len(CurrentClusters) > 0                                */
#define KAD_W_WIDE_SCORES (1u << 11)      /* affinity weights may exceed the narrow i32 path         */

enum kad_batch_array {
  KAD_B_FLAGS = 0,     /* u32[W]                                                          */
  KAD_B_GVK,           /* i32[W]  snapshot GVK id of (GroupVersion, Kind); -1 = none has it */
  KAD_B_REQ_CPU,       /* i64[W]  ResourceRequest.MilliCPU                                */
  KAD_B_REQ_MEM,       /* i64[W]  ResourceRequest.Memory                                  */
  KAD_B_DESIRED,       /* i64[W]  *DesiredReplicas (0 when nil)                           */
  KAD_B_MAX_CLUSTERS,  /* i64[W]  *MaxClusters                                            */
  KAD_B_TOLSET,        /* i32[W]  toleration-set id                                       */
  KAD_B_TOL_ALL,       /* u64[NT][TW] taints tolerated by some toleration                 */
  KAD_B_TOL_PNS,       /* u64[NT][TW] ... by a toleration with effect "" or PreferNoSchedule */
  KAD_B_SREQ_OFF,      /* i32[W+1] scalar requests (ScalarResources map)                  */
  KAD_B_SREQ_ID,       /* i32[]    snapshot scalar id (-1: no cluster has it)             */
  KAD_B_SREQ_VAL,      /* i64[]    requested value                                        */
  KAD_B_FPROG_OFF,     /* i32[W+1] ClusterAffinity filter program (see KAD_OP_*)          */
  KAD_B_FPROG,         /* i32[]                                                           */
  KAD_B_SPROG_OFF,     /* i32[W+1] ClusterAffinity score program                          */
  KAD_B_SPROG,         /* i32[]                                                           */
  KAD_B_PLACE_OFF,     /* i32[W+1] ClusterNames as snapshot cluster ids (sorted, unique)  */
  KAD_B_PLACE,         /* i32[]                                                           */
  KAD_B_CUR_OFF,       /* i32[W+1] CurrentClusters as snapshot ids (sorted)               */
  KAD_B_CUR_ID,        /* i32[]                                                           */
  KAD_B_CUR_REP,       /* i64[]    replicas (nil resolved to DesiredReplicas, rsp.go:119-126) */
  KAD_B_PREF_OFF,      /* i32[W+1] per-cluster Weights/MinReplicas/MaxReplicas/EstimatedCapacity */
  KAD_B_PREF_ID,       /* i32[]    snapshot cluster id (sorted)                           */
  KAD_B_PREF_W,        /* i64[]    Weights[cluster]           (i32[]: KAD_BATCH_NARROW_PREFS) */
  KAD_B_PREF_MIN,      /* i64[]    MinReplicas[cluster]       (i32[]: KAD_BATCH_NARROW_PREFS) */
  KAD_B_PREF_MAX,      /* i64[]    MaxReplicas[cluster]       (i32[]: KAD_BATCH_NARROW_PREFS) */
  KAD_B_PREF_CAP,      /* i64[]    EstimatedCapacity[cluster] (only entries >= 0; i32[] narrow) */
  KAD_B_PREF_FLAGS,    /* u32[]    bit0 has weight, bit1 has max, bit2 has cap            */
  KAD_B_KEY_OFF,       /* i32[W+1] su.Key() bytes (types.go:123-128)                      */
  KAD_B_KEY,           /* u8[]                                                            */
  KAD_B_OUT_OFF,       /* i64[W+1] output slot ranges (host-computed upper bounds)        */
  KAD_B_REQ_OFF,       /* i32[NR+1] batch-wide table of distinct label/field requirements */
  KAD_B_REQ,           /* i32[]     requirement words (see KAD_OP_*)                       */
  KAD_B_NARRAYS
};

#define KAD_PREF_HAS_WEIGHT 1u
#define KAD_PREF_HAS_MAX 2u
#define KAD_PREF_HAS_CAP 4u

/* kad_batch_header.flags */
#define KAD_BATCH_NARROW_PREFS 1u /* every value of every unit's Weights, MinReplicas, MaxReplicas and
                                     (AutoMigration units) EstimatedCapacity map fits int32: the four
                                     KAD_B_PREF_{W,MIN,MAX,CAP} columns are i32[] (the packers decide it
                                     from the input maps, so both produce the same bytes)             */

typedef struct kad_batch_header {
  uint32_t magic;
  uint32_t abi_version;
  int32_t n_units;       /* W                                        */
  int32_t n_clusters;    /* must equal the snapshot's C              */
  int32_t n_taint_words; /* must equal the snapshot's TW             */
  int32_t n_tolsets;     /* NT                                       */
  int64_t n_out_slots;   /* = OUT_OFF[W]                             */
  int32_t max_row_slots; /* max_w OUT_OFF[w+1]-OUT_OFF[w]            */
  uint32_t packed_filter_mask;  /* profile the output bounds were sized for:  */
  int32_t packed_select_plugin; /* kad_schedule rejects any other profile     */
  int32_t n_reqs;       /* NR: distinct requirements in KAD_B_REQ                         */
  uint32_t flags;       /* KAD_BATCH_*                                                    */
  uint32_t reserved;    /* 0                                                              */
  uint64_t total_bytes;
  uint64_t snapshot_fingerprint;
  uint64_t off[KAD_B_NARRAYS];
} kad_batch_header;

/* ------------------------------------------------ predicate programs
 * Requirements are interned batch-wide: KAD_B_REQ holds each distinct one
 * once as  [op | n_payload<<8, key, payload...]  (i32 words):
 *   KAD_OP_IN / NOTIN / EQ : payload = value ids of that key (labels.Requirement
 *                            In / NotIn / SelectorFromSet's Equals)
 *   KAD_OP_EXISTS / DNE    : no payload
 *   KAD_OP_GT / LT         : payload = int64 threshold as (lo, hi) words
 *   KAD_OP_NAME_EQ / NE    : key = snapshot cluster id (-1: no such cluster);
 *                            field selector on metadata.name
 *                            (util/clusterselector/util.go:65-93)
 *   KAD_OP_TRUE / FALSE    : folded on the host (key or value absent from
 *                            every cluster, field keys other than metadata.name)
 * The device evaluates every distinct requirement once per cluster into a
 * bitmask row (NR × ⌈C/64⌉ u64); a unit's programs then combine rows with
 * word-wide AND/OR instead of re-evaluating selectors per (unit, cluster) pair
 * as the reference does (clusterselector/util.go:35-58 per call).
 * Filter program (cluster_affinity.go:50-94, clusterselector/util.go:97-132):
 *   n_sel, <n_sel requirement ids: ClusterSelector map>,
 *   req_present, [n_terms, { tflags, n_expr, n_field, <expr ids>, <field ids> } ...]
 *   tflags: bit0 has_expr, bit1 expr_valid, bit2 has_field, bit3 field_valid
 *   (invalid parts carry no requirements; reaching one makes the whole
 *    MatchClusterSelectorTerms return false, as the reference's error does).
 * Score program (cluster_affinity.go:96-135): n_terms, { weight, n_expr, <expr ids> } ...
 *   (only valid, non-empty terms with weight != 0)                           */
enum kad_op {
  KAD_OP_IN = 1, KAD_OP_NOTIN = 2, KAD_OP_EXISTS = 3, KAD_OP_DNE = 4,
  KAD_OP_GT = 5, KAD_OP_LT = 6, KAD_OP_EQ = 7, KAD_OP_TRUE = 8, KAD_OP_FALSE = 9,
  KAD_OP_NAME_EQ = 10, KAD_OP_NAME_NE = 11
};
#define KAD_TERM_HAS_EXPR 1
#define KAD_TERM_EXPR_VALID 2
#define KAD_TERM_HAS_FIELD 4
#define KAD_TERM_FIELD_VALID 8

/* ------------------------------------------------------------ results
 * Per unit: status, count and flags; pairs in the unit's output slot range
 * [OUT_OFF[w], OUT_OFF[w] + count) in ascending cluster id.
 *   Duplicate mode: replicas = -1 (the Go nil pointer).
 *   Divide mode   : replicas > 0 (zero entries are dropped, rsp.go:170-179).
 *   KAD_ST_STICKY : SuggestedClusters = CurrentClusters (host copies it).
 *   KAD_ST_NO_FEASIBLE: SuggestedClusters = nil (generic_scheduler.go:112-114). */
enum kad_status {
  KAD_ST_OK = 0,
  KAD_ST_STICKY = 1,
  KAD_ST_NO_FEASIBLE = 2,
  KAD_ST_ERR_SCORE = 3,    /* "failed to scoreClusters"      */
  KAD_ST_ERR_SELECT = 4,   /* "failed to selectClusters"     */
  KAD_ST_ERR_REPLICAS = 5  /* "failed to do replicaScheduling" */
};
/* result flags */
#define KAD_RF_TIE_STRADDLE 1u  /* MaxCluster cut fell inside a run of equal scores: pdqsort emulated */
#define KAD_RF_REMAINDER_TIE 2u /* AvailableToPercentage remainder had tied recipients (rsp.go:257-270) */
#define KAD_RF_HASH_TIE 4u      /* planner (weight, FNV) tie: reference order is map-order dependent */

typedef struct kad_result_view {
  int32_t* status;      /* [W]           */
  int32_t* count;       /* [W]           */
  uint32_t* flags;      /* [W]           */
  int32_t* cluster;     /* [n_out_slots] */
  int64_t* replicas;    /* [n_out_slots] */
} kad_result_view;

/* ------------------------------------------------------------ context */
typedef struct kad_ctx kad_ctx;

int kad_ctx_create(int hip_device, kad_ctx** out);
int kad_ctx_destroy(kad_ctx* ctx);
const char* kad_last_error(kad_ctx* ctx);
int kad_abi_version(void);

/* snapshot / batch residency (H2D, or D2D from a device buffer e.g. after an
 * RCCL broadcast of the snapshot blob). Allocation happens here, never in
 * kad_schedule.                                                              */
int kad_snapshot_upload(kad_ctx* ctx, const void* blob, size_t nbytes);
int kad_snapshot_upload_device(kad_ctx* ctx, const void* dev_blob, size_t nbytes);
/* Apply a kad_snapshot_delta blob to the resident snapshot (one H2D of the
 * delta + one scatter kernel, ordered on the ctx stream after any schedule
 * already issued). The resident batch stays valid.  ← cluster update events
 * (scheduler.go:157-177) that re-enqueue objects against changed clusters. */
int kad_snapshot_update(kad_ctx* ctx, const void* delta, size_t nbytes);
int kad_batch_upload(kad_ctx* ctx, const void* blob, size_t nbytes);

/* Run the pipeline for the resident batch; asynchronous on the ctx stream. */
int kad_schedule(kad_ctx* ctx, const kad_profile* profile);
int kad_sync(kad_ctx* ctx);
/* Device time of the last kad_schedule, from HIP events on the ctx stream:
 * ms[0] = whole pipeline, ms[1] = filter/score/select kernel, ms[2] = planner. */
int kad_last_timing(kad_ctx* ctx, float ms[3]);
/* Record those events in later kad_schedule calls (default on). Off, the
 * stream carries only the kernels (no marker packets between passes) and
 * kad_last_timing returns KAD_ESTATE.  No reference counterpart (instrumentation). */
int kad_set_timing(kad_ctx* ctx, int on);
/* Per-stage device times of the last kad_schedule run with timing on (n <= 7 entries):
 * ms[0] req_mask_kernel, [1] prep_kernel, [2] the main schedule kernel (lean / wide / full),
 * [3] the defer pass (schedule_kernel), [4] the replica planner, [5] the whole pipeline,
 * [6] the long-feasible-list pass (schedule_row_kernel). No reference counterpart. */
int kad_stage_timing(kad_ctx* ctx, float* ms, int n);
/* Which kernel took how many units in the last kad_schedule (blocks until it is done): out[0] units,
 * [1] the full kernel (defer list), [2] the long-feasible-list kernel, [3] planner rows (Divide units).
 * Measurement only (bench.py's per-kernel byte models). No reference counterpart. */
int kad_path_counts(kad_ctx* ctx, int32_t* out);
/* How the resident snapshot is scheduled (no device work): out[0] its resource class (2 every cluster
 * has 1 <= allocatable and used <= allocatable; 1 some cluster has allocatable 0 or available < 0 — the
 * clusters federatedcluster/util.go:178-214 reports when cordoned / tainted nodes are left out of
 * allocatable —, all below 2^46; 0 otherwise), [1] 1 if the exact-f64 fast path applies (class 2, or class
 * 1 with the filter folded), [2] 1 if the main kernel is schedule_wide_kernel, [3] taint / API filters
 * folded into the static words, [4] the fit threshold rows folded too. Returns KAD_ESTATE without a
 * snapshot. Measurement / tests only. No reference counterpart. */
int kad_snapshot_paths(kad_ctx* ctx, int32_t* out);
/* The kernels a kad_schedule launches and their shapes, as the library's route decision computes them (csrc/
 * kad_route.h route_schedule). No device work and no ctx: in[KAD_ROUTE_IN_FIELDS] is
 *   [0] C, [1] exact-f64 path (kad_snapshot_paths out[1]), [2] fold, [3] fitfold, [4] taint words TW,
 *   [5] some cpu / memory amount < 0 or >= 2^46,
 *   [6] W, [7] some unit has CurrentClusters, [8] no unit has a ResourceRequest, [9] some unit uses a feature
 *   the lean kernel defers, [10] some unit has more than 8 preferred terms,
 *   [11] filter_mask, [12] score_mask,
 *   [13] debug capture requested (kad_debug_scores), [14] a side stream exists, [15] compute units,
 *   [16] KAD_NO_ROWS (0), [17] KAD_ROWS_AFTER (0), [18] KAD_ROWS_NO_INLINE (0), [19] KAD_PREP_WAVE (1),
 *   [20] KAD_WIDE_MIN_NCH (5), [21] KAD_LEAN_BLOCKS_PER_CU (0: the occupancy query's answer) — the tuning
 *   variables of measurement builds, with the defaults every product build runs;
 *   [22] every row table prep_kernel reads or writes starts on a 16-byte boundary (kad_schedule checks the
 *   device pointers; 0 keeps prep_kernel's 8-byte accesses);
 * per_cu / row_per_cu stand for the occupancy queries of the main and the row kernel. out[KAD_ROUTE_FIELDS] is
 *   [0] prep kernel (0 prep_kernel, 1..3 prep_wave_kernel<2..4>, 4 prep_kernel with 16-byte row accesses:
 *   [22] set and a multiple of 4 chunks),
 *   [1] prep_kernel lanes per unit, [2] family (0 lean, 1 wide), [3] the main kernel's variant
 *   (kad_route_variant_name), [4] the row kernel's, [5] the defer pass's, [6] use_rows, [7] early_rows,
 *   [8] may_defer, [9] row kernel placement (0 none, 1 inside the wide kernel, 2 beside it, 3 after the main
 *   kernel), [10] 1 if the defer pass runs, [11] cache_ne, [12] cache_pn, [13] cache_zs, [14] waves per block,
 *   [15] block threads, [16] dynamic LDS bytes, [17] of them per wave, [18] grid, [19] work-queue batch size,
 *   [20] the row kernel's grid (0 unless placement 2 or 3); [18..20] are 0 at W = 0 (prep alone runs then).
 * [15] compute units is the count of the first device the process scheduled on, whichever device ctx is on.
 * kad_last_route: the same record for what the last kad_schedule launched (KAD_ESTATE before one).
 * Measurement / tests only. No reference counterpart. */
#define KAD_ROUTE_IN_FIELDS 23
#define KAD_ROUTE_FIELDS 21
int kad_route_eval(const int32_t* in, int32_t per_cu, int32_t row_per_cu, int32_t* out);
int kad_last_route(kad_ctx* ctx, int32_t* out);
const char* kad_route_variant_name(int32_t variant);
int kad_results_download(kad_ctx* ctx, const kad_result_view* out);
/* Page-locked host memory for the download's (or a batch blob's) buffers, reused across batches: the
 * copies then DMA straight into / out of it (no staging). kad_host_free(NULL) is a no-op. Caller-side
 * plumbing, no reference counterpart. */
int kad_host_alloc(size_t nbytes, void** out);
int kad_host_free(void* p);
/* The same results copied device-to-device into caller DEVICE buffers of the result view's sizes
 * (e.g. the send buffers of an RCCL all-gather of placements across GPUs); blocking. */
int kad_results_copy_device(kad_ctx* ctx, const kad_result_view* dev_out);

/* All in one: upload batch, schedule, download (blocking). */
int kad_schedule_batch(kad_ctx* ctx, const kad_profile* profile, const void* batch_blob, size_t nbytes,
                       const kad_result_view* out);

/* ---------------------------------------------------- multi-GPU group
 * One process driving N GPUs of a node: the reference runs one scheduler process whose --worker-count
 * goroutines call Schedule (worker.go:132-134, scheduler.go:507), and units are independent given the
 * read-only cluster list (scheduler.go:246-309), so a batch splits into N contiguous unit ranges with no
 * exchange while scheduling. A kad_group holds one kad_ctx per listed device (a device may repeat: the
 * members then share it, e.g. tests on one GPU) and one host thread per member, so every member's
 * uploads, launches and copies are issued concurrently.
 *   kad_group_snapshot_upload: H2D to member 0, then device to device to the others (xGMI peer copies);
 *                              each member rebuilds its derived snapshot state on its own device.
 *   kad_group_snapshot_update: the delta applied on every member.
 *   kad_group_batch_upload   : the whole blob validated once; member i takes units
 *                              [unit_lo[i], unit_lo[i+1]) (kad_batch_split) and H2Ds only the blob bytes
 *                              those units read (their per-unit entries, their CSR data, the batch-wide
 *                              tables) into a buffer of the blob's layout.
 *   kad_group_schedule       : every member's pipeline, asynchronous on its stream.
 *   kad_group_results_download: each member writes its units' status / count / flags at unit_lo[i] and
 *                              its slots at slot_lo[i] = OUT_OFF[unit_lo[i]] of the ONE caller view sized
 *                              for the whole batch — the same bytes as one kad_ctx over the whole batch.
 * A kad_group is internally serialised (a mutex), like a kad_ctx. */
typedef struct kad_group kad_group;
int kad_group_create(const int* hip_devices, int n, kad_group** out);
int kad_group_destroy(kad_group* group);
const char* kad_group_last_error(kad_group* group);
int kad_group_size(kad_group* group);
int kad_group_snapshot_upload(kad_group* group, const void* blob, size_t nbytes);
int kad_group_snapshot_update(kad_group* group, const void* delta, size_t nbytes);
int kad_group_batch_upload(kad_group* group, const void* blob, size_t nbytes);
int kad_group_schedule(kad_group* group, const kad_profile* profile);
int kad_group_sync(kad_group* group);
int kad_group_results_download(kad_group* group, const kad_result_view* out);
/* All in one: upload batch, schedule on every member, download (blocking). */
int kad_group_schedule_batch(kad_group* group, const kad_profile* profile, const void* batch_blob, size_t nbytes,
                             const kad_result_view* out);
/* The resident batch's split: unit_lo[n+1], slot_lo[n+1]. */
int kad_group_ranges(kad_group* group, int64_t* unit_lo, int64_t* slot_lo);
/* kad_path_counts summed over the members; kad_set_timing on every member. */
int kad_group_path_counts(kad_group* group, int32_t* out);
int kad_group_set_timing(kad_group* group, int on);
/* Member i's kad_ctx, for per-member instrumentation only (kad_stage_timing, kad_path_counts): it
 * schedules units [unit_lo[i], unit_lo[i+1]) of the group's batch; its own kad_results_download writes
 * them at offset 0. */
int kad_group_member(kad_group* group, int i, kad_ctx** out);
/* Host only (no device): the split kad_group_batch_upload makes of a packed batch blob for n members —
 * unit_lo[i] = W*i/n, slot_lo[i] = OUT_OFF[unit_lo[i]], i = 0..n. */
int kad_batch_split(const void* batch_blob, size_t nbytes, int n, int64_t* unit_lo, int64_t* slot_lo);

/* ---------------------------------------------------- stage entry points
 * The select and planner stages on caller-provided rows, for parity tests of
 * each plugin in isolation (max_cluster_test.go, planner_test.go).          */
/* MaxCluster over rows of scores in input order; out_sel gets, per row, the
 * selected input positions (ascending) in [row_off[r], row_off[r]+out_count[r]). */
int kad_select_rows(kad_ctx* ctx, int n_rows, const int32_t* row_off, const int64_t* scores,
                    const int64_t* max_clusters /* <0: error, INT64_MAX: nil */, uint32_t profile_flags,
                    int32_t* out_count, int32_t* out_sel, int32_t* out_status);

/* planner.Plan over rows: per element name hash (FNV-1 of name‖key), weight,
 * min, max (flags bit1), capacity (flags bit2), current; per row total
 * replicas, avoid_disruption / keep_unschedulable (row_flags bit0 / bit1).
 * Outputs per element plan and overflow.                                    */
int kad_plan_rows(kad_ctx* ctx, int n_rows, const int32_t* row_off, const uint32_t* hash, const int64_t* weight,
                  const int64_t* min_r, const int64_t* max_r, const int64_t* cap, const int64_t* current,
                  const uint32_t* elem_flags, const int64_t* total, const uint32_t* row_flags,
                  int64_t* out_plan, int64_t* out_overflow);

/* Debug: per (unit, cluster) feasibility and total score of the last
 * kad_schedule (feasible: u8[W*C]; total: i64[W*C], meaningful where feasible). */
int kad_debug_scores(kad_ctx* ctx, const kad_profile* profile, uint8_t* feasible, int64_t* total);

/* ------------------------------------------------------ filter diagnosis
 * Why a unit got no cluster. findClustersThatFitWorkload logs, per cluster, the reason of the filter
 * plugin that rejected it (core/generic_scheduler.go:161-166); that plugin is the first one in the
 * framework's filter order whose Filter does not succeed (RunFilterPlugins,
 * framework/runtime/framework.go:114-126). kad_profile keeps the filters as a mask, so the order is an
 * argument here: filter_order lists the KAD_PL_* ids of the filter plugins in framework order
 * (EnabledPlugins.FilterPlugins) and must be a permutation of the bits of profile->filter_mask.
 * For each listed unit of the resident batch (unit_idx entries in [0, W), any order, repeats allowed; row i
 * of every output belongs to unit_idx[i]) the call reports how many clusters each plugin rejected, how many
 * passed every filter, which resources ClusterResourcesFit found short (fitsRequest collects all of them,
 * clusterresources/fit.go:73-134, so the three counts may overlap) and, optionally, the rejecting plugin
 * per cluster. Sticky units are not filtered (generic_scheduler.go:101-104): zero counts, feasible = -1.
 * The profile must be the one the batch was packed for, as for kad_schedule. Works before or after
 * kad_schedule on the resident snapshot and batch (it rebuilds the requirement rows itself) and leaves the
 * last results, the timings and any later kad_schedule as they were. Runs on the ctx stream; blocks until
 * the outputs are in the caller's buffers. Typical use: after a schedule, over the KAD_ST_NO_FEASIBLE
 * units only. Members of a kad_group: through kad_group_member (unit indices within the member's shard). */
typedef struct kad_explain_view {
  int32_t* rejected;    /* [n][5]  by KAD_PL_* id 0..4: clusters whose first failing filter is that plugin */
  int32_t* feasible;    /* [n]     clusters passing every enabled filter; -1 = sticky unit, not filtered */
  int32_t* fit_detail;  /* [n][3]  cpu, memory, any scalar — among rejected[.][FIT]; may be NULL */
  uint8_t* first_fail;  /* [n][C]  plugin id or 0xFF (passed, or a sticky unit); may be NULL */
} kad_explain_view;
int kad_explain(kad_ctx* ctx, const kad_profile* profile, const int32_t* filter_order, int n_order,
                const int32_t* unit_idx, int n_units, const kad_explain_view* out);
/* Device time of the last kad_explain that launched (n_units > 0), from HIP events on the ctx stream:
 * ms[0] = the requirement rows' rebuild, ms[1] = filter_explain_kernel. No reference counterpart. */
int kad_explain_timing(kad_ctx* ctx, float ms[2]);

/* ------------------------------------------------------ override policies
 * The controller that runs after the scheduler on every federated object is the override-policy controller
 * (pkg/controllers/override/overridepolicy_controller.go:254-376). Per object it looks up at most two
 * policies (the ClusterOverridePolicy, then the OverridePolicy: lookForMatchedPolicies, override/util.go:45-97)
 * and, for every placed cluster and every override rule, asks isClusterMatched (util.go:154-221) whether the
 * rule's TargetClusters select the cluster (parseOverrides, util.go:99-140). That is the (object, cluster)
 * selector evaluation of ClusterAffinity again, so the same requirement rows serve it: the policies' distinct
 * requirements are evaluated once per cluster, each rule becomes two cluster rows (matches, errors), and a
 * batch of objects only gathers bits of those rows at its placed clusters.
 *
 * isClusterMatched per rule and cluster, an AND with this short-circuit:
 *   TargetClusters == nil          matches every cluster;
 *   Clusters                       empty: any cluster; else the name must be listed (a miss is false, no error,
 *                                  whatever the selector below looks like);
 *   ClusterSelector                metav1.LabelSelectorAsSelector{MatchLabels}: validates keys and values (an
 *                                  invalid map is an ERROR, unlike the scheduler's SelectorFromSet), else an AND
 *                                  of equals;
 *   ClusterAffinity                empty: any cluster; else MatchClusterSelectorTerms
 *                                  (clusterselector/util.go:97-132), whose errors (invalid expressions or fields of
 *                                  a term that the cluster reaches) are ERRORS here, not "false".
 * parseOverrides fails for an object iff some (placed cluster, rule) pair errors, or a rule that matches a placed
 * cluster carries a JSON-patch value that does not unmarshal (util.go:125-131, 223-240).
 *
 * Policy-set blob (packed against one snapshot, kubeadmiral_amd/overrides.py PolicySet): P policies, policy p's
 * rules are [POL_RULE_OFF[p], POL_RULE_OFF[p+1]) of the R rules; requirements are interned set-wide and
 * encoded exactly as KAD_B_REQ; a rule's target program has the filter-program format above
 * (n_sel, selector ids, req_present, [n_terms, terms with KAD_TERM_* flags]); an invalid selector carries no
 * requirements (KAD_OVR_SEL_INVALID).                                                                      */
#define KAD_OVERRIDE_MAGIC 0x4F44414Bu /* "KADO" */
enum kad_override_array {
  KAD_O_POL_RULE_OFF = 0, /* i32[P+1]                                                         */
  KAD_O_RULE_FLAGS,       /* u32[R]   KAD_OVR_*                                               */
  KAD_O_RULE_NAME_OFF,    /* i32[R+1] TargetClusters.Clusters as snapshot ids                 */
  KAD_O_RULE_NAME,        /* i32[]    sorted, unique; names the snapshot lacks are dropped    */
  KAD_O_RULE_PROG_OFF,    /* i32[R+1]                                                         */
  KAD_O_RULE_PROG,        /* i32[]    target programs                                         */
  KAD_O_REQ_OFF,          /* i32[NR+1]                                                        */
  KAD_O_REQ,              /* i32[]    requirement words (KAD_OP_*)                            */
  KAD_O_NARRAYS
};
#define KAD_OVR_HAS_TARGET 1u  /* TargetClusters != nil                                              */
#define KAD_OVR_HAS_NAMES 2u   /* len(Clusters) > 0 (a list whose names are all unknown matches nothing) */
#define KAD_OVR_SEL_INVALID 4u /* LabelSelectorAsSelector(ClusterSelector) returns an error          */
#define KAD_OVR_BAD_VALUE 8u   /* some JsonPatch value (non-empty raw bytes) does not unmarshal      */
typedef struct kad_override_header {
  uint32_t magic;
  uint32_t abi_version;
  int32_t n_policies; /* P  */
  int32_t n_rules;    /* R  */
  int32_t n_reqs;     /* NR */
  int32_t n_clusters; /* must equal the snapshot's C */
  uint64_t total_bytes;
  uint64_t snapshot_fingerprint;
  uint64_t off[KAD_O_NARRAYS];
} kad_override_header;

/* Validates every offset, id and program length (KAD_EINVAL), then keeps the set resident. Needs a resident
 * snapshot with the blob's fingerprint. kad_snapshot_update keeps the set (its rows are rebuilt from the
 * snapshot's current labels by every kad_override_match); kad_snapshot_upload drops it, as it drops the batch. */
int kad_override_policies_upload(kad_ctx* ctx, const void* blob, size_t nbytes);
/* Host only (no device): the same validation against the header of a packed snapshot blob. */
int kad_override_policies_check(const void* blob, size_t nbytes, const void* snapshot_blob, size_t snapshot_nbytes);

/* A batch of objects. obj_policy[i][0] is object i's ClusterOverridePolicy and [i][1] its OverridePolicy, as
 * indices into the uploaded set (-1: none); the object's rule list is the first policy's rules followed by the
 * second's. Placed clusters: place_off / place_cluster (snapshot ids, unique per object, any order; -1 = a
 * name the snapshot does not know: matches nothing, errors nothing), or place_off == NULL: the resident
 * results of the last kad_schedule (KAD_ESTATE if nothing was scheduled), n_objects = the resident batch's
 * units, object i = unit i. Then the slot space is the batch's output slots followed by its KAD_B_CUR_ID
 * entries: unit i's placed clusters are slots [OUT_OFF[i], OUT_OFF[i] + count[i]) when its status is KAD_ST_OK,
 * slots n_out_slots + [CUR_OFF[i], CUR_OFF[i+1]) when it is sticky (KAD_ST_STICKY), none otherwise
 * (KAD_ST_NO_FEASIBLE, errors); n_slots = n_out_slots + CUR_OFF[W] (a kad_group member: of its shard).     */
typedef struct kad_override_batch {
  int32_t n_objects;
  int32_t rule_words;           /* RW: u32 words per slot row; every object's rule count must be <= 32*RW */
  const int32_t* obj_policy;    /* [n_objects][2] */
  const int32_t* place_off;     /* [n_objects + 1] or NULL */
  const int32_t* place_cluster; /* [place_off[n_objects]] */
} kad_override_batch;
typedef struct kad_override_view {
  int32_t* status;   /* [n_objects] 0 = OK, 1 = the first policy failed, 2 = the second policy failed      */
  uint32_t* matched; /* [n_slots][RW] bit j: rule j of the object's rule list matches the slot's cluster;
                        all zero for failed objects and for slots that hold no placed cluster            */
} kad_override_view;
/* Runs on the ctx stream (requirement rows of the set, override_rule_rows_kernel, override_status_kernel +
 * override_match_kernel: kad_override.hip); blocks until the outputs are in the caller's buffers. Leaves the
 * last results, the timings and any later kad_schedule as they were, like kad_explain. Members of a
 * kad_group: through kad_group_member (objects = the member's shard of units). */
int kad_override_match(kad_ctx* ctx, const kad_override_batch* batch, const kad_override_view* out);
/* Device time of the last kad_override_match that launched, from HIP events: ms[0] = the set's requirement
 * rows, ms[1] = the rule rows, ms[2] = the status + match kernels. No reference counterpart. */
int kad_override_timing(kad_ctx* ctx, float ms[3]);

/* ------------------------------------------------------ follower scheduling
 * The third consumer of the placements is the follower controller (pkg/controllers/follower/controller.go):
 * for every ConfigMap, Secret, PVC, ServiceAccount, Service and Ingress that workloads reference
 * (supportedFollowerTypes, controller.go:80-87) it sets the follower's placement to the union of
 * ClusterNameUnion() (pkg/apis/types/v1alpha1/extensions_placements.go:24-33) over its leaders
 * (updateFollower / leaderPlacementUnion, controller.go:380-421, 532-550) through SetPlacementNames
 * (extensions_placements.go:78-103), whose hasChange decides whether the follower object is updated.
 * kad_follower_union computes, for a batch of followers, that union, hasChange against the placement the
 * follower holds now, and the union's members in ascending id order for the followers that change.
 *
 * Id space: n_ids cluster ids — the resident snapshot's C clusters (id = snapshot position) followed by names
 * the caller interned itself, because a leader may still hold a placement on a cluster that left the snapshot
 * and the reference unions it by name. C <= n_ids <= 131072, else KAD_EINVAL. -1 is not an id here.
 *
 * Leaders, n_leaders of them; a leader's set is ClusterNameUnion() of the object as it stands after this
 * reconcile:
 *   explicit (lead_off != NULL): lead_off[n_leaders + 1] / lead_cluster, any order, duplicates allowed;
 *   resident (lead_off == NULL): leader i < W is unit i of the last kad_schedule (KAD_ESTATE if nothing was
 *     scheduled; W = the resident batch's units, n_leaders >= W, leaders from W on have only keep_* entries).
 *     The slot rules are kad_override_match's: status KAD_ST_OK gives the unit's count output slots,
 *     KAD_ST_STICKY its KAD_B_CUR_ID entries (current clusters outside the snapshot are not in that array:
 *     the caller, who holds the names, passes them in keep_*), KAD_ST_NO_FEASIBLE nothing. For a unit whose
 *     status is an error class nothing is applied to the object (scheduler.go:505-517), so the leader keeps
 *     its current scheduler placement: sched_off[W + 1] / sched_cluster (NULL: none), the CSR
 *     kad_result_state.place_* describes, read ONLY for error-status units.
 *   keep_off[n_leaders + 1] / keep_cluster (NULL: empty), both modes: always unioned in — the placements other
 *     controllers keep on the leader object.
 * Followers, n_followers of them: fol_off[F + 1] / fol_leader are indices into the leaders; -1 is a leader
 * absent from the store, skipped (controller.go:541-543); a leader may repeat. cur_off[F + 1] / cur_cluster
 * are the follower-controller placement the follower object holds now (duplicates allowed) and cur_has[F]
 * says whether that placement entry exists; cur_has[i] = 0 with a non-empty range is KAD_EINVAL (an entry that
 * does not exist holds no clusters; an entry that exists may be empty).
 *
 * Outputs: changed[F] is exactly SetPlacementNames' hasChange — an empty union gives cur_has
 * (DeletePlacement), otherwise inequality of the union and cur_cluster as sets; count[F] = |union|;
 * out_off[F + 1] and out_cluster hold the union in ascending id order for changed followers only (unchanged
 * ones occupy zero slots), or for every follower with KAD_FOL_EMIT_ALL; the offsets come from a device scan.
 * out_cluster has out_capacity elements: if out_off[F] exceeds it the call returns KAD_ENOSPC with nothing
 * written to out_cluster and changed / count / out_off valid, and the caller retries with out_off[F] slots.
 *
 * Every offset array (monotone from 0), id and leader index is validated on the host before anything is
 * launched (KAD_EINVAL). Runs on the ctx stream (follower_union_*_kernel, the offset scan,
 * follower_emit_*_kernel: kad_follower.hip); blocks until the outputs are in the caller's buffers. Leaves the
 * last results, the timings and any later kad_schedule as they were, like kad_explain. A kad_group member
 * accepts explicit mode only: resident mode there is KAD_EUNSUPPORTED, because a follower's leaders may live
 * in other members' shards. */
#define KAD_FOL_EMIT_ALL 1u
typedef struct kad_follower_batch {
  int32_t n_ids;
  int32_t n_leaders;
  int32_t n_followers; /* F */
  uint32_t flags;      /* KAD_FOL_* */
  const int32_t* lead_off;      /* [n_leaders + 1] or NULL (resident mode) */
  const int32_t* lead_cluster;  /* [lead_off[n_leaders]] */
  const int32_t* sched_off;     /* resident mode: [W + 1] or NULL */
  const int32_t* sched_cluster; /* [sched_off[W]] */
  const int32_t* keep_off;      /* [n_leaders + 1] or NULL */
  const int32_t* keep_cluster;  /* [keep_off[n_leaders]] */
  const int32_t* fol_off;       /* [F + 1] */
  const int32_t* fol_leader;    /* [fol_off[F]] */
  const int32_t* cur_off;       /* [F + 1] */
  const int32_t* cur_cluster;   /* [cur_off[F]] */
  const uint8_t* cur_has;       /* [F] */
  int64_t out_capacity;         /* elements of out_cluster */
} kad_follower_batch;
typedef struct kad_follower_view {
  uint8_t* changed;     /* [F] */
  int32_t* count;       /* [F] */
  int64_t* out_off;     /* [F + 1] */
  int32_t* out_cluster; /* [out_capacity]; may be NULL at capacity 0 */
} kad_follower_view;
int kad_follower_union(kad_ctx* ctx, const kad_follower_batch* batch, const kad_follower_view* out);
/* Host only (no device, no ctx): the same validation against a snapshot of n_clusters clusters and, for a
 * resident-mode batch, a resident batch of n_units units (n_units < 0: nothing scheduled, KAD_ESTATE). */
int kad_follower_check(const kad_follower_batch* batch, const kad_follower_view* out, int32_t n_clusters,
                       int32_t n_units);
/* Device time of the last kad_follower_union that launched (n_followers > 0), from HIP events: ms[0] = the
 * union / compare kernel, ms[1] = the offset scan + the emit kernel. No reference counterpart. */
int kad_follower_timing(kad_ctx* ctx, float ms[2]);
/* What a kad_follower_union launches, as the library's one decision computes it (csrc/kad_follower.h
 * route_follower; no device work, no ctx): out[KAD_FOL_ROUTE_FIELDS] is [0] path (0: one follower per wave
 * at a time, n_ids <= 8192; 1: one per 256-thread block), [1] u32 words per bitmap, [2] block threads,
 * [3] grid of the union and the emit kernel, [4] static LDS bytes per block, [5] the distance between two
 * consecutive followers of one wave (path 0) or block (path 1). kad_follower_last_route: the same record for
 * the last kad_follower_union that launched (KAD_ESTATE before one). Measurement / tests only. */
#define KAD_FOL_ROUTE_FIELDS 6
int kad_follower_route_eval(int32_t n_ids, int32_t n_followers, int32_t n_cu, int32_t* out);
int kad_follower_last_route(kad_ctx* ctx, int32_t* out);

/* ------------------------------------------------------ auto-migration
 * The producer of kubeadmiral.io/auto-migration-info is the auto-migration controller
 * (pkg/controllers/automigration/controller.go:178-378, util.go:29-64): for every object that carries the
 * scheduler's pod-unschedulable-threshold annotation it walks the pods of every member cluster, counts those
 * that have been unschedulable for longer than the threshold, and writes the clusters whose estimated capacity
 * falls short of the desired replicas. kad_migrate_estimate does that for a batch of objects.
 *
 * Times are int64 Unix nanoseconds. The batch carries ONE now_ns (the reference calls time.Now() per
 * cluster: a declared deviation). 0 <= now_ns <= 2^61, |obj_threshold_ns| <= 2^61 and |pod_t_ns| <= 2^61, else
 * KAD_EINVAL: then (t + threshold) - now cannot overflow and Go's saturating Time.Sub never engages.
 *
 * Objects, n_objects of them (only objects with a parseable threshold annotation; the disabled case,
 * controller.go:217-224, stays with the caller): obj_seg_off[O + 1] are the object's segments, one per member
 * cluster object (controller.go:303), obj_threshold_ns[O] the threshold.
 * Segments, n_segments: seg_cluster[S] is an id of the kad_follower_union id space (the snapshot's C clusters,
 * then names the caller interned; C <= n_ids <= 131072), strictly ascending within an object; seg_desired[S]
 * is getDesiredReplicas (controller.go:406-415); seg_pod_off[S + 1] the segment's pods (at most 2^31 - 1).
 * seg_flags[S]: KAD_MIG_SEG_SKIP for a segment the reference leaves before it counts — totalReplicas ==
 * readyReplicas with no error (:310-314), getDesiredReplicas failed (:316-320), the pod listing failed
 * (:323-330) — which contributes no entry and nothing to retry_after, and whose pods, if any, are not read;
 * KAD_MIG_SEG_BACKOFF (only with SKIP) when the listing failed with clusterNeedsBackoff.
 * Pods, n_pods: pod_t_ns[P] is lastTransitionTime of the first PodScheduled condition; pod_flags[P]:
 * KAD_MIG_POD_DELETING (a deletion timestamp: skipped, util.go:35-37, but counted in len(pods)),
 * KAD_MIG_POD_UNSCHED (that condition exists with Status False and Reason Unschedulable, util.go:47-51),
 * KAD_MIG_POD_TZERO (lastTransitionTime absent or null: Go's zero time, which Unix nanoseconds cannot hold;
 * the pod always counts as crossed and pod_t_ns is not read).
 * The existing annotation: old_off[O + 1] / old_cluster (strictly ascending within an object) / old_cap, n_old
 * = old_off[O] entries; an annotation that is absent, null, or does not unmarshal (:239-245) is an empty range.
 *
 * Outputs, per segment: uns[S] = the unschedulable count, next_cross[S] = nextCrossIn (INT64_MAX: none), cap[S]
 * = the estimated capacity written for the cluster (-1: no entry; n >= desired ? n - uns : desired - uns, no
 * entry at cap >= desired, clamped at 0, controller.go:345-366); a skipped segment gives 0, INT64_MAX, -1. Per
 * object: n_written[O] entries, retry_after[O] = the minimum next_cross (INT64_MAX: none), backoff[O] (the
 * worker result is nil iff neither, :369-377), and changed[O] = !equality.Semantic.DeepEqual(existing, new)
 * (:247; nil and empty maps are equal).
 *
 * Every offset array (monotone from 0, ending at its count), id, ascending rule, flag and time is validated on
 * the host before anything is launched (KAD_EINVAL). Runs on the ctx stream (migrate_segment_kernel,
 * migrate_object_kernel: kad_migrate.hip); blocks until the outputs are in the caller's buffers. Needs a
 * snapshot only for C; reads no resident state, so a kad_group member accepts it. Leaves the last results,
 * the timings and any later kad_schedule as they were, like kad_explain. n_objects == 0 returns 0 without
 * launching. */
#define KAD_MIG_SEG_SKIP 1u
#define KAD_MIG_SEG_BACKOFF 2u
#define KAD_MIG_POD_DELETING 1u
#define KAD_MIG_POD_UNSCHED 2u
#define KAD_MIG_POD_TZERO 4u
#define KAD_MIG_TIME_MAX (1ll << 61)
typedef struct kad_migrate_batch {
  int32_t n_ids;
  int32_t n_objects;  /* O */
  int32_t n_segments; /* S */
  int32_t n_old;      /* entries of the existing annotations = old_off[O] */
  int64_t n_pods;     /* P */
  int64_t now_ns;
  const int32_t* obj_seg_off;      /* [O + 1] */
  const int64_t* obj_threshold_ns; /* [O] */
  const int32_t* seg_cluster;      /* [S] */
  const int64_t* seg_desired;      /* [S] */
  const uint8_t* seg_flags;        /* [S] KAD_MIG_SEG_* */
  const int64_t* seg_pod_off;      /* [S + 1] */
  const int64_t* pod_t_ns;         /* [P] */
  const uint8_t* pod_flags;        /* [P] KAD_MIG_POD_* */
  const int32_t* old_off;          /* [O + 1] */
  const int32_t* old_cluster;      /* [n_old] */
  const int64_t* old_cap;          /* [n_old] */
} kad_migrate_batch;
typedef struct kad_migrate_view {
  int32_t* uns;         /* [S] */
  int64_t* next_cross;  /* [S] */
  int64_t* cap;         /* [S] */
  uint8_t* changed;     /* [O] */
  int32_t* n_written;   /* [O] */
  int64_t* retry_after; /* [O] */
  uint8_t* backoff;     /* [O] */
} kad_migrate_view;
int kad_migrate_estimate(kad_ctx* ctx, const kad_migrate_batch* batch, const kad_migrate_view* out);
/* Host only (no device, no ctx): the same validation against a snapshot of n_clusters clusters. */
int kad_migrate_check(const kad_migrate_batch* batch, const kad_migrate_view* out, int32_t n_clusters);
/* Device time of the last kad_migrate_estimate that launched, from HIP events: ms[0] = migrate_segment_kernel,
 * ms[1] = migrate_object_kernel. No reference counterpart. */
int kad_migrate_timing(kad_ctx* ctx, float ms[2]);
/* What a kad_migrate_estimate launches, as the library's one decision computes it (csrc/kad_migrate.h
 * route_migrate; no device work, no ctx) for n_segments segments holding n_pods pods, n_long of them longer
 * than the route's long_min, in n_objects objects: out[KAD_MIG_ROUTE_FIELDS] is [0] the lanes per segment of
 * the group path (a power of two in [8, 64] from the mean segment length), [1] long_min (a segment with MORE
 * pods takes one 256-thread block), [2] block threads, [3] blocks of the group path, [4] blocks of the long
 * path, [5] the distance between two consecutive segments of one lane group, [6] the lanes per object of the
 * object kernel, [7] its blocks. kad_migrate_last_route: the same record for the last kad_migrate_estimate
 * that launched (KAD_ESTATE before one). force_width / force_long_min of kad_migrate_debug_route (0: the
 * route's own) replace [0] and [1] for the following calls on this ctx. Measurement / tests only. */
#define KAD_MIG_ROUTE_FIELDS 8
int kad_migrate_route_eval(int32_t n_segments, int64_t n_pods, int32_t n_long, int32_t n_objects, int32_t n_cu,
                           int32_t* out);
int kad_migrate_last_route(kad_ctx* ctx, int32_t* out);
int kad_migrate_debug_route(kad_ctx* ctx, int32_t force_width, int32_t force_long_min);

/* ------------------------------------------------------ cluster status
 * The producer of a FederatedCluster's status.resources is the federated-cluster controller
 * (pkg/controllers/federatedcluster/clusterstatus.go:162-202, util.go:113-214): every collection interval and per
 * ready member cluster, Allocatable = the per-name sum of status.allocatable over the schedulable nodes, Available
 * = Allocatable minus the requests of every pod whose phase is not Succeeded or Failed, schedulableNodes = the
 * count. kad_cluster_resources does that for a batch of member clusters.
 *
 * Quantities are int64 at one decimal scale per resource name, which the caller chooses (the device never
 * sees it). n_res resource names R, 1 <= R <= 64; the caller leaves the name "pods" out of the node entries
 * (util.go:192), after which pod entries naming it are ignored by the presence rule.
 * Nodes: cl_node_off[K + 1] are a cluster's nodes; node_flags[N]: KAD_CS_NODE_SCHEDULABLE where isNodeSchedulable
 * (util.go:114-132) holds; node_ent_off[N + 1] a node's entries (nent_res[EN] < R, nent_val[EN]), one per name
 * of its status.allocatable.
 * Pods: cl_pod_off[K + 1]; pod_flags[P]: KAD_CS_POD_TERMINAL for phase Succeeded / Failed; pod_ent_off[P + 1] a
 * pod's entries (pent_res[EP] < R, pent_kind[EP]: 0 a container's request, 1 an init container's, 2 the
 * overhead's; pent_val[EP]), ascending by (res, kind) within the pod, several of one (res, kind) allowed. The
 * pod's request for a name is max(sum of kind 0, every kind 1) + sum of kind 2 (getPodResourceRequests,
 * util.go:155-173, under values >= 0).
 * Domain: every value >= 0; max nent_val x the most node entries of one cluster <= 2^62, and the same for pod
 * entries: no sum can wrap. Anything else is KAD_EINVAL (the caller computes such clusters on the host).
 *
 * Outputs, cluster-major: alloc[K * R], avail[K * R] (may be negative), has[K] (bit r: some schedulable node of
 * the cluster lists name r, even with value 0; where it is clear alloc and avail are 0 and requests for r are
 * ignored), sched_nodes[K].
 *
 * Every offset array, resource id, kind, order rule, flag and the domain is validated on the host before
 * anything is launched (KAD_EINVAL). Runs on the ctx stream (cstat_node_kernel, cstat_pod_kernel,
 * cstat_combine_kernel: kad_cstat.hip); blocks until the outputs are in the caller's buffers. Needs no snapshot
 * and reads no resident state, so a kad_group member accepts it. Leaves the last results, the timings and any
 * later kad_schedule as they were. n_clusters == 0 returns 0 without launching. */
#define KAD_CS_NODE_SCHEDULABLE 1u
#define KAD_CS_POD_TERMINAL 1u
#define KAD_CS_VALUE_BOUND (1ll << 62)
typedef struct kad_cstat_batch {
  int32_t n_clusters;  /* K */
  int32_t n_res;       /* R */
  int64_t n_nodes;     /* N */
  int64_t n_pods;      /* P */
  int64_t n_node_ents; /* EN */
  int64_t n_pod_ents;  /* EP */
  const int64_t* cl_node_off;  /* [K + 1] */
  const uint8_t* node_flags;   /* [N] KAD_CS_NODE_* */
  const int64_t* node_ent_off; /* [N + 1] */
  const uint8_t* nent_res;     /* [EN] */
  const int64_t* nent_val;     /* [EN] */
  const int64_t* cl_pod_off;   /* [K + 1] */
  const uint8_t* pod_flags;    /* [P] KAD_CS_POD_* */
  const int64_t* pod_ent_off;  /* [P + 1] */
  const uint8_t* pent_res;     /* [EP] */
  const uint8_t* pent_kind;    /* [EP] 0 container, 1 init container, 2 overhead */
  const int64_t* pent_val;     /* [EP] */
} kad_cstat_batch;
typedef struct kad_cstat_view {
  int64_t* alloc;       /* [K * R] */
  int64_t* avail;       /* [K * R] */
  uint64_t* has;        /* [K] */
  int64_t* sched_nodes; /* [K] */
} kad_cstat_view;
int kad_cluster_resources(kad_ctx* ctx, const kad_cstat_batch* batch, const kad_cstat_view* out);
/* Host only (no device, no ctx): the same validation. */
int kad_cstat_check(const kad_cstat_batch* batch, const kad_cstat_view* out);
/* Device time of the last kad_cluster_resources that launched, from HIP events: ms[0] = cstat_node_kernel,
 * ms[1] = cstat_pod_kernel + cstat_combine_kernel. No reference counterpart. */
int kad_cstat_timing(kad_ctx* ctx, float ms[2]);
/* What a kad_cluster_resources launches, as the library's one decision computes it (csrc/kad_cstat.h
 * route_cstat; no device work, no ctx) for n_clusters clusters, n_long of them with more entries (node + pod)
 * than the route's long_min, the others holding short_nodes nodes and short_pods pods, and n_chunks blocks of
 * the long clusters' pods: out[KAD_CS_ROUTE_FIELDS] is [0] / [1] the lanes per cluster of the node / pod pass's
 * group path (a power of two in [8, 64] from the mean nodes / pods per short cluster / 8), [2] long_min, [3]
 * block threads, [4] / [5] blocks of the node / pod pass's group path, [6] blocks of the node pass's long path
 * (one per long cluster), [7] blocks of the pod pass's long path (one per chunk). kad_cstat_last_route: the same
 * record for the last kad_cluster_resources that launched (KAD_ESTATE before one). force_width /
 * force_long_min of kad_cstat_debug_route (0: the route's own) replace [0], [1] and [2] for the following calls
 * on this ctx. Measurement / tests only. */
#define KAD_CS_ROUTE_FIELDS 8
int kad_cstat_route_eval(int32_t n_clusters, int32_t n_long, int64_t short_nodes, int64_t short_pods, int32_t n_chunks,
                         int32_t n_cu, int32_t* out);
int kad_cstat_last_route(kad_ctx* ctx, int32_t* out);
int kad_cstat_debug_route(kad_ctx* ctx, int32_t force_width, int32_t force_long_min);

/* ------------------------------------------------------ status aggregation
 * The status aggregator (pkg/controllers/statusaggregator/controller.go:249-348) folds, per source object and on
 * every member-object event, the statuses of the object's copies in the member clusters into the source
 * object's status. kad_status_aggregate does the numeric part of its Deployment plugin (plugins/
 * deployment.go:42-186) or its Job plugin (plugins/job.go:43-163) for a batch of source objects of one kind,
 * and compares the result with each object's old status.
 *
 * kind: KAD_SAGG_DEPLOYMENT or KAD_SAGG_JOB. obj_seg_off[O + 1] are an object's segments, one per member cluster
 * that holds a copy (the order within an object does not matter).
 * Per object: obj_flags[O]: KAD_SAGG_OBJ_UPTODATE = clusterObjsUpToDate (propagationstatus.IsResourcePropagated);
 * KAD_SAGG_OBJ_ERROR = the caller found an object-level error (a member's status missing, not a map or not
 * convertible): every output of the object is 0, changed included, and its segments are not read;
 * KAD_SAGG_OBJ_OLD_OTHER = the old status can never compare equal (another key, an explicit zero, a value that
 * is not an integer): changed is 1. obj_generation[O] = metadata.generation and obj_observed[O] = the current
 * status.observedGeneration (Deployment only; null for a Job). old_vals[NOLD][O], row-major, the old status with
 * an absent key as 0: Deployment NOLD = 6: replicas, updatedReplicas, readyReplicas, availableReplicas,
 * unavailableReplicas, observedGeneration; Job NOLD = 5: active, succeeded, failed, startTime (INT64_MAX: none),
 * completionTime (INT64_MIN: none).
 * Per segment: seg_vals[NV][S], row-major int32: Deployment NV = 5 (the five replica counts in the order above),
 * Job NV = 3 (active, succeeded, failed). seg_flags[S]: KAD_SAGG_SEG_NIL = the member's status is nil (skipped;
 * it clears the Deployment's observed-generation flag and still counts as a member of the Job);
 * Deployment: KAD_SAGG_SEG_SYNCED = the cluster is listed in fedObject.status.clusters, with seg_synced[S] its
 * generation there and seg_observed[S] the member's status.observedGeneration; Job: KAD_SAGG_SEG_START = startTime
 * is set, seg_start[S]; KAD_SAGG_SEG_DONE = completionTime is set and not zero, seg_done[S]; KAD_SAGG_SEG_FAILED =
 * not DONE and a Failed condition with status True. The arrays of the other kind may be null.
 * Times are int64 Unix seconds. Domain: |t| <= KAD_SAGG_TIME_MAX and t != KAD_SAGG_TIME_ZERO (Go's zero time,
 * which makes the reference's start-time rule depend on its map order: the caller answers such objects itself),
 * checked where the segment's flag makes the time count.
 *
 * Outputs per object: sums[NV][O], row-major: the int32 sums, wrapped as Go's. Deployment: observed[O] =
 * obj_generation if the object is UPTODATE, no member is NIL and every member is SYNCED with seg_synced ==
 * seg_observed, else obj_observed. Job: start_min[O] (INT64_MAX: none), done_max[O] (INT64_MIN: none), n_done[O],
 * n_failed[O], finished[O] = n_done + n_failed > 0 and equal to the object's segments (the aggregated condition
 * is appended; the caller builds it and ORs its compare into changed; completionTime = done_max is written only
 * if also n_failed == 0). changed[O]: the new numeric status differs from old_vals, or OLD_OTHER. The arrays of
 * the other kind may be null.
 *
 * The kind, the offsets, every flag (unknown to the kind; NIL with START / DONE / FAILED; DONE with FAILED) and
 * the time domain are validated on the host before anything is launched (KAD_EINVAL). Runs on the ctx stream
 * (sagg_kernel: kad_statusagg.hip); blocks until the outputs are in the caller's buffers. Needs no snapshot and
 * reads no resident state, so a kad_group member accepts it. Leaves the last results, the timings and any later
 * kad_schedule as they were. n_objects == 0 returns 0 without launching. */
#define KAD_SAGG_DEPLOYMENT 0
#define KAD_SAGG_JOB 1
#define KAD_SAGG_OBJ_UPTODATE 1u
#define KAD_SAGG_OBJ_ERROR 2u
#define KAD_SAGG_OBJ_OLD_OTHER 4u
#define KAD_SAGG_SEG_NIL 1u
#define KAD_SAGG_SEG_SYNCED 2u
#define KAD_SAGG_SEG_START 4u
#define KAD_SAGG_SEG_DONE 8u
#define KAD_SAGG_SEG_FAILED 16u
#define KAD_SAGG_TIME_MAX (1ll << 61)
#define KAD_SAGG_TIME_ZERO (-62135596800ll) /* time.Time{} as Unix seconds */
typedef struct kad_sagg_batch {
  int32_t kind;       /* KAD_SAGG_DEPLOYMENT / KAD_SAGG_JOB */
  int32_t n_objects;  /* O */
  int32_t n_segments; /* S */
  int32_t reserved;   /* 0 */
  const int32_t* obj_seg_off;    /* [O + 1] */
  const uint8_t* obj_flags;      /* [O] KAD_SAGG_OBJ_* */
  const int64_t* obj_generation; /* [O] Deployment */
  const int64_t* obj_observed;   /* [O] Deployment */
  const int64_t* old_vals;       /* [NOLD * O] */
  const int32_t* seg_vals;       /* [NV * S] */
  const uint8_t* seg_flags;      /* [S] KAD_SAGG_SEG_* */
  const int64_t* seg_observed;   /* [S] Deployment */
  const int64_t* seg_synced;     /* [S] Deployment */
  const int64_t* seg_start;      /* [S] Job */
  const int64_t* seg_done;       /* [S] Job */
} kad_sagg_batch;
typedef struct kad_sagg_view {
  int32_t* sums;      /* [NV * O] */
  uint8_t* changed;   /* [O] */
  int64_t* observed;  /* [O] Deployment */
  int64_t* start_min; /* [O] Job */
  int64_t* done_max;  /* [O] Job */
  int32_t* n_done;    /* [O] Job */
  int32_t* n_failed;  /* [O] Job */
  uint8_t* finished;  /* [O] Job */
} kad_sagg_view;
int kad_status_aggregate(kad_ctx* ctx, const kad_sagg_batch* batch, const kad_sagg_view* out);
/* Host only (no device, no ctx): the same validation. */
int kad_sagg_check(const kad_sagg_batch* batch, const kad_sagg_view* out);
/* Device time of the last kad_status_aggregate that launched, from HIP events: ms[0] = sagg_kernel. No reference
 * counterpart. */
int kad_sagg_timing(kad_ctx* ctx, float ms[1]);
/* What a kad_status_aggregate launches, as the library's one decision computes it (csrc/kad_statusagg.h
 * route_sagg; no device work, no ctx) for n_objects objects, n_long of them (not in error) with more segments
 * than the route's long_min, the other objects that are not in error holding short_segments segments:
 * out[KAD_SAGG_ROUTE_FIELDS] is [0] the lanes per object of the group path (a power of two in [1, 64] from the mean
 * segments per short object / 8), [1] long_min, [2] block threads, [3] blocks of the group path, [4] blocks of the
 * long path (one per long object), [5] objects between two consecutive objects of one lane group.
 * kad_sagg_last_route: the same record for the last kad_status_aggregate that launched (KAD_ESTATE before one).
 * force_width (a power of two in [1, 64]) / force_long_min of kad_sagg_debug_route (0: the route's own) replace
 * [0] and [1] for the following calls on this ctx. Measurement / tests only. */
#define KAD_SAGG_ROUTE_FIELDS 6
int kad_sagg_route_eval(int32_t n_objects, int32_t n_long, int64_t short_segments, int32_t n_cu, int32_t* out);
int kad_sagg_last_route(kad_ctx* ctx, int32_t* out);
int kad_sagg_debug_route(kad_ctx* ctx, int32_t force_width, int32_t force_long_min);

/* ------------------------------------------------------ rollout planning
 * While a Deployment rolls out across member clusters the sync controller asks, per member cluster, which replicas,
 * maxSurge and maxUnavailable it may be given now, so that the federation as a whole stays inside the template's
 * own maxSurge / maxUnavailable (RolloutPlanner.Plan, pkg/controllers/util/rolloutplan.go:569-695, driven by
 * pkg/controllers/sync/dispatch/managed.go:160-323). kad_rollout_plan does that for a batch of objects.
 *
 * obj_tgt_off[O + 1] are an object's targets, one per member cluster, SORTED BY CLUSTER NAME in byte order (the
 * order the budgets are handed out in; the library cannot check it).
 * Per object: obj_max_surge[O] / obj_max_unavailable[O] = the template's resolved fenceposts, obj_replicas[O] =
 * the replicas over the selected clusters (NewRolloutPlanner, :459-487); obj_flags[O]: KAD_ROLLOUT_OBJ_ERROR = the
 * caller found a host-side error: nothing is computed, the status is KAD_ROLLOUT_ST_ERROR and no target is planned.
 * Per target: tgt_vals[KAD_ROLLOUT_NV][T], row-major int32: TargetStatus' Replicas, ActualReplicas,
 * AvailableReplicas, UpdatedReplicas, UpdatedAvailableReplicas, CurrentNewReplicas, CurrentNewAvailableReplicas,
 * MaxSurge, MaxUnavailable (:166-177), then DesiredReplicas; tgt_flags[T]: KAD_ROLLOUT_TGT_UPDATED = Status.Updated,
 * KAD_ROLLOUT_TGT_EXISTS = the member object is not nil (without it the status rows are 0, :367-372),
 * KAD_ROLLOUT_TGT_TO_DELETE = the cluster is no longer selected (DesiredReplicas is 0).
 *
 * Outputs per target: plan_flags[T]: KAD_ROLLOUT_PLAN_PLANNED = the cluster has a plan; _HAS_REPLICAS / _HAS_SURGE /
 * _HAS_UNAVAILABLE = the plan's field is not nil, its value in replicas[T] / max_surge[T] / max_unavailable[T] (0
 * otherwise); _ONLY_PATCH_REPLICAS. action[T] = the dispatch operation of managed.go:219-249, KAD_ROLLOUT_ACT_*.
 * Per object: status[O]: KAD_ROLLOUT_ST_OK; _SCALE = PlanScale (every target planned, every field nil); _INVALID =
 * validatePlans failed (no target planned); _ERROR. All arithmetic is Go's int32 and wraps.
 *
 * Everything is validated on the host before anything is launched (KAD_EINVAL): the counts, the offsets, unknown
 * flags, a target without EXISTS that is UPDATED, TO_DELETE or has a non-zero status, a target TO_DELETE with
 * DesiredReplicas != 0. Runs on the ctx stream (rollout_kernel: kad_rollout.hip); blocks until the outputs are in
 * the caller's buffers. Needs no snapshot and reads no resident state, so a kad_group member accepts it. Leaves the
 * last results, the timings and any later kad_schedule as they were. n_objects == 0 returns 0 without launching. */
#define KAD_ROLLOUT_NV 10
#define KAD_ROLLOUT_OBJ_ERROR 1u
#define KAD_ROLLOUT_TGT_UPDATED 1u
#define KAD_ROLLOUT_TGT_EXISTS 2u
#define KAD_ROLLOUT_TGT_TO_DELETE 4u
#define KAD_ROLLOUT_PLAN_PLANNED 1u
#define KAD_ROLLOUT_PLAN_HAS_REPLICAS 2u
#define KAD_ROLLOUT_PLAN_HAS_SURGE 4u
#define KAD_ROLLOUT_PLAN_HAS_UNAVAILABLE 8u
#define KAD_ROLLOUT_PLAN_ONLY_PATCH_REPLICAS 16u
#define KAD_ROLLOUT_ACT_KEEP_TEMPLATE_PATCH 0 /* not planned, the member object exists: patch, keep its template */
#define KAD_ROLLOUT_ACT_NONE 1                /* not planned and no member object */
#define KAD_ROLLOUT_ACT_DELETE 2
#define KAD_ROLLOUT_ACT_CREATE 3
#define KAD_ROLLOUT_ACT_PATCH_REPLICAS 4      /* patch with the planned replicas, keep its template */
#define KAD_ROLLOUT_ACT_UPDATE 5
#define KAD_ROLLOUT_ST_OK 0
#define KAD_ROLLOUT_ST_SCALE 1
#define KAD_ROLLOUT_ST_INVALID 2
#define KAD_ROLLOUT_ST_ERROR 3
typedef struct kad_rollout_batch {
  int32_t n_objects; /* O */
  int32_t n_targets; /* T */
  const int32_t* obj_tgt_off;         /* [O + 1] */
  const int32_t* obj_max_surge;       /* [O] */
  const int32_t* obj_max_unavailable; /* [O] */
  const int32_t* obj_replicas;        /* [O] */
  const uint8_t* obj_flags;           /* [O] KAD_ROLLOUT_OBJ_* */
  const int32_t* tgt_vals;            /* [KAD_ROLLOUT_NV * T] */
  const uint8_t* tgt_flags;           /* [T] KAD_ROLLOUT_TGT_* */
} kad_rollout_batch;
typedef struct kad_rollout_view {
  int32_t* replicas;        /* [T] */
  int32_t* max_surge;       /* [T] */
  int32_t* max_unavailable; /* [T] */
  uint8_t* plan_flags;      /* [T] KAD_ROLLOUT_PLAN_* */
  uint8_t* action;          /* [T] KAD_ROLLOUT_ACT_* */
  uint8_t* status;          /* [O] KAD_ROLLOUT_ST_* */
} kad_rollout_view;
int kad_rollout_plan(kad_ctx* ctx, const kad_rollout_batch* batch, const kad_rollout_view* out);
/* Host only (no device, no ctx): the same validation. nowrap[O] (may be null) receives 1 for every object whose
 * inputs' absolute values sum to less than 2^29: nothing in Plan() can wrap int32 there and the device plans it
 * with prefix sums; the other objects are walked serially in wrapping arithmetic, with the same results. */
int kad_rollout_check(const kad_rollout_batch* batch, const kad_rollout_view* out, uint8_t* nowrap);
/* Device time of the last kad_rollout_plan that launched, from HIP events: ms[0] = rollout_kernel. */
int kad_rollout_timing(kad_ctx* ctx, float ms[1]);
/* What a kad_rollout_plan launches, as the library's one decision computes it (csrc/kad_rollout.h route_rollout; no
 * device work, no ctx) for n_objects objects, n_long of them (not in error) with more targets than the route's
 * long_min, the other objects that are not in error holding short_targets targets, n_serial objects on the serial
 * walk: out[KAD_ROLLOUT_ROUTE_FIELDS] is [0] the lanes per object of the group path (the mean targets per short
 * object rounded up to a power of two in [1, 64]), [1] long_min, [2] block threads, [3] blocks of the group path,
 * [4] blocks of the long path (four long objects each, one per wave), [5] objects between two consecutive objects
 * of one lane group, [6] n_serial. kad_rollout_last_route: the same record for the last kad_rollout_plan that
 * launched (KAD_ESTATE before one). force_width (a power of two in [1, 64]) / force_long_min of
 * kad_rollout_debug_route (0: the route's own) replace [0] and [1] for the following calls on this ctx;
 * force_serial = 1 walks every object serially. Measurement / tests only. */
#define KAD_ROLLOUT_ROUTE_FIELDS 7
int kad_rollout_route_eval(int32_t n_objects, int32_t n_long, int64_t short_targets, int32_t n_serial, int32_t n_cu,
                           int32_t* out);
int kad_rollout_last_route(kad_ctx* ctx, int32_t* out);
int kad_rollout_debug_route(kad_ctx* ctx, int32_t force_width, int32_t force_long_min, int32_t force_serial);

/* ------------------------------------------------------ sync dispatch planning
 * Every reconcile of a federated object computes its placement and walks every joined cluster: is the member object
 * created, updated, deleted, orphaned or left alone, and which propagation status does the cluster get before
 * anything is dispatched (syncToClusters, pkg/controllers/sync/controller.go:425-544; ComputePlacement,
 * sync/placement.go:45-116, resource.go:170-175). kad_dispatch_plan does that for a batch of objects.
 *
 * Cluster ids are indices into the caller's list of joined clusters, 0 .. n_clusters - 1 (at most
 * KAD_DISPATCH_MAX_CLUSTERS; more is KAD_EUNSUPPORTED).
 * Per cluster: cluster_flags[C]: KAD_DISPATCH_CL_READY = a Ready condition with status True
 * (util/federatedinformer.go:292-301), _TERMINATING = a deletion timestamp is set, _CASCADING = the cascading-delete
 * annotation is present (util/cascadingdeleteannotation.go:29-40), _FINALIZER = the cluster carries the sync
 * controller's cascading-delete finalizer.
 * Per object: obj_flags[O]: KAD_DISPATCH_OBJ_ERROR = the placement could not be unmarshalled: nothing is emitted and
 * obj_result is KAD_DISPATCH_RES_PLACEMENT_FAILED; _ORPHAN_ALL / _ORPHAN_ADOPTED = GetOrphaningBehavior
 * (util/orphaningannotation.go:48-62), never both. obj_ns[O]: >= 0 = a row of the namespace table whose placement is
 * intersected with the object's; KAD_DISPATCH_NS_NONE = no intersection (a cluster-scoped type, or limited scope
 * without a federated namespace); KAD_DISPATCH_NS_UNFEDERATED = a namespaced type without a federated namespace:
 * nothing is selected (placement.go:55-64).
 * Placement: obj_pl_off[O + 1] into pl_cluster[]: every controller's ClusterNames() in the object's own order,
 * unsorted, duplicates allowed, -1 for a name that is not a joined cluster (dropped); the union is taken on the
 * device. The namespace table ns_pl_off[N + 1] / ns_cluster[] follows the same rules, a row per federated namespace.
 * Observations: obj_ob_off[O + 1] into ob_cluster[] (STRICTLY ASCENDING within an object) and ob_flags[]: an entry
 * for every cluster where the informer holds the target (KAD_DISPATCH_OB_EXISTS, with _DELETING = it has a deletion
 * timestamp, _ADOPTED = it carries the adopted annotation) or the lookup failed (_RETRIEVAL_FAILED); exactly one of
 * EXISTS and RETRIEVAL_FAILED is set.
 * out_off[O + 1] (built by the caller, from 0): object o may emit out_off[o + 1] - out_off[o] entries, which must be
 * at least its placement entries plus its observations (a cluster neither selected nor observed never emits).
 *
 * Outputs: object o's entries are out_cluster / out_op (KAD_DISPATCH_OP_*) / out_status (KAD_DISPATCH_ST_*) at
 * [out_off[o], out_off[o] + count[o]), ascending by cluster id, only clusters with an operation or a status; the
 * slots behind them are not written. n_ops[O] = the operations started, n_selected[O] = the size of the computed
 * placement, obj_result[O]: KAD_DISPATCH_RES_RECHECK = shouldRecheckAfterDispatch, _PLACEMENT_FAILED. The status of
 * an entry with an operation is the one the dispatcher records when the operation is started (CreationTimedOut ...:
 * dispatch/managed.go:330, 403, 477-481, 566-570); Wait() moves it on.
 * The decision per (object, cluster) is csrc/kad_dispatch.h di_decide, the same function on the device and the host
 * (kad_dispatch_decide). Declared deviation: the error branch of finalizersutil.HasFinalizer (:523-528) cannot be
 * reached for a typed cluster object and has no input bit.
 *
 * Everything is validated on the host before anything is launched (KAD_EINVAL): the counts, the offsets, ids
 * outside [-1, C) (observations: [0, C)), observations not strictly ascending, unknown or inconsistent flags,
 * obj_ns outside [-2, N), a capacity below the bound. Runs on the ctx stream (dispatch_wave_kernel:
 * kad_dispatch.hip); blocks until the outputs are in the caller's buffers. Needs no snapshot and reads no resident
 * state, so a kad_group member accepts it. Leaves the last results, the timings and any later kad_schedule as they
 * were. n_objects == 0 returns 0 without launching. */
#define KAD_DISPATCH_MAX_CLUSTERS 16384
#define KAD_DISPATCH_CL_READY 1u
#define KAD_DISPATCH_CL_TERMINATING 2u
#define KAD_DISPATCH_CL_CASCADING 4u
#define KAD_DISPATCH_CL_FINALIZER 8u
#define KAD_DISPATCH_OBJ_ERROR 1u
#define KAD_DISPATCH_OBJ_ORPHAN_ALL 2u
#define KAD_DISPATCH_OBJ_ORPHAN_ADOPTED 4u
#define KAD_DISPATCH_OB_EXISTS 1u
#define KAD_DISPATCH_OB_DELETING 2u
#define KAD_DISPATCH_OB_ADOPTED 4u
#define KAD_DISPATCH_OB_RETRIEVAL_FAILED 8u
#define KAD_DISPATCH_NS_NONE (-1)
#define KAD_DISPATCH_NS_UNFEDERATED (-2)
#define KAD_DISPATCH_OP_NONE 0
#define KAD_DISPATCH_OP_CREATE 1
#define KAD_DISPATCH_OP_UPDATE 2
#define KAD_DISPATCH_OP_DELETE 3
#define KAD_DISPATCH_OP_REMOVE_LABEL 4
#define KAD_DISPATCH_ST_NONE 0 /* never emitted */
#define KAD_DISPATCH_ST_CLUSTER_NOT_READY 1
#define KAD_DISPATCH_ST_CACHED_RETRIEVAL_FAILED 2
#define KAD_DISPATCH_ST_WAITING_FOR_REMOVAL 3
#define KAD_DISPATCH_ST_LABEL_REMOVAL_TIMED_OUT 4
#define KAD_DISPATCH_ST_DELETION_TIMED_OUT 5
#define KAD_DISPATCH_ST_CLUSTER_TERMINATING 6
#define KAD_DISPATCH_ST_FINALIZER_CHECK_FAILED 7
#define KAD_DISPATCH_ST_CREATION_TIMED_OUT 8
#define KAD_DISPATCH_ST_UPDATE_TIMED_OUT 9
#define KAD_DISPATCH_RES_RECHECK 1u
#define KAD_DISPATCH_RES_PLACEMENT_FAILED 2u
typedef struct kad_dispatch_batch {
  int32_t n_clusters;   /* C */
  int32_t n_objects;    /* O */
  int32_t n_namespaces; /* N */
  const uint8_t* cluster_flags; /* [C] KAD_DISPATCH_CL_* */
  const uint8_t* obj_flags;     /* [O] KAD_DISPATCH_OBJ_* */
  const int32_t* obj_ns;        /* [O] */
  const int32_t* obj_pl_off;    /* [O + 1] */
  const int32_t* pl_cluster;    /* [obj_pl_off[O]] */
  const int32_t* ns_pl_off;     /* [N + 1] */
  const int32_t* ns_cluster;    /* [ns_pl_off[N]] */
  const int32_t* obj_ob_off;    /* [O + 1] */
  const int32_t* ob_cluster;    /* [obj_ob_off[O]] */
  const uint8_t* ob_flags;      /* [obj_ob_off[O]] KAD_DISPATCH_OB_* */
  const int64_t* out_off;       /* [O + 1] */
} kad_dispatch_batch;
typedef struct kad_dispatch_view {
  int32_t* out_cluster; /* [out_off[O]] */
  uint8_t* out_op;      /* [out_off[O]] KAD_DISPATCH_OP_* */
  uint8_t* out_status;  /* [out_off[O]] KAD_DISPATCH_ST_* */
  int32_t* count;       /* [O] */
  int32_t* n_ops;       /* [O] */
  int32_t* n_selected;  /* [O] */
  uint8_t* obj_result;  /* [O] KAD_DISPATCH_RES_* */
} kad_dispatch_view;
int kad_dispatch_plan(kad_ctx* ctx, const kad_dispatch_batch* batch, const kad_dispatch_view* out);
/* Host only (no device, no ctx): the same validation; KAD_EUNSUPPORTED above KAD_DISPATCH_MAX_CLUSTERS. */
int kad_dispatch_check(const kad_dispatch_batch* batch, const kad_dispatch_view* out);
/* Host only: the decision for one (object, cluster) pair as the kernel takes it (csrc/kad_dispatch.h di_decide):
 * out[0] = the operation, out[1] = the status, out[2] = 1 when the object is to be rechecked after dispatch. */
int kad_dispatch_decide(uint32_t cluster_flags, int32_t selected, uint32_t ob_flags, uint32_t obj_flags, uint8_t out[3]);
/* Times of the last kad_dispatch_plan that launched, from HIP events: ms[0] = the inputs' copies to the device,
 * ms[1] = dispatch_wave_kernel, ms[2] = the outputs' copies back. */
int kad_dispatch_timing(kad_ctx* ctx, float ms[3]);
/* What a kad_dispatch_plan launches, as the library's one decision computes it (csrc/kad_dispatch.h route_dispatch;
 * no device work, no ctx): out[KAD_DISPATCH_ROUTE_FIELDS] is [0] the u32 words of one bitmap = ceil(C / 32), [1]
 * block threads, [2] blocks (one object per wave at a time, four waves a block; at most as many blocks as stay
 * resident), [3] dynamic LDS bytes a block (three bitmaps per wave), [4] objects between two consecutive objects of
 * one wave. kad_dispatch_last_route: the same record for the last kad_dispatch_plan that launched (KAD_ESTATE
 * before one). */
#define KAD_DISPATCH_ROUTE_FIELDS 5
int kad_dispatch_route_eval(int32_t n_clusters, int32_t n_objects, int32_t n_cu, int32_t* out);
int kad_dispatch_last_route(kad_ctx* ctx, int32_t* out);

/* ------------------------------------------------------ policy reference counts
 * The policy reference counter (pkg/controllers/policyrc) keeps, per PropagationPolicy / ClusterPropagationPolicy and
 * per OverridePolicy / ClusterOverridePolicy, the number of federated objects of one type that reference it
 * (Counter.Update, counter.go:50-80: a map under one mutex, "only one worker is meaningful", :33-34) and writes it
 * into the policy's status.typedRefCount and status.refCount (reconcilePersist, controller.go:280-366).
 * kad_policyrc_count does the counting and the persist decision for a batch of reference changes.
 *
 * The device never sees objects: the caller interns policy keys to ids 0 .. n_policies - 1 (propagation and override
 * policies share the table, so one call serves both of the reference's counters) and lists one id per reference
 * removed in dec_ids[n_dec] (an object's previously known policies, counter.go:67-74) and one per reference added in
 * inc_ids[n_inc] (:76-78); either list may be null when its count is 0. Per policy: count[P] = the counter's current
 * value; stored_typed[P] = the policy's stored TypedRefCount.Count for this type config's (group, resource), 0
 * without such an entry (controller.go:320-335); stored_rest[P] = the sum of its other typed entries;
 * stored_total[P] = its status.refCount; pol_flags[P]: KAD_PRC_POL_EXISTS = the policy is in the store
 * (controller.go:307-310), KAD_PRC_POL_ENQUEUED = it is to be persisted even if no id names it (a policy informer
 * event: the informers' EnqueueObject, controller.go:146-192).
 *
 * Outputs: new_count[P] = count + adds - removals; new_total[P] = stored_rest + new_count (both wrap as Go's
 * int64); state[P]: KAD_PRC_FLAGGED = at least one id of either list names the policy (the reference's
 * flaggedPolicies as a set: a policy removed and added equally often is flagged with a delta of 0), KAD_PRC_UPDATE =
 * EXISTS and (FLAGGED or ENQUEUED) and (new_count != stored_typed or new_total != stored_total): reconcilePersist's
 * hasChange (controller.go:337-353), KAD_PRC_NEGATIVE = new_count < 0; n_negative[1] = the policies with
 * KAD_PRC_NEGATIVE.
 * Declared deviation: the reference panics the moment a decrement takes a count below 0 (counter.go:69-72). The call
 * reports the final count instead and never aborts: a count that dips below 0 between two events of one batch and
 * recovers is not seen. The caller's bookkeeping keeps the invariant (an id is only ever removed after it was added).
 *
 * Everything is validated on the host before anything is launched (KAD_EINVAL): a negative count, a null array with a
 * non-zero count, an id outside [0, P), unknown pol_flags bits, reserved != 0, a missing output. Runs on the ctx
 * stream (prc_count_kernel builds the two histograms, prc_apply_kernel the outputs: kad_policyrc.hip); blocks until
 * the outputs are in the caller's buffers. Everything is integer: the results do not depend on the order in which
 * ids arrive. Needs no snapshot and reads no resident state, so a kad_group member accepts it. Leaves the last
 * results, the timings and any later kad_schedule as they were. n_policies == 0 returns 0 without launching. */
#define KAD_PRC_POL_EXISTS 1u
#define KAD_PRC_POL_ENQUEUED 2u
#define KAD_PRC_FLAGGED 1u
#define KAD_PRC_UPDATE 2u
#define KAD_PRC_NEGATIVE 4u
typedef struct kad_policyrc_batch {
  int32_t n_policies; /* P */
  int32_t n_dec;
  int32_t n_inc;
  int32_t reserved;   /* 0 */
  const int32_t* dec_ids;      /* [n_dec] in [0, P) */
  const int32_t* inc_ids;      /* [n_inc] in [0, P) */
  const int64_t* count;        /* [P] */
  const int64_t* stored_typed; /* [P] */
  const int64_t* stored_rest;  /* [P] */
  const int64_t* stored_total; /* [P] */
  const uint8_t* pol_flags;    /* [P] KAD_PRC_POL_* */
} kad_policyrc_batch;
typedef struct kad_policyrc_view {
  int64_t* new_count;  /* [P] */
  int64_t* new_total;  /* [P] */
  uint8_t* state;      /* [P] KAD_PRC_FLAGGED | _UPDATE | _NEGATIVE */
  int32_t* n_negative; /* [1] */
} kad_policyrc_view;
int kad_policyrc_count(kad_ctx* ctx, const kad_policyrc_batch* batch, const kad_policyrc_view* out);
/* Host only (no device, no ctx): the same validation. */
int kad_policyrc_check(const kad_policyrc_batch* batch, const kad_policyrc_view* out);
/* Times of the last kad_policyrc_count that launched, from HIP events: ms[0] = the inputs' copies to the device,
 * ms[1] = the zeroing of the histograms and prc_count_kernel, ms[2] = prc_apply_kernel. */
int kad_policyrc_timing(kad_ctx* ctx, float ms[3]);
/* What a kad_policyrc_count launches, as the library's one decision computes it (csrc/kad_policyrc.h
 * route_policyrc; no device work, no ctx): n_ids = n_dec + n_inc. out[KAD_PRC_ROUTE_FIELDS] is [0] the count
 * kernel's path: 0 = LDS-private (every block counts into 2 * P bins of its own in LDS and adds its non-zero bins
 * to the histograms), 1 = global (every wave merges runs of equal neighbouring ids and adds one global atomic per
 * run), [1] the bins limit: the largest P of the LDS-private path, [2] block threads, [3] count-kernel blocks (0
 * without ids: only the zeroing and the apply kernel run), [4] ids a lane reads per step, [5] apply-kernel blocks
 * (one thread per policy). kad_policyrc_last_route: the same record for the last kad_policyrc_count that launched
 * (KAD_ESTATE before one). */
#define KAD_PRC_ROUTE_FIELDS 6
int kad_policyrc_route_eval(int32_t n_policies, int64_t n_ids, int32_t n_cu, int32_t* out);
int kad_policyrc_last_route(kad_ctx* ctx, int32_t* out);
/* Measurement and tests only: the count kernel's path of the following kad_policyrc_count calls: 0 = the route's
 * own, 1 = LDS-private, 2 = global. LDS-private forced on more policies than the bins limit: KAD_EINVAL from that
 * call. */
int kad_policyrc_debug_route(kad_ctx* ctx, int32_t force_path);

/* ------------------------------------------------------ sync completion: propagated versions and status
 * The second half of the sync controller's syncToClusters (pkg/controllers/sync/controller.go:425-596), after
 * kad_dispatch_plan has decided the operations: kad_sync_needs_update is the version check of every update
 * (dispatch/managed.go:450-460, util/propagatedversion.go:54-119, sync/version/manager.go:119-148) and runs before
 * the operations; kad_sync_finish closes the reconcile after dispatcher.Wait() (controller.go:546-596): Wait's
 * status transitions (managed.go:137-155), the new cluster versions and whether the PropagatedVersion object is
 * written (manager.go:152-210, 448-479), ConvertVersionMapToGenerationMap (propagatedversion.go:138-157) and
 * status.update (sync/status/status.go:87-229).
 *
 * Shared conventions. Cluster ids 0 .. C - 1 index the joined clusters in ascending byte order of their names, so
 * that ascending id is sort.Strings / SortClusterVersions order; C <= KAD_DISPATCH_MAX_CLUSTERS, more is
 * KAD_EUNSUPPORTED. The device never sees a version string: the caller interns the distinct version strings of the
 * batch into a table of V entries, id 0 = no version (its flags are 0), equal id <=> equal string;
 * ver_flags[V]: KAD_SYNC_VER_HAS_GEN = ConvertVersionMapToGenerationMap has an entry for the string, ver_gen[V] its
 * value (0 for an "rv:" prefix, the parsed number for a "gen:" prefix that strconv.ParseInt(.., 10, 64) accepts);
 * KAD_SYNC_VER_IS_GEN = the string starts with "gen:" (propagatedversion.go:118). Propagation statuses are the u8
 * codes KAD_SYNC_ST_*: 1 .. 23 in the order of the constants of pkg/apis/types/v1alpha1/types_status.go:71-99,
 * 0 = none. Aggregate reasons are interned per batch into R ids, 0 = AggregateSuccess; the ids of CheckClusters and
 * NamespaceNotFederated are given in the batch (distinct, in [1, R)).
 *
 * kad_sync_needs_update: one row per (object, cluster) whose operation is an update. row_obj / row_cluster /
 * row_target[n_rows]: the object, the cluster and the id of ObjectVersion(clusterObj); row_flags: KAD_SYNC_ROW_* =
 * what ObjectNeedsUpdate reads from the two objects, decided on the host (replicas equal; maxSurge equal;
 * maxUnavailable equal; ObjectMetaObjEquivalent). obj_flags[O]: KAD_SYNC_VERSIONS_CURRENT = a PropagatedVersion is
 * stored and its template and override versions equal the object's (manager.go:140-141); rec_off[O + 1] /
 * rec_cluster / rec_version: its recorded cluster versions, strictly ascending by cluster within an object.
 * recorded[row] = the version VersionForCluster returns: the object's entry for the cluster (binary search), 0
 * without one or when the object is not VERSIONS_CURRENT. needs_update[row] = recorded != target, or one of the three
 * equality flags is clear, or the target is IS_GEN and META_EQUIVALENT is clear. One lane per row.
 *
 * kad_sync_finish: per object four lists as CSRs, each strictly ascending by cluster id: sel (the selected clusters),
 * ent (the dispatcher's records: cluster, the status recorded when the operation ended and before Wait's
 * transitions, the version recordVersion recorded or 0), oldv (the stored PropagatedVersion's cluster versions) and
 * olds (the stored status.clusters: cluster, status, generation). obj_flags[O] (KAD_SYNC_OBJ_*): VERSION_EXISTS,
 * VERSIONS_CURRENT (needs VERSION_EXISTS), OLDV_NIL (the stored list is absent, not empty: reflect.DeepEqual tells
 * them apart; oldv must be empty), OLDV_IRREGULAR (the caller dropped an unknown cluster or a duplicate, keeping the
 * first as updateClusterVersions does, or reordered), RESOURCES_UPDATED, SCALARS_CHANGED (syncedGeneration or
 * collisionCount moved, status.go:94-102), COND_EXISTS, COND_TRUE, STATUS_ON_HOST. Without VERSION_EXISTS oldv is
 * empty. reason_in[O]: the reason setFederatedStatus hands to update (NamespaceNotFederated applied by the caller,
 * controller.go:649-656); cond_reason[O]: the stored condition's reason id, -1 for a stored condition that can equal
 * no new one (a status that is neither True nor False). ver_off[O + 1] / st_off[O + 1]: where an object's version
 * and status entries go; capacities of at least |ent| + |oldv| and |ent|.
 * Per object: (1) CreationTimedOut / UpdateTimedOut become OK, DeletionTimedOut WaitingForRemoval, a
 * LabelRemovalTimedOut entry loses its status. (2) The new cluster versions: every ent with a version, and, only if
 * VERSIONS_CURRENT, every oldv entry whose cluster is selected and has no ent version; ascending from ver_off[o],
 * ver_count[o] of them. (3) ver_write[o] = !VERSION_EXISTS, !VERSIONS_CURRENT, OLDV_IRREGULAR, OLDV_NIL with an empty
 * new list, or the new list differs from oldv (PropagatedVersionStatusEquivalent). (4) The status map is the ent
 * with a status left, the generation map the ent with a HAS_GEN version; clustersDiffers compares len(olds) with
 * both sizes separately (status.go:164-169), then every olds entry with the maps. (5) reason_out = reason_in, or
 * CheckClusters where that is success and a status is not OK. (6) status.clusters: one (cluster, status, generation
 * or 0) per status-map entry from st_off[o], st_count[o] of them, always written. (7) obj_out[o] (KAD_SYNC_OUT_*):
 * CLUSTERS_CHANGED; CHANGES_PROPAGATED = that, or a non-empty status map with RESOURCES_UPDATED; TRANSITION =
 * !COND_EXISTS or COND_TRUE != (reason == success) or cond_reason != reason; UPDATE_REQUIRED = CHANGES_PROPAGATED or
 * TRANSITION; STATUS_WRITE = SCALARS_CHANGED or UPDATE_REQUIRED. Slots behind an object's counts are unspecified.
 * Declared deviations: an ent version of 0 is "no record": the reference could hold an empty string there, which
 * nothing in it records. Objects whose Wait() timed out never reach this code (controller.go:550-554): the caller
 * leaves them out. A stored status.clusters with a duplicate name, a cluster that is not joined or a status outside
 * the constants meets corners of Go's map lookups ([a, a] against {a, b} does not differ): the caller marks the
 * object STATUS_ON_HOST (olds must then be empty), the device writes 0 to its st_count, obj_out and reason_out and
 * the caller decides it; its version outputs still come from the device.
 *
 * Everything is validated on the host before anything is launched (KAD_EINVAL): counts, offsets, lists not strictly
 * ascending, ids outside [0, C), version ids outside [0, V), unknown status codes or flag bits, reason ids,
 * capacities below the bound, missing arrays. Both run on the ctx stream (syncfin_rows_kernel; syncfin_kernel:
 * kad_syncfin.hip) and block until the outputs are in the caller's buffers. Integers only, no atomics: the results
 * do not depend on any order. They need no snapshot and read no resident state, so a kad_group member accepts them;
 * they leave the last results, the timings and any later kad_schedule as they were. n_objects == 0 (n_rows == 0)
 * returns 0 without launching. */
#define KAD_SYNC_ST_OK 1u
#define KAD_SYNC_ST_WAITING_FOR_REMOVAL 2u
#define KAD_SYNC_ST_CREATION_TIMED_OUT 20u
#define KAD_SYNC_ST_UPDATE_TIMED_OUT 21u
#define KAD_SYNC_ST_DELETION_TIMED_OUT 22u
#define KAD_SYNC_ST_LABEL_REMOVAL_TIMED_OUT 23u
#define KAD_SYNC_ST_MAX 23u
#define KAD_SYNC_VER_HAS_GEN 1u
#define KAD_SYNC_VER_IS_GEN 2u
#define KAD_SYNC_ROW_REPLICAS_EQUAL 1u
#define KAD_SYNC_ROW_SURGE_EQUAL 2u
#define KAD_SYNC_ROW_UNAVAILABLE_EQUAL 4u
#define KAD_SYNC_ROW_META_EQUIVALENT 8u
#define KAD_SYNC_VERSIONS_CURRENT 1u /* kad_sync_needs_update's obj_flags */
#define KAD_SYNC_OBJ_VERSION_EXISTS 1u
#define KAD_SYNC_OBJ_VERSIONS_CURRENT 2u
#define KAD_SYNC_OBJ_OLDV_NIL 4u
#define KAD_SYNC_OBJ_OLDV_IRREGULAR 8u
#define KAD_SYNC_OBJ_RESOURCES_UPDATED 16u
#define KAD_SYNC_OBJ_SCALARS_CHANGED 32u
#define KAD_SYNC_OBJ_COND_EXISTS 64u
#define KAD_SYNC_OBJ_COND_TRUE 128u
#define KAD_SYNC_OBJ_STATUS_ON_HOST 256u
#define KAD_SYNC_OUT_CLUSTERS_CHANGED 1u
#define KAD_SYNC_OUT_CHANGES_PROPAGATED 2u
#define KAD_SYNC_OUT_TRANSITION 4u
#define KAD_SYNC_OUT_UPDATE_REQUIRED 8u
#define KAD_SYNC_OUT_STATUS_WRITE 16u
typedef struct kad_sync_nu_batch {
  int32_t n_clusters; /* C */
  int32_t n_objects;  /* O */
  int32_t n_rows;
  int32_t n_versions; /* V >= 1 */
  const int32_t* row_obj;     /* [n_rows] in [0, O) */
  const int32_t* row_cluster; /* [n_rows] in [0, C) */
  const int32_t* row_target;  /* [n_rows] in [0, V) */
  const uint8_t* row_flags;   /* [n_rows] KAD_SYNC_ROW_* */
  const uint8_t* obj_flags;   /* [O] KAD_SYNC_VERSIONS_CURRENT */
  const int32_t* rec_off;     /* [O + 1] */
  const int32_t* rec_cluster; /* [rec_off[O]] */
  const int32_t* rec_version; /* [rec_off[O]] in [0, V) */
  const uint8_t* ver_flags;   /* [V] KAD_SYNC_VER_* */
} kad_sync_nu_batch;
typedef struct kad_sync_nu_view {
  uint8_t* needs_update; /* [n_rows] */
  int32_t* recorded;     /* [n_rows] */
} kad_sync_nu_view;
int kad_sync_needs_update(kad_ctx* ctx, const kad_sync_nu_batch* batch, const kad_sync_nu_view* out);
/* Host only (no device, no ctx): the same validation. */
int kad_sync_needs_update_check(const kad_sync_nu_batch* batch, const kad_sync_nu_view* out);
/* ms[0] = the inputs' copies to the device, ms[1] = syncfin_rows_kernel, ms[2] = the outputs' copies back. */
int kad_sync_needs_update_timing(kad_ctx* ctx, float ms[3]);
/* csrc/kad_syncfin.h route_sync_rows: out[KAD_SYNC_NU_ROUTE_FIELDS] is [0] block threads, [1] blocks (a lane per
 * row; at most 8 blocks a CU), [2] rows between two consecutive rows of one lane. */
#define KAD_SYNC_NU_ROUTE_FIELDS 3
int kad_sync_needs_update_route_eval(int32_t n_rows, int32_t n_cu, int32_t* out);
int kad_sync_needs_update_last_route(kad_ctx* ctx, int32_t* out);

typedef struct kad_sync_fin_batch {
  int32_t n_clusters; /* C */
  int32_t n_objects;  /* O */
  int32_t n_versions; /* V >= 1 */
  int32_t n_reasons;  /* R >= 3 */
  int32_t reason_check_clusters;
  int32_t reason_ns_not_federated;
  const uint16_t* obj_flags;   /* [O] KAD_SYNC_OBJ_* */
  const int32_t* reason_in;    /* [O] in [0, R) */
  const int32_t* cond_reason;  /* [O] in [-1, R) */
  const int32_t* sel_off;      /* [O + 1] */
  const int32_t* sel_cluster;
  const int32_t* ent_off;      /* [O + 1] */
  const int32_t* ent_cluster;
  const uint8_t* ent_status;   /* 0 .. KAD_SYNC_ST_MAX */
  const int32_t* ent_version;  /* in [0, V) */
  const int32_t* oldv_off;     /* [O + 1] */
  const int32_t* oldv_cluster;
  const int32_t* oldv_version; /* in [1, V) */
  const int32_t* olds_off;     /* [O + 1] */
  const int32_t* olds_cluster;
  const uint8_t* olds_status;  /* 1 .. KAD_SYNC_ST_MAX */
  const int64_t* olds_gen;
  const int64_t* ver_gen;      /* [V] */
  const uint8_t* ver_flags;    /* [V] KAD_SYNC_VER_* */
  const int64_t* ver_off;      /* [O + 1] */
  const int64_t* st_off;       /* [O + 1] */
} kad_sync_fin_batch;
typedef struct kad_sync_fin_view {
  int32_t* out_ver_cluster; /* [ver_off[O]] */
  int32_t* out_ver_id;      /* [ver_off[O]] */
  int32_t* ver_count;       /* [O] */
  uint8_t* ver_write;       /* [O] */
  int32_t* out_st_cluster;  /* [st_off[O]] */
  uint8_t* out_st_status;   /* [st_off[O]] */
  int64_t* out_st_gen;      /* [st_off[O]] */
  int32_t* st_count;        /* [O] */
  uint8_t* obj_out;         /* [O] KAD_SYNC_OUT_* */
  int32_t* reason_out;      /* [O] */
} kad_sync_fin_view;
int kad_sync_finish(kad_ctx* ctx, const kad_sync_fin_batch* batch, const kad_sync_fin_view* out);
/* Host only (no device, no ctx): the same validation. */
int kad_sync_finish_check(const kad_sync_fin_batch* batch, const kad_sync_fin_view* out);
/* ms[0] = the inputs' copies to the device, ms[1] = syncfin_kernel, ms[2] = the outputs' copies back. */
int kad_sync_finish_timing(kad_ctx* ctx, float ms[3]);
/* csrc/kad_syncfin.h route_sync_finish: an object's size is its longest list of ent, oldv and olds; n_long = the
 * objects larger than the route's long_min, short_items = the summed sizes of the others.
 * out[KAD_SYNC_FIN_ROUTE_FIELDS] is [0] lanes per object on the group path (the mean size of a short object over
 * the elements a lane takes, a power of two in [1, 64]), [1] long_min, [2] block threads, [3] blocks of the group
 * path, [4] blocks of the long path (one object per block), [5] objects between two consecutive objects of one lane
 * group. */
#define KAD_SYNC_FIN_ROUTE_FIELDS 6
int kad_sync_finish_route_eval(int32_t n_objects, int32_t n_long, int64_t short_items, int32_t n_cu, int32_t* out);
int kad_sync_finish_last_route(kad_ctx* ctx, int32_t* out);
/* Measurement and tests only: the lane-group width (0 or a power of two in [1, 64]) and long_min (0: the route's
 * own) of the following kad_sync_finish calls. */
int kad_sync_finish_debug_route(kad_ctx* ctx, int32_t force_width, int32_t force_long_min);

/* ------------------------------------------------------ monitor: per-object sync and status meters, their report
 * The monitor controller (pkg/controllers/monitor) keeps one BaseMeter per federated object (monitor_controller.go:
 * 75-82), updates it on every object event (MonitorSubController.reconcile, monitor_subcontroller.go:172-343) and
 * walks all of them every ReportInterval (DoReport, report.go:31-163). The meters are the one consumer state that
 * stays on the device between calls: a table of slots, one per meter, a column per field (creation, last_update,
 * sync_success, last_status_synced as times, out_of_sync_ns as a duration, the interned kind type_id = the text before
 * the first '/' of the meter key, flags with KAD_MON_LIVE). The caller maps meter keys to slots, interns kinds and
 * cluster names, and keeps every meter's lastStatus map; the device says when to replace one.
 *
 * Time: int64 nanoseconds since the Unix epoch, a real time in [0, 2^62). Go's zero time.Time is KAD_MON_TIME_ZERO
 * (-2^62); a time derived from it by Add is KAD_MON_TIME_ZERO plus the duration (all such values lie below -2^61 and
 * order as Go orders them). After is >, IsZero is == KAD_MON_TIME_ZERO, and Sub saturates at MinInt64 / MaxInt64
 * whenever exactly one operand lies below -2^61, as Go's does for operands more than 292 years apart. `now` is always
 * an argument and a real time.
 *
 * kad_monitor_reserve grows the table to at least `capacity` slots and keeps its contents (it never shrinks);
 * kad_monitor_load writes n slots (distinct, in [0, capacity)) from the caller's columns, kad_monitor_read reads n
 * slots back (any array of either may be null: that column is left alone / not returned; load's times must be real,
 * or within 2^60 of KAD_MON_TIME_ZERO; flags only KAD_MON_LIVE; type_id >= 0); kad_monitor_clear empties the table
 * and keeps its capacity; kad_monitor_info: out[0] capacity, out[1] n_slots = one past the highest slot ever written
 * since the last clear (what the report walks), out[2] the live slots, out[3] the highest type id stored, -1 without.
 *
 * kad_monitor_reconcile: a batch of n_objects events, slot[i] distinct within the call (the reference's worker
 * serialises per key: a caller whose batch repeats a key splits it into successive calls). obj_flags[i] carries what
 * the caller read from strings: KAD_MON_OBJ_DELETED (the object is absent or has a deletionTimestamp: the meter is
 * deleted and nothing else happens, :182-191), _NEW (no meter yet: creation_ns[i], KAD_MON_TIME_ZERO without a
 * creationTimestamp, starts one; it must agree with the slot's LIVE flag), _SS_PARSED (the syncSuccessTimestamp
 * annotation parsed: sync_success_ns[i]; an absent or unparsable one keeps the meter's value, :257-262),
 * _LASTGEN_PRESENT / _LASTGEN_EQUAL and _LSSG_PRESENT / _LSSG_EQUAL (the lastGeneration / lastSyncSuccessGeneration
 * annotation exists / equals strconv.FormatInt(generation) as a string, :266-293), _STATUS_ENABLED (the type config's,
 * :210), _STATUS_ABSENT (the status object is absent or being deleted, :216-224), _FED_MISSING (a clusterStatus entry
 * lacks clusterName or status.observedGeneration: ErrMissingObservedGenerationField, checked before the member
 * clusters, :388-402), _CLUSTER_ERR (a member object lacks status.observedGeneration, :418-429), _HAS_LAST (the
 * meter's lastStatus is not nil, which an empty map is not). Three CSR lists of (cluster id, observedGeneration) per
 * object, each strictly ascending by cluster id (the caller dedupes, the later of two equal names winning as in the
 * Go map): fed (the status object's clusterStatus), mem (the member clusters' objects), last (the meter's lastStatus).
 * reflect.DeepEqual of two such maps is "same length and equal entry by entry".
 * Outputs per object: result[i] (KAD_MON_RESULT_ALL_OK, _STATUS_ERROR, _REQUEUE = worker.Result{RequeueAfter: 5 s});
 * bits[i]: KAD_MON_BIT_METER_DELETED, _UPDATE_ANNOTATION (write lastGeneration = generation, :295-298),
 * _STATUS_STORED (the status half was stored: the second meters.Store, :250), _REPLACE_LAST (the stored lastStatus
 * becomes this call's mem list), _MISSING_OBSERVED_GENERATION, _LOG_LAST_CLUSTER (the log line's lastStatus is the mem
 * list); meter[i][5] = the slot's five columns after the call (zeros for a deleted meter); would[i][2] = the log
 * line's lastStatusSyncedTimestamp and outOfSyncDuration (:228-249). On ErrStatusOutOfSync the reference has changed
 * its local copy of the meter and returns without storing it (:236-237): would[] and _LOG_LAST_CLUSTER carry those
 * values, the slot's status columns stay as they were.
 * One launch (monitor_reconcile_kernel: a lane group per object, the two DeepEquals as strided compares and a ballot,
 * the group's lane 0 runs the state machine and writes the slot in place). Validated on the host first (KAD_EINVAL;
 * more than KAD_DISPATCH_MAX_CLUSTERS clusters: KAD_EUNSUPPORTED; a slot at or beyond the capacity: KAD_ENOSPC).
 *
 * kad_monitor_report: DoReportLatencyCount, DoReportSyncLatency and DoReportStatusLatency at now_ns over slots
 * [0, n_slots). counters[14]: [0..5] the latency5min, 10min, 30min, 1hour, 6hour (180 minutes as in the reference) and
 * 1day counts, [6..11] their .status counts (counted inside start.After(syncSuccessTimestamp), as report.go:112-141
 * does), [12] totalsync.throughput, [13] totalstatus.throughput; type_sync[n_types] / type_status[n_types] the
 * typelatency5min.count / .status.count per type id (the reference emits the non-zero ones); the timer lists
 * (slot, Milliseconds()) of totalsync.latency.ms and totalstatus.latency.ms in ascending slot order, n_timers[2]
 * their lengths. A list longer than timer_cap: KAD_ENOSPC with n_timers and everything else filled in and the first
 * timer_cap entries of the list. n_types must exceed every stored type id. Integer atomics only: nothing depends on an
 * order. Neither call reads or writes state that kad_schedule uses; a kad_group member accepts them.
 * A call that fails its validation changes nothing. The host's record of the table (the LIVE flags that _NEW is
 * checked against, n_slots, the highest type id) follows a call only once its kernel and copies have completed: after
 * a KAD_EHIP from kad_monitor_reconcile or kad_monitor_load the device table and that record may disagree, and the
 * table is to be emptied (kad_monitor_clear) and loaded again before it is used. */
#define KAD_MON_TIME_ZERO (-(1ll << 62))
#define KAD_MON_LIVE 1u
#define KAD_MON_OBJ_DELETED 1u
#define KAD_MON_OBJ_NEW 2u
#define KAD_MON_OBJ_SS_PARSED 4u
#define KAD_MON_OBJ_LASTGEN_PRESENT 8u
#define KAD_MON_OBJ_LASTGEN_EQUAL 16u
#define KAD_MON_OBJ_LSSG_PRESENT 32u
#define KAD_MON_OBJ_LSSG_EQUAL 64u
#define KAD_MON_OBJ_STATUS_ENABLED 128u
#define KAD_MON_OBJ_STATUS_ABSENT 256u
#define KAD_MON_OBJ_FED_MISSING 512u
#define KAD_MON_OBJ_CLUSTER_ERR 1024u
#define KAD_MON_OBJ_HAS_LAST 2048u
#define KAD_MON_RESULT_ALL_OK 0
#define KAD_MON_RESULT_STATUS_ERROR 1
#define KAD_MON_RESULT_REQUEUE 2
#define KAD_MON_BIT_METER_DELETED 1u
#define KAD_MON_BIT_UPDATE_ANNOTATION 2u
#define KAD_MON_BIT_STATUS_STORED 4u
#define KAD_MON_BIT_REPLACE_LAST 8u
#define KAD_MON_BIT_MISSING_OBSERVED_GENERATION 16u
#define KAD_MON_BIT_LOG_LAST_CLUSTER 32u
int kad_monitor_reserve(kad_ctx* ctx, int64_t capacity);
int kad_monitor_load(kad_ctx* ctx, int32_t n, const int32_t* slots, const int64_t* creation, const int64_t* last_update,
                     const int64_t* sync_success, const int64_t* last_status_synced, const int64_t* out_of_sync_ns,
                     const int32_t* type_id, const uint8_t* flags);
int kad_monitor_read(kad_ctx* ctx, int32_t n, const int32_t* slots, int64_t* creation, int64_t* last_update,
                     int64_t* sync_success, int64_t* last_status_synced, int64_t* out_of_sync_ns, int32_t* type_id,
                     uint8_t* flags);
int kad_monitor_clear(kad_ctx* ctx);
int kad_monitor_info(kad_ctx* ctx, int64_t out[4]);
typedef struct kad_monitor_batch {
  int32_t n_objects;
  int32_t n_clusters;
  int64_t now_ns;
  const int32_t* slot;            /* [n_objects] distinct */
  const uint16_t* obj_flags;      /* [n_objects] KAD_MON_OBJ_* */
  const int32_t* type_id;         /* [n_objects] >= 0 */
  const int64_t* creation_ns;     /* [n_objects] read with _NEW */
  const int64_t* sync_success_ns; /* [n_objects] read with _SS_PARSED */
  const int32_t* fed_off;         /* [n_objects + 1] */
  const int32_t* fed_cluster;
  const int64_t* fed_gen;
  const int32_t* mem_off;         /* [n_objects + 1] */
  const int32_t* mem_cluster;
  const int64_t* mem_gen;
  const int32_t* last_off;        /* [n_objects + 1] */
  const int32_t* last_cluster;
  const int64_t* last_gen;
} kad_monitor_batch;
typedef struct kad_monitor_view {
  uint8_t* result; /* [n_objects] KAD_MON_RESULT_* */
  uint8_t* bits;   /* [n_objects] KAD_MON_BIT_* */
  int64_t* meter;  /* [n_objects][5] */
  int64_t* would;  /* [n_objects][2] */
} kad_monitor_view;
int kad_monitor_reconcile(kad_ctx* ctx, const kad_monitor_batch* batch, const kad_monitor_view* out);
/* Host only (no device, no ctx): the same validation, except what needs the table (a slot's capacity and LIVE flag). */
int kad_monitor_reconcile_check(const kad_monitor_batch* batch, const kad_monitor_view* out);
/* ms[0] = the inputs' copies to the device, ms[1] = monitor_reconcile_kernel, ms[2] = the outputs' copies back. */
int kad_monitor_reconcile_timing(kad_ctx* ctx, float ms[3]);
/* The launch decision (csrc/kad_monitor.h route_monitor_reconcile; no device work, no ctx): n_long objects with a
 * list of more than long_min entries, short_items = the other objects' longest lists summed.
 * out[KAD_MON_REC_ROUTE_FIELDS] is [0] the lane-group width, [1] long_min, [2] block threads, [3] group-path blocks,
 * [4] long-path blocks, [5] the objects between two of one group. */
#define KAD_MON_REC_ROUTE_FIELDS 6
int kad_monitor_reconcile_route_eval(int32_t n_objects, int32_t n_long, int64_t short_items, int32_t n_cu, int32_t* out);
int kad_monitor_reconcile_last_route(kad_ctx* ctx, int32_t* out);
/* Measurement and tests only: the lane-group width (0, or a power of two in [1, 64]) and long_min (0: the route's own)
 * of the following kad_monitor_reconcile calls. */
int kad_monitor_reconcile_debug_route(kad_ctx* ctx, int32_t force_width, int32_t force_long_min);
typedef struct kad_monitor_report_batch {
  int64_t now_ns;
  int32_t n_types;
  int32_t timer_cap; /* entries either timer list holds */
} kad_monitor_report_batch;
typedef struct kad_monitor_report_view {
  int32_t* counters;    /* [14] */
  int32_t* type_sync;   /* [n_types] */
  int32_t* type_status; /* [n_types] */
  int32_t* sync_slot;   /* [timer_cap] */
  int64_t* sync_ms;     /* [timer_cap] */
  int32_t* status_slot; /* [timer_cap] */
  int64_t* status_ms;   /* [timer_cap] */
  int32_t* n_timers;    /* [2] */
} kad_monitor_report_view;
int kad_monitor_report(kad_ctx* ctx, const kad_monitor_report_batch* batch, const kad_monitor_report_view* out);
/* Host only: the validation that needs no table. */
int kad_monitor_report_check(const kad_monitor_report_batch* batch, const kad_monitor_report_view* out);
/* ms[0] = the zeroing, ms[1] = monitor_scan_kernel (the counters, the histograms, the timers' counts), ms[2] = the
 * counts' exclusive sums and monitor_scatter_kernel (the timer lists). */
int kad_monitor_report_timing(kad_ctx* ctx, float ms[3]);
/* The launch decision (csrc/kad_monitor.h route_monitor_report): out[KAD_MON_REP_ROUTE_FIELDS] is [0] the histogram
 * path: 0 = LDS-private (a block counts into 2 * n_types bins of its own), 1 = global atomics, [1] the bins limit: the
 * largest n_types of the LDS-private path, [2] block threads, [3] blocks, [4] slots a lane reads per step, [5] wave
 * tiles (the entries of the timer lists' counts). */
#define KAD_MON_REP_ROUTE_FIELDS 6
int kad_monitor_report_route_eval(int64_t n_slots, int32_t n_types, int32_t n_cu, int32_t* out);
int kad_monitor_report_last_route(kad_ctx* ctx, int32_t* out);
/* Measurement and tests only: the histogram path (0 = the route's own, 1 = LDS-private, 2 = global; LDS-private forced
 * above the bins limit: KAD_EINVAL from that call) and the blocks (0 = the route's own) of the following reports. */
int kad_monitor_report_debug_route(kad_ctx* ctx, int32_t force_path, int32_t force_grid);

/* ------------------------------------------------------ revision history: current, numbered and truncated revisions
 * The sync controller's syncRevisions (pkg/controllers/sync/history.go:36-120, with pkg/controllers/util/history/
 * controller_history.go:91-176) for a batch of federated objects of a type with revisionHistoryEnabled, between
 * ensureFinalizer and ensureAnnotations (sync/controller.go:401-409). The API calls are never made: the product is, per
 * object, the ordered plan of actions on its listed ControllerRevisions and what the three return values are built from.
 *
 * Inputs. One blob holds every object's patch (getPatch, history.go:252-278: the caller's json.Marshal) and every
 * listed revision's Data.Raw, each at a multiple of 16 bytes and followed by the bytes up to the next multiple of 16
 * (any value: they are not compared or hashed, only read). Per object: limit = spec.revisionHistoryLimit (0: the
 * object gets no actions, hash 0 and nothing of it is read, history.go:47-50; the caller also passes 0 for an object
 * whose patch failed); collision = the collision count, hashed only with KAD_REV_OBJ_COLLISION (a non-nil pointer);
 * patch_off / patch_len; rev_off[O + 1]: its listed revisions in list order (ListControllerRevisions' filter is the
 * caller's), at most KAD_REV_MAX_REVISIONS each (more: KAD_EUNSUPPORTED); want_off[O + 1] / want_lab: the wanted labels
 * (uid plus the object's labels, history.go:291-304) as ids of (key, value) pairs interned per batch, strictly
 * ascending. Per revision: rev_data_off / rev_data_len; rev_revision; rev_time = creationTimestamp in seconds;
 * rev_name_rank = the rank of its name among its object's revisions' names in byte order, equal names equal ranks;
 * rev_flags: KAD_REV_HASH_PARSED = strconv.ParseInt(its controller.kubernetes.io/hash label, 10, 32) succeeds, rev_hash
 * = uint32 of that number; rev_lab_off[R + 1] / rev_lab: its labels as pair ids, strictly ascending.
 *
 * Per object with limit != 0: (1) hash = FNV-1 32 (fnv.New32) over the patch, then with KAD_REV_OBJ_COLLISION over the
 * ASCII of strconv.FormatInt(collision, 10) (controller_history.go:93-105). (2) The update revision's own hash label
 * is rand.SafeEncodeString(fmt.Sprint(hash)): upd_parsed = ParseInt accepts it (the decimal holds no digit above 5 and,
 * every digit raised by 4, is at most 2^31 - 1), upd_hash its uint32. (3) equal[r] = EqualRevision(listed, update)
 * (:120-143): the lengths equal, not both labels parsed with different numbers, the bytes equal. (4) The equal ones
 * are current, the others old; rev_number = max(0, max old Revision) + 1 in wrapping int64 (history.go:71). (5) No
 * current one: KAD_REV_ACT_CREATE (revision index -1). Else keep = the first current one with the largest Revision
 * (:221-228); KAD_REV_ACT_DELETE for every other current one whose name differs from the kept one's, in list order;
 * then KAD_REV_ACT_RENUMBER(keep) if its Revision < rev_number, else KAD_REV_ACT_RELABEL(keep) unless its labels hold
 * every wanted pair (:83-93, 122-162). (6) order = the old ones in sort.Stable(byRevision) order (Revision, rev_time,
 * name, then list index); the first min(n_old, max(0, n_old - limit)) of them (Go's wrapping int) get DELETE
 * (:164-183). (7) last = the last of order if n_old >= 1 and limit >= 1, else -1 (:103-105). (8) Every old one in
 * sorted order, the deleted ones included, gets RELABEL unless its labels hold every wanted pair (:114-118).
 * IsLabelSubset reads a missing key as "": an object whose wanted set holds an empty value is marked
 * KAD_REV_OBJ_LABELS_ON_HOST, the device emits no RELABEL for it and the caller decides them from keep, order and
 * rev_number. Actions go to act_kind / act_rev (a revision's index within its object) from out_off[o], n_actions[o] of
 * them; out_off[O + 1] is computed by the call (2 n + 1 slots for an object of n revisions) and returned in the view;
 * action_capacity = what act_kind / act_rev hold (less than out_off[O]: KAD_ENOSPC). Slots behind an object's counts,
 * and order / equal of an object with limit 0, are unspecified.
 *
 * Everything is validated on the host before anything is launched (KAD_EINVAL): counts, offsets, data outside the
 * blob or not 16-byte aligned, unknown flag bits, name ranks outside the object, pair lists not strictly ascending or
 * outside [0, n_pairs), missing arrays. Three kernels on the ctx stream (hr_hash_kernel, hr_compare_kernel,
 * hr_plan_kernel: kad_history.hip); the call blocks until the outputs are in the caller's buffers. Integers only, no
 * atomics. It needs no snapshot and reads no resident state, so a kad_group member accepts it. n_objects == 0 returns
 * 0 without launching. */
#define KAD_REV_MAX_REVISIONS 4096
#define KAD_REV_OBJ_COLLISION 1u
#define KAD_REV_OBJ_LABELS_ON_HOST 2u
#define KAD_REV_HASH_PARSED 1u
#define KAD_REV_ACT_CREATE 1u
#define KAD_REV_ACT_DELETE 2u
#define KAD_REV_ACT_RENUMBER 3u
#define KAD_REV_ACT_RELABEL 4u
typedef struct kad_revision_batch {
  int32_t n_objects; /* O */
  int32_t n_pairs;   /* interned (key, value) label pairs */
  int64_t blob_len;
  int64_t action_capacity;
  const int64_t* limit;         /* [O] */
  const int32_t* collision;     /* [O] */
  const uint8_t* obj_flags;     /* [O] KAD_REV_OBJ_* */
  const int64_t* patch_off;     /* [O] multiples of 16 */
  const int32_t* patch_len;     /* [O] */
  const uint8_t* blob;          /* [blob_len] */
  const int32_t* rev_off;       /* [O + 1] */
  const int64_t* rev_data_off;  /* [R] multiples of 16 */
  const int32_t* rev_data_len;  /* [R] */
  const int64_t* rev_revision;  /* [R] */
  const int64_t* rev_time;      /* [R] */
  const int32_t* rev_name_rank; /* [R] */
  const uint8_t* rev_flags;     /* [R] KAD_REV_HASH_PARSED */
  const uint32_t* rev_hash;     /* [R] */
  const int32_t* rev_lab_off;   /* [R + 1] */
  const int32_t* rev_lab;
  const int32_t* want_off;      /* [O + 1] */
  const int32_t* want_lab;
} kad_revision_batch;
typedef struct kad_revision_view {
  int64_t* out_off;     /* [O + 1] written by the call */
  uint32_t* hash;       /* [O] */
  uint32_t* upd_hash;   /* [O] */
  uint8_t* upd_parsed;  /* [O] */
  uint8_t* equal;       /* [R] */
  int32_t* order;       /* [R] object o's sorted old revisions at rev_off[o] .. + n_old[o] */
  int32_t* n_old;       /* [O] */
  int32_t* keep;        /* [O] -1: no current revision */
  int32_t* n_actions;   /* [O] */
  int32_t* last;        /* [O] */
  int64_t* rev_number;  /* [O] */
  uint8_t* act_kind;    /* [action_capacity] KAD_REV_ACT_* */
  int32_t* act_rev;     /* [action_capacity] */
} kad_revision_view;
int kad_revision_plan(kad_ctx* ctx, const kad_revision_batch* batch, const kad_revision_view* out);
/* Host only (no device, no ctx): the same validation. */
int kad_revision_plan_check(const kad_revision_batch* batch, const kad_revision_view* out);
/* ms[0] = hr_hash_kernel, ms[1] = hr_compare_kernel, ms[2] = hr_plan_kernel (the copies either side are not in them). */
int kad_revision_plan_timing(kad_ctx* ctx, float ms[3]);
/* csrc/kad_history.h route_revision: n_hash = the objects with limit != 0, n_long = the objects with more revisions
 * than the route's long_min, short_revs = the other objects' revisions, n_pairs = all revisions, pair_chunks = their data
 * lengths in 16-byte chunks (rounded up each). out[KAD_REV_ROUTE_FIELDS] is [0] the plan kernel's lanes per object
 * (the mean revisions of a short object, a power of two in [1, 64]), [1] long_min, [2] the compare kernel's lanes per
 * pair (the mean chunks of a pair over the chunks a lane takes), [3] hash-kernel blocks (a lane per object, in
 * descending order of patch length), [4] compare-kernel blocks, [5] plan-kernel blocks of the group path, [6] of the long
 * path (one object per block), [7] block threads. */
#define KAD_REV_ROUTE_FIELDS 8
int kad_revision_plan_route_eval(int32_t n_objects, int32_t n_hash, int32_t n_long, int64_t short_revs, int64_t n_pairs,
                                 int64_t pair_chunks, int32_t n_cu, int32_t* out);
int kad_revision_plan_last_route(kad_ctx* ctx, int32_t* out);
/* Measurement and tests only: the lane-group width of the compare and the plan kernel (0, or a power of two in
 * [1, 64]) and long_min (0: the route's own) of the following kad_revision_plan calls. */
int kad_revision_plan_debug_route(kad_ctx* ctx, int32_t force_width, int32_t force_long_min);

/* ------------------------------------------------ sync deletion
 * The other arm of the sync controller's reconcile (pkg/controllers/sync/controller.go:340-378, 723-979): a federated
 * object with a deletion timestamp (ensureDeletion → deleteFromClusters or removeManagedLabel), or an event for a
 * target that has no federated object (reconcile's possibleOrphan arm → removeManagedLabel). Both walk the joined
 * clusters in handleDeletionInClusters. kad_deletion_plan is that walk before anything is sent; kad_deletion_finish is
 * what follows the dispatcher's Wait() and, where the delete arm found nothing remaining, ensureRemovedOrUnmanaged's
 * live checks. The operations, the GETs, DeleteVersions, deleteHistory and the finalizer updates stay with the caller.
 *
 * The clusters and the observations are kad_dispatch_plan's: n_clusters (at most KAD_DISPATCH_MAX_CLUSTERS, more is
 * KAD_EUNSUPPORTED), cluster_flags[C] (KAD_DISPATCH_CL_*; only _READY is read, an unknown bit is KAD_EINVAL),
 * obj_ob_off[O + 1] / ob_cluster / ob_flags (strictly ascending ids per object, exactly one of KAD_DISPATCH_OB_EXISTS
 * and _RETRIEVAL_FAILED, _DELETING and _ADOPTED with _EXISTS only).
 * Per object: obj_flags[O]: KAD_DEL_OBJ_HAS_FINALIZER = the object carries the sync controller's finalizer (:734-739;
 * without it nothing is walked), _ORPHAN_ALL / _ORPHAN_ADOPTED = GetOrphaningBehavior (never both), _POSSIBLE_ORPHAN =
 * no federated object exists (:350-363; exclusive with the other three).
 *
 * kad_deletion_plan. Per observation, aligned with it: out_op = KAD_DISPATCH_OP_NONE, _DELETE or _REMOVE_LABEL. An
 * unready cluster is skipped; a failed retrieval is counted and gets no op; in the label-removal arms (orphan all,
 * possible orphan) an existing object gets _REMOVE_LABEL unless it is _DELETING (:802-807); in the delete arm every
 * existing object is a remaining cluster and gets _REMOVE_LABEL where _ORPHAN_ADOPTED meets _ADOPTED, else _DELETE, a
 * _DELETING one included (dispatch/unmanaged.go:93-140 still strips the retain finalizer). Per object: n_ops,
 * n_remaining (deleteFromClusters' remainingClusters; 0 in the label-removal arms), n_retrieval_failed, obj_pre
 * (KAD_DEL_PRE_RETRIEVAL_FAILED; _NOT_READY on every object that walks when any joined cluster is not ready), obj_first
 * (KAD_DEL_ACT_DELETE_HISTORY | _REMOVE_FINALIZER: the orphan-all arm does both before its label removals, :741-766;
 * _NOTHING: no finalizer, nothing walked, every count 0 and every out_op of the object _NONE).
 *
 * kad_deletion_finish takes the same batch and recomputes the plan's decision. results: op_ok[obj_ob_off[O]] (0 or 1;
 * read only where the plan gives an op), obj_wait[O] (KAD_DEL_WAIT_TIMED_OUT = the operations' Wait() timed out, read
 * only where the plan gives the object an op, because Wait() over no operation cannot; _CHECK_TIMED_OUT likewise for
 * the checks, read only where a listed cluster is ready), chk_off[O + 1] / chk_cluster (ascending per object) /
 * chk_flags (exactly one of KAD_DEL_CHK_*) = the answers of ensureRemovedOrUnmanaged's GETs other than NotFound,
 * chk_cluster_flags[C] = the joined clusters as listed the second time. A ready cluster without an entry answered
 * NotFound; an entry on an unready cluster is ignored; an object outside the delete arm, one that failed before the
 * checks or one with remaining clusters ignores its rows. Outputs per object: obj_status (KAD_DEL_ST_*), obj_reason
 * (KAD_DEL_RSN_*, the first that holds in the enum's order, which is the reference's: :965-978, :861-866, :867-871,
 * :908-918), obj_then (KAD_DEL_ACT_DELETE_HISTORY | _REMOVE_FINALIZER where the delete arm verified clean, :877-881 and
 * :780; _RECORD_ERROR where ensureDeletion records EnsureDeletionFailed, :771-776), n_failed_ops, n_failed_checks (0
 * where the checks were not reached).
 *
 * Everything is validated on the host before any launch (KAD_EINVAL, nothing launched); O == 0 returns 0, launches
 * nothing and leaves the last route. Neither call touches the resident batch, the last schedule's results or another
 * stage's timings; a kad_group member accepts both. */
#define KAD_DEL_OBJ_HAS_FINALIZER 1u
#define KAD_DEL_OBJ_ORPHAN_ALL 2u
#define KAD_DEL_OBJ_ORPHAN_ADOPTED 4u
#define KAD_DEL_OBJ_POSSIBLE_ORPHAN 8u
#define KAD_DEL_PRE_RETRIEVAL_FAILED 1u
#define KAD_DEL_PRE_NOT_READY 2u
#define KAD_DEL_ACT_DELETE_HISTORY 1u
#define KAD_DEL_ACT_REMOVE_FINALIZER 2u
#define KAD_DEL_ACT_NOTHING 4u
#define KAD_DEL_ACT_RECORD_ERROR 8u
#define KAD_DEL_WAIT_TIMED_OUT 1u
#define KAD_DEL_WAIT_CHECK_TIMED_OUT 2u
#define KAD_DEL_CHK_GET_FAILED 1u
#define KAD_DEL_CHK_DELETING 2u
#define KAD_DEL_CHK_LABELLED 4u
#define KAD_DEL_CHK_UNLABELLED 8u
#define KAD_DEL_ST_OK 0
#define KAD_DEL_ST_ERROR 1
#define KAD_DEL_ST_RECHECK 2
#define KAD_DEL_RSN_NONE 0
#define KAD_DEL_RSN_TIMED_OUT 1
#define KAD_DEL_RSN_RETRIEVAL_FAILED 2
#define KAD_DEL_RSN_NOT_READY 3
#define KAD_DEL_RSN_OPS_FAILED 4
#define KAD_DEL_RSN_WAITING 5
#define KAD_DEL_RSN_CHECK_TIMED_OUT 6
#define KAD_DEL_RSN_CHECK_NOT_READY 7
#define KAD_DEL_RSN_CHECKS_FAILED 8
typedef struct kad_deletion_batch {
  int32_t n_clusters, n_objects;
  const uint8_t* cluster_flags; /* [C] KAD_DISPATCH_CL_* */
  const uint8_t* obj_flags;     /* [O] KAD_DEL_OBJ_* */
  const int32_t* obj_ob_off;    /* [O + 1] */
  const int32_t* ob_cluster;    /* [obj_ob_off[O]] */
  const uint8_t* ob_flags;      /* [obj_ob_off[O]] KAD_DISPATCH_OB_* */
} kad_deletion_batch;
typedef struct kad_deletion_view {
  uint8_t* out_op;             /* [obj_ob_off[O]] KAD_DISPATCH_OP_* */
  int32_t* n_ops;              /* [O] */
  int32_t* n_remaining;        /* [O] */
  int32_t* n_retrieval_failed; /* [O] */
  uint8_t* obj_pre;            /* [O] KAD_DEL_PRE_* */
  uint8_t* obj_first;          /* [O] KAD_DEL_ACT_* */
} kad_deletion_view;
typedef struct kad_deletion_results {
  const uint8_t* op_ok;             /* [obj_ob_off[O]] */
  const uint8_t* obj_wait;          /* [O] KAD_DEL_WAIT_* */
  const int32_t* chk_off;           /* [O + 1] */
  const int32_t* chk_cluster;       /* [chk_off[O]] */
  const uint8_t* chk_flags;         /* [chk_off[O]] KAD_DEL_CHK_* */
  const uint8_t* chk_cluster_flags; /* [C] KAD_DISPATCH_CL_* */
} kad_deletion_results;
typedef struct kad_deletion_finish_view {
  uint8_t* obj_status;      /* [O] KAD_DEL_ST_* */
  uint8_t* obj_reason;      /* [O] KAD_DEL_RSN_* */
  uint8_t* obj_then;        /* [O] KAD_DEL_ACT_* */
  int32_t* n_failed_ops;    /* [O] */
  int32_t* n_failed_checks; /* [O] */
} kad_deletion_finish_view;
int kad_deletion_plan(kad_ctx* ctx, const kad_deletion_batch* batch, const kad_deletion_view* out);
int kad_deletion_finish(kad_ctx* ctx, const kad_deletion_batch* batch, const kad_deletion_results* results,
                        const kad_deletion_finish_view* out);
/* Host only (no device, no ctx): the same validations; KAD_EUNSUPPORTED above KAD_DISPATCH_MAX_CLUSTERS. */
int kad_deletion_check(const kad_deletion_batch* batch, const kad_deletion_view* out);
int kad_deletion_finish_check(const kad_deletion_batch* batch, const kad_deletion_finish_view* out,
                              const kad_deletion_results* results);
/* Host only: one (object, observed cluster) pair as both kernels decide it (csrc/kad_deletion.h del_decide): out[0] the
 * op, out[1] = 1 where the cluster counts as remaining, out[2] = 1 where it counts as a retrieval failure. */
int kad_deletion_decide(uint32_t obj_flags, int32_t cluster_ready, uint32_t ob_flags, uint8_t out[3]);
/* ms[0] = inputs to the device, ms[1] = deletion_count_kernel + deletion_kernel, ms[2] = outputs back. */
int kad_deletion_timing(kad_ctx* ctx, float ms[3]);
int kad_deletion_finish_timing(kad_ctx* ctx, float ms[3]);
/* csrc/kad_deletion.h route_deletion: n_long = the objects with more entries (observations; for finish observations
 * plus check rows) than the route's long_min, short_items = the other objects' entries. out[KAD_DEL_ROUTE_FIELDS] is
 * [0] the lanes per object (the mean entries of a short object over the entries a lane takes, a power of two in
 * [1, 64]), [1] long_min, [2] block threads, [3] blocks of the group path, [4] of the long path (four objects a block),
 * [5] objects between two consecutive objects of one lane group, [6] dynamic LDS bytes a block (the clusters' flags). */
#define KAD_DEL_ROUTE_FIELDS 7
int kad_deletion_route_eval(int32_t n_clusters, int32_t n_objects, int32_t n_long, int64_t short_items, int32_t n_cu,
                            int32_t* out);
int kad_deletion_finish_route_eval(int32_t n_clusters, int32_t n_objects, int32_t n_long, int64_t short_items,
                                   int32_t n_cu, int32_t* out);
int kad_deletion_last_route(kad_ctx* ctx, int32_t* out);
int kad_deletion_finish_last_route(kad_ctx* ctx, int32_t* out);
/* Measurement and tests only: the lane-group width (0, or a power of two in [1, 64]) and long_min (0: the route's own)
 * of the following calls. */
int kad_deletion_debug_route(kad_ctx* ctx, int32_t force_width, int32_t force_long_min);
int kad_deletion_finish_debug_route(kad_ctx* ctx, int32_t force_width, int32_t force_long_min);

/* ------------------------------------------------ result application (§8 f3)
 * applySchedulingResult (pkg/controllers/scheduler/scheduler.go:632-695) writes a unit's result into its
 * federated object: the scheduler controller's placement (util.SetPlacementClusterNames,
 * util/placement.go:48-59 → SetPlacementNames, types/v1alpha1/extensions_placements.go:78-103) and its
 * replicas overrides (UpdateReplicasOverride → OverrideUpdateNeeded, scheduler/util.go:71-94, 154-185).
 * kad_result_diff decides on the device, where the results of the last kad_schedule are, which of the two
 * would change for every unit, so the caller edits and re-serialises only those objects. The caller
 * describes each object's CURRENT state with snapshot cluster positions (-1: a name not in the snapshot):
 *   place_off[W+1] / place_cluster: the clusters of the FIRST placement whose controller is the scheduler
 *     (any order, duplicates allowed); place_has[W] = 1 if that placement exists (DeletePlacement's
 *     hasChange when the result is empty);
 *   ovr_off[W+1] / ovr_cluster / ovr_value / ovr_kind: the scheduler controller's override patches whose
 *     path is the replicas path (util.GetOverrides, one entry per patch); ovr_kind 0: the value decoded as
 *     a JSON number (float64) and ovr_value = int64(value) (Go's truncating conversion); 1: any other type.
 * out_flags[W]: KAD_DIFF_PLACEMENT and / or KAD_DIFF_OVERRIDES as the reference reports them
 * (placementUpdated, overridesUpdated); KAD_DIFF_SKIP for units whose Schedule returned an error (nothing is
 * applied, scheduler.go:505-517); KAD_DIFF_STICKY for sticky units (the result is su.CurrentClusters, which
 * the caller holds and applies itself). The annotation half of applySchedulingResult (follower scheduling,
 * unschedulable threshold) does not depend on the result and stays with the caller. Blocks until done.  */
typedef struct kad_result_state {
  int32_t n_units;              /* = the resident batch's n_units */
  const int32_t* place_off;     /* [n_units + 1] */
  const int32_t* place_cluster; /* [place_off[n_units]] */
  const uint8_t* place_has;     /* [n_units] */
  const int32_t* ovr_off;       /* [n_units + 1] */
  const int32_t* ovr_cluster;   /* [ovr_off[n_units]] */
  const int64_t* ovr_value;     /* [ovr_off[n_units]] */
  const uint8_t* ovr_kind;      /* [ovr_off[n_units]] */
} kad_result_state;
#define KAD_DIFF_PLACEMENT 1u
#define KAD_DIFF_OVERRIDES 2u
#define KAD_DIFF_SKIP 4u
#define KAD_DIFF_STICKY 8u
int kad_result_diff(kad_ctx* ctx, const kad_result_state* state, uint32_t* out_flags);

/* ------------------------------------------- scheduling-trigger hashes
 * Replaces the FNV-1 half of Scheduler.computeSchedulingTriggerHash
 * (pkg/controllers/scheduler/schedulingtriggers.go:106-147, called per object
 * from prepareToSchedule, scheduler.go:394). The caller splits each object's
 * json.Marshal(schedulingTriggers) bytes at the "clusterLabels" value: the
 * object part (prefix: scheduling annotations, replica count, resource
 * request, auto-migration info, policy name + generation, up to and including
 * `"clusterLabels":`) and the cluster part (suffix: clusterLabels value,
 * clusterTaints, clusterAPIResourceTypes, closing brace), which is identical
 * for every object scheduled against the same joined-cluster list. Output:
 * hash.Sum32() per object (the reference formats it with strconv.FormatInt).
 *   suffix: uploaded once per cluster-set change (bytes, any alignment)
 *   prefixes: CSR, prefix_off[0] = 0, non-decreasing, n+1 entries
 *   run: asynchronous on the ctx stream (summarises the suffix into a
 *        256-entry FNV table, then hashes every object); download blocks.  */
int kad_trigger_suffix_upload(kad_ctx* ctx, const uint8_t* suffix, size_t nbytes);
int kad_trigger_prefixes_upload(kad_ctx* ctx, int n, const int64_t* prefix_off, const uint8_t* prefix);
int kad_trigger_run(kad_ctx* ctx);
/* ms[0] = whole trigger run, ms[1] = the cluster-part summary kernels */
int kad_trigger_timing(kad_ctx* ctx, float ms[2]);
int kad_trigger_download(kad_ctx* ctx, uint32_t* out_hash);
/* All in one (blocking): both uploads, run, download. */
int kad_trigger_hashes(kad_ctx* ctx, int n, const int64_t* prefix_off, const uint8_t* prefix, const uint8_t* suffix,
                       size_t suffix_len, uint32_t* out_hash);

/* Profiling builds only (-DKAD_PHASE_PROF): copy 32 per-phase cycle / event
 * counters of the kernels to out (and zero them if reset). Returns 32, or
 * 0 in product builds (no counters compiled in). Not part of the reference. */
int kad_debug_phase_counters(uint64_t* out, int reset);

/* Tests only: fault injection. where = 1: the next rebuild of the snapshot's
 * derived state (kad_snapshot_upload / _upload_device / _update) fails with
 * KAD_ENOMEM, as an allocation failure would. A failed snapshot upload or
 * update leaves no snapshot and no batch resident (kad_schedule then returns
 * KAD_ESTATE). where = 0 clears a pending fault. Not part of the reference. */
int kad_debug_inject_fault(kad_ctx* ctx, int where);

/* Tests only: on = 1 sends every row of kad_plan_rows through the LDS-workspace planner (the path of rows
 * with more than 64 clusters), so the golden planner cases cover both planners; on = 2 runs rows two per
 * wave where both hold at most 32 clusters (plan_pair_kernel's half-wave planner); 0 restores the default
 * choice by row length. Not part of the reference. */
int kad_debug_plan_force_workspace(kad_ctx* ctx, int on);

#ifdef __cplusplus
}
#endif
#endif /* KAD_SCHED_H */
