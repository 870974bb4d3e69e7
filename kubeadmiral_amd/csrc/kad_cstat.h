// kad_cluster_resources (kad_cstat.hip): one call's nodes and pods per member cluster, the launch decision,
// the launches.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kad_groups.h"

namespace kad {

constexpr int CS_MAX_RES = 64;         // resource names of a call: one presence bit each
constexpr int CS_LONG_MIN = 4096;      // clusters with more entries (node + pod) than this take the long path (a
                                       // starting value, see DESIGN §7 for the measured comparison)
constexpr int CS_POD_CHUNK = 4096;     // pods per block of the long path's pod pass
constexpr int CS_MIN_WIDTH = 8;        // lane-group widths: powers of two in [8, 64]
constexpr int CS_SLAB = CS_MAX_RES + 2;  // u64 per team in LDS: the sums, then the presence bits, then the node count
constexpr uint8_t CS_NODE_SCHEDULABLE = 1;  // KAD_CS_NODE_SCHEDULABLE
constexpr uint8_t CS_POD_TERMINAL = 1;      // KAD_CS_POD_TERMINAL

struct CstatDev {
  int K, R;
  int n_long, n_chunks;
  const int64_t* cl_node_off;   // [K + 1]
  const uint8_t* node_flags;    // [N]
  const int64_t* node_ent_off;  // [N + 1]
  const uint8_t* nent_res;      // [EN]
  const int64_t* nent_val;      // [EN]
  const int64_t* cl_pod_off;    // [K + 1]
  const uint8_t* pod_flags;     // [P]
  const int64_t* pod_ent_off;   // [P + 1]
  const uint8_t* pent_res;      // [EP]
  const uint8_t* pent_kind;     // [EP]
  const int64_t* pent_val;      // [EP]
  // built on the host while it validates
  const uint8_t* cl_long;         // [K] 1: the cluster is on the long path
  const int32_t* long_list;       // [n_long] the clusters of the long path, ascending
  const int32_t* long_chunk_off;  // [n_long + 1] the chunks of each long cluster
  const int32_t* chunk_cluster;   // [n_chunks]
  const int64_t* chunk_pod_lo;    // [n_chunks] pods [lo, hi) of the chunk
  const int64_t* chunk_pod_hi;    // [n_chunks]
  uint64_t* partial;              // [n_chunks * R] requests summed per chunk (pod pass → combine)
  int64_t* alloc;                 // [K * R]
  int64_t* avail;                 // [K * R]
  uint64_t* has;                  // [K]
  int64_t* sched_nodes;           // [K]
};

// The launch decision of one kad_cluster_resources, taken here and nowhere else (kad_cstat_route_eval /
// kad_cstat_last_route show it). Group path: a wave is 64 / width lane groups, every group takes one cluster at a
// time and its lanes stride over the cluster's nodes (node pass) or pods (pod pass), each lane walking its
// item's entries; the groups of a grid stride over the clusters. The width starts at the mean items per
// short cluster / 8, rounded up to a power of two in [8, 64]: several clusters in flight per wave (what the
// auto-migration sweep measured), not one. Clusters with more than long_min entries (the caller counts them:
// n_long, and the short clusters' nodes and pods) are left out there: one 256-thread block each in the node
// pass, one block per CS_POD_CHUNK pods in the pod pass (n_chunks, partial sums, a combine kernel).
struct CstatRoute {
  int32_t node_width;   // lanes per cluster on the node pass's group path
  int32_t pod_width;    // lanes per cluster on the pod pass's group path
  int32_t long_min;     // a cluster with more entries than this is on the long path
  int32_t threads;      // per block, every kernel
  int32_t node_grid;    // blocks of the node pass's group path (0 when every cluster is long)
  int32_t pod_grid;     // blocks of the pod pass's group path
  int32_t long_grid;    // blocks of the node pass's long path = n_long
  int32_t chunk_grid;   // blocks of the pod pass's long path = n_chunks
};

inline CstatRoute route_cstat(int K, int n_long, int64_t short_nodes, int64_t short_pods, int n_chunks, int n_cu) {
  CstatRoute r{};
  const int n_short = K - n_long;
  r.node_width = group_width(short_nodes, n_short, CS_MIN_WIDTH, 8);
  r.pod_width = group_width(short_pods, n_short, CS_MIN_WIDTH, 8);
  r.long_min = CS_LONG_MIN;
  r.threads = 256;
  // the groups stride over all K clusters and skip the long ones; at most 16.5 KiB of LDS a block
  r.node_grid = n_short > 0 ? group_grid(K, r.node_width, n_cu) : 0;
  r.pod_grid = n_short > 0 ? group_grid(K, r.pod_width, n_cu) : 0;
  r.long_grid = n_long;
  r.chunk_grid = n_chunks;
  return r;
}

}  // namespace kad
