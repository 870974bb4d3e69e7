// Unit work queue of the lean and wide schedule kernels.
// Part of kad_kernels.hip's translation unit, which includes the kernels' headers in definition order.
#pragma once

#include "kad_device.h"
#include "kad_wave.h"

namespace kad {

static_assert(WQ_HEADS == 64, "drained-head set is one u64; heads map to XCDs by h & 7");
// Work queue: WQ_HEADS = 64 heads; head h hands out the batches of the h-th contiguous 64th of the
// units. 64 counters (not 8) spread the returning atomics over as many lines: the device-scope
// atomics of 8 XCDs on a few addresses serialise. A wave of block b starts at head b & 63 (blocks go
// round-robin over the 8 XCDs, so head h is started by XCD h & 7) and, when it is drained, moves to
// the next head of its own XCD (h + 8, h + 16, ...) that still has batches, then to any other. A ticket is one
// returning atomicAdd (lane 0), resolved into a batch one batch later, so its latency hides behind a
// batch of work. Every wave's first batch is static (no atomic): wave wv of block b takes batch
// (b >> 6) * wpb + wv of head b & 63, and that head's atomics count on from its static_batches.
// Every wave ends once all heads are drained.
struct WorkTicket {
  int x;             // head of the pending ticket
  int i;             // its atomicAdd result (lane 0); batch index = i + static_batches(x)
  int wpb, nblocks;  // waves per block, grid size: the static first round
  int B;             // units per batch (<= WQ_BATCH): small enough that a wave takes >= ~12 batches
};
// the static first-round batches of head x: one per wave of every block b < nblocks with b & 63 == x
__device__ __forceinline__ int static_batches(const WorkTicket& t, int x) { return t.wpb * ((t.nblocks - x + 63) >> 6); }
__device__ __forceinline__ WorkTicket wq_start(int wpb, int B = WQ_BATCH) {
  const int wv = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
  WorkTicket t{(int)(blockIdx.x & (WQ_HEADS - 1)), 0, wpb, (int)gridDim.x, B};
  t.i = (int)(blockIdx.x >> 6) * wpb + wv - static_batches(t, t.x);
  return t;
}
__device__ __forceinline__ void wq_issue(uint32_t* heads, WorkTicket& t) {
  if (lane_id() == 0) t.i = (int)atomicAdd(heads + t.x * WQ_STRIDE, 1u);
}
__device__ __forceinline__ int wq_head_batches(int W, int x, int B) {
  const int s0 = (int)((int64_t)W * x / WQ_HEADS), s1 = (int)((int64_t)W * (x + 1) / WQ_HEADS);
  return (s1 - s0 + B - 1) / B;
}
// the batch [first, first + count) of a ticket; count 0 = queue drained. A drained head costs one
// wave-wide look at all 64 counters (lane l loads head l, device-coherent) and one atomic on a head
// that still has batches — not a walk over the heads with one atomic round trip each.
__device__ __forceinline__ int2 wq_resolve(uint32_t* heads, int W, WorkTicket& t) {
  const int lane = lane_id();
  for (;;) {
    const int x = t.x;
    const int bi = __builtin_amdgcn_readfirstlane(t.i) + static_batches(t, x);
    if (bi < wq_head_batches(W, x, t.B)) {
      const int s0 = (int)((int64_t)W * x / WQ_HEADS), s1 = (int)((int64_t)W * (x + 1) / WQ_HEADS);
      const int first = s0 + bi * t.B;
      return make_int2(first, (s1 - first) < t.B ? (s1 - first) : t.B);
    }
    const uint32_t taken = __hip_atomic_load(heads + lane * WQ_STRIDE, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const uint64_t open = ballot((int)taken + static_batches(t, lane) < wq_head_batches(W, lane, t.B));
    if (!open) return make_int2(0, 0);
    // same XCD first (heads x & 7 + 8j), in rotation order after x; then the lowest open head
    const uint64_t same = open & (0x0101010101010101ull << (x & 7));
    int nx;
    if (same) {
      const int sh = (x + 1) & 63;
      const uint64_t rot = sh ? (same >> sh) | (same << (64 - sh)) : same;
      nx = (x + 1 + __builtin_ctzll(rot)) & 63;
    } else {
      nx = __builtin_ctzll(open);
    }
    t.x = nx;
    if (lane == 0) t.i = (int)atomicAdd(heads + nx * WQ_STRIDE, 1u);
  }
}

}  // namespace kad
