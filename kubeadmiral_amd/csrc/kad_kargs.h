// How the schedule kernels read their arguments, and the per-unit exits the full, lean and wide kernels share.
#pragma once

#include "kad_wave.h"

namespace kad {

// A schedule kernel takes one by-value argument block (SchedArgs, LeanArgs, WideArgs, RowArgs: each begins
// SnapDev s, BatchDev b, OutDev o, ProfDev p) and reads it through the kernarg segment pointer, laundered
// per phase: argument loads then sit next to their uses instead of being hoisted to the entry, where ~60 live
// pointers overflow the SGPR file and spill to VGPR lanes.
// (Inline, in the kernel body alone: a callee does not receive the kernarg segment pointer, isa_check.py.)
template <class Args>
__device__ __forceinline__ const __attribute__((address_space(4))) Args* kernarg() {
  return (const __attribute__((address_space(4))) Args*)opq((uintptr_t)__builtin_amdgcn_kernarg_segment_ptr());
}

// The unit ends without clusters: status, zero count and flags, on lane 0. With the kernel's pointer where the
// caller holds one (the full kernel), else laundered inside lane 0's branch.
template <class A>
__device__ __forceinline__ void status_words(A a, int w, int32_t st) {
  a->o.status[w] = st;
  a->o.count[w] = 0;
  a->o.flags[w] = 0;
}
template <class A>
__device__ __forceinline__ void unit_status(A a, int w, int32_t st) {
  if (lane_id() == 0) status_words(a, w, st);
}
template <class Args>
__device__ __forceinline__ void unit_status(int w, int32_t st) {
  if (lane_id() == 0) status_words(kernarg<Args>(), w, st);
}

// The unit goes on to schedule_kernel's defer list.
template <class Args>
__device__ __forceinline__ void unit_defer(int w) {
  if (lane_id() == 0) {
    auto a = kernarg<Args>();
    const int slot = atomicAdd(a->b.defer_n, 1);
    a->b.defer[slot] = w;
  }
}

// feasible lists longer than the kernel's register positions: the row kernel's list when it runs
// (BatchDev::use_rows: every filter is in the static words), else the full kernel's defer list.
// LATE: not when prep routed the long units early (BatchDev::early_rows: the row kernel may already be done)
template <class Args, bool LATE = false>
__device__ __forceinline__ void unit_row_or_defer(int w) {
  if (lane_id() == 0) {
    auto a = kernarg<Args>();
    if (a->b.use_rows && !(LATE && a->b.early_rows)) {
      const int slot = atomicAdd(a->b.rows_n, 1);
      a->b.rows[slot] = w;
    } else {
      const int slot = atomicAdd(a->b.defer_n, 1);
      a->b.defer[slot] = w;
    }
  }
}

}  // namespace kad
