// Phase-profiling globals and macros of the schedule kernels (empty outside -DKAD_PHASE_PROF builds).
// Part of kad_kernels.hip's translation unit, which includes the kernels' headers in definition order.
#pragma once

#include "kad_wave.h"

namespace kad {

// Phase profiling (only in builds with -DKAD_PHASE_PROF; scripts/phase_prof.py):
// per-phase s_memtime cycles summed over units, plus event counters.
// Accumulated per wave in registers, flushed once at wave exit into one of
// 256 stripes (a shared counter per phase would serialise the waves).
#ifdef KAD_PHASE_PROF
constexpr int KAD_PSLOTS = 40;  // per-block phase slots (scripts/phase_prof.py NAMES)
__device__ unsigned long long g_phase[256 * KAD_PSLOTS];
// lean kernel: (start, end) s_memtime of every wave of the last launch, for the wave-lifetime split
__device__ unsigned long long g_wavetime[8192 * 2];
// wide kernel: per wave (units taken, the longest unit's s_memtime cycles, realtime of the last dequeue, units
// that straddled a tie, HW_ID, XCC_ID)
__device__ unsigned long long g_wavex[8192 * 6];
// wide kernel, per unit of the last launch (units < 2^20): realtime start; (duration in realtime ticks,
// feasible count n << 32, straddle << 47, global wave << 48) — scripts/unit_trace.py
constexpr int KAD_UTRACE_MAX = 1 << 20;
__device__ unsigned long long g_ustart[KAD_UTRACE_MAX];
__device__ unsigned long long g_uinfo[KAD_UTRACE_MAX];
#define KAD_PT(v) const unsigned long long v = __builtin_readcyclecounter()
#define KAD_PACC uint32_t pacc[12] = {0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0, 0}
#define KAD_PADD(i, x) pacc[i] += (uint32_t)(x)
#define KAD_PFLUSH                                                                       \
  if (lane_id() == 0)                                                                    \
    for (int i_ = 0; i_ < 10; ++i_) atomicAdd(&g_phase[(blockIdx.x & 255) * KAD_PSLOTS + i_], pacc[i_])
// lean / wide kernel: slots 10..15 (A, B, D, E, straddles, D on straddles), 24..29 (replay: setup,
// partitions, pivots, insertion sorts, #partitions, feasible count of replayed units)
#define KAD_PFLUSH_LEAN                                                                  \
  if (lane_id() == 0) {                                                                  \
    for (int i_ = 0; i_ < 6; ++i_) atomicAdd(&g_phase[(blockIdx.x & 255) * KAD_PSLOTS + 10 + i_], pacc[i_]); \
    for (int i_ = 6; i_ < 12; ++i_) atomicAdd(&g_phase[(blockIdx.x & 255) * KAD_PSLOTS + 18 + i_], pacc[i_]); \
  }
// plan kernel: slots 16..23 (setup, dynamic weights, first plan, avoid-disruption, output, units)
#define KAD_PFLUSH_PLAN                                                                  \
  if (lane_id() == 0)                                                                    \
    for (int i_ = 0; i_ < 6; ++i_) atomicAdd(&g_phase[(blockIdx.x & 255) * KAD_PSLOTS + 16 + i_], pacc[i_])
// row kernel (thread 0, block-synchronous phases): slots 9 (units), 20 (compaction), 22 (scores),
// 23 (normalise), 30 (select: radix + counts), 31 (pdqsort replay); within the scores 32 (preferred-term
// words) and 33 (thread 0's position loop)
#define KAD_PFLUSH_ROW                                                                   \
  if (threadIdx.x == 0) {                                                                \
    const int sl_[8] = {9, 20, 22, 23, 30, 31, 32, 33};                                  \
    for (int i_ = 0; i_ < 8; ++i_) atomicAdd(&g_phase[(blockIdx.x & 255) * KAD_PSLOTS + sl_[i_]], pacc[i_]); \
  }
#else
#define KAD_PFLUSH_ROW
#define KAD_PFLUSH_LEAN
#define KAD_PFLUSH_PLAN
#define KAD_PT(v)
#define KAD_PACC
#define KAD_PADD(i, x)
#define KAD_PFLUSH
#endif

}  // namespace kad
