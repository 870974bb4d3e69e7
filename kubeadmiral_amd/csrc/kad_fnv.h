// FNV-1 32 (hash/fnv New32: multiply, then xor) as the kernels fold it: the constants and the four-bytes-a-step fold
// that kad_trigger.hip and kad_history.hip share.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace kad {

constexpr uint32_t kFnvPrime = 16777619u;
constexpr uint32_t kFnvOffset = 2166136261u;

__device__ __forceinline__ uint32_t fnv_word(uint32_t h, uint32_t w) {
  h = (h * kFnvPrime) ^ (w & 0xffu);
  h = (h * kFnvPrime) ^ ((w >> 8) & 0xffu);
  h = (h * kFnvPrime) ^ ((w >> 16) & 0xffu);
  return (h * kFnvPrime) ^ (w >> 24);
}

}  // namespace kad
