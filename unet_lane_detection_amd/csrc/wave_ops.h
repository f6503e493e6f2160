// Exact integer sums and exchanges over the 64 lanes of a wave.  Integers only: the order of additions does not show in
// the result, so these may be shared freely; the float and block-wide reductions stay with their kernels.
#pragma once

#include <hip/hip_runtime.h>

#include <cstdint>

namespace unet {

// every lane receives the sum over the wave
__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += __shfl_xor(v, d, 64);
  return v;
}
__device__ __forceinline__ uint32_t wave_sum32(uint32_t v) {
#pragma unroll
  for (int d = 32; d >= 1; d >>= 1) v += (uint32_t)__shfl_xor((int)v, d, 64);
  return v;
}

// lane ^ d's 64-bit value, as two 32-bit exchanges
__device__ __forceinline__ unsigned long long shfl_xor64(unsigned long long v, int d) {
  const uint32_t lo = __shfl_xor((uint32_t)v, d, 64), hi = __shfl_xor((uint32_t)(v >> 32), d, 64);
  return ((unsigned long long)hi << 32) | lo;
}

}  // namespace unet
