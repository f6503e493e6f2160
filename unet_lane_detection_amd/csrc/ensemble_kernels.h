// Between the head and the mask that leaves the device: the weighted mean of several models' probability planes
// (unet_ensemble_combine) and confusion counts of a score plane at many thresholds in one pass
// (unet_score_sweep_accumulate).  The kernels are in ensemble_kernels.cpp, a translation unit of their own like
// validate_kernels.cpp and calib_kernels.cpp: the code object of unet_hip.cpp does not change when kernels are added here.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace unet {

constexpr int ENSEMBLE_MAX = 8;   // UNET_ENSEMBLE_MAX of include/unet_hip.h
constexpr int SWEEP_MAX = 64;     // UNET_SWEEP_MAX

// by value in the kernel's arguments: the caller's arrays are free once the launch returns
struct EnsembleMembers {
  const float* p[ENSEMBLE_MAX];
  float w[ENSEMBLE_MAX];
};
struct SweepThresholds {
  float t[SWEEP_MAX];
};

// acc = w[0] * p0, then acc = acc + w[k] * pk for k = 1 .. K-1, every product and sum rounded to fp32 on its own;
// probsOut[i] = acc, maskOut[i] = acc > threshold ? 255 : 0 (either may be null, not both).
hipError_t launch_ensemble_combine(const EnsembleMembers& m, int k, size_t numel, float threshold, float* probsOut,
                                   uint8_t* maskOut, hipStream_t s);

constexpr unsigned SWEEP_MAX_GRID = 1024;          // blocks of one sweep launch (see sweep_grid)
constexpr unsigned SWEEP_ITEMS_PER_BLOCK = 4096;   // elements a block takes before another block is worth its flush
constexpr int SWEEP_MAX_NUMEL_LOG2 = 41;

// Blocks for `numel` elements, as histogram_grid of calib_kernels.h: a block is added per 4096 elements, 1024 at the
// most.  A block of 256 threads then takes ceil(numel / 4 / (256 grid)) rounds of 1024 elements and one of the tail (or,
// on the unaligned path, ceil(numel / (256 grid)) rounds of 256): at most 2^31 + 2^8 for every numel below 2^41, which
// its 32-bit LDS counters hold.  sweep_numel_supported is that bound; launch_score_sweep refuses more.
inline unsigned sweep_grid(size_t numel) {
  const size_t b = (numel + SWEEP_ITEMS_PER_BLOCK - 1) / SWEEP_ITEMS_PER_BLOCK;
  return (unsigned)(b < 1 ? 1 : (b > SWEEP_MAX_GRID ? SWEEP_MAX_GRID : b));
}
inline bool sweep_numel_supported(size_t numel) { return numel != 0 && (numel >> SWEEP_MAX_NUMEL_LOG2) == 0; }

// counts[cls * (T + 1) + bin] += 1 per element, bin = #{ j : score > t[j] }, cls = target is positive.  waveCombine:
// equal bins of a wave are added to LDS once (the default); false: every lane adds its own.  hipErrorInvalidValue for a
// numel the grid rule cannot cover or T outside 1 .. SWEEP_MAX, before anything is launched.
hipError_t launch_score_sweep(const float* scores, const void* targets, bool targetsU8, size_t numel,
                              const SweepThresholds& thr, int nThresholds, bool waveCombine, unsigned long long* counts,
                              hipStream_t s);

}  // namespace unet
