// int8 calibration beyond min/max: the activation histogram behind the 'mmse' / 'kl_divergence' range selection
// (unet_forward_u8_histograms, unet_op_histogram_f32) and the float-vs-int8 probability error of compare_outputs
// (unet_prob_mae_accumulate).  The kernels are in calib_kernels.cpp, a translation unit of their own like
// validate_kernels.cpp: the code object of unet_hip.cpp does not change when kernels are added here.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>

namespace unet {

constexpr int HIST_MIN_BINS = 64, HIST_MAX_BINS = 4096;   // powers of two in between
constexpr unsigned HIST_MAX_GRID = 1024;                  // blocks of one histogram launch (see histogram_grid)
constexpr unsigned HIST_ITEMS_PER_BLOCK = 4096;           // elements a block takes before another block is worth its flush

inline bool histogram_bins_supported(int bins) {
  return bins >= HIST_MIN_BINS && bins <= HIST_MAX_BINS && (bins & (bins - 1)) == 0;
}
// fp32 bins / (hi - lo): the one factor of the binning rule, computed here and nowhere else (quant.histogram_model
// forms it the same way).  Not finite or not positive: the span cannot be binned.
inline float histogram_inv(float lo, float hi, int bins) { return (float)bins / (hi - lo); }

// Blocks for `total` elements: every block pays up to `bins` global atomics when it flushes, so a block is only added
// per 4096 elements, 1024 at the most.  A block then sees ceil(total / grid) + 1024 elements at the most, which keeps
// its 32-bit LDS counters exact for every total below 2^41; launch_histogram_f32 refuses more.
inline unsigned histogram_grid(size_t total) {
  const size_t b = (total + HIST_ITEMS_PER_BLOCK - 1) / HIST_ITEMS_PER_BLOCK;
  return (unsigned)(b < 1 ? 1 : (b > HIST_MAX_GRID ? HIST_MAX_GRID : b));
}

// hist[0 .. bins) += counts of x (npix pixels of c channels at pixel stride ld) binned over [lo, hi); hist[bins] +=
// the number of exact zeros.  hipErrorInvalidValue for an unsupported bin count, a span that cannot be binned or
// c > ld, before anything is launched.
hipError_t launch_histogram_f32(const float* x, size_t npix, int c, int ld, float lo, float hi, int bins,
                                unsigned long long* hist, hipStream_t s);

constexpr unsigned MAE_BLOCKS_PER_FRAME = 64;
// acc[f] += sum over frame f of |pa - pb| (each term fp32, the sum in double, fixed order).  partial:
// frames * MAE_BLOCKS_PER_FRAME doubles of device scratch.
hipError_t launch_prob_mae(const float* pa, const float* pb, int frames, size_t perFrame, double* partial, double* acc,
                           hipStream_t s);

}  // namespace unet
