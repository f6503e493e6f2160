// Lane fit on the device: the bird's-eye mask reduced to the moment sums of its two lane markings - a column histogram
// of the bottom half for the two bases, a sliding-window search upwards (or, with a prior, a band around last frame's
// curves), and S_k = sum y^k, T_k = sum x y^k over the pixels found.  The host solves x = a y^2 + b y + c from those
// sums (lanefit.py).  The arithmetic is stated in include/unet_hip.h and tests/lanefit_model.py; the kernel in
// lanefit_kernels.cpp reproduces it bit for bit.  A translation unit of its own, like follow_kernels.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace unet {

constexpr int LANE_FIT_WORDS = 16;          // UNET_LANE_FIT_WORDS
constexpr int LANE_FIT_WINDOWS_MAX = 64;    // UNET_LANE_FIT_WINDOWS_MAX
constexpr int LANE_FIT_HEIGHT_MAX = 2048, LANE_FIT_WIDTH_MAX = 8192, LANE_FIT_MARGIN_MAX = 512;

// masks (n,height,width) u8 -> out (n,2,16) u64 records; prior (n,2,height) i32 or null (window mode).  The caller has
// checked the domain of unet_lane_fit_u8_batch.
hipError_t launch_lane_fit(const uint8_t* masks, int n, int height, int width, int level, int nWindows, int margin,
                           int minPixels, const int32_t* prior, unsigned long long* out, hipStream_t s);

}  // namespace unet
