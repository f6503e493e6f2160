// Lane view on the device: the bird's-eye results - the area between fitted curves, the mask's markings, the curves -
// drawn in the camera frame and blended onto it.  One kernel that, per camera pixel, goes forward through the
// perspective matrix, asks the curves and the mask what lies there, and blends.  The arithmetic is stated in
// include/unet_hip.h and tests/laneview_model.py; the kernel in laneview_kernels.cpp reproduces it bit for bit.  A
// translation unit of its own, like lanefit_kernels.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

#include "../../include/unet_hip.h"

namespace unet {

constexpr int LANE_VIEW_WORDS = 8;   // UNET_LANE_VIEW_WORDS
constexpr int LANE_VIEW_MAX = 8;     // UNET_LANE_VIEW_MAX
constexpr int LANE_VIEW_SIZE_MAX = 4096, LANE_VIEW_WARP_W_MAX = 8192, LANE_VIEW_WARP_H_MAX = 2048;
constexpr int LANE_VIEW_THICKNESS_MAX = 64;

// The caller has checked the domain of unet_lane_view_u8_batch.
hipError_t launch_lane_view(const uint8_t* frames, int n, int height, int width, int step, const double* m, int warpW,
                            int warpH, const uint8_t* masks, int level, const long long* curves, int k,
                            const unet_lane_view_style& style, uint8_t* view, uint8_t* layers, hipStream_t s);

}  // namespace unet
