// Lane following on the device (reference README.md:206-227, `extract_white_lanes`, and :4087-4126, `LineFollower`):
// the HSV colour-threshold lane extractor the network is measured against, and the scan-row lane centre the mask is
// reduced to.  The arithmetic is stated in include/unet_hip.h and tests/follow_model.py; the kernels in
// follow_kernels.cpp reproduce it bit for bit.  A translation unit of its own, like video_kernels.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace unet {

constexpr int LANE_ROWS_MAX = 64;   // UNET_LANE_ROWS_MAX

// the scan rows of a launch, by value in the kernel's arguments
struct LaneRows {
  int r[LANE_ROWS_MAX];
};

// frames (n,height,width,3) u8 -> mask (n,height,width) u8 of 0 / 255: 8-bit HSV, inRange(lower, upper), CLOSE with a
// closeK x closeK box, OPEN with an openK x openK box; closeK, openK in {1,3,5,7}; n * height * width < 2^31
hipError_t launch_hsv_lanes(const uint8_t* frames, int n, int height, int width, int isBgr, const uint8_t lower[3],
                            const uint8_t upper[3], int closeK, int openK, uint8_t* maskOut, hipStream_t s);

// masks (n,height,width) u8 -> out (n,nRows,2) u32: count and sum of the x with mask[i,rows[j],x] > level
hipError_t launch_lane_center(const uint8_t* masks, int n, int height, int width, const LaneRows& rows, int nRows,
                              int level, uint32_t* out, hipStream_t s);

}  // namespace unet
