// Frame and output diagnostics on the device (reference README.md:4476-4496, `diagnose_input_image`, and :4615-4640,
// `quick_test`): pixel range, brightness and Laplacian sharpness of a frame, and range, mean, share above the threshold
// and NaN count of a probability plane, as a few integer words per frame.  The arithmetic is stated in
// include/unet_hip.h and tests/diagnose_model.py; the kernels in diagnose_kernels.cpp reproduce it bit for bit.  A
// translation unit of its own, like follow_kernels.cpp.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace unet {

constexpr int FRAME_STATS_WORDS = 8;   // unsigned 64-bit words of a frame's record
constexpr int PROB_STATS_WORDS = 4;    // ... of a probability plane's

// frames: n frames of height rows of rowStride bytes (>= 3 * width), the first 3 * width of a row are pixels ->
// out (n, 8) u64: min, max and sum of the pixel bytes, sum and sum of squares of the 4-neighbour Laplacian of the
// 8-bit gray plane (reflect-101), three zeros.  n * height * width < 2^31.  Every call overwrites the records.
hipError_t launch_frame_stats(const uint8_t* frames, int n, int height, int width, long long rowStride, int isBgr,
                              unsigned long long* out, hipStream_t s);

// scores (n, numel) fp32 -> out (n, 4) u64: fp32 bits of the minimum (low half) and maximum (high half) over the
// non-NaN values, #{s > threshold}, sum of floor(clamp(s, 0, 1) * 2^32), number of NaNs.  numel < 2^31.
hipError_t launch_prob_stats(const float* scores, int n, unsigned numel, float threshold, unsigned long long* out,
                             hipStream_t s);

}  // namespace unet
