// The bilinear sample of cv::warpPerspective (INTER_LINEAR, constant border 0, 8-bit) at a fixed-point position:
// shared by the camera stage (camera_stage.h, three channels of the camera frame) and the lane view
// (laneview_kernels.cpp, one channel of the bird's-eye mask).  oracle/camera_oracle.py states the integers.
#pragma once
#include <hip/hip_runtime.h>
#include <stddef.h>
#include <stdint.h>

namespace unet {

// (X, Y): the position in 1/32 pixel.  img: `height` rows of `step` bytes, CN interleaved channels, `width` pixels a row.
template <int CN>
__device__ __forceinline__ void warp_sample(const uint8_t* __restrict__ img, int height, int width, size_t step,
                                            long long X, long long Y, int (&v)[CN]) {
  const long long sx = X >> 5, sy = Y >> 5;
  const int fa = (int)(X & 31), fb = (int)(Y & 31);
  const int wgt[4] = {(32 - fb) * (32 - fa) * 32, (32 - fb) * fa * 32, fb * (32 - fa) * 32, fb * fa * 32};
  int acc[CN];
#pragma unroll
  for (int c = 0; c < CN; ++c) acc[c] = 0;
#pragma unroll
  for (int t = 0; t < 4; ++t) {
    const long long yy = sy + (t >> 1), xx = sx + (t & 1);
    if (yy >= 0 && yy < height && xx >= 0 && xx < width) {
      const uint8_t* p = img + (size_t)yy * step + (size_t)xx * CN;
#pragma unroll
      for (int c = 0; c < CN; ++c) acc[c] += wgt[t] * (int)p[c];
    }
  }
#pragma unroll
  for (int c = 0; c < CN; ++c) v[c] = (acc[c] + (1 << 14)) >> 15;
}

}  // namespace unet
