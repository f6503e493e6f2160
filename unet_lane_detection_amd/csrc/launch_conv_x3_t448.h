// The funnel of conv_x3_t448.h's launch units.  Two units share the structure's instances by the waves along the
// channels: launch_conv_x3_t448.cpp (one wave: 64 channels per block, and the entry launch.h declares) and
// launch_conv_x3_t448_c.cpp (two and four waves).
#pragma once
#include "launch.h"

#include "conv_x3_t448.h"

namespace unet {
hipError_t launch_conv_t448_c(const ConvX3Args& a, int grid, int waves, int epi, bool flat, hipStream_t s);
}

namespace {

// Third structure (conv_x3_t448.h): 16 x 28 / 16 x 32 pixel tiles for the layers with 64 / 128 output channels
template <int TWX, int WCO, int EPI, bool FLAT = false>
hipError_t launch_conv_t448(const unet::ConvX3Args& a, int grid, hipStream_t s) {
  using S = unet::X3TShape<TWX, unet::x3t_row_blocks(WCO)>;
  constexpr int ldsBytes = FLAT ? S::LDS_BYTES_FLAT : S::LDS_BYTES_PLAIN;
  auto kern = unet::conv3x3_x3_t448_kernel<TWX, WCO, EPI, FLAT>;
  hipError_t e = unet::ensure_dyn_lds((const void*)kern, ldsBytes);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), (size_t)ldsBytes, s, a);
  return hipGetLastError();
}
template <int TWX, int WCO>
hipError_t launch_conv_t448(const unet::ConvX3Args& a, int grid, int epi, bool flat, hipStream_t s) {
  if constexpr (WCO == 1) {
    if (epi == 2) return launch_conv_t448<TWX, 1, 2>(a, grid, s);
  }
  if constexpr (WCO == 4) {
    if (flat)
      return epi == 0 ? launch_conv_t448<TWX, 4, 0, true>(a, grid, s)
           : epi == 1 ? launch_conv_t448<TWX, 4, 1, true>(a, grid, s)
                      : launch_conv_t448<TWX, 4, 3, true>(a, grid, s);
  }
  return epi == 0 ? launch_conv_t448<TWX, WCO, 0>(a, grid, s)
       : epi == 1 ? launch_conv_t448<TWX, WCO, 1>(a, grid, s)
                  : launch_conv_t448<TWX, WCO, 3>(a, grid, s);
}

}  // namespace
