// The funnel of conv_x3_r512.h's launch units.  The structure's 32 instances are the library's longest compile, so two units
// share them by tile width: launch_conv_x3_r512.cpp (28 / 14, and the entry launch.h declares) and
// launch_conv_x3_r512_w32.cpp (32 / 16 / 8).
#pragma once
#include "launch.h"

#include "conv_x3_r512.h"

namespace unet {
hipError_t launch_conv_r512_w32(const ConvX3Args& a, int grid, int tw, int waves, bool flat, bool f32out, hipStream_t s);
}

namespace {

// Second structure (conv_x3_r512.h): 224-pixel tiles of 8 x 28 or 16 x 14, one wave per SIMD
template <int TWX, int WPX, int EPI, bool FLAT>
hipError_t launch_conv_r512(const unet::ConvX3Args& a, int grid, hipStream_t s) {
  using S = unet::X3RShape<TWX>;
  auto kern = unet::conv3x3_x3_r512_kernel<TWX, WPX, EPI, FLAT>;
  hipError_t e = unet::ensure_dyn_lds((const void*)kern, S::LDS_BYTES);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), (size_t)S::LDS_BYTES, s, a);
  return hipGetLastError();
}
template <int TWX, int WPX>
hipError_t launch_conv_r512(const unet::ConvX3Args& a, int grid, bool flat, bool f32out, hipStream_t s) {
  if (f32out) return flat ? launch_conv_r512<TWX, WPX, 3, true>(a, grid, s) : launch_conv_r512<TWX, WPX, 3, false>(a, grid, s);
  return flat ? launch_conv_r512<TWX, WPX, 0, true>(a, grid, s) : launch_conv_r512<TWX, WPX, 0, false>(a, grid, s);
}

}  // namespace
