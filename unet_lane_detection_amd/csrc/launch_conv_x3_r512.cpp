// Launch unit of conv_x3_r512.h: the instances of the second f16x3 structure the library carries (launch.h), tile widths
// 28 and 14; the others are launch_conv_x3_r512_w32.cpp's.
#include "launch_conv_x3_r512.h"

hipError_t unet::launch_conv_r512(const ConvX3Args& a, int grid, int tw, int waves, bool flat, bool f32, hipStream_t s) {
  const bool w1 = waves == 1;
  switch (tw) {
    case 28: return w1 ? ::launch_conv_r512<28, 1>(a, grid, flat, f32, s) : ::launch_conv_r512<28, 2>(a, grid, flat, f32, s);
    case 14: return w1 ? ::launch_conv_r512<14, 1>(a, grid, flat, f32, s) : ::launch_conv_r512<14, 2>(a, grid, flat, f32, s);
    default: return launch_conv_r512_w32(a, grid, tw, waves, flat, f32, s);
  }
}
