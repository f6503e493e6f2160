// Launch unit of conv_x3_r512.h, tile widths 32, 16 and 8 (launch_conv_x3_r512.h).
#include "launch_conv_x3_r512.h"

hipError_t unet::launch_conv_r512_w32(const ConvX3Args& a, int grid, int tw, int waves, bool flat, bool f32, hipStream_t s) {
  const bool w1 = waves == 1;
  switch (tw) {
    case 32: return w1 ? ::launch_conv_r512<32, 1>(a, grid, flat, f32, s) : ::launch_conv_r512<32, 2>(a, grid, flat, f32, s);
    case 16: return ::launch_conv_r512<16, 1>(a, grid, flat, f32, s);
    default: return ::launch_conv_r512<8, 1>(a, grid, flat, f32, s);
  }
}
