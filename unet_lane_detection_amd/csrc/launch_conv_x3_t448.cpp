// Launch unit of conv_x3_t448.h: the instances of the third f16x3 structure the library carries (launch.h), those of 64
// channels per block; the others are launch_conv_x3_t448_c.cpp's.  The structure's second kernel,
// conv3x3_x3_t448add_kernel, belongs to the decoder step: launch_conv_x3_dec.cpp.
#include "launch_conv_x3_t448.h"

hipError_t unet::launch_conv_t448(const ConvX3Args& a, int grid, int tw, int waves, int epi, bool flat, hipStream_t s) {
  if (tw == 32) return ::launch_conv_t448<32, 1>(a, grid, epi, false, s);
  return waves == 4 || waves == 2 ? launch_conv_t448_c(a, grid, waves, epi, flat, s)
                                  : ::launch_conv_t448<28, 1>(a, grid, epi, false, s);
}
