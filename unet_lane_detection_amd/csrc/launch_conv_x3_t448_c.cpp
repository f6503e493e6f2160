// Launch unit of conv_x3_t448.h, 16 x 28 tiles with two or four waves along the channels (launch_conv_x3_t448.h).
#include "launch_conv_x3_t448.h"

hipError_t unet::launch_conv_t448_c(const ConvX3Args& a, int grid, int waves, int epi, bool flat, hipStream_t s) {
  return waves == 4 ? ::launch_conv_t448<28, 4>(a, grid, epi, flat, s) : ::launch_conv_t448<28, 2>(a, grid, epi, false, s);
}
