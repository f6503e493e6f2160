// Launch unit of conv_q8_r512.h: the instances of the f16q8 tier's convolution the library carries (launch.h).
#include "launch.h"

#include "conv_q8_r512.h"

namespace {

template <int TWX, int EPI, bool FLAT>
hipError_t launch_conv_q8(const unet::ConvQ8Args& a, int grid, hipStream_t s) {
  using S = unet::X3RShape<TWX>;
  auto kern = unet::conv3x3_q8_r512_kernel<TWX, EPI, FLAT>;
  hipError_t e = unet::ensure_dyn_lds((const void*)kern, S::LDS_BYTES);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), (size_t)S::LDS_BYTES, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t unet::launch_conv_q8(const ConvQ8Args& a, int grid, int tw, int epi, bool flat, hipStream_t s) {
  if (tw == 14) return epi == 4 ? ::launch_conv_q8<14, 4, true>(a, grid, s) : ::launch_conv_q8<14, 0, true>(a, grid, s);
  if (epi == 4) return flat ? ::launch_conv_q8<28, 4, true>(a, grid, s) : ::launch_conv_q8<28, 4, false>(a, grid, s);
  return flat ? ::launch_conv_q8<28, 0, true>(a, grid, s) : ::launch_conv_q8<28, 0, false>(a, grid, s);
}
