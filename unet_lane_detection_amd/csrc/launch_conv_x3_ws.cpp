// Launch unit of conv_x3_ws.h: the instances of the first f16x3 structure the library carries (launch.h).
#include "launch.h"

#include "conv_x3_ws.h"

namespace {

template <int TW, int EPI, bool FLAT = false>
hipError_t launch_conv_x3(const unet::ConvX3Args& a, int grid, hipStream_t s) {
  using S = unet::X3Shape<TW>;
  auto kern = unet::conv3x3_x3_ws_kernel<TW, EPI, FLAT>;
  hipError_t e = unet::ensure_dyn_lds((const void*)kern, S::LDS_BYTES);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(512), (size_t)S::LDS_BYTES, s, a);
  return hipGetLastError();
}
template <int TW>
hipError_t launch_conv_x3(const unet::ConvX3Args& a, int grid, int epi, bool flat, hipStream_t s) {
  if (flat)
    return epi == 0   ? launch_conv_x3<TW, 0, true>(a, grid, s)
           : epi == 1 ? launch_conv_x3<TW, 1, true>(a, grid, s)
                      : launch_conv_x3<TW, 3, true>(a, grid, s);
  return epi == 0   ? launch_conv_x3<TW, 0>(a, grid, s)
         : epi == 1 ? launch_conv_x3<TW, 1>(a, grid, s)
         : epi == 2 ? launch_conv_x3<TW, 2>(a, grid, s)
                    : launch_conv_x3<TW, 3>(a, grid, s);
}

}  // namespace

hipError_t unet::launch_conv_x3(const ConvX3Args& a, int grid, int tw, int epi, bool flat, hipStream_t s) {
  return tw == 32 ? ::launch_conv_x3<32>(a, grid, epi, flat, s) : ::launch_conv_x3<16>(a, grid, epi, flat, s);
}
