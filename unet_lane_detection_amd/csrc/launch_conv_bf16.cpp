// Launch unit of the bf16 tier's GEMM-shaped kernels: igemm_bf16.h, conv_bf16_r512.h and conv_bf16_ws.h (launch.h).
#include "launch.h"

#include <algorithm>

#include "igemm_bf16.h"
#include "conv_bf16_r512.h"
#include "conv_bf16_ws.h"

namespace {

template <int TAPS, int MODE>
hipError_t launch_bf(const unet::ConvArgsBf& a, dim3 grid, int ms, int ns, hipStream_t s) {
  constexpr int NLD7 = 6, NLD4 = 4;
#define LB(MS_, NS_, NLD_)                                                                                       \
  hipLaunchKernelGGL((unet::igemm_bf16_kernel<TAPS, MS_, NS_, NLD_, MODE>), grid, dim3(256),                     \
                     std::max<size_t>((size_t)2 * NLD_ * 256 * 16 + 64, (size_t)MS_ * 16 * (32 * NS_ + 4) * 4), s, a)
  if (ms == 7 && ns == 4)
    LB(7, 4, NLD7);
  else if (ms == 7)
    LB(7, 2, NLD7);
  else if (ns == 4)
    LB(4, 4, NLD4);
  else
    LB(4, 2, NLD4);
#undef LB
  return hipGetLastError();
}

template <int TWX, int WPX>
hipError_t launch_bf_r512(const unet::ConvBfRArgs& a, int grid, bool flat, hipStream_t s) {
  using S = unet::BfRShape<TWX>;
  void (*kern)(unet::ConvBfRArgs) = flat ? unet::conv3x3_bf16_r512_kernel<TWX, WPX, true>
                                         : unet::conv3x3_bf16_r512_kernel<TWX, WPX, false>;
  hipError_t e = unet::ensure_dyn_lds((const void*)kern, S::LDS_BYTES);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(256), (size_t)S::LDS_BYTES, s, a);
  return hipGetLastError();
}

}  // namespace

hipError_t unet::launch_bf(const ConvArgsBf& a, dim3 grid, int taps, int ms, int ns, hipStream_t s) {
  return taps == 9 ? ::launch_bf<9, 0>(a, grid, ms, ns, s) : ::launch_bf<1, 1>(a, grid, ms, ns, s);
}

hipError_t unet::launch_bf_r512(const ConvBfRArgs& a, int grid, int tw, int wpx, bool flat, hipStream_t s) {
  if (tw == 28) return wpx == 1 ? ::launch_bf_r512<28, 1>(a, grid, flat, s) : ::launch_bf_r512<28, 2>(a, grid, flat, s);
  return wpx == 1 ? ::launch_bf_r512<14, 1>(a, grid, flat, s) : ::launch_bf_r512<14, 2>(a, grid, flat, s);
}

hipError_t unet::launch_bf_ws(const ConvWsArgs& a, int grid, int epi, hipStream_t s) {
  using S = WsShape;
  void (*kern)(ConvWsArgs) = epi == 2   ? conv3x3_bf16_ws_kernel<2>
                             : epi == 1 ? conv3x3_bf16_ws_kernel<1>
                                        : conv3x3_bf16_ws_kernel<0>;
  const hipError_t e = ensure_dyn_lds((const void*)kern, S::LDS_BYTES);
  if (e != hipSuccess) return e;
  hipLaunchKernelGGL(kern, dim3(grid), dim3(512), (size_t)S::LDS_BYTES, s, a);
  return hipGetLastError();
}
